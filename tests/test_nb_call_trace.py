"""The launch sequence of the native narrow-band runners (nbss_amd/nbc2.py, nbc.py, blstm.py over the launcher of nbss_amd/nb.py) against the recorded one:
tests/golden/nb_call_trace.json holds every `lib.call` of an inference call and of one training step (forward + backward) per architecture and stream
dtype — symbol, integer / float arguments by value, pointer arguments as given / None — as recorded by tests/golden/make_nb_call_trace.py on the commit
the fixture names.  The host sequencing may be re-arranged freely as long as what it launches, in which order and with which arguments stays the same."""
import importlib.util
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_nb_call_trace", GOLDEN / "make_nb_call_trace.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

WANT = json.loads((GOLDEN / "nb_call_trace.json").read_text())["cases"]


def test_the_fixture_holds_every_case():
    assert sorted(WANT) == sorted("/".join(c) for c in rec.CASES)
    assert all(len(v) >= 5 for v in WANT.values())  # (the shortest: NB-BLSTM inference, 2 x (input map, recurrence) + the linear map)


@pytest.mark.parametrize("arch,dtype,mode", rec.CASES, ids=["-".join(c) for c in rec.CASES])
def test_launch_sequence_is_the_recorded_one(backend, arch, dtype, mode):
    got = json.loads(json.dumps(rec.trace(backend.lib, backend.device, arch, dtype, mode)))  # (through JSON: tuples / floats as the fixture stores them)
    want = WANT["/".join((arch, dtype, mode))]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}: {g} != recorded {w}"
    assert len(got) == len(want), [r[0] for r in got[len(want):] or want[len(got):]]
