"""The launch sequence of one step of the native streamers (nbss_amd/online.py: NativeOnlineStreamer, nbss_amd/online_io.py: NativeWaveStreamer) against the
recorded one: tests/golden/online_call_trace.json holds every `lib.call` of a step per attention variant — symbol, integers by value, and for every pointer
WHICH tensor it is (shape, dtype, content digest, ordinal of first appearance) — as recorded by tests/golden/make_online_call_trace.py on the commit the
fixture names.  The host side may be re-arranged freely as long as what it launches, in which order and with which arguments stays the same."""
import importlib.util
import json
from pathlib import Path

import pytest

GOLDEN = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_online_call_trace", GOLDEN / "make_online_call_trace.py")
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

WANT = json.loads((GOLDEN / "online_call_trace.json").read_text())["cases"]


def test_the_fixture_holds_every_case():
    assert sorted(WANT) == sorted("/".join(c) for c in rec.CASES)
    for (kind, attention) in rec.CASES:  # 2 layers: encoder, 5 per layer, decoder (+ the frame counter's advance for 'mhsa'); 1 layer between STFT and iSTFT steps
        assert len(WANT[f"{kind}/{attention}"]) == (12 + attention.startswith("mhsa") if kind == "step" else 9), (kind, attention)
    assert not any("unresolved" in json.dumps(v) for v in WANT.values())


@pytest.mark.parametrize("kind,attention", rec.CASES, ids=["-".join(c) for c in rec.CASES])
def test_launch_sequence_is_the_recorded_one(backend, kind, attention):
    got = json.loads(json.dumps(rec.trace(backend.lib, backend.device, kind, attention)))  # (through JSON: tuples / floats as the fixture stores them)
    want = WANT[f"{kind}/{attention}"]
    for i, (g, w) in enumerate(zip(got, want)):
        assert not any(isinstance(a, list) and a[0] == "unresolved" for a in g), f"launch {i}: a pointer of {g} is no tensor of the streamer"
        assert g == w, f"launch {i}: {g} != recorded {w}"
    assert len(got) == len(want), [r[0] for r in got[len(want):] or want[len(got):]]
