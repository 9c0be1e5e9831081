"""Generate tests/golden/traj_convolve.npz FROM THE REFERENCE ITSELF (needs the reference tree at REF): inputs and outputs
of the reference's two trajectory convolutions, data_loaders/utils/mix.py

    convolve_traj_with_win(wav, traj_rirs, hop, 'trapezium20')           (mix.py:197-244)  -> win_<i>    [2, N + L - 1] float32
    convolve_traj(wav, traj_rirs, traj_rirs, hop, align=False)[0]        (mix.py:151-194)  -> switch_<i> [2, N + L - 1] float32

for the seven (N, hop, L) of CASES with two microphones.  mix.py is loaded by file path (its package imports are not needed).  Only the data is
committed.  The inputs are seeded standard-normal draws rounded to sixteenths and stored as int8 counts of 1/16 (x16_<i> [N], h16_<i> [P, 2, L];
P = len(range(0, N + hop - 1, hop)), of which convolve_traj takes the first ceil(N / hop)): at float32 precision the file would hold 140 KB, this way
the outputs, sums of multiples of 1 / 256 outside the ramps, also deflate, and the whole file stays under 100 KB.

    python tests/golden/make_golden_traj.py"""
import importlib.util
from pathlib import Path

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent / "traj_convolve.npz"
CASES = [(1000, 100, 37), (1003, 100, 64), (950, 100, 5), (260, 21, 33), (999, 333, 70), (1000, 1000, 16), (64, 23, 300)]  # (N, hop, L)
M = 2


def sixteenths(rng, *shape):
    return np.clip(np.round(rng.standard_normal(shape) * 16.0), -127, 127).astype(np.int8)


def main():
    assert REF.exists(), "the reference tree is needed to (re)generate the fixture"
    spec = importlib.util.spec_from_file_location("reference_mix", REF / "data_loaders" / "utils" / "mix.py")
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    out = {"cases": np.array(CASES, dtype=np.int64)}
    for i, (N, hop, L) in enumerate(CASES):
        rng = np.random.default_rng(20260 + i)
        P = len(range(0, N + hop - 1, hop))
        x16, h16 = sixteenths(rng, N), sixteenths(rng, P, M, L)
        x, h = x16.astype(np.float64) / 16.0, h16.astype(np.float64) / 16.0
        P0 = -(-N // hop)
        out[f"x16_{i}"], out[f"h16_{i}"] = x16, h16
        out[f"win_{i}"] = mix.convolve_traj_with_win(x, h, hop, wintype="trapezium20").astype(np.float32)
        out[f"switch_{i}"] = mix.convolve_traj(x, h[:P0], h[:P0], hop, align=False)[0].astype(np.float32)
    np.savez_compressed(OUT, **out)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
