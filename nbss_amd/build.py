"""Build the gfx950 shared library (libnbss_hip.so) from nbss_amd/csrc/*.hip with hipcc.

In-tree build so that the .so travels with the repo snapshot to the GPU box.  Also knows how to
build the host *emulator* flavour of the same sources (tests/hipemu, -DNBSS_EMU) which the CPU
test-suite uses to exercise the kernels' index math without a GPU — that library is test
infrastructure and is never loaded by the product code.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "nbss_amd" / "csrc"
LIBDIR = ROOT / "nbss_amd" / "lib"
EMUDIR = ROOT / "tests" / "hipemu"
HIP_LIB = LIBDIR / "libnbss_hip.so"
EMU_LIB = EMUDIR / "libnbss_emu.so"


# The SLP vectoriser turns adjacent f32 adds / multiplies into v_pk_*_f32.  On gfx950 a packed f32 instruction issues no faster than its two
# scalar halves (SIMD-32: 157 TFLOP/s IS the unpacked rate) and constrains register pairing; measured per kernel in one call (profiles/README.md,
# round 5): mhsa_bwd 1417 -> 1406 us without it, fconv_bwd within noise, the T-ConvFFN kernels 4 % SLOWER (fewer issue slots matter there), full_bwd
# 766 -> 716 us (+1 % on the step) — but full.hip stays vectorised: without it one tensor of tests/test_bf16_vs_reference.py (layers.1.squeeze.0.bias,
# a heavily cancelling sum) lands at 1.58x the reference's own bf16 error instead of 1.45x (other FMA contractions, same algorithm), above the 1.5x bar,
# and the bar is not what gets moved.
PER_FILE_FLAGS = {k: ["-fno-slp-vectorize"] for k in ("mhsa", "mhsa_bwd")}
# The machine scheduler's strategy, per file (round 6; `-mllvm -amdgpu-sched-strategy=...` changes the order of the same instructions, not the arithmetic).
# Measured per kernel in one call with the whole library built under each strategy (us per launch at batch 32, default -> strategy):
#   iterative-minreg   full_bwd 526-535 -> 485, mhsa_bwd_h 795 -> 767      (but fconv_bwd 312 -> 464, tconvffn_bwd_q 1 092 -> 1 167, tconvffn_fwd 614 -> 640)
#   iterative-maxocc   full_bwd -> 495, mhsa_bwd_h -> 771                   (fconv_fwd 141 -> 153)
#   max-ilp            tailw<288> 336 -> 317, tailw<192> 277 -> 269, tconvffn_fwd 614 -> 604   (fconv_bwd 308 -> 434, mhsa_bwd_h -> 871, tconvffn_bwd_q +28)
#   max-memory-clause  tailw<288> -> 323; mhsa_bwd_h -> 914
# tconvffn_s.hip holds a kernel that gains (forward) and one that loses (backward) under max-ilp: it keeps the default.
_SCHED = lambda s: ["-mllvm", f"-amdgpu-sched-strategy={s}"]
PER_FILE_FLAGS["full"] = _SCHED("iterative-minreg")
PER_FILE_FLAGS["mhsa_bwd"] = PER_FILE_FLAGS["mhsa_bwd"] + _SCHED("iterative-minreg")
PER_FILE_FLAGS["tailw"] = _SCHED("max-ilp")
# metrics.hip is fp64 arithmetic pinned to 1e-4 dB against an fp64 restatement: no reassociation, exact division and square root
PER_FILE_FLAGS["metrics"] = ["-fno-fast-math"]
# rir.hip splits a delay of up to 65 536 samples into integer and fraction in fp64 and is held to a few fp32 ulp per image: accurate sinf / cosf, no reassociation
PER_FILE_FLAGS["rir"] = ["-fno-fast-math"]
# stoi.hip: a keep-or-drop threshold on fp64 frame energies and fp64 correlation statistics held against an fp64 restatement
PER_FILE_FLAGS["stoi"] = ["-fno-fast-math"]


def _sources():
    return sorted(CSRC.glob("*.hip"))


def _headers():
    return sorted(CSRC.glob("*.h")) + [ROOT / "include" / "nbss_hip.h"]


def _newer(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(map(str, cmd)) + "\n" + r.stdout + r.stderr)
        raise RuntimeError(f"build failed: {cmd[0]} {cmd[-1]}")
    return r


def hipcc_path() -> str:
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(p):
        raise RuntimeError("hipcc not found")
    return p


def build_hip(force: bool = False, verbose: bool = False, phase_prof: bool = False, flavour: str = "", defines=()) -> Path:
    """Compile every .hip for gfx950 and link libnbss_hip.so (no-op when up to date).

    phase_prof=True builds the diagnostic flavour lib/libnbss_hip_phase.so (-DNBSS_PHASE_PROF: in-kernel phase
    timers, csrc/prof.h) that only tools/phase_prof.py loads."""
    LIBDIR.mkdir(parents=True, exist_ok=True)
    if phase_prof:
        flavour, defines = "phase", ["-DNBSS_PHASE_PROF", *defines]
    objdir = LIBDIR / (f"obj_{flavour}" if flavour else "obj")
    objdir.mkdir(exist_ok=True)
    hipcc = hipcc_path()
    hdrs = _headers()
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffast-math", "-fno-finite-math-only",
             "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-Wno-pass-failed"]
    HIP_LIB = LIBDIR / (f"libnbss_hip_{flavour}.so" if flavour else "libnbss_hip.so")
    flags += list(defines)  # side-by-side experiment builds (NBSS_HIP_FLAVOUR=<name> selects one; tools only)
    jobs = []
    objs = []
    for s in _sources():
        o = objdir / (s.stem + ".o")
        objs.append(o)
        if force or _newer(o, [s] + hdrs + [Path(__file__)]):
            jobs.append([hipcc, *flags, *PER_FILE_FLAGS.get(s.stem, []), "-c", str(s), "-o", str(o)])
    if jobs:
        if verbose:
            print(f"[nbss_amd.build] hipcc: compiling {len(jobs)} file(s) for gfx950", flush=True)
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            list(ex.map(_run, jobs))
    if force or jobs or _newer(HIP_LIB, objs):
        # do not record an rpath to /opt/rocm/lib: the process already has torch's HIP runtime loaded
        _run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(HIP_LIB), *map(str, objs)])
    return HIP_LIB


def build_emu(force: bool = False, verbose: bool = False) -> Path:
    """Host build of the same kernel sources on top of tests/hipemu (CPU tests only)."""
    objdir = EMUDIR / "obj"
    objdir.mkdir(parents=True, exist_ok=True)
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        cxx = shutil.which("clang++") or cxx
    hdrs = _headers() + [EMUDIR / "hipemu.h"]
    flags = ["-x", "c++", "-DNBSS_EMU", "-O2", "-std=c++17", "-fPIC", f"-I{EMUDIR}", "-Wno-unused-variable",
             "-Wno-unused-but-set-variable", "-Wno-pass-failed", "-Wno-unknown-attributes"]
    jobs = []
    objs = []
    for s in _sources() + [EMUDIR / "hipemu.cpp"]:
        o = objdir / (s.stem + ".o")
        objs.append(o)
        if force or _newer(o, [s] + hdrs):
            jobs.append([cxx, *flags, "-c", str(s), "-o", str(o)])
    if jobs:
        if verbose:
            print(f"[nbss_amd.build] emulator: compiling {len(jobs)} file(s)", flush=True)
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
            list(ex.map(_run, jobs))
    if force or jobs or _newer(EMU_LIB, objs):
        _run([cxx, "-shared", "-fPIC", "-o", str(EMU_LIB), *map(str, objs), "-lpthread"])
    return EMU_LIB


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "hip"
    if which in ("hip", "all"):
        print(build_hip(verbose=True))
    if which == "phase":
        print(build_hip(verbose=True, phase_prof=True))
    if which == "flavour":  # python -m nbss_amd.build flavour <name> [-DFOO ...]
        print(build_hip(verbose=True, force=True, flavour=sys.argv[2], defines=sys.argv[3:]))
    if which in ("emu", "all"):
        print(build_emu(verbose=True))
