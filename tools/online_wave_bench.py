"""What waveform-to-waveform streaming costs over feature-level streaming, on the device (BASELINE config 5's geometry: 129 bins, 8 layers,
6 microphones -> 2 speakers, batch 1, 8 kHz / hop 128: a frame is 16 ms), for 'ret(2)' and 'mhsa(251)' and chunks of 2 / 4 / 8 / 16 / 32 frames.

Per point, in ONE process, the two captured graphs alternating round by round (--rounds rounds of --replays back-to-back replays each, timed
with a pair of HIP events around the whole round; a round's figure is its time / replays; reported: the median over the rounds, and min / max):
  feature   NativeOnlineStreamer: 6 L + 2 network launches per replay (what the parent of this work could already run)
  wave      NativeWaveStreamer: STFT step (2 launches) + the same network launches + iSTFT step (1 launch)
  io        wave - feature: the cost of the two new entry points inside the graph
  rtf       real-time factor of the wave graph: chunk duration / replay time
and, to say which end is the slow one and how it compares with the network's own two ends, graphs that hold --inner back-to-back calls of ONE
entry point (time / inner per call: kernel time plus the gap to the next launch of the same graph, no graph-launch floor):
  stft, istft, encdec (nbss_online_encoder_step + nbss_decoder_fwd).
Every (attention) run is a child process of its own under a time limit; the parent never opens the device and stops at the first child that fails.
usage: python tools/online_wave_bench.py [--chunks 2,4,8,16,32] [--attentions "ret(2),mhsa(251)"] [--rounds 9] [--replays 200] [--json out.json]
('mamba(16,4)' and 'mamba(16,4,not_replace_ffn)' are accepted as attentions: the child sets NBSS_ONLINE_MAMBA=1 and NBSS_ONLINE_NATIVE_MAMBA_STEP=1 itself)"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _rounds(graphs, rounds, replays):
    """alternate the graphs round by round; us per replay of each: (median, min, max) over the rounds"""
    import torch
    for g in graphs:  # warm-up: every graph once through a whole round
        for _ in range(replays):
            g.replay()
    torch.cuda.synchronize()
    us = [[] for _ in graphs]
    for _ in range(rounds):
        for i, g in enumerate(graphs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            b.synchronize()
            us[i].append(a.elapsed_time(b) * 1e3 / replays)
    return [(statistics.median(u), min(u), max(u)) for u in us]


def _graph_of(fn, inner, dev):
    import torch
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    return g


def point(attention, chunks, rounds, replays, inner):
    import ctypes as C

    import torch
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    from models.io.stft import STFT
    from nbss_amd import ops
    from nbss_amd.online import NativeOnlineStreamer
    from nbss_amd.online_io import NativeWaveStreamer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if attention.startswith("mamba"):  # the variant's own switch and that of its native step (both opt-in)
        os.environ["NBSS_ONLINE_MAMBA"] = os.environ["NBSS_ONLINE_NATIVE_MAMBA_STEP"] = "1"
    net = OnlineSpatialNet(dim_input=12, dim_output=4, num_layers=8, dim_squeeze=8, num_freqs=129, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192,
                           num_heads=4, dropout=(0, 0, 0), kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], full_share=0,
                           attention=attention, decay=[4, 5, 9, 10], rope=False).eval().to(dev)
    stft = STFT(n_fft=256, n_hop=128, win_len=256)
    rows = []
    for chunk in chunks:
        fs = NativeOnlineStreamer(net, 1, chunk, device=dev, use_graph=True)
        ws = NativeWaveStreamer(net, 1, chunk, stft, "frequency", list(range(6)), 0, device=dev, use_graph=True)
        x = torch.randn(1, 6, (chunk + 1) * 128, device=dev)
        fs.step(torch.randn(1, 129, chunk, 12, device=dev))  # captures
        ws.push(x[..., :chunk * 128])
        lib, P = ws.lib, ops._ptr
        f = lambda t: P(lib, t, torch.float32)  # noqa: E731
        st = lambda: ops._stream(lib, ws.xw)  # noqa: E731
        g_stft = _graph_of(lambda: lib.call("nbss_online_stft_step", 256, ws.norm, 1, 6, chunk, 0, f(ws.tables), f(ws.xw), f(ws.tail), f(ws.x), f(ws.xrmm), None,
                                            st()), inner, dev)
        g_istft = _graph_of(lambda: lib.call("nbss_online_istft_step", 256, ws.norm, 1, 2, chunk, f(ws.tables), f(ws.y), f(ws.xrmm), f(ws.ola), f(ws.yw), st()),
                            inner, dev)

        def encdec():
            lib.call("nbss_online_encoder_step", 129, chunk, 12, f(ws.enc_w), f(ws.enc_b), f(ws.x), f(ws.state["enc"]), f(ws.h[0]), st())
            lib.call("nbss_decoder_fwd", C.byref(ws.cfg), f(ws.flat), P(lib, ws.packed), f(ws.h[0]), f(ws.y), st())
        g_encdec = _graph_of(encdec, inner, dev)
        feat, wave = _rounds([fs.graph, ws.graph], rounds, replays)
        small = _rounds([g_stft, g_istft, g_encdec], rounds, max(replays // inner, 4))
        row = {"attention": attention, "chunk": chunk, "feature_us": round(feat[0], 1), "feature_min_max": [round(feat[1], 1), round(feat[2], 1)],
               "wave_us": round(wave[0], 1), "wave_min_max": [round(wave[1], 1), round(wave[2], 1)], "io_us": round(wave[0] - feat[0], 1),
               "rtf": round(chunk * 128 / 8000 * 1e6 / wave[0], 1), "stft_us": round(small[0][0] / inner, 2), "istft_us": round(small[1][0] / inner, 2),
               "encdec_us": round(small[2][0] / inner, 2)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def table(rows):
    out = ["| attention | chunk | feature graph us | wave graph us | wave - feature us | real-time factor | stft step us | istft step us | encoder + decoder us |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['attention']} | {r['chunk']} | {r['feature_us']} ({r['feature_min_max'][0]}-{r['feature_min_max'][1]}) | {r['wave_us']} "
                   f"({r['wave_min_max'][0]}-{r['wave_min_max'][1]}) | {r['io_us']} | {r['rtf']} | {r['stft_us']} | {r['istft_us']} | {r['encdec_us']} |")
    for r in rows:
        if r["chunk"] == 16:
            io, slow = r["stft_us"] + r["istft_us"], ("stft" if r["stft_us"] > r["istft_us"] else "istft")
            out.append(f"\n{r['attention']}, chunk 16: the two I/O steps take {io:.1f} us back to back, the network's encoder + decoder {r['encdec_us']:.1f} us: "
                       f"{'MORE' if io > r['encdec_us'] else 'not more'} than those; the slower of the two is the {slow} step.")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", default="2,4,8,16,32")
    ap.add_argument("--attentions", default="ret(2),mhsa(251)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--json", default=None)
    ap.add_argument("--point", default=None, help="(internal) run one attention in this process")
    a = ap.parse_args()
    chunks = [int(c) for c in a.chunks.split(",")]
    if a.point is not None:
        point(a.point, chunks, a.rounds, a.replays, a.inner)
        return 0
    rows = []
    for att in re.split(r",(?![^(]*\))", a.attentions):  # commas outside parentheses: "ret(2),mamba(16,4)" names two
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--point", att, "--chunks", a.chunks, "--rounds", str(a.rounds),
               "--replays", str(a.replays), "--inner", str(a.inner)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-4000:])
        if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started on the device
            print(f"[online_wave_bench] {att}: child ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        rows += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        print(r.stdout, end="", flush=True)
    print(table(rows))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
