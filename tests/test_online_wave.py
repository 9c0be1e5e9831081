"""Waveform-to-waveform streaming of an OnlineSpatialNet (csrc/online_io.hip, nbss_amd/online_io.py): the two I/O kernels against torch.stft /
torch.istft in fp64 on the host, their round trip, their independence of the chunk size (bitwise), NativeWaveStreamer against today's
feature-level streaming (TrainModule.forward_streaming with the torch.nn step), the torch WaveStreamer against the whole-signal forward, the
refusals, and — on the GPU — the one-graph-per-chunk streamer at BASELINE config 5's geometry.  The `backend` cases run the same kernel source
on the host emulator (-m "not gpu") and on the device (-m gpu)."""
import functools

import pytest
import torch

from util import rel_l2

from nbss_amd import ops
from nbss_amd._lib import NBSS_ONLINE_NORM_FREQUENCY, NBSS_ONLINE_NORM_NONE, NBSS_ONLINE_NORM_UTTERANCE

NONE, FREQ, UTT = NBSS_ONLINE_NORM_NONE, NBSS_ONLINE_NORM_FREQUENCY, NBSS_ONLINE_NORM_UTTERANCE
CHUNKS = [2, 5, 16, 17, 32]  # the minimum, a partial tile, one full tile, a tile plus one frame, two tiles


def _window(n_fft, win):
    w = torch.hann_window(n_fft, dtype=torch.float64)
    return w if win == 0 else w.sqrt()


class IO:
    """the two C entry points on caller-owned state, primed the way the wrapper primes it; outputs start as NaN (every element must be written)"""

    def __init__(self, backend, n_fft, win, B, M, S, C, norm, ref=0):
        self.lib, self.dev, self.n_fft, self.hop, self.F = backend.lib, backend.device, n_fft, n_fft // 2, n_fft // 2 + 1
        self.B, self.M, self.S, self.C, self.norm, self.ref = B, M, S, C, norm, ref
        self.tab = ops.stft_tables(self.lib, n_fft, win, self.dev)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)  # noqa: E731
        self.tail, self.ola, self.ws = z(B, M, self.hop), z(B, S, self.hop), z(B, self.F, C)
        self.xr_shape = {NONE: None, FREQ: (B, self.F, C), UTT: (B, 1, C)}[norm]

    def prime(self, x):
        self.tail.copy_(x[..., 1:self.hop + 1].flip(-1))
        self.ola.zero_()

    def stft(self, xc):
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=self.dev)  # noqa: E731
        feats, xrmm = nan(self.B, self.F, self.C, 2 * self.M), (nan(*self.xr_shape) if self.xr_shape else None)
        f = lambda t: ops._ptr(self.lib, t, torch.float32)  # noqa: E731
        xc = xc.contiguous()
        self.lib.call("nbss_online_stft_step", self.n_fft, self.norm, self.B, self.M, self.C, self.ref, f(self.tab), f(xc), f(self.tail), f(feats),
                      f(xrmm), f(self.ws), ops._stream(self.lib, feats))
        return feats, xrmm

    def istft(self, out, xrmm):
        y = torch.full((self.B, self.S, self.C * self.hop), float("nan"), dtype=torch.float32, device=self.dev)
        f = lambda t: ops._ptr(self.lib, t, torch.float32)  # noqa: E731
        out = out.contiguous()
        self.lib.call("nbss_online_istft_step", self.n_fft, self.norm, self.B, self.S, self.C, f(self.tab), f(out), f(xrmm), f(self.ola), f(y),
                      ops._stream(self.lib, y))
        return y

    def stft_all(self, x):
        """x [B, M, n C hop] -> feats [B, F, n C, 2M], xrmm [B, F | 1, n C] | None"""
        self.prime(x)
        step = self.C * self.hop
        parts = [self.stft(x[..., k:k + step]) for k in range(0, x.shape[-1], step)]
        return torch.cat([p[0] for p in parts], 2), (torch.cat([p[1] for p in parts], 2) if self.xr_shape else None)


@functools.lru_cache(maxsize=None)
def _signal(n_fft, win, C, B=2, M=3):
    """three chunks of signal and its torch.stft in fp64 (computed once, shared by the normalisation modes)"""
    g = torch.Generator().manual_seed(1000 * n_fft + 100 * win + C)
    x = torch.randn(B, M, 3 * C * (n_fft // 2), generator=g)
    X = torch.stft(x.double().reshape(B * M, -1), n_fft=n_fft, hop_length=n_fft // 2, win_length=n_fft, window=_window(n_fft, win), return_complex=True)
    return x, X.reshape(B, M, n_fft // 2 + 1, -1)[..., :3 * C]  # [B, M, F, 3C]: the stream has not seen the last frame (right padding) yet


def _as_complex(feats, M):
    B, F, T, _ = feats.shape
    return torch.view_as_complex(feats.double().cpu().reshape(B, F, T, M, 2).contiguous()).permute(0, 3, 1, 2)  # [B, M, F, T]


@pytest.mark.parametrize("C", CHUNKS)
@pytest.mark.parametrize("win", [0, 1])
@pytest.mark.parametrize("n_fft", [256, 512])
def test_stft_step_matches_torch_stft(backend, n_fft, win, C):
    """three pushes against torch.stft (fp64, center=True): the un-normalised frames feats * xrmm and xrmm itself, rel-L2 < 2e-5 (the bar of the
    whole-signal kernel in test_signal_loss_optim.py: the same arithmetic), for all three normalisation modes"""
    x, X = _signal(n_fft, win, C)
    ref = 1
    mag = X[:, ref].abs()  # [B, F, T]
    for norm, want in ((NONE, None), (FREQ, mag + 1e-6), (UTT, mag.mean(1, keepdim=True) + 1e-6)):
        io = IO(backend, n_fft, win, 2, 3, 2, C, norm, ref)
        feats, xrmm = io.stft_all(x.to(backend.device))
        got = _as_complex(feats, 3)
        if want is not None:
            e = rel_l2(xrmm, want)
            print(f"n_fft {n_fft} win {win} C {C} norm {norm}: xrmm {e:.2e}")
            assert e < 2e-5, (norm, e)
            got = got * xrmm.double().cpu()[:, None]
        e = rel_l2(got, X)
        print(f"n_fft {n_fft} win {win} C {C} norm {norm}: frames {e:.2e}")
        assert e < 2e-5, (norm, e)
        assert torch.equal(io.tail.cpu(), x[..., -(n_fft // 2):])  # the state: the last hop pushed


@pytest.mark.parametrize("C", CHUNKS)
@pytest.mark.parametrize("win", [0, 1])
@pytest.mark.parametrize("n_fft", [256, 512])
def test_istft_step_matches_torch_istft(backend, n_fft, win, C):
    """random spectra of 3 C frames: the delayed stream equals torch.istift (fp64) shifted by one hop, rel-L2 < 2e-5, without and with xrmm
    (per bin, per frame)"""
    B, S, hop, F, T = 2, 2, n_fft // 2, n_fft // 2 + 1, 3 * C
    g = torch.Generator().manual_seed(7 * n_fft + win + 10 * C)
    Y = torch.randn(B, S, F, T, 2, generator=g)
    want = torch.istft(torch.view_as_complex(Y.double()).reshape(B * S, F, T), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=_window(n_fft, win),
                       length=(T - 1) * hop).reshape(B, S, -1)
    for norm in (NONE, FREQ, UTT):
        io = IO(backend, n_fft, win, B, 1, S, C, norm)
        xr = None if norm == NONE else torch.rand(io.xr_shape[0], io.xr_shape[1], T, generator=g) + 0.5
        Yn = Y if xr is None else Y / xr[:, None, :, :, None]
        out = Yn.permute(0, 2, 3, 1, 4).reshape(B, F, T, 2 * S).to(backend.device)  # [B, F, T, 2S]
        ys = [io.istft(out[:, :, k:k + C], None if xr is None else xr[:, :, k:k + C].contiguous().to(backend.device)) for k in range(0, T, C)]
        y = torch.cat(ys, -1)
        assert torch.isfinite(y).all()
        e = rel_l2(y[..., hop:], want)
        print(f"n_fft {n_fft} win {win} C {C} norm {norm}: istft {e:.2e}")
        assert e < 2e-5, (norm, e)


@pytest.mark.parametrize("C", CHUNKS)
@pytest.mark.parametrize("n_fft,win,norms", [(256, 0, (NONE, FREQ)), (512, 1, (UTT,))])
def test_round_trip_is_a_one_hop_delay(backend, n_fft, win, norms, C):
    """stft step -> istft step returns the input one hop late, < 1e-5 (the bar of test_stft_istft_roundtrip)"""
    x, _ = _signal(n_fft, win, C)
    hop = n_fft // 2
    for norm in norms:
        io = IO(backend, n_fft, win, 2, 3, 3, C, norm, 1)
        xd = x.to(backend.device)
        io.prime(xd)
        ys = []
        for k in range(0, x.shape[-1], C * hop):
            feats, xrmm = io.stft(xd[..., k:k + C * hop])
            ys.append(io.istft(feats, xrmm))  # 2M = 2S: the microphones come back as "speakers"
        y = torch.cat(ys, -1)
        e = rel_l2(y[..., hop:], x[..., :-hop])
        print(f"n_fft {n_fft} C {C} norm {norm}: round trip {e:.2e}")
        assert e < 1e-5, (norm, e)


@pytest.mark.parametrize("norm", [FREQ, UTT])
def test_io_kernels_do_not_depend_on_the_chunk_size(backend, norm):
    """the same 160 frames of signal in chunks of 2, 5, 16 and 32: feats, xrmm and the sample stream are BITWISE the same (a frame is a GEMM
    column: its K order does not depend on its neighbours; the per-frame fold over F has a fixed order), and so is a second pass after a reset"""
    n_fft, hop, T = 256, 128, 160
    x = torch.randn(1, 2, T * hop, generator=torch.Generator().manual_seed(3)).to(backend.device)

    def run(io):
        io.prime(x)
        fs, xs, ys = [], [], []
        for k in range(0, x.shape[-1], io.C * hop):
            feats, xrmm = io.stft(x[..., k:k + io.C * hop])
            fs.append(feats), xs.append(xrmm), ys.append(io.istft(feats, xrmm))
        return torch.cat(fs, 2), torch.cat(xs, 2), torch.cat(ys, -1)

    want = None
    for C in (2, 5, 16, 32):
        io = IO(backend, n_fft, 0, 1, 2, 2, C, norm, 1)
        got = run(io)
        assert all(torch.isfinite(t).all() for t in got)
        if want is None:
            want = got
        for a, b, name in zip(got, want, ("feats", "xrmm", "samples")):
            assert torch.equal(a, b), (C, name, float((a - b).abs().max()))
        if C == 16:
            again = run(io)  # prime() is what a reset does to the I/O state
            assert all(torch.equal(a, b) for a, b in zip(again, got)), C


def test_entry_points_refuse(backend):
    lib = backend.lib
    io = IO(backend, 256, 0, 1, 2, 2, 4, FREQ)
    f = lambda t: ops._ptr(lib, t, torch.float32)  # noqa: E731
    z = torch.zeros(1, 129, 4, 4, device=backend.device)
    x, y, xr, st = torch.zeros(1, 2, 4 * 128, device=backend.device), torch.zeros(1, 2, 4 * 128, device=backend.device), torch.ones(1, 129, 4, device=backend.device), None
    st = ops._stream(lib, z)
    stft = lambda n_fft, C, xp=f(x), B=1: lib.nbss_online_stft_step(n_fft, FREQ, B, 2, C, 0, f(io.tab), xp, f(io.tail), f(z), f(xr), None, st)  # noqa: E731
    istft = lambda n_fft, C, op=f(z), B=1: lib.nbss_online_istft_step(n_fft, FREQ, B, 2, C, f(io.tab), op, f(xr), f(io.ola), f(y), st)  # noqa: E731
    for fn in (stft, istft):
        assert fn(256, 1) == -2 and fn(256, 33) == -2 and fn(128, 4) == -2 and fn(1024, 4) == -2  # NBSS_EUNSUPPORTED
        assert fn(256, 4, None) == -1 and fn(256, 4, B=0) == -1 and fn(256, 0) == -1  # NBSS_EINVAL: null pointer, empty shapes
    assert lib.nbss_online_stft_step(256, UTT, 1, 2, 4, 0, f(io.tab), f(x), f(io.tail), f(z), f(xr), None, st) == -1  # 'utterance' needs its scratch
    assert lib.nbss_online_stft_step(256, FREQ, 1, 2, 4, 2, f(io.tab), f(x), f(io.tail), f(z), f(xr), None, st) == -1  # reference channel out of range


# ---- the streamers ------------------------------------------------------------------------------------------------------------------------
NATIVE_KW = dict(dim_input=4, dim_output=4, num_layers=1, dim_squeeze=8, num_freqs=129, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192, num_heads=4,
                 dropout=(0, 0, 0), kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], full_share=0, attention="ret(2)",
                 decay=[4, 5, 9, 10], rope=False)


def _module(norm=("frequency", True), seed=5, n_fft=256, n_hop=128, channels=(0, 1), **over):
    from SharedTrainer import TrainModule
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    from models.io.norm import Norm
    from models.io.stft import STFT
    torch.manual_seed(seed)
    net = OnlineSpatialNet(**{**NATIVE_KW, **over}).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return TrainModule(arch=net, channels=list(channels), ref_channel=channels[-1], stft=STFT(n_fft=n_fft, n_hop=n_hop, win_len=n_fft), norm=Norm(*norm)).eval()


def _check_against_feature_level_streaming(name, lib, device, attention, norm):
    from nbss_amd.online_io import NativeWaveStreamer
    m = _module(norm=norm, attention=attention).to(device)
    B = 1 if name == "emu" else 2
    x = torch.randn(B, 2, 12 * 128, generator=torch.Generator().manual_seed(0)).to(device)
    want, _ = m.forward_streaming(x, 4, native=False)
    s = NativeWaveStreamer(m.arch, B, 4, m.stft, m.norm, m.channels, m.ref_channel, device=device, lib=lib, use_graph=name == "hip")
    y = s.separate(x)
    assert y.shape == want.shape and s.latency_samples == 128 and s.chunks == 4
    e = rel_l2(y, want)
    print(f"{name} {attention} {norm}: separate vs forward_streaming(native=False) {e:.2e}")
    assert e < 2e-4, e
    assert (s.graph is not None) == (name == "hip")


def test_native_wave_streamer_matches_feature_level_streaming(backend):
    """NativeWaveStreamer.separate against TrainModule.forward_streaming(native=False) (whole-utterance STFT, the torch.nn step, one iSTFT) on the same
    module: rel-L2 < 2e-4 on the waveform, the bar test_native_streaming_step_matches_module holds the feature-level native step to against the torch
    step.  129 bins, one layer, 2 microphones -> 2 speakers, 'ret(2)', Norm('frequency', online), chunk 4, 12 * 128 samples; B = 1 on the emulator, 2 on
    the device."""
    _check_against_feature_level_streaming(backend.name, backend.lib, backend.device, "ret(2)", ("frequency", True))


@pytest.mark.gpu
@pytest.mark.parametrize("attention,norm", [("ret(2)", ("utterance", True)), ("mhsa(11)", ("frequency", True)), ("mhsa(11)", ("utterance", True))])
def test_native_wave_streamer_matches_feature_level_streaming_on_the_device(hip_lib, attention, norm):
    """the same on the device for windowed attention and for Norm('utterance', online=True) (what configs/onlineSpatialNet.yaml names)"""
    _check_against_feature_level_streaming("hip", hip_lib, torch.device("cuda:0"), attention, norm)


@pytest.mark.gpu
def test_native_wave_streamer_behaviour(hip_lib):
    """open_stream on the device: one captured graph; separate twice is bitwise the same; push after reset() re-primes; a signal that is no
    multiple of the chunk goes through the zero-padded last chunk"""
    from nbss_amd.online_io import NativeWaveStreamer
    dev = torch.device("cuda:0")
    m = _module().to(dev)
    s = m.open_stream(2, 4)
    assert isinstance(s, NativeWaveStreamer)
    x = torch.randn(2, 2, 12 * 128, device=dev)
    y1 = s.separate(x)
    assert s.graph is not None
    y2 = s.separate(x)
    assert torch.equal(y1, y2)
    s.reset()  # by hand: three pushes and the closing step
    ys = [s.push(x[..., k:k + 512]) for k in range(0, 1536, 512)] + [s.finish()]
    assert torch.equal(torch.cat(ys, -1)[..., 128:128 + 1536], y1)
    xo = x[..., :11 * 128]  # 11 frames of signal: two chunks + a last one of 3 frames, the reflect padding and zeros
    yo = s.separate(xo)
    want, _ = m.forward_streaming(xo, 4, native=False)
    assert s.chunks == 3 and yo.shape == want.shape and rel_l2(yo, want) < 2e-4, rel_l2(yo, want)


@pytest.mark.parametrize("chunk,frames,norm", [(4, 12, ("frequency", True)), (5, 12, ("utterance", True)), (40, 12, ("frequency", True))])
def test_wave_streamer_matches_whole_signal_forward(chunk, frames, norm):
    """WaveStreamer (torch ops only) on the CPU against TrainModule.forward on the whole signal, 'mhsa(7)': < 1e-5 (the bar of tests/test_online.py
    for that attention)"""
    from nbss_amd.online_io import WaveStreamer
    m = _module(norm=norm, attention="mhsa(7)", dim_hidden=32, dim_ffn=64)
    x = torch.randn(2, 2, frames * 128, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want, _ = m.forward(x)
    s = m.open_stream(2, chunk)
    assert isinstance(s, WaveStreamer) and s.latency_samples == 128 and s.graph is None
    y = s.separate(x)
    e = rel_l2(y, want)
    print(f"chunk {chunk} {norm}: WaveStreamer vs forward {e:.2e}")
    assert y.shape == want.shape and e < 1e-5, e


def test_refusals():
    """what the native streamer refuses, with the reason; open_stream then hands back WaveStreamer where the torch ops can serve the request — a stream
    cannot serve chunk 1 (no x[hop] for the left reflect padding), an offline normalisation or an unbounded attention state at all, and hop != n_fft/2
    is out of scope: there WaveStreamer refuses as well"""
    from models.io.norm import Norm
    from models.io.stft import STFT
    from nbss_amd.online_io import NativeWaveStreamer, WaveStreamer, norm_kind
    good = _module()
    mk = lambda m, chunk, **kw: NativeWaveStreamer(m.arch, 1, chunk, kw.get("stft", m.stft), kw.get("norm", m.norm), m.channels, m.ref_channel, device="cpu",  # noqa: E731
                                                   lib=object())
    with pytest.raises(NotImplementedError, match="frames per chunk"):
        mk(good, 1)
    with pytest.raises(NotImplementedError, match="frames per chunk"):
        mk(good, 33)
    with pytest.raises(NotImplementedError, match="n_hop must be n_fft / 2"):
        mk(good, 4, stft=STFT(n_fft=256, n_hop=64, win_len=256))
    with pytest.raises(NotImplementedError, match="n_fft 256 and 512"):
        mk(good, 4, stft=STFT(n_fft=128, n_hop=64, win_len=128))
    with pytest.raises(NotImplementedError, match="offline normalisation"):
        mk(good, 4, norm=Norm("utterance", online=False))
    with pytest.raises(NotImplementedError, match="forgetting"):
        norm_kind(("forgetting", True))
    inf = _module(attention="mhsa(inf)")
    with pytest.raises(NotImplementedError, match="finite window"):
        mk(inf, 4)
    # the fall-back: what torch ops can stream
    assert isinstance(good.open_stream(1, 33), WaveStreamer)  # (host module: WaveStreamer whatever the chunk)
    assert isinstance(_module(dim_hidden=32, dim_ffn=64).open_stream(1, 4), WaveStreamer)
    # ... and what no stream can
    with pytest.raises(NotImplementedError, match="frames per chunk"):
        good.open_stream(1, 1)
    with pytest.raises(NotImplementedError, match="offline normalisation"):
        _module(norm=("utterance", False)).open_stream(1, 4)
    with pytest.raises(NotImplementedError, match="fixed-size state"):
        inf.open_stream(1, 4)
    with pytest.raises(NotImplementedError, match="n_hop must be n_fft / 2"):
        _module(n_hop=64).open_stream(1, 4)


@pytest.mark.gpu
def test_refused_requests_fall_back_on_the_device(hip_lib):
    """on a HIP device open_stream tries the native streamer first: chunk 33 and a network outside the native geometry come back as WaveStreamer"""
    from nbss_amd.online_io import NativeWaveStreamer, WaveStreamer
    dev = torch.device("cuda:0")
    good = _module().to(dev)
    assert isinstance(good.open_stream(1, 4), NativeWaveStreamer)
    assert isinstance(good.open_stream(1, 33), WaveStreamer)
    assert isinstance(good.open_stream(1, 4, native=False), WaveStreamer)
    assert isinstance(_module(dim_hidden=32, dim_ffn=64).to(dev).open_stream(1, 4), WaveStreamer)
    with pytest.raises(NotImplementedError, match="frames per chunk"):
        good.open_stream(1, 33, native=True)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_native_wave_streamer_at_the_config5_geometry(hip_lib):
    """BASELINE config 5's geometry: 129 bins, 8 layers, 6 microphones -> 2 speakers, 'ret(2)', 400 frames in 16-frame chunks, one graph replay per chunk:
    separate equals forward_streaming(native=True) (whole-utterance STFT / iSTFT around the same native step) to the 2e-4 of the one-layer case, and a
    second pass is bitwise the first"""
    from nbss_amd.online_io import NativeWaveStreamer
    dev = torch.device("cuda:0")
    m = _module(seed=0, channels=(0, 1, 2, 3, 4, 5), dim_input=12, num_layers=8).to(dev)
    x = torch.randn(1, 6, 400 * 128, device=dev)
    s = m.open_stream(1, 16)
    assert isinstance(s, NativeWaveStreamer)
    y = s.separate(x)
    assert s.graph is not None and s.chunks == 26 and torch.isfinite(y).all()
    assert torch.equal(s.separate(x), y)
    want, st = m.forward_streaming(x, 16, native=True)
    assert st["native"]
    e = rel_l2(y, want)
    print(f"config 5: separate vs forward_streaming(native=True) {e:.2e}")
    assert e < 2e-4, e


def test_predict_stream_wave_switch(tmp_path):
    """`predict --stream_wave true` of an OnlineSpatialNet routes through open_stream(...).separate (here: the torch WaveStreamer on the CPU) and reports
    chunks / graph_replays / native / latency_samples; the default stays on the feature-level path.  8000 samples are 62.5 hops: the stream is filled up with
    zeros where forward_streaming reflects, which the causal network carries into the last two frames only"""
    from pathlib import Path

    from SharedTrainer import TrainCLI
    root = Path(__file__).resolve().parent.parent
    args = ["--config", str(root / "configs" / "onlineSpatialNet.yaml"), "--config", str(root / "configs" / "datasets" / "synthetic.yaml"), "--model.arch.dim_input=12",
            "--model.arch.dim_output=4", "--model.arch.num_freqs=129", "--data.num_samples=[4,2,2]", "--trainer.accelerator=cpu", "--model.arch.num_layers=1",
            "--model.arch.dim_hidden=32", "--model.arch.dim_ffn=64", "--model.arch.dim_squeeze=4", "--data.audio_time_len=[0.5,0.5,1.0]"]
    feat = TrainCLI(argv=["predict"] + args + ["--stream_chunk=8"]).result
    wave = TrainCLI(argv=["predict"] + args + ["--stream_chunk=8", "--stream_wave=true"]).result
    assert "latency_samples" not in feat and feat["streamed"]
    assert wave["streamed"] and wave["latency_samples"] == 128 and wave["native"] is False and wave["graph_replays"] == 0
    assert wave["chunks"] == len(wave["yr_hat"]) * 8  # 63 frames of signal + the right padding: 8 chunks of 8 per batch
    a, b = wave["yr_hat"][0], feat["yr_hat"][0]
    assert a.shape == b.shape == (2, 2, 8000)
    assert float((a[..., :7680] - b[..., :7680]).norm() / b[..., :7680].norm()) < 1e-4
