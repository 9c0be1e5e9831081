"""OnlineSpatialNet's 'mamba(16,4)' and 'mamba(16,4,not_replace_ffn)' variants through the native streaming step (nbss_amd/online.py with
NBSS_ONLINE_NATIVE_MAMBA_STEP=1: one nbss_online_mamba_step per Mamba block) at the public interface: the gate `supported`, NativeOnlineStreamer against
the module's torch streaming step and its whole-signal forward, NativeWaveStreamer against the torch WaveStreamer, and — on the GPU — BASELINE config 5's
geometry and TrainModule's streaming predict.  The nets are the 2-layer, 9-frequency, 4 -> 4 nets of tests/test_online.py (NATIVE_KW) with the attention
replaced; the `backend` cases run the same kernel source on the host emulator (-m "not gpu") and on the device (-m gpu)."""
import pytest
import torch

from util import rel_l2

SWITCH = "NBSS_ONLINE_NATIVE_MAMBA_STEP"
VARIANTS = ["mamba(16,4)", "mamba(16,4,not_replace_ffn)"]
NATIVE_KW = dict(dim_input=4, dim_output=4, num_layers=2, dim_squeeze=8, num_freqs=9, encoder_kernel_size=5, dim_hidden=96, dim_ffn=192, num_heads=4,
                 dropout=(0, 0, 0), kernel_size=(5, 3), conv_groups=(8, 8), norms=["LN", "LN", "GN", "LN", "LN", "LN"], full_share=0, rope=False)


def _net(monkeypatch, attention, seed=5, **over):
    from models.arch.OnlineSpatialNet import OnlineSpatialNet
    monkeypatch.setenv("NBSS_ONLINE_MAMBA", "1")
    torch.manual_seed(seed)
    net = OnlineSpatialNet(**{**NATIVE_KW, "attention": attention, **over}).eval()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return net


@pytest.mark.parametrize("attention", VARIANTS)
def test_switch_off_names_the_switch(monkeypatch, attention, emu_lib):
    """the default answer stays a refusal that says 'mamba' and now names the switch; values other than '1' leave it off"""
    from nbss_amd.online import NativeOnlineStreamer, supported
    net = _net(monkeypatch, attention)
    for value in (None, "0", "true", "11"):
        monkeypatch.delenv(SWITCH, raising=False)
        if value is not None:
            monkeypatch.setenv(SWITCH, value)
        why = supported(net)
        assert why is not None and "mamba" in why and SWITCH in why, (value, why)
        with pytest.raises(NotImplementedError, match="mamba.*" + SWITCH):
            NativeOnlineStreamer(net, 1, 4, device="cpu", lib=emu_lib)


def test_switch_on_accepts_the_geometry_and_refuses_others(monkeypatch):
    """read when `supported` is called: the same net is accepted once the switch is '1'; another (d_state, d_conv) gets mamba_supported's reason"""
    from nbss_amd.online import supported
    nets = [_net(monkeypatch, a) for a in VARIANTS]
    assert all(supported(n) is not None for n in nets)
    monkeypatch.setenv(SWITCH, "1")
    assert all(supported(n) is None for n in nets)
    assert "d_state must be 16 (got 8)" in supported(_net(monkeypatch, "mamba(8,3,not_replace_ffn)"))
    assert "d_conv must be 4 (got 3)" in supported(_net(monkeypatch, "mamba(16,3)"))
    assert supported(_net(monkeypatch, "ret(2)", decay=[4, 5, 9, 10])) is None  # the other variants do not depend on the switch
    monkeypatch.setenv(SWITCH, "0")
    assert all(supported(n) is not None for n in nets)
    assert supported(_net(monkeypatch, "ret(2)", decay=[4, 5, 9, 10])) is None


@pytest.mark.parametrize("chunk", [1, 5, 8, 25, 32])
@pytest.mark.parametrize("attention", VARIANTS)
def test_native_streaming_step_matches_module(monkeypatch, backend, attention, chunk):
    """NativeOnlineStreamer.step chunk by chunk (T = 3 chunks, batch 2) against the module's torch streaming step (Mamba.step frame by frame) and against
    the whole-signal forward: rel-L2 < 2e-4 for both (the bound of tests/test_online.py for the native step against the torch step; the Mamba step form
    equals the whole-sequence form to 1e-5); one captured graph exactly on the device; after reset() a second pass gives the same bits"""
    from nbss_amd.online import NativeOnlineStreamer
    net = _net(monkeypatch, attention).to(backend.device)
    monkeypatch.setenv(SWITCH, "1")
    T = 3 * chunk
    x = torch.randn(2, 9, T, 4, device=backend.device)
    with torch.no_grad():
        y = net(x)
        st = net.init_stream(2, device=backend.device)
        ys = torch.cat([net.forward_stream(x[:, :, c:c + chunk], st) for c in range(0, T, chunk)], 2)
    s = NativeOnlineStreamer(net, 2, chunk, device=backend.device, lib=backend.lib, use_graph=backend.name == "hip")
    from nbss_amd.online import MAMBA, TCONVFFN
    ffn_mamba = "not_replace_ffn" not in attention
    assert s.kinds == (MAMBA, MAMBA if ffn_mamba else TCONVFFN) and all([k for k, _, _ in steps] == list(s.kinds) for steps in s.steps)
    assert ("ffn_s1" in s.state) == (not ffn_mamba) and ("a3" in s.shared) == ("gn_sums" in s.shared) == (not ffn_mamba)  # no T-ConvFFN buffers behind a replaced FFN
    assert ("ffn_conv" in s.state) == ("ffn_ssm" in s.state) == ffn_mamba and not hasattr(s, "a3")
    yn = torch.cat([s.step(x[:, :, c:c + chunk]) for c in range(0, T, chunk)], 2)
    e = (rel_l2(yn, ys), rel_l2(yn, y))
    print(f"{backend.name} {attention} chunk {chunk}: vs forward_stream {e[0]:.2e}, vs forward {e[1]:.2e}")
    assert e[0] < 2e-4 and e[1] < 2e-4, e
    assert (s.graph is not None) == (backend.name == "hip")
    assert all(b.any() for b in s._buffers())  # every state buffer is in use ...
    s.reset()
    assert not any(b.any() for b in s._buffers())  # ... and reset() covers it
    yn2 = torch.cat([s.step(x[:, :, c:c + chunk]) for c in range(0, T, chunk)], 2)
    assert torch.equal(yn, yn2)


def _wave_module(monkeypatch, attention):
    from SharedTrainer import TrainModule
    from models.io.norm import Norm
    from models.io.stft import STFT
    net = _net(monkeypatch, attention, num_layers=1, num_freqs=129)  # (tests/test_online_wave.py: _module — 2 microphones -> 2 speakers, n_fft 256)
    return TrainModule(arch=net, channels=[0, 1], ref_channel=1, stft=STFT(n_fft=256, n_hop=128, win_len=256), norm=Norm("frequency", True)).eval()


@pytest.mark.parametrize("attention", VARIANTS)
def test_native_wave_streamer_matches_torch_wave_streamer(monkeypatch, backend, attention):
    """NativeWaveStreamer (STFT step, the network step with its Mamba launches, iSTFT step) against the torch WaveStreamer on 12 hops of signal in chunks of
    4 frames: rel-L2 < 2e-4 on the waveform, the bound tests/test_online_wave.py holds the native wave streamer to; B = 1 on the emulator, 2 on the device"""
    from nbss_amd.online_io import NativeWaveStreamer, WaveStreamer
    m = _wave_module(monkeypatch, attention).to(backend.device)
    B = 1 if backend.name == "emu" else 2
    x = torch.randn(B, 2, 12 * 128, generator=torch.Generator().manual_seed(0)).to(backend.device)
    ref = m.open_stream(B, 4, native=False)
    assert isinstance(ref, WaveStreamer)
    want = ref.separate(x)
    monkeypatch.setenv(SWITCH, "1")
    s = NativeWaveStreamer(m.arch, B, 4, m.stft, m.norm, m.channels, m.ref_channel, device=backend.device, lib=backend.lib, use_graph=backend.name == "hip")
    y = s.separate(x)
    e = rel_l2(y, want)
    print(f"{backend.name} {attention}: NativeWaveStreamer vs WaveStreamer {e:.2e}")
    assert y.shape == want.shape and e < 2e-4, e
    assert (s.graph is not None) == (backend.name == "hip")
    assert torch.equal(s.separate(x), y)
    if backend.name == "hip":  # open_stream dispatches on `supported`: native with the switch, the torch streamer without
        assert isinstance(m.open_stream(B, 4), NativeWaveStreamer)
        monkeypatch.delenv(SWITCH)
        assert isinstance(m.open_stream(B, 4), WaveStreamer)


@pytest.mark.gpu
@pytest.mark.parametrize("attention", VARIANTS)
def test_native_streaming_step_at_the_config5_geometry(monkeypatch, hip_lib, attention):
    """BASELINE config 5's geometry on the GPU: 129 frequencies, 8 layers, 12 -> 4, 320 frames in 16-frame chunks, one HIP graph per chunk — the native step
    against the torch.nn streaming step of the same module under graph capture (< 1e-4), finite, and bitwise equal to itself on a second pass"""
    from models.arch.OnlineSpatialNet import OnlineStreamer
    from nbss_amd.online import NativeOnlineStreamer
    dev = torch.device("cuda:0")
    net = _net(monkeypatch, attention, seed=0, dim_input=12, num_layers=8, num_freqs=129).to(dev)
    monkeypatch.setenv(SWITCH, "1")
    chunk, T = 16, 320
    x = torch.randn(1, 129, T, 12, device=dev)
    ref, s = OnlineStreamer(net, 1, chunk, use_graph=True), NativeOnlineStreamer(net, 1, chunk)
    want = torch.cat([ref.step(x[:, :, c:c + chunk]) for c in range(0, T, chunk)], 2)
    y = torch.cat([s.step(x[:, :, c:c + chunk]) for c in range(0, T, chunk)], 2)
    assert s.graph is not None and ref.graph is not None
    assert torch.isfinite(y).all()
    e = rel_l2(y, want)
    print(f"config 5 {attention}: native step vs OnlineStreamer {e:.2e}")
    assert e < 1e-4, e
    s.reset()
    y2 = torch.cat([s.step(x[:, :, c:c + chunk]) for c in range(0, T, chunk)], 2)
    assert torch.equal(y, y2)


@pytest.mark.gpu
def test_streaming_predict_takes_the_native_path_with_the_switch(monkeypatch, hip_lib):
    """TrainModule.forward_streaming (what `predict --stream_chunk` runs) on a mamba model: stats["native"] is True with the switch and False without, on the
    same module (the cached streamer is not reused across the switch), and the two paths agree to the 2e-4 of the feature-level tests"""
    m = _wave_module(monkeypatch, "mamba(16,4)").to(torch.device("cuda:0"))
    x = torch.randn(2, 2, 12 * 128, device="cuda:0")
    monkeypatch.delenv(SWITCH, raising=False)
    y0, st0 = m.forward_streaming(x, 4)
    monkeypatch.setenv(SWITCH, "1")
    y1, st1 = m.forward_streaming(x, 4)
    monkeypatch.delenv(SWITCH)
    _, st2 = m.forward_streaming(x, 4)
    assert st0["native"] is False and st1["native"] is True and st2["native"] is False
    assert st1["graph_replays"] == st1["chunks"]
    assert rel_l2(y1, y0) < 2e-4, rel_l2(y1, y0)
