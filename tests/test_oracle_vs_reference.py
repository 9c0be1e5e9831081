"""Pin the oracle against the reference's OWN modules, through what they computed (tests/golden/make_golden.py oraclepin ->
tests/golden/oracle_pins.npz, fp64 outputs of the reference's SpatialNet; tests/golden/stft_norm_n1500.npz, its STFT / Norm / iSTFT).
Parameters are not stored: this repo's drop-in SpatialNet draws the same ones from the same seed, which a checksum per case pins."""
from pathlib import Path

import numpy as np
import pytest
import torch

from models.arch.SpatialNet import SpatialNet
from oracle import io_ref
from oracle import spatialnet_ref as ref
from util import rel_l2

GOLDEN = Path(__file__).resolve().parent / "golden"
PINS = GOLDEN / "oracle_pins.npz"
SMALL = dict(dim_input=12, dim_output=4, num_layers=8, dim_hidden=96, dim_ffn=192, num_heads=4, kernel_size=(5, 3), conv_groups=(8, 8),
             norms=("LN", "LN", "GN", "LN", "LN", "LN"), dim_squeeze=8, num_freqs=129, full_share=0)


def sketch(t):
    """[..., 96] -> [..., 1] through the seeded fp64 vector make_golden.py's sketch() stored the reference's sub-block outputs with"""
    return t @ torch.randn(t.shape[-1], 1, generator=torch.Generator().manual_seed(11), dtype=torch.float64)


@pytest.fixture(scope="module")
def pins():
    return np.load(PINS)


def _params(net, want_checksum):
    """the drop-in module's parameters (fp64), checked to be the ones the reference drew from the same seed"""
    sd = net.state_dict()
    got = [sum(float(v.double().sum()) for v in sd.values()), sum(float(v.double().abs().sum()) for v in sd.values())]
    assert np.allclose(got, want_checksum, rtol=1e-12, atol=0), "the drop-in module's seeded parameters differ from the reference's"
    return {k: v.detach().double() for k, v in sd.items()}


def test_spatialnet_small_forward_and_grads(pins):
    """SpatialNet-small exactly as configs/SpatialNet.yaml builds it (1 191 092 parameters), short input"""
    torch.manual_seed(0)
    torch.set_num_threads(4)
    net = SpatialNet(**SMALL).double()
    assert sum(p.numel() for p in net.parameters()) == 1191092  # images/model_size_and_flops.png: 1.2 M
    x = torch.randn(1, 129, 30, 12, dtype=torch.float64)
    p = _params(net, pins["small/checksum"])
    assert rel_l2(ref.spatialnet(x, p, 8), pins["small/y"]) < 1e-10
    # each sub-block against the reference layer's own methods (layer 3), through a fixed random projection of the 96 channels
    h = torch.randn(1, 129, 30, 96, dtype=torch.float64)
    assert rel_l2(sketch(ref.fconv(h, p, "layers.3.fconv1")), pins["small/fconv1"]) < 1e-10
    assert rel_l2(sketch(ref.full(h, p, "layers.3")), pins["small/full"]) < 1e-10
    assert rel_l2(sketch(ref.mhsa(h, p, "layers.3")), pins["small/mhsa"]) < 1e-10
    assert rel_l2(sketch(ref.tconvffn(h, p, "layers.3")), pins["small/tconvffn"]) < 1e-10


def test_spatialnet_large_16khz_forward(pins):
    """SpatialNet-large as the "for large" comments of configs/SpatialNet.yaml build it (12 layers, 192 / 384 / squeeze 16), 257 frequencies
    (16 kHz): the oracle the large-geometry HIP kernels are tested against (tests/test_large.py) IS the reference's forward"""
    torch.manual_seed(1)
    torch.set_num_threads(4)
    net = SpatialNet(**dict(SMALL, num_layers=12, dim_hidden=192, dim_ffn=384, dim_squeeze=16, num_freqs=257)).double()
    x = torch.randn(1, 257, 12, 12, dtype=torch.float64)
    p = _params(net, pins["large/checksum"])
    assert rel_l2(ref.spatialnet(x, p, 12), pins["large/y"]) < 1e-10


def test_state_dict_interchanges_with_the_reference(pins, tmp_path):
    """checkpoint contract: the drop-in module's state_dict has the reference SpatialNet's keys and shapes, in its order
    (what a strict load into the reference checks), and survives a round trip through a file into another drop-in module"""
    kw = dict(SMALL, num_layers=3)
    torch.manual_seed(3)
    ours = SpatialNet(**kw)
    sd = ours.state_dict()
    assert list(sd.keys()) == [str(k) for k in pins["sd/keys"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in pins["sd/shapes"]]
    torch.save(sd, tmp_path / "sd.pt")
    torch.manual_seed(4)
    ours2 = SpatialNet(**kw)
    ours2.load_state_dict(torch.load(tmp_path / "sd.pt"), strict=True)
    for (k, a), (_, b) in zip(sd.items(), ours2.state_dict().items()):
        assert torch.equal(a, b), k
    # and the oracle evaluated on these weights is the reference's forward (so the HIP path, pinned to the oracle, is too)
    x = torch.randn(1, 129, 12, 12, dtype=torch.float64)
    p = _params(ours, pins["sd/checksum"])
    assert rel_l2(ref.spatialnet(x, p, 3), pins["sd/y"]) < 1e-10


def test_stft_norm_istft():
    z = np.load(GOLDEN / "stft_norm_n1500.npz")  # the reference's STFT(256, 128) / Norm("frequency", ref_channel=1) / iSTFT
    x = torch.from_numpy(z["sig"])
    X = torch.complex(torch.from_numpy(z["X_re"]), torch.from_numpy(z["X_im"]))
    back = torch.from_numpy(z["back"])
    assert rel_l2(io_ref.stft(x), X) < 1e-6
    on, omm = io_ref.norm_frequency_online(X, 1)
    B, C, F, T = X.shape
    assert rel_l2(torch.view_as_real(on.permute(0, 2, 3, 1)).reshape(B, F, T, 2 * C), z["Xl"]) < 1e-6 and rel_l2(omm, z["XrMM"]) < 1e-6
    assert rel_l2(io_ref.istft(X, x.shape[-1]), back) < 1e-6
    assert rel_l2(back, x) < 1e-5  # the reference's own round-trip smoke check (stft.py:106-112)
