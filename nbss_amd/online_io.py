"""Waveform-to-waveform streaming of an OnlineSpatialNet: samples in, samples out, `chunk` frames (chunk * hop samples) per call.

Alignment.  Frame t of the stream is frame t of torch.stft(center=True) on the whole signal: it covers the samples [(t-1) hop, (t+1) hop)
(hop = n_fft / 2).  The frames of a chunk are cut from `tail | chunk` (tail = the hop samples before the chunk), and the overlap-add of
frame t completes the samples [(t-1) hop, t hop) — so the sample stream leaves ONE HOP late: call k returns y[k C hop - hop : (k+1) C hop - hop].
That hop is the algorithmic latency (`latency_samples`).  The reflect padding of torch.stft at both ends of the signal is handled here, not
in the kernels: the first push after a reset primes `tail` with flip(x[1 : hop+1]) (which is why a chunk has at least two frames: a one-frame
first chunk does not hold x[hop]), and `finish()` pushes x[N-2] .. x[N-hop-1] followed by zeros (the network is causal: the frames after the
padding cannot reach a real one).

`NativeWaveStreamer` is NativeOnlineStreamer's launch sequence between the two kernels of csrc/online_io.hip — STFT step (+ online
normalisation) -> 6 L + 2 network launches -> (inverse normalisation +) iSTFT step — captured as ONE HIP graph, all state (network, `tail`,
overlap-add) in device buffers; `WaveStreamer` is the same interface on torch ops (torch.fft + the torch.nn step OnlineStreamer) for host
tensors and for what the native step refuses, the way OnlineStreamer stands behind NativeOnlineStreamer."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import Tensor

from . import ops
from ._lib import NBSS_ONLINE_NORM_FREQUENCY, NBSS_ONLINE_NORM_NONE, NBSS_ONLINE_NORM_UTTERANCE, Lib
from .online import NativeOnlineStreamer

_WHAT = "waveform streaming: "


def norm_kind(norm_mode) -> int:
    """NBSS_ONLINE_NORM_* of a models.io.norm.Norm, a mode name ('none' | 'frequency' | 'utterance': online) or a (mode, online) pair;
    NotImplementedError with the reason for what cannot be streamed"""
    if norm_mode is None or isinstance(norm_mode, str):
        mode, online = norm_mode, True
    elif isinstance(norm_mode, (tuple, list)):
        mode, online = norm_mode
    else:
        mode, online = norm_mode.mode, norm_mode.online
    if mode in (None, "none"):
        return NBSS_ONLINE_NORM_NONE
    if mode == "forgetting":
        raise NotImplementedError(_WHAT + "Norm('forgetting') is not provided")
    if mode not in ("frequency", "utterance"):
        raise NotImplementedError(_WHAT + f"unknown normalisation {mode!r}")
    if not online:
        raise NotImplementedError(_WHAT + f"Norm('{mode}', online=False) is an offline normalisation (statistics of the whole utterance); streaming needs online=True")
    return NBSS_ONLINE_NORM_FREQUENCY if mode == "frequency" else NBSS_ONLINE_NORM_UTTERANCE


def _check_stft(stft) -> None:
    if stft.n_hop * 2 != stft.n_fft or stft.win_len != stft.n_fft:
        raise NotImplementedError(_WHAT + f"n_hop must be n_fft / 2 and win_len n_fft (got n_fft {stft.n_fft}, n_hop {stft.n_hop}, win_len {stft.win_len}): "
                                  "the one-hop overlap-add state and latency rest on it")


class _WaveIO:
    """what both streamers share: the reflect padding at the two ends, the bookkeeping of a stream, separate()"""

    B: int
    C: int
    hop: int
    channels: Optional[List[int]]

    def _init_io(self, batch: int, chunk: int, stft, channels: Optional[Sequence[int]], ref_channel: Optional[int], n_in: int) -> None:
        self.B, self.C, self.stft, self.n_fft, self.hop = batch, chunk, stft, stft.n_fft, stft.n_hop
        self.channels = list(channels) if channels is not None else None
        self.M = len(self.channels) if self.channels is not None else n_in // 2
        if 2 * self.M != n_in:
            raise ValueError(f"the network reads {n_in} input features = {n_in // 2} microphones, `channels` selects {self.M}")
        ref = 0 if ref_channel is None else ref_channel
        self.ref = self.channels.index(ref) if self.channels is not None else ref
        self.primed, self.last, self.chunks = False, None, 0

    @property
    def latency_samples(self) -> int:
        return self.hop

    def _select(self, x: Tensor) -> Tensor:
        return (x[:, self.channels] if self.channels is not None else x).float()

    def _step(self, xs: Tensor) -> Tensor:  # xs [B, M, C hop] -> [B, S, C hop]; state in place
        raise NotImplementedError

    def _prime(self, left: Tensor) -> None:  # left [B, M, hop] = the reflect padding in front of the signal
        raise NotImplementedError

    def _advance(self, xs: Tensor, real: Tensor) -> Tensor:
        if not self.primed:
            if real.shape[-1] < self.hop + 1:
                raise ValueError(f"the first chunk of a stream must hold at least hop + 1 = {self.hop + 1} samples (left reflect padding)")
            self._prime(real[..., 1:self.hop + 1].flip(-1))
            self.primed = True
        if real.shape[-1]:
            self.last = (real if self.last is None else torch.cat([self.last, real], -1))[..., -(self.hop + 1):].clone()
        self.chunks += 1
        return self._step(xs)

    @torch.no_grad()
    def push(self, x_chunk: Tensor) -> Tensor:
        """x_chunk [B, channels, chunk * hop] -> y [B, speakers, chunk * hop]: the separated stream, one hop late"""
        xs = self._select(x_chunk)
        if tuple(xs.shape) != (self.B, self.M, self.C * self.hop):
            raise ValueError(f"push takes [{self.B}, {self.M}, {self.C * self.hop}] samples, got {tuple(xs.shape)}")
        return self._advance(xs, xs)

    @torch.no_grad()
    def finish(self, x_rest: Optional[Tensor] = None) -> Tensor:
        """the last step of a stream: the samples not pushed yet (`x_rest`: fewer than a chunk, a multiple of hop; default none), the right
        reflect padding x[N-2] .. x[N-hop-1], then zeros.  Returns a whole chunk: what lies past the end of the signal is the caller's to trim."""
        rest = self._select(x_rest) if x_rest is not None else None
        n = 0 if rest is None else rest.shape[-1]
        if n % self.hop or n > (self.C - 1) * self.hop:
            raise ValueError(f"finish takes a multiple of hop = {self.hop} samples below a chunk, got {n}")
        last = rest if self.last is None else (self.last if rest is None else torch.cat([self.last, rest], -1))
        if last is None or last.shape[-1] < self.hop + 1:
            raise ValueError(f"a stream must hold at least hop + 1 = {self.hop + 1} samples")
        last = last[..., -(self.hop + 1):]
        xs = torch.zeros(self.B, self.M, self.C * self.hop, dtype=torch.float32, device=last.device)
        if n:
            xs[..., :n] = rest
        xs[..., n:n + self.hop] = last[..., :self.hop].flip(-1)
        return self._advance(xs, rest if rest is not None else xs[..., :0])

    def _reset_io(self) -> None:
        self.primed, self.last, self.chunks = False, None, 0

    @torch.no_grad()
    def separate(self, x: Tensor) -> Tensor:
        """a whole signal through the stream: x [B, channels, N] (N a multiple of hop) -> y [B, speakers, N]"""
        N, step = x.shape[-1], self.C * self.hop
        if N % self.hop or N < 2 * self.hop:
            raise ValueError(f"separate takes a multiple of hop = {self.hop} samples, two hops at least; got {N}")
        self.reset()
        nfull = N // step
        ys = [self.push(x[..., k * step:(k + 1) * step]) for k in range(nfull)]
        ys.append(self.finish(x[..., nfull * step:] if N > nfull * step else None))
        return torch.cat(ys, -1)[..., self.hop:self.hop + N]


class NativeWaveStreamer(NativeOnlineStreamer, _WaveIO):
    """NativeWaveStreamer(net, batch, chunk, stft, norm_mode, channels, ref_channel): push / finish / reset / separate / latency_samples.
    One step = nbss_online_stft_step -> NativeOnlineStreamer's launches -> nbss_online_istft_step, captured as one HIP graph."""

    def __init__(self, net, batch: int, chunk: int, stft, norm_mode="frequency", channels: Optional[Sequence[int]] = None, ref_channel: Optional[int] = None,
                 device=None, use_graph: Optional[bool] = None, lib: Optional[Lib] = None):
        if not 2 <= chunk <= 32:
            raise NotImplementedError(_WHAT + f"2..32 frames per chunk (got {chunk}): frame 0's reflect padding needs sample x[hop], which a one-frame first "
                                      "chunk does not hold; the native step keeps at most 32 frames")
        _check_stft(stft)
        if not stft.hip_ok:
            raise NotImplementedError(_WHAT + f"the native STFT kernels cover n_fft 256 and 512 (got {stft.n_fft})")
        self.norm = norm_kind(norm_mode)
        NativeOnlineStreamer.__init__(self, net, batch, chunk, device=device, use_graph=use_graph, lib=lib)  # (refuses what supported() rejects)
        self._init_io(batch, chunk, stft, channels, ref_channel, self.din)
        self.S = self.dout // 2
        self.tables = ops.stft_tables(self.lib, self.n_fft, 0 if stft.win == "hann_window" else 1, self.dev)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.dev)  # noqa: E731
        self.xw, self.yw = z(batch, self.M, chunk * self.hop), z(batch, self.S, chunk * self.hop)
        self.tail, self.ola = z(batch, self.M, self.hop), z(batch, self.S, self.hop)
        xr = {NBSS_ONLINE_NORM_NONE: None, NBSS_ONLINE_NORM_FREQUENCY: (batch, self.F, chunk), NBSS_ONLINE_NORM_UTTERANCE: (batch, 1, chunk)}[self.norm]
        self.xrmm = z(*xr) if xr is not None else None
        self.mag = z(batch, self.F, chunk) if self.norm == NBSS_ONLINE_NORM_UTTERANCE else None
        if self.F != self.n_fft // 2 + 1:
            raise ValueError(f"the network has {self.F} frequencies, n_fft {self.n_fft} gives {self.n_fft // 2 + 1}")

    def _buffers(self):
        return NativeOnlineStreamer._buffers(self) + [self.tail, self.ola]

    def _run(self) -> None:
        lib, P = self.lib, ops._ptr
        st = ops._stream(lib, self.xw)
        f = lambda t: P(lib, t, torch.float32)  # noqa: E731
        lib.call("nbss_online_stft_step", self.n_fft, self.norm, self.B, self.M, self.C, self.ref, f(self.tables), f(self.xw), f(self.tail), f(self.x),
                 f(self.xrmm), f(self.mag), st)
        NativeOnlineStreamer._run(self)
        lib.call("nbss_online_istft_step", self.n_fft, self.norm, self.B, self.S, self.C, f(self.tables), f(self.y), f(self.xrmm), f(self.ola), f(self.yw), st)

    @torch.no_grad()
    def reset(self) -> None:
        NativeOnlineStreamer.reset(self)
        self._reset_io()

    def _prime(self, left: Tensor) -> None:
        self.tail.copy_(left)  # (outside the graph; `ola` is zero after a reset)

    def _step(self, xs: Tensor) -> Tensor:
        self.xw.copy_(xs)
        self._replay()
        return self.yw.clone()

    def step(self, x_chunk: Tensor) -> Tensor:
        raise TypeError("NativeWaveStreamer takes samples: push(x_chunk) (feature frames go to NativeOnlineStreamer.step)")


class WaveStreamer(_WaveIO):
    """the same interface on torch ops: torch.fft.rfft / irfft on the framed `tail | chunk`, the online normalisation of models/io/norm.py, and the
    torch.nn step (models.arch.OnlineSpatialNet.OnlineStreamer; its HIP graph, when `use_graph`, covers the network only).  Any n_fft with
    n_hop = n_fft / 2, any chunk >= 2, any network OnlineStreamer takes; host or device tensors."""

    def __init__(self, net, batch: int, chunk: int, stft, norm_mode="frequency", channels: Optional[Sequence[int]] = None, ref_channel: Optional[int] = None,
                 device=None, use_graph: Optional[bool] = None, lib=None):
        from models.arch.OnlineSpatialNet import OnlineStreamer
        if chunk < 2:
            raise NotImplementedError(_WHAT + f"at least 2 frames per chunk (got {chunk}): frame 0's reflect padding needs sample x[hop], which a one-frame "
                                      "first chunk does not hold")
        _check_stft(stft)
        self.norm = norm_kind(norm_mode)
        self.net_step = OnlineStreamer(net, batch, chunk, device=device, use_graph=use_graph)  # (NotImplementedError for an unbounded state: 'mhsa(inf)')
        self.dev = self.net_step.dev
        self._init_io(batch, chunk, stft, channels, ref_channel, self.net_step.din)
        self.S = net.decoder.out_features // 2
        self.win = stft.window.detach().float().to(self.dev)
        self.env = self.win[:self.hop] ** 2 + self.win[self.hop:] ** 2
        self.tail = torch.zeros(batch, self.M, self.hop, device=self.dev)
        self.ola = torch.zeros(batch, self.S, self.hop, device=self.dev)

    @property
    def graph(self):
        return self.net_step.graph

    @torch.no_grad()
    def reset(self) -> None:
        self.net_step.reset()
        self.tail.zero_()
        self.ola.zero_()
        self._reset_io()

    def _prime(self, left: Tensor) -> None:
        self.tail.copy_(left)

    def _step(self, xs: Tensor) -> Tensor:
        B, M, C, hop = self.B, self.M, self.C, self.hop
        ext = torch.cat([self.tail, xs.to(self.dev)], -1)  # [B, M, (C + 1) hop]
        self.tail.copy_(ext[..., -hop:])
        X = torch.fft.rfft(ext.unfold(-1, self.n_fft, hop) * self.win, dim=-1).permute(0, 1, 3, 2)  # [B, M, F, C]
        mag = X[:, [self.ref]].abs()
        mm = None
        if self.norm == NBSS_ONLINE_NORM_FREQUENCY:
            mm = mag + 1e-6
        elif self.norm == NBSS_ONLINE_NORM_UTTERANCE:
            mm = mag.mean(dim=2, keepdim=True) + 1e-6
        if mm is not None:
            X = X / mm
        feats = torch.view_as_real(X.permute(0, 2, 3, 1).contiguous()).reshape(B, -1, C, 2 * M)
        out = self.net_step.step(feats)  # [B, F, C, 2S]
        Y = torch.view_as_complex(out.float().reshape(B, out.shape[1], C, self.S, 2).contiguous()).permute(0, 3, 1, 2)  # [B, S, F, C]
        if mm is not None:
            Y = Y * mm
        z = torch.fft.irfft(Y.permute(0, 1, 3, 2), n=self.n_fft, dim=-1) * self.win  # [B, S, C, n_fft]
        first, second = z[..., :hop], z[..., hop:]
        prev = torch.cat([self.ola[:, :, None], second[:, :, :-1]], 2)  # the second half of the frame before each frame
        self.ola.copy_(second[:, :, -1])
        return ((first + prev) / self.env).reshape(B, self.S, C * hop)


def open_wave_stream(net, batch: int, chunk: int, stft, norm_mode, channels, ref_channel, device=None, use_graph: Optional[bool] = None,
                     native: Optional[bool] = None):
    """NativeWaveStreamer on a HIP device when it serves the configuration (native=True: or raise its reason), else WaveStreamer"""
    dev = torch.device(device) if device is not None else net.decoder.weight.device
    if native is not False and (dev.type == "cuda" or native):
        try:
            return NativeWaveStreamer(net, batch, chunk, stft, norm_mode, channels, ref_channel, device=dev, use_graph=use_graph)
        except NotImplementedError:
            if native:
                raise
    return WaveStreamer(net, batch, chunk, stft, norm_mode, channels, ref_channel, device=dev, use_graph=use_graph)
