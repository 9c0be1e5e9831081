// online_io.hip — the waveform ends of the OnlineSpatialNet streaming step (nbss_amd/online_io.py: NativeWaveStreamer): samples in, samples
// out, one chunk of C frames per call, all state in caller-owned device buffers that a call updates in place (capturable in a HIP graph
// together with the network step of online.hip).  hop = n_fft/2, win_len = n_fft, the tables of nbss_stft_tables (signal.hip).
//
// Alignment.  Frame t of the stream is frame t of torch.stft(center=True): it covers the samples [(t-1) hop, (t+1) hop).  The C frames of a
// chunk are therefore cut from `tail | x_chunk` (tail = the hop samples before the chunk), and the overlap-add of frame t completes the
// samples [(t-1) hop, t hop): the sample stream leaves one hop late.  Neither kernel knows a first or a last chunk: the reflect padding of
// both ends of the signal is what the caller puts into `tail` before the first chunk and into the chunk after the last sample.
//
//   online_stft_kernel    one wave = (batch item, 16-frame tile, 16 rows q = (f, re|im) of the DFT, a share of the microphones): the DFT as a
//                         GEMM on the exact-f32 matrix cores with frames as the N dimension (as stft_norm_kernel), the rows AND the microphones
//                         dealt to waves of their own workgroups — a batch-1 chunk of 16 frames and 6 microphones is 102 waves of two
//                         dependent 16 x 256 x 16 products instead of 6 waves of 17 x 6
//   online_stft_finish    tail <- the last hop of the chunk (after every wave of the first kernel has read the old one), and for
//                         Norm('utterance', online=True) the per-frame mean over F of |X_ref|: folded in LDS in a fixed order (no float atomics)
//   online_istft_kernel   one wave = (batch item, speaker, 16 + 16 rows m and m + hop of the windowed inverse DFT): the lane that holds the first
//                         half of frame t fetches the second half of frame t - 1 from its neighbour lane (the previous tile's last frame, or
//                         `ola`, for the first lane), divides by the window envelope and writes the sample: one lane per sample, no atomics
#include "launch.h"
#include "layout.h"

struct OioGeom {
    int nfft, hop, F, MTq, KSm, MTm, KSq;
};
NBSS_HD OioGeom online_stft_geom(int nfft) {  // as signal.hip: stft_geom (the layout of the tables)
    OioGeom g;
    g.nfft = nfft; g.hop = nfft / 2; g.F = nfft / 2 + 1;
    g.MTq = cdiv(2 * g.F, 16); g.KSm = nfft / 32; g.MTm = nfft / 16; g.KSq = cdiv(2 * g.F, 32);
    return g;
}

#define OIO_NONE 0
#define OIO_FREQUENCY 1
#define OIO_UTTERANCE 2
#define OIO_CMAX 32

// grid = B * ntile * MTq * np workgroups of one wave.  x [B][M][C hop], tail [B][M][hop] (read only here), feats [B][F][C][2M];
// frequency: xrmm [B][F][C] = |X_ref| + 1e-6 and feats normalised; utterance: mag [B][F][C] = |X_ref|, feats left un-normalised (finish kernel)
template <int NFFT>
__global__ __launch_bounds__(64) void online_stft_kernel(int M, int C, int ref, int norm, int np, const float* __restrict__ tab,
                                                         const float* __restrict__ x, const float* __restrict__ tail, float* __restrict__ feats,
                                                         float* __restrict__ xrmm, float* __restrict__ mag) {
    constexpr int HOP = NFFT / 2, F = NFFT / 2 + 1, KSm = NFFT / 32, MTq = (2 * F + 15) / 16;
    const float* Dp = tab + NFFT;
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4;
    const int ntile = cdiv(C, 16);
    int task = (int)blockIdx.x;
    const int part = task % np;
    task /= np;
    const int mt = task % MTq;
    task /= MTq;
    const int st = task % ntile, b = task / ntile;
    const int t = st * 16 + l15;  // frame of the chunk in this lane's column (columns >= C of a partial tile are masked)
    Frag<float> a[KSm];
#pragma unroll
    for (int ks = 0; ks < KSm; ++ks) wfrag_load(a[ks], Dp, mt, KSm, ks);
    auto dft = [&](int m) {
        const float* xc = x + ((size_t)b * M + m) * C * HOP;
        const float* tl = tail + ((size_t)b * M + m) * HOP;
        f32x4 acc = F32X4_ZERO;
#pragma unroll
        for (int ks = 0; ks < KSm; ++ks) {
            Frag<float> bq;
            const int p0 = t * HOP + ks * 32 + 8 * g4;  // first of this lane's 8 samples inside tail | chunk (a run never straddles the two: 8 | hop)
            if (t < C) load8(p0 < HOP ? tl + p0 : xc + (p0 - HOP), bq.v);
            else frag_zero(bq);
            acc = mma(a[ks], bq, acc);
        }
        return acc;
    };
    // lane: frame t, rows q = 16 mt + 4 g4 + {0,1,2,3} = (f0,re) (f0,im) (f0+1,re) (f0+1,im)
    const int f0 = (16 * mt + 4 * g4) >> 1;
    float mm[2] = {1.f, 1.f};
    if (norm == OIO_FREQUENCY || (norm == OIO_UTTERANCE && part == 0)) {  // (wave-uniform)
        const f32x4 r = dft(ref);
        const float m0 = sqrtf(r[0] * r[0] + r[1] * r[1]), m1 = sqrtf(r[2] * r[2] + r[3] * r[3]);
        if (norm == OIO_FREQUENCY) {
            mm[0] = m0 + 1e-6f;
            mm[1] = m1 + 1e-6f;
        }
        if (part == 0 && t < C) {
            float* o = norm == OIO_FREQUENCY ? xrmm : mag;
            if (f0 < F) o[((size_t)b * F + f0) * C + t] = norm == OIO_FREQUENCY ? mm[0] : m0;
            if (f0 + 1 < F) o[((size_t)b * F + f0 + 1) * C + t] = norm == OIO_FREQUENCY ? mm[1] : m1;
        }
    }
    for (int m = part; m < M; m += np) {
        const f32x4 acc = dft(m);
        if (t < C) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int f = f0 + e;
                if (f < F) {
                    f32x2 v = {acc[2 * e] / mm[e], acc[2 * e + 1] / mm[e]};
                    *reinterpret_cast<f32x2*>(feats + (((size_t)b * F + f) * C + t) * (2 * M) + 2 * m) = v;
                }
            }
        }
    }
}

// blocks 0 .. nnorm-1 (utterance only, nnorm = B * C): frame (b, c): xrmm[b][c] = mean_f mag[b][f][c] + 1e-6, feats[b][:][c][:] /= it;
// the blocks behind them: tail[b][m][:] = x[b][m][(C-1) hop ..]
__global__ __launch_bounds__(256) void online_stft_finish_kernel(int B, int M, int C, int F, int hop, int nnorm, const float* __restrict__ x,
                                                                float* __restrict__ tail, float* __restrict__ feats, float* __restrict__ xrmm,
                                                                const float* __restrict__ mag) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [256]
    const int i = (int)threadIdx.x;
    if ((int)blockIdx.x < nnorm) {
        const int b = (int)blockIdx.x / C, c = (int)blockIdx.x % C;
        float s = 0.f;
        for (int f = i; f < F; f += 256) s += mag[((size_t)b * F + f) * C + c];
        red[i] = s;
        __syncthreads();
        for (int h = 128; h >= 1; h >>= 1) {  // a fixed tree: the same sum whatever the chunk size
            if (i < h) red[i] += red[i + h];
            __syncthreads();
        }
        const float mmv = red[0] / (float)F + 1e-6f;
        if (i == 0) xrmm[(size_t)b * C + c] = mmv;
        for (int e = i; e < F * 2 * M; e += 256) {
            const int f = e / (2 * M), k = e - f * 2 * M;
            float* o = feats + (((size_t)b * F + f) * C + c) * (2 * M) + k;
            *o = *o / mmv;
        }
        return;
    }
    const size_t total = (size_t)B * M * hop, stride = (size_t)(gridDim.x - nnorm) * 256;
    for (size_t e = (size_t)((int)blockIdx.x - nnorm) * 256 + i; e < total; e += stride) {
        const size_t bm = e / hop;
        tail[e] = x[bm * C * hop + (size_t)(C - 1) * hop + (e - bm * hop)];
    }
}

// grid = B * S * (NFFT / 32) workgroups of one wave.  out [B][F][C][2S], xrmm [B][F][C] (frequency) | [B][C] (utterance) | unused,
// ola [B][S][hop] = the windowed second half of the frame before the chunk (in: read first; out: of the chunk's last frame), y [B][S][C hop]
template <int NFFT>
__global__ __launch_bounds__(64) void online_istft_kernel(int S, int C, int norm, const float* __restrict__ tab, const float* __restrict__ out,
                                                          const float* __restrict__ xrmm, float* __restrict__ ola, float* __restrict__ y) {
    constexpr int HOP = NFFT / 2, F = NFFT / 2 + 1, MTm = NFFT / 16, HT = MTm / 2, KSq = (2 * F + 31) / 32;
    const OioGeom g = online_stft_geom(NFFT);
    const float* win = tab;
    const float* Ep = tab + NFFT + (size_t)2 * g.MTq * g.KSm * 512;
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4;
    int task = (int)blockIdx.x;
    const int mp = task % HT;  // row tiles mp (first half of a frame) and mp + HT (second half, the same offsets j)
    task /= HT;
    const int s = task % S, b = task / S;
    const int j0 = 16 * mp + 4 * g4;  // this lane's 4 offsets inside a hop
    float* olap = ola + ((size_t)b * S + s) * HOP + j0;
    float* yb = y + ((size_t)b * S + s) * C * HOP + j0;
    float carry[4], env[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        carry[r] = olap[r];
        // every sample lies under exactly two frames (hop = n_fft / 2): the window envelope is the same everywhere
        env[r] = win[j0 + r] * win[j0 + r] + win[j0 + r + HOP] * win[j0 + r + HOP];
    }
    const int ntile = cdiv(C, 16);
    for (int st = 0; st < ntile; ++st) {
        const int t = st * 16 + l15;
        f32x4 lo = F32X4_ZERO, hi = F32X4_ZERO;
#pragma unroll
        for (int ks = 0; ks < KSq; ++ks) {
            Frag<float> bq, a;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int f = (ks * 32 + 8 * g4) / 2 + e;
                float re = 0.f, im = 0.f;
                if (t < C && f < F) {
                    const size_t n = ((size_t)b * F + f) * C + t;
                    const float mmv = norm == OIO_FREQUENCY ? xrmm[n] : (norm == OIO_UTTERANCE ? xrmm[(size_t)b * C + t] : 1.0f);
                    const f32x2 v = *reinterpret_cast<const f32x2*>(out + n * (2 * S) + 2 * s);
                    re = v[0] * mmv;
                    im = v[1] * mmv;
                }
                bq.v[2 * e] = re;
                bq.v[2 * e + 1] = im;
            }
            wfrag_load(a, Ep, mp, KSq, ks);
            lo = mma(a, bq, lo);
            wfrag_load(a, Ep, mp + HT, KSq, ks);
            hi = mma(a, bq, hi);
        }
        const int last = (C - 1 - st * 16) < 15 ? (C - 1 - st * 16) : 15;  // column of the tile's last frame
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float prev = __shfl(hi[r], l15 > 0 ? lane - 1 : lane);  // second half of frame t - 1 (every lane takes part)
            o[r] = (lo[r] + (l15 > 0 ? prev : carry[r])) / env[r];
            carry[r] = __shfl(hi[r], (lane & 48) | last);
        }
        if (t < C) store4(yb + (size_t)t * HOP, o[0], o[1], o[2], o[3]);
    }
    if (l15 == 0) store4(olap, carry[0], carry[1], carry[2], carry[3]);
}

static bool oio_geom_ok(int n_fft, int C) { return (n_fft == 256 || n_fft == 512) && C >= 2 && C <= OIO_CMAX; }

extern "C" {

int nbss_online_stft_step(int n_fft, int norm, int B, int M, int C, int ref_channel, const float* tables, const float* x_chunk, float* tail,
                          float* feats, float* xrmm, float* ws, void* stream) {
    if (!tables || !x_chunk || !tail || !feats || B <= 0 || M <= 0 || C <= 0 || ref_channel < 0 || ref_channel >= M) return NBSS_EINVAL;
    if (norm != OIO_NONE && norm != OIO_FREQUENCY && norm != OIO_UTTERANCE) return NBSS_EINVAL;
    if ((norm != OIO_NONE && !xrmm) || (norm == OIO_UTTERANCE && !ws)) return NBSS_EINVAL;
    if (!oio_geom_ok(n_fft, C)) return NBSS_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const OioGeom g = online_stft_geom(n_fft);
    const long tiles = (long)B * cdiv(C, 16) * g.MTq;
    if (tiles * M >= (1L << 30)) return NBSS_EUNSUPPORTED;
    // microphones of a (tile, rows) task dealt to np waves, until the launch has a wave per compute unit
    int np = 1;
    while (np < M && tiles * np < 256) ++np;
    const dim3 grid((unsigned)(tiles * np));
    if (n_fft == 256) NBSS_LAUNCH((online_stft_kernel<256>), grid, dim3(64), 0, st, M, C, ref_channel, norm, np, tables, x_chunk, (const float*)tail, feats, xrmm, ws);
    else NBSS_LAUNCH((online_stft_kernel<512>), grid, dim3(64), 0, st, M, C, ref_channel, norm, np, tables, x_chunk, (const float*)tail, feats, xrmm, ws);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    const long nnorm = norm == OIO_UTTERANCE ? (long)B * C : 0;
    const long tb = ((long)B * M * g.hop + 255) / 256;
    if (nnorm >= (1L << 30)) return NBSS_EUNSUPPORTED;
    NBSS_LAUNCH(online_stft_finish_kernel, dim3((unsigned)(nnorm + (tb < 64 ? tb : 64))), dim3(256), 256 * sizeof(float), st, B, M, C, g.F, g.hop, (int)nnorm, x_chunk, tail, feats,
                xrmm, (const float*)ws);
    return NBSS_CHECK_LAUNCH();
}

int nbss_online_istft_step(int n_fft, int norm, int B, int S, int C, const float* tables, const float* out, const float* xrmm, float* ola,
                           float* y_chunk, void* stream) {
    if (!tables || !out || !ola || !y_chunk || B <= 0 || S <= 0 || C <= 0) return NBSS_EINVAL;
    if (norm != OIO_NONE && norm != OIO_FREQUENCY && norm != OIO_UTTERANCE) return NBSS_EINVAL;
    if (norm != OIO_NONE && !xrmm) return NBSS_EINVAL;
    if (!oio_geom_ok(n_fft, C)) return NBSS_EUNSUPPORTED;
    const long nwg = (long)B * S * (n_fft / 32);
    if (nwg >= (1L << 30)) return NBSS_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (n_fft == 256) NBSS_LAUNCH((online_istft_kernel<256>), dim3((unsigned)nwg), dim3(64), 0, st, S, C, norm, tables, out, xrmm, ola, y_chunk);
    else NBSS_LAUNCH((online_istft_kernel<512>), dim3((unsigned)nwg), dim3(64), 0, st, S, C, norm, tables, out, xrmm, ola, y_chunk);
    return NBSS_CHECK_LAUNCH();
}

}  // extern "C"
