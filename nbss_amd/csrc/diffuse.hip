// diffuse.hip — spatially diffuse noise of the on-device simulator (utils/diffuse_noise.py:64-93; data_loaders/gpu_simulation.py: gen_diffuse_noise):
// M independent noises -> mean removal -> STFT (nfft 256, periodic Hann, hop nfft/4, scipy's zero padding) -> one M x M complex mix per bin
// -> inverse STFT (window, overlap-add, division by the window envelope, trim), fused: `white` is read once, `noise` written once, nothing of size
// B M N in between.  The definition is the one of include/nbss_hip.h.
//
//   diffuse_tables_kernel  the windowed DFT matrices as MFMA A fragments and the window, into the workspace (every call: 131 328 floats).
//                          The real transform has nfft real rows: q = 0 is Re bin 0, q = 1 is Re bin nfft/2 (it sits where Im bin 0 would: the
//                          imaginary parts of the two edge bins of a real signal are zero going in and ignored coming out), q = 2 f + ri for the others.
//                              D[q][j] = w[j] cos | -sin (2 pi f j / nfft)                   forward, rows q, K = j
//                              E[j][q] = w[j] c_q / nfft cos | -sin (2 pi f j / nfft)        inverse, rows j, K = q, c_q = 1 for q < 2, else 2
//                          so both transforms are nfft x nfft GEMMs against 16 frames of M channels (v_mfma_f32_16x16x4_f32: exact fp32 products).
//   diffuse_mean_kernel    one workgroup per row (b, m): the mean over N in fp64, thread t sums n = t, t + 256, ... in rising order, then an LDS tree.
//   diffuse_noise_kernel   a workgroup (4 waves) owns one item, DN_STRIP = 13 hops = 832 output samples and all M channels: the 16 frames that touch
//                          them (frames 13 k - 1 .. 13 k + 14 for strip k: three frames of halo in front; frames < 0 or >= T do not exist and are zeroed
//                          after the mix).  LDS image, floats:
//                              XS[M][19][68]    the strip (19 hops of 64 samples, rows padded to 68 words: frame li starts 68 li words in, the 16 frames
//                                               of a B fragment fall into distinct banks), white minus the row mean (subtracted in fp64), zeros outside
//                                               [0, N); after the transforms the same memory is the overlap-add image of the strip
//                              XB[4][M][64][4]  the mixed spectra of the four row tiles of a step, in the lanes' own fragment order
//                          9 264 M bytes: 54.3 KB at M = 6, 144.8 KB at M = 16 (above 64 KB the dynamic LDS limit is raised).
//                          Four steps; in step s wave w transforms row tile Q = 4 s + w: 64 K steps over j (lane group kk owns j = 64 kk .. 64 kk + 63, a
//                          16-byte LDS read and a 16-byte table read per 4 K steps), M accumulators; the mix X[n] = sum_m conj(Cs[f][m][n]) Nf[m] is
//                          lane-local (a lane holds (re, im) of two bins of one frame for every channel), rising m; X goes to XB.  After a barrier every
//                          wave multiplies its four row tiles j = 16 (w + 4 d) .. + 15, d = 0 .. 3, of E with the step's four X tiles: 4 M accumulators
//                          that live across the steps.  A lane's X fragment is its own accumulator: K = q needs no transposition.
//                          Overlap-add: wave w holds, for every frame, the samples j = 64 d + 16 w + (0 .. 15): all four frames that reach an output
//                          sample are in the same wave, which adds them into XS in the order d = 0, 1, 2, 3 (barriers in between).  Then the envelope
//                          sum_t w^2[p - 64 t] over the frames that exist, the division, and contiguous stores.
// The order of every sum is fixed by N and M alone: j within a K step as the MFMA chains it (kk = 0 .. 3), K steps rising, m rising, q rising, frames from
// the latest to the earliest.  No atomics, every output is stored exactly once, two calls give the same bits, an item does not depend on its batch.
#include "launch.h"
#include "layout.h"
#include "conv_common.h"

#define DN_THREADS 256
#define DN_PI 3.14159265358979323846
#define DN_MAX_M 16
#define DN_MAX_N (1 << 24)
#define DN_MAX_ROWS (1 << 22)  // B M
#define DN_MAX_ITEMS 128       // items per grid pass; a workgroup walks the others in steps of the grid

// geometry of one transform size; the kernel's wave <-> tile mapping (4 waves x 4 row tiles, 4 frames per output sample) is that of TILES == 16
template <int NFFT>
struct DiffuseGeom {
    static constexpr int nfft = NFFT, hop = NFFT / 4, F = NFFT / 2 + 1;
    static constexpr int TILES = NFFT / 16;            // row tiles of both GEMMs
    static constexpr int KS4 = NFFT / 16;              // forward: groups of 4 K steps (4 lane groups x 4 samples each)
    static constexpr int FRAMES = 16;                  // frames of a workgroup: the MFMA's columns
    static constexpr int OUT_HOPS = FRAMES - 3;        // hops that get all their frames from the workgroup's own
    static constexpr int IN_HOPS = FRAMES + 3;         // hops the frames span
    static constexpr int HS = hop + 4;                 // LDS row of one hop, in floats
    static constexpr int STRIP = OUT_HOPS * hop;       // output samples per workgroup
    static constexpr int TAB = NFFT * NFFT;            // floats of one packed matrix
};
typedef DiffuseGeom<256> DG;
static_assert(DG::TILES == 16 && DG::hop == 64, "the wave <-> tile mapping of diffuse_noise_kernel");
static_assert((DG::HS * 4) % 16 == 0, "16-byte LDS rows");

static size_t dn_table_floats() { return (size_t)DG::nfft + 2 * (size_t)DG::TAB; }  // [w][D pack][E pack]; a multiple of 2: the fp64 means follow

NBSS_DEV double dn_win(int j) { return 0.5 - 0.5 * cos(2.0 * DN_PI * j / DG::nfft); }  // periodic Hann

NBSS_DEV float dn_coeff(int q, int j, bool inverse) {
    const int f = q == 0 ? 0 : (q == 1 ? DG::nfft / 2 : q >> 1), ri = q < 2 ? 0 : (q & 1);
    const double ang = 2.0 * DN_PI * (double)((f * j) % DG::nfft) / DG::nfft;
    const double v = dn_win(j) * (ri == 0 ? cos(ang) : -sin(ang));
    return (float)(inverse ? v * (q < 2 ? 1.0 : 2.0) / DG::nfft : v);
}

// D pack [Q][ks4][lane][e]: row q = 16 Q + li, j = 64 kk + 4 ks4 + e;  E pack [J][Q][lane][e]: row j = 16 J + li, q = 16 Q + 4 kk + e
__global__ void diffuse_tables_kernel(float* __restrict__ tab) {
    const int total = DG::nfft + 2 * DG::TAB;
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < total; i += (int)(gridDim.x * blockDim.x)) {
        if (i < DG::nfft) {
            tab[i] = (float)dn_win(i);
            continue;
        }
        int r = i - DG::nfft;
        const bool inverse = r >= DG::TAB;
        if (inverse) r -= DG::TAB;
        const int e = r & 3, lane = (r >> 2) & 63, li = lane & 15, kk = lane >> 4, inner = (r >> 8) & 15, outer = r >> 12;
        tab[i] = inverse ? dn_coeff(16 * inner + 4 * kk + e, 16 * outer + li, true) : dn_coeff(16 * outer + li, 64 * kk + 4 * inner + e, false);
    }
}

__global__ __launch_bounds__(DN_THREADS) void diffuse_mean_kernel(int rows, int N, const float* __restrict__ white, double* __restrict__ mean) {
    NBSS_LDS(smem);
    double* sd = reinterpret_cast<double*>(smem);  // [256]
    const int tid = (int)threadIdx.x;
    for (int row = (int)blockIdx.x; row < rows; row += (int)gridDim.x) {
        const float* x = white + (size_t)row * (size_t)N;
        double s = 0.0;
        for (int n = tid; n < N; n += DN_THREADS) s += (double)x[n];
        sd[tid] = s;
        __syncthreads();
        for (int half = DN_THREADS / 2; half >= 1; half >>= 1) {
            if (tid < half) sd[tid] += sd[tid + half];
            __syncthreads();
        }
        if (tid == 0) mean[row] = sd[0] / (double)N;
        __syncthreads();
    }
}

template <int M>
__global__ __launch_bounds__(DN_THREADS) void diffuse_noise_kernel(int B, int N, int T, const float* __restrict__ white, const float* __restrict__ Cs,
                                                                   const float* __restrict__ tab, const double* __restrict__ mean, float* __restrict__ noise) {
    constexpr int HS = DG::HS, IN_HOPS = DG::IN_HOPS, HOP = DG::hop, ROW = IN_HOPS * HS;
    NBSS_LDS(smem);
    float* XS = reinterpret_cast<float*>(smem);            // [M][IN_HOPS][HS]
    f32x4* XB = reinterpret_cast<f32x4*>(XS + M * ROW);    // [4][M][64]; 16-byte aligned: ROW floats are a multiple of 16 bytes
    const float* win = tab;
    const f32x4* Dp = reinterpret_cast<const f32x4*>(tab + DG::nfft);
    const f32x4* Ep = Dp + DG::TAB / 4;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = wave_id_u();
    const int li = lane & 15, kk = lane >> 4;
    const int strip = (int)blockIdx.x;
    const int tb = DG::OUT_HOPS * strip - 1;               // the first frame of the workgroup
    const int i0 = DG::STRIP * strip;                      // its first output sample
    const bool frame_ok = tb + li >= 0 && tb + li < T;
    for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
        __syncthreads();  // the previous item's readers are done
        // ---- stage the strip: padded sample p = 64 (tb + h) + c is white[p - nfft/2] - mean inside [0, N), zero outside
        for (int e = tid; e < M * IN_HOPS * HOP; e += DN_THREADS) {
            const int m = e / (IN_HOPS * HOP), r = e - m * (IN_HOPS * HOP), h = r / HOP, c = r - h * HOP;
            const int i = HOP * (tb + h) + c - DG::nfft / 2;
            float v = 0.f;
            if (i >= 0 && i < N) v = (float)((double)white[((size_t)b * M + m) * (size_t)N + i] - mean[b * M + m]);
            XS[m * ROW + h * HS + c] = v;
        }
        __syncthreads();
        f32x4 acc[4][M];
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int n = 0; n < M; ++n) acc[d][n] = F32X4_ZERO;

#pragma unroll 1
        for (int s = 0; s < 4; ++s) {
            // ---- forward: row tile Q of D against the 16 frames of every channel
            const int Q = 4 * s + wv;
            f32x4 fa[M];
#pragma unroll
            for (int m = 0; m < M; ++m) fa[m] = F32X4_ZERO;
            {
                const f32x4* pa = Dp + (size_t)Q * DG::KS4 * 64 + lane;
                const float* pb = XS + (li + kk) * HS;
#pragma unroll 2
                for (int ks4 = 0; ks4 < DG::KS4; ++ks4) {
                    const f32x4 a = pa[ks4 * 64];
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const f32x4 x4 = *reinterpret_cast<const f32x4*>(pb + m * ROW + 4 * ks4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) fa[m] = conv_mfma(a[e], x4[e], fa[m]);
                    }
                }
            }
            // ---- mix: the lane holds rows q = 16 Q + 4 kk + (0 .. 3) of frame li: (re, im) of bins f0 and f0 + 1, or, for q = 0 and 1, Re of bins 0 and nfft/2
            {
                const int f0 = 8 * Q + 2 * kk;
                const bool edge = f0 == 0;
                const float* c0 = Cs + (size_t)(edge ? 0 : f0) * M * M * 2;
                const float* ce = Cs + (size_t)(DG::nfft / 2) * M * M * 2;
                const float* c1 = Cs + (size_t)(f0 + 1) * M * M * 2;
#pragma unroll
                for (int n = 0; n < M; ++n) {
                    f32x4 x = F32X4_ZERO;
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const f32x4 z = fa[m];
                        const f32x2 a = *reinterpret_cast<const f32x2*>(c0 + (m * M + n) * 2);
                        const f32x2 g = *reinterpret_cast<const f32x2*>(c1 + (m * M + n) * 2);
                        if (edge) {
                            const float ar = ce[(m * M + n) * 2];
                            x[0] += a[0] * z[0];
                            x[1] += ar * z[1];
                        } else {
                            x[0] += a[0] * z[0] + a[1] * z[1];  // conj(c) z = (cr zr + ci zi) + i (cr zi - ci zr)
                            x[1] += a[0] * z[1] - a[1] * z[0];
                        }
                        x[2] += g[0] * z[2] + g[1] * z[3];
                        x[3] += g[0] * z[3] - g[1] * z[2];
                    }
                    XB[(wv * M + n) * 64 + lane] = frame_ok ? x : F32X4_ZERO;
                }
            }
            __syncthreads();
            // ---- inverse: this wave's row tiles J = wv + 4 d of E against the step's four X tiles
#pragma unroll 2
            for (int qt = 0; qt < 4; ++qt) {
                f32x4 ea[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) ea[d] = Ep[((size_t)(wv + 4 * d) * DG::TILES + 4 * s + qt) * 64 + lane];
#pragma unroll
                for (int n = 0; n < M; ++n) {
                    const f32x4 x4 = XB[(qt * M + n) * 64 + lane];
#pragma unroll
                    for (int d = 0; d < 4; ++d)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[d][n] = conv_mfma(ea[d][e], x4[e], acc[d][n]);
                }
            }
            __syncthreads();  // XB is rewritten by the next step; after the last one XS is free
        }
        // ---- overlap-add: acc[d][n] holds samples j = 64 d + 16 wv + 4 kk + (0 .. 3) of frame li, i.e. hop li + d of the strip, columns 16 wv + 4 kk ...
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            const int h = li + d;
            if (h >= 3 && h < 3 + DG::OUT_HOPS) {
#pragma unroll
                for (int n = 0; n < M; ++n) {
                    f32x4* o = reinterpret_cast<f32x4*>(XS + n * ROW + h * HS + 16 * wv + 4 * kk);
                    *o = d == 0 ? acc[d][n] : *o + acc[d][n];
                }
            }
            __syncthreads();
        }
        // ---- envelope, division, store
        for (int e = tid; e < M * DG::STRIP; e += DN_THREADS) {
            const int n = e / DG::STRIP, r = e - n * DG::STRIP, i = i0 + r;
            if (i >= N) continue;
            const int h = 3 + r / HOP, c = r % HOP, u = tb + h;  // u: the hop of padded sample i + nfft/2
            float env = 0.f;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const float w = win[c + HOP * d];
                if (u - d >= 0 && u - d < T) env += w * w;
            }
            noise[((size_t)b * M + n) * (size_t)N + i] = XS[n * ROW + h * HS + c] / fmaxf(env, 1e-10f);
        }
    }
}

// ---------------- host side ----------------
size_t diffuse_noise_ws_bytes_impl(int B, int M) { return dn_table_floats() * sizeof(float) + (size_t)B * M * sizeof(double); }

template <int M>
static int dn_launch(dim3 grid, hipStream_t st, int B, int N, int T, const float* white, const float* Cs, const float* tab, const double* mean, float* noise) {
    const size_t lds = (size_t)M * (DG::IN_HOPS * DG::HS * sizeof(float) + 4 * 64 * sizeof(f32x4));
    if (lds > 64 * 1024) {
        int e = NBSS_SET_MAX_LDS((diffuse_noise_kernel<M>), lds);
        if (e) return e;
    }
    NBSS_LAUNCH((diffuse_noise_kernel<M>), grid, dim3(DN_THREADS), lds, st, B, N, T, white, Cs, tab, mean, noise);
    return NBSS_CHECK_LAUNCH();
}

int diffuse_noise_impl(int nfft, int B, int M, int N, const float* white, const float* Cs, float* ws, float* noise, hipStream_t st) {
    if (N < 1 || B < 1 || M < 1) return NBSS_EINVAL;
    if (nfft != DG::nfft || M > DN_MAX_M || N > DN_MAX_N || (int64_t)B * M > DN_MAX_ROWS) return NBSS_EUNSUPPORTED;
    {
        const char *w0 = (const char*)white, *n0 = (const char*)noise;
        const size_t bytes = (size_t)B * M * (size_t)N * sizeof(float);
        if (w0 < n0 + bytes && n0 < w0 + bytes) return NBSS_EINVAL;  // the output may not alias the input
    }
    float* tab = ws;
    double* mean = reinterpret_cast<double*>(ws + dn_table_floats());
    NBSS_LAUNCH(diffuse_tables_kernel, dim3(128), dim3(256), 0, st, tab);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    const int rows = B * M;
    NBSS_LAUNCH(diffuse_mean_kernel, dim3(rows < 4096 ? rows : 4096), dim3(DN_THREADS), DN_THREADS * sizeof(double), st, rows, N, white, mean);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    const int T = cdiv(N, DG::hop) + 1;  // frames of the padded signal: (Np - nfft) / hop + 1 with Np = N + nfft + (-N mod hop)
    const dim3 grid(cdiv(N, DG::STRIP), B < DN_MAX_ITEMS ? B : DN_MAX_ITEMS);
    switch (M) {
#define DN_CASE(m) case m: return dn_launch<m>(grid, st, B, N, T, white, Cs, tab, mean, noise);
        DN_CASE(1) DN_CASE(2) DN_CASE(3) DN_CASE(4) DN_CASE(5) DN_CASE(6) DN_CASE(7) DN_CASE(8)
        DN_CASE(9) DN_CASE(10) DN_CASE(11) DN_CASE(12) DN_CASE(13) DN_CASE(14) DN_CASE(15) DN_CASE(16)
#undef DN_CASE
    }
    return NBSS_EUNSUPPORTED;
}
