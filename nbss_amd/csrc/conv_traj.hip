// conv_traj.hip — time-varying FIR convolution for moving sources: a trajectory of P room impulse responses, one per `hop` source samples, switched
// (mode 0, utils/mix.py:151-194 convolve_traj) or cross-faded with a trapezium window (mode 1, mix.py:197-244 convolve_traj_with_win), cut at the
// direct-path delay.  The definition is the one of include/nbss_hip.h: with H = hop[b][s], d = delay[b][s] and j = n + d - k,
//   y[b][s][m][n] = sum_{k < L} sum_p w_p(j) h[b][s][p][m][k] x[b][s][j],   terms with j outside [0, N) are zero,
//   mode 0: w_p(j) = [j / H == p];   mode 1: w_q(j) = down(r), w_{q+1}(j) = up(r) for q = j / H, r = j % H (z = (H - ramp) / 2, o = H - ramp - z):
//   up(r) = 0 | (r - z) / (ramp - 1) | 1 on r < z | < z + ramp | else;   down(r) = 1 | (ramp - 1 - (r - o)) / (ramp - 1) | 0 on r < o | < o + ramp | else.
//
// For a fixed point p the inner sum is a static convolution of h[p] with xw_p = x w_p, which is zero outside the point's support
//   mode 0: [p H, (p + 1) H);   mode 1: [(p - 1) H + z + 1, p H + o + ramp - 1)   (H + ramp samples, one more when H - ramp is odd),
// so the kernel is fir_convolve_kernel's blocked Hankel product (conv1d.hip; v_mfma_f32_16x16x4_f32) run once per point that an output tile can hear:
//   a workgroup (4 waves) owns one (b, s), TRAJ_NT = 256 outputs [n0, n0 + 256) (ONE MFMA tile) and MB microphones.  The source range of the tile is
//   [n0 + d - L + 1, n0 + 255 + d]; the points whose support meets it are walked in rising p.  For each, the taps that can meet the support from the tile,
//   k in [n0 + d - (b - 1), n_last + d - a] for the clipped support [a, b), are walked in chunks of 2048 from the first such tap rounded down to a multiple
//   of 16; per chunk the workgroup stages HT (the tap blocks of h[p] transposed, zero columns around, as conv1d.hip) and XS (the strip of x TIMES w_p, zero
//   outside [a, b)), and the K steps of the chunk are split over the four waves in contiguous quarters, all four accumulating the same 256 outputs.
//   The tile is small because the zero padding per point grows with the tile: a point costs 256 + H + ramp taps for H + ramp useful ones
//   (H = 1000: 1.36 x the useful products at L = 3200, where 2048 outputs per workgroup would pay 5 x), plus the 30 zero blocks of a Hankel chunk.
//   After the last point the waves' partial sums meet in LDS (over the HT image) and wave 0 adds them in the order ((w0 + w1) + w2) + w3 and stores.
// x w_p is rounded once to fp32 when the strip is staged; its product with a tap is fused into the MFMA's fp32 fmaf chain, so every product of the sum is
// rounded once.  The order of an output's sum is point, chunk, wave quarter, K step, residue, MFMA column: fixed by n, L, H and d of its item alone.  No
// atomics; every output is stored exactly once; two calls give the same bits; an item does not depend on the batch it shares a launch with; no workspace.
// A response p is read only if some x[j] w_p(j) != 0 lies in the tile's source range, so surplus responses (and, with exactly the required P, the index P
// that only up(0) = 0 would reach) are never read.  Items are validated on the device: H < 1, in mode 1 H <= ramp or ramp < 2, or too few responses for
// this H give zeros; a delay outside [0, L) is clamped; both set the status word (a plain store of 1 by thread 0 of the workgroups that meet it).
#include "launch.h"
#include "layout.h"
#include "conv_common.h"

#define TRAJ_NT 256                          // outputs per workgroup: one MFMA tile, 16 rows i x 16 columns c
#define TRAJ_XS (16 * (4 * CONV_TMAX - 1) + 36)  // strip in floats, a multiple of 4: one tile reads up to li + 15 + 16 w_max + the alignment remainder = 33 + 16 w_max

static_assert(TRAJ_XS % 4 == 0, "the strip is staged in 16-byte pieces");
static_assert(3 * TRAJ_NT <= 16 * CONV_HS, "the partial sums of waves 1..3 lie over the HT image of as many microphones");

struct TrajWin {  // the window of one item
    int mode, H, ramp, z, o;
};

// w_p at the source sample c0 + t, c0 = p H, for a sample inside the point's support: t in [0, H) is heard through down, t in [-H, 0) through up
NBSS_DEV float traj_weight(const TrajWin& w, int t) {
    if (w.mode == 0) return 1.f;
    if (t >= 0) return t < w.o ? 1.f : (float)(w.ramp - 1 - (t - w.o)) / (float)(w.ramp - 1);
    const int r = t + w.H;
    return r >= w.z + w.ramp ? 1.f : (float)(r - w.z) / (float)(w.ramp - 1);
}

template <int MB, bool VEC>
__global__ __launch_bounds__(CONV_THREADS) void fir_convolve_traj_kernel(int BS, int P, int M, int N, int L, int mode, int ramp, const float* __restrict__ x,
                                                                         const float* __restrict__ h, const int32_t* __restrict__ hop,
                                                                         const int32_t* __restrict__ delay, float* __restrict__ y,
                                                                         int32_t* __restrict__ status) {
    NBSS_LDS(smem);
    float* HT = reinterpret_cast<float*>(smem);      // [MB][16][CONV_HS]; after the last point RED [3][MB][4][64]
    float* XS = HT + MB * 16 * CONV_HS;              // [TRAJ_XS], 16-byte aligned: 16 CONV_HS floats are a multiple of 16 bytes
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = wave_id_u();
    const int li = lane & 15, kk = lane >> 4;
    const int n0 = (int)blockIdx.x * TRAJ_NT, m0 = (int)blockIdx.y * MB;
    const int nlast = (n0 + TRAJ_NT < N ? n0 + TRAJ_NT : N) - 1;  // the tile's last output; n0 < N by the grid
    for (int bs = (int)blockIdx.z; bs < BS; bs += (int)gridDim.z) {
        TrajWin win;
        win.mode = mode, win.H = hop[bs], win.ramp = ramp;
        const int H = win.H;
        bool bad = H < 1 || (mode == 1 && (ramp < 2 || H <= ramp));
        if (!bad) {  // responses this H needs: mode 0 ceil(N / H), mode 1 ceil((N + H - 1) / H)
            const long long need = mode == 0 ? ((long long)N + H - 1) / H : ((long long)N + 2LL * H - 2) / H;
            bad = (long long)P < need;
        }
        if (bad) {  // workgroup-uniform
            if (tid == 0 && status) status[0] = 1;
            const int n = n0 + tid;
            if (n < N)
                for (int m = 0; m < MB && m0 + m < M; ++m) y[((size_t)bs * M + m0 + m) * (size_t)N + n] = 0.f;
            continue;
        }
        int d = delay[bs];
        if (d < 0 || d >= L) {
            if (tid == 0 && status) status[0] = 1;
            d = d < 0 ? 0 : L - 1;
        }
        win.z = mode == 1 ? (H - ramp) / 2 : 0;
        win.o = mode == 1 ? H - ramp - win.z : H;
        const float* xrow = x + (size_t)bs * (size_t)N;
        f32x4 acc[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m] = F32X4_ZERO;

        // the source samples the tile hears, and the points that weigh any of them
        const int jlo = n0 + d - L + 1 > 0 ? n0 + d - L + 1 : 0, jhi = nlast + d < N - 1 ? nlast + d : N - 1;
        int plast = jhi / H + (mode == 1 ? 1 : 0);
        if (plast > P - 1) plast = P - 1;  // taken with exactly the required P when (N - 1) % H == 0 in mode 1: the index P would have an empty support anyway
        for (int p = jlo / H; p <= plast; ++p) {
            const long long c0 = (long long)p * H;
            long long sa = mode == 0 ? c0 : c0 - H + win.z + 1, sb = mode == 0 ? c0 + H : c0 + win.o + ramp - 1;
            if (sa < jlo) sa = jlo;
            if (sb > (long long)jhi + 1) sb = (long long)jhi + 1;
            if (sa >= sb) continue;                   // workgroup-uniform, as everything that steers the loops
            const int a = (int)sa, b = (int)sb;       // the support [a, b), inside [0, N)
            const int klo = n0 + d - (b - 1) > 0 ? n0 + d - (b - 1) : 0, khi = nlast + d - a < L - 1 ? nlast + d - a : L - 1;
            const float* hrow = h + (((size_t)bs * P + p) * M + m0) * (size_t)L;
            for (int k0 = klo & ~15; k0 <= khi; k0 += CONV_KT) {
                const int left = khi + 1 - k0;
                const int qn = left >= CONV_KT ? CONV_QMAX : (left + 15) >> 4;  // tap blocks of this chunk
                const int T = (qn + 15 + 3) >> 2, wmax = 4 * T - 1;
                // the strip: x indices from g = n0 - k0 + 225 - 16 wmax + d, staged from g4 = g rounded down to a multiple of 4
                const int g = n0 - k0 + 225 - 16 * wmax + d, g4 = g & ~3, oa = g - g4;
                const int xlen = 16 * wmax + 36;            // <= TRAJ_XS, a multiple of 4: the last word read is 33 + 16 wmax
                __syncthreads();                            // the previous chunk's (or item's) readers are done
                conv_stage_taps<MB, VEC>(HT, hrow, m0, M, L, k0, qn, tid);
                // ---- stage the strip of x w_p: zero outside the support [a, b) (a select, not a product with 0)
                if (VEC) {
                    for (int s4 = tid * 4; s4 < xlen; s4 += CONV_THREADS * 4) {
                        const int gi = g4 + s4;  // a multiple of 4, as N is: the piece is inside or outside [0, N) as a whole
                        f32x4 t = F32X4_ZERO;
                        if (gi + 3 >= a && gi < b) {  // a >= 0 and b <= N: such a piece lies inside [0, N)
                            const f32x4 xv = *reinterpret_cast<const f32x4*>(xrow + gi);
#pragma unroll
                            for (int e4 = 0; e4 < 4; ++e4)
                                if (gi + e4 >= a && gi + e4 < b) t[e4] = xv[e4] * traj_weight(win, (int)((long long)(gi + e4) - c0));
                        }
                        *reinterpret_cast<f32x4*>(XS + s4) = t;
                    }
                } else {
                    for (int s1 = tid; s1 < xlen; s1 += CONV_THREADS) {
                        const int gi = g4 + s1;
                        XS[s1] = (gi >= a && gi < b) ? xrow[gi] * traj_weight(win, (int)((long long)gi - c0)) : 0.f;
                    }
                }
                __syncthreads();
                // ---- the products of this wave's quarter of the K steps.  A: HT[m][r][li + kk + 4 t]; B: XS[li + 15 + 16 (wmax - kk - 4 t) - r + oa]
                {
                    const int per = (T + 3) >> 2, tb = wv * per, te = tb + per < T ? tb + per : T;
                    const float* pa = HT + li + kk + 4 * tb;
                    const float* pb = XS + li + 15 + 16 * (wmax - kk) + oa - 64 * tb;
                    for (int t = tb; t < te; ++t) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            float av[MB];
#pragma unroll
                            for (int m = 0; m < MB; ++m) av[m] = pa[(m * 16 + r) * CONV_HS];
                            const float bv = pb[-r];
#pragma unroll
                            for (int m = 0; m < MB; ++m) acc[m] = conv_mfma(av[m], bv, acc[m]);
                        }
                        pa += 4;
                        pb -= 64;
                    }
                }
            }
        }
        // ---- the four partial sums: waves 1..3 hand theirs over through LDS, wave 0 adds them in a fixed order
        __syncthreads();  // the last chunk's readers are done
        if (wv > 0) {
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) HT[(((wv - 1) * MB + m) * 4 + j) * 64 + lane] = acc[m][j];
        }
        __syncthreads();
        // ---- D[i = 4 kk + j][c = li] -> y[n0 + 16 i + c]
        if (wv == 0) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (m0 + m >= M) break;
                float* yrow = y + ((size_t)bs * M + m0 + m) * (size_t)N;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v = acc[m][j];
#pragma unroll
                    for (int w = 0; w < 3; ++w) v += HT[((w * MB + m) * 4 + j) * 64 + lane];
                    const int n = n0 + 16 * (4 * kk + j) + li;
                    if (n < N) yrow[n] = v;
                }
            }
        }
    }
}

// ---------------- host side ----------------
int fir_convolve_traj_impl(int B, int S, int P, int M, int N, int L, int mode, int ramp, const float* x, const float* h, const int32_t* hop, const int32_t* delay,
                           float* y, int32_t* status, hipStream_t st) {
    if (N < 1 || L < 1 || P < 1 || mode < 0 || mode > 1) return NBSS_EINVAL;
    if (B < 1 || S < 1 || M < 1) return NBSS_EUNSUPPORTED;
    if (L > CONV_MAX_L || M > CONV_MAX_M || N > CONV_MAX_N || (int64_t)B * S * P * M > CONV_MAX_ROWS) return NBSS_EUNSUPPORTED;
    const int BS = B * S;
    const int MB = conv_mic_group(M);
    const dim3 grid(cdiv(N, TRAJ_NT), cdiv(M, MB), BS < CONV_MAX_ITEMS ? BS : CONV_MAX_ITEMS);
    const size_t lds = ((size_t)MB * 16 * CONV_HS + TRAJ_XS) * sizeof(float);  // 39.3 KB at MB = 3: four workgroups share a CU's 160 KB
    return conv_dispatch(MB, conv_vec(N, L, x, h), [&](auto mb, auto vec) {
        NBSS_LAUNCH((fir_convolve_traj_kernel<decltype(mb)::value, decltype(vec)::value>), grid, dim3(CONV_THREADS), lds, st, BS, P, M, N, L, mode, ramp, x, h, hop,
                    delay, y, status);
        return NBSS_CHECK_LAUNCH();
    });
}
