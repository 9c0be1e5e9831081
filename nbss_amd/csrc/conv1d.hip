// conv1d.hip — FIR convolution of dry sources with room impulse responses, cut at the direct-path delay (utils/mix.py:122-134, align=True), and the
// delay itself.  The definition is the one of include/nbss_hip.h:
//   y[b][s][m][n] = sum_k h[b][s][m][k] x[b][s][n + d - k],  d = delay[b][s],  terms with an x index outside [0, N) are zero.
//
//   rir_delay_kernel     one workgroup per (b, s): index of the maximum of h[b][s][ref][:], the lowest index on a tie.  Thread t scans k = t, t + 256, ...
//                        in rising order and keeps (value, index) under `>`; the 256 candidates meet in an LDS tree that prefers the lower index.
//   fir_convolve_kernel  a direct convolution as a blocked Hankel product on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32).  With xs(p) = x[p + d],
//                        an output tile of 256 samples n = nb + 16 i + c and the taps k = k0 + 16 q + r of a chunk:
//                            y[nb + 16 i + c] += sum_r sum_u A_r[i][u] B_r[u][c],   u = q - i,
//                            A_r[i][u] = h[k0 + 16 (i + u) + r]   (zero when i + u is no tap block of the chunk),
//                            B_r[u][c] = xs(nb - k0 + c - 16 u - r),
//                        one 16 x 16 product per residue r whose K dimension walks the tap blocks.  The x index does not depend on the row i, so the
//                        256 outputs of a tile share one strip of x; the triangles i + u < 0 and i + u >= blocks cost 30 zero blocks per CHUNK of
//                        128 tap blocks (2048 taps), not one per tap block: 12 % more MFMA work than useful at a full chunk, where the Toeplitz form
//                        (16 outputs x 16 taps per tile, 31 of 32 K columns) pays 100 %.
//                        A workgroup (4 waves) owns one (b, s), CONV_NT = 2048 outputs and MB microphones; a wave owns 2 tiles of 256 outputs, i.e.
//                        2 MB accumulators: per K step and residue MB + 2 ds_read_b32 feed 2 MB MFMAs (the strip of x is shared by the microphones,
//                        a tap fragment by the two tiles).  Per chunk the workgroup stages
//                            HT[m][r][j] = h[m][k0 + 16 (j - 15) + r]   tap blocks transposed, 15 zero columns in front and >= 15 behind,
//                            XS[p]       = x[g4 + p]                    g4 = the strip's first x index rounded down to a multiple of 4, zeros outside [0, N),
//                        so that the padding is zero-filled LDS and the tap loop has neither selects nor index arithmetic: the per-lane offsets
//                        (A: i + kk, B: c - 16 kk + the strip's alignment remainder) are computed once per chunk, the loop adds compile-time constants.
//                        Lanes of a 16-lane group read consecutive words (A: j = i + ..., B: c + ...), the groups overlap (A, broadcast) or sit 16
//                        words apart (B): no bank conflict.
//                        Rows that start on 16-byte boundaries (N % 4 == 0, L % 4 == 0, aligned base pointers) are staged with 16-byte loads (VEC), any
//                        other shape element by element.
// The order of the sum for an output is chunk, K step, residue, then the four K columns inside the MFMA (an fp32 fmaf chain): it is fixed by n and L
// alone.  Two calls give the same bits, an item does not depend on the batch it shares a launch with.  No atomics; every output is stored exactly once.
// A delay outside [0, L) is clamped into the range and reported through the status word (a plain store of 1 by thread 0 of the workgroups that meet it).
#include "launch.h"
#include "layout.h"
#include "conv_common.h"

#define CONV_TILE 256                       // outputs of one MFMA tile: 16 rows i x 16 columns c
#define CONV_C 2                            // tiles per wave
#define CONV_NT (4 * CONV_C * CONV_TILE)    // outputs per workgroup
#define CONV_XS (CONV_NT + 16 * (4 * CONV_TMAX - 1) + 20)  // strip in floats, a multiple of 4: the last read is at CONV_NT + 16 w_max - 223 + 3

static_assert(CONV_XS % 4 == 0, "the strip is staged in 16-byte pieces");

__global__ __launch_bounds__(CONV_THREADS) void rir_delay_kernel(int BS, int M, int L, int ref, const float* __restrict__ h, int32_t* __restrict__ delay) {
    NBSS_LDS(smem);
    float* sv = reinterpret_cast<float*>(smem);                // [256]
    int* si = reinterpret_cast<int*>(sv + CONV_THREADS);       // [256]
    const int tid = (int)threadIdx.x;
    for (int bs = (int)blockIdx.x; bs < BS; bs += (int)gridDim.x) {
        const float* row = h + ((size_t)bs * M + ref) * (size_t)L;
        float best = 0.f;
        int at = L;  // no candidate yet
        for (int k = tid; k < L; k += CONV_THREADS) {
            const float v = row[k];
            if (at == L || v > best) best = v, at = k;
        }
        sv[tid] = best;
        si[tid] = at;
        __syncthreads();
        for (int half = CONV_THREADS / 2; half >= 1; half >>= 1) {
            if (tid < half) {
                const float vo = sv[tid + half];
                const int io = si[tid + half];
                const float vm = sv[tid];
                const int im = si[tid];
                if (io < L && (im == L || vo > vm || (vo == vm && io < im))) sv[tid] = vo, si[tid] = io;
            }
            __syncthreads();
        }
        if (tid == 0) delay[bs] = si[0] < L ? si[0] : 0;  // a row without any comparable value (all NaN): 0
        __syncthreads();
    }
}

template <int MB, bool VEC>
__global__ __launch_bounds__(CONV_THREADS) void fir_convolve_kernel(int BS, int M, int N, int L, const float* __restrict__ x, const float* __restrict__ h,
                                                                    const int32_t* __restrict__ delay, float* __restrict__ y, int32_t* __restrict__ status) {
    NBSS_LDS(smem);
    float* HT = reinterpret_cast<float*>(smem);      // [MB][16][CONV_HS]
    float* XS = HT + MB * 16 * CONV_HS;              // [CONV_XS], 16-byte aligned: 16 CONV_HS floats are a multiple of 16 bytes
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = wave_id_u();
    const int li = lane & 15, kk = lane >> 4;
    const int n0 = (int)blockIdx.x * CONV_NT, m0 = (int)blockIdx.y * MB;
    const int nbw = n0 + wv * CONV_C * CONV_TILE;    // this wave's first output
    for (int bs = (int)blockIdx.z; bs < BS; bs += (int)gridDim.z) {
        int d = delay[bs];
        if (d < 0 || d >= L) {
            if (tid == 0 && status) status[0] = 1;
            d = d < 0 ? 0 : L - 1;
        }
        const float* xrow = x + (size_t)bs * (size_t)N;
        const float* hrow = h + ((size_t)bs * M + m0) * (size_t)L;
        f32x4 acc[MB][CONV_C];
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int ch = 0; ch < CONV_C; ++ch) acc[m][ch] = F32X4_ZERO;

        for (int k0 = 0; k0 < L; k0 += CONV_KT) {
            const int left = L - k0;
            const int qn = left >= CONV_KT ? CONV_QMAX : (left + 15) >> 4;  // tap blocks of this chunk
            const int T = (qn + 15 + 3) >> 2, wmax = 4 * T - 1;
            // the strip: xs(lo + p), lo = n0 - k0 + 225 - 16 wmax; in x indices g = lo + d, staged from g4 = g rounded down to a multiple of 4
            const int g = n0 - k0 + 225 - 16 * wmax + d, g4 = g & ~3, o = g - g4;
            const int xlen = CONV_NT + 16 * wmax + 20;  // <= CONV_XS, a multiple of 4
            __syncthreads();                            // the previous chunk's (or item's) readers are done
            conv_stage_taps<MB, VEC>(HT, hrow, m0, M, L, k0, qn, tid);
            // ---- stage the strip of x
            if (VEC) {
                for (int p = tid * 4; p < xlen; p += CONV_THREADS * 4) {
                    const int gi = g4 + p;  // a multiple of 4, as N is: the piece is inside or outside as a whole
                    f32x4 t = F32X4_ZERO;
                    if (gi >= 0 && gi < N) t = *reinterpret_cast<const f32x4*>(xrow + gi);
                    *reinterpret_cast<f32x4*>(XS + p) = t;
                }
            } else {
                for (int p = tid; p < xlen; p += CONV_THREADS) {
                    const int gi = g4 + p;
                    XS[p] = (gi >= 0 && gi < N) ? xrow[gi] : 0.f;
                }
            }
            __syncthreads();
            // ---- the products.  A: HT[m][r][li + kk + 4 t]; B: XS[(nb - n0) + li + 15 + 16 (wmax - kk - 4 t) - r + o]
            if (nbw < N) {  // wave-uniform: a wave whose outputs all lie beyond N only stages
                const float* pa = HT + li + kk;
                const float* pb = XS + (nbw - n0) + li + 15 + 16 * (wmax - kk) + o;
                for (int t = 0; t < T; ++t) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float a[MB], b[CONV_C];
#pragma unroll
                        for (int m = 0; m < MB; ++m) a[m] = pa[(m * 16 + r) * CONV_HS];
#pragma unroll
                        for (int ch = 0; ch < CONV_C; ++ch) b[ch] = pb[ch * CONV_TILE - r];
#pragma unroll
                        for (int m = 0; m < MB; ++m)
#pragma unroll
                            for (int ch = 0; ch < CONV_C; ++ch) acc[m][ch] = conv_mfma(a[m], b[ch], acc[m][ch]);
                    }
                    pa += 4;
                    pb -= 64;
                }
            }
        }
        // ---- D[i = 4 kk + j][c = li] -> y[nb + 16 i + c]
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            if (m0 + m >= M) break;
            float* yrow = y + ((size_t)bs * M + m0 + m) * (size_t)N;
#pragma unroll
            for (int ch = 0; ch < CONV_C; ++ch)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = nbw + ch * CONV_TILE + 16 * (4 * kk + j) + li;
                    if (n < N) yrow[n] = acc[m][ch][j];
                }
        }
    }
}

// ---------------- host side ----------------
static int conv_check_rows(int B, int S, int M, int L) {
    if (L < 1) return NBSS_EINVAL;
    if (B < 1 || S < 1 || M < 1) return NBSS_EUNSUPPORTED;
    if (L > CONV_MAX_L || M > CONV_MAX_M || (int64_t)B * S * M > CONV_MAX_ROWS) return NBSS_EUNSUPPORTED;
    return 0;
}

int rir_delay_impl(int B, int S, int M, int L, int ref_channel, const float* h, int32_t* delay, hipStream_t st) {
    int e = conv_check_rows(B, S, M, L);
    if (e) return e;
    if (ref_channel < 0 || ref_channel >= M) return NBSS_EINVAL;
    const int BS = B * S;
    NBSS_LAUNCH(rir_delay_kernel, dim3(BS < CONV_MAX_ITEMS ? BS : CONV_MAX_ITEMS), dim3(CONV_THREADS), CONV_THREADS * 8, st, BS, M, L, ref_channel, h, delay);
    return NBSS_CHECK_LAUNCH();
}

int fir_convolve_impl(int B, int S, int M, int N, int L, const float* x, const float* h, const int32_t* delay, float* y, int32_t* status, hipStream_t st) {
    if (N < 1) return NBSS_EINVAL;
    int e = conv_check_rows(B, S, M, L);
    if (e) return e;
    if (N > CONV_MAX_N) return NBSS_EUNSUPPORTED;
    const int BS = B * S;
    const int MB = conv_mic_group(M);
    const dim3 grid(cdiv(N, CONV_NT), cdiv(M, MB), BS < CONV_MAX_ITEMS ? BS : CONV_MAX_ITEMS);
    const size_t lds = ((size_t)MB * 16 * CONV_HS + CONV_XS) * sizeof(float);  // 48.4 KB at MB = 3: under the 64 KB a kernel gets without asking
    return conv_dispatch(MB, conv_vec(N, L, x, h), [&](auto mb, auto vec) {
        NBSS_LAUNCH((fir_convolve_kernel<decltype(mb)::value, decltype(vec)::value>), grid, dim3(CONV_THREADS), lds, st, BS, M, N, L, x, h, delay, y, status);
        return NBSS_CHECK_LAUNCH();
    });
}
