// gb_rows.hip — the row kernels of the geometry-generic path (gb.h): LayerNorm forward / backward (+ affine gradients), SiLU / PReLU backward,
// the [N][SQ] <-> [B T][SQ][F] transposes of the full-band block, the decoder's column padding, GroupNorm and GroupBatchNorm forward / backward.
#include "gb.h"
#include "blocks.h"

// ------------------------------------------------------------------------------------------------------------------------------------
// row kernels: one wave per row, lanes over the channels (C <= 64 * GB_CPL)
#define GB_CPL 6  // channels per lane: 384 / 64

// LayerNorm over the last dim (eps 1e-5): u = xhat gamma + beta (optional), stats = (mean, rstd)
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               T* __restrict__ u, float* __restrict__ stats, long N, int C) {
    const int lane = lane_id();
    const long nw = (long)gridDim.x * (GB_THREADS / 64);
    for (long n = (long)blockIdx.x * (GB_THREADS / 64) + wave_id(); n < N; n += nw) {
        float v[GB_CPL];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < GB_CPL; ++i) {
            const int c = lane + 64 * i;
            v[i] = c < C ? load1(x + n * C + c) : 0.f;
            s += v[i];
        }
        const float mean = wave_sum64(s) / C;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < GB_CPL; ++i) {
            const int c = lane + 64 * i;
            const float d = c < C ? v[i] - mean : 0.f;
            q += d * d;
        }
        const float rstd = rsqrtf(wave_sum64(q) / C + 1e-5f);
        if (lane == 0) {
            stats[2 * n] = mean;
            stats[2 * n + 1] = rstd;
        }
        if (u) {
#pragma unroll
            for (int i = 0; i < GB_CPL; ++i) {
                const int c = lane + 64 * i;
                if (c < C) store1(u + n * C + c, (v[i] - mean) * rstd * gamma[c] + beta[c]);
            }
        }
    }
}

// dx = dy + rstd (g - mean(g) - xhat mean(g xhat)), g = du gamma;  dgamma += sum du xhat, dbeta += sum du   (per-lane sums, one atomicAdd per
// (workgroup, channel) at the end)
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_ln_bwd_kernel(const T* __restrict__ du, const T* __restrict__ x, const float* __restrict__ stats,
                                                               const float* __restrict__ gamma, const T* __restrict__ dy, T* __restrict__ dx,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta, long N, int C) {
    NBSS_LDS(smem);
    float (*red)[64 * GB_CPL] = reinterpret_cast<float (*)[64 * GB_CPL]>(smem);  // [2][64 GB_CPL]
    const int lane = lane_id();
    for (int i = threadIdx.x; i < 2 * 64 * GB_CPL; i += GB_THREADS) (&red[0][0])[i] = 0.f;
    __syncthreads();
    float dg[GB_CPL], db[GB_CPL];
#pragma unroll
    for (int i = 0; i < GB_CPL; ++i) dg[i] = db[i] = 0.f;
    const long nw = (long)gridDim.x * (GB_THREADS / 64);
    for (long n = (long)blockIdx.x * (GB_THREADS / 64) + wave_id(); n < N; n += nw) {
        const float mean = stats[2 * n], rstd = stats[2 * n + 1];
        float xh[GB_CPL], g[GB_CPL];
        float m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int i = 0; i < GB_CPL; ++i) {
            const int c = lane + 64 * i;
            xh[i] = g[i] = 0.f;
            if (c < C) {
                xh[i] = (load1(x + n * C + c) - mean) * rstd;
                const float d = load1(du + n * C + c);
                dg[i] += d * xh[i];
                db[i] += d;
                g[i] = d * gamma[c];
                m1 += g[i];
                m2 += g[i] * xh[i];
            }
        }
        m1 = wave_sum64(m1) / C;
        m2 = wave_sum64(m2) / C;
#pragma unroll
        for (int i = 0; i < GB_CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < C) store1(dx + n * C + c, load1(dy + n * C + c) + rstd * (g[i] - m1 - xh[i] * m2));
        }
    }
#pragma unroll
    for (int i = 0; i < GB_CPL; ++i) {
        atomicAdd(&red[0][lane + 64 * i], dg[i]);
        atomicAdd(&red[1][lane + 64 * i], db[i]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += GB_THREADS) {
        atomicAdd(dgamma + c, red[0][c]);
        atomicAdd(dbeta + c, red[1][c]);
    }
}


// ---- row kernels for widths that are multiples of 64 with fewer lanes per row: a whole wave per 192-wide row spent its time in six-step wave
// reductions (LayerNorm backward: 144 us per launch for a 50 MB tensor; with 16 lanes per row 82 us; 8 lanes and one load burst: below)
// ---- LayerNorm forward / backward with 8 lanes per row (8 rows per wave; lane = 16-byte pieces l7 + 8 k of the row): every load of an iteration is
// independent of its reductions and issued up front — x, du AND dy: the 16-lane version fetched dy after the row sums, a second memory round trip per
// 4 rows (82 us per launch for 200 MB of traffic at batch 4) — and the clamped (not branched) addresses keep them in one burst.
NBSS_DEV float row_sum8(float v) {  // sum over the 8 lanes of a row (lanes sharing l >> 3), result in every lane
#ifdef NBSS_EMU
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
#else
#define NBSS_DPP_ADD(ctrl) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xF, 0xF, true))
    NBSS_DPP_ADD(0xB1);   // quad_perm [1,0,3,2]
    NBSS_DPP_ADD(0x4E);   // quad_perm [2,3,0,1]
    NBSS_DPP_ADD(0x141);  // row_half_mirror
#undef NBSS_DPP_ADD
    return v;
#endif
}
template <class T, int NP>  // C = 64 NP
__global__ __launch_bounds__(GB_THREADS) void gb_ln_fwd8_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                T* __restrict__ u, float* __restrict__ stats, long N) {
    constexpr int C = 64 * NP;
    const int lane = lane_id(), l7 = lane & 7, g8 = lane >> 3;
    const long nw = (long)gridDim.x * (GB_THREADS / 64) * 8;
    for (long n0 = ((long)blockIdx.x * (GB_THREADS / 64) + wave_id()) * 8; n0 < N; n0 += nw) {  // (whole-wave loop: row_sum8 is a wave collective)
        const long n = n0 + g8;
        const bool v_ = n < N;
        const T* xr = x + (v_ ? n : N - 1) * C + 8 * l7;
        float v[NP][8];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) load8(xr + 64 * k, v[k]);
#pragma unroll
        for (int k = 0; k < NP; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[k][j];
        const float mean = row_sum8(s) * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[k][j] - mean;
                q += d * d;
            }
        const float rstd = rsqrtf(row_sum8(q) * (1.0f / C) + 1e-5f);
        if (v_ && l7 == 0) {
            stats[2 * n] = mean;
            stats[2 * n + 1] = rstd;
        }
        if (u && v_) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                float gm[8], bt[8], o[8];
                load8(gamma + 64 * k + 8 * l7, gm);
                load8(beta + 64 * k + 8 * l7, bt);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (v[k][j] - mean) * rstd * gm[j] + bt[j];
                store8(u + n * C + 64 * k + 8 * l7, o);
            }
        }
    }
}
template <class T, int NP>
__global__ __launch_bounds__(GB_THREADS) void gb_ln_bwd8_kernel(const T* __restrict__ du, const T* __restrict__ x, const float* __restrict__ stats,
                                                                const float* __restrict__ gamma, const T* __restrict__ dy, T* __restrict__ dx,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ part, long N) {
    constexpr int C = 64 * NP;
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [2][C]
    const int lane = lane_id(), l7 = lane & 7, g8 = lane >> 3;
    for (int i = threadIdx.x; i < 2 * C; i += GB_THREADS) red[i] = 0.f;
    __syncthreads();
    float dg[NP][8], db[NP][8];
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) dg[k][j] = db[k][j] = 0.f;
    const long nw = (long)gridDim.x * (GB_THREADS / 64) * 8;
    for (long n0 = ((long)blockIdx.x * (GB_THREADS / 64) + wave_id()) * 8; n0 < N; n0 += nw) {
        const long n = n0 + g8;
        const bool v_ = n < N;
        const long nc = v_ ? n : N - 1;
        const float mean = stats[2 * nc], rstd = v_ ? stats[2 * nc + 1] : 0.f;
        float xh[NP][8], g[NP][8], yv[NP][8];
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            load8(x + nc * C + 64 * k + 8 * l7, xh[k]);
            load8(du + nc * C + 64 * k + 8 * l7, g[k]);
            load8(dy + nc * C + 64 * k + 8 * l7, yv[k]);
        }
        float m1 = 0.f, m2 = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float gm[8];
            load8(gamma + 64 * k + 8 * l7, gm);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float dv = v_ ? g[k][j] : 0.f;
                xh[k][j] = (xh[k][j] - mean) * rstd;
                dg[k][j] += dv * xh[k][j];
                db[k][j] += dv;
                g[k][j] = dv * gm[j];
                m1 += g[k][j];
                m2 += g[k][j] * xh[k][j];
            }
        }
        m1 = row_sum8(m1) * (1.0f / C);
        m2 = row_sum8(m2) * (1.0f / C);
        if (v_) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                float o[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = yv[k][j] + rstd * (g[k][j] - m1 - xh[k][j] * m2);
                store8(dx + n * C + 64 * k + 8 * l7, o);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            atomicAdd(&red[64 * k + 8 * l7 + j], dg[k][j]);
            atomicAdd(&red[C + 64 * k + 8 * l7 + j], db[k][j]);
        }
    __syncthreads();
    // part: one row per workgroup, folded by affine_reduce (1 024 workgroups adding to the same 2 C addresses are 1 024-deep chains of same-address
    // atomics: ~50 us behind a kernel whose memory phase takes 30)
    for (int c = threadIdx.x; c < C; c += GB_THREADS) {
        if (part) {
            part[(size_t)blockIdx.x * 2 * C + c] = red[c];
            part[(size_t)blockIdx.x * 2 * C + C + c] = red[C + c];
        } else {
            atomicAdd(dgamma + c, red[c]);
            atomicAdd(dbeta + c, red[C + c]);
        }
    }
}
template <class T, int NQ>
__global__ __launch_bounds__(GB_THREADS) void gb_prelu_bwd4_kernel(const T* __restrict__ a, const T* __restrict__ dy, const float* __restrict__ alpha,
                                                                   T* __restrict__ da, float* __restrict__ dalpha, long N) {
    constexpr int C = 64 * NQ;
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [C]
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4;
    for (int i = threadIdx.x; i < C; i += GB_THREADS) red[i] = 0.f;
    __syncthreads();
    float ds[NQ][4], al[NQ][4];
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ds[i][r] = 0.f;
            al[i][r] = alpha[64 * i + 4 * l15 + r];
        }
    const long nw = (long)gridDim.x * (GB_THREADS / 64) * 4;
    for (long n = ((long)blockIdx.x * (GB_THREADS / 64) + wave_id()) * 4 + g4; n < N; n += nw) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int c = 64 * i + 4 * l15;
            float av[4], dv[4], o[4];
            load4(a + n * C + c, av);
            load4(dy + n * C + c, dv);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[r] = av[r] > 0.f ? dv[r] : dv[r] * al[i][r];
                if (av[r] <= 0.f) ds[i][r] += dv[r] * av[r];
            }
            store4(da + n * C + c, o[0], o[1], o[2], o[3]);
        }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(&red[64 * i + 4 * l15 + r], ds[i][r]);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += GB_THREADS) atomicAdd(dalpha + c, red[c]);
}

// gout = gin * SiLU'(a)   (dense tensors; gout may be gin)
template <class T>
__global__ void gb_silu_bwd_kernel(const T* __restrict__ a, const T* gin, T* gout, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) store1(gout + i, load1(gin + i) * dsilu_f(load1(a + i)));
}
// PReLU: y = x + (a > 0 ? a : alpha a) is the block output; da = dy (a > 0 ? 1 : alpha[c]), dalpha[c] += sum dy min(a, 0)
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_prelu_bwd_kernel(const T* __restrict__ a, const T* __restrict__ dy, const float* __restrict__ alpha,
                                                                  T* __restrict__ da, float* __restrict__ dalpha, long N, int C) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [64 GB_CPL]
    const int lane = lane_id();
    for (int i = threadIdx.x; i < 64 * GB_CPL; i += GB_THREADS) red[i] = 0.f;
    __syncthreads();
    float ds[GB_CPL];
#pragma unroll
    for (int i = 0; i < GB_CPL; ++i) ds[i] = 0.f;
    const long nw = (long)gridDim.x * (GB_THREADS / 64);
    for (long n = (long)blockIdx.x * (GB_THREADS / 64) + wave_id(); n < N; n += nw) {
#pragma unroll
        for (int i = 0; i < GB_CPL; ++i) {
            const int c = lane + 64 * i;
            if (c < C) {
                const float av = load1(a + n * C + c), d = load1(dy + n * C + c);
                store1(da + n * C + c, av > 0.f ? d : d * alpha[c]);
                if (av <= 0.f) ds[i] += d * av;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < GB_CPL; ++i) atomicAdd(&red[lane + 64 * i], ds[i]);
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += GB_THREADS) atomicAdd(dalpha + c, red[c]);
}

// [N = (b, f, t)][SQ] -> [(b, t)][SQ][FK] (columns F..FK zero) and back
template <class T>
__global__ void gb_sq_to_f_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int F, int Tn, int SQ, int FK) {
    const long total = (long)B * Tn * SQ * FK;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int f = (int)(e % FK);
        long r = e / FK;
        const int g = (int)(r % SQ);
        r /= SQ;
        const int t = (int)(r % Tn), b = (int)(r / Tn);
        store1(dst + e, f < F ? load1(src + (((long)b * F + f) * Tn + t) * SQ + g) : 0.f);
    }
}
template <class T>
__global__ void gb_f_to_sq_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int F, int Tn, int SQ, int FK) {
    const long total = (long)B * F * Tn * SQ;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int g = (int)(e % SQ);
        long r = e / SQ;
        const int t = (int)(r % Tn);
        r /= Tn;
        const int f = (int)(r % F), b = (int)(r / F);
        store1(dst + e, load1(src + (((long)b * Tn + t) * SQ + g) * FK + f));
    }
}
// fp32 [N][Co] -> stream dtype [N][CP] (zero padded): the decoder's upstream gradient as a tap_gemm / wgrad operand
template <class T>
__global__ void gb_pad_cols_kernel(const float* __restrict__ src, T* __restrict__ dst, long N, int Co, int CP) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < N * CP; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % CP);
        store1(dst + e, c < Co ? src[(e / CP) * Co + c] : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// GroupNorm(groups, FFN) over (T x CG) per sequence and group (eps 1e-5): statistics, h = SiLU(xhat gamma + beta), backward
// one workgroup per (sequence, group); thread = (frame lane, channel)
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_gn_fwd_kernel(const T* __restrict__ a, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               T* __restrict__ h, float* __restrict__ stats, int Tn, int C, int CG, int act = 1) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [8]
    const int G = C / CG, seq = blockIdx.x / G, g = blockIdx.x % G;
    const int M = Tn * CG;
    const T* ab = a + (size_t)seq * Tn * C + g * CG;
    T* hb = h + (size_t)seq * Tn * C + g * CG;
    auto block_sum = [&](float v) -> float {
        v = wave_sum64(v);
        __syncthreads();
        if (lane_id() == 0) red[wave_id()] = v;
        __syncthreads();
        float s = 0.f;
        for (int i = 0; i < GB_THREADS / 64; ++i) s += red[i];
        return s;
    };
    float s = 0.f;
    for (int e = threadIdx.x; e < M; e += GB_THREADS) s += load1(ab + (size_t)(e / CG) * C + e % CG);
    const float mean = block_sum(s) / M;
    float q = 0.f;
    for (int e = threadIdx.x; e < M; e += GB_THREADS) {
        const float d = load1(ab + (size_t)(e / CG) * C + e % CG) - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(block_sum(q) / M + 1e-5f);
    if (stats && threadIdx.x == 0) {
        stats[2 * blockIdx.x] = mean;
        stats[2 * blockIdx.x + 1] = rstd;
    }
    for (int e = threadIdx.x; e < M; e += GB_THREADS) {
        const int c = e % CG;
        const size_t o = (size_t)(e / CG) * C + c;
        const float v = (load1(ab + o) - mean) * rstd * gamma[g * CG + c] + beta[g * CG + c];
        store1(hb + o, act ? silu_f(v) : v);
    }
}
// in: dh = gradient w.r.t. h = SiLU(a4), a4 = xhat gamma + beta; out (in place): gradient w.r.t. the GroupNorm input a; dgamma / dbeta accumulate
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_gn_bwd_kernel(const T* __restrict__ a, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, T* __restrict__ dh, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, int Tn, int C, int CG) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [8]
    float *cg_w = red + 8, *cg_b = cg_w + 64;    // [64] each: CG <= 64
    const int G = C / CG, seq = blockIdx.x / G, g = blockIdx.x % G;
    const int M = Tn * CG;
    const T* ab = a + (size_t)seq * Tn * C + g * CG;
    T* db = dh + (size_t)seq * Tn * C + g * CG;
    const float mean = stats[2 * blockIdx.x], rstd = stats[2 * blockIdx.x + 1];
    for (int i = threadIdx.x; i < 64; i += GB_THREADS) cg_w[i] = cg_b[i] = 0.f;
    __syncthreads();
    auto block_sum = [&](float v) -> float {
        v = wave_sum64(v);
        __syncthreads();
        if (lane_id() == 0) red[wave_id()] = v;
        __syncthreads();
        float s = 0.f;
        for (int i = 0; i < GB_THREADS / 64; ++i) s += red[i];
        return s;
    };
    // thread = (frame lane tl, channel ch): the channel's affine sums stay in registers over the frames (one LDS atomic per thread at the end;
    // as one LDS atomic per ELEMENT on 48 addresses the kernel took 531 us per launch)
    const int TPC = GB_THREADS / CG, tl = threadIdx.x / CG, ch = threadIdx.x % CG;
    const bool act = tl < TPC;
    const float gm = act ? gamma[g * CG + ch] : 0.f, bt = act ? beta[g * CG + ch] : 0.f;
    float s1 = 0.f, s2 = 0.f, dw = 0.f, dbv = 0.f;
    if (act) {
        for (int t = tl; t < Tn; t += TPC) {
            const size_t o = (size_t)t * C + ch;
            const float xh = (load1(ab + o) - mean) * rstd;
            const float d4 = load1(db + o) * dsilu_f(xh * gm + bt);
            dw += d4 * xh;
            dbv += d4;
            s1 += d4 * gm;
            s2 += d4 * gm * xh;
        }
        atomicAdd(&cg_w[ch], dw);
        atomicAdd(&cg_b[ch], dbv);
    }
    const float m1 = block_sum(s1) / M;
    const float m2 = block_sum(s2) / M;
    if (act) {
        for (int t = tl; t < Tn; t += TPC) {
            const size_t o = (size_t)t * C + ch;
            const float xh = (load1(ab + o) - mean) * rstd;
            const float d4 = load1(db + o) * dsilu_f(xh * gm + bt);
            store1(db + o, rstd * (d4 * gm - m1 - xh * m2));
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < CG; c += GB_THREADS) {
        atomicAdd(dgamma + g * CG + c, cg_w[c]);
        atomicAdd(dbeta + g * CG + c, cg_b[c]);
    }
}


// GroupBatchNorm of the narrow-band conformer (models/arch/NBC2.py:57-145 in the reference; share_along_sequence_dim = False): statistics over the
// F sequences of one utterance x the C features, per frame, always from the input itself (training AND evaluation); per-feature affine, optional SiLU.
// x [B][F][T][C]; one workgroup per (b, t).
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_gbn_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, T* __restrict__ y,
                                                            int F, int Tn, int C, float eps, int act) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [8]
    const int b = blockIdx.x / Tn, t = blockIdx.x % Tn;
    const size_t base = ((size_t)b * F * Tn + t) * C, fs = (size_t)Tn * C;  // element (f, c) at base + f fs + c
    const int M = F * C;
    auto block_sum = [&](float v) -> float {
        v = wave_sum64(v);
        __syncthreads();
        if (lane_id() == 0) red[wave_id()] = v;
        __syncthreads();
        float s = 0.f;
        for (int i = 0; i < GB_THREADS / 64; ++i) s += red[i];
        return s;
    };
    float s = 0.f;
    for (int e = threadIdx.x; e < M; e += GB_THREADS) s += load1(x + base + (size_t)(e / C) * fs + e % C);
    const float mean = block_sum(s) / M;
    float q = 0.f;
    for (int e = threadIdx.x; e < M; e += GB_THREADS) {
        const float d = load1(x + base + (size_t)(e / C) * fs + e % C) - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(block_sum(q) / M + eps);
    for (int e = threadIdx.x; e < M; e += GB_THREADS) {
        const int c = e % C;
        const size_t o = base + (size_t)(e / C) * fs + c;
        float v = (load1(x + o) - mean) * rstd;
        if (gamma) v = v * gamma[c] + beta[c];
        store1(y + o, act ? silu_f(v) : v);
    }
}

// Backward of the GroupBatchNorm above (+ its optional SiLU): one workgroup per (b, t), statistics recomputed from x.
//   a = xhat gamma + beta, y = act ? SiLU(a) : a;  d4 = dy (act ? SiLU'(a) : 1);  g = d4 gamma
//   dx = rstd (g - mean(g) - xhat mean(g xhat))  over the F x C elements of the frame;  dgamma[c] += sum_f d4 xhat, dbeta[c] += sum_f d4
// dy and dx may alias.  Per-channel sums: registers over the frequencies, one LDS atomic per thread, C global atomics per workgroup.
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_gbn_bwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                const T* dy, T* dx, float* __restrict__ dgamma, float* __restrict__ dbeta, int F, int Tn, int C,
                                                                float eps, int act) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);  // [8]
    float *cw = red + 8, *cb = cw + C;            // [C] each
    const int b = blockIdx.x / Tn, t = blockIdx.x % Tn;
    const size_t base = ((size_t)b * F * Tn + t) * C, fs = (size_t)Tn * C;
    const int M = F * C;
    for (int i = threadIdx.x; i < 2 * C; i += GB_THREADS) cw[i] = 0.f;
    auto block_sum = [&](float v) -> float {
        v = wave_sum64(v);
        __syncthreads();
        if (lane_id() == 0) red[wave_id()] = v;
        __syncthreads();
        float s = 0.f;
        for (int i = 0; i < GB_THREADS / 64; ++i) s += red[i];
        return s;
    };
    float s = 0.f;
    for (int e = threadIdx.x; e < M; e += GB_THREADS) s += load1(x + base + (size_t)(e / C) * fs + e % C);
    const float mean = block_sum(s) / M;
    float q = 0.f;
    for (int e = threadIdx.x; e < M; e += GB_THREADS) {
        const float d = load1(x + base + (size_t)(e / C) * fs + e % C) - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(block_sum(q) / M + eps);
    // thread = (frequency lane fl, channel c): C <= GB_THREADS is not required — channels are walked in rounds of GB_THREADS
    float s1 = 0.f, s2 = 0.f;
    for (int c0 = 0; c0 < C; c0 += GB_THREADS) {
        const int c = c0 + threadIdx.x;
        if (c < C) {
            const float gm = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
            float dw = 0.f, dbv = 0.f;
            for (int f = 0; f < F; ++f) {
                const size_t o = base + (size_t)f * fs + c;
                const float xh = (load1(x + o) - mean) * rstd;
                const float d4 = load1(dy + o) * (act ? dsilu_f(xh * gm + bt) : 1.f);
                dw += d4 * xh;
                dbv += d4;
                s1 += d4 * gm;
                s2 += d4 * gm * xh;
            }
            cw[c] = dw;  // (one thread per channel in this round: plain stores)
            cb[c] = dbv;
        }
    }
    const float m1 = block_sum(s1) / M;
    const float m2 = block_sum(s2) / M;
    for (int e = threadIdx.x; e < M; e += GB_THREADS) {
        const int c = e % C;
        const size_t o = base + (size_t)(e / C) * fs + c;
        const float gm = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
        const float xh = (load1(x + o) - mean) * rstd;
        const float d4 = load1(dy + o) * (act ? dsilu_f(xh * gm + bt) : 1.f);
        store1(dx + o, rstd * (d4 * gm - m1 - xh * m2));
    }
    __syncthreads();
    if (dgamma)
        for (int c = threadIdx.x; c < C; c += GB_THREADS) {
            atomicAdd(dgamma + c, cw[c]);
            atomicAdd(dbeta + c, cb[c]);
        }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// launchers
template <class T>
int gb_ln_fwd(const void* x, const float* gamma, const float* beta, void* u, float* stats, long N, int C, hipStream_t st) {
    if (C > 64 * GB_CPL) return NBSS_EUNSUPPORTED;
    if (C == 192) NBSS_LAUNCH((gb_ln_fwd8_kernel<T, 3>), dim3(gb_blocks(N, 32 * 2)), dim3(GB_THREADS), 0, st, (const T*)x, gamma, beta, (T*)u, stats, N);
    else if (C == 384) NBSS_LAUNCH((gb_ln_fwd8_kernel<T, 6>), dim3(gb_blocks(N, 32 * 2)), dim3(GB_THREADS), 0, st, (const T*)x, gamma, beta, (T*)u, stats, N);
    else NBSS_LAUNCH((gb_ln_fwd_kernel<T>), dim3(gb_blocks(N, 4)), dim3(GB_THREADS), 0, st, (const T*)x, gamma, beta, (T*)u, stats, N, C);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_ln_bwd(const void* du, const void* x, const float* stats, const float* gamma, const void* dy, void* dx, float* dgamma, float* dbeta, long N,
                     int C, hipStream_t st, float* part, size_t part_floats) {
    if (C > 64 * GB_CPL) return NBSS_EUNSUPPORTED;
    const int blocks = gb_blocks(N, 4 * 16) < 1024 ? gb_blocks(N, 4 * 16) : 1024;  // >= 16 rows per wave: the affine sums end in C atomics per workgroup
    int blocks8 = gb_blocks(N, 32 * 4) < 1024 ? gb_blocks(N, 32 * 4) : 1024;  // (>= 4 rows per 8-lane group)
    if (part && (C == 192 || C == 384)) {
        if ((size_t)blocks8 * 2 * C > part_floats) blocks8 = (int)(part_floats / (2 * C));
        if (blocks8 < 64) part = nullptr, blocks8 = gb_blocks(N, 32 * 4) < 1024 ? gb_blocks(N, 32 * 4) : 1024;
    } else part = nullptr;
    if (C == 192)
        NBSS_LAUNCH((gb_ln_bwd8_kernel<T, 3>), dim3(blocks8), dim3(GB_THREADS), 2 * 192 * sizeof(float), st, (const T*)du, (const T*)x, stats, gamma, (const T*)dy, (T*)dx, dgamma, dbeta, part, N);
    else if (C == 384)
        NBSS_LAUNCH((gb_ln_bwd8_kernel<T, 6>), dim3(blocks8), dim3(GB_THREADS), 2 * 384 * sizeof(float), st, (const T*)du, (const T*)x, stats, gamma, (const T*)dy, (T*)dx, dgamma, dbeta, part, N);
    else
        NBSS_LAUNCH((gb_ln_bwd_kernel<T>), dim3(blocks), dim3(GB_THREADS), 2 * 64 * GB_CPL * sizeof(float), st, (const T*)du, (const T*)x, stats, gamma, (const T*)dy, (T*)dx, dgamma, dbeta, N, C);
    int e = NBSS_CHECK_LAUNCH();
    if (e || !part) return e;
    AffSegs sg;
    sg.n = 2;
    sg.off[0] = 0; sg.off[1] = dbeta - dgamma;  // (relative to dgamma)
    sg.cnt[0] = sg.cnt[1] = C;
    return affine_reduce_launch(part, blocks8, sg, dgamma, st);
}
template <class T>
int gb_silu_bwd(const void* a, const void* gin, void* gout, long n, hipStream_t st) {
    NBSS_LAUNCH((gb_silu_bwd_kernel<T>), dim3(gb_blocks(n, 1024)), dim3(256), 0, st, (const T*)a, (const T*)gin, (T*)gout, n);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_prelu_bwd(const void* a, const void* dy, const float* alpha, void* da, float* dalpha, long N, int C, hipStream_t st) {
    if (C > 64 * GB_CPL) return NBSS_EUNSUPPORTED;
    if (C == 192)
        NBSS_LAUNCH((gb_prelu_bwd4_kernel<T, 3>), dim3(gb_blocks(N, 16 * 8) < 1024 ? gb_blocks(N, 16 * 8) : 1024), dim3(GB_THREADS), 192 * sizeof(float), st, (const T*)a,
                    (const T*)dy, alpha, (T*)da, dalpha, N);
    else
        NBSS_LAUNCH((gb_prelu_bwd_kernel<T>), dim3(gb_blocks(N, 64) < 1024 ? gb_blocks(N, 64) : 1024), dim3(GB_THREADS), 64 * GB_CPL * sizeof(float), st, (const T*)a, (const T*)dy,
                    alpha, (T*)da, dalpha, N, C);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_sq_to_f(const void* src, void* dst, int B, int F, int Tn, int SQ, int FK, hipStream_t st) {
    NBSS_LAUNCH((gb_sq_to_f_kernel<T>), dim3(gb_blocks((long)B * Tn * SQ * FK, 1024)), dim3(256), 0, st, (const T*)src, (T*)dst, B, F, Tn, SQ, FK);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_f_to_sq(const void* src, void* dst, int B, int F, int Tn, int SQ, int FK, hipStream_t st) {
    NBSS_LAUNCH((gb_f_to_sq_kernel<T>), dim3(gb_blocks((long)B * F * Tn * SQ, 1024)), dim3(256), 0, st, (const T*)src, (T*)dst, B, F, Tn, SQ, FK);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_pad_cols(const float* src, void* dst, long N, int Co, int CP, hipStream_t st) {
    NBSS_LAUNCH((gb_pad_cols_kernel<T>), dim3(gb_blocks(N * CP, 1024)), dim3(256), 0, st, src, (T*)dst, N, Co, CP);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_gn_fwd(const void* a, const float* gamma, const float* beta, void* h, float* stats, long nsg, int Tn, int C, int CG, int act, hipStream_t st) {
    NBSS_LAUNCH((gb_gn_fwd_kernel<T>), dim3((unsigned)nsg), dim3(GB_THREADS), 8 * sizeof(float), st, (const T*)a, gamma, beta, (T*)h, stats, Tn, C, CG, act);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_gn_bwd(const void* a, const float* stats, const float* gamma, const float* beta, void* dh, float* dgamma, float* dbeta, long nsg, int Tn, int C, int CG,
              hipStream_t st) {
    if (CG > 64) return NBSS_EUNSUPPORTED;  // (the kernel's per-channel LDS sums)
    NBSS_LAUNCH((gb_gn_bwd_kernel<T>), dim3((unsigned)nsg), dim3(GB_THREADS), (8 + 128) * sizeof(float), st, (const T*)a, stats, gamma, beta, (T*)dh, dgamma, dbeta, Tn, C, CG);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_gbn_fwd(const void* x, const float* gamma, const float* beta, void* y, int B, int F, int Tn, int C, float eps, int act, hipStream_t st) {
    NBSS_LAUNCH((gb_gbn_kernel<T>), dim3(B * Tn), dim3(GB_THREADS), 8 * sizeof(float), st, (const T*)x, gamma, beta, (T*)y, F, Tn, C, eps, act);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_gbn_bwd(const void* x, const float* gamma, const float* beta, const void* dy, void* dx, float* dgamma, float* dbeta, int B, int F, int Tn, int C, float eps,
               int act, hipStream_t st) {
    NBSS_LAUNCH((gb_gbn_bwd_kernel<T>), dim3(B * Tn), dim3(GB_THREADS), (8 + 2 * (size_t)C) * sizeof(float), st, (const T*)x, gamma, beta, (const T*)dy, (T*)dx, dgamma, dbeta,
                F, Tn, C, eps, act);
    return NBSS_CHECK_LAUNCH();
}

#define GB_INSTANTIATE(T)                                                                                                                                  \
    template int gb_ln_fwd<T>(const void*, const float*, const float*, void*, float*, long, int, hipStream_t);                                            \
    template int gb_ln_bwd<T>(const void*, const void*, const float*, const float*, const void*, void*, float*, float*, long, int, hipStream_t, float*, size_t); \
    template int gb_silu_bwd<T>(const void*, const void*, void*, long, hipStream_t);                                                                       \
    template int gb_prelu_bwd<T>(const void*, const void*, const float*, void*, float*, long, int, hipStream_t);                                           \
    template int gb_sq_to_f<T>(const void*, void*, int, int, int, int, int, hipStream_t);                                                                  \
    template int gb_f_to_sq<T>(const void*, void*, int, int, int, int, int, hipStream_t);                                                                  \
    template int gb_pad_cols<T>(const float*, void*, long, int, int, hipStream_t);                                                                         \
    template int gb_gn_fwd<T>(const void*, const float*, const float*, void*, float*, long, int, int, int, int, hipStream_t);                              \
    template int gb_gn_bwd<T>(const void*, const float*, const float*, const float*, void*, float*, float*, long, int, int, int, hipStream_t);             \
    template int gb_gbn_fwd<T>(const void*, const float*, const float*, void*, int, int, int, int, float, int, hipStream_t);                               \
    template int gb_gbn_bwd<T>(const void*, const float*, const float*, const void*, void*, float*, float*, int, int, int, int, float, int, hipStream_t);
GB_INSTANTIATE(float)
GB_INSTANTIATE(bf16_t)
