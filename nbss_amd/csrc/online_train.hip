// online_train.hip — the causal T-ConvFFN of the OnlineSpatialNet for TRAINING: forward that keeps what the backward needs, and the backward with
// every parameter gradient (reference: models/arch/OnlineSpatialNet.py:114-126 `_tconvffn`; the streaming form of the same block is online.hip).
//
//   y = x + W2 SiLU(conv3(SiLU(GN(conv2(SiLU(conv1(SiLU(W1 LN(x) + b1))))))))           x, y [B][F][T][96], stream dtype fp32 or bf16
//   conv = causal grouped Conv1d (k = 3, 8 groups of 24, zero history before frame 0); GN = GroupNorm(8, 192) of each (b, t) over 24 channels x F frequencies
//
// Nothing depends on the whole time axis: every pass works on the flattened token axis n = (b F + f) T + t (the convs look at n - 2 .. n inside a sequence),
// so T is only bounded by NBSS_T_MAX.  Pass structure — the streaming step's, one tensor pass per launch:
//   forward   LN (gb_ln_fwd, keeps mean / rstd)  ->  a1 = W1 u + b1  ->  a2 = conv1(SiLU a1)  ->  a3 = conv2(SiLU a2)            [tap-GEMMs of gb_gemm.hip on MFMA:
//             -> per-(token, group) (mean, M2) of a3 from deviations -> fold over the frequencies IN ORDER -> (mean, rstd) per      a causal conv is the tap-GEMM
//             (b, t, group) -> h4 = SiLU(GN a3) -> a4 = conv3(h4) -> y = x + W2 SiLU(a4) + b2                                        with its centre on the last tap]
//   backward  the chain in reverse: the data gradients are tap-GEMMs with the re-laid (transposed, tap-flipped) weights and centre 0 (anti-causal), SiLU' applied
//             on store; the GroupNorm's two per-frame sums come from per-(token, group) partials folded over the frequencies in order; LN' at the end adds dy.
//   weight gradients  ot_wgrad_kernel: dW[o][i][tap] = sum_n dY[n][o] X[n + tap - (taps - 1)][i] on MFMA with the TOKEN axis as K — a workgroup owns a slab
//             of tokens and one (group | 32 output rows), stages 32 tokens of both operands transposed in LDS (SiLU or LayerNorm applied on the way in), and
//             writes its partial dW / dbias; ot_fold_kernel adds the slabs' partials in slab order into the caller's fp32 buffers (accumulate).
// No atomics anywhere, every fold in a fixed order: two calls give the same bits, and a batch item's y / dx rows do not depend on the other items.
//
// SAVED in `save` (nbss_online_tconvffn_train_save_bytes): LN (mean, rstd) [N][2], GN (mean, rstd) [B][T][8][2] (fp32), and the five [N][192] stream tensors
// a1, a2, a3, h4, a4 — the pre-activations every SiLU' needs plus the one post-norm activation (h4), whose recomputation would need the statistics in the
// weight-gradient kernel.  RECOMPUTED in the backward: u = LN(x) (from x and the kept statistics, inside the W1 weight-gradient staging), SiLU(a1), SiLU(a2),
// SiLU(a4) (on load) and the GroupNorm's xhat.
#include "gb.h"

#define OT_H 96
#define OT_FFN 192
#define OT_G 8
#define OT_CG 24
#define OT_TAPS 3
#define OT_WSLOT 24576   // elements of the largest re-laid weight (8 groups x 3 taps x 32 x 32)
#define OT_SLABS 128     // token slabs of the parameter-gradient partials
#define OT_CHUNK 32      // tokens per MFMA K block of the weight-gradient kernel
#define OT_LDT 40        // LDS row of a transposed operand: 32 tokens + 8 (rows stay 16-byte aligned and spread over the banks)
#define OT_PART (OT_FFN * OT_H + OT_FFN)  // floats of the largest partial (dW1 + db1)

struct OtGeom {
    long N;
    size_t esz, act, save_total, ws_total;
    // save
    size_t s_ln, s_gn, s_a1, s_a2, s_a3, s_h4, s_a4;
    // ws
    size_t w_u, w_g1, w_g2, w_gpart, w_gfold, w_wp, w_part;
    int slab_len, slabs;
};
static OtGeom ot_geom(int dtype, int B, int F, int T) {
    OtGeom g;
    g.N = (long)B * F * T;
    g.esz = dtype == NBSS_BF16 ? 2 : 4;
    g.act = ws_align((size_t)g.N * OT_FFN * g.esz);
    size_t o = 0;
    g.s_ln = o; o += ws_align((size_t)g.N * 2 * sizeof(float));
    g.s_gn = o; o += ws_align((size_t)B * T * OT_G * 2 * sizeof(float));
    g.s_a1 = o; o += g.act;
    g.s_a2 = o; o += g.act;
    g.s_a3 = o; o += g.act;
    g.s_h4 = o; o += g.act;
    g.s_a4 = o; o += g.act;
    g.save_total = o;
    o = 0;
    g.w_u = o; o += ws_align((size_t)g.N * OT_H * g.esz);
    g.w_g1 = o; o += g.act;
    g.w_g2 = o; o += g.act;
    g.w_gpart = o; o += ws_align((size_t)g.N * OT_G * 2 * sizeof(float));
    g.w_gfold = o; o += ws_align((size_t)B * T * OT_G * 2 * sizeof(float));
    g.w_wp = o; o += 5 * ws_align((size_t)OT_WSLOT * g.esz);
    g.w_part = o; o += ws_align((size_t)OT_SLABS * OT_PART * sizeof(float));
    g.ws_total = o;
    const long per = (g.N + OT_SLABS - 1) / OT_SLABS;
    g.slab_len = (int)((per + OT_CHUNK - 1) / OT_CHUNK * OT_CHUNK);
    g.slabs = (int)((g.N + g.slab_len - 1) / g.slab_len);
    return g;
}
// NBSS_OK, or why the shape is refused
static int ot_check(int dtype, int B, int F, int T) {
    if ((dtype != NBSS_F32 && dtype != NBSS_BF16) || B < 1 || F < 1) return NBSS_EINVAL;
    if (T < 1 || T > NBSS_T_MAX || F > NBSS_F_MAX || (long)B * F * T > (1L << 28)) return NBSS_EUNSUPPORTED;
    return NBSS_OK;
}
static int ot_grid(long total) {
    const long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : b > (1 << 20) ? (1 << 20) : b);
}

// ---- GroupNorm of each frame over (24 channels x F frequencies) ------------------------------------------------------------------------------------
// one (token, group) per thread: (mean, M2 = sum of squared deviations from it) of the 24 inputs, formed from their deviations from one of them (online.hip:
// E[a^2] - mean^2 in fp32 loses the variance once |mean| / std reaches a few hundred)
template <class T>
__global__ __launch_bounds__(256) void ot_gn_part_kernel(const T* __restrict__ a3, float* __restrict__ part, long N) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N * OT_G; i += (long)gridDim.x * 256) {
#pragma clang fp reassociate(off)
        float r[OT_CG];
        const T* p = a3 + i * OT_CG;  // (token n, group g): n * 192 + g * 24
        load8(p, r);
        load8(p + 8, r + 8);
        load8(p + 16, r + 16);
        const float piv = r[0];
        float sd = 0.f, m2 = 0.f;
#pragma unroll
        for (int c = 1; c < OT_CG; ++c) sd += r[c] - piv;
        const float md = sd * (1.0f / OT_CG);
#pragma unroll
        for (int c = 0; c < OT_CG; ++c) {
            const float d = (r[c] - piv) - md;
            m2 += d * d;
        }
        part[2 * i] = piv + md;
        part[2 * i + 1] = m2;
    }
}
// the frequencies' pairs combined in frequency order, one thread per (b, t, group) (online_gn_fold_kernel's formula) -> (mean, rstd)
__global__ __launch_bounds__(256) void ot_gn_fold_kernel(const float* __restrict__ part, float* __restrict__ stat, int B, int F, int Tn) {
    const long per_b = (long)Tn * OT_G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < B * per_b; i += (long)gridDim.x * 256) {
        const long b = i / per_b, r = i - b * per_b;
        const int t = (int)(r / OT_G), g = (int)(r % OT_G);
        const float* p = part + (((size_t)b * F * Tn + t) * OT_G + g) * 2;
        const size_t fs = (size_t)Tn * OT_G * 2;
        const float piv = p[0];
        float sd = 0.f, sq = 0.f, m2 = 0.f;
        for (int f = 0; f < F; ++f) {
#pragma clang fp reassociate(off)
            const float d = p[f * fs] - piv;
            sd += d;
            sq += d * d;
            m2 += p[f * fs + 1];
        }
        const float md = sd / (float)F;
        stat[2 * i] = piv + md;
        stat[2 * i + 1] = rsqrtf((m2 + (float)OT_CG * fmaxf(sq - sd * md, 0.f)) / (float)(OT_CG * F) + 1e-5f);
    }
}
// h4 = SiLU((a3 - mean) rstd gamma + beta): one thread per (token, 8 channels)
template <class T>
__global__ __launch_bounds__(256) void ot_gn_apply_kernel(const T* __restrict__ a3, const float* __restrict__ stat, const float* __restrict__ gw,
                                                          const float* __restrict__ gb, T* __restrict__ h4, long N, int F, int Tn) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N * (OT_FFN / 8); i += (long)gridDim.x * 256) {
        const long n = i / (OT_FFN / 8);
        const int c0 = (int)(i - n * (OT_FFN / 8)) * 8, g = c0 / OT_CG;
        const long b = n / ((long)F * Tn);
        const int t = (int)(n % Tn);
        const float* st = stat + ((b * Tn + t) * OT_G + g) * 2;
        const float mean = st[0], rstd = st[1];
        float v[8];
        load8(a3 + n * OT_FFN + c0, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = silu_f((v[j] - mean) * rstd * gw[c0 + j] + gb[c0 + j]);
        store8(h4 + n * OT_FFN + c0, v);
    }
}
// backward, first pass: per (token, group) the two sums of gy = dh4 SiLU'(z) gamma:  sum gy,  sum gy xhat
template <class T>
__global__ __launch_bounds__(256) void ot_gn_bwd_part_kernel(const T* __restrict__ a3, const T* __restrict__ dh4, const float* __restrict__ stat,
                                                             const float* __restrict__ gw, const float* __restrict__ gb, float* __restrict__ part, long N, int F,
                                                             int Tn) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N * OT_G; i += (long)gridDim.x * 256) {
        const long n = i / OT_G;
        const int g = (int)(i % OT_G);
        const long b = n / ((long)F * Tn);
        const int t = (int)(n % Tn);
        const float* st = stat + ((b * Tn + t) * OT_G + g) * 2;
        const float mean = st[0], rstd = st[1];
        float a[OT_CG], d[OT_CG];
        load8(a3 + i * OT_CG, a); load8(a3 + i * OT_CG + 8, a + 8); load8(a3 + i * OT_CG + 16, a + 16);
        load8(dh4 + i * OT_CG, d); load8(dh4 + i * OT_CG + 8, d + 8); load8(dh4 + i * OT_CG + 16, d + 16);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < OT_CG; ++c) {
            const float xh = (a[c] - mean) * rstd, gam = gw[g * OT_CG + c];
            const float gy = d[c] * dsilu_f(xh * gam + gb[g * OT_CG + c]) * gam;
            s1 += gy;
            s2 += gy * xh;
        }
        part[2 * i] = s1;
        part[2 * i + 1] = s2;
    }
}
// ... folded over the frequencies in order -> the two means over the 24 F values of a (b, t, group)
__global__ __launch_bounds__(256) void ot_gn_bwd_fold_kernel(const float* __restrict__ part, float* __restrict__ fold, int B, int F, int Tn) {
    const long per_b = (long)Tn * OT_G;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < B * per_b; i += (long)gridDim.x * 256) {
        const long b = i / per_b, r = i - b * per_b;
        const float* p = part + ((size_t)b * F * per_b + r) * 2;
        const size_t fs = (size_t)per_b * 2;
        float s1 = 0.f, s2 = 0.f;
        for (int f = 0; f < F; ++f) {
#pragma clang fp reassociate(off)
            s1 += p[f * fs];
            s2 += p[f * fs + 1];
        }
        fold[2 * i] = s1 / (float)(OT_CG * F);
        fold[2 * i + 1] = s2 / (float)(OT_CG * F);
    }
}
// second pass, in place (d: dh4 in, da3 out): da3 = rstd (gy - mean(gy) - xhat mean(gy xhat)); one channel per thread over a slab of tokens, whose
// dgamma = sum dz xhat, dbeta = sum dz go to part[slab][2][192] (folded in slab order by ot_fold_kernel)
template <class T>
__global__ __launch_bounds__(OT_FFN) void ot_gn_bwd_apply_kernel(const T* __restrict__ a3, T* __restrict__ d, const float* __restrict__ stat,
                                                                 const float* __restrict__ fold, const float* __restrict__ gw, const float* __restrict__ gb,
                                                                 float* __restrict__ part, long N, int F, int Tn, int slab_len) {
    const int c = threadIdx.x, g = c / OT_CG;
    const long n0 = (long)blockIdx.x * slab_len, n1 = n0 + slab_len < N ? n0 + slab_len : N;
    const float gam = gw[c], bet = gb[c];
    float dg = 0.f, db = 0.f;
    for (long n = n0; n < n1; ++n) {
#pragma clang fp reassociate(off)
        const long b = n / ((long)F * Tn);
        const int t = (int)(n % Tn);
        const size_t si = ((size_t)(b * Tn + t) * OT_G + g) * 2;
        const float mean = stat[si], rstd = stat[si + 1];
        const float xh = (load1(a3 + n * OT_FFN + c) - mean) * rstd;
        const float dz = load1(d + n * OT_FFN + c) * dsilu_f(xh * gam + bet);
        store1(d + n * OT_FFN + c, rstd * (dz * gam - fold[si] - xh * fold[si + 1]));
        dg += dz * xh;
        db += dz;
    }
    part[(size_t)blockIdx.x * 2 * OT_FFN + c] = dg;
    part[(size_t)blockIdx.x * 2 * OT_FFN + OT_FFN + c] = db;
}

// ---- LayerNorm backward: dx = dy + rstd (g - mean(g) - xhat mean(g xhat)), g = du gamma; one wave per token, a slab of tokens per workgroup -------------
template <class T>
__global__ __launch_bounds__(256) void ot_ln_bwd_kernel(const T* __restrict__ du, const T* __restrict__ x, const float* __restrict__ stats,
                                                        const float* __restrict__ gamma, const T* __restrict__ dy, T* __restrict__ dx, float* __restrict__ part,
                                                        long N, int slab_len) {
    NBSS_LDS(smem);
    float(*red)[2][OT_H] = reinterpret_cast<float(*)[2][OT_H]>(smem);  // [4 waves][dgamma | dbeta][96]
    const int lane = lane_id(), w = wave_id();
    const bool hi = lane < 32;  // channels lane and (lanes 0..31) 64 + lane
    const long n0 = (long)blockIdx.x * slab_len, n1 = n0 + slab_len < N ? n0 + slab_len : N;
    const float g0 = gamma[lane], g1 = hi ? gamma[64 + lane] : 0.f;
    float dg0 = 0.f, dg1 = 0.f, db0 = 0.f, db1 = 0.f;
    for (long n = n0 + w; n < n1; n += 4) {
        const float mean = stats[2 * n], rstd = stats[2 * n + 1];
        const float u0 = load1(du + n * OT_H + lane), u1 = hi ? load1(du + n * OT_H + 64 + lane) : 0.f;
        const float x0 = (load1(x + n * OT_H + lane) - mean) * rstd, x1 = hi ? (load1(x + n * OT_H + 64 + lane) - mean) * rstd : 0.f;
        const float m1 = wave_sum64(u0 * g0 + u1 * g1) * (1.0f / OT_H), m2 = wave_sum64(u0 * g0 * x0 + u1 * g1 * x1) * (1.0f / OT_H);
        store1(dx + n * OT_H + lane, load1(dy + n * OT_H + lane) + rstd * (u0 * g0 - m1 - x0 * m2));
        if (hi) store1(dx + n * OT_H + 64 + lane, load1(dy + n * OT_H + 64 + lane) + rstd * (u1 * g1 - m1 - x1 * m2));
        dg0 += u0 * x0; dg1 += u1 * x1;
        db0 += u0; db1 += u1;
    }
    red[w][0][lane] = dg0; red[w][1][lane] = db0;
    if (hi) { red[w][0][64 + lane] = dg1; red[w][1][64 + lane] = db1; }
    __syncthreads();
    if (threadIdx.x < 2 * OT_H) {  // the four waves' sums in wave order
        const int k = threadIdx.x / OT_H, c = threadIdx.x % OT_H;
        part[(size_t)blockIdx.x * 2 * OT_H + threadIdx.x] = ((red[0][k][c] + red[1][k][c]) + red[2][k][c]) + red[3][k][c];
    }
}

// dst[i] += sum over the slabs (in slab order) of part[slab][i], i < n
__global__ __launch_bounds__(256) void ot_fold_kernel(const float* __restrict__ part, int slabs, int stride, int n1, float* __restrict__ dst1, int n2,
                                                      float* __restrict__ dst2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n1 + n2) return;
    const float s = fold_strided<8>(part + i, (size_t)stride, 0, slabs);
    if (i < n1) dst1[i] += s;
    else dst2[i - n1] += s;
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------------------------------------
enum { OT_X_PLAIN, OT_X_SILU, OT_X_LN };
struct OtWgrad {
    const void* A;  // dY [N][lda]
    const void* X;  // the forward's input [N][ldx] (before `xf`)
    int lda, ldx;
    int grouped;    // 1: 8 groups of 24 x 24 (blockIdx.y = group), 0: dense M x K (blockIdx.y = 32 output rows)
    int K;          // inputs per output row (24 grouped)
    int taps, Tn;
    const float* stats;  // OT_X_LN: (mean, rstd) per token, gamma, beta
    const float* gamma;
    const float* beta;
    float* part;    // [slabs][stride]: dW [M][K][taps] then dbias [M]
    int stride, M;
    long N;
    int slab_len;
};
// grid (slabs, M / 32 | 8 groups), 256 threads.  Per 32-token chunk: A^T [32 rows][32 tokens] and X^T [taps][KP rows][32 tokens] (tap image = the tokens shifted
// by tap - (taps - 1), zero before frame 0) in LDS; wave w owns the (tap, 16-input tile) pairs w, w + 4, w + 8 for both 16-row tiles of A.
template <class T, int XF>
__global__ __launch_bounds__(256) void ot_wgrad_kernel(OtWgrad a) {
    NBSS_LDS(smem);
    const int KP = (a.K + 15) & ~15, NT = KP / 16, combos = a.taps * NT;
    T* At = reinterpret_cast<T*>(smem);  // [32][OT_LDT]
    T* Xt = At + 32 * OT_LDT;            // [taps][KP][OT_LDT]
    const int tid = threadIdx.x, lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id_u();
    const int m0 = a.grouped ? blockIdx.y * OT_CG : blockIdx.y * 32, mlen = a.grouped ? OT_CG : 32, k0 = a.grouped ? blockIdx.y * OT_CG : 0;
    const long n0 = (long)blockIdx.x * a.slab_len, n1 = n0 + a.slab_len < a.N ? n0 + a.slab_len : a.N;
    const T* A = reinterpret_cast<const T*>(a.A);
    const T* X = reinterpret_cast<const T*>(a.X);
    f32x4 acc[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = F32X4_ZERO;
    float bacc = 0.f;
    for (long nc = n0; nc < n1; nc += OT_CHUNK) {
        for (int e = tid; e < OT_CHUNK * 32; e += 256) {
            const int col = e & 31, tok = e >> 5;
            const long n = nc + tok;
            store1(At + col * OT_LDT + tok, (n < n1 && col < mlen) ? load1(A + n * a.lda + m0 + col) : 0.f);
        }
        for (int e = tid; e < a.taps * OT_CHUNK * KP; e += 256) {
            const int col = e % KP, r = e / KP, tok = r % OT_CHUNK, tap = r / OT_CHUNK;
            const long n = nc + tok;
            const int d = tap - (a.taps - 1);
            float v = 0.f;
            if (n < n1 && col < a.K && (int)(n % a.Tn) + d >= 0) {
                const long src = n + d;
                v = load1(X + src * a.ldx + k0 + col);
                if (XF == OT_X_SILU) v = silu_f(v);
                if (XF == OT_X_LN) v = (v - a.stats[2 * src]) * a.stats[2 * src + 1] * a.gamma[col] + a.beta[col];
            }
            store1(Xt + ((size_t)tap * KP + col) * OT_LDT + tok, v);
        }
        __syncthreads();
        if (tid < 32) {  // dbias: the chunk's column sum, tokens in order
#pragma clang fp reassociate(off)
            float s = 0.f;
            for (int k = 0; k < OT_CHUNK; ++k) s += load1(At + tid * OT_LDT + k);
            bacc += s;
        }
        Frag<T> fa0, fa1;
        frag_load(fa0, At + l15 * OT_LDT + 8 * g4);
        frag_load(fa1, At + (16 + l15) * OT_LDT + 8 * g4);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int cb = w + 4 * j;  // wave-uniform
            if (cb < combos) {
                const int tap = cb / NT, nt = cb % NT;
                Frag<T> fb;
                frag_load(fb, Xt + ((size_t)tap * KP + nt * 16 + l15) * OT_LDT + 8 * g4);
                acc[0][j] = mma(fa0, fb, acc[0][j]);
                acc[1][j] = mma(fa1, fb, acc[1][j]);
            }
        }
        __syncthreads();
    }
    float* pt = a.part + (size_t)blockIdx.x * a.stride;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int cb = w + 4 * j;
        if (cb >= combos) continue;
        const int tap = cb / NT, i = (cb % NT) * 16 + l15;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt * 16 + 4 * g4 + r;
                if (m < mlen && i < a.K) pt[((size_t)(m0 + m) * a.K + i) * a.taps + tap] = acc[mt][j][r];
            }
    }
    if (tid < mlen) pt[(size_t)a.M * a.K * a.taps + m0 + tid] = bacc;
}

template <class T>
static int ot_wgrad(const OtGeom& g, int xf, const void* A, int M, const void* X, int K, int grouped, int Tn, const float* stats, const float* gamma,
                    const float* beta, float* part, float* dW, float* dbias, hipStream_t st) {
    OtWgrad a;
    a.A = A; a.X = X; a.lda = M; a.ldx = grouped ? OT_FFN : K;
    a.grouped = grouped; a.K = grouped ? OT_CG : K; a.taps = grouped ? OT_TAPS : 1; a.Tn = Tn;
    a.stats = stats; a.gamma = gamma; a.beta = beta;
    a.part = part; a.M = M; a.stride = M * a.K * a.taps + M;
    a.N = g.N; a.slab_len = g.slab_len;
    const int KP = (a.K + 15) & ~15;
    const size_t lds = (size_t)(32 + a.taps * KP) * OT_LDT * sizeof(T);
    const dim3 grid(g.slabs, grouped ? OT_G : M / 32);
    if (xf == OT_X_PLAIN) NBSS_LAUNCH((ot_wgrad_kernel<T, OT_X_PLAIN>), grid, dim3(256), lds, st, a);
    else if (xf == OT_X_SILU) NBSS_LAUNCH((ot_wgrad_kernel<T, OT_X_SILU>), grid, dim3(256), lds, st, a);
    else NBSS_LAUNCH((ot_wgrad_kernel<T, OT_X_LN>), grid, dim3(256), lds, st, a);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    const int n1 = M * a.K * a.taps;
    NBSS_FOLD_LAUNCH(ot_fold_kernel, dim3((n1 + M + 255) / 256), dim3(256), 0, st, (const float*)part, g.slabs, a.stride, n1, dW, M, dbias);
    return NBSS_CHECK_LAUNCH();
}

// ---- sequencing ---------------------------------------------------------------------------------------------------------------------------------------
struct OtParams {
    const float *ln_w, *ln_b, *w1, *b1, *c1w, *c1b, *c2w, *c2b, *gn_w, *gn_b, *c3w, *c3b, *w2, *b2;
    bool ok() const { return ln_w && ln_b && w1 && b1 && c1w && c1b && c2w && c2b && gn_w && gn_b && c3w && c3b && w2 && b2; }
};
struct OtGrads {
    float *ln_w, *ln_b, *w1, *b1, *c1w, *c1b, *c2w, *c2b, *gn_w, *gn_b, *c3w, *c3b, *w2, *b2;
    bool ok() const { return ln_w && ln_b && w1 && b1 && c1w && c1b && c2w && c2b && gn_w && gn_b && c3w && c3b && w2 && b2; }
};
// the causal conv and its data gradient as tap-GEMMs: forward reads rows n - 2 .. n (centre = the last tap), the gradient rows n .. n + 2 of dy
static TapGemm ot_conv(const void* X, const void* Wp, const float* bias, void* Y, long N, int Tn, int center) {
    TapGemm p = gb_conv(X, Wp, bias, Y, N, OT_FFN, OT_G, OT_TAPS, 1, 1, Tn);
    p.center = center;
    return p;
}

template <class T>
static int ot_fwd(int B, int F, int Tn, const OtParams& P, const void* x, void* y, void* save, void* ws, hipStream_t st) {
    const OtGeom g = ot_geom(sizeof(T) == 2 ? NBSS_BF16 : NBSS_F32, B, F, Tn);
    const long N = g.N;
    char* W = (char*)ws;
    char* S = (char*)save;
    // without `save` (inference) the activations ping-pong between the two workspace tensors; the LayerNorm statistics, which the forward never reads
    // back, land where the GroupNorm partials are written later
    void* u = W + g.w_u;
    float* ln_stats = S ? (float*)(S + g.s_ln) : (float*)(W + g.w_gpart);
    float* gn_stats = S ? (float*)(S + g.s_gn) : (float*)(W + g.w_gfold);
    void* a1 = S ? S + g.s_a1 : W + g.w_g1;
    void* a2 = S ? S + g.s_a2 : W + g.w_g2;
    void* a3 = S ? S + g.s_a3 : W + g.w_g1;
    void* h4 = S ? S + g.s_h4 : W + g.w_g1;  // (element-wise from a3: in place)
    void* a4 = S ? S + g.s_a4 : W + g.w_g2;
    float* gpart = (float*)(W + g.w_gpart);
    const size_t slot = ws_align((size_t)OT_WSLOT * sizeof(T));
    void* wp[5];
    for (int i = 0; i < 5; ++i) wp[i] = W + g.w_wp + i * slot;
    int e;
    WPrepBatch<T> wb;
    wb.add(P.w1, wp[0], WP_LIN_FWD, 1, 1, OT_FFN, OT_H, OT_FFN, OT_H);
    wb.add(P.c1w, wp[1], WP_CONV_FWD, OT_G, OT_TAPS, OT_CG, OT_CG, 32, 32);
    wb.add(P.c2w, wp[2], WP_CONV_FWD, OT_G, OT_TAPS, OT_CG, OT_CG, 32, 32);
    wb.add(P.c3w, wp[3], WP_CONV_FWD, OT_G, OT_TAPS, OT_CG, OT_CG, 32, 32);
    wb.add(P.w2, wp[4], WP_LIN_FWD, 1, 1, OT_H, OT_FFN, OT_H, OT_FFN);
    if ((e = wb.launch(st))) return e;
    if ((e = gb_ln_fwd<T>(x, P.ln_w, P.ln_b, u, ln_stats, N, OT_H, st))) return e;
    TapGemm p = gb_lin(u, OT_H, wp[0], P.b1, a1, OT_FFN, N, OT_FFN, OT_H);
    if ((e = gb_gemm<T>(p, st))) return e;
    p = ot_conv(a1, wp[1], P.c1b, a2, N, Tn, OT_TAPS - 1);
    p.xact = 1;
    if ((e = gb_gemm<T>(p, st))) return e;
    p = ot_conv(a2, wp[2], P.c2b, a3, N, Tn, OT_TAPS - 1);
    p.xact = 1;
    if ((e = gb_gemm<T>(p, st))) return e;
    NBSS_LAUNCH((ot_gn_part_kernel<T>), dim3(ot_grid(N * OT_G)), dim3(256), 0, st, (const T*)a3, gpart, N);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH(ot_gn_fold_kernel, dim3(ot_grid((long)B * Tn * OT_G)), dim3(256), 0, st, (const float*)gpart, gn_stats, B, F, Tn);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH((ot_gn_apply_kernel<T>), dim3(ot_grid(N * (OT_FFN / 8))), dim3(256), 0, st, (const T*)a3, (const float*)gn_stats, P.gn_w, P.gn_b, (T*)h4, N, F, Tn);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    p = ot_conv(h4, wp[3], P.c3b, a4, N, Tn, OT_TAPS - 1);
    if ((e = gb_gemm<T>(p, st))) return e;
    p = gb_lin(a4, OT_FFN, wp[4], P.b2, y, OT_H, N, OT_H, OT_FFN);
    p.xact = 1;
    p.R = x; p.ldr = OT_H;
    return gb_gemm<T>(p, st);
}

template <class T>
static int ot_bwd(int B, int F, int Tn, const OtParams& P, const void* x, const void* save, const void* dy, void* dx, const OtGrads& D, void* ws, hipStream_t st) {
    const int dtype = sizeof(T) == 2 ? NBSS_BF16 : NBSS_F32;
    const OtGeom g = ot_geom(dtype, B, F, Tn);
    const long N = g.N;
    char* W = (char*)ws;
    const char* S = (const char*)save;
    const float* ln_stats = (const float*)(S + g.s_ln);
    const float* gn_stats = (const float*)(S + g.s_gn);
    const void *a1 = S + g.s_a1, *a2 = S + g.s_a2, *a3 = S + g.s_a3, *h4 = S + g.s_h4, *a4 = S + g.s_a4;
    void *du = W + g.w_u, *g1 = W + g.w_g1, *g2 = W + g.w_g2;
    float *gpart = (float*)(W + g.w_gpart), *gfold = (float*)(W + g.w_gfold), *part = (float*)(W + g.w_part);
    const size_t slot = ws_align((size_t)OT_WSLOT * sizeof(T));
    void* wp[5];
    for (int i = 0; i < 5; ++i) wp[i] = W + g.w_wp + i * slot;
    int e;
    WPrepBatch<T> wb;  // the transposed maps: outputs = the forward's inputs
    wb.add(P.w2, wp[4], WP_LIN_DGRAD, 1, 1, OT_FFN, OT_H, OT_FFN, OT_H);
    wb.add(P.c3w, wp[3], WP_CONV_DGRAD, OT_G, OT_TAPS, OT_CG, OT_CG, 32, 32);
    wb.add(P.c2w, wp[2], WP_CONV_DGRAD, OT_G, OT_TAPS, OT_CG, OT_CG, 32, 32);
    wb.add(P.c1w, wp[1], WP_CONV_DGRAD, OT_G, OT_TAPS, OT_CG, OT_CG, 32, 32);
    wb.add(P.w1, wp[0], WP_LIN_DGRAD, 1, 1, OT_H, OT_FFN, OT_H, OT_FFN);
    if ((e = wb.launch(st))) return e;
    // W2: dW2 += dy^T SiLU(a4);  da4 = (dy W2) SiLU'(a4)
    if ((e = ot_wgrad<T>(g, OT_X_SILU, dy, OT_H, a4, OT_FFN, 0, Tn, nullptr, nullptr, nullptr, part, D.w2, D.b2, st))) return e;
    TapGemm p = gb_lin(dy, OT_H, wp[4], nullptr, g1, OT_FFN, N, OT_FFN, OT_H);
    p.Dact = a4;
    if ((e = gb_gemm<T>(p, st))) return e;
    // conv3: dW += da4^T h4 (shifted);  dh4 = conv3^T(da4)
    if ((e = ot_wgrad<T>(g, OT_X_PLAIN, g1, OT_FFN, h4, OT_FFN, 1, Tn, nullptr, nullptr, nullptr, part, D.c3w, D.c3b, st))) return e;
    p = ot_conv(g1, wp[3], nullptr, g2, N, Tn, 0);
    p.bgs = 0;
    if ((e = gb_gemm<T>(p, st))) return e;
    // GroupNorm + SiLU: g2 becomes da3
    NBSS_LAUNCH((ot_gn_bwd_part_kernel<T>), dim3(ot_grid(N * OT_G)), dim3(256), 0, st, (const T*)a3, (const T*)g2, gn_stats, P.gn_w, P.gn_b, gpart, N, F, Tn);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH(ot_gn_bwd_fold_kernel, dim3(ot_grid((long)B * Tn * OT_G)), dim3(256), 0, st, (const float*)gpart, gfold, B, F, Tn);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH((ot_gn_bwd_apply_kernel<T>), dim3(g.slabs), dim3(OT_FFN), 0, st, (const T*)a3, (T*)g2, gn_stats, (const float*)gfold, P.gn_w, P.gn_b, part, N, F, Tn,
                g.slab_len);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_FOLD_LAUNCH(ot_fold_kernel, dim3((2 * OT_FFN + 255) / 256), dim3(256), 0, st, (const float*)part, g.slabs, 2 * OT_FFN, OT_FFN, D.gn_w, OT_FFN, D.gn_b);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    // conv2: dW += da3^T SiLU(a2);  da2 = conv2^T(da3) SiLU'(a2)
    if ((e = ot_wgrad<T>(g, OT_X_SILU, g2, OT_FFN, a2, OT_FFN, 1, Tn, nullptr, nullptr, nullptr, part, D.c2w, D.c2b, st))) return e;
    p = ot_conv(g2, wp[2], nullptr, g1, N, Tn, 0);
    p.bgs = 0;
    p.Dact = a2;
    if ((e = gb_gemm<T>(p, st))) return e;
    // conv1: dW += da2^T SiLU(a1);  da1 = conv1^T(da2) SiLU'(a1)
    if ((e = ot_wgrad<T>(g, OT_X_SILU, g1, OT_FFN, a1, OT_FFN, 1, Tn, nullptr, nullptr, nullptr, part, D.c1w, D.c1b, st))) return e;
    p = ot_conv(g1, wp[1], nullptr, g2, N, Tn, 0);
    p.bgs = 0;
    p.Dact = a1;
    if ((e = gb_gemm<T>(p, st))) return e;
    // W1: dW1 += da1^T LN(x);  du = da1 W1
    if ((e = ot_wgrad<T>(g, OT_X_LN, g2, OT_FFN, x, OT_H, 0, Tn, ln_stats, P.ln_w, P.ln_b, part, D.w1, D.b1, st))) return e;
    p = gb_lin(g2, OT_FFN, wp[0], nullptr, du, OT_H, N, OT_H, OT_FFN);
    if ((e = gb_gemm<T>(p, st))) return e;
    // LayerNorm, and the residual path
    NBSS_LAUNCH((ot_ln_bwd_kernel<T>), dim3(g.slabs), dim3(256), 4 * 2 * OT_H * sizeof(float), st, (const T*)du, (const T*)x, ln_stats, P.ln_w, (const T*)dy, (T*)dx, part, N, g.slab_len);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_FOLD_LAUNCH(ot_fold_kernel, dim3((2 * OT_H + 255) / 256), dim3(256), 0, st, (const float*)part, g.slabs, 2 * OT_H, OT_H, D.ln_w, OT_H, D.ln_b);
    return NBSS_CHECK_LAUNCH();
}

extern "C" {

int64_t nbss_online_tconvffn_train_save_bytes(int dtype, int B, int F, int T) {
    const int e = ot_check(dtype, B, F, T);
    return e ? e : (int64_t)ot_geom(dtype, B, F, T).save_total;
}
int64_t nbss_online_tconvffn_train_ws_bytes(int dtype, int B, int F, int T) {
    const int e = ot_check(dtype, B, F, T);
    return e ? e : (int64_t)ot_geom(dtype, B, F, T).ws_total;
}

int nbss_online_tconvffn_train_fwd(int dtype, int B, int F, int T, const float* ln_w, const float* ln_b, const float* w1, const float* b1, const float* c1w,
                                   const float* c1b, const float* c2w, const float* c2b, const float* gn_w, const float* gn_b, const float* c3w, const float* c3b,
                                   const float* w2, const float* b2, const void* x, void* y, void* save, void* ws, void* stream) {
    const int e = ot_check(dtype, B, F, T);
    if (e) return e;
    const OtParams P = {ln_w, ln_b, w1, b1, c1w, c1b, c2w, c2b, gn_w, gn_b, c3w, c3b, w2, b2};
    if (!P.ok() || !x || !y || !ws || x == y) return NBSS_EINVAL;
    return dtype == NBSS_BF16 ? ot_fwd<bf16_t>(B, F, T, P, x, y, save, ws, (hipStream_t)stream) : ot_fwd<float>(B, F, T, P, x, y, save, ws, (hipStream_t)stream);
}

int nbss_online_tconvffn_train_bwd(int dtype, int B, int F, int T, const float* ln_w, const float* ln_b, const float* w1, const float* b1, const float* c1w,
                                   const float* c1b, const float* c2w, const float* c2b, const float* gn_w, const float* gn_b, const float* c3w, const float* c3b,
                                   const float* w2, const float* b2, const void* x, const void* save, const void* dy, void* dx, float* d_ln_w, float* d_ln_b,
                                   float* d_w1, float* d_b1, float* d_c1w, float* d_c1b, float* d_c2w, float* d_c2b, float* d_gn_w, float* d_gn_b, float* d_c3w,
                                   float* d_c3b, float* d_w2, float* d_b2, void* ws, void* stream) {
    const int e = ot_check(dtype, B, F, T);
    if (e) return e;
    const OtParams P = {ln_w, ln_b, w1, b1, c1w, c1b, c2w, c2b, gn_w, gn_b, c3w, c3b, w2, b2};
    const OtGrads D = {d_ln_w, d_ln_b, d_w1, d_b1, d_c1w, d_c1b, d_c2w, d_c2b, d_gn_w, d_gn_b, d_c3w, d_c3b, d_w2, d_b2};
    if (!P.ok() || !D.ok() || !x || !save || !dy || !dx || !ws || dx == dy || dx == x) return NBSS_EINVAL;
    return dtype == NBSS_BF16 ? ot_bwd<bf16_t>(B, F, T, P, x, save, dy, dx, D, ws, (hipStream_t)stream)
                              : ot_bwd<float>(B, F, T, P, x, save, dy, dx, D, ws, (hipStream_t)stream);
}

}  // extern "C"
