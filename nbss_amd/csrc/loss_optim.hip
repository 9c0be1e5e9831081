// loss_optim.hip — uPIT negative SI-SDR loss (forward + gradient) and the fused clip + Adam step.
//
// Loss (models/io/loss.py:21-29,95-118 + torchmetrics si_sdr / pit, restated in oracle/loss_ref.py):
//   alpha = (<p,t> + eps) / (<t,t> + eps);  si_sdr = 10 log10((|alpha t|^2 + eps) / (|alpha t - p|^2 + eps)),
//   eps = finfo(float32).eps, zero_mean = False;  loss_b = min over speaker permutations pi of
//   -mean_s si_sdr(p_{pi(s)}, t_s);  loss = mean_b loss_b;  the gradient flows through the argmin only.
// Three launches: (1) all pairwise dot products as deterministic two-stage block reductions,
// (2) one thread per batch item enumerates the permutations and derives, for the winning one, the two
// scalars of d loss / d p_i = ct_i * t_{sel(i)} + cp_i * p_i, (3) an elementwise kernel applies them.
// The reference's other objectives (neg_snr, neg_sa_sdr, cc_mse; PIT or identity pairing) follow the same scheme further down: "the loss family".
//
// Optimizer (general_steps.py:243-271: torch.optim.Adam; Trainer gradient_clip_val=5, 'norm'):
// global L2 norm (two-stage reduction), clip coefficient min(1, max_norm / (norm + 1e-6)), Adam with
// bias correction; all 1.19 M parameters live in one flat fp32 buffer, so the whole update is one
// elementwise launch which also re-zeroes the gradient buffer for the next step.
#include "launch.h"
#include "layout.h"
#include "prof.h"

#define LS_MAXS 4
#define LS_CHUNKS 64

NBSS_DEV float block_sum_256(float v, float* red) {  // red: >= 4 floats of LDS
    v = wave_sum64(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    float s = 0.f;
    for (unsigned i = 0; i < (blockDim.x >> 6); ++i) s += red[i];
    return s;
}

// part[b][chunk][S*S + 2S]: <p_i,t_j> (i*S+j), <p_i,p_i>, <t_j,t_j>
__global__ __launch_bounds__(256) void sisdr_dots_kernel(int S, int N, const float* __restrict__ p, const float* __restrict__ t,
                                                         float* __restrict__ part) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);
    const int b = blockIdx.y, chunk = blockIdx.x, nq = S * S + 2 * S;
    const int per = cdiv(N, (int)gridDim.x), n0 = chunk * per, n1 = n0 + per < N ? n0 + per : N;
    float acc[LS_MAXS * LS_MAXS + 2 * LS_MAXS];
    for (int q = 0; q < nq; ++q) acc[q] = 0.f;
    for (int n = n0 + threadIdx.x; n < n1; n += blockDim.x) {
        float pv[LS_MAXS], tv[LS_MAXS];
        for (int s = 0; s < S; ++s) {
            pv[s] = p[((size_t)b * S + s) * N + n];
            tv[s] = t[((size_t)b * S + s) * N + n];
        }
        for (int i = 0; i < S; ++i) {
            for (int j = 0; j < S; ++j) acc[i * S + j] += pv[i] * tv[j];
            acc[S * S + i] += pv[i] * pv[i];
            acc[S * S + S + i] += tv[i] * tv[i];
        }
    }
    for (int q = 0; q < nq; ++q) {
        const float s = block_sum_256(acc[q], red);
        if (threadIdx.x == 0) part[((size_t)b * gridDim.x + chunk) * nq + q] = s;
    }
}

NBSS_DEV float sisdr_from_dots(float pt, float pp, float tt, float eps) {
    const float alpha = (pt + eps) / (tt + eps);
    const float num = alpha * alpha * tt + eps;
    const float den = alpha * alpha * tt - 2.f * alpha * pt + pp + eps;
    return 10.f * (__logf(num / den) * 0.4342944819032518f);
}

// one thread per batch item: PIT over S! permutations; coef[b][i] = {ct, cp, sel}; loss_b; perm[b][s]
__global__ void pit_finalize_kernel(int B, int S, int nchunks, const float* __restrict__ part, float* __restrict__ loss_b,
                                    int* __restrict__ perm_out, float* __restrict__ coef, float* __restrict__ loss_mean) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const float eps = 1.1920928955078125e-07f;
    const int nq = S * S + 2 * S;
    if (b < B) {
        float d[LS_MAXS * LS_MAXS + 2 * LS_MAXS];
        for (int q = 0; q < nq; ++q) {
            float s = 0.f;
            for (int c = 0; c < nchunks; ++c) s += part[((size_t)b * nchunks + c) * nq + q];
            d[q] = s;
        }
        float sd[LS_MAXS][LS_MAXS];
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) sd[i][j] = sisdr_from_dots(d[i * S + j], d[S * S + i], d[S * S + S + j], eps);
        // enumerate permutations in itertools.permutations order (what torchmetrics uses): perm[s] = prediction paired with target s
        int best[LS_MAXS], cur[LS_MAXS];
        float bestv = 3.0e38f;
        int nperm = 1;
        for (int s = 2; s <= S; ++s) nperm *= s;
        for (int pi = 0; pi < nperm; ++pi) {
            int avail[LS_MAXS], k = pi, fact = nperm;
            for (int s = 0; s < S; ++s) avail[s] = s;
            for (int s = 0; s < S; ++s) {
                fact /= (S - s);
                const int idx = k / fact;
                k %= fact;
                cur[s] = avail[idx];
                for (int e = idx; e < S - 1 - s; ++e) avail[e] = avail[e + 1];
            }
            float v = 0.f;
            for (int s = 0; s < S; ++s) v += sd[cur[s]][s];
            v = -v / S;
            if (v < bestv) {
                bestv = v;
                for (int s = 0; s < S; ++s) best[s] = cur[s];
            }
        }
        loss_b[b] = bestv;
        const float gscale = -(10.f * 0.4342944819032518f) / (float)(B * S);  // d loss / d si_sdr(pair) * d(10 log10)/d ln
        for (int s = 0; s < S; ++s) {
            const int i = best[s];
            perm_out[b * S + s] = i;
            const float pt = d[i * S + s], pp = d[S * S + i], tt = d[S * S + S + s];
            const float alpha = (pt + eps) / (tt + eps);
            const float num = alpha * alpha * tt + eps;
            const float den = alpha * alpha * tt - 2.f * alpha * pt + pp + eps;
            const float da = 1.f / (tt + eps);  // d alpha / d p = t * da
            const float a1 = 2.f * alpha * tt * da / num;
            const float d1 = ((2.f * alpha * tt - 2.f * pt) * da - 2.f * alpha) / den;
            const float d2 = 2.f / den;
            coef[(b * S + i) * 3 + 0] = gscale * (a1 - d1);
            coef[(b * S + i) * 3 + 1] = -gscale * d2;
            coef[(b * S + i) * 3 + 2] = (float)s;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // B is small: serial, deterministic mean (this kernel is launched with one block)
        float s = 0.f;
        for (int i = 0; i < B; ++i) s += loss_b[i];
        *loss_mean = s / B;
    }
}

__global__ void sisdr_grad_kernel(int BS, int S, int N, const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ coef,
                                  float* __restrict__ dp) {
    const size_t total = (size_t)BS * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t bi = i / N;
        const int n = (int)(i % N);
        const int b = (int)(bi / S);
        const float ct = coef[bi * 3], cp = coef[bi * 3 + 1];
        const int sel = (int)coef[bi * 3 + 2];
        dp[i] = ct * t[((size_t)b * S + sel) * N + n] + cp * p[i];
    }
}

// ws: part[B][LS_CHUNKS][nq] | loss_b[B] | coef[B*S*3]   (floats)
size_t pit_ws_floats(int B, int S) { return (size_t)B * LS_CHUNKS * (S * S + 2 * S) + B + (size_t)B * S * 3; }

int pit_sisdr_impl(int B, int S, int N, const float* p, const float* t, float* loss, int* perm, float* dp, float* ws, hipStream_t st) {
    if (S < 1 || S > LS_MAXS || B < 1 || B > 1024) return NBSS_EUNSUPPORTED;
    const int nq = S * S + 2 * S;
    float* part = ws;
    float* loss_b = part + (size_t)B * LS_CHUNKS * nq;
    float* coef = loss_b + B;
    ProfScope ps(PK_LOSS, st);
    NBSS_LAUNCH(sisdr_dots_kernel, dim3(LS_CHUNKS, B), dim3(256), 64, st, S, N, p, t, part);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH(pit_finalize_kernel, dim3(1), dim3(1024), 0, st, B, S, LS_CHUNKS, part, loss_b, perm, coef, loss);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    if (dp) {
        const size_t total = (size_t)B * S * N;
        NBSS_LAUNCH(sisdr_grad_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0, st, B * S, S, N, p, t, coef,
                    dp);
        e = NBSS_CHECK_LAUNCH();
    }
    return e;
}

// ---------------- the loss family: SI-SDR | SNR | SA-SDR | MSE, PIT or identity pairing ----------------
// models/io/loss.py:15-71,95-118 (torchmetrics snr / sa_sdr / pit restated; include/nbss_hip.h: nbss_pit_loss).  The same three launches.  Every
// kind is a function of the per-item table part[b][chunk][nq]: <p_i,t_j> (i*S+j), <p_i,p_i>, <t_j,t_j> and, for the kinds whose distortion is t - p
// itself (SNR, unscaled SA-SDR, MSE), D_ij = sum_n (p_i - t_j)^2 accumulated element by element as the reference does: tt - 2 pt + pp from fp32 dots
// carries an absolute error of a few 1e-6 tt, which is 0.1 dB at 40 dB SNR.  The scale-invariant kinds only know alpha after the reduction and use the
// dot form, as the SI-SDR kernel above does.  Every gradient is d loss / d p_i = ct_i * t_sel(i) + cp_i * p_i: sisdr_grad_kernel applies it.
enum { LK_SI_SDR = 0, LK_SNR = 1, LK_SA_SDR = 2, LK_MSE = 3 };
#define LF_PIT 1
#define LF_SCALE_INV 2

template <int V> NBSS_DEV void ls_load(const float* __restrict__ src, float* dst) {
    if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src);
        dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
    } else if constexpr (V == 2) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(src);
        dst[0] = v.x, dst[1] = v.y;
    } else {
        dst[0] = *src;
    }
}

// V floats per load (the host side checks that V divides N and that both bases are 4 V-byte aligned, so every row is); chunk bounds and the per-thread
// order are fixed by (N, V) alone: bitwise repeatable
template <int S, int V, bool DIRECT>
__global__ __launch_bounds__(256) void loss_dots_kernel(int N, const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ part) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);
    constexpr int NQ = S * S + 2 * S + (DIRECT ? S * S : 0);
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int nv = N / V, per = cdiv(nv, (int)gridDim.x), v0 = chunk * per, v1 = v0 + per < nv ? v0 + per : nv;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    for (int v = v0 + (int)threadIdx.x; v < v1; v += (int)blockDim.x) {
        float pv[S][V], tv[S][V];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            ls_load<V>(p + ((size_t)b * S + s) * N + (size_t)v * V, pv[s]);
            ls_load<V>(t + ((size_t)b * S + s) * N + (size_t)v * V, tv[s]);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
#pragma unroll
            for (int i = 0; i < S; ++i) {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    acc[i * S + j] += pv[i][e] * tv[j][e];
                    if constexpr (DIRECT) {
                        const float df = pv[i][e] - tv[j][e];
                        acc[S * S + 2 * S + i * S + j] += df * df;
                    }
                }
                acc[S * S + i] += pv[i][e] * pv[i][e];
                acc[S * S + S + i] += tv[i][e] * tv[i][e];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const float s = block_sum_256(acc[q], red);
        if (threadIdx.x == 0) part[((size_t)b * gridDim.x + chunk) * NQ + q] = s;
    }
}

// The finalize arithmetic of the family runs in double: one thread per item and a handful of divisions and logarithms, so it costs nothing, and the
// result is then the fp32 partial sums' error alone (a level near 40 dB leaves less than one fp32 step between torchmetrics' published digits).
NBSS_DEV double ls_db(double ratio) { return log(ratio) * 4.342944819032518; }  // 10 log10

NBSS_DEV double ls_sisdr(double pt, double pp, double tt, double eps) {
    const double alpha = (pt + eps) / (tt + eps);
    return ls_db((alpha * alpha * tt + eps) / (alpha * alpha * tt - 2.0 * alpha * pt + pp + eps));
}

// the loss of one pairing (cur[s] = estimate paired with target s) from the table d = pt[S*S] | pp[S] | tt[S] | D[S*S]
NBSS_DEV double loss_of_pairing(int kind, bool scale_inv, int S, int N, const double* d, const int* cur, double eps) {
    const double *pt = d, *pp = d + S * S, *tt = d + S * S + S, *D = d + S * S + 2 * S;
    double v = 0.0;
    if (kind == LK_SI_SDR) {
        for (int s = 0; s < S; ++s) v += ls_sisdr(pt[cur[s] * S + s], pp[cur[s]], tt[s], eps);
        return -v / S;
    }
    if (kind == LK_SNR) {
        for (int s = 0; s < S; ++s) v += ls_db((tt[s] + eps) / (D[cur[s] * S + s] + eps));
        return -v / S;
    }
    if (kind == LK_SA_SDR && scale_inv) {  // SI-SDR of the item's S signals laid end to end
        double PT = 0.0, PP = 0.0, TT = 0.0;
        for (int s = 0; s < S; ++s) PT += pt[cur[s] * S + s], PP += pp[s], TT += tt[s];
        return -ls_sisdr(PT, PP, TT, eps);
    }
    double TT = 0.0;
    for (int s = 0; s < S; ++s) v += D[cur[s] * S + s], TT += tt[s];
    if (kind == LK_SA_SDR) return -ls_db((TT + eps) / (v + eps));
    return v / ((double)S * (double)N);  // LK_MSE
}

// one thread per batch item, as pit_finalize_kernel: the pairing (all S! in itertools order, or the identity alone), loss_b, perm, coef[b][i] = {ct, cp, sel}
__global__ void loss_finalize_kernel(int kind, int flags, int B, int S, int N, int nq, int nchunks, const float* __restrict__ part,
                                     float* __restrict__ loss_b, int* __restrict__ perm_out, float* __restrict__ coef, float* __restrict__ loss_mean) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const double eps = 1.1920928955078125e-07;
    const bool scale_inv = flags & LF_SCALE_INV;
    if (b < B) {
        double d[2 * LS_MAXS * LS_MAXS + 2 * LS_MAXS];
        for (int q = 0; q < nq; ++q) {
            double s = 0.0;
            for (int c = 0; c < nchunks; ++c) s += (double)part[((size_t)b * nchunks + c) * nq + q];
            d[q] = s;
        }
        int best[LS_MAXS], cur[LS_MAXS];
        float bestv = 3.0e38f;
        int nperm = 1;
        if (flags & LF_PIT)
            for (int s = 2; s <= S; ++s) nperm *= s;
        for (int pi = 0; pi < nperm; ++pi) {  // pi = 0 is the identity
            int avail[LS_MAXS], k = pi, fact = 1;
            for (int s = 2; s <= S; ++s) fact *= s;
            for (int s = 0; s < S; ++s) avail[s] = s;
            for (int s = 0; s < S; ++s) {
                fact /= (S - s);
                const int idx = k / fact;
                k %= fact;
                cur[s] = avail[idx];
                for (int e = idx; e < S - 1 - s; ++e) avail[e] = avail[e + 1];
            }
            const float v = (float)loss_of_pairing(kind, scale_inv, S, N, d, cur, eps);  // compared as the fp32 values the reference compares
            if (v < bestv || pi == 0) {
                bestv = v;
                for (int s = 0; s < S; ++s) best[s] = cur[s];
            }
        }
        loss_b[b] = bestv;
        const double *pt = d, *pp = d + S * S, *tt = d + S * S + S, *D = d + S * S + 2 * S;
        const double k10 = 4.342944819032518;  // d(10 log10 x) = k10 dx / x
        // item-level sums of the source-aggregated kinds
        double PT = 0.0, PP = 0.0, TT = 0.0, DD = 0.0;
        for (int s = 0; s < S; ++s) {
            PT += pt[best[s] * S + s], PP += pp[s], TT += tt[s];
            if (!(kind == LK_SI_SDR || scale_inv)) DD += D[best[s] * S + s];
        }
        for (int s = 0; s < S; ++s) {
            const int i = best[s];
            perm_out[b * S + s] = i;
            double ct, cp;
            if (kind == LK_SI_SDR || (kind == LK_SA_SDR && scale_inv)) {
                const bool agg = kind == LK_SA_SDR;
                const double xpt = agg ? PT : pt[i * S + s], xpp = agg ? PP : pp[i], xtt = agg ? TT : tt[s];
                const double gscale = -k10 / (agg ? (double)B : (double)B * S);
                const double alpha = (xpt + eps) / (xtt + eps);
                const double num = alpha * alpha * xtt + eps;
                const double den = alpha * alpha * xtt - 2.0 * alpha * xpt + xpp + eps;
                const double da = 1.0 / (xtt + eps);  // d alpha / d p_i = t_s * da
                const double a1 = 2.0 * alpha * xtt * da / num;
                const double d1 = ((2.0 * alpha * xtt - 2.0 * xpt) * da - 2.0 * alpha) / den;
                ct = gscale * (a1 - d1);
                cp = -gscale * (2.0 / den);
            } else {  // the distortion is t - p: d loss / d p_i = cp * (p_i - t_s)
                if (kind == LK_SNR) cp = 2.0 * k10 / ((double)B * S * (D[i * S + s] + eps));
                else if (kind == LK_SA_SDR) cp = 2.0 * k10 / ((double)B * (DD + eps));
                else cp = 2.0 / ((double)B * (double)S * (double)N);
                ct = -cp;
            }
            coef[(b * S + i) * 3 + 0] = (float)ct;
            coef[(b * S + i) * 3 + 1] = (float)cp;
            coef[(b * S + i) * 3 + 2] = (float)s;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // launched with one block: serial, deterministic mean
        double s = 0.0;
        for (int i = 0; i < B; ++i) s += (double)loss_b[i];
        *loss_mean = (float)(s / B);
    }
}

static bool loss_direct(int kind, int flags) { return kind == LK_SNR || kind == LK_MSE || (kind == LK_SA_SDR && !(flags & LF_SCALE_INV)); }
static int loss_nq(int S, bool direct) { return S * S + 2 * S + (direct ? S * S : 0); }

// ws: part[B][LS_CHUNKS][nq] (sized for the kind's larger table) | loss_b[B] | coef[B*S*3]   (floats): the tail of pit_ws_floats
size_t pit_loss_ws_floats(int kind, int B, int S) {
    return (size_t)B * LS_CHUNKS * loss_nq(S, kind != LK_SI_SDR) + B + (size_t)B * S * 3;
}

template <int S, int V>
static void loss_dots_launch(bool direct, int B, int N, const float* p, const float* t, float* part, hipStream_t st) {
    if (direct) NBSS_LAUNCH((loss_dots_kernel<S, V, true>), dim3(LS_CHUNKS, B), dim3(256), 64, st, N, p, t, part);
    else NBSS_LAUNCH((loss_dots_kernel<S, V, false>), dim3(LS_CHUNKS, B), dim3(256), 64, st, N, p, t, part);
}

template <int S>
static void loss_dots_launch_s(int V, bool direct, int B, int N, const float* p, const float* t, float* part, hipStream_t st) {
    if (V == 4) loss_dots_launch<S, 4>(direct, B, N, p, t, part, st);
    else if (V == 2) loss_dots_launch<S, 2>(direct, B, N, p, t, part, st);
    else loss_dots_launch<S, 1>(direct, B, N, p, t, part, st);
}

int pit_loss_impl(int kind, int flags, int B, int S, int N, const float* p, const float* t, float* loss, int* perm, float* dp, float* ws,
                  hipStream_t st) {
    if (kind < LK_SI_SDR || kind > LK_MSE || (flags & ~(LF_PIT | LF_SCALE_INV)) || ((flags & LF_SCALE_INV) && kind != LK_SA_SDR)) return NBSS_EINVAL;
    if (S < 1 || S > LS_MAXS || B < 1 || B > 1024) return NBSS_EUNSUPPORTED;
    const bool direct = loss_direct(kind, flags);
    const int nq = loss_nq(S, direct);
    float* part = ws;
    float* loss_b = ws + (size_t)B * LS_CHUNKS * loss_nq(S, kind != LK_SI_SDR);
    float* coef = loss_b + B;
    const uintptr_t al = (uintptr_t)p | (uintptr_t)t;
    const int V = (N % 4 == 0 && al % 16 == 0) ? 4 : (N % 2 == 0 && al % 8 == 0) ? 2 : 1;
    ProfScope ps(PK_LOSS, st);
    if (S == 1) loss_dots_launch_s<1>(V, direct, B, N, p, t, part, st);
    else if (S == 2) loss_dots_launch_s<2>(V, direct, B, N, p, t, part, st);
    else if (S == 3) loss_dots_launch_s<3>(V, direct, B, N, p, t, part, st);
    else loss_dots_launch_s<4>(V, direct, B, N, p, t, part, st);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH(loss_finalize_kernel, dim3(1), dim3(1024), 0, st, kind, flags, B, S, N, nq, LS_CHUNKS, (const float*)part, loss_b, perm, coef, loss);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    if (dp) {
        const size_t total = (size_t)B * S * N;
        NBSS_LAUNCH(sisdr_grad_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0, st, B * S, S, N, p, t,
                    (const float*)coef, dp);
        e = NBSS_CHECK_LAUNCH();
    }
    return e;
}

// ---------------- clip + Adam ----------------
#define OP_BLOCKS 256

__global__ __launch_bounds__(256) void sumsq_kernel(size_t n, const float* __restrict__ g, float* __restrict__ part) {
    NBSS_LDS(smem);
    float* red = reinterpret_cast<float*>(smem);
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc += g[i] * g[i];
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// scal[0] = total grad norm, scal[1] = clip coefficient
__global__ void clip_coef_kernel(int nparts, const float* __restrict__ part, float max_norm, float gscale, float* __restrict__ scal) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s = 0.f;
        for (int i = 0; i < nparts; ++i) s += part[i];
        const float norm = sqrtf(s) * gscale;
        float coef = max_norm > 0.f ? max_norm / (norm + 1e-6f) : 1.f;
        if (coef > 1.f) coef = 1.f;
        scal[0] = norm;
        scal[1] = coef * gscale;
    }
}

__global__ void adam_kernel(size_t n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            const float* __restrict__ scal, float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2_sqrt,
                            int flags) {
    const float coef = scal[1];
    const bool zero_grad = flags & 1, decoupled = flags & 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float gi = g[i] * coef;
        float pi = p[i];
        if (decoupled) pi -= lr * wd * pi;       // torch.optim.AdamW: p *= 1 - lr * wd before the Adam update
        else if (wd != 0.f) gi += wd * pi;       // torch.optim.Adam: L2 term added to the gradient
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
        if (zero_grad) g[i] = 0.f;
    }
}

// the same update with the per-step scalars read from device memory: hyper = [lr, 1 - beta1^step, sqrt(1 - beta2^step)] (adam_hyper_impl) — a launch
// without per-step arguments, replayable from a HIP graph (engine.py: TrainStep.graph_step)
__global__ void adam_dev_kernel(size_t n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                const float* __restrict__ scal, const float* __restrict__ hyper, float beta1, float beta2, float eps, float wd, int flags) {
    const float coef = scal[1], lr = hyper[0], bc1 = hyper[1], bc2_sqrt = hyper[2];
    const bool zero_grad = flags & 1, decoupled = flags & 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float gi = g[i] * coef;
        float pi = p[i];
        if (decoupled) pi -= lr * wd * pi;
        else if (wd != 0.f) gi += wd * pi;
        const float mi = beta1 * m[i] + (1.f - beta1) * gi;
        const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = pi - (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
        if (zero_grad) g[i] = 0.f;
    }
}

// host side of the pair: the three floats exactly as clip_adam_impl computes them (same powf / sqrtf), so that a replayed step is bitwise the eager one
int adam_hyper_impl(int step, float lr, float beta1, float beta2, float* out) {
    if (step < 1 || !out) return NBSS_EINVAL;
    out[0] = lr;
    out[1] = 1.f - powf(beta1, (float)step);
    out[2] = sqrtf(1.f - powf(beta2, (float)step));
    return NBSS_OK;
}

int clip_adam_dev_impl(size_t n, float* p, float* g, float* m, float* v, float* scal, const float* hyper, float max_norm, float grad_scale, float beta1,
                       float beta2, float eps, float wd, int flags, hipStream_t st) {
    float* part = scal + 2;
    ProfScope ps(PK_ADAM, st);
    NBSS_LAUNCH(sumsq_kernel, dim3(OP_BLOCKS), dim3(256), 64, st, n, (const float*)g, part);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH(clip_coef_kernel, dim3(1), dim3(64), 0, st, OP_BLOCKS, (const float*)part, max_norm, grad_scale, scal);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH(adam_dev_kernel, dim3(1024), dim3(256), 0, st, n, p, g, m, v, (const float*)scal, hyper, beta1, beta2, eps, wd, flags);
    return NBSS_CHECK_LAUNCH();
}

int clip_adam_impl(size_t n, float* p, float* g, float* m, float* v, float* scal /* >= 2 + OP_BLOCKS floats */, float max_norm, float grad_scale,
                   float lr, float beta1, float beta2, float eps, float wd, int step, int flags, hipStream_t st) {
    if (step < 1) return NBSS_EINVAL;
    float* part = scal + 2;
    ProfScope ps(PK_ADAM, st);
    NBSS_LAUNCH(sumsq_kernel, dim3(OP_BLOCKS), dim3(256), 64, st, n, (const float*)g, part);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH(clip_coef_kernel, dim3(1), dim3(64), 0, st, OP_BLOCKS, (const float*)part, max_norm, grad_scale, scal);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    const float bc1 = 1.f - powf(beta1, (float)step), bc2s = sqrtf(1.f - powf(beta2, (float)step));
    NBSS_LAUNCH(adam_kernel, dim3(1024), dim3(256), 0, st, n, p, g, m, v, (const float*)scal, lr, beta1, beta2, eps, wd, bc1, bc2s, flags);
    return NBSS_CHECK_LAUNCH();
}
