// metrics.hip — the evaluation metrics of the reference's validation / test steps (SharedTrainer.py:163-182,239-248; models/utils/metrics.py:14-151,
// 192-218), which it takes from torchmetrics: signal_noise_ratio, scale_invariant_signal_distortion_ratio, scale_invariant_signal_noise_ratio,
// signal_distortion_ratio, and its own recover_scale.  Inputs and outputs are fp32; every sum is accumulated in fp64 (a product of two fp32 values is exact
// in fp64), in an order fixed by the shapes alone: chunks of samples per workgroup, a shuffle tree per wave, waves and chunks folded in index order.  No
// atomics: two calls give the same bits.  This file is built without -ffast-math (nbss_amd/build.py): no reassociation, no approximate division.
//
// SDR (torchmetrics signal_distortion_ratio = BSS-eval with a distortion filter of L taps, fp64): unit-norm both signals, r[k] = sum_n t[n] t[n+k],
// b[k] = sum_n t[n] p[n+k] (linear correlations, k < L), solve Toeplitz(r) x = b, coh = <b, x>, SDR = 10 log10(coh / (1 - coh)).  Three launches:
//   sdr_stats_kernel  one workgroup per pair: the means (NBSS_SDR_ZERO_MEAN, else 0) and the energies of the mean-free signals;
//   sdr_corr_kernel   one workgroup per (pair, chunk of samples): the chunk and a halo of L - 1 samples in LDS as fp64, every thread owns the lags
//                     tid and tid + 256; the raw signals are correlated, the normalisation scales r and b once afterwards;
//   sdr_solve_kernel  one wave per pair: folds the chunks' partial lag sums in chunk order, then Levinson-Durbin for a general right-hand side on four
//                     LDS-resident vectors (r, b, the prediction polynomial a, the solution x): one pair of wave reductions per order.
#include "launch.h"
#include "layout.h"

#define MT_MAXS 4
#define MT_CHUNKS 64
#define SDR_MAXL 512
#define SDR_TILE 1024
#define SDR_MAXCH 64
#define MT_EPS 1.1920928955078125e-07  // finfo(float32).eps, what torchmetrics adds to float32 inputs

NBSS_DEV double wave_sum64_d(double v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);  // every lane adds the same two values at every level: the same bits in all lanes
    return v;
}

NBSS_DEV double block_sum_d(double v, double* red) {  // red: one double of LDS per wave
    v = wave_sum64_d(v);
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    double s = 0.0;
    for (unsigned i = 0; i < (blockDim.x >> 6); ++i) s += red[i];
    return s;
}

NBSS_DEV double block_max_d(double v, double* red) {
    for (int m = 1; m < 64; m <<= 1) v = fmax(v, __shfl_xor(v, m));
    __syncthreads();
    if (lane_id() == 0) red[wave_id()] = v;
    __syncthreads();
    double s = red[0];
    for (unsigned i = 1; i < (blockDim.x >> 6); ++i) s = fmax(s, red[i]);
    return s;
}

NBSS_DEV double mt_db(double ratio) { return 10.0 * log10(ratio); }

// ---------------- SNR | SI-SDR | SI-SNR ----------------
// part[pair][chunk][6]: sum t, sum p, sum t^2, sum p^2, sum p t, sum (t - p)^2 (the distortion of SNR element by element, as torchmetrics forms it)
__global__ __launch_bounds__(256) void ratios_sums_kernel(int N, const float* __restrict__ p, const float* __restrict__ t, double* __restrict__ part) {
    NBSS_LDS(smem);
    double* red = reinterpret_cast<double*>(smem);
    const int pair = blockIdx.y, chunk = blockIdx.x;
    const int per = cdiv(N, (int)gridDim.x), n0 = chunk * per, n1 = n0 + per < N ? n0 + per : N;
    const float* pr = p + (size_t)pair * N;
    const float* tr = t + (size_t)pair * N;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n = n0 + (int)threadIdx.x; n < n1; n += (int)blockDim.x) {
        const double pv = (double)pr[n], tv = (double)tr[n], d = tv - pv;
        acc[0] += tv;
        acc[1] += pv;
        acc[2] += tv * tv;
        acc[3] += pv * pv;
        acc[4] += pv * tv;
        acc[5] += d * d;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const double s = block_sum_d(acc[q], red);
        if (threadIdx.x == 0) part[((size_t)pair * gridDim.x + chunk) * 6 + q] = s;
    }
}

// torchmetrics si_sdr from the dot products: alpha = (pt + eps) / (tt + eps); (|alpha t|^2 + eps) / (|alpha t - p|^2 + eps).  alpha is known only after
// the reduction, so the distortion is alpha^2 tt - 2 alpha pt + pp; in fp64 its cancellation error is 1e-16 tt, far below eps for any audible level
NBSS_DEV double mt_sisdr(double pt, double pp, double tt) {
    const double alpha = (pt + MT_EPS) / (tt + MT_EPS);
    const double num = alpha * alpha * tt;
    return mt_db((num + MT_EPS) / (fmax(num - 2.0 * alpha * pt + pp, 0.0) + MT_EPS));
}

// one thread per pair: out[pair][3] = SNR, SI-SDR, SI-SNR (= SI-SDR of the mean-free signals)
__global__ void ratios_finalize_kernel(int BS, int N, int nchunks, const double* __restrict__ part, float* __restrict__ out) {
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= BS) return;
    double s[6];
    for (int q = 0; q < 6; ++q) {
        double v = 0.0;
        for (int c = 0; c < nchunks; ++c) v += part[((size_t)pair * nchunks + c) * 6 + q];
        s[q] = v;
    }
    const double st = s[0], sp = s[1], tt = s[2], pp = s[3], pt = s[4], dd = s[5];
    const double mt = st / N, mp = sp / N;
    out[pair * 3 + 0] = (float)mt_db((tt + MT_EPS) / (dd + MT_EPS));
    out[pair * 3 + 1] = (float)mt_sisdr(pt, pp, tt);
    out[pair * 3 + 2] = (float)mt_sisdr(pt - N * mp * mt, fmax(pp - N * mp * mp, 0.0), fmax(tt - N * mt * mt, 0.0));
}

size_t signal_ratios_ws_bytes_impl(int B, int S) { return (size_t)B * S * MT_CHUNKS * 6 * sizeof(double); }

int signal_ratios_impl(int B, int S, int N, const float* p, const float* t, float* out, void* ws, hipStream_t st) {
    if (B < 1 || S < 1 || N < 1) return NBSS_EINVAL;
    if (S > MT_MAXS || B > 1024) return NBSS_EUNSUPPORTED;
    double* part = reinterpret_cast<double*>(ws);
    NBSS_LAUNCH(ratios_sums_kernel, dim3(MT_CHUNKS, B * S), dim3(256), 64, st, N, p, t, part);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH(ratios_finalize_kernel, dim3(cdiv(B * S, 256)), dim3(256), 0, st, B * S, N, MT_CHUNKS, (const double*)part, out);
    return NBSS_CHECK_LAUNCH();
}

// ---------------- SDR ----------------
// stats[pair][4]: mean t, mean p (0 without zero_mean), |t - mean t|^2, |p - mean p|^2
__global__ __launch_bounds__(256) void sdr_stats_kernel(int N, int zero_mean, const float* __restrict__ p, const float* __restrict__ t,
                                                        double* __restrict__ stats) {
    NBSS_LDS(smem);
    double* red = reinterpret_cast<double*>(smem);
    const int pair = blockIdx.x;
    const float* pr = p + (size_t)pair * N;
    const float* tr = t + (size_t)pair * N;
    double mt = 0.0, mp = 0.0;
    if (zero_mean) {
        double a = 0.0, b = 0.0;
        for (int n = (int)threadIdx.x; n < N; n += (int)blockDim.x) a += (double)tr[n], b += (double)pr[n];
        mt = block_sum_d(a, red) / N;
        mp = block_sum_d(b, red) / N;
    }
    double a = 0.0, b = 0.0;
    for (int n = (int)threadIdx.x; n < N; n += (int)blockDim.x) {
        const double tv = (double)tr[n] - mt, pv = (double)pr[n] - mp;
        a += tv * tv;
        b += pv * pv;
    }
    a = block_sum_d(a, red);
    b = block_sum_d(b, red);
    if (threadIdx.x == 0) {
        stats[pair * 4 + 0] = mt;
        stats[pair * 4 + 1] = mp;
        stats[pair * 4 + 2] = a;
        stats[pair * 4 + 3] = b;
    }
}

// part[pair][chunk][2][L]: the share of the samples n in [chunk per, (chunk + 1) per) in r[k] and b[k]; n + k >= N reads zeros
__global__ __launch_bounds__(256) void sdr_corr_kernel(int N, int L, int per, const float* __restrict__ p, const float* __restrict__ t,
                                                       const double* __restrict__ stats, double* __restrict__ part) {
    NBSS_LDS(smem);
    double* tw = reinterpret_cast<double*>(smem);  // [SDR_TILE + SDR_MAXL]
    double* pw = tw + SDR_TILE + SDR_MAXL;
    const int pair = blockIdx.y, chunk = blockIdx.x, tid = (int)threadIdx.x;
    const int c0 = chunk * per, c1 = c0 + per < N ? c0 + per : N;
    const float* pr = p + (size_t)pair * N;
    const float* tr = t + (size_t)pair * N;
    const double mt = stats[pair * 4 + 0], mp = stats[pair * 4 + 1];
    const int k0 = tid, k1 = tid + 256;
    const bool on0 = k0 < L, on1 = k1 < L;
    double r0 = 0.0, r1 = 0.0, b0 = 0.0, b1 = 0.0;
    for (int base = c0; base < c1; base += SDR_TILE) {
        const int nt = c1 - base < SDR_TILE ? c1 - base : SDR_TILE, W = nt + L - 1;
        __syncthreads();  // the previous tile has been read
        for (int i = tid; i < W; i += 256) {
            const int n = base + i;
            tw[i] = n < N ? (double)tr[n] - mt : 0.0;
            pw[i] = n < N ? (double)pr[n] - mp : 0.0;
        }
        __syncthreads();
        if (on1) {
#pragma unroll 4
            for (int n = 0; n < nt; ++n) {
                const double tv = tw[n];
                r0 += tv * tw[n + k0];
                b0 += tv * pw[n + k0];
                r1 += tv * tw[n + k1];
                b1 += tv * pw[n + k1];
            }
        } else if (on0) {
#pragma unroll 4
            for (int n = 0; n < nt; ++n) {
                const double tv = tw[n];
                r0 += tv * tw[n + k0];
                b0 += tv * pw[n + k0];
            }
        }
    }
    double* out = part + ((size_t)pair * gridDim.x + chunk) * 2 * L;
    if (on0) out[k0] = r0, out[L + k0] = b0;
    if (on1) out[k1] = r1, out[L + k1] = b1;
}

// One wave per pair.  Levinson-Durbin with a right-hand side: after order m, a[1..m] is the prediction polynomial of Toeplitz(r[0..m]) (a[0] = 1 is
// implicit) with error E, and x[0..m] solves the leading (m + 1) x (m + 1) system.  Order m needs mu = r[m] + sum_{i=1}^{m-1} a[i] r[m-i] and
// sum_{i=0}^{m-1} x[i] r[m-i] (both from the state before the step: one pair of reductions), then k = -mu / E, a'[i] = a[i] + k a[m-i], a'[m] = k,
// E' = E (1 - k^2), q = (b[m] - sum) / E', x'[i] = x[i] + q a'[m-i], x'[m] = q.  The update walks the index pairs (i, m - i): each pair is read and
// written by one lane, so a is updated in place.
__global__ __launch_bounds__(64) void sdr_solve_kernel(int L, int nchunks, const double* __restrict__ part, const double* __restrict__ stats,
                                                       float* __restrict__ sdr) {
    NBSS_LDS(smem);
    double* r = reinterpret_cast<double*>(smem);  // [4][SDR_MAXL]
    double* b = r + SDR_MAXL;
    double* a = b + SDR_MAXL;
    double* x = a + SDR_MAXL;
    const int pair = blockIdx.x, lane = (int)threadIdx.x;
    const double nt = fmax(sqrt(stats[pair * 4 + 2]), 1e-6), np = fmax(sqrt(stats[pair * 4 + 3]), 1e-6);
    for (int k = lane; k < L; k += 64) {
        double sr = 0.0, sb = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            const double* src = part + ((size_t)pair * nchunks + c) * 2 * L;
            sr += src[k];
            sb += src[L + k];
        }
        r[k] = sr / (nt * nt);
        b[k] = sb / (nt * np);
        a[k] = 0.0;
        x[k] = 0.0;
    }
    wave_lds_sync();
    double E = r[0];
    if (lane == 0) x[0] = b[0] / E;
    wave_lds_sync();
    for (int m = 1; m < L; ++m) {
        double pa = 0.0, px = 0.0;
        for (int i = lane; i < m; i += 64) {
            const double rv = r[m - i];
            px += x[i] * rv;
            if (i >= 1) pa += a[i] * rv;
        }
        pa = wave_sum64_d(pa);
        px = wave_sum64_d(px);
        wave_lds_sync();  // every lane has read the old a and x
        const double k = -(r[m] + pa) / E;
        E *= 1.0 - k * k;
        const double q = (b[m] - px) / E;
        for (int i = 1 + lane; 2 * i <= m; i += 64) {
            const int j = m - i;
            const double ai = a[i], aj = a[j];
            const double an = ai + k * aj, ajn = aj + k * ai;
            a[i] = an;
            x[i] += q * ajn;
            if (j != i) {
                a[j] = ajn;
                x[j] += q * an;
            }
        }
        if (lane == 0) {
            a[m] = k;
            x[0] += q * k;
            x[m] = q;
        }
        wave_lds_sync();
    }
    double coh = 0.0;
    for (int i = lane; i < L; i += 64) coh += b[i] * x[i];
    coh = wave_sum64_d(coh);
    if (lane == 0) sdr[pair] = (float)mt_db(coh / (1.0 - coh));
}

static int sdr_chunks(int N) {
    const int c = cdiv(N, SDR_TILE);
    return c < SDR_MAXCH ? c : SDR_MAXCH;
}

// ws: stats[B S][4] | part[B S][chunks][2][L]   (doubles)
size_t sdr_ws_bytes_impl(int B, int S, int N, int L) { return ((size_t)B * S * 4 + (size_t)B * S * sdr_chunks(N) * 2 * L) * sizeof(double); }

int sdr_impl(int B, int S, int N, int L, int flags, const float* p, const float* t, float* sdr, void* ws, hipStream_t st) {
    if (B < 1 || S < 1 || N < 1 || (flags & ~1)) return NBSS_EINVAL;
    if (L < 1 || L > SDR_MAXL || N < L || S > MT_MAXS || B > 1024) return NBSS_EUNSUPPORTED;
    double* stats = reinterpret_cast<double*>(ws);
    double* part = stats + (size_t)B * S * 4;
    const int nch = sdr_chunks(N), per = cdiv(N, nch);
    NBSS_LAUNCH(sdr_stats_kernel, dim3(B * S), dim3(256), 64, st, N, flags & 1, p, t, stats);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH(sdr_corr_kernel, dim3(nch, B * S), dim3(256), 2 * (SDR_TILE + SDR_MAXL) * sizeof(double), st, N, L, per, p, t, (const double*)stats, part);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH(sdr_solve_kernel, dim3(B * S), dim3(64), 4 * SDR_MAXL * sizeof(double), st, L, nch, (const double*)part, (const double*)stats, sdr);
    return NBSS_CHECK_LAUNCH();
}

// ---------------- recover_scale ----------------
// part[b][chunk][S S + 2 S]: G[i][j] = <p_i, p_j> (j >= i only), h[i] = <p_i, x>, max_n |p_i[n]|
template <int S>
__global__ __launch_bounds__(256) void scale_sums_kernel(int N, const float* __restrict__ p, const float* __restrict__ x, double* __restrict__ part) {
    NBSS_LDS(smem);
    double* red = reinterpret_cast<double*>(smem);
    constexpr int NQ = S * S + 2 * S;
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int per = cdiv(N, (int)gridDim.x), n0 = chunk * per, n1 = n0 + per < N ? n0 + per : N;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    for (int n = n0 + (int)threadIdx.x; n < n1; n += (int)blockDim.x) {
        double pv[S];
#pragma unroll
        for (int s = 0; s < S; ++s) pv[s] = (double)p[((size_t)b * S + s) * N + n];
        const double xv = (double)x[(size_t)b * N + n];
#pragma unroll
        for (int i = 0; i < S; ++i) {
#pragma unroll
            for (int j = i; j < S; ++j) acc[i * S + j] += pv[i] * pv[j];
            acc[S * S + i] += pv[i] * xv;
            acc[S * S + S + i] = fmax(acc[S * S + S + i], fabs(pv[i]));
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double s = q < S * S + S ? block_sum_d(acc[q], red) : block_max_d(acc[q], red);
        if (threadIdx.x == 0) part[((size_t)b * gridDim.x + chunk) * NQ + q] = s;
    }
}

// one thread per utterance: the normal equations G a = h (Gaussian elimination with partial pivoting), or with `together` the one scale
// sum(h) / sum(G) of the summed estimate; scale[b][s] = a_s, divided by max |a_s p_s| where norm_max is set and that exceeds 1
__global__ void scale_solve_kernel(int B, int S, int nchunks, int together, int norm_max, const double* __restrict__ part, double* __restrict__ scale) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int nq = S * S + 2 * S;
    double d[MT_MAXS * MT_MAXS + 2 * MT_MAXS];
    for (int q = 0; q < nq; ++q) {
        double v = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            const double w = part[((size_t)b * nchunks + c) * nq + q];
            v = q < S * S + S ? v + w : fmax(v, w);
        }
        d[q] = v;
    }
    double G[MT_MAXS][MT_MAXS + 1], a[MT_MAXS];
    for (int i = 0; i < S; ++i) {
        for (int j = 0; j < S; ++j) G[i][j] = j >= i ? d[i * S + j] : d[j * S + i];
        G[i][S] = d[S * S + i];
    }
    if (together) {
        double g = 0.0, h = 0.0;
        for (int i = 0; i < S; ++i) {
            for (int j = 0; j < S; ++j) g += G[i][j];
            h += G[i][S];
        }
        for (int i = 0; i < S; ++i) a[i] = h / g;
    } else {
        for (int c = 0; c < S; ++c) {
            int piv = c;
            for (int i = c + 1; i < S; ++i)
                if (fabs(G[i][c]) > fabs(G[piv][c])) piv = i;
            for (int j = c; j <= S; ++j) {
                const double tmp = G[c][j];
                G[c][j] = G[piv][j];
                G[piv][j] = tmp;
            }
            for (int i = c + 1; i < S; ++i) {
                const double f = G[i][c] / G[c][c];
                for (int j = c; j <= S; ++j) G[i][j] -= f * G[c][j];
            }
        }
        for (int i = S - 1; i >= 0; --i) {
            double v = G[i][S];
            for (int j = i + 1; j < S; ++j) v -= G[i][j] * a[j];
            a[i] = v / G[i][i];
        }
    }
    for (int i = 0; i < S; ++i) {
        const double mx = fabs(a[i]) * d[S * S + S + i];
        scale[b * S + i] = norm_max && mx > 1.0 ? a[i] / mx : a[i];
    }
}

__global__ void scale_apply_kernel(size_t total, int N, const float* __restrict__ p, const double* __restrict__ scale, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        out[i] = (float)((double)p[i] * scale[i / (size_t)N]);
}

// ws: part[B][MT_CHUNKS][S S + 2 S] | scale[B][S]   (doubles)
size_t recover_scale_ws_bytes_impl(int B, int S) { return ((size_t)B * MT_CHUNKS * (S * S + 2 * S) + (size_t)B * S) * sizeof(double); }

int recover_scale_impl(int B, int S, int N, int flags, const float* p, const float* x, float* out, void* ws, hipStream_t st) {
    if (B < 1 || S < 1 || N < 1 || (flags & ~3)) return NBSS_EINVAL;
    if (S > MT_MAXS || B > 1024) return NBSS_EUNSUPPORTED;
    double* part = reinterpret_cast<double*>(ws);
    double* scale = part + (size_t)B * MT_CHUNKS * (S * S + 2 * S);
    if (S == 1) NBSS_LAUNCH(scale_sums_kernel<1>, dim3(MT_CHUNKS, B), dim3(256), 64, st, N, p, x, part);
    else if (S == 2) NBSS_LAUNCH(scale_sums_kernel<2>, dim3(MT_CHUNKS, B), dim3(256), 64, st, N, p, x, part);
    else if (S == 3) NBSS_LAUNCH(scale_sums_kernel<3>, dim3(MT_CHUNKS, B), dim3(256), 64, st, N, p, x, part);
    else NBSS_LAUNCH(scale_sums_kernel<4>, dim3(MT_CHUNKS, B), dim3(256), 64, st, N, p, x, part);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH(scale_solve_kernel, dim3(cdiv(B, 256)), dim3(256), 0, st, B, S, MT_CHUNKS, flags & 1, (flags >> 1) & 1, (const double*)part, scale);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    const size_t total = (size_t)B * S * N;
    NBSS_LAUNCH(scale_apply_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0, st, total, N, p,
                (const double*)scale, out);
    return NBSS_CHECK_LAUNCH();
}
