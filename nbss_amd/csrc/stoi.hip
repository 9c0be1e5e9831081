// stoi.hip — short-time objective intelligibility (Taal et al., 2011) and its extended form (Jensen & Taal, 2016) of every pair (estimate s, target s):
// what the reference's test step takes from torchmetrics -> pystoi in CPU process pools.  The definition is the one of include/nbss_hip.h (parity with
// pystoi is not pinned).  Inputs and the result are fp32.  Six launches, the workspace between them:
//   stoi_taps_kernel      one workgroup: the Kaiser-windowed sinc of the p/q resampler in fp64 (I0 by its power series), normalised to sum p; h = [1]
//                         at 10 kHz.  The taps stay at the head of the workspace.
//   stoi_dft_kernel       w = hanning(258)[1:-1] and the windowed 512-point DFT of a 256-sample frame as MFMA A fragments: bins 0 .. 223 (the highest
//                         band ends at bin 219), one row tile of cosines and one of sines per 16 bins, D[bin][j] = w[j] cos | -sin (2 pi bin j / 512).
//   stoi_resample_kernel  one thread per output sample of both signals: out[m] = sum_k h[m q - k p + L] x[k], rising k, accumulated in fp64,
//                         rounded to fp32 once.
//   stoi_mask_kernel      one workgroup per pair, the only data-dependent stage: the energy of every clean frame in fp64 (a wave per frame, a shuffle
//                         tree), their maximum, the mask E_k > max - 40 and its prefix sum: kept[i] = the i-th kept frame, K of them.
//   stoi_bands_kernel     a workgroup owns 16 frames of the compacted signals of one pair, clean and estimate.  Frame m of the compacted signal is
//                         rebuilt from the kept frames m - 1, m, m + 1 that overlap it (the compacted signal is never stored), into LDS
//                         Z[2][16][260]; wave w multiplies the row tiles of bins 16 T .. 16 T + 15, T = w, w + 4, ... < 14, with both images
//                         (v_mfma_f32_16x16x4_f32, lane group kk owns j = 64 kk .. 64 kk + 63: one 16-byte LDS read and one 16-byte table read per
//                         4 K steps); a lane holds re and im of the same (bin, frame): |X|^2 goes to LDS P[2][224][17], then one thread per
//                         (signal, band, frame) sums its bins in rising order and takes the root.
//   stoi_final_kernel     one workgroup per pair, a thread per segment of 30 frames, fp64: the clipped correlation of every band (STOI) or the
//                         row- and column-normalised inner product (eSTOI); a thread adds its segments in rising order, the threads meet in a
//                         shuffle tree and the waves in index order.
// No atomics, every out[pair] is stored once, the order of every sum is fixed by N and fs (and, in the last kernel, by K): two calls give the same
// bits and an item does not depend on its batch.  Built without -ffast-math (nbss_amd/build.py).
#include <math.h>
#include "launch.h"
#include "layout.h"
#include "conv_common.h"

#define ST_MAXS 4
#define ST_MAXB 1024
#define ST_MAX_N (1 << 24)
#define ST_ITEMS 64          // pairs per grid pass of the per-pair kernels; a workgroup walks the others in steps of the grid
#define ST_FS 10000
#define ST_FRAME 256
#define ST_HOP 128
#define ST_NFFT 512
#define ST_BANDS 15
#define ST_SEG 30
#define ST_TILES 14          // row tiles of 16 bins
#define ST_BINS (16 * ST_TILES)
#define ST_ZS 260            // LDS row of one frame, in floats: the 16 frames of a B fragment start in distinct banks
#define ST_PS 17
#define ST_MAX_TAPS 592      // 2 L + 1 = 581 at 16 kHz, padded
#define ST_EPS 2.220446049250313e-16
#define ST_PI 3.14159265358979323846
#define ST_KS4 16            // groups of 4 K steps: 4 lane groups x 4 samples each
#define ST_TAB_FLOATS (ST_FRAME + ST_TILES * 2 * ST_KS4 * 64 * 4)

struct StoiBands {
    int lo[ST_BANDS], hi[ST_BANDS];
};

struct StoiPlan {
    int p, q, L, Nr, NrP, nf, nfP, pairs;
    size_t off_tab, off_res, off_energy, off_kept, off_K, off_bands, bytes;
};

NBSS_DEV double st_wave_sum(double v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

NBSS_DEV double st_win(int j) { return 0.5 - 0.5 * cos(2.0 * ST_PI * (double)(j + 1) / 257.0); }  // hanning(258)[1:-1]

NBSS_DEV double st_i0(double x) {
    double term = 1.0, sum = 1.0;
    const double y = 0.25 * x * x;
    for (int k = 1; k <= 60; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
    }
    return sum;
}

__global__ __launch_bounds__(256) void stoi_taps_kernel(int p, int q, int L, double* __restrict__ taps) {
    NBSS_LDS(smem);
    double* h = reinterpret_cast<double*>(smem);  // [2 L + 1], then the sum
    const int n = 2 * L + 1, tid = (int)threadIdx.x;
    const double fc = 1.0 / (2.0 * (double)(p > q ? p : q)), beta = 0.1102 * (60.0 - 8.7);
    for (int i = tid; i < n; i += 256) {
        double v = 1.0;
        if (L > 0) {
            const double t = (double)(i - L), r = t / (double)L, a = ST_PI * 2.0 * fc * t;
            const double kaiser = st_i0(beta * sqrt(fmax(1.0 - r * r, 0.0))) / st_i0(beta);
            v = kaiser * 2.0 * (double)p * fc * (i == L ? 1.0 : sin(a) / a);
        }
        h[i] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += h[i];
        h[n] = s;
    }
    __syncthreads();
    for (int i = tid; i < ST_MAX_TAPS; i += 256) taps[i] = i < n ? (double)p * h[i] / h[n] : 0.0;
}

// tab: [w 256][pack [T][re | im][ks4][lane][e]]: row bin = 16 T + li, j = 64 kk + 4 ks4 + e
__global__ void stoi_dft_kernel(float* __restrict__ tab) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < ST_TAB_FLOATS; i += (int)(gridDim.x * blockDim.x)) {
        if (i < ST_FRAME) {
            tab[i] = (float)st_win(i);
            continue;
        }
        const int r = i - ST_FRAME;
        const int e = r & 3, lane = (r >> 2) & 63, li = lane & 15, kk = lane >> 4, ks4 = (r >> 8) & (ST_KS4 - 1), im = (r >> 12) & 1, T = r >> 13;
        const int bin = 16 * T + li, j = 64 * kk + 4 * ks4 + e;
        const double ang = 2.0 * ST_PI * (double)((bin * j) % ST_NFFT) / ST_NFFT;
        tab[i] = (float)(st_win(j) * (im ? -sin(ang) : cos(ang)));
    }
}

// row = 2 pair + (0: target, 1: estimate); res [rows][NrP]
__global__ __launch_bounds__(256) void stoi_resample_kernel(int N, int Nr, int NrP, int p, int q, int L, const float* __restrict__ preds,
                                                            const float* __restrict__ target, const double* __restrict__ taps, float* __restrict__ res) {
    NBSS_LDS(smem);
    double* h = reinterpret_cast<double*>(smem);
    for (int i = (int)threadIdx.x; i < 2 * L + 1; i += 256) h[i] = taps[i];
    __syncthreads();
    const int row = (int)blockIdx.y, m = (int)(blockIdx.x * 256 + threadIdx.x);
    if (m >= Nr) return;
    const float* x = ((row & 1) ? preds : target) + (size_t)(row >> 1) * (size_t)N;
    const int a = m * q - L, b = m * q + L;
    int k0 = a >= 0 ? (a + p - 1) / p : 0, k1 = b / p;
    if (k1 > N - 1) k1 = N - 1;
    double acc = 0.0;
    for (int k = k0; k <= k1; ++k) acc += h[b - k * p] * (double)x[k];
    res[(size_t)row * NrP + m] = (float)acc;
}

__global__ __launch_bounds__(256) void stoi_mask_kernel(int pairs, int NrP, int nf, int nfP, const float* __restrict__ res, double* __restrict__ energy,
                                                        int* __restrict__ kept, int* __restrict__ Kout) {
    NBSS_LDS(smem);
    double* w = reinterpret_cast<double*>(smem);  // [256]
    double* red = w + ST_FRAME;                    // [4]
    int* cnt = reinterpret_cast<int*>(red + 4);    // [257]
    const int tid = (int)threadIdx.x, lane = lane_id(), wv = wave_id();
    w[tid] = st_win(tid);
    for (int pair = (int)blockIdx.x; pair < pairs; pair += (int)gridDim.x) {
        __syncthreads();
        const float* x = res + (size_t)(2 * pair) * NrP;
        double* E = energy + (size_t)pair * nf;
        int* kp = kept + (size_t)pair * nfP;
        double mx = -INFINITY;
        for (int k = wv; k < nf; k += 4) {
            double s = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double v = w[4 * lane + e] * (double)x[ST_HOP * k + 4 * lane + e];
                s += v * v;
            }
            s = st_wave_sum(s);
            const double db = 20.0 * log10(sqrt(s) + ST_EPS);
            if (lane == 0) E[k] = db;
            mx = fmax(mx, db);
        }
        if (lane == 0) red[wv] = mx;
        __syncthreads();  // E and red are written
        const double thr = fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) - 40.0;
        const int per = cdiv(nf, 256), k0 = tid * per, k1 = k0 + per < nf ? k0 + per : nf;
        int c = 0;
        for (int k = k0; k < k1; ++k) c += E[k] > thr ? 1 : 0;
        cnt[tid] = c;
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int i = 0; i < 256; ++i) {
                const int v = cnt[i];
                cnt[i] = s;
                s += v;
            }
            cnt[256] = s;
        }
        __syncthreads();
        int o = cnt[tid];
        for (int k = k0; k < k1; ++k)
            if (E[k] > thr) kp[o++] = k;
        if (tid == 0) Kout[pair] = cnt[256];
    }
}

// bands [pair][signal][band][nfP]: the one-third-octave magnitudes of the K - 1 frames of the compacted signals
__global__ __launch_bounds__(256) void stoi_bands_kernel(int pairs, int NrP, int nfP, StoiBands bd, const float* __restrict__ res, const float* __restrict__ tab,
                                                         const int* __restrict__ kept, const int* __restrict__ Kin, float* __restrict__ bands) {
    NBSS_LDS(smem);
    float* Z = reinterpret_cast<float*>(smem);  // [2][16][ST_ZS]
    float* P = Z + 2 * 16 * ST_ZS;              // [2][ST_BINS][ST_PS]
    const float* win = tab;
    const f32x4* Dp = reinterpret_cast<const f32x4*>(tab + ST_FRAME);
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = wave_id_u(), li = lane & 15, kk = lane >> 4;
    const int m0 = 16 * (int)blockIdx.x;
    for (int pair = (int)blockIdx.y; pair < pairs; pair += (int)gridDim.y) {
        const int Mf = Kin[pair] - 1;  // frames of the compacted signal
        if (m0 >= Mf) continue;        // the whole workgroup
        __syncthreads();               // the previous item's readers are done
        const int* kp = kept + (size_t)pair * nfP;
        for (int e = tid; e < 2 * 16 * ST_FRAME; e += 256) {
            const int sig = e >> 12, f = (e >> 8) & 15, j = e & 255, m = m0 + f;
            float v = 0.f;
            if (m < Mf) {
                const float* x = res + (size_t)(2 * pair + sig) * NrP;
                const float own = win[j] * x[ST_HOP * kp[m] + j];
                if (j < ST_HOP) v = m >= 1 ? win[j + ST_HOP] * x[ST_HOP * kp[m - 1] + ST_HOP + j] + own : own;
                else v = own + win[j - ST_HOP] * x[ST_HOP * kp[m + 1] + j - ST_HOP];
            }
            Z[(sig * 16 + f) * ST_ZS + j] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int T = wv; T < ST_TILES; T += 4) {
            f32x4 re[2] = {F32X4_ZERO, F32X4_ZERO}, im[2] = {F32X4_ZERO, F32X4_ZERO};
            const f32x4* pr = Dp + (size_t)(2 * T) * ST_KS4 * 64 + lane;
            const f32x4* pi = pr + ST_KS4 * 64;
            const float* pb = Z + li * ST_ZS + 64 * kk;
#pragma unroll 2
            for (int ks4 = 0; ks4 < ST_KS4; ++ks4) {
                const f32x4 ar = pr[ks4 * 64], ai = pi[ks4 * 64];
#pragma unroll
                for (int sig = 0; sig < 2; ++sig) {
                    const f32x4 x4 = *reinterpret_cast<const f32x4*>(pb + sig * 16 * ST_ZS + 4 * ks4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        re[sig] = conv_mfma(ar[e], x4[e], re[sig]);
                        im[sig] = conv_mfma(ai[e], x4[e], im[sig]);
                    }
                }
            }
            // the lane holds bins 16 T + 4 kk + (0 .. 3) of frame li
#pragma unroll
            for (int sig = 0; sig < 2; ++sig)
#pragma unroll
                for (int r = 0; r < 4; ++r) P[(sig * ST_BINS + 16 * T + 4 * kk + r) * ST_PS + li] = re[sig][r] * re[sig][r] + im[sig][r] * im[sig][r];
        }
        __syncthreads();
        for (int e = tid; e < 2 * ST_BANDS * 16; e += 256) {
            const int f = e & 15, band = (e >> 4) % ST_BANDS, sig = e / (16 * ST_BANDS);
            if (m0 + f >= Mf) continue;
            float s = 0.f;
            for (int b = bd.lo[band]; b < bd.hi[band]; ++b) s += P[(sig * ST_BINS + b) * ST_PS + f];
            bands[((size_t)(2 * pair + sig) * ST_BANDS + band) * nfP + m0 + f] = sqrtf(s);
        }
    }
}

template <bool EXT>
NBSS_DEV double stoi_segment(const float* __restrict__ X, const float* __restrict__ Y, int nfP, int seg) {
    if (!EXT) {
        const double clip = 1.0 + pow(10.0, 15.0 / 20.0);
        double total = 0.0;
        for (int band = 0; band < ST_BANDS; ++band) {
            const float* xr = X + (size_t)band * nfP + seg;
            const float* yr = Y + (size_t)band * nfP + seg;
            double x[ST_SEG], y[ST_SEG], xx = 0.0, yy = 0.0;
#pragma unroll
            for (int n = 0; n < ST_SEG; ++n) {
                x[n] = (double)xr[n];
                y[n] = (double)yr[n];
                xx += x[n] * x[n];
                yy += y[n] * y[n];
            }
            const double alpha = sqrt(xx) / (sqrt(yy) + ST_EPS);
            double sx = 0.0, sy = 0.0;
#pragma unroll
            for (int n = 0; n < ST_SEG; ++n) {
                y[n] = fmin(alpha * y[n], x[n] * clip);
                sx += x[n];
                sy += y[n];
            }
            const double mx = sx / ST_SEG, my = sy / ST_SEG;
            double cxx = 0.0, cyy = 0.0, cxy = 0.0;
#pragma unroll
            for (int n = 0; n < ST_SEG; ++n) {
                const double a = x[n] - mx, b = y[n] - my;
                cxx += a * a;
                cyy += b * b;
                cxy += a * b;
            }
            total += cxy / ((sqrt(cxx) + ST_EPS) * (sqrt(cyy) + ST_EPS));
        }
        return total;
    } else {
        double mx[ST_BANDS], ix[ST_BANDS], my[ST_BANDS], iy[ST_BANDS];
        for (int band = 0; band < ST_BANDS; ++band) {
            const float* xr = X + (size_t)band * nfP + seg;
            const float* yr = Y + (size_t)band * nfP + seg;
            double sx = 0.0, sy = 0.0;
            for (int n = 0; n < ST_SEG; ++n) sx += (double)xr[n], sy += (double)yr[n];
            sx /= ST_SEG, sy /= ST_SEG;
            double cxx = 0.0, cyy = 0.0;
            for (int n = 0; n < ST_SEG; ++n) {
                const double a = (double)xr[n] - sx, b = (double)yr[n] - sy;
                cxx += a * a;
                cyy += b * b;
            }
            mx[band] = sx, my[band] = sy;
            ix[band] = 1.0 / (sqrt(cxx) + ST_EPS), iy[band] = 1.0 / (sqrt(cyy) + ST_EPS);
        }
        double total = 0.0;
        for (int n = 0; n < ST_SEG; ++n) {
            double x[ST_BANDS], y[ST_BANDS], sx = 0.0, sy = 0.0;
            for (int band = 0; band < ST_BANDS; ++band) {
                x[band] = ((double)X[(size_t)band * nfP + seg + n] - mx[band]) * ix[band];
                y[band] = ((double)Y[(size_t)band * nfP + seg + n] - my[band]) * iy[band];
                sx += x[band];
                sy += y[band];
            }
            sx /= ST_BANDS, sy /= ST_BANDS;
            double cxx = 0.0, cyy = 0.0, cxy = 0.0;
            for (int band = 0; band < ST_BANDS; ++band) {
                const double a = x[band] - sx, b = y[band] - sy;
                cxx += a * a;
                cyy += b * b;
                cxy += a * b;
            }
            total += cxy / ((sqrt(cxx) + ST_EPS) * (sqrt(cyy) + ST_EPS));
        }
        return total;
    }
}

template <bool EXT>
__global__ __launch_bounds__(256) void stoi_final_kernel(int pairs, int nfP, const float* __restrict__ bands, const int* __restrict__ Kin,
                                                         float* __restrict__ out) {
    NBSS_LDS(smem);
    double* red = reinterpret_cast<double*>(smem);  // [4]
    const int tid = (int)threadIdx.x;
    for (int pair = (int)blockIdx.x; pair < pairs; pair += (int)gridDim.x) {
        const int M = Kin[pair] - 1 - ST_SEG + 1;  // segments
        if (M < 1) {
            if (tid == 0) out[pair] = 1e-5f;
            continue;
        }
        const float* X = bands + (size_t)(2 * pair) * ST_BANDS * nfP;
        const float* Y = X + (size_t)ST_BANDS * nfP;
        double acc = 0.0;
        for (int seg = tid; seg < M; seg += 256) acc += stoi_segment<EXT>(X, Y, nfP, seg);
        acc = st_wave_sum(acc);
        __syncthreads();
        if (lane_id() == 0) red[wave_id()] = acc;
        __syncthreads();
        if (tid == 0) out[pair] = (float)((red[0] + red[1] + red[2] + red[3]) / ((double)(EXT ? ST_SEG : ST_BANDS) * (double)M));
    }
}

// ---------------- host side ----------------
static size_t st_align(size_t v) { return (v + 15) & ~(size_t)15; }

// 0, or the error code
static int stoi_plan(int B, int S, int N, int fs, StoiPlan* pl) {
    if (B < 1 || S < 1 || N < 1) return NBSS_EINVAL;
    if (S > ST_MAXS || B > ST_MAXB || N > ST_MAX_N) return NBSS_EUNSUPPORTED;
    if (fs == 8000) pl->p = 5, pl->q = 4;
    else if (fs == 16000) pl->p = 5, pl->q = 8;
    else if (fs == ST_FS) pl->p = 1, pl->q = 1;
    else return NBSS_EUNSUPPORTED;
    const int mx = pl->p > pl->q ? pl->p : pl->q;
    pl->L = mx == 1 ? 0 : (int)ceil((60.0 - 8.0) / (28.714 * (1.0 / (2.0 * mx)) / 10.0));
    if (2 * pl->L + 1 > ST_MAX_TAPS - 1) return NBSS_EUNSUPPORTED;
    pl->Nr = (int)(((int64_t)N * pl->p + pl->q - 1) / pl->q);
    if (pl->Nr < ST_FRAME + 1) return NBSS_EUNSUPPORTED;
    pl->NrP = (pl->Nr + 3) & ~3;
    pl->nf = cdiv(pl->Nr - ST_FRAME, ST_HOP);  // starts 0, 128, ... < Nr - 256
    pl->nfP = (pl->nf + 3) & ~3;
    pl->pairs = B * S;
    const size_t pairs = (size_t)pl->pairs;
    size_t o = 0;
    o += st_align(ST_MAX_TAPS * sizeof(double));
    pl->off_tab = o, o += st_align((size_t)ST_TAB_FLOATS * sizeof(float));
    pl->off_res = o, o += st_align(pairs * 2 * pl->NrP * sizeof(float));
    pl->off_energy = o, o += st_align(pairs * pl->nf * sizeof(double));
    pl->off_kept = o, o += st_align(pairs * pl->nfP * sizeof(int));
    pl->off_K = o, o += st_align(pairs * sizeof(int));
    pl->off_bands = o, o += st_align(pairs * 2 * ST_BANDS * pl->nfP * sizeof(float));
    pl->bytes = o;
    return 0;
}

// band k sums the bins [argmin_j (f_j - low_k)^2, argmin_j (f_j - high_k)^2), f_j = j 10000 / 512, j = 0 .. 256
static int stoi_band_edges(StoiBands* bd) {
    for (int k = 0; k < ST_BANDS; ++k) {
        const double edge[2] = {150.0 * pow(2.0, (2 * k - 1) / 6.0), 150.0 * pow(2.0, (2 * k + 1) / 6.0)};
        int idx[2];
        for (int s = 0; s < 2; ++s) {
            double best = INFINITY;
            idx[s] = 0;
            for (int j = 0; j <= ST_NFFT / 2; ++j) {
                const double d = (double)j * ((double)ST_FS / ST_NFFT) - edge[s], d2 = d * d;
                if (d2 < best) best = d2, idx[s] = j;
            }
        }
        if (idx[1] > ST_BINS) return NBSS_EUNSUPPORTED;
        bd->lo[k] = idx[0], bd->hi[k] = idx[1];
    }
    return 0;
}

int64_t stoi_ws_bytes_impl(int B, int S, int N, int fs) {
    StoiPlan pl;
    const int e = stoi_plan(B, S, N, fs, &pl);
    return e ? (int64_t)e : (int64_t)pl.bytes;
}

int stoi_impl(int B, int S, int N, int fs, int flags, const float* preds, const float* target, float* out, void* ws, hipStream_t st) {
    if (flags & ~1) return NBSS_EINVAL;
    StoiPlan pl;
    StoiBands bd;
    int e = stoi_plan(B, S, N, fs, &pl);
    if (e || (e = stoi_band_edges(&bd))) return e;
    char* base = reinterpret_cast<char*>(ws);
    double* taps = reinterpret_cast<double*>(base);
    float* tab = reinterpret_cast<float*>(base + pl.off_tab);
    float* res = reinterpret_cast<float*>(base + pl.off_res);
    double* energy = reinterpret_cast<double*>(base + pl.off_energy);
    int* kept = reinterpret_cast<int*>(base + pl.off_kept);
    int* K = reinterpret_cast<int*>(base + pl.off_K);
    float* bands = reinterpret_cast<float*>(base + pl.off_bands);
    const int pairs = pl.pairs, items = pairs < ST_ITEMS ? pairs : ST_ITEMS;
    const size_t tap_lds = (size_t)(2 * pl.L + 2) * sizeof(double);
    NBSS_LAUNCH(stoi_taps_kernel, dim3(1), dim3(256), tap_lds, st, pl.p, pl.q, pl.L, taps);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH(stoi_dft_kernel, dim3(256), dim3(256), 0, st, tab);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH(stoi_resample_kernel, dim3(cdiv(pl.Nr, 256), 2 * pairs), dim3(256), tap_lds, st, N, pl.Nr, pl.NrP, pl.p, pl.q, pl.L, preds, target,
                (const double*)taps, res);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH(stoi_mask_kernel, dim3(items), dim3(256), (ST_FRAME + 4) * sizeof(double) + 260 * sizeof(int), st, pairs, pl.NrP, pl.nf, pl.nfP,
                (const float*)res, energy, kept, K);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    if (pl.nf > 1) {  // one kept frame at most otherwise: no frame of the compacted signal
        NBSS_LAUNCH(stoi_bands_kernel, dim3(cdiv(pl.nf - 1, 16), items), dim3(256), (2 * 16 * ST_ZS + 2 * ST_BINS * ST_PS) * sizeof(float), st, pairs, pl.NrP,
                    pl.nfP, bd, (const float*)res, (const float*)tab, (const int*)kept, (const int*)K, bands);
        if ((e = NBSS_CHECK_LAUNCH())) return e;
    }
    if (flags & 1) NBSS_LAUNCH(stoi_final_kernel<true>, dim3(items), dim3(256), 64, st, pairs, pl.nfP, (const float*)bands, (const int*)K, out);
    else NBSS_LAUNCH(stoi_final_kernel<false>, dim3(items), dim3(256), 64, st, pairs, pl.nfP, (const float*)bands, (const int*)K, out);
    return NBSS_CHECK_LAUNCH();
}
