// online_mamba_train.hip — the core of a Mamba block of the OnlineSpatialNet ('mamba(16,4)' at width 96) for TRAINING: what models/arch/base/mamba.py
// computes between in_proj and out_proj (Mamba.core), forward and backward, for E = 192 channels, N = 16 states, a causal depthwise convolution of K = 4
// taps and dt rank R = 6.  Written from the published equations (Gu & Dao 2023); all arithmetic fp32 in either stream dtype.
//
// Per sequence, with xz_t = (xr_t, z_t) [384] and the parameters cw [192][4], cb [192], wx [38][192], wdt [192][6], bdt [192], A_log [192][16], D [192]:
//   xc_t[e]  = SiLU(cb[e] + sum_k cw[e][k] xr_{t-3+k}[e])                 zeros before frame 0
//   (dtr_t [6], B_t [16], C_t [16]) = wx xc_t                             the 38 x_proj outputs of a frame
//   dt_t[e]  = softplus(bdt[e] + sum_r wdt[e][r] dtr_t[r])                A[e][n] = -exp(A_log[e][n])
//   h_t[e][n] = exp(dt_t[e] A[e][n]) h_{t-1}[e][n] + dt_t[e] B_t[n] xc_t[e]        h_{-1} = 0
//   out_t[e] = (sum_n C_t[n] h_t[e][n] + D[e] xc_t[e]) SiLU(z_t[e])
//
// One workgroup of 192 threads owns a sequence (a grid-stride loop over the BF sequences, at most MB_GRID_CAP workgroups); thread e is channel e and keeps
// its 16 states in registers.  The frames are walked in runs of MB_CKPT = 8: the run's xc rows go to LDS, the 38 x_proj outputs of each of its frames are
// dot products over those rows against the x_proj matrix (LDS, rows of 193 floats), and B_t / C_t are then read from LDS by every channel.
//
// The backward does not get h of every frame (16 x an activation).  SAVED by the forward: h at the START of every run of 8 frames, [BF][ceil(T/8)][16][192]
// fp32 (two fp32 activation tensors' worth at 8 frames: at 16 the recomputed states of the 192 channels, 16 x 16 x 192 fp32 = 192 KB, would not fit the
// 160 KB of LDS), and the x_proj outputs [BF][T][38] fp32.  RECOMPUTED per run, in reverse run order: xc, dt, and the state BEFORE each frame of the run,
// into LDS (96 KB); then the reverse recurrence over the run's frames, which carries dh, never divides by exp(dt A), and leaves per frame the gradient of
// the 38 x_proj outputs — sums over the 192 channels, folded in a fixed order through LDS (four partial sums of 48 channels, then their sum); then the
// x_proj and convolution backward of the run's frames.  Each thread carries its channel's 67 parameter-gradient sums (conv 4 + 1, x_proj 38, dt_proj 6 + 1,
// A 16, D 1) across the sequences of its workgroup and writes them as one partial row per workgroup; a second launch folds the partial rows in workgroup
// order.  No atomics, every sum in a fixed order: two calls give the same bits, and a sequence's rows of out and dxz do not depend on the other sequences.
#include "gb.h"
#include "mamba_core.h"  // MB_E, MB_N, MB_K, MB_R, MB_J, MB_JL; MbChan, mb_conv, mb_dt, mb_scan_frame (shared with online_mamba_step.hip)

#define MB_CKPT 8               // frames per run: the forward saves h at the start of each
#define MB_THREADS MB_E
#define MB_GRID_CAP 512         // workgroups per launch; more sequences are walked by the grid-stride loop
#define MB_LW 193               // row of the x_proj matrix in LDS
#define MB_SLOTS 67             // parameter-gradient sums per channel: cw 0..3, cb 4, wx 5..42, wdt 43..48, bdt 49, A_log 50..65, D 66
#define MB_STATE (MB_N * MB_E)  // floats of one checkpoint
// LDS of the forward (floats)
#define MF_O_WX 0
#define MF_O_XC (MF_O_WX + MB_J * MB_LW)
#define MF_O_DBC (MF_O_XC + MB_CKPT * MB_E)
#define MF_FLOATS (MF_O_DBC + MB_CKPT * MB_JL)
// LDS of the backward (floats)
#define MW_O_HS 0                                       // [8][16][192]: h before each frame of the run; after a frame's step its dB contributions
#define MW_O_XR (MW_O_HS + MB_CKPT * MB_STATE)          // [8 + 3][192]: xr of the run and of the three frames before it
#define MW_O_XPRE (MW_O_XR + (MB_CKPT + 3) * MB_E)      // [8][192]: the convolution output before its SiLU
#define MW_O_XC (MW_O_XPRE + MB_CKPT * MB_E)            // [8][192]
#define MW_O_DT (MW_O_XC + MB_CKPT * MB_E)              // [8][192]: the channel's d xc of each frame without the x_proj part
#define MW_O_DBC (MW_O_DT + MB_CKPT * MB_E)             // [8][40]: the saved x_proj outputs
#define MW_O_DDBC (MW_O_DBC + MB_CKPT * MB_JL)          // [8][40]: their gradients
#define MW_O_REDC (MW_O_DDBC + MB_CKPT * MB_JL)         // [16][192]: dC contributions of the frame
#define MW_O_REDR (MW_O_REDC + MB_N * MB_E)             // [6][192]: d dt_r contributions of the frame
#define MW_O_PART (MW_O_REDR + MB_R * MB_E)             // [38][4]
#define MW_FLOATS (MW_O_PART + MB_J * 4)

NBSS_HD int mb_runs(int T) { return (T + MB_CKPT - 1) / MB_CKPT; }
static int mb_grid(int64_t BF) { return (int)(BF < MB_GRID_CAP ? BF : MB_GRID_CAP); }
NBSS_HD size_t mb_ckpt_bytes(int64_t BF, int T) { return ws_align((size_t)BF * mb_runs(T) * MB_STATE * sizeof(float)); }
// NBSS_OK, or why the shape is refused
static int mb_check(int dtype, int64_t BF, int T) {
    if (BF < 1 || T < 1 || T > NBSS_T_MAX) return NBSS_EINVAL;
    if ((dtype != NBSS_F32 && dtype != NBSS_BF16) || BF * T > (1L << 28)) return NBSS_EUNSUPPORTED;
    return NBSS_OK;
}

struct MbArgs {
    const void* xz;
    const float *cw, *cb, *wx, *wdt, *bdt, *alog, *dp;
    void* y;
    float* save;
    const void* dy;
    void* dxz;
    float* part;
    long BF;
    int T;
};

NBSS_DEV void mb_chan(MbChan& c, const MbArgs& a, int e) { mb_chan(c, a.cw, a.cb, a.wdt, a.bdt, a.alog, a.dp, e); }

template <class T>
__global__ __launch_bounds__(MB_THREADS) void mb_fwd_kernel(MbArgs a) {
    NBSS_LDS(smem);
    float* L = reinterpret_cast<float*>(smem);
    float *WX = L + MF_O_WX, *XC = L + MF_O_XC, *DBC = L + MF_O_DBC;
    const int e = threadIdx.x, Tn = a.T, nck = (Tn + MB_CKPT - 1) / MB_CKPT;
    for (int i = e; i < MB_J * MB_E; i += MB_THREADS) WX[(i / MB_E) * MB_LW + i % MB_E] = a.wx[i];
    MbChan c;
    mb_chan(c, a, e);
    float* dbcs = a.save ? a.save + mb_ckpt_bytes(a.BF, Tn) / sizeof(float) : nullptr;
    for (long n = blockIdx.x; n < a.BF; n += gridDim.x) {
        const T* xz = (const T*)a.xz + (size_t)n * Tn * (2 * MB_E);
        T* y = (T*)a.y + (size_t)n * Tn * MB_E;
        float h[MB_N], xm1 = 0.f, xm2 = 0.f, xm3 = 0.f;
#pragma unroll
        for (int k = 0; k < MB_N; ++k) h[k] = 0.f;
        for (int ck = 0; ck < nck; ++ck) {
            const int t0 = ck * MB_CKPT, m = Tn - t0 < MB_CKPT ? Tn - t0 : MB_CKPT;
            __syncthreads();  // the x_proj matrix is in LDS; the previous run's readers are done
            if (a.save) {
                float* sv = a.save + ((size_t)n * nck + ck) * MB_STATE;
#pragma unroll
                for (int k = 0; k < MB_N; ++k) sv[k * MB_E + e] = h[k];
            }
            for (int i = 0; i < m; ++i) {
                const float xr = load1(xz + (size_t)(t0 + i) * (2 * MB_E) + e);
                XC[i * MB_E + e] = mb_conv(c, xm3, xm2, xm1, xr);
                xm3 = xm2;
                xm2 = xm1;
                xm1 = xr;
            }
            __syncthreads();
            for (int o = e; o < m * MB_J; o += MB_THREADS) {
                const int i = o / MB_J, j = o % MB_J;
                const float *w = WX + j * MB_LW, *x = XC + i * MB_E;
                float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
                for (int q = 0; q < MB_E; q += 4) {
                    s0 += w[q] * x[q];
                    s1 += w[q + 1] * x[q + 1];
                    s2 += w[q + 2] * x[q + 2];
                    s3 += w[q + 3] * x[q + 3];
                }
                const float s = (s0 + s1) + (s2 + s3);
                DBC[i * MB_JL + j] = s;
                if (dbcs) dbcs[((size_t)n * Tn + t0 + i) * MB_J + j] = s;
            }
            __syncthreads();
            for (int i = 0; i < m; ++i) {
                const float ys = mb_scan_frame(c, h, DBC + i * MB_JL, XC[i * MB_E + e]);
                const float z = load1(xz + (size_t)(t0 + i) * (2 * MB_E) + MB_E + e);
                store1(y + (size_t)(t0 + i) * MB_E + e, ys * silu_f(z));
            }
        }
    }
}

template <class T>
__global__ __launch_bounds__(MB_THREADS) void mb_bwd_kernel(MbArgs a) {
    NBSS_LDS(smem);
    float* L = reinterpret_cast<float*>(smem);
    float *HS = L + MW_O_HS, *XR = L + MW_O_XR, *XPRE = L + MW_O_XPRE, *XC = L + MW_O_XC, *DT = L + MW_O_DT, *DBC = L + MW_O_DBC, *DDBC = L + MW_O_DDBC,
          *REDC = L + MW_O_REDC, *REDR = L + MW_O_REDR, *PART = L + MW_O_PART;
    const int e = threadIdx.x, Tn = a.T, nck = (Tn + MB_CKPT - 1) / MB_CKPT;
    MbChan c;
    mb_chan(c, a, e);
    float wxc[MB_J];  // the channel's column of the x_proj matrix
#pragma unroll
    for (int j = 0; j < MB_J; ++j) wxc[j] = a.wx[j * MB_E + e];
    // the channel's parameter-gradient sums over every frame of every sequence of this workgroup
    float gcw[MB_K], gcb = 0.f, gwx[MB_J], gwdt[MB_R], gbdt = 0.f, gA[MB_N], gD = 0.f;
#pragma unroll
    for (int k = 0; k < MB_K; ++k) gcw[k] = 0.f;
#pragma unroll
    for (int j = 0; j < MB_J; ++j) gwx[j] = 0.f;
#pragma unroll
    for (int r = 0; r < MB_R; ++r) gwdt[r] = 0.f;
#pragma unroll
    for (int k = 0; k < MB_N; ++k) gA[k] = 0.f;
    const float* dbcs = a.save + mb_ckpt_bytes(a.BF, Tn) / sizeof(float);
    for (long n = blockIdx.x; n < a.BF; n += gridDim.x) {
        const T* xz = (const T*)a.xz + (size_t)n * Tn * (2 * MB_E);
        const T* dy = (const T*)a.dy + (size_t)n * Tn * MB_E;
        T* dxz = (T*)a.dxz + (size_t)n * Tn * (2 * MB_E);
        float dh[MB_N], dp1 = 0.f, dp2 = 0.f, dp3 = 0.f;  // dh: exp(dt A) dh of the frame behind; dp: d xpre of the three frames behind
#pragma unroll
        for (int k = 0; k < MB_N; ++k) dh[k] = 0.f;
        for (int ck = nck - 1; ck >= 0; --ck) {
            const int t0 = ck * MB_CKPT, m = Tn - t0 < MB_CKPT ? Tn - t0 : MB_CKPT;
            // ---- the run's inputs: xr (the channel's own column) and the saved x_proj rows -----------------------------------------------------------
            for (int i = 0; i < m + 3; ++i) {
                const int t = t0 - 3 + i;
                XR[i * MB_E + e] = t >= 0 ? load1(xz + (size_t)t * (2 * MB_E) + e) : 0.f;
            }
            for (int o = e; o < m * MB_J; o += MB_THREADS) DBC[(o / MB_J) * MB_JL + o % MB_J] = dbcs[((size_t)n * Tn + t0) * MB_J + o];
            __syncthreads();
            // ---- the forward again: xpre, xc, dt and the state before each frame ---------------------------------------------------------------------
            {
                float h[MB_N];
                const float* sv = a.save + ((size_t)n * nck + ck) * MB_STATE;
#pragma unroll
                for (int k = 0; k < MB_N; ++k) h[k] = sv[k * MB_E + e];
                for (int i = 0; i < m; ++i) {
                    const float* row = DBC + i * MB_JL;
                    const float xpre = c.cb + c.cw[0] * XR[i * MB_E + e] + c.cw[1] * XR[(i + 1) * MB_E + e] + c.cw[2] * XR[(i + 2) * MB_E + e] +
                                       c.cw[3] * XR[(i + 3) * MB_E + e];
                    const float xc = silu_f(xpre);
                    float pre;
                    const float dt = mb_dt(c, row, pre), dtx = dt * xc;
                    XPRE[i * MB_E + e] = xpre;
                    XC[i * MB_E + e] = xc;
#pragma unroll
                    for (int k = 0; k < MB_N; ++k) {
                        HS[(i * MB_N + k) * MB_E + e] = h[k];
                        h[k] = expf(dt * c.A[k]) * h[k] + dtx * row[MB_R + k];
                    }
                }
            }
            // ---- the reverse recurrence ----------------------------------------------------------------------------------------------------------------
            for (int i = m - 1; i >= 0; --i) {
                const float* row = DBC + i * MB_JL;
                const float xc = XC[i * MB_E + e];
                float pre;
                const float dt = mb_dt(c, row, pre), dtx = dt * xc;
                const float z = load1(xz + (size_t)(t0 + i) * (2 * MB_E) + MB_E + e), g = load1(dy + (size_t)(t0 + i) * MB_E + e);
                const float dys = g * silu_f(z);
                float ys = c.dp * xc, dxc = dys * c.dp, ddt = 0.f;
                gD += dys * xc;
#pragma unroll
                for (int k = 0; k < MB_N; ++k) {
                    float* hs = HS + (i * MB_N + k) * MB_E + e;
                    const float hp = *hs, dA = expf(dt * c.A[k]), Bk = row[MB_R + k], Ck = row[MB_R + MB_N + k];
                    const float hk = dA * hp + dtx * Bk, dhk = dh[k] + Ck * dys, t1 = dhk * hp * dA;
                    ys += Ck * hk;
                    REDC[k * MB_E + e] = dys * hk;
                    *hs = dhk * dtx;
                    ddt += t1 * c.A[k] + dhk * Bk * xc;
                    gA[k] += t1 * dt;
                    dxc += dhk * dt * Bk;
                    dh[k] = dhk * dA;
                }
                store1(dxz + (size_t)(t0 + i) * (2 * MB_E) + MB_E + e, g * ys * dsilu_f(z));
                const float ddtp = ddt / (1.0f + expf(-pre));  // softplus'
                gbdt += ddtp;
#pragma unroll
                for (int r = 0; r < MB_R; ++r) {
                    gwdt[r] += ddtp * row[r];
                    REDR[r * MB_E + e] = ddtp * c.wdt[r];
                }
                DT[i * MB_E + e] = dxc;
                __syncthreads();
                if (e < 4 * MB_J) {  // the 38 sums over the channels: four partial sums of 48 each, in channel order
#pragma clang fp reassociate(off)
                    const int j = e >> 2, q = e & 3;
                    const float* src = (j < MB_R ? REDR + j * MB_E : j < MB_R + MB_N ? HS + (i * MB_N + j - MB_R) * MB_E : REDC + (j - MB_R - MB_N) * MB_E) + 48 * q;
                    float s = 0.f;
                    for (int x = 0; x < 48; ++x) s += src[x];
                    PART[e] = s;
                }
                __syncthreads();
                if (e < MB_J) DDBC[i * MB_JL + e] = (PART[4 * e] + PART[4 * e + 1]) + (PART[4 * e + 2] + PART[4 * e + 3]);
            }
            __syncthreads();  // the gradients of the run's x_proj rows are complete
            // ---- x_proj and the convolution backward -----------------------------------------------------------------------------------------------------
            for (int i = m - 1; i >= 0; --i) {
                const float* drow = DDBC + i * MB_JL;
                const float xc = XC[i * MB_E + e];
                float dxc = DT[i * MB_E + e];
#pragma unroll
                for (int j = 0; j < MB_J; ++j) {
                    dxc += wxc[j] * drow[j];
                    gwx[j] += drow[j] * xc;
                }
                const float dpre = dxc * dsilu_f(XPRE[i * MB_E + e]);
                gcb += dpre;
#pragma unroll
                for (int k = 0; k < MB_K; ++k) gcw[k] += dpre * XR[(i + k) * MB_E + e];
                store1(dxz + (size_t)(t0 + i) * (2 * MB_E) + e, c.cw[3] * dpre + c.cw[2] * dp1 + c.cw[1] * dp2 + c.cw[0] * dp3);
                dp3 = dp2;
                dp2 = dp1;
                dp1 = dpre;
            }
            __syncthreads();  // the run's rows are consumed: the next run loads its own
        }
    }
    float* pr = a.part + (size_t)blockIdx.x * MB_SLOTS * MB_E + e;
#pragma unroll
    for (int k = 0; k < MB_K; ++k) pr[k * MB_E] = gcw[k];
    pr[4 * MB_E] = gcb;
#pragma unroll
    for (int j = 0; j < MB_J; ++j) pr[(5 + j) * MB_E] = gwx[j];
#pragma unroll
    for (int r = 0; r < MB_R; ++r) pr[(43 + r) * MB_E] = gwdt[r];
    pr[49 * MB_E] = gbdt;
#pragma unroll
    for (int k = 0; k < MB_N; ++k) pr[(50 + k) * MB_E] = gA[k] * c.A[k];  // d A_log = A dA
    pr[66 * MB_E] = gD;
}

struct MbGrads {
    float *cw, *cb, *wx, *wdt, *bdt, *alog, *dp;
};
// the partial rows of `rows` workgroups summed in workgroup order; block = slot, thread = channel
__global__ __launch_bounds__(MB_THREADS) void mb_fold_kernel(const float* part, int rows, MbGrads g) {
    const int s = blockIdx.x, e = threadIdx.x;
    const float v = fold_strided<16>(part + s * MB_E + e, (size_t)MB_SLOTS * MB_E, 0, rows);
    if (s < 4) g.cw[e * MB_K + s] = v;
    else if (s == 4) g.cb[e] = v;
    else if (s < 43) g.wx[(s - 5) * MB_E + e] = v;
    else if (s < 49) g.wdt[e * MB_R + s - 43] = v;
    else if (s == 49) g.bdt[e] = v;
    else if (s < 66) g.alog[e * MB_N + s - 50] = v;
    else g.dp[e] = v;
}

template <class T>
static int mb_fwd(const MbArgs& a, hipStream_t st) {
    const size_t lds = MF_FLOATS * sizeof(float);
    NBSS_LAUNCH((mb_fwd_kernel<T>), dim3(mb_grid(a.BF)), dim3(MB_THREADS), lds, st, a);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
static int mb_bwd(const MbArgs& a, const MbGrads& g, hipStream_t st) {
    const size_t lds = MW_FLOATS * sizeof(float);
    static_assert(MW_FLOATS * sizeof(float) <= 160 * 1024, "the backward's LDS image must fit a CU");
    int e = NBSS_SET_MAX_LDS((mb_bwd_kernel<T>), lds);
    if (e) return e;
    const int grid = mb_grid(a.BF);
    NBSS_LAUNCH((mb_bwd_kernel<T>), dim3(grid), dim3(MB_THREADS), lds, st, a);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_FOLD_LAUNCH(mb_fold_kernel, dim3(MB_SLOTS), dim3(MB_THREADS), 0, st, (const float*)a.part, grid, g);
    return NBSS_CHECK_LAUNCH();
}

extern "C" {

int64_t nbss_online_mamba_train_save_bytes(int dtype, int64_t BF, int T) {
    const int e = mb_check(dtype, BF, T);
    return e ? e : (int64_t)(mb_ckpt_bytes(BF, T) + ws_align((size_t)BF * T * MB_J * sizeof(float)));
}
int64_t nbss_online_mamba_train_ws_bytes(int dtype, int64_t BF, int T) {
    const int e = mb_check(dtype, BF, T);
    return e ? e : (int64_t)ws_align((size_t)mb_grid(BF) * MB_SLOTS * MB_E * sizeof(float));
}

int nbss_online_mamba_train_fwd(int dtype, int64_t BF, int T, const void* xz, const float* conv_w, const float* conv_b, const float* xproj_w,
                                const float* dt_w, const float* dt_b, const float* A_log, const float* D, void* y, void* save, void* ws, void* stream) {
    const int e = mb_check(dtype, BF, T);
    if (e) return e;
    if (!xz || !conv_w || !conv_b || !xproj_w || !dt_w || !dt_b || !A_log || !D || !y || !ws || y == xz) return NBSS_EINVAL;
    MbArgs a = {xz, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, y, (float*)save, nullptr, nullptr, nullptr, (long)BF, T};
    return dtype == NBSS_BF16 ? mb_fwd<bf16_t>(a, (hipStream_t)stream) : mb_fwd<float>(a, (hipStream_t)stream);
}

int nbss_online_mamba_train_bwd(int dtype, int64_t BF, int T, const void* xz, const float* conv_w, const float* conv_b, const float* xproj_w,
                                const float* dt_w, const float* dt_b, const float* A_log, const float* D, const void* save, const void* dy, void* dxz,
                                float* d_conv_w, float* d_conv_b, float* d_xproj_w, float* d_dt_w, float* d_dt_b, float* d_A_log, float* d_D, void* ws,
                                void* stream) {
    const int e = mb_check(dtype, BF, T);
    if (e) return e;
    if (!xz || !conv_w || !conv_b || !xproj_w || !dt_w || !dt_b || !A_log || !D || !save || !dy || !dxz || !d_conv_w || !d_conv_b || !d_xproj_w ||
        !d_dt_w || !d_dt_b || !d_A_log || !d_D || !ws || dxz == xz || dxz == dy)
        return NBSS_EINVAL;
    MbArgs a = {xz, conv_w, conv_b, xproj_w, dt_w, dt_b, A_log, D, nullptr, (float*)save, dy, dxz, (float*)ws, (long)BF, T};
    MbGrads g = {d_conv_w, d_conv_b, d_xproj_w, d_dt_w, d_dt_b, d_A_log, d_D};
    return dtype == NBSS_BF16 ? mb_bwd<bf16_t>(a, g, (hipStream_t)stream) : mb_bwd<float>(a, g, (hipStream_t)stream);
}

}  // extern "C"
