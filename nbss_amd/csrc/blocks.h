// Register-level building blocks shared by the narrow-band / cross-band kernels.
//
// The LayerNorm of a row over H = 32 KS = 16 MT channels (base/norm.py:11-27, eps 1e-5, fp32 statistics) lives here, once per register layout:
//   forward, B fragments (lane = row l&15, channels 32ks + 8(l>>4) + j):  ln_stats (statistics only) | ln_strip (two affine forms)
//   backward, C tiles    (lane = row,      channels 16mt + 4(l>>4) + r):  ln_bwd_row (from memory, with dgamma / dbeta) | ln_bwd_row_raw (from RawC4 registers, without)
// Each of the five is ONE flat body on purpose: the library is built with -ffast-math, and a first version that nested them (strip over statistics,
// both backward forms over one core) was the same arithmetic on the emulator but came out 1 - 3 ulp away from the copies it replaced in the fp32
// instances on the device (profiles/README.md, "LayerNorm row helpers").  tconvffn.hip and tconvffn_g.hip keep their own copies for the same reason.
// KS / MT are deduced from the arrays: 3 / 6 (BK_KS / BK_MT, H = 96) and 6 / 12 (the geometry-generic instances at H = 192).
// Other LayerNorms of the library are different algorithms or layouts and are NOT built on these: ln_halfrow_inplace (fconv.hip: two lanes per row,
// DPP exchange), the T-ConvFFN step kernel (tconvffn_s.hip), gb_rows.hip, tchain.hip, on_layernorm (online.hip) and online_train.hip.
#pragma once
#include "common.h"

#define BK_H 96
#define BK_KS 3   // H / 32
#define BK_MT 6   // H / 16

template <int KS>
NBSS_DEV void load_ln_affine(const float* __restrict__ lnw, const float* __restrict__ lnb, float (&gam)[KS][8], float (&bet)[KS][8]) {
    const int g4 = lane_id() >> 4;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            gam[ks][j] = lnw[ks * 32 + 8 * g4 + j];
            bet[ks][j] = lnb[ks * 32 + 8 * g4 + j];
        }
}

// (mean, rstd) of a row held as v[ks][j] = channel 32ks + 8(l>>4) + j by the four lanes l, l^16, l^32, l^48.  The variance is the mean of the
// squared DEVIATIONS (two reductions): a common offset far above the row's spread costs nothing.  Lanes without a row pass zeros or a clamped row.
// For the kernels that keep only the statistics or use them their own way; the strip and row helpers below carry the same lines themselves.
template <int KS>
NBSS_DEV void ln_stats(const float (&v)[KS][8], float& mean, float& rstd) {
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[ks][j];
    mean = wave_sum16(sum) * (1.0f / (32 * KS));
    float q = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[ks][j] - mean;
            q += d * d;
        }
    rstd = rsqrtf(wave_sum16(q) * (1.0f / (32 * KS)) + 1e-5f);
}

// LayerNorm of a 16-row strip into natural-order B fragments, the affine preloaded (load_ln_affine); stat: the training-mode forward's save
// buffer for the row statistics (layout.h: mhsa_stat_offset), or null
template <class T, int KS>
NBSS_DEV void ln_strip(const T* __restrict__ xr, bool valid, const float (&gam)[KS][8], const float (&bet)[KS][8], Frag<T> (&u)[KS], float* __restrict__ stat = nullptr) {
    const int g4 = lane_id() >> 4;
    float v[KS][8];
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (valid) load8(xr + ks * 32 + 8 * g4, v[ks]);
        else
#pragma unroll
            for (int j = 0; j < 8; ++j) v[ks][j] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[ks][j];
    }
    const float mean = wave_sum16(sum) * (1.0f / (32 * KS));
    float q = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[ks][j] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(wave_sum16(q) * (1.0f / (32 * KS)) + 1e-5f);
    if (stat && valid && g4 == 0) {
        stat[0] = mean;
        stat[1] = rstd;
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) frag_set(u[ks], j, (v[ks][j] - mean) * rstd * gam[ks][j] + bet[ks][j]);
}

// the same with the affine read where it is used: kernels that normalise one strip per wave keep 16 KS registers free until then
template <class T, int KS>
NBSS_DEV void ln_strip(const T* __restrict__ xr, bool valid, const float* __restrict__ lnw, const float* __restrict__ lnb, Frag<T> (&u)[KS]) {
    const int g4 = lane_id() >> 4;
    float v[KS][8];
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        if (valid) load8(xr + ks * 32 + 8 * g4, v[ks]);
        else
#pragma unroll
            for (int j = 0; j < 8; ++j) v[ks][j] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += v[ks][j];
    }
    const float mean = wave_sum16(sum) * (1.0f / (32 * KS));
    float q = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = v[ks][j] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(wave_sum16(q) * (1.0f / (32 * KS)) + 1e-5f);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        float gam[8], bet[8];
        load8(lnw + ks * 32 + 8 * g4, gam);
        load8(lnb + ks * 32 + 8 * g4, bet);
#pragma unroll
        for (int j = 0; j < 8; ++j) frag_set(u[ks], j, (v[ks][j] - mean) * rstd * gam[j] + bet[j]);
    }
}

// LayerNorm backward + residual for one row per lane, entirely in registers, x and dy rows in memory.
//   du[mt][r] : gradient w.r.t. the LN output, C-tile layout (lane = row, channels 16mt + 4(l>>4) + r)
//   dx = dy + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = gamma * du
// Also emits (mean, rstd) of the row for the wgrad kernels (stat may be null) and accumulates dgamma / dbeta partials (ln_affine_flush).
// Lanes without a row read nothing and hold zeros; dyr / dxr / stat are touched by valid lanes only.
template <class T, int MT>
NBSS_DEV void ln_bwd_row(f32x4 (&du)[MT], const T* __restrict__ xr, const T* __restrict__ dyr, T* __restrict__ dxr, float* __restrict__ stat, bool valid,
                         const float* __restrict__ lnw, float (&dlw)[MT][4], float (&dlb)[MT][4]) {
    const int g4 = lane_id() >> 4;
    float xv[MT][4];
    float sum = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (valid) load4(xr + 16 * mt + 4 * g4, xv[mt]);
        else xv[mt][0] = xv[mt][1] = xv[mt][2] = xv[mt][3] = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) sum += xv[mt][r];
    }
    const float mean = wave_sum16(sum) * (1.0f / (16 * MT));
    float q = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xv[mt][r] -= mean;
            q += xv[mt][r] * xv[mt][r];
        }
    const float rstd = rsqrtf(wave_sum16(q) * (1.0f / (16 * MT)) + 1e-5f);
    if (valid && g4 == 0 && stat) {
        stat[0] = mean;
        stat[1] = rstd;
    }
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ch = 16 * mt + 4 * g4 + r;
            xv[mt][r] *= rstd;  // xhat
            const float dv = valid ? du[mt][r] : 0.f;
            dlw[mt][r] += dv * xv[mt][r];
            dlb[mt][r] += dv;
            du[mt][r] = dv * lnw[ch];
            m1 += du[mt][r];
            m2 += du[mt][r] * xv[mt][r];
        }
    m1 = wave_sum16(m1) * (1.0f / (16 * MT));
    m2 = wave_sum16(m2) * (1.0f / (16 * MT));
    if (valid) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int ch = 16 * mt + 4 * g4;
            float dv[4], o[4];
            load4(dyr + ch, dv);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = dv[r] + rstd * (du[mt][r] - m1 - xv[mt][r] * m2);
            store4(dxr + ch, o[0], o[1], o[2], o[3]);
        }
    }
}

// ---- raw C-layout row pieces (lane = row, 4 channels per 16-channel tile) for software-pipelined row loops --------------------------
// The cross-band row loops (full.hip) are bound by exposed HBM latency at one workgroup per CU: the next iteration's x / dy pieces are
// requested before the current iteration's math.  Addresses are clamped by the caller (always readable), validity is applied on use.
template <class T> struct RawC4;
template <> struct RawC4<bf16_t> { u32x2 v; };
template <> struct RawC4<float> { f32x4 v; };
NBSS_DEV void rawc_load(RawC4<bf16_t>& r, const bf16_t* p) { r.v = *reinterpret_cast<const u32x2*>(p); }
NBSS_DEV void rawc_load(RawC4<float>& r, const float* p) { r.v = *reinterpret_cast<const f32x4*>(p); }
NBSS_DEV void rawc_get(const RawC4<bf16_t>& r, float (&o)[4]) {
    o[0] = bf2f((bf16_t)(r.v[0] & 0xFFFF)); o[1] = bf2f((bf16_t)(r.v[0] >> 16));
    o[2] = bf2f((bf16_t)(r.v[1] & 0xFFFF)); o[3] = bf2f((bf16_t)(r.v[1] >> 16));
}
NBSS_DEV void rawc_get(const RawC4<float>& r, float (&o)[4]) { o[0] = r.v[0]; o[1] = r.v[1]; o[2] = r.v[2]; o[3] = r.v[3]; }
template <class T>
NBSS_DEV void rawc_load_row(RawC4<T> (&r)[BK_MT], const T* __restrict__ row) {
    const int g4 = lane_id() >> 4;
#pragma unroll
    for (int mt = 0; mt < BK_MT; ++mt) rawc_load(r[mt], row + 16 * mt + 4 * g4);
}

// ln_bwd_row with the x and dy pieces of the row already in registers (rawc_load_row, requested one iteration ahead) and WITHOUT the affine-gradient
// sums: for kernels that get dgamma / dbeta from the weight gradient of the first linear map instead (tailw.hip, full.hip: dgamma[i] =
// sum_o W[o][i] D[o][i], dbeta[i] = sum_o W[o][i] db[o], D = da^T xhat).  STAT: write the row's (mean, rstd) for the weight-gradient kernel.
template <bool STAT, class T, int MT>
NBSS_DEV void ln_bwd_row_raw(f32x4 (&du)[MT], const RawC4<T> (&xr)[MT], const RawC4<T> (&dyr)[MT], T* __restrict__ dxr, float* __restrict__ stat, bool valid,
                             const float* __restrict__ lnw) {
    const int g4 = lane_id() >> 4;
    float xv[MT][4];
    float sum = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        rawc_get(xr[mt], xv[mt]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xv[mt][r] = keep_if(valid, xv[mt][r]);
            sum += xv[mt][r];
        }
    }
    const float mean = wave_sum16(sum) * (1.0f / (16 * MT));
    float q = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xv[mt][r] -= mean;
            q += xv[mt][r] * xv[mt][r];
        }
    const float rstd = rsqrtf(wave_sum16(q) * (1.0f / (16 * MT)) + 1e-5f);
    if (STAT && valid && g4 == 0) {
        stat[0] = mean;
        stat[1] = rstd;
    }
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        float gq[4];
        load4(lnw + 16 * mt + 4 * g4, gq);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xv[mt][r] *= rstd;  // xhat
            du[mt][r] = keep_if(valid, du[mt][r]) * gq[r];
            m1 += du[mt][r];
            m2 += du[mt][r] * xv[mt][r];
        }
    }
    m1 = wave_sum16(m1) * (1.0f / (16 * MT));
    m2 = wave_sum16(m2) * (1.0f / (16 * MT));
    if (valid) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int ch = 16 * mt + 4 * g4;
            float dv[4], o[4];
            rawc_get(dyr[mt], dv);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = dv[r] + rstd * (du[mt][r] - m1 - xv[mt][r] * m2);
            store4(dxr + ch, o[0], o[1], o[2], o[3]);
        }
    }
}

// Small per-channel parameter gradients (LN / GN affine, PReLU slope) are summed per workgroup in LDS
// (ds_add_f32) and written as ONE partial row per workgroup; util.hip's affine_reduce folds the rows
// into the gradient buffer.  (Same-address global atomics from every wave serialise in the memory
// system and stalled the barriers of the first version: 24.7 ms -> see profiles/.)
struct AffSegs {
    int n;
    long long off[8];  // destination offsets in the flat gradient buffer
    int cnt[8];        // consecutive elements per segment; the partial row is the concatenation
};
int affine_reduce_launch(const float* part, int nwg, const AffSegs& segs, float* G, hipStream_t st);

// reduce the per-lane dgamma/dbeta partials over the 16 rows of the lane group and add them to the
// workgroup's LDS accumulators (gw/gb may also be global: then these are plain atomicAdd's)
template <int MT>
NBSS_DEV void ln_affine_flush(float (&dlw)[MT][4], float (&dlb)[MT][4], float* __restrict__ gw, float* __restrict__ gb) {
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = row_sum16(dlw[mt][r]), b = row_sum16(dlb[mt][r]);
            if (l15 == 0) {
                atomicAdd(gw + 16 * mt + 4 * g4 + r, a);
                atomicAdd(gb + 16 * mt + 4 * g4 + r, b);
            }
        }
}
