// gb_attn.hip — whole-head attention of the geometry-generic path (gb.h), forward and backward.
// Attention backward for one (sequence, head), T <= 256, any head width DH % 8 == 0 (<= 64).  qkv [N][3H] (q | k | v, head h at columns h DH),
// scores = q k^T / sqrt(DH), softmax over the keys, O = P V.
//   kernel Q (queries are the MFMA N dimension; K, V of the head in LDS):  O, lse = log sum exp, D = rowsum(P dP), dQ
//   kernel K (keys are the N dimension; Q, dO of the head in LDS):         dK, dV
// The row-major [TP][DH] LDS images, their transposed reads (V^T, K^T, Q^T, dO^T: the token axis as K dimension), the softmax steps and the store of the
// output tiles are attn_tiles.h's, shared with the key-blocked and the relative-position kernels.
#include "gb.h"
#include "attn_tiles.h"

// BWD = false: the forward alone (O; dO / dqkv / lse / Dv are not touched) — the attention of the narrow-band building blocks (nbss_nb_attention_fwd)
template <class T, int DH, bool BWD>
__global__ __launch_bounds__(GB_THREADS) void gb_attn_q_kernel(const T* __restrict__ qkv, const T* __restrict__ dO, T* __restrict__ O, T* __restrict__ dqkv,
                                                               float* __restrict__ lse, float* __restrict__ Dv, int Tn, int H, int heads) {
    constexpr int KS = (DH + 31) / 32, MTD = (DH + 15) / 16, NTM = GA_TMAX / 16;
    NBSS_LDS(smem);
    const int NT = cdiv(Tn, 16), TP = 32 * cdiv(Tn, 32);
    T* Ks = reinterpret_cast<T*>(smem);  // [TP][DH]
    T* Vs = Ks + (size_t)TP * DH;        // [TP][DH]
    const int seq = blockIdx.x, head = blockIdx.y;
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id();
    const size_t n0 = (size_t)seq * Tn;
    const int ld = 3 * H;
    at_stage<T, DH, DH, GB_THREADS>(Ks, qkv + n0 * ld + H + head * DH, ld, 0, TP, Tn);
    at_stage<T, DH, DH, GB_THREADS>(Vs, qkv + n0 * ld + 2 * H + head * DH, ld, 0, TP, Tn);
    __syncthreads();
    const float scale = rsqrtf((float)DH);
    for (int qt = w; qt < NT; qt += GB_THREADS / 64) {
        const int q = qt * 16 + l15;
        const bool qv = q < Tn;
        const size_t nq = n0 + (qv ? q : 0);
        Frag<T> qf[KS], dof[KS];
        at_frag_rows<T, DH>(qf, qkv + nq * ld + head * DH, qv);
        at_frag_rows<T, DH>(dof, BWD ? dO + nq * H + head * DH : nullptr, BWD && qv);
        // S^T and dP^T tiles: rows = keys 16 jt + 4 g4 + r, column = the lane's query
        f32x4 st[NTM], dp[NTM];
        float mx = AT_NEG;
#pragma unroll
        for (int jt = 0; jt < NTM; ++jt) {
            st[jt] = F32X4_ZERO;
            dp[jt] = F32X4_ZERO;
            if (jt < NT) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    Frag<T> kf, vf;
                    at_frag_row<T, DH>(kf, Ks + (size_t)(16 * jt + l15) * DH, ks);
                    st[jt] = mma(kf, qf[ks], st[jt]);
                    if (BWD) {
                        at_frag_row<T, DH>(vf, Vs + (size_t)(16 * jt + l15) * DH, ks);
                        dp[jt] = mma(vf, dof[ks], dp[jt]);
                    }
                }
                mx = fmaxf(mx, at_mask_scale_max<1>(st + jt, 16 * jt, Tn, scale));
            }
        }
        mx = wave_max16(mx);
        const float sum = wave_sum16(at_exp_sum<NTM>(st, 0, Tn, mx));
        const float inv = 1.0f / sum;
        float dsum = 0.f;
#pragma unroll
        for (int jt = 0; jt < NTM; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                st[jt][r] *= inv;  // P^T
                dsum += st[jt][r] * dp[jt][r];
            }
        dsum = wave_sum16(dsum);  // D = rowsum(P dP) = rowsum(dO O)
        if (BWD && qv && g4 == 0) {
            lse[nq * heads + head] = mx + __logf(sum);
            Dv[nq * heads + head] = dsum;
        }
        // O^T = V^T P^T and dQ^T = K^T dS^T: K dimension = keys in pairs of tiles (permuted order of two stacked C tiles)
        f32x4 oacc[MTD], qacc[MTD];
#pragma unroll
        for (int mt = 0; mt < MTD; ++mt) oacc[mt] = qacc[mt] = F32X4_ZERO;
#pragma unroll
        for (int kk = 0; kk < NTM / 2; ++kk) {
            if (2 * kk < NT) {
                f32x4 ds0, ds1;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ds0[r] = st[2 * kk][r] * (dp[2 * kk][r] - dsum) * scale;
                    ds1[r] = st[2 * kk + 1][r] * (dp[2 * kk + 1][r] - dsum) * scale;
                }
                Frag<T> pf, dsf;
                frag_from_c2(pf, st[2 * kk], st[2 * kk + 1]);
                frag_from_c2(dsf, ds0, ds1);
                at_mma_t<T, DH, DH>(oacc, Vs, 32 * kk, pf);
                if (BWD) at_mma_t<T, DH, DH>(qacc, Ks, 32 * kk, dsf);
            }
        }
        if (qv) {
            at_store_row<T, DH>(O + nq * H + head * DH, oacc);
            if (BWD) at_store_row<T, DH>(dqkv + nq * ld + head * DH, qacc);
        }
    }
}

template <class T, int DH>
__global__ __launch_bounds__(GB_THREADS) void gb_attn_k_kernel(const T* __restrict__ qkv, const T* __restrict__ dO, T* __restrict__ dqkv,
                                                               const float* __restrict__ lse, const float* __restrict__ Dv, int Tn, int H, int heads) {
    constexpr int KS = (DH + 31) / 32, MTD = (DH + 15) / 16;
    NBSS_LDS(smem);
    const int NT = cdiv(Tn, 16), TP = 32 * cdiv(Tn, 32);
    T* Qs = reinterpret_cast<T*>(smem);   // [TP][DH]
    T* dOs = Qs + (size_t)TP * DH;        // [TP][DH]
    float* ls = reinterpret_cast<float*>(dOs + (size_t)TP * DH);  // [TP] lse | [TP] D
    float* Ds = ls + TP;
    const int seq = blockIdx.x, head = blockIdx.y;
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id();
    const size_t n0 = (size_t)seq * Tn;
    const int ld = 3 * H;
    at_stage<T, DH, DH, GB_THREADS>(Qs, qkv + n0 * ld + head * DH, ld, 0, TP, Tn);
    at_stage<T, DH, DH, GB_THREADS>(dOs, dO + n0 * H + head * DH, H, 0, TP, Tn);
    for (int t = threadIdx.x; t < TP; t += GB_THREADS) {
        ls[t] = t < Tn ? lse[(n0 + t) * heads + head] : 0.f;
        Ds[t] = t < Tn ? Dv[(n0 + t) * heads + head] : 0.f;
    }
    __syncthreads();
    const float scale = rsqrtf((float)DH);
    for (int kt = w; kt < NT; kt += GB_THREADS / 64) {
        const int key = kt * 16 + l15;
        const bool kv = key < Tn;
        const size_t nk = n0 + (kv ? key : 0);
        Frag<T> kf[KS], vf[KS];
        at_frag_rows<T, DH>(kf, qkv + nk * ld + H + head * DH, kv);
        at_frag_rows<T, DH>(vf, qkv + nk * ld + 2 * H + head * DH, kv);
        f32x4 kacc[MTD], vacc[MTD];
#pragma unroll
        for (int mt = 0; mt < MTD; ++mt) kacc[mt] = vacc[mt] = F32X4_ZERO;
        for (int kk = 0; 2 * kk < NT; ++kk) {
            // S and dP tiles of query tiles 2 kk, 2 kk + 1: rows = queries 16 it + 4 g4 + r, column = the lane's key
            f32x4 pt[2], dst[2];
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const int it = 2 * kk + h2;
                f32x4 s = F32X4_ZERO, dpv = F32X4_ZERO;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    Frag<T> qf, dof;
                    at_frag_row<T, DH>(qf, Qs + (size_t)(16 * it + l15) * DH, ks);
                    at_frag_row<T, DH>(dof, dOs + (size_t)(16 * it + l15) * DH, ks);
                    s = mma(qf, kf[ks], s);
                    dpv = mma(dof, vf[ks], dpv);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = 16 * it + 4 * g4 + r;
                    const bool ok = kv && q < Tn;
                    const float p = ok ? __expf(s[r] * scale - ls[q]) : 0.f;
                    pt[h2][r] = p;
                    dst[h2][r] = p * (dpv[r] - Ds[q]) * scale;
                }
            }
            Frag<T> pf, dsf;
            frag_from_c2(pf, pt[0], pt[1]);
            frag_from_c2(dsf, dst[0], dst[1]);
            at_mma_t<T, DH, DH>(vacc, dOs, 32 * kk, pf);
            at_mma_t<T, DH, DH>(kacc, Qs, 32 * kk, dsf);
        }
        if (kv) {
            at_store_row<T, DH>(dqkv + nk * ld + H + head * DH, kacc);
            at_store_row<T, DH>(dqkv + nk * ld + 2 * H + head * DH, vacc);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// launchers
template <class T, int DH>
int gb_attn_launch(const nbss_cfg& c, const void* qkv, const void* dO, void* O, void* dqkv, float* lse, float* Dv, hipStream_t st) {
    const int TP = 32 * cdiv(c.T, 32);
    const size_t ldsq = (size_t)2 * TP * DH * sizeof(T) + 64, ldsk = ldsq + (size_t)2 * TP * sizeof(float);  // (+64: the transposing reads of a 24-wide head's second channel tile run 16 bytes past the last row)
    if (c.T > GA_TMAX || ldsk > 160 * 1024) return NBSS_EUNSUPPORTED;
    int e;
    if ((e = NBSS_SET_MAX_LDS((gb_attn_q_kernel<T, DH, true>), ldsq))) return e;
    if ((e = NBSS_SET_MAX_LDS((gb_attn_k_kernel<T, DH>), ldsk))) return e;
    dim3 grid(c.B * c.F, c.heads);
    NBSS_LAUNCH((gb_attn_q_kernel<T, DH, true>), grid, dim3(GB_THREADS), ldsq, st, (const T*)qkv, (const T*)dO, (T*)O, (T*)dqkv, lse, Dv, c.T, c.H, c.heads);
    if ((e = NBSS_CHECK_LAUNCH())) return e;
    NBSS_LAUNCH((gb_attn_k_kernel<T, DH>), grid, dim3(GB_THREADS), ldsk, st, (const T*)qkv, (const T*)dO, (T*)dqkv, (const float*)lse, (const float*)Dv, c.T, c.H, c.heads);
    return NBSS_CHECK_LAUNCH();
}
// the forward alone: the attention of the narrow-band building blocks (nbss_nb_attention_fwd)
template <class T, int DH>
int nb_attn_fwd(long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st) {
    const int TP = 32 * cdiv(Tn, 32);
    const size_t lds = (size_t)2 * TP * DH * sizeof(T) + 64;
    if (Tn > GA_TMAX || lds > 160 * 1024) return NBSS_EUNSUPPORTED;
    int e = NBSS_SET_MAX_LDS((gb_attn_q_kernel<T, DH, false>), lds);
    if (e) return e;
    NBSS_LAUNCH((gb_attn_q_kernel<T, DH, false>), dim3((unsigned)nseq, heads), dim3(GB_THREADS), lds, st, (const T*)qkv, (const T*)nullptr, (T*)o, (T*)nullptr, (float*)nullptr,
                (float*)nullptr, Tn, H, heads);
    return NBSS_CHECK_LAUNCH();
}

#define GB_INSTANTIATE(fn, ...)             \
    template int fn<bf16_t, 48>(__VA_ARGS__); \
    template int fn<float, 48>(__VA_ARGS__);  \
    template int fn<bf16_t, 24>(__VA_ARGS__); \
    template int fn<float, 24>(__VA_ARGS__);
GB_INSTANTIATE(nb_attn_fwd, long, int, int, int, const void*, void*, hipStream_t)
GB_INSTANTIATE(gb_attn_launch, const nbss_cfg&, const void*, const void*, void*, void*, float*, float*, hipStream_t)
