// Key-blocked scaled-dot-product attention for wide heads (head width 96: NBC2-large, dim_hidden 192 / 2 heads), forward and backward.
//
// gb_attn.hip's gb_attn_q_kernel / gb_attn_k_kernel keep a whole head's K and V (or Q and dO) in LDS and a whole score row in registers: at head width
// 96 and T = 251 that is 2 x 256 x 96 x 4 B = 196 KB in fp32, more than a CU has.  Here the OTHER axis is walked in blocks of KB_BLK = 64 rows:
//
//   kb_attn_q_kernel   one workgroup per (sequence, head, 64 queries); each of the 4 waves owns one 16-query tile (queries = the MFMA N dimension) and
//                      keeps its q (and dO) fragments in registers.  K / V come through LDS 64 keys at a time; running max / running sum per query
//                      (online softmax), O rescaled per block.  BWD: also lse = max + log(sum) and D = rowsum(P dP) to the workspace, then a SECOND
//                      sweep over the key blocks (last block first: it is still staged) for dQ = sum_blocks K^T dS, dS = P (dP - D) scale.
//   kb_attn_k_kernel   one workgroup per (sequence, head, 64 keys); each wave owns one 16-key tile (keys = the N dimension) with k / v fragments in
//                      registers.  Q / dO / lse / D come through LDS 64 queries at a time; dK = sum dS^T Q, dV = sum P^T dO.
//
// The two-kernel split of the siblings is kept (rather than one sweep that produces dQ, dK and dV together): a one-sweep backward has to add the dQ
// (or dK / dV) contributions of different workgroups — atomics, i.e. gradients that differ from run to run — or hold all of a head's dQ in LDS
// (256 x 96 x 4 B = 96 KB on top of the operand blocks).  With the split every output element is written by exactly one wave in a fixed order.
//
// LDS: two images of 64 rows x (DH + 16 bytes of padding): 2 x 64 x 100 x 4 B = 50 KB in fp32, 26 KB in bf16 (+ 512 B of lse / D in the K kernel),
// single-buffered: three fp32 workgroups fit in a CU's 160 KB, so one workgroup's staging overlaps the others' MFMAs without a second buffer (and a
// (sequence, head) is 4 workgroups at T = 251 instead of 1: 1 032 workgroups for one 129-frequency utterance on 256 CUs).  The 16-byte row padding moves
// consecutive rows 100 (fp32) / 52 (bf16) banks apart instead of 96 / 48: the 16 rows a ds_read_b128 group touches land on distinct banks but for one pair.
// Transposed operands (token axis as the K dimension) are read as in the siblings: ds_read_b64_tr_b16 for bf16, element gathers for fp32 (conflict-free:
// 16 consecutive words x 4 rows that are 400 words apart).  Staging, fragments, softmax steps and stores are attn_tiles.h's, with LD = DH + 16 bytes.
// Tail rows of a block (>= T) are staged as zeros and their scores masked, so any T >= 1 works; the training launchers keep the narrow-band cap of 256 frames.
//
// Long sequences (nbss_nb_attention_long_fwd: inference on whole utterances, T <= 4096): the same forward kernel, also instantiated for the narrow heads
// (DH = 24, 48) the whole-head kernels of gb_attn.hip serve up to 256 frames.  K steps (DH + 31) / 32 with zero fragment lanes from DH on, (DH + 15) / 16
// output tiles whose rows >= DH are never stored; the backward kernels stay at whole 32-wide K steps (DH = 96).
#include "kb.h"
#include "attn_tiles.h"
#include "layout.h"
#include "blocks.h"
#include "nb.h"

// BWD = false: the forward alone (O; dO / dqkv / lse / Dv are not touched)
template <class T, int DH, bool BWD>
__global__ __launch_bounds__(KB_THREADS) void kb_attn_q_kernel(const T* __restrict__ qkv, const T* __restrict__ dO, T* __restrict__ O, T* __restrict__ dqkv,
                                                               float* __restrict__ lse, float* __restrict__ Dv, int Tn, int H, int heads) {
    static_assert(DH % 8 == 0 && (DH % 32 == 0 || !BWD), "the backward takes whole 32-wide K steps");
    constexpr int KS = (DH + 31) / 32, MTD = (DH + 15) / 16, LD = DH + 16 / sizeof(T), JT = KB_BLK / 16;
    NBSS_LDS(smem);
    T* Ks = reinterpret_cast<T*>(smem);  // [KB_BLK][LD]
    T* Vs = Ks + (size_t)KB_BLK * LD;    // [KB_BLK][LD]
    const int seq = blockIdx.x, head = blockIdx.y, q0 = (int)blockIdx.z * KB_BLK;
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id_u();
    const size_t n0 = (size_t)seq * Tn;
    const int ld = 3 * H, NB = cdiv(Tn, KB_BLK);
    const T* kbase = qkv + n0 * ld + H + head * DH;
    const T* vbase = qkv + n0 * ld + 2 * H + head * DH;
    const bool wave_on = q0 + 16 * w < Tn;  // (wave-uniform) a tile past the end only helps staging
    const int q = q0 + 16 * w + l15;
    const bool qv = q < Tn;
    const size_t nq = n0 + (qv ? q : 0);
    const float scale = rsqrtf((float)DH);
    Frag<T> qf[KS], dof[KS];  // (DH % 32 != 0: fragment lanes from DH on are zeros)
    at_frag_rows<T, DH>(qf, qkv + nq * ld + head * DH, qv);
    at_frag_rows<T, DH>(dof, BWD ? dO + nq * H + head * DH : nullptr, BWD && qv);
    // ---- sweep 1: O^T = V^T P^T with the running max m and running sum l of the lane's query (the same in its 4 lane groups) ----
    // BWD: D = rowsum(P dP) runs along like l (the same rescale), from the dP tiles of the block — not rowsum(dO o O) afterwards: the same sums as the siblings,
    // and exact where the softmax is (one key: D == dP bit for bit, so dS == 0)
    float m = AT_NEG, l = 0.f, dsum = 0.f;
    f32x4 oacc[MTD];
#pragma unroll
    for (int mt = 0; mt < MTD; ++mt) oacc[mt] = F32X4_ZERO;
    for (int b = 0; b < NB; ++b) {
        if (b) lds_barrier();
        at_stage<T, DH, LD, KB_THREADS>(Ks, kbase, ld, b * KB_BLK, KB_BLK, Tn);
        at_stage<T, DH, LD, KB_THREADS>(Vs, vbase, ld, b * KB_BLK, KB_BLK, Tn);
        __syncthreads();
        if (!wave_on) continue;
        // S^T tiles: rows = keys 64 b + 16 jt + 4 g4 + r, column = the lane's query
        f32x4 st[JT], dp[JT];
        float bm = AT_NEG;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            st[jt] = dp[jt] = F32X4_ZERO;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                Frag<T> kf, vf;
                at_frag_row<T, DH>(kf, Ks + (size_t)(16 * jt + l15) * LD, ks);
                st[jt] = mma(kf, qf[ks], st[jt]);
                if (BWD) {
                    at_frag_row<T, DH>(vf, Vs + (size_t)(16 * jt + l15) * LD, ks);
                    dp[jt] = mma(vf, dof[ks], dp[jt]);
                }
            }
            bm = fmaxf(bm, at_mask_scale_max<1>(st + jt, b * KB_BLK + 16 * jt, Tn, scale));
        }
        const float mn = fmaxf(m, wave_max16(bm));  // (every block holds at least one valid key: finite from the first block on)
        float pd = 0.f;
        const float ps = at_exp_sum<JT, BWD>(st, b * KB_BLK, Tn, mn, dp, &pd);
        const float alpha = at_online_rescale<MTD>(m, l, oacc, mn, wave_sum16(ps));
        if (BWD) dsum = dsum * alpha + wave_sum16(pd);
#pragma unroll
        for (int kk = 0; kk < JT / 2; ++kk) {
            Frag<T> pf;
            frag_from_c2(pf, st[2 * kk], st[2 * kk + 1]);
            at_mma_t<T, DH, LD>(oacc, Vs, 32 * kk, pf);
        }
    }
    const float inv = 1.0f / l;
    if (wave_on) {
#pragma unroll
        for (int mt = 0; mt < MTD; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[mt][r] *= inv;
        if (qv) at_store_row<T, DH>(O + nq * H + head * DH, oacc);
    }
    if (!BWD) return;
    dsum *= inv;  // D = rowsum(P dP) = rowsum(dO o O)
    const float lq = m + __logf(l);
    if (wave_on && qv && g4 == 0) {
        lse[nq * heads + head] = lq;
        Dv[nq * heads + head] = dsum;
    }
    // ---- sweep 2: dQ^T = K^T dS^T, scores recomputed; block NB - 1 is still in LDS ----
    f32x4 qacc[MTD];
#pragma unroll
    for (int mt = 0; mt < MTD; ++mt) qacc[mt] = F32X4_ZERO;
    for (int b = NB - 1; b >= 0; --b) {
        if (b != NB - 1) {
            lds_barrier();
            at_stage<T, DH, LD, KB_THREADS>(Ks, kbase, ld, b * KB_BLK, KB_BLK, Tn);
            at_stage<T, DH, LD, KB_THREADS>(Vs, vbase, ld, b * KB_BLK, KB_BLK, Tn);
            __syncthreads();
        }
        if (!wave_on) continue;
        f32x4 ds[JT];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            f32x4 s = F32X4_ZERO, dp = F32X4_ZERO;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                Frag<T> kf, vf;
                at_frag_row<T, DH>(kf, Ks + (size_t)(16 * jt + l15) * LD, ks);
                at_frag_row<T, DH>(vf, Vs + (size_t)(16 * jt + l15) * LD, ks);
                s = mma(kf, qf[ks], s);
                dp = mma(vf, dof[ks], dp);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool kv = b * KB_BLK + 16 * jt + 4 * g4 + r < Tn;
                const float p = keep_if(kv, __expf(s[r] * scale - lq));
                ds[jt][r] = p * (dp[r] - dsum) * scale;
            }
        }
#pragma unroll
        for (int kk = 0; kk < JT / 2; ++kk) {
            Frag<T> dsf;
            frag_from_c2(dsf, ds[2 * kk], ds[2 * kk + 1]);
            at_mma_t<T, DH, LD>(qacc, Ks, 32 * kk, dsf);
        }
    }
    if (wave_on && qv) at_store_row<T, DH>(dqkv + nq * ld + head * DH, qacc);
}

template <class T, int DH>
__global__ __launch_bounds__(KB_THREADS) void kb_attn_k_kernel(const T* __restrict__ qkv, const T* __restrict__ dO, T* __restrict__ dqkv,
                                                               const float* __restrict__ lse, const float* __restrict__ Dv, int Tn, int H, int heads) {
    static_assert(DH % 32 == 0, "whole 32-wide K steps");
    constexpr int KS = DH / 32, MTD = DH / 16, LD = DH + 16 / sizeof(T);
    NBSS_LDS(smem);
    T* Qs = reinterpret_cast<T*>(smem);                                    // [KB_BLK][LD]
    T* dOs = Qs + (size_t)KB_BLK * LD;                                     // [KB_BLK][LD]
    float* ls = reinterpret_cast<float*>(dOs + (size_t)KB_BLK * LD);       // [KB_BLK] lse | [KB_BLK] D
    float* Ds = ls + KB_BLK;
    const int seq = blockIdx.x, head = blockIdx.y, k0 = (int)blockIdx.z * KB_BLK;
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id_u();
    const size_t n0 = (size_t)seq * Tn;
    const int ld = 3 * H, NB = cdiv(Tn, KB_BLK);
    const bool wave_on = k0 + 16 * w < Tn;
    const int key = k0 + 16 * w + l15;
    const bool kv = key < Tn;
    const size_t nk = n0 + (kv ? key : 0);
    const float scale = rsqrtf((float)DH);
    Frag<T> kf[KS], vf[KS];
    at_frag_rows<T, DH>(kf, qkv + nk * ld + H + head * DH, kv);
    at_frag_rows<T, DH>(vf, qkv + nk * ld + 2 * H + head * DH, kv);
    f32x4 kacc[MTD], vacc[MTD];
#pragma unroll
    for (int mt = 0; mt < MTD; ++mt) kacc[mt] = vacc[mt] = F32X4_ZERO;
    for (int b = 0; b < NB; ++b) {
        if (b) lds_barrier();
        at_stage<T, DH, LD, KB_THREADS>(Qs, qkv + n0 * ld + head * DH, ld, b * KB_BLK, KB_BLK, Tn);
        at_stage<T, DH, LD, KB_THREADS>(dOs, dO + n0 * H + head * DH, H, b * KB_BLK, KB_BLK, Tn);
        if (threadIdx.x < KB_BLK) {
            const int t = b * KB_BLK + (int)threadIdx.x;
            ls[threadIdx.x] = t < Tn ? lse[(n0 + t) * heads + head] : 0.f;
            Ds[threadIdx.x] = t < Tn ? Dv[(n0 + t) * heads + head] : 0.f;
        }
        __syncthreads();
        if (!wave_on) continue;
#pragma unroll
        for (int kk = 0; kk < KB_BLK / 32; ++kk) {
            // S and dP tiles of query tiles 2 kk, 2 kk + 1 of the block: rows = queries 16 it + 4 g4 + r, column = the lane's key
            f32x4 pt[2], dst[2];
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                const int it = 2 * kk + h2;
                f32x4 s = F32X4_ZERO, dpv = F32X4_ZERO;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    Frag<T> qf, dof;
                    at_frag_row<T, DH>(qf, Qs + (size_t)(16 * it + l15) * LD, ks);
                    at_frag_row<T, DH>(dof, dOs + (size_t)(16 * it + l15) * LD, ks);
                    s = mma(qf, kf[ks], s);
                    dpv = mma(dof, vf[ks], dpv);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ql = 16 * it + 4 * g4 + r;
                    const bool ok = kv && b * KB_BLK + ql < Tn;
                    const float p = keep_if(ok, __expf(s[r] * scale - ls[ql]));
                    pt[h2][r] = p;
                    dst[h2][r] = p * (dpv[r] - Ds[ql]) * scale;
                }
            }
            Frag<T> pf, dsf;
            frag_from_c2(pf, pt[0], pt[1]);
            frag_from_c2(dsf, dst[0], dst[1]);
            at_mma_t<T, DH, LD>(vacc, dOs, 32 * kk, pf);
            at_mma_t<T, DH, LD>(kacc, Qs, 32 * kk, dsf);
        }
    }
    if (wave_on && kv) {
        at_store_row<T, DH>(dqkv + nk * ld + H + head * DH, kacc);
        at_store_row<T, DH>(dqkv + nk * ld + 2 * H + head * DH, vacc);
    }
}

template <class T, int DH>
static int kb_attn_fwd(long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st) {
    const size_t lds = (size_t)2 * KB_BLK * (DH + 16 / sizeof(T)) * sizeof(T);
    NBSS_LAUNCH((kb_attn_q_kernel<T, DH, false>), dim3((unsigned)nseq, heads, cdiv(Tn, KB_BLK)), dim3(KB_THREADS), lds, st, (const T*)qkv, (const T*)nullptr, (T*)o,
                (T*)nullptr, (float*)nullptr, (float*)nullptr, Tn, H, heads);
    return NBSS_CHECK_LAUNCH();
}
template <class T, int DH>
static int kb_attn_bwd(long nseq, int Tn, int H, int heads, const void* qkv, const void* dO, void* O, void* dqkv, float* lse, float* Dv, hipStream_t st) {
    const size_t ldsq = (size_t)2 * KB_BLK * (DH + 16 / sizeof(T)) * sizeof(T), ldsk = ldsq + (size_t)2 * KB_BLK * sizeof(float);
    const dim3 grid((unsigned)nseq, heads, cdiv(Tn, KB_BLK));
    NBSS_LAUNCH((kb_attn_q_kernel<T, DH, true>), grid, dim3(KB_THREADS), ldsq, st, (const T*)qkv, (const T*)dO, (T*)O, (T*)dqkv, lse, Dv, Tn, H, heads);
    int e = NBSS_CHECK_LAUNCH();
    if (e) return e;
    NBSS_LAUNCH((kb_attn_k_kernel<T, DH>), grid, dim3(KB_THREADS), ldsk, st, (const T*)qkv, (const T*)dO, (T*)dqkv, (const float*)lse, (const float*)Dv, Tn, H, heads);
    return NBSS_CHECK_LAUNCH();
}

// head width 96 (nb_blocks.hip dispatches here: nb_attention_fwd_impl / nb_attention_bwd_impl); same tensors and workspace pieces as the narrow kernels
int nb_attention_kb_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st) {
    if (heads <= 0 || H != heads * 96 || Tn > KB_TMAX || heads > 65535) return NBSS_EUNSUPPORTED;
    return AT_DISPATCH(dtype, kb_attn_fwd, 96, nseq, Tn, H, heads, qkv, o, st);
}
int nb_attention_kb_bwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* dO, void* O, void* dqkv, float* lse, float* Dv, hipStream_t st) {
    if (heads <= 0 || H != heads * 96 || Tn > KB_TMAX || heads > 65535) return NBSS_EUNSUPPORTED;
    return AT_DISPATCH(dtype, kb_attn_bwd, 96, nseq, Tn, H, heads, qkv, dO, O, dqkv, lse, Dv, st);
}
// forward on long sequences (nbss_nb_attention_long_fwd): the key-blocked kernel at every head width the narrow-band networks use, T <= KB_TLONG
int nb_attention_long_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st) {
    if (heads <= 0 || H % heads) return NBSS_EINVAL;
    if (Tn > KB_TLONG || heads > 65535) return NBSS_EUNSUPPORTED;
    const int dh = H / heads;
    return dh == 96 ? AT_DISPATCH(dtype, kb_attn_fwd, 96, nseq, Tn, H, heads, qkv, o, st) : AT_DISPATCH_NARROW(dtype, dh, kb_attn_fwd, nseq, Tn, H, heads, qkv, o, st);
}
