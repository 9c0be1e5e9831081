// gbwd.hip — the backward pass for geometries the fused training kernels are not specialised for (SpatialNet-large: dim_hidden 192,
// dim_ffn 384, dim_squeeze 16, head width 48; configs/SpatialNet.yaml "for large" comments, models/arch/SpatialNet.py:154-171), and the
// T-ConvFFN forward on the same pieces.  This file holds the SEQUENCING only — which piece runs on which workspace tensor, in which order, on
// which stream — and no kernel.
//
// The fused backward kernels (fconv.hip, full.hip, mhsa_bwd.hip, tconvffn_s.hip) keep a whole slab / sequence of the small geometry in LDS;
// at twice the widths their images do not fit, so this path is built from geometry-generic pieces instead, one tensor
// pass each, every intermediate in the workspace (288 GB of HBM: a 4-utterance large step keeps ~40 [N][FFN] tensors per block alive
// for microseconds).  The pieces (interface: gb.h):
//   * tap_gemm      gb_gemm.hip: every per-token linear map, the grouped convolutions along F and along T, the LinearGroup and their data gradients
//   * row kernels   gb_rows.hip: LayerNorm forward / backward (+ affine gradients), SiLU / PReLU backward, GroupNorm statistics / apply / backward,
//                   the [N][SQ] <-> [B T][SQ][F] transposes of the full-band block
//   * attention     gb_attn.hip: two kernels per (sequence, head)
//   * one-kernel forms where the shape allows: fconv_g.hip, tchain.hip, gemm_g.hip (bf16)
//   * weight gradients: wgrad.hip's token-contraction kernels, which are generic in their dimensions already, and wgrad_g.hip
// Semantics and parity: the same oracle functions as the fused path (oracle/spatialnet_ref.py), tests/test_large.py.
#include "gb.h"
#include "prof.h"
#include "wgrad.h"
#include "side.h"
#include "tchain.h"
#include "blocks.h"

static void gb_wgrad_base(WgradArgs& a, const nbss_cfg& c, void* ws, long Ntok) {
    a.part = (float*)((char*)ws + ws_wgpart_offset(c));
    a.mvalid = 0; a.nvalid = 0;
    a.Ntok = (int)Ntok; a.F = c.F; a.T = c.T; a.shift_stride = 1; a.shift_dim = 0; a.groups = 1; a.taps = 1;
    a.stats = nullptr; a.gamma = nullptr; a.beta = nullptr;
}
// dW[M][K] += A^T B over the rows, dbias += colsum(A).  M in slices whose tiles fit one workgroup of wgrad.hip's transposing-read kernel
// (<= 112 tiles of 16 x 16, <= 7 staging slots): as one 576 x 192 problem the in_proj gradient took the column-range fallback with its
// atomic flush (17.8 % of the large train step for the five dense problems of a layer)
static int gb_wgrad_dense(const nbss_cfg& c, void* ws, const void* A, int lda, int M, const void* B, int ldb, int K, float* dW, float* dbias, long Ntok,
                          hipStream_t st) {
    const size_t esz = c.dtype == NBSS_BF16 ? 2 : 4;
    if (c.dtype == NBSS_BF16) {  // 192 x 96 output tiles with fragment reuse (wgrad_g.hip) where the shape allows
        const int e = wgrad_dense_g(A, lda, M, B, ldb, K, dW, dbias, Ntok, (float*)((char*)ws + ws_wgpart_offset(c)), st);
        if (e != NBSS_EUNSUPPORTED) return e;
    }
    int mt = 112 / cdiv(K, 16);
    if (mt > 12) mt = 12;
    while (mt > 1 && cdiv(mt * 16, 64) + cdiv(K, 64) > 7) --mt;
    const int ms = mt * 16;
    for (int m0 = 0; m0 < M; m0 += ms) {
        const int mm = M - m0 < ms ? M - m0 : ms;
        WgradArgs a;
        gb_wgrad_base(a, c, ws, Ntok);
        a.A = (const char*)A + (size_t)m0 * esz; a.lda = lda; a.MA = mm;
        a.B = B; a.ldb = ldb; a.NB = K;
        a.dW = dW + (size_t)m0 * K; a.dbias = dbias ? dbias + m0 : nullptr;
        int e = wgrad_launch(a, c.dtype, st);
        if (e) return e;
    }
    return NBSS_OK;
}

// ---- F-conv block (SpatialNet.py:116-127): y = x + PReLU(conv_F(LN(x))) ----------------------------------------------------------------
template <class T>
static int gb_fconv_bwd_t(const nbss_cfg& c, const float* P, float* G, int layer, int which, const void* x, const void* dy, void* dx, void* ws, hipStream_t st,
                          const Side* sd) {
    const LayerPtrs lp = layer_ptrs(c, P, layer);
    const long N = (long)c.B * c.F * c.T;
    const int H = c.H, CG = H / c.f_groups, Mp = pad16(CG), Kp = pad32(CG);
    const int pLW = which ? P_FC2_LN_W : P_FC1_LN_W, pLB = which ? P_FC2_LN_B : P_FC1_LN_B, pW = which ? P_FC2_W : P_FC1_W, pB = which ? P_FC2_B : P_FC1_B,
              pA = which ? P_FC2_PRELU : P_FC1_PRELU;
    float* stats = (float*)ws;
    GbArena ar = gb_arena(c, ws);
    if (sizeof(T) == 2 && fconv_g_takes(c)) {  // the whole block in one kernel per (b, t) slab (fconv_g.hip)
        void* dv = ar.take(N * H * sizeof(T));
        void* wfr = ar.take(fconv_g_wfrag_elems() * sizeof(T));
        void* wdr = ar.take(fconv_g_wfrag_elems() * sizeof(T));
        if (!wdr) return NBSS_EUNSUPPORTED;
        int e = fconv_g_bwd(c, P, G, layer, which, x, dy, dx, dv, stats, wfr, wdr, gb_part_floats(c) >= (size_t)c.B * c.T * 576 ? gb_part(c, ws) : nullptr, st);
        if (e) return e;
        // conv weight: dW[o][i][tap] = sum_n dv[n][o] LN(x)[n + (tap - 2) T][i] (LayerNorm applied on the fly from the statistics), bias = colsum(dv)
        const hipStream_t gs = side_fork(sd, st);
        WgradArgs wa;
        gb_wgrad_base(wa, c, ws, N);
        wa.shift_stride = c.T; wa.shift_dim = 1; wa.groups = c.f_groups; wa.taps = c.f_ks;
        wa.A = dv; wa.lda = H; wa.MA = H; wa.B = x; wa.ldb = H; wa.NB = H;
        wa.stats = stats; wa.gamma = lp.p[pLW]; wa.beta = lp.p[pLB];
        wa.dW = G + param_off(c, layer, pW); wa.dbias = G + param_off(c, layer, pB);
        return wgrad_launch(wa, c.dtype, gs);
    }
    void* u = ar.take(N * H * sizeof(T));
    void* a = ar.take(N * H * sizeof(T));
    void* da = ar.take(N * H * sizeof(T));
    void* du = ar.take(N * H * sizeof(T));
    void* wf = ar.take((size_t)c.f_groups * c.f_ks * Mp * Kp * sizeof(T));
    void* wd = ar.take((size_t)c.f_groups * c.f_ks * Mp * Kp * sizeof(T));
    if (!wd) return NBSS_EUNSUPPORTED;
    int e;
    if ((e = gb_wprep<T>(lp.p[pW], wf, WP_CONV_FWD, c.f_groups, c.f_ks, CG, CG, Mp, Kp, st))) return e;
    if ((e = gb_wprep<T>(lp.p[pW], wd, WP_CONV_DGRAD, c.f_groups, c.f_ks, CG, CG, Mp, Kp, st))) return e;
    if ((e = gb_ln_fwd<T>(x, lp.p[pLW], lp.p[pLB], u, stats, N, H, st))) return e;
    // a = conv along F (rows T apart, position f = (n / T) % F)
    if ((e = gb_gemm<T>(gb_conv(u, wf, lp.p[pB], a, N, H, c.f_groups, c.f_ks, c.T, c.T, c.F), st))) return e;
    if ((e = gb_prelu_bwd<T>(a, dy, lp.p[pA], da, G + param_off(c, layer, pA), N, H, st))) return e;
    if ((e = gb_gemm<T>(gb_conv(da, wd, nullptr, du, N, H, c.f_groups, c.f_ks, c.T, c.T, c.F), st))) return e;
    if ((e = gb_ln_bwd<T>(du, x, stats, lp.p[pLW], dy, dx, G + param_off(c, layer, pLW), G + param_off(c, layer, pLB), N, H, st, gb_part(c, ws), gb_part_floats(c)))) return e;
    // conv weight: dW[o][i][tap] = sum_n da[n][o] u[n + (tap - 2) T][i], bias = colsum(da)
    const hipStream_t gs = side_fork(sd, st);
    WgradArgs wa;
    gb_wgrad_base(wa, c, ws, N);
    wa.shift_stride = c.T; wa.shift_dim = 1; wa.groups = c.f_groups; wa.taps = c.f_ks;
    wa.A = da; wa.lda = H; wa.MA = H; wa.B = u; wa.ldb = H; wa.NB = H;
    wa.dW = G + param_off(c, layer, pW); wa.dbias = G + param_off(c, layer, pB);
    return wgrad_launch(wa, c.dtype, gs);
}

// ---- full-band block (SpatialNet.py:129-146): y = x + SiLU(Wu LinearGroup_F(SiLU(Ws LN(x) + bs)) + bu) ---------------------------------
template <class T>
static int gb_full_bwd_t(const nbss_cfg& c, const float* P, float* G, int layer, const void* x, const void* dy, void* dx, void* ws, hipStream_t st, const Side* sd) {
    const LayerPtrs lp = layer_ptrs(c, P, layer);
    const long N = (long)c.B * c.F * c.T, BT = (long)c.B * c.T;
    const int H = c.H, SQ = c.SQ, F = c.F, FK = pad8(F);
    float* stats = (float*)ws;
    GbArena ar = gb_arena(c, ws);
    void* u = ar.take(N * H * sizeof(T));
    void* sp = ar.take(N * SQ * sizeof(T));    // squeeze pre-activation, later ds_pre
    void* s = ar.take(N * SQ * sizeof(T));     // SiLU(sp), later ds
    void* sT = ar.take(BT * SQ * FK * sizeof(T));
    void* zT = ar.take(BT * SQ * FK * sizeof(T));   // later ds^T
    void* z = ar.take(N * SQ * sizeof(T));     // later dz
    void* dzT = ar.take(BT * SQ * FK * sizeof(T));
    void* yp = ar.take(N * H * sizeof(T));     // unsqueeze pre-activation
    void* dyp = ar.take(N * H * sizeof(T));    // later du
    const int Fp16 = pad16(F), Fp32 = pad32(FK);
    void* w_sq = ar.take((size_t)pad16(SQ) * pad32(H) * sizeof(T));
    void* w_sqT = ar.take((size_t)pad16(H) * pad32(SQ) * sizeof(T));
    void* w_us = ar.take((size_t)pad16(H) * pad32(SQ) * sizeof(T));
    void* w_usT = ar.take((size_t)pad16(SQ) * pad32(H) * sizeof(T));
    void* w_lg = ar.take((size_t)SQ * Fp16 * Fp32 * sizeof(T));
    void* w_lgT = ar.take((size_t)SQ * Fp16 * Fp32 * sizeof(T));
    if (!w_lgT) return NBSS_EUNSUPPORTED;
    int e;
    {
        WPrepBatch<T> wb;
        wb.add(lp.p[P_SQ_W], w_sq, WP_LIN_FWD, 1, 1, SQ, H, pad16(SQ), pad32(H));
        wb.add(lp.p[P_SQ_W], w_sqT, WP_LIN_DGRAD, 1, 1, H, SQ, pad16(H), pad32(SQ));
        wb.add(lp.p[P_USQ_W], w_us, WP_LIN_FWD, 1, 1, H, SQ, pad16(H), pad32(SQ));
        wb.add(lp.p[P_USQ_W], w_usT, WP_LIN_DGRAD, 1, 1, SQ, H, pad16(SQ), pad32(H));
        wb.add(lp.p[P_FULL_W], w_lg, WP_LG_FWD, SQ, 1, F, F, Fp16, Fp32);
        wb.add(lp.p[P_FULL_W], w_lgT, WP_LG_DGRAD, SQ, 1, F, F, Fp16, Fp32);
        if ((e = wb.launch(st))) return e;
    }
    // forward chain
    if ((e = gb_ln_fwd<T>(x, lp.p[P_FULL_LN_W], lp.p[P_FULL_LN_B], u, stats, N, H, st))) return e;
    {
        TapGemm p = gb_lin(u, H, w_sq, lp.p[P_SQ_B], sp, SQ, N, SQ, H);
        p.Y2 = s;  // s = SiLU(s_pre) in the same pass
        if ((e = gb_gemm<T>(p, st))) return e;
    }
    if ((e = gb_sq_to_f<T>(s, sT, c.B, F, c.T, SQ, FK, st))) return e;
    auto lg = [&](const void* X, const void* Wp, const float* bias, void* Y) {
        TapGemm p = gb_lin(X, SQ * FK, Wp, bias, Y, SQ * FK, BT, F, FK);
        p.groups = SQ; p.xgs = FK; p.ygs = FK; p.bgs = F;
        p.Mp = Fp16; p.Kp = Fp32;
        return p;
    };
    if ((e = gb_gemm<T>(lg(sT, w_lg, lp.p[P_FULL_B], zT), st))) return e;
    if ((e = gb_f_to_sq<T>(zT, z, c.B, F, c.T, SQ, FK, st))) return e;
    if ((e = gb_gemm<T>(gb_lin(z, SQ, w_us, lp.p[P_USQ_B], yp, H, N, H, SQ), st))) return e;
    // backward chain
    if ((e = gb_silu_bwd<T>(yp, dy, dyp, N * H, st))) return e;                               // dy_pre
    void* dz = ar.take(N * SQ * sizeof(T));
    void* ds = ar.take(N * SQ * sizeof(T));
    if (!ds) return NBSS_EUNSUPPORTED;
    if ((e = gb_gemm<T>(gb_lin(dyp, H, w_usT, nullptr, dz, SQ, N, SQ, H), st))) return e;      // dz = Wu^T dy_pre
    if ((e = gb_sq_to_f<T>(dz, dzT, c.B, F, c.T, SQ, FK, st))) return e;
    void* dsT = ar.take(BT * SQ * FK * sizeof(T));
    if (!dsT) return NBSS_EUNSUPPORTED;
    if ((e = gb_gemm<T>(lg(dzT, w_lgT, nullptr, dsT), st))) return e;                         // ds^T = Wf^T dz^T
    if ((e = gb_f_to_sq<T>(dsT, ds, c.B, F, c.T, SQ, FK, st))) return e;
    if ((e = gb_silu_bwd<T>(sp, ds, ds, N * SQ, st))) return e;                               // ds_pre (in ds)
    void* du = ar.take(N * H * sizeof(T));
    if (!du) return NBSS_EUNSUPPORTED;
    if ((e = gb_gemm<T>(gb_lin(ds, SQ, w_sqT, nullptr, du, H, N, H, SQ), st))) return e;
    if ((e = gb_ln_bwd<T>(du, x, stats, lp.p[P_FULL_LN_W], dy, dx, G + param_off(c, layer, P_FULL_LN_W), G + param_off(c, layer, P_FULL_LN_B), N, H, st, gb_part(c, ws), gb_part_floats(c)))) return e;
    // weight gradients
    const hipStream_t gs = side_fork(sd, st);
    if ((e = gb_wgrad_dense(c, ws, dyp, H, H, z, SQ, SQ, G + param_off(c, layer, P_USQ_W), G + param_off(c, layer, P_USQ_B), N, gs))) return e;
    WgradArgs wa;
    gb_wgrad_base(wa, c, ws, BT);
    wa.groups = SQ; wa.mvalid = F; wa.nvalid = F;
    wa.A = dzT; wa.lda = SQ * FK; wa.MA = SQ * FK; wa.B = sT; wa.ldb = SQ * FK; wa.NB = SQ * FK;
    wa.dW = G + param_off(c, layer, P_FULL_W); wa.dbias = G + param_off(c, layer, P_FULL_B);
    if ((e = wgrad_launch(wa, c.dtype, gs))) return e;
    return gb_wgrad_dense(c, ws, ds, SQ, SQ, u, H, H, G + param_off(c, layer, P_SQ_W), G + param_off(c, layer, P_SQ_B), N, gs);
}

// ---- attention block (SpatialNet.py:93-100): y = x + out_proj(MHSA(LN(x))) ---------------------------------------------------------------
template <class T>
static int gb_mhsa_bwd_t(const nbss_cfg& c, const float* P, float* G, int layer, const void* x, const void* dy, void* dx, void* ws, hipStream_t st, const Side* sd) {
    const LayerPtrs lp = layer_ptrs(c, P, layer);
    const long N = (long)c.B * c.F * c.T;
    const int H = c.H, DH = H / c.heads;
    float* stats = (float*)ws;
    GbArena ar = gb_arena(c, ws);
    void* u = ar.take(N * H * sizeof(T));
    void* qkv = ar.take(N * 3 * H * sizeof(T));
    void* dO = ar.take(N * H * sizeof(T));
    void* O = ar.take(N * H * sizeof(T));
    void* dqkv = ar.take(N * 3 * H * sizeof(T));
    void* du = ar.take(N * H * sizeof(T));
    float* lse = (float*)ar.take(N * c.heads * sizeof(float));
    float* Dv = (float*)ar.take(N * c.heads * sizeof(float));
    void* w_in = ar.take((size_t)pad16(3 * H) * pad32(H) * sizeof(T));
    void* w_inT = ar.take((size_t)pad16(H) * pad32(3 * H) * sizeof(T));
    void* w_outT = ar.take((size_t)pad16(H) * pad32(H) * sizeof(T));
    if (!w_outT) return NBSS_EUNSUPPORTED;
    int e;
    {
        WPrepBatch<T> wb;
        wb.add(lp.p[P_INP_W], w_in, WP_LIN_FWD, 1, 1, 3 * H, H, pad16(3 * H), pad32(H));
        wb.add(lp.p[P_INP_W], w_inT, WP_LIN_DGRAD, 1, 1, H, 3 * H, pad16(H), pad32(3 * H));
        wb.add(lp.p[P_OUTP_W], w_outT, WP_LIN_DGRAD, 1, 1, H, H, pad16(H), pad32(H));
        if ((e = wb.launch(st))) return e;
    }
    if ((e = gb_ln_fwd<T>(x, lp.p[P_MH_LN_W], lp.p[P_MH_LN_B], u, stats, N, H, st))) return e;
    if ((e = gb_gemm<T>(gb_lin(u, H, w_in, lp.p[P_INP_B], qkv, 3 * H, N, 3 * H, H), st))) return e;
    if ((e = gb_gemm<T>(gb_lin(dy, H, w_outT, nullptr, dO, H, N, H, H), st))) return e;  // dO = dy Wo
    if (DH == 48) e = gb_attn_launch<T, 48>(c, qkv, dO, O, dqkv, lse, Dv, st);
    else if (DH == 24) e = gb_attn_launch<T, 24>(c, qkv, dO, O, dqkv, lse, Dv, st);
    else e = NBSS_EUNSUPPORTED;
    if (e) return e;
    if ((e = gb_gemm<T>(gb_lin(dqkv, 3 * H, w_inT, nullptr, du, H, N, H, 3 * H), st))) return e;
    if ((e = gb_ln_bwd<T>(du, x, stats, lp.p[P_MH_LN_W], dy, dx, G + param_off(c, layer, P_MH_LN_W), G + param_off(c, layer, P_MH_LN_B), N, H, st, gb_part(c, ws), gb_part_floats(c)))) return e;
    const hipStream_t gs = side_fork(sd, st);
    if ((e = gb_wgrad_dense(c, ws, dy, H, H, O, H, H, G + param_off(c, layer, P_OUTP_W), G + param_off(c, layer, P_OUTP_B), N, gs))) return e;
    return gb_wgrad_dense(c, ws, dqkv, 3 * H, 3 * H, u, H, H, G + param_off(c, layer, P_INP_W), G + param_off(c, layer, P_INP_B), N, gs);
}

// ---- T-ConvFFN block (SpatialNet.py:102-114) -----------------------------------------------------------------------------------------------
template <class T>
static int gb_tconvffn_bwd_t(const nbss_cfg& c, const float* P, float* G, int layer, const void* x, const void* dy, void* dx, void* ws, hipStream_t st,
                             const Side* sd) {
    const LayerPtrs lp = layer_ptrs(c, P, layer);
    const long N = (long)c.B * c.F * c.T;
    const int H = c.H, FFN = c.FFN, CG = FFN / c.t_groups, nseq = c.B * c.F;
    if (CG > 64) return NBSS_EUNSUPPORTED;
    float* stats = (float*)ws;
    GbArena ar = gb_arena(c, ws);
    void* u = ar.take(N * H * sizeof(T));
    void* du = ar.take(N * H * sizeof(T));
    void* t[12];  // a1 h1 a2 h2 a3 h4 a5 h5 | g5 g3 g2 g1
    for (int i = 0; i < 12; ++i) t[i] = ar.take(N * FFN * sizeof(T));
    void *a1 = t[0], *h1 = t[1], *a2 = t[2], *h2 = t[3], *a3 = t[4], *h4 = t[5], *a5 = t[6], *h5 = t[7], *g5 = t[8], *g3 = t[9], *g2 = t[10], *g1 = t[11];
    float* gstats = (float*)ar.take((size_t)nseq * c.t_groups * 2 * sizeof(float));
    const int Mp = pad16(CG), Kp = pad32(CG);
    void* w1 = ar.take((size_t)pad16(FFN) * pad32(H) * sizeof(T));
    void* w1T = ar.take((size_t)pad16(H) * pad32(FFN) * sizeof(T));
    void* w2T = ar.take((size_t)pad16(FFN) * pad32(H) * sizeof(T));
    void* cw[3], *cwT[3];
    for (int k = 0; k < 3; ++k) {
        cw[k] = ar.take((size_t)c.t_groups * c.t_ks * Mp * Kp * sizeof(T));
        cwT[k] = ar.take((size_t)c.t_groups * c.t_ks * Mp * Kp * sizeof(T));
    }
    if (!cwT[2]) return NBSS_EUNSUPPORTED;
    const int convW[3] = {P_TF_C1W, P_TF_C2W, P_TF_C3W}, convB[3] = {P_TF_C1B, P_TF_C2B, P_TF_C3B};
    int e;
    {
        WPrepBatch<T> wb;
        wb.add(lp.p[P_TF_W1], w1, WP_LIN_FWD, 1, 1, FFN, H, pad16(FFN), pad32(H));
        wb.add(lp.p[P_TF_W1], w1T, WP_LIN_DGRAD, 1, 1, H, FFN, pad16(H), pad32(FFN));
        wb.add(lp.p[P_TF_W2], w2T, WP_LIN_DGRAD, 1, 1, FFN, H, pad16(FFN), pad32(H));
        if ((e = wb.launch(st))) return e;
    }
    auto with = [](TapGemm p, void* y2, const void* dact) {  // second output SiLU(Y) / result times SiLU'(dact): the activation passes ride along
        p.Y2 = y2;
        p.Dact = dact;
        return p;
    };
    if ((e = gb_ln_fwd<T>(x, lp.p[P_TF_LN_W], lp.p[P_TF_LN_B], u, stats, N, H, st))) return e;
    if (tc_chain_takes(c.dtype, CG, c.t_ks, c.T)) {
        // the conv chain between the two dense maps in ONE kernel per layer (tchain.hip): a1 and dh5 in, every operand of the weight gradients out
        void* dh5 = a2;  // (the buffers of the pre-activations the chain keeps in registers)
        TChain tc;
        const float* wsrc[3];
        for (int k = 0; k < 3; ++k) {
            wsrc[k] = lp.p[convW[k]];
            tc.wf[k] = cw[k];
            tc.wd[k] = cwT[k];
            tc.cb[k] = lp.p[convB[k]];
        }
        if (tc_wfrag_elems(c.t_groups, CG, c.t_ks) > (size_t)c.t_groups * c.t_ks * Mp * Kp) return NBSS_EUNSUPPORTED;
        {
            void* wfv[3] = {cw[0], cw[1], cw[2]};
            void* wdv[3] = {cwT[0], cwT[1], cwT[2]};
            if ((e = tc_wprep(wsrc, wfv, wdv, c.t_groups, CG, c.t_ks, st))) return e;
        }
        if ((e = gb_gemm<T>(gb_lin(u, H, w1, lp.p[P_TF_B1], a1, FFN, N, FFN, H), st))) return e;
        if ((e = gb_gemm<T>(gb_lin(dy, H, w2T, nullptr, dh5, FFN, N, FFN, H), st))) return e;
        tc.a1 = a1; tc.dh5 = dh5;
        tc.gn_w = lp.p[P_TF_GN_W]; tc.gn_b = lp.p[P_TF_GN_B];
        tc.h1 = h1; tc.h2 = h2; tc.h4 = h4; tc.h5 = h5; tc.g5 = g5; tc.g3 = g3; tc.g2 = g2; tc.g1 = g1;
        tc.dgn_w = G + param_off(c, layer, P_TF_GN_W); tc.dgn_b = G + param_off(c, layer, P_TF_GN_B);
        tc.part = gb_part_floats(c) >= (size_t)nseq * 2 * FFN ? gb_part(c, ws) : nullptr;
        tc.nseq = nseq; tc.T = c.T; tc.FFN = FFN; tc.groups = c.t_groups;
        if ((e = tc_chain_launch(tc, CG, c.t_ks, true, st))) return e;
        if (tc.part) {
            AffSegs sg;
            sg.n = 2;
            sg.off[0] = param_off(c, layer, P_TF_GN_W); sg.off[1] = param_off(c, layer, P_TF_GN_B);
            sg.cnt[0] = sg.cnt[1] = FFN;
            if ((e = affine_reduce_launch(tc.part, nseq, sg, G, st))) return e;
        }
    } else {
        for (int k = 0; k < 3; ++k) {
            if ((e = gb_wprep<T>(lp.p[convW[k]], cw[k], WP_CONV_FWD, c.t_groups, c.t_ks, CG, CG, Mp, Kp, st))) return e;
            if ((e = gb_wprep<T>(lp.p[convW[k]], cwT[k], WP_CONV_DGRAD, c.t_groups, c.t_ks, CG, CG, Mp, Kp, st))) return e;
        }
        auto tconv = [&](const void* X, const void* Wp, const float* bias, void* Y) {  // along T: rows 1 apart, position t = n % T
            return gb_conv(X, Wp, bias, Y, N, FFN, c.t_groups, c.t_ks, 1, 1, c.T);
        };
        // forward chain, every pre-activation and activation kept
        if ((e = gb_gemm<T>(with(gb_lin(u, H, w1, lp.p[P_TF_B1], a1, FFN, N, FFN, H), h1, nullptr), st))) return e;
        if ((e = gb_gemm<T>(with(tconv(h1, cw[0], lp.p[convB[0]], a2), h2, nullptr), st))) return e;
        if ((e = gb_gemm<T>(tconv(h2, cw[1], lp.p[convB[1]], a3), st))) return e;
        if ((e = gb_gn_fwd<T>(a3, lp.p[P_TF_GN_W], lp.p[P_TF_GN_B], h4, gstats, nseq * c.t_groups, c.T, FFN, CG, 1, st))) return e;
        if ((e = gb_gemm<T>(with(tconv(h4, cw[2], lp.p[convB[2]], a5), h5, nullptr), st))) return e;
        // backward chain: g5 = da5, g3 = da3 (through the GroupNorm), g2 = da2, g1 = da1
        if ((e = gb_gemm<T>(with(gb_lin(dy, H, w2T, nullptr, g5, FFN, N, FFN, H), nullptr, a5), st))) return e;
        if ((e = gb_gemm<T>(tconv(g5, cwT[2], nullptr, g3), st))) return e;
        if ((e = gb_gn_bwd<T>(a3, gstats, lp.p[P_TF_GN_W], lp.p[P_TF_GN_B], g3, G + param_off(c, layer, P_TF_GN_W), G + param_off(c, layer, P_TF_GN_B), nseq * c.t_groups,
                              c.T, FFN, CG, st)))
            return e;
        if ((e = gb_gemm<T>(with(tconv(g3, cwT[1], nullptr, g2), nullptr, a2), st))) return e;
        if ((e = gb_gemm<T>(with(tconv(g2, cwT[0], nullptr, g1), nullptr, a1), st))) return e;
    }
    if ((e = gb_gemm<T>(gb_lin(g1, FFN, w1T, nullptr, du, H, N, H, FFN), st))) return e;
    if ((e = gb_ln_bwd<T>(du, x, stats, lp.p[P_TF_LN_W], dy, dx, G + param_off(c, layer, P_TF_LN_W), G + param_off(c, layer, P_TF_LN_B), N, H, st, gb_part(c, ws), gb_part_floats(c)))) return e;
    // weight gradients (every operand above is still in place: nothing was overwritten)
    const hipStream_t gs = side_fork(sd, st);
    if ((e = gb_wgrad_dense(c, ws, dy, H, H, h5, FFN, FFN, G + param_off(c, layer, P_TF_W2), G + param_off(c, layer, P_TF_B2), N, gs))) return e;
    const void* cA[3] = {g2, g3, g5};
    const void* cB[3] = {h1, h2, h4};
    for (int k = 0; k < 3; ++k) {
        WgradArgs wa;
        gb_wgrad_base(wa, c, ws, N);
        wa.groups = c.t_groups; wa.taps = c.t_ks;
        wa.A = cA[k]; wa.lda = FFN; wa.MA = FFN; wa.B = cB[k]; wa.ldb = FFN; wa.NB = FFN;
        wa.dW = G + param_off(c, layer, convW[k]); wa.dbias = G + param_off(c, layer, convB[k]);
        if ((e = wgrad_launch(wa, c.dtype, gs))) return e;
    }
    return gb_wgrad_dense(c, ws, g1, FFN, FFN, u, H, H, G + param_off(c, layer, P_TF_W1), G + param_off(c, layer, P_TF_B1), N, gs);
}

// ---- T-ConvFFN forward on the same pieces (bf16 stream): LN -> dense map -> conv chain -> dense map + residual.  tconvffn_g.hip's one-kernel
// forward walks a sequence's 8 groups serially with every weight fragment from L2 (1.1 ms per layer at batch 4); these four launches take a third.
int gb_tconvffn_fwd(const nbss_cfg& c, const float* P, int layer, const void* x, void* y, void* ws, hipStream_t st) {
    typedef bf16_t T;
    const LayerPtrs lp = layer_ptrs(c, P, layer);
    const long N = (long)c.B * c.F * c.T;
    const int H = c.H, FFN = c.FFN, CG = FFN / c.t_groups;
    if (!ws || !tc_chain_takes(c.dtype, CG, c.t_ks, c.T)) return NBSS_EUNSUPPORTED;
    ProfScope ps(PK_TCF_F, st);
    float* stats = (float*)ws;
    GbArena ar = gb_arena(c, ws);
    void* u = ar.take(N * H * sizeof(T));
    void* a1 = ar.take(N * FFN * sizeof(T));
    void* h5 = ar.take(N * FFN * sizeof(T));
    void* w1 = ar.take((size_t)pad16(FFN) * pad32(H) * sizeof(T));
    void* w2 = ar.take((size_t)pad16(H) * pad32(FFN) * sizeof(T));
    void* cw[3];
    for (int k = 0; k < 3; ++k) cw[k] = ar.take(tc_wfrag_elems(c.t_groups, CG, c.t_ks) * sizeof(T));
    if (!cw[2]) return NBSS_EUNSUPPORTED;
    int e;
    {
        WPrepBatch<T> wb;
        wb.add(lp.p[P_TF_W1], w1, WP_LIN_FWD, 1, 1, FFN, H, pad16(FFN), pad32(H));
        wb.add(lp.p[P_TF_W2], w2, WP_LIN_FWD, 1, 1, H, FFN, pad16(H), pad32(FFN));
        if ((e = wb.launch(st))) return e;
    }
    const float* wsrc[3] = {lp.p[P_TF_C1W], lp.p[P_TF_C2W], lp.p[P_TF_C3W]};
    void* none[3] = {nullptr, nullptr, nullptr};
    if ((e = tc_wprep(wsrc, cw, none, c.t_groups, CG, c.t_ks, st))) return e;
    if ((e = gb_ln_fwd<T>(x, lp.p[P_TF_LN_W], lp.p[P_TF_LN_B], u, stats, N, H, st))) return e;
    if ((e = gb_gemm<T>(gb_lin(u, H, w1, lp.p[P_TF_B1], a1, FFN, N, FFN, H), st))) return e;
    TChain tc = {};
    tc.a1 = a1;
    for (int k = 0; k < 3; ++k) tc.wf[k] = cw[k];
    tc.cb[0] = lp.p[P_TF_C1B]; tc.cb[1] = lp.p[P_TF_C2B]; tc.cb[2] = lp.p[P_TF_C3B];
    tc.gn_w = lp.p[P_TF_GN_W]; tc.gn_b = lp.p[P_TF_GN_B];
    tc.h5 = h5;
    tc.nseq = c.B * c.F; tc.T = c.T; tc.FFN = FFN; tc.groups = c.t_groups;
    if ((e = tc_chain_launch(tc, CG, c.t_ks, false, st))) return e;
    TapGemm p2 = gb_lin(h5, FFN, w2, lp.p[P_TF_B2], y, H, N, H, FFN);
    p2.R = x; p2.ldr = H;
    return gb_gemm<T>(p2, st);
}

// ---- decoder (SpatialNet.py:200,216): out = Wd x + bd; dx = Wd^T dout ---------------------------------------------------------------------
template <class T>
static int gb_decoder_bwd_t(const nbss_cfg& c, const float* P, float* G, const void* x, const float* dout, void* dx, void* ws, hipStream_t st) {
    const long N = (long)c.B * c.F * c.T;
    const int H = c.H, Co = c.C_out, CP = pad8(Co);
    GbArena ar = gb_arena(c, ws);
    void* dpad = ar.take(N * CP * sizeof(T));
    void* wT = ar.take((size_t)pad16(H) * pad32(CP) * sizeof(T));
    if (!wT) return NBSS_EUNSUPPORTED;
    int e;
    if ((e = gb_pad_cols<T>(dout, dpad, N, Co, CP, st))) return e;
    // W^T as a tap_gemm weight: M = H inputs of the decoder, K = its outputs (valid Co, stored CP wide)
    if ((e = gb_wprep<T>(P + param_off_dec_w(c), wT, WP_LIN_DGRAD, 1, 1, H, Co, pad16(H), pad32(CP), st))) return e;
    TapGemm p = gb_lin(dpad, CP, wT, nullptr, dx, H, N, H, CP);
    if ((e = gb_gemm<T>(p, st))) return e;
    WgradArgs wa;
    gb_wgrad_base(wa, c, ws, N);
    wa.mvalid = Co;
    wa.A = dpad; wa.lda = CP; wa.MA = CP; wa.B = x; wa.ldb = H; wa.NB = H;
    wa.dW = G + param_off_dec_w(c); wa.dbias = G + param_off_dec_b(c);
    return wgrad_launch(wa, c.dtype, st);
}

// ---- entry points (capi.hip dispatches here for every geometry but SpatialNet-small) ----------------------------------------------------------
#define GB_DISPATCH(fn, ...) (c.dtype == NBSS_BF16 ? fn<bf16_t>(__VA_ARGS__) : fn<float>(__VA_ARGS__))
int gb_fconv_bwd(const nbss_cfg& c, const float* P, float* G, int layer, int which, const void* x, const void* dy, void* dx, void* ws, hipStream_t st, const Side* sd) {
    ProfScope ps(PK_FCONV_B, st);
    return GB_DISPATCH(gb_fconv_bwd_t, c, P, G, layer, which, x, dy, dx, ws, st, sd);
}
int gb_full_bwd(const nbss_cfg& c, const float* P, float* G, int layer, const void* x, const void* dy, void* dx, void* ws, hipStream_t st, const Side* sd) {
    ProfScope ps(PK_FULL_B, st);
    return GB_DISPATCH(gb_full_bwd_t, c, P, G, layer, x, dy, dx, ws, st, sd);
}
int gb_mhsa_bwd(const nbss_cfg& c, const float* P, float* G, int layer, const void* x, const void* dy, void* dx, void* ws, hipStream_t st, const Side* sd) {
    ProfScope ps(PK_MHSA_B, st);
    return GB_DISPATCH(gb_mhsa_bwd_t, c, P, G, layer, x, dy, dx, ws, st, sd);
}
int gb_tconvffn_bwd(const nbss_cfg& c, const float* P, float* G, int layer, const void* x, const void* dy, void* dx, void* ws, hipStream_t st, const Side* sd) {
    ProfScope ps(PK_TCF_B, st);
    return GB_DISPATCH(gb_tconvffn_bwd_t, c, P, G, layer, x, dy, dx, ws, st, sd);
}
int gb_decoder_bwd(const nbss_cfg& c, const float* P, float* G, const void* x, const float* dout, void* dx, void* ws, hipStream_t st) {
    return GB_DISPATCH(gb_decoder_bwd_t, c, P, G, x, dout, dx, ws, st);
}
