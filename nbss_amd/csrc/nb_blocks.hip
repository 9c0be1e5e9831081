// nb_blocks.hip — the narrow-band building blocks behind the C ABI (nbss_nb_*: include/nbss_hip.h; prototypes: nb.h).
// The generic pieces of gb.h, one operation per call on caller-owned tensors: what a narrow-band network other than SpatialNet (NBC2: pre-norm
// attention over time + convolutional feed-forward with GroupBatchNorm; NBC; NBC2-large) is sequenced from on the host side (nbss_amd/nbc2.py).
// The relative-position attention of NBC is attn_relpos.hip, head width 96 attn_kb.hip; the (dtype, head width) dispatch is attn_tiles.h's AT_DISPATCH.
#include "gb.h"
#include "attn_tiles.h"
#include "nb.h"
#include "wgrad.h"

size_t nb_ws_bytes_impl(int M, int K, int groups, int taps) { return ws_align((size_t)groups * taps * pad16(M / groups) * pad32(pad8(K / groups)) * sizeof(float)); }

#define NB_DISPATCH(fn, ...) (dtype == NBSS_BF16 ? fn<bf16_t>(__VA_ARGS__) : fn<float>(__VA_ARGS__))

// y = conv along T (dense: taps = groups = 1) of x [N][ldx] (valid columns Cin), SiLU on load / on store, + residual; y2 (optional) = SiLU(y)
template <class T>
static int nb_conv_t(long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const float* bias, void* y, void* y2,
                     const void* residual, int act_in, int act_out, void* ws, hipStream_t st) {
    if (groups <= 0 || Cin % groups || Cout % groups || (groups > 1 && ldx != Cin)) return NBSS_EINVAL;
    const int Kv = Cin / groups, Kg = groups > 1 ? Kv : pad8(Kv), Mg = Cout / groups;
    if (Kg % 8 || ldx < (groups > 1 ? Cin : Kg)) return NBSS_EUNSUPPORTED;
    int e = gb_wprep<T>(w, ws, taps > 1 || groups > 1 ? WP_CONV_FWD : WP_LIN_FWD, groups, taps, Mg, Kv, pad16(Mg), pad32(Kg), st);
    if (e) return e;
    TapGemm p = gb_lin(x, ldx, ws, bias, y, Cout, nseq * Tn, Mg, Kg);
    p.groups = groups; p.xgs = groups > 1 ? Kv : 0; p.ygs = groups > 1 ? Mg : 0; p.bgs = Mg;
    p.taps = taps; p.center = taps / 2; p.shift = 1; p.pos_div = 1; p.pos_len = Tn;
    p.xact = act_in; p.yact = act_out;
    p.R = residual; p.ldr = Cout;
    p.Y2 = y2;
    return gb_gemm<T>(p, st);
}
int nb_conv_t_impl(int dtype, long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const float* bias, void* y,
                   const void* residual, int act_in, int act_out, void* ws, hipStream_t st) {
    return NB_DISPATCH(nb_conv_t, nseq, Tn, Cin, ldx, Cout, groups, taps, x, w, bias, y, nullptr, residual, act_in, act_out, ws, st);
}
int nb_layernorm_impl(int dtype, long rows, int C, const void* x, const float* gamma, const float* beta, void* y, float* stats, hipStream_t st) {
    return NB_DISPATCH(gb_ln_fwd, x, gamma, beta, y, stats, rows, C, st);
}
int nb_gbn_impl(int dtype, int B, int F, int Tn, int C, const void* x, const float* gamma, const float* beta, float eps, int act, void* y, hipStream_t st) {
    return NB_DISPATCH(gb_gbn_fwd, x, gamma, beta, y, B, F, Tn, C, eps, act, st);
}
int nb_attention_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st) {
    if (heads <= 0 || H % heads) return NBSS_EINVAL;
    const int dh = H / heads;
    if (dh == 96) return nb_attention_kb_fwd_impl(dtype, nseq, Tn, H, heads, qkv, o, st);
    return AT_DISPATCH_NARROW(dtype, dh, nb_attn_fwd, nseq, Tn, H, heads, qkv, o, st);
}

// GroupNorm forward that keeps its (mean, rstd) per (sequence, group) for nb_group_norm_bwd_impl (dx in place of dy; dgamma / dbeta accumulated)
int nb_group_norm_train_impl(int dtype, long nseq, int Tn, int C, int groups, const void* x, const float* gamma, const float* beta, int act, void* y, float* stats,
                             hipStream_t st) {
    if (groups <= 0 || C % groups) return NBSS_EINVAL;
    return NB_DISPATCH(gb_gn_fwd, x, gamma, beta, y, stats, nseq * groups, Tn, C, C / groups, act, st);
}
int nb_group_norm_bwd_impl(int dtype, long nseq, int Tn, int C, int groups, const void* x, const float* stats, const float* gamma, const float* beta, void* dy_dx,
                           float* dgamma, float* dbeta, hipStream_t st) {
    if (groups <= 0 || C % groups) return NBSS_EINVAL;
    return NB_DISPATCH(gb_gn_bwd, x, stats, gamma, beta, dy_dx, dgamma, dbeta, nseq * groups, Tn, C, C / groups, st);
}
// GroupNorm(groups, C) over (C / groups x T) per sequence (eps 1e-5), optional SiLU: x, y [nseq][T][C]
int nb_group_norm_impl(int dtype, long nseq, int Tn, int C, int groups, const void* x, const float* gamma, const float* beta, int act, void* y, hipStream_t st) {
    return nb_group_norm_train_impl(dtype, nseq, Tn, C, groups, x, gamma, beta, act, y, nullptr, st);
}

// ---- training-mode building blocks (nbss_nb_*_train / _bwd: include/nbss_hip.h) ------------------------------------------------------------
// ws layout of the backward calls: [re-laid weights: nb_ws_bytes_impl()] [WGPART_BYTES of weight-gradient partial tiles]
size_t nb_bwd_ws_bytes_impl(int M, int K, int groups, int taps) {
    const size_t a = nb_ws_bytes_impl(M, K, groups, taps), b = nb_ws_bytes_impl(K, M, groups, taps);
    return (a > b ? a : b) + ws_align(WGPART_BYTES);
}
// the forward that also keeps y2 = SiLU(y) (no activation on load / on store: the backward call takes the pre-activation)
int nb_conv_t_train_impl(int dtype, long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const float* bias, void* y,
                         void* y2, const void* residual, void* ws, hipStream_t st) {
    return NB_DISPATCH(nb_conv_t, nseq, Tn, Cin, ldx, Cout, groups, taps, x, w, bias, y, y2, residual, 0, 0, ws, st);
}
// data gradient (dx [N][Cin] = conv^T(dy), optionally times SiLU'(dact)) and weight / bias gradient (dw [Cout][Cin / groups][taps] += dy^T x) of
// y = conv(x): x [N][ldx] is the tensor the forward call read (valid columns Cin), dy [N][Cout]
template <class T>
static int nb_conv_t_bwd(int dtype, long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const void* dy, const void* dact,
                         void* dx, float* dw, float* dbias, void* ws, hipStream_t st) {
    if (groups <= 0 || Cin % groups || Cout % groups || (groups > 1 && ldx != Cin)) return NBSS_EINVAL;
    const long N = nseq * Tn;
    const int Kv = Cin / groups, Mg = Cout / groups;
    int e;
    if (dx) {
        // the transposed map: outputs = the forward's inputs (Cin, written ldx wide: padding columns get zero weight rows), K = Cout
        if (Mg % 8 || (groups == 1 && ldx % 4)) return NBSS_EUNSUPPORTED;
        const int Mo = groups > 1 ? Kv : ldx;  // rows of the re-laid weight per group: valid Kv, the rest zero
        if ((e = gb_wprep<T>(w, ws, taps > 1 || groups > 1 ? WP_CONV_DGRAD : WP_LIN_DGRAD, groups, taps, Kv, Mg, pad16(Mo), pad32(Mg), st))) return e;
        TapGemm p = gb_lin(dy, Cout, ws, nullptr, dx, ldx, N, Mo, Mg);
        p.groups = groups; p.xgs = groups > 1 ? Mg : 0; p.ygs = groups > 1 ? Kv : 0; p.bgs = 0;
        p.taps = taps; p.center = taps / 2; p.shift = 1; p.pos_div = 1; p.pos_len = Tn;
        p.Dact = dact;
        if ((e = gb_gemm<T>(p, st))) return e;
    }
    if (dw) {
        if (Kv % 4 || Mg % 4) return NBSS_EUNSUPPORTED;
        float* part = (float*)((char*)ws + nb_bwd_ws_bytes_impl(Cout, Cin, groups, taps) - ws_align(WGPART_BYTES));
        const size_t esz = sizeof(T);
        // dense problems in row slices that fit one workgroup of the transposing-read kernel (gb_wgrad_dense's rule); grouped convs as one problem
        int mt = groups > 1 ? Cout / 16 + 1 : 112 / cdiv(Cin, 16);
        if (groups == 1) {
            if (mt > 12) mt = 12;
            while (mt > 1 && cdiv(mt * 16, 64) + cdiv(Cin, 64) > 7) --mt;
            if (mt < 1) mt = 1;
        }
        const int ms = groups > 1 ? Cout : mt * 16;
        for (int m0 = 0; m0 < Cout; m0 += ms) {
            const int mm = Cout - m0 < ms ? Cout - m0 : ms;
            WgradArgs a;
            a.part = part;
            a.mvalid = 0; a.nvalid = 0;
            a.Ntok = (int)N; a.F = (int)nseq; a.T = Tn; a.shift_stride = 1; a.shift_dim = 0;
            a.groups = groups; a.taps = taps;
            a.stats = nullptr; a.gamma = nullptr; a.beta = nullptr;
            a.A = (const char*)dy + (size_t)m0 * esz; a.lda = Cout; a.MA = mm;
            a.B = x; a.ldb = ldx; a.NB = Cin;
            a.dW = dw + (size_t)m0 * Kv * taps; a.dbias = dbias ? dbias + m0 : nullptr;
            if ((e = wgrad_launch(a, dtype, st))) return e;
        }
    }
    return NBSS_OK;
}
int nb_conv_t_bwd_impl(int dtype, long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const void* dy, const void* dact,
                       void* dx, float* dw, float* dbias, void* ws, hipStream_t st) {
    return NB_DISPATCH(nb_conv_t_bwd, dtype, nseq, Tn, Cin, ldx, Cout, groups, taps, x, w, dy, dact, dx, dw, dbias, ws, st);
}
int nb_layernorm_bwd_impl(int dtype, long rows, int C, const void* x, const float* stats, const float* gamma, const void* du, const void* dres, void* dx, float* dgamma,
                          float* dbeta, hipStream_t st) {
    return NB_DISPATCH(gb_ln_bwd, du, x, stats, gamma, dres, dx, dgamma, dbeta, rows, C, st);
}
int nb_gbn_bwd_impl(int dtype, int B, int F, int Tn, int C, const void* x, const float* gamma, const float* beta, float eps, int act, const void* dy, void* dx,
                    float* dgamma, float* dbeta, hipStream_t st) {
    return NB_DISPATCH(gb_gbn_bwd, x, gamma, beta, dy, dx, dgamma, dbeta, B, F, Tn, C, eps, act, st);
}
// attention backward from the packed projections: qkv [N][3H] (q | k | v), dO [N][H] -> dqkv [N][3H].  ws: O [N][H] (recomputed) | lse, D [N][heads] fp32
size_t nb_attn_bwd_ws_bytes_impl(long N, int H, int heads, int dtype) {
    return ws_align((size_t)N * H * (dtype == NBSS_BF16 ? 2 : 4)) + 2 * ws_align((size_t)N * heads * sizeof(float));
}
int nb_attention_bwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* dO, void* dqkv, void* ws, hipStream_t st) {
    if (heads <= 0 || H % heads) return NBSS_EINVAL;
    nbss_cfg c = {};
    c.B = 1; c.F = (int)nseq; c.T = Tn; c.H = H; c.heads = heads; c.dtype = dtype;
    const long N = nseq * Tn;
    void* O = ws;
    float* lse = (float*)((char*)ws + ws_align((size_t)N * H * (dtype == NBSS_BF16 ? 2 : 4)));
    float* Dv = (float*)((char*)lse + ws_align((size_t)N * heads * sizeof(float)));
    const int dh = H / heads;
    if (dh == 96) return nb_attention_kb_bwd_impl(dtype, nseq, Tn, H, heads, qkv, dO, O, dqkv, lse, Dv, st);
    return AT_DISPATCH_NARROW(dtype, dh, gb_attn_launch, c, qkv, dO, O, dqkv, lse, Dv, st);
}
