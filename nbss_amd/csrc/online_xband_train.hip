// online_xband_train.hip — the cross-band trio of an OnlineSpatialNet layer for TRAINING (reference: models/arch/OnlineSpatialNet.py `SpatialNetLayer.forward`):
//
//   x1 = x + fconv1(x);   x2 = x1 + full(x1);   y = x2 + fconv2(x2)                      x, y [B][F][T][96], stream dtype fp32 or bf16
//
// Those three blocks are not causal: with the shipped configuration they are SpatialNet-small's cross-band blocks, for which fconv.hip and full.hip hold the
// fused MFMA kernels (fconv_fwd_impl / fconv_bwd_impl / full_fwd_impl / full_bwd_impl).  This file REUSES them — nothing of theirs is copied or changed.  They
// read a flat SpatialNet parameter buffer (layout.h), a packed-fragment buffer (pack.hip) and an nbss_cfg; an OnlineSpatialNet has none of the three, so the
// entry points here take the module's 18 tensors by pointer and build all three inside the caller's workspace:
//   1. a one-layer SpatialNet-small nbss_cfg (L 1, full_share 0, C_in 4, C_out 2, groups (8, 8), kernels (5, 3));
//   2. xb_gather_kernel: the 18 tensors -> their slots of the flat buffer (they are adjacent there, in state_dict order); every other slot — encoder,
//      attention, T-ConvFFN, decoder — is written as zeros;
//   3. pack_params_impl on that buffer (the whole layer: pack.hip has no per-kind switch; the absent blocks pack zeros);
//   4. forward: fconv_fwd_impl(0) -> full_fwd_impl -> fconv_fwd_impl(1);  backward: the three *_bwd_impl in reverse with sd = nullptr (in order on the
//      caller's stream, like the per-block entry points of capi.hip) into a zeroed flat gradient region, then xb_scatter_kernel WRITES the 18 slices out.
// The device code of this file is the gather and the scatter; the rest is sequencing.  The backward repeats steps 2 and 3 (a few microseconds) instead of
// keeping them: `save` is exactly the two block inputs x1 and x2, and backward recomputes everything else from x, x1, x2 as the kernels always have.
// No atomics are added; the reused kernels fold in fixed orders: two calls give the same bits.
#include "launch.h"
#include "layout.h"
#include "side.h"

int pack_params_impl(const nbss_cfg& c, const float* params, void* packed, hipStream_t stream);
int fconv_fwd_impl(const nbss_cfg& c, const float* P, const void* packed, int layer, int which, const void* x, void* y, hipStream_t st);
int full_fwd_impl(const nbss_cfg& c, const float* P, const void* packed, int layer, const void* x, void* y, hipStream_t st);
int fconv_bwd_impl(const nbss_cfg& c, const float* P, float* G, const void* packed, int layer, int which, const void* x, const void* dy, void* dx,
                   void* ws, hipStream_t st, const Side* sd);
int full_bwd_impl(const nbss_cfg& c, const float* P, float* G, const void* packed, int layer, const void* x, const void* dy, void* dx, void* ws,
                  hipStream_t st, const Side* sd);

#define XB_NP 18  // P_FC1_LN_W .. P_FC2_PRELU: the first 18 parameters of a layer in layout.h
static_assert(P_FC1_LN_W == 0 && P_FC2_PRELU == XB_NP - 1 && P_MH_LN_W == XB_NP, "layout.h: the cross-band parameters lead a layer's block, in state_dict order");

static nbss_cfg xb_cfg(int dtype, int B, int F, int T) {
    nbss_cfg c;
    c.B = B; c.F = F; c.T = T;
    c.C_in = 4; c.C_out = 2;
    c.H = 96; c.FFN = 192; c.SQ = 8;
    c.L = 1; c.heads = 4;
    c.enc_ks = 5; c.f_ks = 5; c.t_ks = 3;
    c.f_groups = 8; c.t_groups = 8;
    c.full_share = 0;
    c.dtype = dtype;
    return c;
}
// backward (and a forward that keeps state for it) exists for these shapes only: a whole sequence per workgroup, and the fp32 F-conv backward's LDS images
static bool xb_trainable(const nbss_cfg& c) { return c.T <= NBSS_T_TRAIN_MAX && !(c.dtype == NBSS_F32 && c.F > 160); }

// ws = [flat parameters | packed fragments | two stream tensors (forward without `save`: x1, x2; backward: the gradients between the blocks)
//       | trainable shapes only: flat gradients | one workspace of the reused backward kernels]
struct XbGeom {
    size_t sb;  // one stream tensor
    size_t w_p, w_pk, w_t0, w_t1, w_g, w_ws, ws_total, save_total;
    long long total, lo, hi;  // floats of the flat buffer; [lo, hi): the 18 tensors
};
static XbGeom xb_geom(const nbss_cfg& c) {
    XbGeom g;
    const size_t esz = c.dtype == NBSS_BF16 ? 2 : 4;
    g.sb = ws_align((size_t)c.B * c.F * c.T * c.H * esz);
    g.total = param_total(c);
    g.lo = param_off(c, 0, P_FC1_LN_W);
    g.hi = param_off(c, 0, P_MH_LN_W);
    size_t o = 0;
    g.w_p = o; o += ws_align((size_t)g.total * sizeof(float));
    g.w_pk = o; o += ws_align((size_t)pack_total(c) * esz);
    g.w_t0 = o; o += g.sb;
    g.w_t1 = o; o += g.sb;
    g.w_g = o;
    g.w_ws = o;
    if (xb_trainable(c)) {
        o += ws_align((size_t)g.total * sizeof(float));
        g.w_ws = o; o += workspace_bytes(c);
    }
    g.ws_total = o;
    g.save_total = 2 * g.sb;
    return g;
}

// the 18 tensors and where each starts inside [lo, hi) of the flat buffer (off[XB_NP] = hi - lo); passed to the kernels by value
struct XbTable {
    float* p[XB_NP];
    long long off[XB_NP + 1];
};
static XbTable xb_table(const nbss_cfg& c, const XbGeom& g, float* const* ptrs) {
    XbTable t;
    for (int i = 0; i < XB_NP; ++i) {
        t.p[i] = ptrs[i];
        t.off[i] = param_off(c, 0, i) - g.lo;
    }
    t.off[XB_NP] = g.hi - g.lo;
    return t;
}
NBSS_DEV int xb_slot(const XbTable& t, long long r) {
    int s = 0;
    while (s + 1 < XB_NP && r >= t.off[s + 1]) ++s;
    return s;
}
// flat[i] = the tensor that owns slot i, 0 outside [lo, hi)
__global__ __launch_bounds__(256) void xb_gather_kernel(XbTable t, float* __restrict__ flat, long long total, long long lo, long long hi) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float v = 0.f;
        if (i >= lo && i < hi) {
            const int s = xb_slot(t, i - lo);
            v = t.p[s][i - lo - t.off[s]];
        }
        flat[i] = v;
    }
}
// the 18 slices of the flat gradient buffer -> the caller's buffers (written, not accumulated)
__global__ __launch_bounds__(256) void xb_scatter_kernel(XbTable t, const float* __restrict__ flat, long long lo, long long hi) {
    for (long long i = lo + (long long)blockIdx.x * 256 + threadIdx.x; i < hi; i += (long long)gridDim.x * 256) {
        const int s = xb_slot(t, i - lo);
        t.p[s][i - lo - t.off[s]] = flat[i];
    }
}
static int xb_grid(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

// NBSS_OK, or why the shape is refused (check_cfg: dtype, B, F <= 272, T <= 4096, the 32-bit token offsets)
static int xb_check(const nbss_cfg& c, bool train) {
    const int e = check_cfg(c);
    if (e) return e;
    return train && !xb_trainable(c) ? NBSS_EUNSUPPORTED : NBSS_OK;
}

// flat parameters and packed fragments into ws
static int xb_prepare(const nbss_cfg& c, const XbGeom& g, const float* const* params, char* ws, hipStream_t st) {
    float* P = (float*)(ws + g.w_p);
    const XbTable t = xb_table(c, g, (float* const*)params);
    NBSS_LAUNCH(xb_gather_kernel, dim3(xb_grid(g.total)), dim3(256), 0, st, t, P, g.total, g.lo, g.hi);
    const int e = NBSS_CHECK_LAUNCH();
    return e ? e : pack_params_impl(c, P, ws + g.w_pk, st);
}

static bool xb_all(const float* const* p) {
    for (int i = 0; i < XB_NP; ++i)
        if (!p[i]) return false;
    return true;
}

extern "C" {

int64_t nbss_online_xband_save_bytes(int dtype, int B, int F, int T) {
    const nbss_cfg c = xb_cfg(dtype, B, F, T);
    const int e = xb_check(c, true);
    return e ? e : (int64_t)xb_geom(c).save_total;
}
int64_t nbss_online_xband_ws_bytes(int dtype, int B, int F, int T) {
    const nbss_cfg c = xb_cfg(dtype, B, F, T);
    const int e = xb_check(c, false);
    return e ? e : (int64_t)xb_geom(c).ws_total;
}

int nbss_online_xband_train_fwd(int dtype, int B, int F, int T, const float* fc1_ln_w, const float* fc1_ln_b, const float* fc1_w, const float* fc1_b,
                                const float* fc1_prelu, const float* full_ln_w, const float* full_ln_b, const float* sq_w, const float* sq_b,
                                const float* full_w, const float* full_b, const float* usq_w, const float* usq_b, const float* fc2_ln_w,
                                const float* fc2_ln_b, const float* fc2_w, const float* fc2_b, const float* fc2_prelu, const void* x, void* y, void* save,
                                void* ws, void* stream) {
    const nbss_cfg c = xb_cfg(dtype, B, F, T);
    int e = xb_check(c, save != nullptr);
    if (e) return e;
    const float* params[XB_NP] = {fc1_ln_w, fc1_ln_b, fc1_w, fc1_b, fc1_prelu, full_ln_w, full_ln_b, sq_w, sq_b,
                                  full_w, full_b, usq_w, usq_b, fc2_ln_w, fc2_ln_b, fc2_w, fc2_b, fc2_prelu};
    if (!xb_all(params) || !x || !y || !ws || x == y) return NBSS_EINVAL;
    const XbGeom g = xb_geom(c);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    if ((e = xb_prepare(c, g, params, w, st))) return e;
    const float* P = (const float*)(w + g.w_p);
    const void* pk = w + g.w_pk;
    void* x1 = save ? save : (void*)(w + g.w_t0);
    void* x2 = save ? (void*)((char*)save + g.sb) : (void*)(w + g.w_t1);
    if ((e = fconv_fwd_impl(c, P, pk, 0, 0, x, x1, st))) return e;
    if ((e = full_fwd_impl(c, P, pk, 0, x1, x2, st))) return e;
    return fconv_fwd_impl(c, P, pk, 0, 1, x2, y, st);
}

int nbss_online_xband_train_bwd(int dtype, int B, int F, int T, const float* fc1_ln_w, const float* fc1_ln_b, const float* fc1_w, const float* fc1_b,
                                const float* fc1_prelu, const float* full_ln_w, const float* full_ln_b, const float* sq_w, const float* sq_b,
                                const float* full_w, const float* full_b, const float* usq_w, const float* usq_b, const float* fc2_ln_w,
                                const float* fc2_ln_b, const float* fc2_w, const float* fc2_b, const float* fc2_prelu, const void* x, const void* save,
                                const void* dy, void* dx, float* d_fc1_ln_w, float* d_fc1_ln_b, float* d_fc1_w, float* d_fc1_b, float* d_fc1_prelu,
                                float* d_full_ln_w, float* d_full_ln_b, float* d_sq_w, float* d_sq_b, float* d_full_w, float* d_full_b, float* d_usq_w,
                                float* d_usq_b, float* d_fc2_ln_w, float* d_fc2_ln_b, float* d_fc2_w, float* d_fc2_b, float* d_fc2_prelu, void* ws,
                                void* stream) {
    const nbss_cfg c = xb_cfg(dtype, B, F, T);
    int e = xb_check(c, true);
    if (e) return e;
    const float* params[XB_NP] = {fc1_ln_w, fc1_ln_b, fc1_w, fc1_b, fc1_prelu, full_ln_w, full_ln_b, sq_w, sq_b,
                                  full_w, full_b, usq_w, usq_b, fc2_ln_w, fc2_ln_b, fc2_w, fc2_b, fc2_prelu};
    float* grads[XB_NP] = {d_fc1_ln_w, d_fc1_ln_b, d_fc1_w, d_fc1_b, d_fc1_prelu, d_full_ln_w, d_full_ln_b, d_sq_w, d_sq_b,
                           d_full_w, d_full_b, d_usq_w, d_usq_b, d_fc2_ln_w, d_fc2_ln_b, d_fc2_w, d_fc2_b, d_fc2_prelu};
    if (!xb_all(params) || !xb_all(grads) || !x || !save || !dy || !dx || !ws || dx == dy) return NBSS_EINVAL;
    const XbGeom g = xb_geom(c);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    if ((e = xb_prepare(c, g, params, w, st))) return e;
    const float* P = (const float*)(w + g.w_p);
    const void* pk = w + g.w_pk;
    float* G = (float*)(w + g.w_g);
    if ((e = memset_async_impl(G, (size_t)g.total * sizeof(float), st))) return e;
    const void *x1 = save, *x2 = (const char*)save + g.sb;
    void *g2 = w + g.w_t0, *g1 = w + g.w_t1, *bws = w + g.w_ws;
    if ((e = fconv_bwd_impl(c, P, G, pk, 0, 1, x2, dy, g2, bws, st, nullptr))) return e;
    if ((e = full_bwd_impl(c, P, G, pk, 0, x1, g2, g1, bws, st, nullptr))) return e;
    if ((e = fconv_bwd_impl(c, P, G, pk, 0, 0, x, g1, dx, bws, st, nullptr))) return e;
    const XbTable t = xb_table(c, g, grads);
    NBSS_LAUNCH(xb_scatter_kernel, dim3(xb_grid(g.hi - g.lo)), dim3(256), 0, st, t, (const float*)G, g.lo, g.hi);
    return NBSS_CHECK_LAUNCH();
}

}  // extern "C"
