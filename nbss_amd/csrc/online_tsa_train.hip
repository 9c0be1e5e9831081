// online_tsa_train.hip — the whole retention block of an OnlineSpatialNet layer for TRAINING as one call (reference: models/arch/OnlineSpatialNet.py
// `SpatialNetLayer._tsa` with attention 'ret(2,*)' and the residual of `SpatialNetLayer.forward`), forward and backward:
//
//   u = LayerNorm(x)   q = Wq u   k = Wk u (absent: shared with q)   v = Wv u   g = Wg u
//   go = SiLU(g) * RMSNorm_head(chunk_retention(q, 24^-0.5 k, v))          the core of online_ret_train.hip, unchanged
//   y = x + Wo go
//
// x, y [BF][T][96] of the stream dtype (fp32 or bf16; fp32 accumulation and fp32 statistics in either), the seven parameters fp32 in the module's layout.
// Two kernels are new, the rest is sequencing of what the library has:
//   tsa_proj_fwd  a workgroup of four waves owns 128 rows of x.  Each wave normalises two 16-row strips in registers (blocks.h: ln_strip) — u exists only as
//                 the B fragments of the products — and multiplies them by the stacked weight [Wq; Wk; Wv; Wg] ([576][96], [480][96] with shared keys) on the
//                 matrix cores.  The weight passes through LDS in slices of 96 output rows, each staged once per workgroup (the whole fp32 weight, 221 KB, is
//                 more than a CU's LDS).  x is read once; q, k, v, g are written as four contiguous tensors, (mean, rstd) per row beside them.
//   tsa_proj_bwd  the same tiling.  du = dq Wq + dk Wk + dv Wv + dg Wg is ONE accumulation over the 576 (480) inputs — the d* fragments come straight from
//                 memory, the transposed weight slices from LDS — then the LayerNorm backward of the row in registers (blocks.h: ln_bwd_row_raw) adds the
//                 residual gradient dy and writes dx.  d_ln_weight / d_ln_bias: per-lane sums over the workgroup's rows (xhat from the saved statistics),
//                 DPP row sums, the four waves added in order in LDS, one partial row per workgroup; util.hip's affine fold sums the rows in a fixed order.
//   sequencing    forward: tsa_proj_fwd -> nbss_online_ret_train_fwd -> nb_conv_t_impl (taps 1, residual = x);  backward: nb_conv_t_bwd_impl (d_go, d_wo) ->
//                 nbss_online_ret_train_bwd -> nb_layernorm_impl (u again, into the workspace) -> four weight gradients d^T u through nb_conv_t_bwd_impl
//                 (dx = NULL) -> tsa_proj_bwd -> the fold.  nb_conv_t_bwd_impl and the fold accumulate: the seven gradient buffers are ZEROED first, so the
//                 entry point's gradients are written.
// SAVED (what the forward keeps): q, k, v, g, the gated core output go, the row statistics and the core's chunk states.  go is kept, not recomputed: it is
// the operand of d_wo, and the core's backward rebuilds o per chunk in registers only — a second core forward would cost more than 192 elements per token.
// Per token: fp32 (576 + 192) 4 + 8 + 288 = 3 368 bytes, bf16 1 832 (shared keys: 384 / 192 less; 288 = the [4][24][48] fp32 states of a 64-frame chunk).
// RECOMPUTED: u (for the weight gradients), everything inside the core.
// No atomics, every sum in a fixed order: two calls give the same bits.  A row of q, k, v, g, y or dx depends on its own row of x (dy) and, through the core,
// on its own sequence only; no grid is capped (one workgroup per 128 rows).
#include "gb.h"
#include "blocks.h"
#include "nb.h"

#define TS_H 96
#define TS_V 192
#define TS_THREADS 256
#define TS_STRIPS 2                    // 16-row strips per wave
#define TS_ROWS (4 * TS_STRIPS * 16)   // rows of x per workgroup
#define TS_CH 96                       // rows (forward) / columns (backward) of the stacked weight per LDS slice
#define TS_KSCALE 0.20412414523193154f  // 24^-0.5: MultiScaleRetention.scaling at 4 heads of key width 24
template <class T> struct TsLd { static constexpr int v = TS_CH + (sizeof(T) == 2 ? 8 : 4); };  // row length of the slice image: 16-byte rows, odd in 16-byte units

struct TsProj {
    const float* w[4];  // wq, wk (null: shared keys), wv, wg: [96 | 96 | 192 | 192][96]
    void* o[4];         // forward: q, k, v, g (written); backward: dq, dk, dv, dg (read)
    const float *ln_w, *ln_b;
    const void *x, *dy;
    void* dx;
    float* stats;  // [N][2]: written by the forward, read by the backward
    float *part_w, *part_b;  // backward: [workgroups][96] each
    long N;
};

// slice c of the stacked weight: the tensor it belongs to (0 q, 1 k, 2 v, 3 g) and its first row there
NBSS_DEV void ts_slice(bool has_k, int c, int& seg, int& r0) {
    const int cc = has_k || c == 0 ? c : c + 1;
    seg = cc < 2 ? cc : 2 + ((cc - 2) >> 1);
    r0 = cc < 2 ? 0 : TS_CH * ((cc - 2) & 1);
}
NBSS_DEV void ts_rows(const TsProj& a, long (&row)[TS_STRIPS], bool (&ok)[TS_STRIPS]) {
    const int w = wave_id_u(), l15 = lane_id() & 15;
#pragma unroll
    for (int s = 0; s < TS_STRIPS; ++s) {
        row[s] = (long)blockIdx.x * TS_ROWS + (w * TS_STRIPS + s) * 16 + l15;
        ok[s] = row[s] < a.N;
    }
}

template <class T>
__global__ __launch_bounds__(TS_THREADS) void tsa_proj_fwd_kernel(TsProj a) {
    NBSS_LDS(smem);
    T* img = reinterpret_cast<T*>(smem);  // [96 output rows][LD]
    constexpr int LD = TsLd<T>::v;
    const int tid = threadIdx.x, lane = lane_id(), l15 = lane & 15, g4 = lane >> 4;
    const bool has_k = a.w[1] != nullptr;
    const int nsl = has_k ? 6 : 5;
    long row[TS_STRIPS];
    bool ok[TS_STRIPS];
    ts_rows(a, row, ok);
    Frag<T> u[TS_STRIPS][BK_KS];
    {
        float gam[BK_KS][8], bet[BK_KS][8];
        load_ln_affine(a.ln_w, a.ln_b, gam, bet);
#pragma unroll
        for (int s = 0; s < TS_STRIPS; ++s) ln_strip<T>((const T*)a.x + row[s] * TS_H, ok[s], gam, bet, u[s], a.stats + row[s] * 2);
    }
    for (int c = 0; c < nsl; ++c) {
        int seg, r0;
        ts_slice(has_k, c, seg, r0);
        const int wd = seg < 2 ? TS_H : TS_V;
        const float* W = a.w[seg] + (size_t)r0 * TS_H;
        __syncthreads();  // the previous slice is consumed
        for (int e = tid; e < TS_CH * (TS_H / 4); e += TS_THREADS) {
            const int r = e / (TS_H / 4), c4 = (e % (TS_H / 4)) * 4;
            float v[4];
            load4(W + r * TS_H + c4, v);
            store4(img + r * LD + c4, v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        T* out = (T*)a.o[seg];
        for (int mt = 0; mt < TS_CH / 16; ++mt) {
            Frag<T> fa[BK_KS];
#pragma unroll
            for (int ks = 0; ks < BK_KS; ++ks) frag_load(fa[ks], img + (16 * mt + l15) * LD + 32 * ks + 8 * g4);
#pragma unroll
            for (int s = 0; s < TS_STRIPS; ++s) {
                f32x4 acc = F32X4_ZERO;
#pragma unroll
                for (int ks = 0; ks < BK_KS; ++ks) acc = mma(fa[ks], u[s][ks], acc);
                if (ok[s]) store4(out + row[s] * wd + r0 + 16 * mt + 4 * g4, acc[0], acc[1], acc[2], acc[3]);
            }
        }
    }
}

template <class T>
__global__ __launch_bounds__(TS_THREADS) void tsa_proj_bwd_kernel(TsProj a) {
    NBSS_LDS(smem);
    T* img = reinterpret_cast<T*>(smem);  // [96 input channels][LD]: the slice transposed
    constexpr int LD = TsLd<T>::v;
    const int tid = threadIdx.x, lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id_u();
    const bool has_k = a.w[1] != nullptr;
    const int nsl = has_k ? 6 : 5;
    long row[TS_STRIPS];
    bool ok[TS_STRIPS];
    ts_rows(a, row, ok);
    f32x4 du[TS_STRIPS][BK_MT];
#pragma unroll
    for (int s = 0; s < TS_STRIPS; ++s)
#pragma unroll
        for (int mt = 0; mt < BK_MT; ++mt) du[s][mt] = F32X4_ZERO;
    for (int c = 0; c < nsl; ++c) {
        int seg, r0;
        ts_slice(has_k, c, seg, r0);
        const int wd = seg < 2 ? TS_H : TS_V;
        const float* W = a.w[seg] + (size_t)r0 * TS_H;
        __syncthreads();
        for (int e = tid; e < TS_CH * (TS_H / 4); e += TS_THREADS) {
            const int o = e / (TS_H / 4), i4 = (e % (TS_H / 4)) * 4;
            float v[4];
            load4(W + o * TS_H + i4, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) store1(img + (i4 + j) * LD + o, v[j]);
        }
        __syncthreads();
        const T* d = (const T*)a.o[seg];
#pragma unroll
        for (int ks = 0; ks < BK_KS; ++ks) {
            Frag<T> fb[TS_STRIPS], fa;
#pragma unroll
            for (int s = 0; s < TS_STRIPS; ++s) {
                if (ok[s]) frag_load(fb[s], d + row[s] * wd + r0 + 32 * ks + 8 * g4);
                else frag_zero(fb[s]);
            }
#pragma unroll
            for (int mt = 0; mt < BK_MT; ++mt) {
                frag_load(fa, img + (16 * mt + l15) * LD + 32 * ks + 8 * g4);
#pragma unroll
                for (int s = 0; s < TS_STRIPS; ++s) du[s][mt] = mma(fa, fb[s], du[s][mt]);
            }
        }
    }
    float dlw[BK_MT][4], dlb[BK_MT][4];
#pragma unroll
    for (int mt = 0; mt < BK_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dlw[mt][r] = dlb[mt][r] = 0.f;
#pragma unroll
    for (int s = 0; s < TS_STRIPS; ++s) {
        const long rc = ok[s] ? row[s] : 0;  // always readable; validity is applied on use
        RawC4<T> xr[BK_MT], dr[BK_MT];
        rawc_load_row(xr, (const T*)a.x + rc * TS_H);
        rawc_load_row(dr, (const T*)a.dy + rc * TS_H);
        const float mean = a.stats[rc * 2], rstd = a.stats[rc * 2 + 1];
#pragma unroll
        for (int mt = 0; mt < BK_MT; ++mt) {
            float xv[4];
            rawc_get(xr[mt], xv);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dv = keep_if(ok[s], du[s][mt][r]);
                dlw[mt][r] += dv * ((xv[r] - mean) * rstd);
                dlb[mt][r] += dv;
            }
        }
        ln_bwd_row_raw<false>(du[s], xr, dr, (T*)a.dx + row[s] * TS_H, nullptr, ok[s], a.ln_w);
    }
    // the workgroup's partial row: 16 rows of a lane group by DPP, the strips in the lane, the four waves in order
    float* red = reinterpret_cast<float*>(smem);  // [4][2][96]
    __syncthreads();  // the last slice is consumed
#pragma unroll
    for (int mt = 0; mt < BK_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sw = row_sum16(dlw[mt][r]), sb = row_sum16(dlb[mt][r]);
            if (l15 == 0) {
                red[(w * 2 + 0) * TS_H + 16 * mt + 4 * g4 + r] = sw;
                red[(w * 2 + 1) * TS_H + 16 * mt + 4 * g4 + r] = sb;
            }
        }
    __syncthreads();
    if (tid < 2 * TS_H) {
#pragma clang fp reassociate(off)
        float s = red[tid];
        for (int k = 1; k < 4; ++k) s += red[k * 2 * TS_H + tid];
        float* dst = tid < TS_H ? a.part_w : a.part_b;
        dst[(size_t)blockIdx.x * TS_H + tid % TS_H] = s;
    }
}

// NBSS_OK, or why the shape is refused
static int ts_check(int dtype, int64_t BF, int T) {
    if ((dtype != NBSS_F32 && dtype != NBSS_BF16) || BF < 1) return NBSS_EINVAL;
    if (T < 1 || T > NBSS_T_MAX || BF * T > (1L << 28)) return NBSS_EUNSUPPORTED;
    return NBSS_OK;
}

// save = [q | k (shared keys: absent) | v | g | go | (mean, rstd) | the core's chunk states]
// ws   = [the workspace of the nb_conv_t calls | the core's | scratch]; scratch: a forward without `save` keeps the first six pieces of `save` there; the
//        backward [d_go, later u: N x 192 | dq | dk | dv | dg | statistics of the second LayerNorm pass | the partial rows of d_ln_weight | of d_ln_bias]
struct TsGeom {
    long N;
    int nwg;
    size_t s_q, s_k, s_v, s_g, s_go, s_stat, s_state, save_total;
    size_t w_core, w_scr, b_a, b_dq, b_dk, b_dv, b_dg, b_stat, b_pw, b_pb, ws_total;
};
static TsGeom ts_geom(int dtype, int64_t BF, int T, bool has_k) {
    TsGeom g;
    const size_t esz = dtype == NBSS_BF16 ? 2 : 4;
    g.N = (long)BF * T;
    g.nwg = (int)((g.N + TS_ROWS - 1) / TS_ROWS);
    const size_t n96 = ws_align((size_t)g.N * TS_H * esz), n192 = ws_align((size_t)g.N * TS_V * esz), nst = ws_align((size_t)g.N * 2 * sizeof(float));
    size_t o = 0;
    g.s_q = o; o += n96;
    g.s_k = o; o += has_k ? n96 : 0;
    g.s_v = o; o += n192;
    g.s_g = o; o += n192;
    g.s_go = o; o += n192;
    g.s_stat = o; o += nst;
    g.s_state = o;
    const size_t fwd_scr = o;
    g.save_total = o + (size_t)nbss_online_ret_train_save_bytes(dtype, BF, T);
    size_t cw = nb_ws_bytes_impl(TS_H, TS_V, 1, 1);
    const size_t c1 = nb_bwd_ws_bytes_impl(TS_H, TS_V, 1, 1), c2 = nb_bwd_ws_bytes_impl(TS_V, TS_H, 1, 1), c3 = nb_bwd_ws_bytes_impl(TS_H, TS_H, 1, 1);
    cw = cw > c1 ? cw : c1;
    cw = cw > c2 ? cw : c2;
    cw = cw > c3 ? cw : c3;
    g.w_core = ws_align(cw);
    g.w_scr = g.w_core + (size_t)nbss_online_ret_train_ws_bytes(dtype, BF, T);
    o = 0;
    g.b_a = o; o += n192;
    g.b_dq = o; o += n96;
    g.b_dk = o; o += has_k ? n96 : 0;
    g.b_dv = o; o += n192;
    g.b_dg = o; o += n192;
    g.b_stat = o; o += nst;
    g.b_pw = o; o += ws_align((size_t)g.nwg * TS_H * sizeof(float));
    g.b_pb = o; o += ws_align((size_t)g.nwg * TS_H * sizeof(float));
    g.ws_total = g.w_scr + (o > fwd_scr ? o : fwd_scr);
    return g;
}

template <class T>
static int ts_proj_fwd(const TsProj& a, int nwg, hipStream_t st) {
    NBSS_LAUNCH((tsa_proj_fwd_kernel<T>), dim3(nwg), dim3(TS_THREADS), (size_t)TS_CH * TsLd<T>::v * sizeof(T), st, a);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
static int ts_proj_bwd(const TsProj& a, int nwg, hipStream_t st) {
    NBSS_LAUNCH((tsa_proj_bwd_kernel<T>), dim3(nwg), dim3(TS_THREADS), (size_t)TS_CH * TsLd<T>::v * sizeof(T), st, a);
    return NBSS_CHECK_LAUNCH();
}

extern "C" {

int64_t nbss_online_tsa_save_bytes(int dtype, int64_t BF, int T, int share_qk) {
    const int e = ts_check(dtype, BF, T);
    return e ? e : (int64_t)ts_geom(dtype, BF, T, !share_qk).save_total;
}
int64_t nbss_online_tsa_ws_bytes(int dtype, int64_t BF, int T, int share_qk) {
    const int e = ts_check(dtype, BF, T);
    return e ? e : (int64_t)ts_geom(dtype, BF, T, !share_qk).ws_total;
}

int nbss_online_tsa_train_fwd(int dtype, int64_t BF, int T, const float* ln_w, const float* ln_b, const float* wq, const float* wk, const float* wv,
                              const float* wg, const float* wo, const float* decay, const void* x, void* y, void* save, void* ws, void* stream) {
    int e = ts_check(dtype, BF, T);
    if (e) return e;
    if (!ln_w || !ln_b || !wq || !wv || !wg || !wo || !decay || !x || !y || !ws || x == y) return NBSS_EINVAL;
    const TsGeom g = ts_geom(dtype, BF, T, wk != nullptr);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    char* S = save ? (char*)save : w + g.w_scr;
    void *q = S + g.s_q, *k = wk ? S + g.s_k : nullptr, *v = S + g.s_v, *gg = S + g.s_g, *go = S + g.s_go;
    TsProj a = {{wq, wk, wv, wg}, {q, k, v, gg}, ln_w, ln_b, x, nullptr, nullptr, (float*)(S + g.s_stat), nullptr, nullptr, g.N};
    if ((e = dtype == NBSS_BF16 ? ts_proj_fwd<bf16_t>(a, g.nwg, st) : ts_proj_fwd<float>(a, g.nwg, st))) return e;
    if ((e = nbss_online_ret_train_fwd(dtype, BF, T, q, k, v, gg, TS_KSCALE, decay, go, save ? S + g.s_state : nullptr, w + g.w_core, stream))) return e;
    return nb_conv_t_impl(dtype, (long)BF, T, TS_V, TS_V, TS_H, 1, 1, go, wo, nullptr, y, x, 0, 0, w, st);
}

int nbss_online_tsa_train_bwd(int dtype, int64_t BF, int T, const float* ln_w, const float* ln_b, const float* wq, const float* wk, const float* wv,
                              const float* wg, const float* wo, const float* decay, const void* x, const void* save, const void* dy, void* dx,
                              float* d_ln_w, float* d_ln_b, float* d_wq, float* d_wk, float* d_wv, float* d_wg, float* d_wo, void* ws, void* stream) {
    int e = ts_check(dtype, BF, T);
    if (e) return e;
    if (!ln_w || !ln_b || !wq || !wv || !wg || !wo || !decay || !x || !save || !dy || !dx || !d_ln_w || !d_ln_b || !d_wq || !d_wv || !d_wg || !d_wo || !ws ||
        (wk == nullptr) != (d_wk == nullptr) || dx == dy || dx == x)
        return NBSS_EINVAL;
    const TsGeom g = ts_geom(dtype, BF, T, wk != nullptr);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const char* S = (const char*)save;
    char* B = w + g.w_scr;
    const void *q = S + g.s_q, *k = wk ? S + g.s_k : nullptr, *v = S + g.s_v, *gg = S + g.s_g, *go = S + g.s_go;
    void *dgo = B + g.b_a, *u = B + g.b_a, *dq = B + g.b_dq, *dk = wk ? B + g.b_dk : nullptr, *dv = B + g.b_dv, *dg = B + g.b_dg;
    // the gradients are written: zero what the accumulating calls add to
    struct { float* p; size_t n; } z[7] = {{d_ln_w, TS_H}, {d_ln_b, TS_H}, {d_wq, TS_H * TS_H}, {d_wk, TS_H * TS_H}, {d_wv, TS_V * TS_H}, {d_wg, TS_V * TS_H},
                                           {d_wo, TS_H * TS_V}};
    for (int i = 0; i < 7; ++i)
        if (z[i].p && (e = memset_async_impl(z[i].p, z[i].n * sizeof(float), st))) return e;
    if ((e = nb_conv_t_bwd_impl(dtype, (long)BF, T, TS_V, TS_V, TS_H, 1, 1, go, wo, dy, nullptr, dgo, d_wo, nullptr, w, st))) return e;
    if ((e = nbss_online_ret_train_bwd(dtype, BF, T, q, k, v, gg, TS_KSCALE, decay, S + g.s_state, dgo, dq, dk, dv, dg, w + g.w_core, stream))) return e;
    if ((e = nb_layernorm_impl(dtype, g.N, TS_H, x, ln_w, ln_b, u, (float*)(B + g.b_stat), st))) return e;  // (d_go is consumed: u takes its place)
    const struct { const float* wt; const void* d; float* dw; int cout; } pr[4] = {{wq, dq, d_wq, TS_H}, {wk, dk, d_wk, TS_H}, {wv, dv, d_wv, TS_V}, {wg, dg, d_wg, TS_V}};
    for (int i = 0; i < 4; ++i)
        if (pr[i].wt && (e = nb_conv_t_bwd_impl(dtype, (long)BF, T, TS_H, TS_H, pr[i].cout, 1, 1, u, pr[i].wt, pr[i].d, nullptr, nullptr, pr[i].dw, nullptr, w, st)))
            return e;
    float *pw = (float*)(B + g.b_pw), *pb = (float*)(B + g.b_pb);
    TsProj a = {{wq, wk, wv, wg}, {dq, dk, dv, dg}, ln_w, ln_b, x, dy, dx, (float*)const_cast<char*>(S + g.s_stat), pw, pb, g.N};
    if ((e = dtype == NBSS_BF16 ? ts_proj_bwd<bf16_t>(a, g.nwg, st) : ts_proj_bwd<float>(a, g.nwg, st))) return e;
    AffSegs sg;
    sg.n = 1; sg.off[0] = 0; sg.cnt[0] = TS_H;
    if ((e = affine_reduce_launch(pw, g.nwg, sg, d_ln_w, st))) return e;
    return affine_reduce_launch(pb, g.nwg, sg, d_ln_b, st);
}

}  // extern "C"
