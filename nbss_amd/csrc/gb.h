// gb.h — internal interface of the geometry-generic pieces: what gbwd.hip (the SpatialNet-large sequencing) and nb_blocks.hip (the nbss_nb_*
// building blocks) are sequenced from.  One tensor pass each, every intermediate in the caller's workspace:
//   gb_gemm.hip   weight re-lay + tap_gemm: every per-token linear map, the grouped convolutions along F and along T, the LinearGroup and their data gradients
//   gb_rows.hip   LayerNorm / GroupNorm / GroupBatchNorm forward and backward, SiLU / PReLU backward, the full-band transposes, the decoder's column padding
//   gb_attn.hip   whole-head attention (head widths 24 and 48): forward alone, and forward + backward in two kernels per (sequence, head); the device
//                 helpers of its kernels (LDS images, fragments, softmax steps) are attn_tiles.h's, shared with the other attention sources
// Every launcher is a template on the stream type (float, bf16_t), takes untyped tensor pointers, the stream last, and returns an NBSS_* code; the file
// that defines it instantiates it for both types.
#pragma once
#include "launch.h"
#include "layout.h"
#include "tapgemm.h"

#define GB_THREADS 256
#define GA_TMAX 256  // frames per sequence of the whole-head attention kernels (gb_attn.hip, attn_relpos.hip)

// ---- workspace ---------------------------------------------------------------------------------------------------------------------------------
inline int gb_blocks(long n, int per_block) {
    const long b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}
inline int pad16(int v) { return (v + 15) & ~15; }
inline int pad32(int v) { return (v + 31) & ~31; }
inline int pad8(int v) { return (v + 7) & ~7; }
// bump allocator over the sub-block's workspace (behind the per-token statistics at its head; 256-byte aligned pieces)
struct GbArena {
    char* p;
    char* end;
    void* take(size_t bytes) {
        void* r = p;
        p += ws_align(bytes);
        return p <= end ? r : nullptr;
    }
};
inline GbArena gb_arena(const nbss_cfg& c, void* ws) {
    const size_t N = (size_t)c.B * c.F * c.T;
    GbArena a;
    a.p = (char*)ws + ws_align(N * 2 * sizeof(float));
    a.end = (char*)ws + ws_part_offset(c);
    return a;
}
// the workspace region of the per-workgroup affine rows (layout.h: ws_part_offset; B max(F, T) rows of 576 floats)
inline float* gb_part(const nbss_cfg& c, void* ws) { return (float*)((char*)ws + ws_part_offset(c)); }
inline size_t gb_part_floats(const nbss_cfg& c) { return (size_t)c.B * (c.F > c.T ? c.F : c.T) * 576; }

// ---- gb_gemm.hip ---------------------------------------------------------------------------------------------------------------------------------
// weights for tap_gemm: [groups][taps][Mp][Kp] of the stream dtype, zero padded (Mp % 16 == 0, Kp % 32 == 0)
enum { WP_LIN_FWD, WP_LIN_DGRAD, WP_CONV_FWD, WP_CONV_DGRAD, WP_LG_FWD, WP_LG_DGRAD };
struct WPrep {
    const float* src;
    void* dst;
    int mode, groups, taps, Mg, Kv, Mp, Kp;  // Mg x Kv valid per (group, tap)
};
// several re-lays in one launch (blockIdx.y = descriptor): a block backward re-laid its 3 - 6 weights with one 5-us launch each, 1 060 per large step
#define GB_WPREP_MAX 6
struct WPrepMulti {
    WPrep d[GB_WPREP_MAX];
};
template <class T>
int gb_wprep(const float* src, void* dst, int mode, int groups, int taps, int Mg, int Kv, int Mp, int Kp, hipStream_t st);
template <class T>
struct WPrepBatch {
    WPrepMulti m;
    int n = 0;
    long most = 0;
    void add(const float* src, void* dst, int mode, int groups, int taps, int Mg, int Kv, int Mp, int Kp) {
        m.d[n++] = {src, dst, mode, groups, taps, Mg, Kv, Mp, Kp};
        const long el = (long)groups * taps * Mp * Kp;
        most = el > most ? el : most;
    }
    int launch(hipStream_t st);
};
template <class T>
int gb_gemm(const TapGemm& p, hipStream_t st);
// dense per-token linear map (taps = 1, one group): Y[rows][M] = act(X[rows][K] Wp^T + bias) (+ R)
inline TapGemm gb_lin(const void* X, int ldx, const void* Wp, const float* bias, void* Y, int ldy, long rows, int M, int K) {
    TapGemm p;
    p.X = X; p.W = Wp; p.bias = bias; p.R = nullptr; p.Y = Y;
    p.rows = (int)rows;
    p.ldx = ldx; p.xcol = 0; p.xgs = 0;
    p.ldy = ldy; p.ycol = 0; p.ygs = 0; p.ldr = 0;
    p.groups = 1; p.Mg = M; p.Kg = K; p.Mp = pad16(M); p.Kp = pad32(K); p.bgs = 0;
    p.taps = 1; p.center = 0; p.shift = 0; p.pos_div = 1; p.pos_len = 1 << 30;
    p.xact = 0; p.yact = 0; p.Y2 = nullptr; p.Dact = nullptr;
    return p;
}
// grouped convolution along one axis of the [B][F][T] token grid on [rows][C] tensors (C = groups * CG in and out)
inline TapGemm gb_conv(const void* X, const void* Wp, const float* bias, void* Y, long rows, int C, int groups, int taps, int shift, int pos_div,
                       int pos_len) {
    const int CG = C / groups;
    TapGemm p = gb_lin(X, C, Wp, bias, Y, C, rows, CG, CG);
    p.groups = groups; p.xgs = CG; p.ygs = CG; p.bgs = CG;
    p.taps = taps; p.center = taps / 2; p.shift = shift; p.pos_div = pos_div; p.pos_len = pos_len;
    return p;
}

// ---- gb_rows.hip ---------------------------------------------------------------------------------------------------------------------------------
// LayerNorm over the last dim (eps 1e-5): u = xhat gamma + beta (u may be null: statistics only), stats [N][2] = (mean, rstd)
template <class T>
int gb_ln_fwd(const void* x, const float* gamma, const float* beta, void* u, float* stats, long N, int C, hipStream_t st);
// dx = dy + LN'(du); dgamma / dbeta accumulate (through `part`, per-workgroup rows folded in a fixed order, where it is given and large enough)
template <class T>
int gb_ln_bwd(const void* du, const void* x, const float* stats, const float* gamma, const void* dy, void* dx, float* dgamma, float* dbeta, long N, int C,
              hipStream_t st, float* part = nullptr, size_t part_floats = 0);
template <class T>
int gb_silu_bwd(const void* a, const void* gin, void* gout, long n, hipStream_t st);
// PReLU of a residual block, y = x + PReLU(a): da = dy (a > 0 ? 1 : alpha[c]), dalpha[c] += sum dy min(a, 0); a, dy, da [N][C]
template <class T>
int gb_prelu_bwd(const void* a, const void* dy, const float* alpha, void* da, float* dalpha, long N, int C, hipStream_t st);
// [N = (b, f, t)][SQ] -> [(b, t)][SQ][FK] (columns F..FK zero) and back
template <class T>
int gb_sq_to_f(const void* src, void* dst, int B, int F, int Tn, int SQ, int FK, hipStream_t st);
template <class T>
int gb_f_to_sq(const void* src, void* dst, int B, int F, int Tn, int SQ, int FK, hipStream_t st);
// fp32 [N][Co] -> stream dtype [N][CP] (zero padded)
template <class T>
int gb_pad_cols(const float* src, void* dst, long N, int Co, int CP, hipStream_t st);
// GroupNorm over (T x CG) per (sequence, group), optional SiLU; nsg = sequences x groups; stats [nsg][2] (forward: may be null); backward in place in dh
template <class T>
int gb_gn_fwd(const void* a, const float* gamma, const float* beta, void* h, float* stats, long nsg, int Tn, int C, int CG, int act, hipStream_t st);
template <class T>
int gb_gn_bwd(const void* a, const float* stats, const float* gamma, const float* beta, void* dh, float* dgamma, float* dbeta, long nsg, int Tn, int C, int CG,
              hipStream_t st);
// GroupBatchNorm over (F x C) per (b, t), optional SiLU: x, y [B][F][T][C]
template <class T>
int gb_gbn_fwd(const void* x, const float* gamma, const float* beta, void* y, int B, int F, int Tn, int C, float eps, int act, hipStream_t st);
template <class T>
int gb_gbn_bwd(const void* x, const float* gamma, const float* beta, const void* dy, void* dx, float* dgamma, float* dbeta, int B, int F, int Tn, int C, float eps,
               int act, hipStream_t st);

// ---- gb_attn.hip ---------------------------------------------------------------------------------------------------------------------------------
// forward (O, lse, D) + backward (dqkv) of scaled-dot-product attention, c.B c.F sequences of c.T frames; DH = c.H / c.heads in {24, 48}
template <class T, int DH>
int gb_attn_launch(const nbss_cfg& c, const void* qkv, const void* dO, void* O, void* dqkv, float* lse, float* Dv, hipStream_t st);
// the forward alone
template <class T, int DH>
int nb_attn_fwd(long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st);
