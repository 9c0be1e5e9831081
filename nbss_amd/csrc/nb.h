// nb.h — the implementations behind the narrow-band building blocks of the C ABI (capi.hip: nbss_nb_*; include/nbss_hip.h documents the arguments).
// Defined in nb_blocks.hip, but for nb_attention_relpos_* / nb_relpos_bwd_ws_bytes_impl (attn_relpos.hip), nb_attention_kb_* / nb_attention_long_fwd_impl
// (attn_kb.hip) and nb_attention_relpos_long_fwd_impl (attn_relpos_kb.hip).
#pragma once
#include "launch.h"

size_t nb_ws_bytes_impl(int M, int K, int groups, int taps);
int nb_conv_t_impl(int dtype, long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const float* bias, void* y,
                   const void* residual, int act_in, int act_out, void* ws, hipStream_t st);
int nb_layernorm_impl(int dtype, long rows, int C, const void* x, const float* gamma, const float* beta, void* y, float* stats, hipStream_t st);
int nb_gbn_impl(int dtype, int B, int F, int Tn, int C, const void* x, const float* gamma, const float* beta, float eps, int act, void* y, hipStream_t st);
int nb_attention_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st);
int nb_attention_relpos_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* pos, const float* ub, const float* vb, float scale, void* o,
                                 hipStream_t st, const uint32_t* mask, float keep);
size_t nb_relpos_bwd_ws_bytes_impl(long nseq, int Tn, int H, int heads);
int nb_attention_relpos_bwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* pos, const float* ub, const float* vb, float scale,
                                 const uint32_t* mask, float keep, const void* dO, void* dqkv, float* dpos, float* du, float* dvb, void* ws, hipStream_t st);
int nb_group_norm_train_impl(int dtype, long nseq, int Tn, int C, int groups, const void* x, const float* gamma, const float* beta, int act, void* y, float* stats,
                             hipStream_t st);
int nb_group_norm_bwd_impl(int dtype, long nseq, int Tn, int C, int groups, const void* x, const float* stats, const float* gamma, const float* beta, void* dy_dx,
                           float* dgamma, float* dbeta, hipStream_t st);
int nb_group_norm_impl(int dtype, long nseq, int Tn, int C, int groups, const void* x, const float* gamma, const float* beta, int act, void* y, hipStream_t st);
size_t nb_bwd_ws_bytes_impl(int M, int K, int groups, int taps);
int nb_conv_t_train_impl(int dtype, long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const float* bias, void* y,
                         void* y2, const void* residual, void* ws, hipStream_t st);
int nb_conv_t_bwd_impl(int dtype, long nseq, int Tn, int Cin, int ldx, int Cout, int groups, int taps, const void* x, const float* w, const void* dy, const void* dact,
                       void* dx, float* dw, float* dbias, void* ws, hipStream_t st);
int nb_layernorm_bwd_impl(int dtype, long rows, int C, const void* x, const float* stats, const float* gamma, const void* du, const void* dres, void* dx, float* dgamma,
                          float* dbeta, hipStream_t st);
int nb_gbn_bwd_impl(int dtype, int B, int F, int Tn, int C, const void* x, const float* gamma, const float* beta, float eps, int act, const void* dy, void* dx,
                    float* dgamma, float* dbeta, hipStream_t st);
size_t nb_attn_bwd_ws_bytes_impl(long N, int H, int heads, int dtype);
int nb_attention_bwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* dO, void* dqkv, void* ws, hipStream_t st);
// head width 96: the key-blocked kernels of attn_kb.hip (nb_attention_fwd_impl / nb_attention_bwd_impl dispatch here)
int nb_attention_kb_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st);
int nb_attention_kb_bwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* dO, void* O, void* dqkv, float* lse, float* Dv, hipStream_t st);
// forward on long sequences (T <= 4096: inference on whole utterances), key-blocked: attn_kb.hip (head widths 24 / 48 / 96), attn_relpos_kb.hip (24 / 48)
int nb_attention_long_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, void* o, hipStream_t st);
int nb_attention_relpos_long_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* pos, const float* ub, const float* vb, float scale,
                                      void* o, hipStream_t st);
