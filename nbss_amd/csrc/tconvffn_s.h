// tconvffn_s.h — what the block's wrappers (tconvffn.hip) use of the bf16-stream T-ConvFFN kernels (tconvffn_s.hip)
#pragma once
#include "launch.h"
#include "layout.h"
#include "side.h"

// What a training-mode forward keeps for the backward pass (tconvffn_bwd_q_kernel): the pre-activations a1 (W1 output), a2, a3
// (conv1 / conv2 outputs; a3 = GroupNorm input) as group-major [G][N][24] bf16 tensors — what the reference's autocast graph holds as
// bf16 conv outputs —, the LayerNorm (mean, rstd) of every token and the GroupNorm (mean, rstd) of every (sequence, group).  With them
// the backward pass evaluates each SiLU / SiLU' pair from ONE sigmoid and recomputes one convolution only: a5 = conv3(h4), whose input
// it has in LDS anyway (saving a5 as well cost 2 S.B of stores here and 2 S.B of loads there for 5 MFMAs per strip).
struct TsSave {
    bf16_t *a1, *a2, *a3;
    float *ln, *gn;  // [N][2], [B*F][G][2]
};
// the caller's t_save block (tconvffn_save_bytes(c) bytes): a1 | a2 | a3 | LayerNorm stats | GroupNorm stats
TsSave ts_save_ptrs(const nbss_cfg& c, void* tsave);
// the same five tensors inside the backward workspace (layout.h: WS_TC_*), for a backward that was handed no t_save
TsSave ts_save_ws(const nbss_cfg& c, void* ws);

// sv != nullptr: training-mode forward (*sv is filled).  flip: launch.h
int tconvffn_fwd_s_impl(const nbss_cfg& c, const float* P, const void* packed, int layer, const void* x, void* y, const TsSave* sv, hipStream_t st, const SeqTail* tl,
                        int flip);
int tconvffn_bwd_q_launch(const nbss_cfg& c, const LayerPtrs& lp, float* part, const void* packed, int layer, const void* dy, const TsSave& sv, void* op_h5, void* op_da1,
                          hipStream_t st);
int tconvffn_v_reduce16(const nbss_cfg& c, const void* part16, float* slices, float* G, const long long* offs, hipStream_t st);
