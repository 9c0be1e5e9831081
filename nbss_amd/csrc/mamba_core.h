// mamba_core.h — one channel of the selective scan of a Mamba block at width 96 (E = 192 channels, N = 16 states, K = 4 taps, dt rank 6): its parameters,
// the causal convolution, dt and one frame of the recurrence.  Shared by the training kernels (online_mamba_train.hip) and the streaming step
// (online_mamba_step.hip): both compute the same forward, in the same order of operations.
#pragma once
#include "common.h"

#define MB_E 192
#define MB_N 16
#define MB_K 4
#define MB_R 6
#define MB_J (MB_R + 2 * MB_N)  // 38: the x_proj outputs of a frame (dt_r, B, C)
#define MB_JL 40                // their row in LDS

// torch.nn.functional.softplus (threshold 20)
NBSS_DEV float mb_softplus(float p) { return p > 20.f ? p : log1pf(expf(p)); }

// the channel's parameters
struct MbChan {
    float cw[MB_K], cb, wdt[MB_R], bdt, A[MB_N], dp;
};
// conv_w [192][4], conv_b [192], dt_w [192][6], dt_b [192], A_log [192][16], D [192]
NBSS_DEV void mb_chan(MbChan& c, const float* __restrict__ cw, const float* __restrict__ cb, const float* __restrict__ wdt, const float* __restrict__ bdt,
                      const float* __restrict__ alog, const float* __restrict__ dp, int e) {
#pragma unroll
    for (int k = 0; k < MB_K; ++k) c.cw[k] = cw[e * MB_K + k];
#pragma unroll
    for (int r = 0; r < MB_R; ++r) c.wdt[r] = wdt[e * MB_R + r];
#pragma unroll
    for (int n = 0; n < MB_N; ++n) c.A[n] = -expf(alog[e * MB_N + n]);
    c.cb = cb[e];
    c.bdt = bdt[e];
    c.dp = dp[e];
}
// the convolution's output of a frame after its SiLU: xr is the frame's input, xm1 .. xm3 those of the one, two and three frames before
NBSS_DEV float mb_conv(const MbChan& c, float xm3, float xm2, float xm1, float xr) {
    return silu_f(c.cb + c.cw[0] * xm3 + c.cw[1] * xm2 + c.cw[2] * xm1 + c.cw[3] * xr);
}
// dt of the channel at a frame from the frame's x_proj row; `pre` gets the value before the softplus
NBSS_DEV float mb_dt(const MbChan& c, const float* row, float& pre) {
    float p = c.bdt;
#pragma unroll
    for (int r = 0; r < MB_R; ++r) p += c.wdt[r] * row[r];
    pre = p;
    return mb_softplus(p);
}
// one frame: h <- exp(dt A) h + dt xc B, returns sum_n C[n] h[n] + D xc (row: the frame's 38 x_proj outputs, xc: the channel's convolution output)
NBSS_DEV float mb_scan_frame(const MbChan& c, float (&h)[MB_N], const float* row, float xc) {
    float pre;
    const float dt = mb_dt(c, row, pre), dtx = dt * xc;
    float ys = c.dp * xc;
#pragma unroll
    for (int k = 0; k < MB_N; ++k) {
        h[k] = expf(dt * c.A[k]) * h[k] + dtx * row[MB_R + k];
        ys += row[MB_R + MB_N + k] * h[k];
    }
    return ys;
}
