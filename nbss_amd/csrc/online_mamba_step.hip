// online_mamba_step.hip — native streaming step of one residual Mamba block of the OnlineSpatialNet ('mamba(16,4)' at width 96; models/arch/base/mamba.py:
// Mamba.step behind a LayerNorm, as models/arch/OnlineSpatialNet.py: _mamba walks it frame by frame):
//   x[bf, c, :] += out_proj( y_c * SiLU(z_c) ),   (xr_c, z_c) = in_proj(LayerNorm(x[bf, c, :])),   y = the selective scan of xr from the carried state
// for a CHUNK of C <= 32 frames per call, in place, fp32 throughout like the rest of the streaming step (online.hip).  The scan itself — convolution,
// softplus, recurrence — is the forward of the training kernels (mamba_core.h), started from the caller's state instead of zeros.
//
// One workgroup of 192 threads per (batch, frequency) sequence; thread e is inner channel e and keeps, across the chunk, its four conv taps with the
// three-frame window, its 16 A = -exp(A_log) and its 16 states h in registers.  Stages, a barrier between each:
//   1. LayerNorm of the C frames                                                     -> U  [C][96]
//   2. in_proj (96 -> 384: thread e computes xr[e] and z[e]), 8 frames per pass so that a weight column is read once per 8 frames   -> XC, Z [C][192]
//   3. causal depthwise conv (k = 4) + SiLU per thread, in place in XC; the new conv state = the last three xr (a copy)
//   4. x_proj: the 38 outputs (6 dt_r | 16 B | 16 C) of a frame are sums over the 192 channels of XC; one (output, run of 8 frames) per thread   -> DBC [C][40]
//      (in U's place: U is dead after stage 2)
//   5. per thread and frame: dt = softplus(dt_proj dt_r + b), h = exp(dt A) h + dt xc B, y = C h + D xc; y SiLU(z) in place in Z
//   6. out_proj (192 -> 96) + residual by threads 0 .. 95
// LDS: 480 C floats = 61 440 bytes at C = 32, below the 64 KiB a launch gets without raising the limit; two workgroups fit a CU.
// State is read once at the start and written once at the end of the kernel; no atomics, every sum in a fixed order that does not depend on BF: two
// calls give the same bits, and a sequence's rows do not depend on the other sequences of the call.
#include "launch.h"
#include "mamba_core.h"
#include "online.h"

static_assert(MB_E == ON_FFN && MB_JL <= ON_H, "the x_proj rows take the place of the LayerNorm output");
#define OM_FLOATS(C) ((size_t)(C) * (ON_H + 2 * MB_E))
static_assert(OM_FLOATS(ON_CMAX) * sizeof(float) <= 64 * 1024, "the LDS image of a full chunk fits the default dynamic limit");

// grid = B*F, block = 192.  win_t [96][384], xproj_t [192][38], wo_t [192][96]: TRANSPOSED projection weights ([in][out]: adjacent threads read adjacent
// addresses).  conv_state [B*F][3][192] (oldest first), ssm_state [B*F][16][192].
__global__ __launch_bounds__(MB_E) void online_mamba_kernel(int C, const float* __restrict__ lw, const float* __restrict__ lb, const float* __restrict__ win_t,
                                                           const float* __restrict__ cw, const float* __restrict__ cb, const float* __restrict__ xproj_t,
                                                           const float* __restrict__ wdt, const float* __restrict__ bdt, const float* __restrict__ alog,
                                                           const float* __restrict__ dp, const float* __restrict__ wo_t, float* __restrict__ conv_state,
                                                           float* __restrict__ ssm_state, float* __restrict__ x) {
    NBSS_LDS(smem);
    float* U = reinterpret_cast<float*>(smem);  // [C][96]   LN(x); from stage 4 on DBC [C][40]
    float* XC = U + C * ON_H;                   // [C][192]  xr, then the convolution's output
    float* Z = XC + C * MB_E;                   // [C][192]  z, then y SiLU(z)
    float* DBC = U;
    const int bf = blockIdx.x, e = threadIdx.x;
    float* xr = x + (size_t)bf * C * ON_H;
    on_layernorm(xr, C, lw, lb, U);
    MbChan ch;
    mb_chan(ch, cw, cb, wdt, bdt, alog, dp, e);
    __syncthreads();
    // in_proj of all frames: the two weight columns of this thread are read once per 8 frames
    for (int c0 = 0; c0 < C; c0 += 8) {
        float ax[8], az[8];
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) ax[cc] = az[cc] = 0.f;
        for (int i = 0; i < ON_H; ++i) {
            const float wx = win_t[i * 2 * MB_E + e], wz = win_t[i * 2 * MB_E + MB_E + e];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                const float uu = U[(c0 + cc < C ? c0 + cc : C - 1) * ON_H + i];
                ax[cc] += wx * uu;
                az[cc] += wz * uu;
            }
        }
#pragma unroll
        for (int cc = 0; cc < 8; ++cc)
            if (c0 + cc < C) {
                XC[(c0 + cc) * MB_E + e] = ax[cc];
                Z[(c0 + cc) * MB_E + e] = az[cc];
            }
    }
    // conv + SiLU: the thread's own column of XC (no barrier needed before it); the state is the last three inputs, also when C < 3
    {
        float* cs = conv_state + (size_t)bf * (MB_K - 1) * MB_E + e;
        float xm3 = cs[0], xm2 = cs[MB_E], xm1 = cs[2 * MB_E];
        for (int c = 0; c < C; ++c) {
            const float xin = XC[c * MB_E + e];
            XC[c * MB_E + e] = mb_conv(ch, xm3, xm2, xm1, xin);
            xm3 = xm2;
            xm2 = xm1;
            xm1 = xin;
        }
        cs[0] = xm3;
        cs[MB_E] = xm2;
        cs[2 * MB_E] = xm1;
    }
    __syncthreads();  // XC is complete; U has been read by every thread
    // x_proj: task = (run of 8 frames, output j); the weight column of j is read once per run
    for (int task = e; task < ((C + 7) >> 3) * MB_J; task += MB_E) {
        const int c0 = (task / MB_J) * 8, j = task % MB_J;
        float acc[8];
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) acc[cc] = 0.f;
        for (int i = 0; i < MB_E; ++i) {
            const float w = xproj_t[i * MB_J + j];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) acc[cc] += w * XC[(c0 + cc < C ? c0 + cc : C - 1) * MB_E + i];
        }
#pragma unroll
        for (int cc = 0; cc < 8; ++cc)
            if (c0 + cc < C) DBC[(c0 + cc) * MB_JL + j] = acc[cc];
    }
    __syncthreads();
    // the recurrence: 16 states per thread, from the caller's state and back to it
    {
        float* hs = ssm_state + (size_t)bf * MB_N * MB_E + e;
        float h[MB_N];
#pragma unroll
        for (int n = 0; n < MB_N; ++n) h[n] = hs[n * MB_E];
        for (int c = 0; c < C; ++c) {
            const float ys = mb_scan_frame(ch, h, DBC + c * MB_JL, XC[c * MB_E + e]);
            Z[c * MB_E + e] = ys * on_silu(Z[c * MB_E + e]);
        }
#pragma unroll
        for (int n = 0; n < MB_N; ++n) hs[n * MB_E] = h[n];
    }
    __syncthreads();
    if (e < ON_H) {
        for (int c0 = 0; c0 < C; c0 += 8) {
            float acc[8];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) acc[cc] = 0.f;
            for (int i = 0; i < MB_E; ++i) {
                const float wo = wo_t[i * ON_H + e];
#pragma unroll
                for (int cc = 0; cc < 8; ++cc) acc[cc] += wo * Z[(c0 + cc < C ? c0 + cc : C - 1) * MB_E + i];
            }
#pragma unroll
            for (int cc = 0; cc < 8; ++cc)
                if (c0 + cc < C) xr[(c0 + cc) * ON_H + e] += acc[cc];
        }
    }
}

extern "C" {

int nbss_online_mamba_step(int BF, int C, const float* ln_w, const float* ln_b, const float* win_t, const float* conv_w, const float* conv_b,
                           const float* xproj_t, const float* dtproj_w, const float* dtproj_b, const float* a_log, const float* d, const float* wo_t,
                           float* conv_state, float* ssm_state, float* x, void* stream) {
    if (BF <= 0 || C <= 0 || !ln_w || !ln_b || !win_t || !conv_w || !conv_b || !xproj_t || !dtproj_w || !dtproj_b || !a_log || !d || !wo_t || !conv_state ||
        !ssm_state || !x)
        return NBSS_EINVAL;
    if (C > ON_CMAX) return NBSS_EUNSUPPORTED;
    NBSS_LAUNCH(online_mamba_kernel, dim3(BF), dim3(MB_E), OM_FLOATS(C) * sizeof(float), (hipStream_t)stream, C, ln_w, ln_b, win_t, conv_w, conv_b, xproj_t,
                dtproj_w, dtproj_b, a_log, d, wo_t, conv_state, ssm_state, x);
    return NBSS_CHECK_LAUNCH();
}

}  // extern "C"
