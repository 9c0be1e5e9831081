// online.h — what the streaming-step kernels of the OnlineSpatialNet share (online.hip, online_mamba_step.hip): the geometry, SiLU and the LayerNorm of a
// chunk's frames.
#pragma once
#include "launch.h"

#define ON_H 96
#define ON_FFN 192
#define ON_CMAX 32  // frames per chunk

NBSS_DEV float on_silu(float x) { return x / (1.0f + __expf(-x)); }

// LayerNorm over H = 96 of the C frames of one sequence: wave w takes frames w, w + nw, ...; u[c][96] in LDS
NBSS_DEV void on_layernorm(const float* __restrict__ xrow, int C, const float* __restrict__ lw, const float* __restrict__ lb, float* u) {
    const int lane = lane_id(), w = wave_id(), nw = (int)(blockDim.x >> 6);
    for (int c = w; c < C; c += nw) {
        const float a = xrow[c * ON_H + lane], b = lane < 32 ? xrow[c * ON_H + 64 + lane] : 0.f;
        const float mean = wave_sum64(a + b) * (1.0f / ON_H);
        const float da = a - mean, db = lane < 32 ? b - mean : 0.f;
        const float rstd = rsqrtf(wave_sum64(da * da + db * db) * (1.0f / ON_H) + 1e-5f);
        u[c * ON_H + lane] = da * rstd * lw[lane] + lb[lane];
        if (lane < 32) u[c * ON_H + 64 + lane] = db * rstd * lw[64 + lane] + lb[64 + lane];
    }
}
