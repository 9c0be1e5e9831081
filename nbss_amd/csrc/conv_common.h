// conv_common.h — what the two RIR convolutions (conv1d.hip: one response per row; conv_traj.hip: a trajectory of responses) share: the limits of the
// C ABI and the exact-fp32 matrix-core product.
#pragma once
#include "common.h"

#define CONV_MAX_L 65536
#define CONV_MAX_N (1 << 24)
#define CONV_MAX_M 4096
#define CONV_MAX_ROWS (1 << 22)             // B S M (conv_traj.hip: B S P M)
#define CONV_MAX_ITEMS 2048                 // (b, s) pairs per grid pass; a workgroup walks the others in steps of the grid

NBSS_DEV f32x4 conv_mfma(float a, float b, f32x4 c) {
#ifdef NBSS_EMU
    return hipemu::mfma_16x16x4_f32(a, b, c);
#else
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
#endif
}
