// conv_common.h — what the two RIR convolutions (conv1d.hip: one response per row; conv_traj.hip: a trajectory of responses) share: the limits of the
// C ABI, the chunk of taps of the blocked Hankel product and its staging into LDS, the exact-fp32 matrix-core product, and the choice of the kernel
// instance.  What differs stays in the two files: the strip of x (plain / weighted), the outputs per workgroup, the split over the waves.
#pragma once
#include <type_traits>
#include "common.h"

#define CONV_MAX_L 65536
#define CONV_MAX_N (1 << 24)
#define CONV_MAX_M 4096
#define CONV_MAX_ROWS (1 << 22)             // B S M (conv_traj.hip: B S P M)
#define CONV_MAX_ITEMS 2048                 // (b, s) pairs per grid pass; a workgroup walks the others in steps of the grid

#define CONV_THREADS 256
#define CONV_QMAX 128                       // tap blocks per chunk
#define CONV_KT (16 * CONV_QMAX)            // taps per chunk
#define CONV_TMAX ((CONV_QMAX + 15 + 3) / 4)  // K steps per chunk: the columns w = u + 15 = 0 .. q_count + 14, four per step
#define CONV_HS 161                         // row of HT in floats: j = i + w <= 15 + 4 CONV_TMAX - 1 = 158

static_assert((16 * CONV_HS) % 4 == 0, "the strip behind HT is staged in 16-byte pieces");
static_assert(15 + 4 * CONV_TMAX - 1 < CONV_HS, "HT row too short");

NBSS_DEV f32x4 conv_mfma(float a, float b, f32x4 c) {
#ifdef NBSS_EMU
    return hipemu::mfma_16x16x4_f32(a, b, c);
#else
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
#endif
}

// One chunk of qn tap blocks from tap k0 of the MB response rows at hrow (microphones m0 .., L taps each) into HT [MB][16][CONV_HS]:
// HT[m][r][15 + q] = h[m][k0 + 16 q + r], zero for taps beyond L and microphones beyond M, and zero columns j < 15 and j >= 15 + qn around them.
// VEC: 16-byte loads (L % 4 == 0 and k % 4 == 0, so a piece is inside or outside as a whole).
template <int MB, bool VEC>
NBSS_DEV void conv_stage_taps(float* __restrict__ HT, const float* __restrict__ hrow, int m0, int M, int L, int k0, int qn, int tid) {
    constexpr int W = VEC ? 4 : 1;
    const int pad = CONV_HS - qn;
    for (int e = tid; e < MB * 16 * pad; e += CONV_THREADS) {
        const int rowi = e / pad, pj = e - rowi * pad;
        HT[rowi * CONV_HS + (pj < 15 ? pj : pj + qn)] = 0.f;
    }
    const int per_m = qn * (16 / W);
    for (int e = tid; e < MB * per_m; e += CONV_THREADS) {
        const int m = e / per_m, rem = e - m * per_m, q = rem / (16 / W), r = (rem - q * (16 / W)) * W;
        const int k = k0 + 16 * q + r;
        const bool in = m0 + m < M && k < L;
        float v[W];
        if (VEC) {
            f32x4 t = F32X4_ZERO;
            if (in) t = *reinterpret_cast<const f32x4*>(hrow + (size_t)m * L + k);
#pragma unroll
            for (int z = 0; z < W; ++z) v[z] = t[z];
        } else {
            v[0] = in ? hrow[(size_t)m * L + k] : 0.f;
        }
#pragma unroll
        for (int z = 0; z < W; ++z) HT[(m * 16 + r + z) * CONV_HS + 15 + q] = v[z];
    }
}

// microphones per workgroup: 3 (the six-microphone arrays take two groups), fewer where 3 would idle a third or more of the accumulators.  A function
// of M alone, so an item's sum order does not depend on the batch.
static inline int conv_mic_group(int M) { return M == 1 ? 1 : (M == 2 || M == 4) ? 2 : 3; }

// rows that start on 16-byte boundaries are staged with 16-byte loads
static inline bool conv_vec(int N, int L, const float* x, const float* h) {
    return N % 4 == 0 && L % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(h)) & 15) == 0;
}

// launch(std::integral_constant<int, MB>, std::bool_constant<vec>) -> return code: the caller launches its kernel<MB, vec> from the types
template <class F>
static int conv_dispatch(int MB, bool vec, F launch) {
    using T = std::true_type;
    using N = std::false_type;
    switch (MB) {
        case 1: return vec ? launch(std::integral_constant<int, 1>(), T()) : launch(std::integral_constant<int, 1>(), N());
        case 2: return vec ? launch(std::integral_constant<int, 2>(), T()) : launch(std::integral_constant<int, 2>(), N());
        default: return vec ? launch(std::integral_constant<int, 3>(), T()) : launch(std::integral_constant<int, 3>(), N());
    }
}
