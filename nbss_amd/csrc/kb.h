// kb.h — what the key-blocked attention kernels share (attn_kb.hip: softmax(q k^T) v at head widths 24 / 48 / 96; attn_relpos_kb.hip: the
// relative-position attention of NBC on long sequences): 64-row LDS blocks of a head's rows, row stride DH + 16 bytes.
#pragma once
#include "launch.h"

#define KB_THREADS 256
#define KB_BLK 64        // rows per LDS block = rows per workgroup (4 waves x one 16-row tile)
#define KB_TMAX 256      // frames per sequence of the training entry points (forward + backward)
#define KB_TLONG 4096    // frames per sequence of the forward-only *_long_fwd entry points

NBSS_DEV int kb_perm_k(int g4, int j) { return j < 4 ? 4 * g4 + j : 16 + 4 * g4 + (j - 4); }

// rows t0 .. t0 + 63 of the head's [Tn][DH] slice of a [N][ld] tensor into a row-major image (row stride DH + 16 bytes), zero rows from Tn on
template <class T, int DH>
NBSS_DEV void kb_stage(T* img, const T* src, int ld, int t0, int Tn) {
    constexpr int VE = 16 / sizeof(T), PR = DH / VE, LD = DH + VE;
    for (int e = threadIdx.x; e < KB_BLK * PR; e += KB_THREADS) {
        const int r = e / PR, pc = e % PR;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (t0 + r < Tn) v = *reinterpret_cast<const u32x4*>(src + (size_t)(t0 + r) * ld + pc * VE);
        *reinterpret_cast<u32x4*>(img + (size_t)r * LD + pc * VE) = v;
    }
}
// A fragment whose K dimension is the token axis (permuted order: two stacked C tiles), rows = channels 16 mt + l15, from such an image.  DH = 24: the
// rows 24 .. 31 of tile mt = 1 are never stored by the caller — bf16 reads them from the row's 16 bytes of padding (whatever they hold: an MFMA row only
// reaches its own output row), fp32 (4 words of padding) takes zeros.
template <class T, int DH>
NBSS_DEV void kb_frag_t(Frag<T>& f, const T* img, int tok0, int mt) {
    constexpr int LD = DH + 16 / sizeof(T);
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4;
    if constexpr (sizeof(T) == 2) {
        frag_load_tr(f, img + (size_t)(tok0 + 4 * g4 + (l15 >> 2)) * LD + 16 * mt + 4 * (l15 & 3), LD);
    } else if constexpr (DH % 16 == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) frag_set(f, j, load1(img + (size_t)(tok0 + kb_perm_k(g4, j)) * LD + 16 * mt + l15));
    } else {
        const int d = 16 * mt + l15;
#pragma unroll
        for (int j = 0; j < 8; ++j) frag_set(f, j, d < DH ? load1(img + (size_t)(tok0 + kb_perm_k(g4, j)) * LD + d) : 0.f);
    }
}
