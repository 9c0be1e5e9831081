// attn_tiles.h — the tile-level pieces the narrow-band attention kernels are written from, each once: gb_attn.hip (whole head in LDS) and attn_kb.hip
// (64-row blocks) use all of them; attn_relpos.hip and attn_relpos_kb.hip (the same two with Transformer-XL relative positions) use the image, the
// transposed fragments and the dispatch, and keep their K-step loops, softmax steps and stores inline (they measured slower on the helpers; their file
// headers say so).  The kernels keep their own loop structure (attn_kb.hip says why); what they share is
//   the LDS image of a head's rows  row-major [token][LD] of T: LD = DH (whole head) or DH + 16 bytes (key-blocked; see attn_kb.hip on the banks)
//   fragments                       rows of q / k / v / dO / P in natural K order (zero lanes from DH on), transposed fragments of an image
//   softmax steps                   mask + scale + running max, exp + sum, the online rescale of the key-blocked sweeps
//   the MTD MFMAs of a 32-token step against a transposed image, the guarded store of the MTD output tiles
//   AT_DISPATCH                     (dtype, head width) -> instantiation, for the launchers
// Lane roles throughout: l15 = lane & 15 is the MFMA N index (the wave's own query or key), rows 4 g4 + r of a C tile belong to lane group g4 = lane >> 4.
// Everything is forced inline and templated on what is a compile-time constant at its call sites.
#pragma once
#include "launch.h"

constexpr float AT_NEG = -3.0e38f;  // score of a masked key

// K index j of a fragment in the permuted order of two stacked C tiles -> token of the 32-token step
NBSS_DEV int at_perm_k(int g4, int j) { return j < 4 ? 4 * g4 + j : 16 + 4 * g4 + (j - 4); }

// ---- the image -------------------------------------------------------------------------------------------------------------------------------------
// rows t0 .. t0 + rows - 1 of the head's [Tn][DH] slice of a [N][ld] tensor into image rows 0 .. rows - 1, zero rows from Tn on: 16-byte pieces, NTH threads
template <class T, int DH, int LD, int NTH>
NBSS_DEV void at_stage(T* img, const T* src, int ld, int t0, int rows, int Tn) {
    constexpr int VE = 16 / sizeof(T), PR = DH / VE;
    for (int e = threadIdx.x; e < rows * PR; e += NTH) {
        const int r = e / PR, pc = e % PR;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (t0 + r < Tn) v = *reinterpret_cast<const u32x4*>(src + (size_t)(t0 + r) * ld + pc * VE);
        *reinterpret_cast<u32x4*>(img + (size_t)r * LD + pc * VE) = v;
    }
}
// A fragment whose K dimension is the token axis (permuted order), rows = channels 16 mt + l15, from an image: bf16 through two transposing reads
// (ds_read_b64_tr_b16), fp32 element by element.  DH = 24: rows 24 .. 31 of tile mt = 1 are never stored by the caller — bf16 reads them from whatever
// lies 16 bytes behind the row's 24 channels (the padding of LD > DH, the next row, the launcher's 64 spare bytes behind the last image: an MFMA row only
// reaches its own output row), fp32 takes zeros.
template <class T, int DH, int LD>
NBSS_DEV void at_frag_t(Frag<T>& f, const T* img, int tok0, int mt) {
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4;
    if constexpr (sizeof(T) == 2) {
        frag_load_tr(f, img + (size_t)(tok0 + 4 * g4 + (l15 >> 2)) * LD + 16 * mt + 4 * (l15 & 3), LD);
    } else if constexpr (DH % 16 == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) frag_set(f, j, load1(img + (size_t)(tok0 + at_perm_k(g4, j)) * LD + 16 * mt + l15));
    } else {
        const int d = 16 * mt + l15;
#pragma unroll
        for (int j = 0; j < 8; ++j) frag_set(f, j, d < DH ? load1(img + (size_t)(tok0 + at_perm_k(g4, j)) * LD + d) : 0.f);
    }
}
// acc[mt] += (tokens tok0 .. tok0 + 31 of the image)^T f, mt < MTD: O += V^T P, dQ += K^T dS, dV += dO^T P, dK += Q^T dS (f: frag_from_c2 of two C tiles)
template <class T, int DH, int LD>
NBSS_DEV void at_mma_t(f32x4* acc, const T* img, int tok0, const Frag<T>& f) {
#pragma unroll
    for (int mt = 0; mt < (DH + 15) / 16; ++mt) {
        Frag<T> t;
        at_frag_t<T, DH, LD>(t, img, tok0, mt);
        acc[mt] = mma(t, f, acc[mt]);
    }
}

// ---- fragments in natural K order --------------------------------------------------------------------------------------------------------------------
// K step ks of a row of DH channels (global memory or an image row): the lane's 8 channels from 32 ks + 8 g4, zeros from DH on and where !valid
template <class T, int DH>
NBSS_DEV void at_frag_row(Frag<T>& f, const T* row, int ks, bool valid = true) {
    const int d0 = 32 * ks + 8 * (lane_id() >> 4);
    frag_zero(f);
    if (valid && (DH % 32 == 0 || d0 < DH)) frag_load(f, row + d0);
}
template <class T, int DH>
NBSS_DEV void at_frag_rows(Frag<T>* f, const T* row, bool valid) {
#pragma unroll
    for (int ks = 0; ks < (DH + 31) / 32; ++ks) at_frag_row<T, DH>(f[ks], row, ks, valid);
}
// the MTD output tiles of the lane's row: channels 16 mt + 4 g4 + r, tiles past DH not stored
template <class T, int DH>
NBSS_DEV void at_store_row(T* row, const f32x4* acc) {
    const int g4 = lane_id() >> 4;
#pragma unroll
    for (int mt = 0; mt < (DH + 15) / 16; ++mt) {
        const int d = 16 * mt + 4 * g4;
        if (DH % 16 == 0 || d < DH) store4(row + d, acc[mt][0], acc[mt][1], acc[mt][2], acc[mt][3]);
    }
}

// ---- softmax over S^T tiles: rows = keys j0 + 16 jt + 4 g4 + r, column = the lane's query ---------------------------------------------------------------
// keys < Tn: score * scale, the others AT_NEG; returns the lane's maximum (reduce with wave_max16)
template <int NT>
NBSS_DEV float at_mask_scale_max(f32x4* st, int j0, int Tn, float scale) {
    const int g4 = lane_id() >> 4;
    float mx = AT_NEG;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool kv = j0 + 16 * jt + 4 * g4 + r < Tn;
            st[jt][r] = kv ? st[jt][r] * scale : AT_NEG;
            mx = fmaxf(mx, st[jt][r]);
        }
    return mx;
}
// keys < Tn: exp(score - mx), the others 0; returns the lane's sum (reduce with wave_sum16).  DOT: pd = the lane's sum of exp(..) dp along with it (the
// same loop: in a loop of its own the device compiler associates that sum differently and D moves by an ulp)
template <int NT, bool DOT = false>
NBSS_DEV float at_exp_sum(f32x4* st, int j0, int Tn, float mx, const f32x4* dp = nullptr, float* pd = nullptr) {
    const int g4 = lane_id() >> 4;
    float sum = 0.f, dot = 0.f;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool kv = j0 + 16 * jt + 4 * g4 + r < Tn;
            st[jt][r] = kv ? __expf(st[jt][r] - mx) : 0.f;
            sum += st[jt][r];
            if (DOT) dot += st[jt][r] * dp[jt][r];
        }
    if (DOT) *pd = dot;
    return sum;
}
// online softmax, one key block on: running max m -> mn, running sum l and the O tiles rescaled by alpha = exp(m - mn), ps = the block's sum of
// exp(score - mn); returns alpha (for whatever else runs along like l)
template <int MTD>
NBSS_DEV float at_online_rescale(float& m, float& l, f32x4* oacc, float mn, float ps) {
    const float alpha = __expf(m - mn);
    l = l * alpha + ps;
    m = mn;
#pragma unroll
    for (int mt = 0; mt < MTD; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) oacc[mt][r] *= alpha;
    return alpha;
}

// ---- launchers: (dtype, head width) -> fn<T, W>(...) ----------------------------------------------------------------------------------------------------
#define AT_DISPATCH(dtype, fn, W, ...) ((dtype) == NBSS_BF16 ? fn<bf16_t, W>(__VA_ARGS__) : fn<float, W>(__VA_ARGS__))
// the head widths of the whole-head kernels
#define AT_DISPATCH_NARROW(dtype, dh, fn, ...) \
    ((dh) == 48 ? AT_DISPATCH(dtype, fn, 48, __VA_ARGS__) : (dh) == 24 ? AT_DISPATCH(dtype, fn, 24, __VA_ARGS__) : NBSS_EUNSUPPORTED)
