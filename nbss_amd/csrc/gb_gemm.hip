// gb_gemm.hip — weight re-lay and tap_gemm of the geometry-generic path (gb.h):
//   Y[n][o] = sum_tap sum_i X[n + (tap - c) S][i] W[g][tap][o][i] (+ bias, SiLU on load / on store): every per-token linear map, the grouped
//   convolutions along F and along T, the LinearGroup (rows = (b, t), groups = squeeze channels) AND their data gradients (same form with the
//   weights re-laid by wprep).  MFMA straight from global memory: weights = A, tokens = N.
#include "gb.h"

// ------------------------------------------------------------------------------------------------------------------------------------
// re-lay of an fp32 parameter into tap_gemm's weight layout (gb.h: WPrep)
template <class T>
NBSS_DEV void gb_wprep_body(const WPrep& p) {
    const long total = (long)p.groups * p.taps * p.Mp * p.Kp;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int k = (int)(e % p.Kp);
        long r = e / p.Kp;
        const int m = (int)(r % p.Mp);
        r /= p.Mp;
        const int tap = (int)(r % p.taps), g = (int)(r / p.taps);
        float v = 0.f;
        if (m < p.Mg && k < p.Kv) {
            switch (p.mode) {
                case WP_LIN_FWD: v = p.src[(long)m * p.Kv + k]; break;                                                   // W[o = m][i = k]
                case WP_LIN_DGRAD: v = p.src[(long)k * p.Mg + m]; break;                                                 // W[o = k][i = m]
                case WP_CONV_FWD: v = p.src[(((long)g * p.Mg + m) * p.Kv + k) * p.taps + tap]; break;                    // W[g Og + o][i][tap]
                case WP_CONV_DGRAD: v = p.src[(((long)g * p.Kv + k) * p.Mg + m) * p.taps + (p.taps - 1 - tap)]; break;   // W[g Og + o = k][i = m][flipped]
                case WP_LG_FWD: v = p.src[((long)g * p.Mg + m) * p.Mg + k]; break;                                       // Wf[g][k' = m][h = k]   (Mg = Kv = F)
                case WP_LG_DGRAD: v = p.src[((long)g * p.Mg + k) * p.Mg + m]; break;                                     // Wf[g][k' = k][h = m]
            }
        }
        store1(reinterpret_cast<T*>(p.dst) + e, v);
    }
}

template <class T>
__global__ void gb_wprep_kernel(WPrep p) { gb_wprep_body<T>(p); }
template <class T>
__global__ void gb_wprep_multi_kernel(WPrepMulti m) { gb_wprep_body<T>(m.d[blockIdx.y]); }

// epilogue of one row: 4 output tiles in C layout (lane: outputs 16 i + 4 g4 + r of its row)
template <class T>
NBSS_DEV void gb_tap_store(const TapGemm& p, const f32x4 (&acc)[4], long row, int g, int mc, int g4) {
    const size_t ro = (size_t)row * p.ldy + p.ycol + (size_t)g * p.ygs;
    T* yr = reinterpret_cast<T*>(p.Y) + ro;
    T* y2 = p.Y2 ? reinterpret_cast<T*>(p.Y2) + ro : nullptr;
    const T* da = p.Dact ? reinterpret_cast<const T*>(p.Dact) + ro : nullptr;
    const T* rr = p.R ? reinterpret_cast<const T*>(p.R) + (size_t)row * p.ldr + p.ycol + (size_t)g * p.ygs : nullptr;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m0 = (mc * 4 + i) * 16 + 4 * g4;
        if (m0 >= p.Mg) continue;
        float o[4], o2[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[i][r];
            const bool ok = m0 + r < p.Mg;
            if (p.bias && ok) v += p.bias[(size_t)g * p.bgs + m0 + r];
            if (p.yact) v = silu_f(v);
            if (da && ok) v *= dsilu_f(load1(da + m0 + r));
            if (rr && ok) v = load1(rr + m0 + r) + round_to(v, yr);
            o[r] = v;
            o2[r] = silu_f(round_to(v, yr));  // (the activation of the STORED pre-activation: what a separate pass over Y would compute)
        }
        if (m0 + 3 < p.Mg) {
            store4(yr + m0, o[0], o[1], o[2], o[3]);
            if (y2) store4(y2 + m0, o2[0], o2[1], o2[2], o2[3]);
        } else {
            for (int r = 0; r < 4 && m0 + r < p.Mg; ++r) {
                store1(yr + m0 + r, o[r]);
                if (y2) store1(y2 + m0 + r, o2[r]);
            }
        }
    }
}

// One wave = 16 rows (the MFMA N dimension) x up to 64 outputs (4 tiles of 16) of one group; operands come straight from global memory
// (B: 8 contiguous inputs of the lane's row; A: 8 contiguous prepared weights of the lane's output row — L2-resident, every wave reads
// the same few KB).  No LDS, no staging: this is the simple generic path, not the speed-of-light one.
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_tap_gemm_kernel(TapGemm p) {
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id();
    const int mchunks = cdiv(p.Mp, 64);
    const int g = blockIdx.y / mchunks, mc = blockIdx.y % mchunks;
    const long row = ((long)blockIdx.x * (GB_THREADS / 64) + w) * 16 + l15;
    const bool rv = row < p.rows;
    const int pos = rv ? (int)((row / p.pos_div) % p.pos_len) : 0;
    const T* X = reinterpret_cast<const T*>(p.X);
    const T* Wg = reinterpret_cast<const T*>(p.W) + (size_t)g * p.taps * p.Mp * p.Kp;
    f32x4 acc[4] = {F32X4_ZERO, F32X4_ZERO, F32X4_ZERO, F32X4_ZERO};
    for (int tap = 0; tap < p.taps; ++tap) {
        const int d = tap - p.center;
        const bool valid = rv && pos + d >= 0 && pos + d < p.pos_len;
        const T* xr = X + (size_t)(valid ? row + (long)d * p.shift : 0) * p.ldx + p.xcol + (size_t)g * p.xgs;
        for (int k0 = 0; k0 < p.Kp; k0 += 32) {
            const int kk = k0 + 8 * g4;
            Frag<T> b;
            if (valid && kk < p.Kg) {
                frag_load(b, xr + kk);
                if (p.xact) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) frag_set(b, j, silu_f(frag_get(b, j)));
                }
            } else {
                frag_zero(b);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m0 = (mc * 4 + i) * 16;
                if (m0 < p.Mp) {
                    Frag<T> a;
                    frag_load(a, Wg + ((size_t)tap * p.Mp + m0 + l15) * p.Kp + kk);
                    acc[i] = mma(a, b, acc[i]);
                }
            }
        }
    }
    if (rv) gb_tap_store<T>(p, acc, row, g, mc, g4);
}

// The same contraction with the weights of the workgroup's (group, 64-output chunk) staged in LDS for all taps and GT_R row tiles per wave:
// without it every wave re-read its 64 x K weight block from L2 for 16 rows of work (25.8 % of the large train step).  Row stride of the image:
// Kp + 8 elements (a multiple of 16 bytes that is not a multiple of 128: the 16 rows of a fragment read spread over the banks).
#define GT_R 4
template <class T>
__global__ __launch_bounds__(GB_THREADS) void gb_tap_gemm_lds_kernel(TapGemm p) {
    NBSS_LDS(smem);
    T* Wl = reinterpret_cast<T*>(smem);  // [taps][64][Kp + 8]
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id();
    const int mchunks = cdiv(p.Mp, 64);
    const int g = blockIdx.y / mchunks, mc = blockIdx.y % mchunks;
    const int LDW = p.Kp + 8;
    const int mrows = p.Mp - mc * 64 < 64 ? p.Mp - mc * 64 : 64;  // rows of this chunk (a multiple of 16)
    {
        const T* Wg = reinterpret_cast<const T*>(p.W) + (size_t)g * p.taps * p.Mp * p.Kp;
        constexpr int VE = 16 / sizeof(T);  // elements per 16-byte piece
        const int vpr = p.Kp / VE, nv = p.taps * mrows * vpr;
        for (int v = threadIdx.x; v < nv; v += GB_THREADS) {
            const int col = (v % vpr) * VE, r = (v / vpr) % mrows, tap = v / (vpr * mrows);
            *reinterpret_cast<u32x4*>(Wl + ((size_t)tap * 64 + r) * LDW + col) =
                *reinterpret_cast<const u32x4*>(Wg + ((size_t)tap * p.Mp + mc * 64 + r) * p.Kp + col);
        }
    }
    __syncthreads();
    const T* X = reinterpret_cast<const T*>(p.X);
    for (int rt = 0; rt < GT_R; ++rt) {
        const long row = (((long)blockIdx.x * (GB_THREADS / 64) + w) * GT_R + rt) * 16 + l15;
        if ((row - l15) >= p.rows) break;  // (wave-uniform: the tile's first row)
        const bool rv = row < p.rows;
        const int pos = rv ? (int)((row / p.pos_div) % p.pos_len) : 0;
        f32x4 acc[4] = {F32X4_ZERO, F32X4_ZERO, F32X4_ZERO, F32X4_ZERO};
        for (int tap = 0; tap < p.taps; ++tap) {
            const int d = tap - p.center;
            const bool valid = rv && pos + d >= 0 && pos + d < p.pos_len;
            const T* xr = X + (size_t)(valid ? row + (long)d * p.shift : 0) * p.ldx + p.xcol + (size_t)g * p.xgs;
            const T* wt = Wl + (size_t)tap * 64 * LDW + (size_t)l15 * LDW;
#pragma unroll 2
            for (int k0 = 0; k0 < p.Kp; k0 += 32) {
                const int kk = k0 + 8 * g4;
                Frag<T> b;
                if (valid && kk < p.Kg) {
                    frag_load(b, xr + kk);
                    if (p.xact) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) frag_set(b, j, silu_f(frag_get(b, j)));
                    }
                } else {
                    frag_zero(b);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i * 16 < mrows) {
                        Frag<T> a;
                        frag_load(a, wt + (size_t)i * 16 * LDW + kk);
                        acc[i] = mma(a, b, acc[i]);
                    }
                }
            }
        }
        if (rv) gb_tap_store<T>(p, acc, row, g, mc, g4);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// launchers
template <class T>
int gb_wprep(const float* src, void* dst, int mode, int groups, int taps, int Mg, int Kv, int Mp, int Kp, hipStream_t st) {
    WPrep p = {src, dst, mode, groups, taps, Mg, Kv, Mp, Kp};
    NBSS_LAUNCH((gb_wprep_kernel<T>), dim3(gb_blocks((long)groups * taps * Mp * Kp, 256)), dim3(256), 0, st, p);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int WPrepBatch<T>::launch(hipStream_t st) {
    NBSS_LAUNCH((gb_wprep_multi_kernel<T>), dim3(gb_blocks(most, 256), n), dim3(256), 0, st, m);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
int gb_gemm(const TapGemm& p, hipStream_t st) {
    if (p.Kg % 8 || p.ldx % 8 || p.xcol % 8 || p.xgs % 8 || p.ycol % 4 || p.ygs % 4 || p.ldy % 4) return NBSS_EUNSUPPORTED;
    if (sizeof(T) == 2 && gl_gemm_takes(p)) return gl_gemm_bf16(p, st);
    const size_t lds = (size_t)p.taps * 64 * (p.Kp + 8) * sizeof(T);
    if (lds <= 150 * 1024) {
        int e = NBSS_SET_MAX_LDS((gb_tap_gemm_lds_kernel<T>), lds);
        if (e) return e;
        dim3 grid(cdiv(p.rows, 64 * GT_R), p.groups * cdiv(p.Mp, 64));
        NBSS_LAUNCH((gb_tap_gemm_lds_kernel<T>), grid, dim3(GB_THREADS), lds, st, p);
        return NBSS_CHECK_LAUNCH();
    }
    dim3 grid(cdiv(p.rows, 64), p.groups * cdiv(p.Mp, 64));
    NBSS_LAUNCH((gb_tap_gemm_kernel<T>), grid, dim3(GB_THREADS), 0, st, p);
    return NBSS_CHECK_LAUNCH();
}

#define GB_INSTANTIATE(T)                                                                          \
    template int gb_wprep<T>(const float*, void*, int, int, int, int, int, int, int, hipStream_t); \
    template int WPrepBatch<T>::launch(hipStream_t);                                               \
    template int gb_gemm<T>(const TapGemm&, hipStream_t);
GB_INSTANTIATE(float)
GB_INSTANTIATE(bf16_t)
