// online_ret_train.hip — the chunkwise retention core of the OnlineSpatialNet for TRAINING: what lies between the q / k / v / g projections and out_proj
// in models/arch/base/retention.py (MultiScaleRetention.chunk_recurrent_forward -> group_norm -> SiLU(g) *), forward and backward, for 4 heads of key
// width 24 and value width 48, chunks of 64 frames, no rotary positions, no look-ahead.
//
// Per sequence n and head h (gamma = decay[h], frames cut into chunks of 64, i / j indices inside a chunk of m <= 64 frames, S the [24][48] fp32 state):
//   k'_j  = k_scale k_j                                    (k == NULL: k' = q)
//   rs_i  = sqrt(sum_{d<=i} gamma^d)
//   sc_ij = (q_i . k'_j) gamma^(i-j) / rs_i                for j <= i
//   ab_i  = max(1, sum_j |sc_ij|)                          a constant for the gradient (the module detaches it)
//   o_i   = sum_j (sc_ij / ab_i) v_j + gamma^(i+1) (q_i S) / (rs_i ab_i)
//   S    <- gamma^m S + sum_i gamma^(m-1-i) k'_i^T v_i
//   out_i = SiLU(g_i) o_i rsqrt(mean_48(o_i^2) + 1e-6)
//
// One workgroup of four waves owns a (sequence, head) and walks its chunks in order (a grid-stride loop over the BF x 4 pairs).  Per chunk the head's q, k', v
// rows are staged as fp32 images in LDS; every product runs on MFMA with fragments built from those images (fp32 stream: fp32 MFMA; bf16 stream: the operands
// rounded to bf16, fp32 accumulation).  Wave w owns the queries 16 w .. 16 w + 15 (the MFMA N index is the lane's own query, so row sums and the RMS
// statistics are sums inside a lane and over the four lane groups), and in the backward also the KEYS 16 w .. 16 w + 15 for dk / dv, whose sums run over
// the queries of all four waves: P and dA pass through one [64][64] LDS image.  The decay powers, rs, ab, the RMS statistics and S / dS are fp32 in either
// stream dtype; the state update and the dS update are plain fp32 FMAs in frame order.
//
// The backward walks the chunks in REVERSE and carries dS.  It needs the forward state at the start of every chunk and takes it from `save`:
//   SAVED       save [BF][4][ceil(T / 64)][24][48] fp32 — S at the start of each chunk (chunk 0: zeros)
//   RECOMPUTED  the scores, ab_i, P, o_i and the RMS statistics of the chunk (one forward pass over the chunk's images)
// With P_ij = sc_ij / ab_i, W_ij = gamma^(i-j) / (rs_i ab_i), c_i = gamma^(i+1) / (rs_i ab_i), e_j = gamma^(m-1-j) and do_i the gradient at o_i:
//   dA_ij = (do_i . v_j) W_ij      dq_i = sum_j dA_ij k'_j + c_i S do_i      dk'_j = sum_i dA_ij q_i + e_j dS v_j      dv_j = sum_i P_ij do_i + e_j k'_j dS
//   dS   <- gamma^m dS + sum_i c_i q_i^T do_i
// No atomics, every sum in a fixed order: two calls give the same bits, and a sequence's rows do not depend on the other sequences of the launch.
#include "gb.h"

#define RT_HEADS 4
#define RT_DK 24
#define RT_DV 48
#define RT_E (RT_HEADS * RT_DK)   // 96: row of q, k
#define RT_VD (RT_HEADS * RT_DV)  // 192: row of v, g, out
#define RT_C 64                   // frames per chunk
#define RT_THREADS 256
#define RT_GRID_CAP 4096          // workgroups per launch; more (sequence, head) pairs are walked by the grid-stride loop
#define RT_STATE (RT_DK * RT_DV)  // floats of one state
// LDS images, fp32, odd row lengths (a fragment's 16 lanes read 16 rows, or 16 columns, of an image at once)
#define RT_LQ 25  // q, k'  [64][24]
#define RT_LV 49  // v, do  [64][48]
#define RT_LP 65  // P / dA [64][64]: row = query, column = key
#define RT_LS 49  // S, dS  [32][48]: rows 24 .. 31 stay zero (the second 16-row tile of an MFMA operand)
#define RT_O_Q 0
#define RT_O_K (RT_O_Q + RT_C * RT_LQ)
#define RT_O_V (RT_O_K + RT_C * RT_LQ)
#define RT_O_P (RT_O_V + RT_C * RT_LV)
#define RT_O_S (RT_O_P + RT_C * RT_LP)
#define RT_O_PW (RT_O_S + 32 * RT_LS)  // gamma^d, d = 0 .. 64
#define RT_O_IRS (RT_O_PW + 68)        // 1 / rs_i
#define RT_O_CF (RT_O_IRS + RT_C)      // c_i of the current chunk (backward)
#define RT_FWD_FLOATS (RT_O_CF + RT_C)
#define RT_O_DO RT_FWD_FLOATS
#define RT_O_DS (RT_O_DO + RT_C * RT_LV)
#define RT_BWD_FLOATS (RT_O_DS + 32 * RT_LS)

static int rt_chunks(int T) { return (T + RT_C - 1) / RT_C; }
// NBSS_OK, or why the shape is refused
static int rt_check(int dtype, int64_t BF, int T) {
    if ((dtype != NBSS_F32 && dtype != NBSS_BF16) || BF < 1) return NBSS_EINVAL;
    if (T < 1 || T > NBSS_T_MAX || BF * T > (1L << 28)) return NBSS_EUNSUPPORTED;
    return NBSS_OK;
}

// ---- fragments from an fp32 LDS image (natural K order: the lane's 8 K indices are k0 + 8 g4 .. + 7) -------------------------------------------------
// the lane's row (row0 + l15), K along the row; zeros from kmax on
template <class T>
NBSS_DEV void rt_frag_rows(Frag<T>& f, const float* img, int ld, int row0, int k0, int kmax) {
    const int lane = lane_id(), kb = k0 + 8 * (lane >> 4);
    const float* p = img + (row0 + (lane & 15)) * ld;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool ok = kb + j < kmax;
        frag_set(f, j, keep_if(ok, p[ok ? kb + j : 0]));
    }
}
// the lane's column (col0 + l15, zeros from cmax on), K down the rows; zeros from kmax on
template <class T>
NBSS_DEV void rt_frag_cols(Frag<T>& f, const float* img, int ld, int col0, int cmax, int k0, int kmax) {
    const int lane = lane_id(), kb = k0 + 8 * (lane >> 4), col = col0 + (lane & 15);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool ok = col < cmax && kb + j < kmax;
        frag_set(f, j, keep_if(ok, img[ok ? (kb + j) * ld + col : 0]));
    }
}

// rows 0 .. m - 1 of a head's [T][width] slice (row length gld) times `scale` into an image, zero rows from m on
template <class T>
NBSS_DEV void rt_stage(float* img, int ld, const T* src, int gld, int width, int m, float scale) {
    const int pr = width / 4;
    for (int e = threadIdx.x; e < RT_C * pr; e += RT_THREADS) {
        const int r = e / pr, c = (e % pr) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < m) load4(src + (size_t)r * gld + c, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) img[r * ld + c + j] = v[j] * scale;
    }
}

// gamma^d (d = 0 .. 64) and 1 / rs_i of a head; ends with a barrier
NBSS_DEV void rt_tables(float* L, float gamma) {
    const int tid = threadIdx.x;
    const float lg = logf(gamma);
    if (tid <= RT_C) L[RT_O_PW + tid] = expf((float)tid * lg);
    __syncthreads();
    if (tid < RT_C) {
#pragma clang fp reassociate(off)
        float s = 0.f;
        for (int d = 0; d <= tid; ++d) s += L[RT_O_PW + d];
        L[RT_O_IRS + tid] = 1.0f / sqrtf(s);
    }
    __syncthreads();
}

// what a wave keeps of its 16 queries (the lane's query: 16 w + l15)
struct RtRows {
    f32x4 p[4];  // P^T tiles: keys 16 jt + 4 g4 + r
    f32x4 o[3];  // o^T tiles: channels 16 mt + 4 g4 + r
    float wrow;  // 1 / (rs_i ab_i)
    float cf;    // gamma^(i+1) / (rs_i ab_i)
};
// scores, ab, P (registers and the wave's rows of the P image) and o of the wave's queries, from the chunk's images and the state at its start.
// A wave whose queries all lie behind the chunk's m frames only clears its rows of the P image.
template <class T>
NBSS_DEV void rt_rows_fwd(RtRows& R, float* L, int w, int m) {
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, i = 16 * w + l15;
    const float* pw = L + RT_O_PW;
    float* prow = L + RT_O_P + i * RT_LP;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) R.p[jt] = F32X4_ZERO;
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) R.o[mt] = F32X4_ZERO;
    R.wrow = 0.f;
    R.cf = 0.f;
    if (16 * w >= m) {
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) prow[16 * jt + 4 * g4 + r] = 0.f;
        return;
    }
    const float irs = L[RT_O_IRS + i];
    Frag<T> fq, fk;
    rt_frag_rows<T>(fq, L + RT_O_Q, RT_LQ, 16 * w, 0, RT_DK);
    float asum = 0.f;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
        if (jt > w) continue;  // keys behind every query of the wave
        rt_frag_rows<T>(fk, L + RT_O_K, RT_LQ, 16 * jt, 0, RT_DK);
        const f32x4 st = mma(fk, fq, F32X4_ZERO);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = i - (16 * jt + 4 * g4 + r);
            const float sc = st[r] * keep_if(d >= 0, pw[d >= 0 ? d : 0] * irs);
            R.p[jt][r] = sc;
            asum += fabsf(sc);
        }
    }
    const float ab = fmaxf(1.0f, wave_sum16(asum));
    R.wrow = irs / ab;
    R.cf = pw[l15 + 16 * w + 1] * R.wrow;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            R.p[jt][r] = R.p[jt][r] / ab;
            prow[16 * jt + 4 * g4 + r] = R.p[jt][r];
        }
    wave_lds_sync();
    const int kend = (m + 31) >> 5;
    Frag<T> fa, fb;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        if (ks > (w >> 1) || ks >= kend) continue;
        rt_frag_rows<T>(fb, L + RT_O_P, RT_LP, 16 * w, 32 * ks, RT_C);
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            rt_frag_cols<T>(fa, L + RT_O_V, RT_LV, 16 * mt, RT_DV, 32 * ks, RT_C);
            R.o[mt] = mma(fa, fb, R.o[mt]);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {  // the part of the earlier chunks: S^T q_i
        rt_frag_cols<T>(fa, L + RT_O_S, RT_LS, 16 * mt, RT_DV, 0, RT_DK);
        const f32x4 xo = mma(fa, fq, F32X4_ZERO);
#pragma unroll
        for (int r = 0; r < 4; ++r) R.o[mt][r] += xo[r] * R.cf;
    }
}
// rsqrt(mean_48(o^2) + 1e-6) of the lane's query
NBSS_DEV float rt_rms(const RtRows& R) {
    float ss = 0.f;
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) ss += R.o[mt][r] * R.o[mt][r];
    return rsqrtf(wave_sum16(ss) * (1.0f / RT_DV) + 1e-6f);
}
// st[c][d] = gamma^m st[c][d] + sum_i coef_i A[i][c] B[i][d] in frame order (the state update: A = k', B = v; the dS update: A = q, B = do)
NBSS_DEV void rt_state_update(float* st, const float* A, const float* B, const float* coef, int cstep, float gm, int m) {
    for (int e = threadIdx.x; e < RT_STATE; e += RT_THREADS) {
#pragma clang fp reassociate(off)
        const int c = e / RT_DV, d = e % RT_DV;
        float s = gm * st[c * RT_LS + d];
        for (int i = 0; i < m; ++i) s += coef[cstep * i] * A[i * RT_LQ + c] * B[i * RT_LV + d];
        st[c * RT_LS + d] = s;
    }
}

struct RtArgs {
    const void *q, *k, *v, *g, *d_out;
    void *out, *dq, *dk, *dv, *dg;
    float* save;
    const float* decay;
    float k_scale;
    long BF;
    int T;
};

template <class T>
__global__ __launch_bounds__(RT_THREADS) void rt_fwd_kernel(RtArgs a) {
    NBSS_LDS(smem);
    float* L = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id_u();
    const int Tn = a.T, nch = (Tn + RT_C - 1) / RT_C;
    for (long wi = blockIdx.x; wi < a.BF * RT_HEADS; wi += gridDim.x) {
        const long n = wi / RT_HEADS;
        const int h = (int)(wi % RT_HEADS);
        __syncthreads();  // the previous pair's readers are done
        for (int e = tid; e < 32 * RT_LS; e += RT_THREADS) L[RT_O_S + e] = 0.f;
        rt_tables(L, a.decay[h]);
        const T* q = (const T*)a.q + n * Tn * RT_E + h * RT_DK;
        const T* k = a.k ? (const T*)a.k + n * Tn * RT_E + h * RT_DK : q;
        const T* v = (const T*)a.v + n * Tn * RT_VD + h * RT_DV;
        const T* g = (const T*)a.g + n * Tn * RT_VD + h * RT_DV;
        T* out = (T*)a.out + n * Tn * RT_VD + h * RT_DV;
        for (int ch = 0; ch < nch; ++ch) {
            const int c0 = ch * RT_C, m = Tn - c0 < RT_C ? Tn - c0 : RT_C;
            __syncthreads();  // the state is updated, the images are free
            rt_stage<T>(L + RT_O_Q, RT_LQ, q + (size_t)c0 * RT_E, RT_E, RT_DK, m, 1.0f);
            rt_stage<T>(L + RT_O_K, RT_LQ, k + (size_t)c0 * RT_E, RT_E, RT_DK, m, a.k ? a.k_scale : 1.0f);
            rt_stage<T>(L + RT_O_V, RT_LV, v + (size_t)c0 * RT_VD, RT_VD, RT_DV, m, 1.0f);
            if (a.save) {
                float* sv = a.save + ((size_t)wi * nch + ch) * RT_STATE;
                for (int e = tid; e < RT_STATE; e += RT_THREADS) sv[e] = L[RT_O_S + (e / RT_DV) * RT_LS + e % RT_DV];
            }
            __syncthreads();
            RtRows R;
            rt_rows_fwd<T>(R, L, w, m);
            const int i = 16 * w + l15;
            if (16 * w < m) {  // wave-uniform: every lane of the wave takes part in rt_rms
                const float rinv = rt_rms(R);
                if (i < m) {
#pragma unroll
                    for (int mt = 0; mt < 3; ++mt) {
                        const size_t off = (size_t)(c0 + i) * RT_VD + 16 * mt + 4 * g4;
                        float gv[4];
                        load4(g + off, gv);
                        store4(out + off, silu_f(gv[0]) * R.o[mt][0] * rinv, silu_f(gv[1]) * R.o[mt][1] * rinv, silu_f(gv[2]) * R.o[mt][2] * rinv,
                               silu_f(gv[3]) * R.o[mt][3] * rinv);
                    }
                }
            }
            __syncthreads();  // every wave has read the state
            rt_state_update(L + RT_O_S, L + RT_O_K, L + RT_O_V, L + RT_O_PW + (m - 1), -1, L[RT_O_PW + m], m);
        }
    }
}

template <class T>
__global__ __launch_bounds__(RT_THREADS) void rt_bwd_kernel(RtArgs a) {
    NBSS_LDS(smem);
    float* L = reinterpret_cast<float*>(smem);
    const int tid = threadIdx.x, lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id_u();
    const int Tn = a.T, nch = (Tn + RT_C - 1) / RT_C;
    const float* pw = L + RT_O_PW;
    for (long wi = blockIdx.x; wi < a.BF * RT_HEADS; wi += gridDim.x) {
        const long n = wi / RT_HEADS;
        const int h = (int)(wi % RT_HEADS);
        __syncthreads();
        for (int e = tid; e < 32 * RT_LS; e += RT_THREADS) {
            L[RT_O_S + e] = 0.f;
            L[RT_O_DS + e] = 0.f;
        }
        rt_tables(L, a.decay[h]);
        const T* q = (const T*)a.q + n * Tn * RT_E + h * RT_DK;
        const T* k = a.k ? (const T*)a.k + n * Tn * RT_E + h * RT_DK : q;
        const T* v = (const T*)a.v + n * Tn * RT_VD + h * RT_DV;
        const T* g = (const T*)a.g + n * Tn * RT_VD + h * RT_DV;
        const T* dout = (const T*)a.d_out + n * Tn * RT_VD + h * RT_DV;
        T* dq = (T*)a.dq + n * Tn * RT_E + h * RT_DK;
        T* dk = a.dk ? (T*)a.dk + n * Tn * RT_E + h * RT_DK : nullptr;
        T* dv = (T*)a.dv + n * Tn * RT_VD + h * RT_DV;
        T* dg = (T*)a.dg + n * Tn * RT_VD + h * RT_DV;
        for (int ch = nch - 1; ch >= 0; --ch) {
            const int c0 = ch * RT_C, m = Tn - c0 < RT_C ? Tn - c0 : RT_C, kend = (m + 31) >> 5;
            const bool act = 16 * w < m;  // wave-uniform: some of the wave's queries / keys are frames of the chunk
            const int tok = 16 * w + l15;  // the lane's query, and its key
            __syncthreads();  // dS is updated, the images are free
            rt_stage<T>(L + RT_O_Q, RT_LQ, q + (size_t)c0 * RT_E, RT_E, RT_DK, m, 1.0f);
            rt_stage<T>(L + RT_O_K, RT_LQ, k + (size_t)c0 * RT_E, RT_E, RT_DK, m, a.k ? a.k_scale : 1.0f);
            rt_stage<T>(L + RT_O_V, RT_LV, v + (size_t)c0 * RT_VD, RT_VD, RT_DV, m, 1.0f);
            {
                const float* sv = a.save + ((size_t)wi * nch + ch) * RT_STATE;
                for (int e = tid; e < RT_STATE; e += RT_THREADS) L[RT_O_S + (e / RT_DV) * RT_LS + e % RT_DV] = sv[e];
            }
            __syncthreads();
            // ---- the wave's queries: the forward again, dg, do, dA^T, and the state's part of dq -------------------------------------------------
            RtRows R;
            rt_rows_fwd<T>(R, L, w, m);
            f32x4 dA[4], xq[2];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt) dA[jt] = F32X4_ZERO;
            xq[0] = xq[1] = F32X4_ZERO;
            float* dorow = L + RT_O_DO + tok * RT_LV;
            if (!act) {
#pragma unroll
                for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dorow[16 * mt + 4 * g4 + r] = 0.f;
                if (g4 == 0) L[RT_O_CF + tok] = 0.f;
            } else {
                const float rinv = rt_rms(R);
                f32x4 dhat[3];  // the gradient at the normalised o
                float dot = 0.f;
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) {
                    const size_t off = (size_t)(c0 + tok) * RT_VD + 16 * mt + 4 * g4;
                    float gv[4] = {0.f, 0.f, 0.f, 0.f}, dy[4] = {0.f, 0.f, 0.f, 0.f};
                    if (tok < m) {
                        load4(g + off, gv);
                        load4(dout + off, dy);
                    }
                    float dgv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float oh = R.o[mt][r] * rinv;
                        dgv[r] = dy[r] * oh * dsilu_f(gv[r]);
                        dhat[mt][r] = dy[r] * silu_f(gv[r]);
                        dot += dhat[mt][r] * oh;
                    }
                    if (tok < m) store4(dg + off, dgv[0], dgv[1], dgv[2], dgv[3]);
                }
                dot = wave_sum16(dot) * (1.0f / RT_DV);
#pragma unroll
                for (int mt = 0; mt < 3; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dorow[16 * mt + 4 * g4 + r] = rinv * (dhat[mt][r] - R.o[mt][r] * rinv * dot);
                if (g4 == 0) L[RT_O_CF + tok] = R.cf;
                wave_lds_sync();
                Frag<T> fdo[2], fa;
                rt_frag_rows<T>(fdo[0], L + RT_O_DO, RT_LV, 16 * w, 0, RT_DV);
                rt_frag_rows<T>(fdo[1], L + RT_O_DO, RT_LV, 16 * w, 32, RT_DV);
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    if (jt > w) continue;
                    f32x4 dp = F32X4_ZERO;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        rt_frag_rows<T>(fa, L + RT_O_V, RT_LV, 16 * jt, 32 * ks, RT_DV);
                        dp = mma(fa, fdo[ks], dp);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int d = tok - (16 * jt + 4 * g4 + r);
                        dA[jt][r] = dp[r] * keep_if(d >= 0, pw[d >= 0 ? d : 0] * R.wrow);
                    }
                }
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        rt_frag_rows<T>(fa, L + RT_O_S, RT_LS, 16 * ct, 32 * ks, RT_DV);
                        xq[ct] = mma(fa, fdo[ks], xq[ct]);
                    }
            }
            __syncthreads();  // the P and do images are complete
            // ---- the wave's keys: dv ----------------------------------------------------------------------------------------------------------------
            const float ej = tok < m ? pw[m - 1 - tok] : 0.f;
            if (act) {
                Frag<T> fa, fb;
                f32x4 acc[3];
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) acc[mt] = F32X4_ZERO;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if (ks < (w >> 1) || ks >= kend) continue;  // queries before every key of the wave, or behind the chunk
                    rt_frag_cols<T>(fb, L + RT_O_P, RT_LP, 16 * w, RT_C, 32 * ks, RT_C);
#pragma unroll
                    for (int mt = 0; mt < 3; ++mt) {
                        rt_frag_cols<T>(fa, L + RT_O_DO, RT_LV, 16 * mt, RT_DV, 32 * ks, RT_C);
                        acc[mt] = mma(fa, fb, acc[mt]);
                    }
                }
                rt_frag_rows<T>(fb, L + RT_O_K, RT_LQ, 16 * w, 0, RT_DK);
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) {
                    rt_frag_cols<T>(fa, L + RT_O_DS, RT_LS, 16 * mt, RT_DV, 0, RT_DK);
                    const f32x4 xv = mma(fa, fb, F32X4_ZERO);
                    if (tok < m)
                        store4(dv + (size_t)(c0 + tok) * RT_VD + 16 * mt + 4 * g4, acc[mt][0] + xv[0] * ej, acc[mt][1] + xv[1] * ej, acc[mt][2] + xv[2] * ej,
                               acc[mt][3] + xv[3] * ej);
                }
            }
            __syncthreads();  // P is consumed: the image takes dA
            {
                float* prow = L + RT_O_P + tok * RT_LP;
#pragma unroll
                for (int jt = 0; jt < 4; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) prow[16 * jt + 4 * g4 + r] = dA[jt][r];
            }
            __syncthreads();
            // ---- dq of the wave's queries, dk' of its keys (the same lanes and registers: 'share_qk' adds them) -----------------------------------------
            if (act) {
                Frag<T> fa, fb;
                f32x4 aq[2], ak[2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    aq[ct] = F32X4_ZERO;
                    ak[ct] = F32X4_ZERO;
                }
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if (ks >= kend) continue;
                    if (ks <= (w >> 1)) {  // keys up to the wave's queries
                        rt_frag_rows<T>(fb, L + RT_O_P, RT_LP, 16 * w, 32 * ks, RT_C);
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) {
                            rt_frag_cols<T>(fa, L + RT_O_K, RT_LQ, 16 * ct, RT_DK, 32 * ks, RT_C);
                            aq[ct] = mma(fa, fb, aq[ct]);
                        }
                    }
                    if (ks >= (w >> 1)) {  // queries from the wave's keys on
                        rt_frag_cols<T>(fb, L + RT_O_P, RT_LP, 16 * w, RT_C, 32 * ks, RT_C);
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct) {
                            rt_frag_cols<T>(fa, L + RT_O_Q, RT_LQ, 16 * ct, RT_DK, 32 * ks, RT_C);
                            ak[ct] = mma(fa, fb, ak[ct]);
                        }
                    }
                }
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    f32x4 xk = F32X4_ZERO;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        rt_frag_rows<T>(fa, L + RT_O_DS, RT_LS, 16 * ct, 32 * ks, RT_DV);
                        rt_frag_rows<T>(fb, L + RT_O_V, RT_LV, 16 * w, 32 * ks, RT_DV);
                        xk = mma(fa, fb, xk);
                    }
                    const int c = 16 * ct + 4 * g4;
                    if (tok < m && c < RT_DK) {
                        const size_t off = (size_t)(c0 + tok) * RT_E + c;
                        float vq[4], vk[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            vq[r] = aq[ct][r] + xq[ct][r] * R.cf;
                            vk[r] = ak[ct][r] + xk[r] * ej;
                        }
                        if (dk) {
                            store4(dq + off, vq[0], vq[1], vq[2], vq[3]);
                            store4(dk + off, vk[0] * a.k_scale, vk[1] * a.k_scale, vk[2] * a.k_scale, vk[3] * a.k_scale);
                        } else {
                            store4(dq + off, vq[0] + vk[0], vq[1] + vk[1], vq[2] + vk[2], vq[3] + vk[3]);
                        }
                    }
                }
            }
            __syncthreads();  // every wave has read dS
            rt_state_update(L + RT_O_DS, L + RT_O_Q, L + RT_O_DO, L + RT_O_CF, 1, pw[m], m);
        }
    }
}

static int rt_grid(int64_t BF) {
    const int64_t n = BF * RT_HEADS;
    return (int)(n < RT_GRID_CAP ? n : RT_GRID_CAP);
}

template <class T>
static int rt_fwd(const RtArgs& a, hipStream_t st) {
    const size_t lds = RT_FWD_FLOATS * sizeof(float);
    NBSS_LAUNCH((rt_fwd_kernel<T>), dim3(rt_grid(a.BF)), dim3(RT_THREADS), lds, st, a);
    return NBSS_CHECK_LAUNCH();
}
template <class T>
static int rt_bwd(const RtArgs& a, hipStream_t st) {
    const size_t lds = RT_BWD_FLOATS * sizeof(float);
    const int e = NBSS_SET_MAX_LDS((rt_bwd_kernel<T>), lds);
    if (e) return e;
    NBSS_LAUNCH((rt_bwd_kernel<T>), dim3(rt_grid(a.BF)), dim3(RT_THREADS), lds, st, a);
    return NBSS_CHECK_LAUNCH();
}

extern "C" {

int64_t nbss_online_ret_train_save_bytes(int dtype, int64_t BF, int T) {
    const int e = rt_check(dtype, BF, T);
    return e ? e : (int64_t)ws_align((size_t)BF * RT_HEADS * rt_chunks(T) * RT_STATE * sizeof(float));
}
int64_t nbss_online_ret_train_ws_bytes(int dtype, int64_t BF, int T) {
    const int e = rt_check(dtype, BF, T);
    return e ? e : (int64_t)ws_align(1);
}

int nbss_online_ret_train_fwd(int dtype, int64_t BF, int T, const void* q, const void* k, const void* v, const void* g, float k_scale, const float* decay,
                              void* out, void* save, void* ws, void* stream) {
    const int e = rt_check(dtype, BF, T);
    if (e) return e;
    if (!q || !v || !g || !decay || !out || !ws || out == q || out == k || out == v || out == g) return NBSS_EINVAL;
    RtArgs a = {q, k, v, g, nullptr, out, nullptr, nullptr, nullptr, nullptr, (float*)save, decay, k_scale, (long)BF, T};
    return dtype == NBSS_BF16 ? rt_fwd<bf16_t>(a, (hipStream_t)stream) : rt_fwd<float>(a, (hipStream_t)stream);
}

int nbss_online_ret_train_bwd(int dtype, int64_t BF, int T, const void* q, const void* k, const void* v, const void* g, float k_scale, const float* decay,
                              const void* save, const void* d_out, void* dq, void* dk, void* dv, void* dg, void* ws, void* stream) {
    const int e = rt_check(dtype, BF, T);
    if (e) return e;
    if (!q || !v || !g || !decay || !save || !d_out || !dq || !dv || !dg || !ws || (k == nullptr) != (dk == nullptr)) return NBSS_EINVAL;
    RtArgs a = {q, k, v, g, d_out, nullptr, dq, dk, dv, dg, (float*)save, decay, k_scale, (long)BF, T};
    return dtype == NBSS_BF16 ? rt_bwd<bf16_t>(a, (hipStream_t)stream) : rt_bwd<float>(a, (hipStream_t)stream);
}

}  // extern "C"
