// attn_relpos_kb.hip — the relative-position attention of NBC (attn_relpos.hip: score(i, j) = ((q_i + u) . k_j + (q_i + v) . P[i - j + T - 1]) scale) on
// sequences longer than a head's K / V / P fit in LDS: forward only (inference on whole utterances, nbss_nb_attention_relpos_long_fwd), any T <= 4096.
//
// One workgroup per (sequence, head, 64 queries), one 16-query tile per wave with its (q + u) and (q + v) fragments in registers; the keys are walked in
// blocks of 64 as in attn_kb.hip (running max / running sum per query, O rescaled per block).  Per key block the workgroup stages K, V and the rows of P
// the block's offsets need: i - j for the 64 queries x 64 keys are the 127 consecutive rows from (q0 - j0 - 63) + T - 1 on (a 128th row completes the last
// 32-row tile pair; its offset + 64 lies on no diagonal); rows outside the table [0, 2T - 2] are staged as zeros — they belong to masked keys or to queries
// >= T.  The position term of a 16 x 16 tile is the whole-head kernel's: two MFMA tiles M[r'][i] = P[rb + r'] . (q_i + v) through 2 KB of wave-private
// LDS, read back along the diagonal r' = i - j + 15.
// LDS: 256 rows x (DH + 16 bytes of padding) + the head's u | v + 4 x 2 KB: 61.8 KB in fp32 at DH = 48 (two workgroups per CU), 25 KB in bf16 at DH = 24.
// The 256 rows are 256 x PR 16-byte pieces, PR per thread: all of a block's global reads are issued before its LDS stores, none of them inside a branch
// (addresses are clamped into the tensors, the values of rows outside replaced by zeros) — this kernel's own staging, not at_stage.  Of attn_tiles.h it
// uses the transposed fragments (at_frag_t) and the dispatch; its K-step loop, softmax steps and store stay inline: on the shared helpers the width-48
// instances measured 2 % slower (profiles/README.md).  Every output element has one writer, no atomics.
#include "kb.h"
#include "attn_tiles.h"
#include "layout.h"
#include "nb.h"

#define RK_PROWS 128  // staged rows of P per (query block, key block)

template <class T, int DH>
__global__ __launch_bounds__(KB_THREADS) void kb_attn_relpos_kernel(const T* __restrict__ qkv, const T* __restrict__ pos, const float* __restrict__ ub,
                                                                    const float* __restrict__ vb, T* __restrict__ O, float scale, int Tn, int H, int heads) {
    constexpr int KS = (DH + 31) / 32, MTD = (DH + 15) / 16, VE = 16 / sizeof(T), PR = DH / VE, LD = DH + VE, JT = KB_BLK / 16;
    constexpr int ROWS = 2 * KB_BLK + RK_PROWS;  // K | V | P rows of a block: ROWS x PR pieces = PR per thread
    static_assert(ROWS == KB_THREADS && DH % 8 == 0, "one row piece column per thread and step");
    NBSS_LDS(smem);
    T* Ks = reinterpret_cast<T*>(smem);     // [KB_BLK][LD]
    T* Vs = Ks + (size_t)KB_BLK * LD;       // [KB_BLK][LD]
    T* Ps = Vs + (size_t)KB_BLK * LD;       // [RK_PROWS][LD]: local row lr <-> table row (q0 - j0 - 63 + Tn - 1) + lr
    float* bs = reinterpret_cast<float*>(Ps + (size_t)RK_PROWS * LD);  // [2][DH]: the head's u | v
    const int seq = blockIdx.x, head = blockIdx.y, q0 = (int)blockIdx.z * KB_BLK;
    const int lane = lane_id(), l15 = lane & 15, g4 = lane >> 4, w = wave_id_u();
    float* Mb = bs + 2 * DH + w * 32 * 16;  // [32 offsets][16 queries] per wave
    const size_t n0 = (size_t)seq * Tn;
    const int ld = 3 * H, NB = cdiv(Tn, KB_BLK), NR = 2 * Tn - 1;
    const T* kbase = qkv + n0 * ld + H + head * DH;
    const T* vbase = qkv + n0 * ld + 2 * H + head * DH;
    const T* pbase = pos + head * DH;
    const bool wave_on = q0 + 16 * w < Tn;  // (wave-uniform) a tile past the end only helps staging
    const int q = q0 + 16 * w + l15;
    const bool qv = q < Tn;
    const size_t nq = n0 + (qv ? q : 0);
    // the lane's q pieces (clamped addresses, selected below) and the head's biases through LDS
    float qraw[KS][8];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int d0 = 32 * ks + 8 * g4;
        load8(qkv + nq * ld + head * DH + (d0 < DH ? d0 : 0), qraw[ks]);
    }
    if (threadIdx.x < 2 * DH) bs[threadIdx.x] = threadIdx.x < DH ? ub[head * DH + threadIdx.x] : vb[head * DH + threadIdx.x - DH];
    Frag<T> qc[KS], qp[KS];
    float m = -3.0e38f, l = 0.f;
    f32x4 oacc[MTD];
#pragma unroll
    for (int mt = 0; mt < MTD; ++mt) oacc[mt] = F32X4_ZERO;
    for (int b = 0; b < NB; ++b) {
        const int j0 = b * KB_BLK, pr0 = q0 - j0 - (KB_BLK - 1) + Tn - 1;
        if (b) lds_barrier();
        {
            u32x4 piece[PR];
#pragma unroll
            for (int i = 0; i < PR; ++i) {
                const int e = (int)threadIdx.x + KB_THREADS * i, r = e / PR, pc = e % PR;
                const int kr = j0 + (r & (KB_BLK - 1)), prow = pr0 + r - 2 * KB_BLK;
                const bool isp = r >= 2 * KB_BLK;
                const bool ok = isp ? (prow >= 0 && prow < NR) : kr < Tn;
                const T* src = isp ? pbase + (size_t)(ok ? prow : 0) * H : (r < KB_BLK ? kbase : vbase) + (size_t)(ok ? kr : 0) * ld;
                piece[i] = *reinterpret_cast<const u32x4*>(src + pc * VE);
                if (!ok) piece[i] = (u32x4){0u, 0u, 0u, 0u};
            }
#pragma unroll
            for (int i = 0; i < PR; ++i) {
                const int e = (int)threadIdx.x + KB_THREADS * i, r = e / PR, pc = e % PR;
                *reinterpret_cast<u32x4*>(Ks + (size_t)r * LD + pc * VE) = piece[i];  // (K, V and P images are contiguous: row r of the three)
            }
        }
        __syncthreads();
        if (b == 0) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int d0 = 32 * ks + 8 * g4, dc = d0 < DH ? d0 : 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    frag_set(qc[ks], j, keep_if(qv && d0 < DH, qraw[ks][j] + bs[dc + j]));
                    frag_set(qp[ks], j, keep_if(qv && d0 < DH, qraw[ks][j] + bs[DH + dc + j]));
                }
            }
        }
        if (!wave_on) continue;
        // S^T tiles: rows = keys j0 + 16 jt + 4 g4 + r, column = the lane's query
        f32x4 st[JT];
        float bm = -3.0e38f;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            st[jt] = F32X4_ZERO;
            const int rl = 16 * w - 16 * jt + (KB_BLK - 16);  // local P row of the tile pair's offset r' = 0 (i - j = -15)
            f32x4 m0 = F32X4_ZERO, m1 = F32X4_ZERO;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int d0 = 32 * ks + 8 * g4;
                Frag<T> kf, p0, p1;
                frag_zero(kf); frag_zero(p0); frag_zero(p1);
                if (d0 < DH) {
                    frag_load(kf, Ks + (size_t)(16 * jt + l15) * LD + d0);
                    frag_load(p0, Ps + (size_t)(rl + l15) * LD + d0);
                    frag_load(p1, Ps + (size_t)(rl + 16 + l15) * LD + d0);
                }
                st[jt] = mma(kf, qc[ks], st[jt]);
                m0 = mma(p0, qp[ks], m0);
                m1 = mma(p1, qp[ks], m1);
            }
            wave_lds_sync();  // (the previous tile's reads of Mb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Mb[(4 * g4 + r) * 16 + l15] = m0[r];
                Mb[(16 + 4 * g4 + r) * 16 + l15] = m1[r];
            }
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool kv = j0 + 16 * jt + 4 * g4 + r < Tn;
                const float pt = Mb[(l15 - (4 * g4 + r) + 15) * 16 + l15];
                st[jt][r] = kv ? (st[jt][r] + pt) * scale : -3.0e38f;
                bm = fmaxf(bm, st[jt][r]);
            }
        }
        const float mn = fmaxf(m, wave_max16(bm));  // (every block holds at least one valid key: finite from the first block on)
        const float alpha = __expf(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool kv = j0 + 16 * jt + 4 * g4 + r < Tn;
                st[jt][r] = kv ? __expf(st[jt][r] - mn) : 0.f;
                ps += st[jt][r];
            }
        l = l * alpha + wave_sum16(ps);
        m = mn;
#pragma unroll
        for (int mt = 0; mt < MTD; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[mt][r] *= alpha;
#pragma unroll
        for (int kk = 0; kk < JT / 2; ++kk) {
            Frag<T> pf;
            frag_from_c2(pf, st[2 * kk], st[2 * kk + 1]);
#pragma unroll
            for (int mt = 0; mt < MTD; ++mt) {
                Frag<T> vt;
                at_frag_t<T, DH, LD>(vt, Vs, 32 * kk, mt);
                oacc[mt] = mma(vt, pf, oacc[mt]);
            }
        }
    }
    if (wave_on && qv) {
        const float inv = 1.0f / l;
#pragma unroll
        for (int mt = 0; mt < MTD; ++mt) {
            const int d = 16 * mt + 4 * g4;
            if (DH % 16 == 0 || d < DH) store4(O + nq * H + head * DH + d, oacc[mt][0] * inv, oacc[mt][1] * inv, oacc[mt][2] * inv, oacc[mt][3] * inv);
        }
    }
}

template <class T, int DH>
static int kb_attn_relpos(long nseq, int Tn, int H, int heads, const void* qkv, const void* pos, const float* ub, const float* vb, float scale, void* o, hipStream_t st) {
    const size_t lds = (size_t)(2 * KB_BLK + RK_PROWS) * (DH + 16 / sizeof(T)) * sizeof(T) + (size_t)2 * DH * sizeof(float) +
                       (size_t)(KB_THREADS / 64) * 32 * 16 * sizeof(float);
    NBSS_LAUNCH((kb_attn_relpos_kernel<T, DH>), dim3((unsigned)nseq, heads, cdiv(Tn, KB_BLK)), dim3(KB_THREADS), lds, st, (const T*)qkv, (const T*)pos, ub, vb, (T*)o, scale,
                Tn, H, heads);
    return NBSS_CHECK_LAUNCH();
}
int nb_attention_relpos_long_fwd_impl(int dtype, long nseq, int Tn, int H, int heads, const void* qkv, const void* pos, const float* ub, const float* vb, float scale,
                                      void* o, hipStream_t st) {
    if (heads <= 0 || H % heads) return NBSS_EINVAL;
    if (Tn > KB_TLONG || heads > 65535) return NBSS_EUNSUPPORTED;
    const int dh = H / heads;
    return AT_DISPATCH_NARROW(dtype, dh, kb_attn_relpos, nseq, Tn, H, heads, qkv, pos, ub, vb, scale, o, st);
}
