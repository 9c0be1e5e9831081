// rir.hip — room impulse responses by the image-source method (Allen & Berkley 1979) with the Hann-windowed sinc of fractional delay that the
// gpuRIR paper describes (Diaz-Guerra, Miguel, Beltran 2021), and this project's own diffuse tail.  The definition is the one of include/nbss_hip.h.
//
//   rir_table_kernel  one workgroup per room: the room's image counts and, per axis and image index i (n = i - N/2), the wall factor
//                     beta_a0^r0(n) beta_a1^r1(n) in fp64 (a running product: 0^0 = 1) into the workspace.
//   rir_ism_kernel    one workgroup per (room, source, receiver, tile of 256 samples).  Passes of two phases until every image is consumed:
//                       A  thread t walks the (nx, ny) pairs t, t + 256, ... ; for a pair it bounds the image indices nz whose delay can reach the tile
//                          (two index ranges, below and above the receiver), evaluates those candidates in fp64 (position, distance, delay x, the split
//                          x = xi + xf with |xf| <= 1/2) and puts up to RIR_SLOTS accepted images into its own segment of the LDS list: amplitude,
//                          xi, xf, A sin(pi xf) / pi and the Hann half-phase (cos, sin)(pi x / (Tw fs)).  A thread resumes where it stopped.
//                       B  thread t owns sample t of the tile and walks the segments in thread order, slot order: per (image, sample) a sign from the
//                          parity of k - xi, one angle addition against the thread's own (cos, sin)(pi k / (Tw fs)), one reciprocal; no transcendental.
//                     The order of the sum is fixed by the room, the pair (source, receiver) and the tile alone: two launches give the same bits, and a
//                     room's response does not depend on the rooms it shares a launch with.  The terms are fp32, the accumulator is fp64 (one rounding
//                     at the store).  Every output element is stored exactly once, by its own thread; no atomics.
//                     The cut-off x_max is per room: the host's k_d[b] travel by value in the kernel's arguments (RirRoomCuts, RIR_ROOMS_PER_LAUNCH
//                     rooms per launch; more rooms take more launches), so nothing is written to memory for them and the workspace keeps its
//                     layout.  The scalar entry points (nbss_rir_ism, nbss_rir_tail) are the same launches with every cut equal.
//   rir_tail_kernel   one workgroup per (room, source, receiver): g^2 = mean of the K samples before k_d (fp64, fixed order), then for k >= k_d
//                     g 10^(-3 (k - k_d) / (fs RT60)) xi(seed, b, s, m, k) with xi a Box-Muller Gaussian from a splitmix64 counter hash, all in fp64.
//                     k_d per room from RirRoomCuts; the workgroups of a room with k_d = 0 return at once.
//
// hann(u) sinc(u) with u = k - x:  0.5 (1 + cos(2 pi u / T)) = cos^2(pi u / T) (no cancellation at the window's ends) and
// sin(pi u) = -(-1)^(k - xi) sin(pi xf).  With |xf| <= 1/2 the fp32 u = (k - xi) - xf is exact for k = xi and good to half an ulp elsewhere.
// Built without -ffast-math (nbss_amd/build.py): accurate sinf / cosf, no reassociation.
#include "launch.h"
#include "layout.h"

#define RIR_TILE 256
#define RIR_SLOTS 8                       // list capacity per pass: RIR_TILE * RIR_SLOTS = 2048 images (tests/test_rir_kernels.py overflows it)
#define RIR_MAX_IMG 512
#define RIR_MAX_SAMPLES 65536
#define RIR_MAX_WIN 256                   // Tw fs + 1 <= 257
#define RIR_PI 3.14159265358979323846
#define RIR_MIN_DIST 1e-3
#define RIR_ROOMS_PER_LAUNCH 256          // per-room k_d of one launch: 1 KB of kernel arguments (tests/test_rir_rooms_kernels.py passes it)

struct RirRoomCuts {  // k_d of the rooms room0 .. room0 + RIR_ROOMS_PER_LAUNCH - 1 of a launch, passed by value
    int32_t v[RIR_ROOMS_PER_LAUNCH];
};

struct alignas(8) RirEntry {  // 24 bytes; phase B reads them with every lane at the same address (broadcast, no bank conflict)
    float A, q, xf, cphi, sphi;
    int xi;
};

// ws: int32 hdr[B][4] = Nx, Ny, Nz, first table element | double table[sum_b (Nx + Ny + Nz)]
static size_t rir_ws_bytes_host(int B, const int32_t* nb) {
    size_t n = 0;
    for (int i = 0; i < 3 * B; ++i) n += (size_t)nb[i];
    return (size_t)B * 16 + n * sizeof(double);
}

NBSS_DEV double rir_wall_factor(double b0, double b1, int n) {
    const int a = n < 0 ? -n : n;
    const int r0 = n >= 0 ? a / 2 : (a + 1) / 2, r1 = n >= 0 ? (a + 1) / 2 : a / 2;
    double f = 1.0;
    for (int i = 0; i < r0; ++i) f *= b0;  // at most 256 factors; 0^0 = 1 by construction
    for (int i = 0; i < r1; ++i) f *= b1;
    return f;
}

__global__ __launch_bounds__(256) void rir_table_kernel(int room, int Nx, int Ny, int Nz, int first, const double* __restrict__ beta, int32_t* __restrict__ hdr,
                                                        double* __restrict__ table) {
    const int N[3] = {Nx, Ny, Nz};
    if (threadIdx.x == 0) {
        hdr[room * 4 + 0] = Nx;
        hdr[room * 4 + 1] = Ny;
        hdr[room * 4 + 2] = Nz;
        hdr[room * 4 + 3] = first;
    }
    int off = first;
    for (int a = 0; a < 3; ++a) {
        const double b0 = beta[room * 6 + 2 * a], b1 = beta[room * 6 + 2 * a + 1];
        for (int i = (int)threadIdx.x; i < N[a]; i += (int)blockDim.x) table[off + i] = rir_wall_factor(b0, b1, i - N[a] / 2);
        off += N[a];
    }
}

NBSS_DEV double rir_image_coord(int n, double L, double s) { return (n & 1) ? (double)(n + 1) * L - s : (double)n * L + s; }

// index range [lo, hi] (clipped to [0, N - 1], possibly empty) of the images whose coordinate lies in [za, zb]: the coordinate of image n is
// in [n L, (n + 1) L] and grows with n, so n in [za / L - 1, zb / L]; one more on either side for the rounding of the bounds
NBSS_DEV void rir_index_range(double za, double zb, double L, int N, int& lo, int& hi) {
    const double half = (double)(N / 2);
    double a = floor(za / L) - 2.0 + half, b = floor(zb / L) + 1.0 + half;
    a = a < 0.0 ? 0.0 : a;
    b = b > (double)(N - 1) ? (double)(N - 1) : b;
    if (!(a <= b)) {
        lo = 1;
        hi = 0;
        return;
    }
    lo = (int)a;
    hi = (int)b;
}

// the workgroup of (room, source s, receiver m, tile blockIdx.x); x_max: only images with x < x_max are admitted
NBSS_DEV void rir_ism_body(int room, int s, int m, int S, int M, int n_samples, double fs_over_c, double Tk, double x_max,
                           const double* __restrict__ room_sz, const double* __restrict__ pos_src, const double* __restrict__ pos_rcv,
                           const int32_t* __restrict__ hdr, const double* __restrict__ table, float* __restrict__ h) {
    NBSS_LDS(smem);
    RirEntry* list = reinterpret_cast<RirEntry*>(smem);                       // [RIR_TILE][RIR_SLOTS]
    int* cnt = reinterpret_cast<int*>(smem + sizeof(RirEntry) * RIR_TILE * RIR_SLOTS);  // [RIR_TILE]
    int* flag = cnt + RIR_TILE;                                               // [2]
    const int tid = (int)threadIdx.x;
    const int t0 = (int)blockIdx.x * RIR_TILE, k = t0 + tid;
    float* out = h + (((size_t)room * S + s) * M + m) * (size_t)n_samples;
    const double half = 0.5 * Tk;
    if ((double)t0 >= x_max + half) {  // no admitted image reaches this tile (only with a diffuse tail)
        if (k < n_samples) out[k] = 0.f;
        return;
    }
    const int Nx = hdr[room * 4 + 0], Ny = hdr[room * 4 + 1], Nz = hdr[room * 4 + 2];
    const double* tx = table + hdr[room * 4 + 3];
    const double* ty = tx + Nx;
    const double* tz = ty + Ny;
    const double Lx = room_sz[room * 3 + 0], Ly = room_sz[room * 3 + 1], Lz = room_sz[room * 3 + 2];
    const double* ps = pos_src + ((size_t)room * S + s) * 3;
    const double* pr = pos_rcv + ((size_t)room * M + m) * 3;
    const double sx = ps[0], sy = ps[1], sz = ps[2], rx = pr[0], ry = pr[1], rz = pr[2];
    // delays that can touch the tile: t0 - half < x < t1 - 1 + half; one sample of slack, phase B applies the window itself
    const double xlo = (double)t0 - half - 1.0, xhi_tile = (double)(t0 + RIR_TILE) + half;
    const double xhi = xhi_tile < x_max ? xhi_tile : x_max;  // admitted: x < x_max (strict, checked per image)
    const double dlo = xlo > 0.0 ? xlo / fs_over_c : 0.0, dhi = xhi_tile / fs_over_c;
    // this thread's sample: the Hann half-phase pi k / Tk, reduced in fp64
    const double kk = (double)k;
    const float thk = (float)(RIR_PI * (kk - 2.0 * Tk * floor(kk / (2.0 * Tk))) / Tk);
    const float ck = cosf(thk), sk = sinf(thk);
    const float halff = (float)half;
    double acc = 0.0;

    if (tid == 0) flag[0] = 0, flag[1] = 0;
    __syncthreads();
    const int NP = Nx * Ny;
    int p = tid;  // next pair of this thread
    bool have = false;
    int iz = 0, r1hi = -1, r2lo = 0, r2hi = -1;
    double r2 = 0.0, Axy = 0.0;
    for (int it = 0;; ++it) {
        // ---- phase A
        int c = 0;
        while (c < RIR_SLOTS) {
            if (!have) {
                if (p >= NP) break;
                const int ix = p / Ny, iy = p - ix * Ny;
                p += RIR_TILE;
                Axy = tx[ix] * ty[iy];
                if (Axy == 0.0) continue;  // every image of the pair is silent
                const double dx = rir_image_coord(ix - Nx / 2, Lx, sx) - rx, dy = rir_image_coord(iy - Ny / 2, Ly, sy) - ry;
                r2 = dx * dx + dy * dy;
                const double dh2 = dhi * dhi * (1.0 + 1e-12) - r2;
                if (dh2 < 0.0) continue;
                const double zhi = sqrt(dh2);
                const double dl2 = dlo * dlo * (1.0 - 1e-12) - r2;
                const double zlo = dl2 > 0.0 ? sqrt(dl2) : 0.0;
                int a0, a1, b0, b1;
                rir_index_range(rz - zhi, rz - zlo, Lz, Nz, a0, a1);
                rir_index_range(rz + zlo, rz + zhi, Lz, Nz, b0, b1);
                if (a0 > a1) a0 = b0, a1 = b0 - 1;           // lower range empty
                if (b0 > b1) b0 = a1 + 1, b1 = a1;           // upper range empty
                if (b0 <= a1 + 1) {                          // the ranges meet: one range
                    a1 = a1 > b1 ? a1 : b1;
                    b0 = a1 + 1;
                    b1 = a1;
                }
                iz = a0, r1hi = a1, r2lo = b0, r2hi = b1;
                have = true;
            }
            if (iz > r1hi && iz < r2lo) iz = r2lo;
            if (iz > r2hi && iz > r1hi) {
                have = false;
                continue;
            }
            const int i = iz++;
            const double Az = tz[i];
            if (Az == 0.0) continue;
            const double dz = rir_image_coord(i - Nz / 2, Lz, sz) - rz;
            double d = sqrt(r2 + dz * dz);
            d = d < RIR_MIN_DIST ? RIR_MIN_DIST : d;
            const double x = d * fs_over_c;
            if (!(x > xlo && x < xhi)) continue;
            const double A = Axy * Az / (4.0 * RIR_PI * d);
            const double xr = rint(x), xf = x - xr;  // |xf| <= 1/2, exact
            const float sn = sinf((float)(RIR_PI * xf));
            const float ph = (float)(RIR_PI * (x - 2.0 * Tk * floor(x / (2.0 * Tk))) / Tk);
            RirEntry e;
            e.A = (float)A;
            e.q = (float)(A * (double)sn / RIR_PI);
            e.xf = (float)xf;
            e.cphi = cosf(ph);
            e.sphi = sinf(ph);
            e.xi = (int)xr;
            list[tid * RIR_SLOTS + c++] = e;
        }
        cnt[tid] = c;
        if (have || p < NP) flag[it & 1] = 1;
        if (tid == 0) flag[(it + 1) & 1] = 0;
        __syncthreads();
        // ---- phase B
        for (int t = 0; t < RIR_TILE; ++t) {
            const int n = cnt[t];
            for (int j = 0; j < n; ++j) {
                const RirEntry e = list[t * RIR_SLOTS + j];
                const int dk = k - e.xi;
                const float u = (float)dk - e.xf;
                if (fabsf(u) < halff) {
                    const float cw = ck * e.cphi + sk * e.sphi;  // cos(pi (k - x) / Tk)
                    const float sg = (dk & 1) ? e.q : -e.q;
                    const float sc = u == 0.f ? e.A : sg * fast_rcp(u);
                    acc += (double)(cw * cw * sc);
                }
            }
        }
        const int more = flag[it & 1];
        __syncthreads();
        if (!more) break;
    }
    if (k < n_samples) out[k] = (float)acc;
}

// rooms room0 + blockIdx.z; half_K = round(Tk) / 2: room b admits x < k_d[b] + half_K, every image when k_d[b] = 0
__global__ __launch_bounds__(RIR_TILE) void rir_ism_kernel(int S, int M, int n_samples, double fs_over_c, double Tk, double half_K, int room0, RirRoomCuts cuts,
                                                           const double* __restrict__ room_sz, const double* __restrict__ pos_src,
                                                           const double* __restrict__ pos_rcv, const int32_t* __restrict__ hdr,
                                                           const double* __restrict__ table, float* __restrict__ h) {
    const int k_d = cuts.v[blockIdx.z];
    const double x_max = k_d > 0 ? (double)k_d + half_K : 1e300;
    rir_ism_body(room0 + (int)blockIdx.z, (int)blockIdx.y / M, (int)blockIdx.y % M, S, M, n_samples, fs_over_c, Tk, x_max, room_sz, pos_src, pos_rcv, hdr, table,
                 h);
}

// ---------------- diffuse tail ----------------
NBSS_DEV uint64_t rir_mix64(uint64_t z) {  // splitmix64 step
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// unit Gaussian of the counter (seed, b, s, m, k): u1 in (0, 1] from 23 bits, u2 in [0, 1) from 24 bits, Box-Muller
NBSS_DEV double rir_gauss(uint64_t key_bsm, int k) {
    const uint64_t h1 = rir_mix64(key_bsm + (uint64_t)k), h2 = rir_mix64(h1);
    const double u1 = (double)((h1 >> 41) + 1) * (1.0 / 8388608.0), u2 = (double)(h2 >> 40) * (1.0 / 16777216.0);
    return sqrt(-2.0 * log(u1)) * cos(2.0 * RIR_PI * u2);
}

// grid (S M, rooms of the launch): the workgroup of row (room0 + blockIdx.y, s, m) of h with the room's own k_d; k_d = 0 leaves the room as it is
// (uniform per workgroup: no barrier is skipped)
__global__ __launch_bounds__(256) void rir_tail_kernel(int S, int M, int n_samples, int K, int room0, RirRoomCuts cuts, double fs, uint64_t seed,
                                                       const double* __restrict__ rt60, float* __restrict__ h) {
    const int k_d = cuts.v[blockIdx.y];
    if (k_d == 0) return;
    const int room = room0 + (int)blockIdx.y, s = (int)blockIdx.x / M, m = (int)blockIdx.x % M;
    float* row = h + ((size_t)room * (size_t)(S * M) + (size_t)blockIdx.x) * (size_t)n_samples;
    NBSS_LDS(smem);
    double* sq = reinterpret_cast<double*>(smem);  // [K]
    double* gs = sq + RIR_MAX_WIN;                 // [1]
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < K; i += (int)blockDim.x) {
        const double v = (double)row[k_d - K + i];
        sq[i] = v * v;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int i = 0; i < K; ++i) a += sq[i];  // K <= 256 terms in index order
        gs[0] = sqrt(a / (double)K);
    }
    __syncthreads();
    const double g = gs[0], rate = 3.0 * 2.302585092994045684 / (fs * rt60[room]);
    const uint64_t key = rir_mix64(rir_mix64(rir_mix64(seed + (uint64_t)room) + (uint64_t)s) + (uint64_t)m);
    for (int kq = k_d + tid; kq < n_samples; kq += (int)blockDim.x)
        row[kq] = (float)(g * exp(-rate * (double)(kq - k_d)) * rir_gauss(key, kq));
}

// ---------------- host side ----------------
static int rir_check_common(int B, int S, int M, int n_samples, double fs, double tw) {
    if (!(fs > 0.0) || !(tw > 0.0)) return NBSS_EINVAL;
    if (B < 1 || S < 1 || M < 1 || n_samples < 1 || n_samples > RIR_MAX_SAMPLES || B > 65535 || (int64_t)S * M > 65535) return NBSS_EUNSUPPORTED;
    if (tw * fs > (double)RIR_MAX_WIN + 1e-6 || tw * fs < 2.0) return NBSS_EUNSUPPORTED;  // Tw fs + 1 <= 257, up to the rounding of the product
    return 0;
}

// The cuts of a call: one k_d per room, or with `broadcast` one for every room (the scalar entry points).  A negative cut is NBSS_EINVAL, a tail
// start outside [K, n_samples) NBSS_EUNSUPPORTED; k_d = 0 is "no tail" except with need_tail (nbss_rir_tail), where every cut must be a tail start.
static int rir_check_cuts(int B, int n_samples, double fs, double tw, const int32_t* k_d, bool broadcast, bool need_tail) {
    const int nk = broadcast ? 1 : B, K = (int)llrint(tw * fs);
    for (int b = 0; b < nk && !need_tail; ++b)
        if (k_d[b] < 0) return NBSS_EINVAL;
    for (int b = 0; b < nk; ++b)
        if ((need_tail || k_d[b] > 0) && (k_d[b] < K || k_d[b] >= n_samples)) return NBSS_EUNSUPPORTED;
    return 0;
}

// launch(room0, rooms, cuts, any room with a tail) -> return code, once per RIR_ROOMS_PER_LAUNCH rooms
template <class F>
static int rir_for_launches(int B, const int32_t* k_d, bool broadcast, F launch) {
    for (int room0 = 0; room0 < B; room0 += RIR_ROOMS_PER_LAUNCH) {
        const int nr = B - room0 < RIR_ROOMS_PER_LAUNCH ? B - room0 : RIR_ROOMS_PER_LAUNCH;
        RirRoomCuts cuts = {};
        bool any = false;
        for (int i = 0; i < nr; ++i) any |= (cuts.v[i] = k_d[broadcast ? 0 : room0 + i]) > 0;
        const int e = launch(room0, nr, cuts, any);
        if (e) return e;
    }
    return 0;
}

int64_t rir_ism_ws_bytes_impl(int B, const int32_t* nb_img) {
    for (int i = 0; i < 3 * B; ++i)
        if (nb_img[i] < 1 || nb_img[i] > RIR_MAX_IMG) return NBSS_EUNSUPPORTED;
    return (int64_t)rir_ws_bytes_host(B, nb_img);
}

// nbss_rir_ism (broadcast: k_d points at its one cut) and nbss_rir_ism_rooms: the checks, the wall-factor tables of every room into ws, the launches
int rir_ism_impl(int B, int S, int M, int n_samples, double fs, double c, double tw, const int32_t* k_d, bool broadcast, const double* room_sz,
                 const double* beta, const double* pos_src, const double* pos_rcv, const int32_t* nb_img, float* h, void* ws, int64_t ws_bytes, hipStream_t st) {
    int e = rir_check_common(B, S, M, n_samples, fs, tw);
    if (e) return e;
    if (!(c > 0.0)) return NBSS_EINVAL;
    if ((e = rir_check_cuts(B, n_samples, fs, tw, k_d, broadcast, false))) return e;
    const int64_t need = rir_ism_ws_bytes_impl(B, nb_img);
    if (need < 0) return (int)need;
    if (ws_bytes < need) return NBSS_EINVAL;
    int32_t* hdr = reinterpret_cast<int32_t*>(ws);
    double* table = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + (size_t)B * 16);
    int first = 0;
    for (int b = 0; b < B; ++b) {
        const int Nx = nb_img[3 * b], Ny = nb_img[3 * b + 1], Nz = nb_img[3 * b + 2];
        NBSS_LAUNCH(rir_table_kernel, dim3(1), dim3(256), 0, st, b, Nx, Ny, Nz, first, beta, hdr, table);
        if ((e = NBSS_CHECK_LAUNCH())) return e;
        first += Nx + Ny + Nz;
    }
    const size_t lds = sizeof(RirEntry) * RIR_TILE * RIR_SLOTS + sizeof(int) * (RIR_TILE + 2);  // 49 KB: three workgroups per CU
    const double Tk = tw * fs, half_K = 0.5 * (double)llrint(Tk);
    return rir_for_launches(B, k_d, broadcast, [&](int room0, int nr, const RirRoomCuts& cuts, bool) {
        NBSS_LAUNCH(rir_ism_kernel, dim3(cdiv(n_samples, RIR_TILE), S * M, nr), dim3(RIR_TILE), lds, st, S, M, n_samples, fs / c, Tk, half_K, room0, cuts, room_sz,
                    pos_src, pos_rcv, hdr, table, h);
        return NBSS_CHECK_LAUNCH();
    });
}

// nbss_rir_tail (broadcast: one cut, which must be a tail start) and nbss_rir_tail_rooms; a launch in which no room has a tail is skipped
int rir_tail_impl(int B, int S, int M, int n_samples, double fs, double tw, const int32_t* k_d, bool broadcast, const double* rt60, int64_t seed, float* h,
                  hipStream_t st) {
    int e = rir_check_common(B, S, M, n_samples, fs, tw);
    if (e) return e;
    if ((e = rir_check_cuts(B, n_samples, fs, tw, k_d, broadcast, broadcast))) return e;
    const int K = (int)llrint(tw * fs);
    return rir_for_launches(B, k_d, broadcast, [&](int room0, int nr, const RirRoomCuts& cuts, bool any) {
        if (!any) return 0;
        NBSS_LAUNCH(rir_tail_kernel, dim3(S * M, nr), dim3(256), (RIR_MAX_WIN + 1) * sizeof(double), st, S, M, n_samples, K, room0, cuts, fs, (uint64_t)seed, rt60,
                    h);
        return NBSS_CHECK_LAUNCH();
    });
}
