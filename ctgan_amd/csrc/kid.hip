// kid.hip - the all-pairs polynomial-kernel sums of score_cifar.py's unbiased kernel distance (Binkowski et al. 2018) in a feature space:
//   k(i, j) = (gamma a_i . b_j + coef0)^3        (fp64 over fp32 features [m, d] and [n, d], widened exactly)
//   sums[p][q] = sum of k(i, j) over i in [64 p, min(64 p + 64, m)), j in [64 q, min(64 q + 64, n)), without i == j when exclude_diag
// The distance is a difference of nearly equal sums of m n terms of size O(1 - 10) at a target of 1e-4 or below, so nothing here is fp32:
// an fp32 value converts to fp64 exactly and the fp64 product of two of them is exact, the dot products run on v_mfma_f64_16x16x4_f64 and
// only their sums round; v = gamma dot + coef0 and v v v are fp64 too.
//
// The tile structure is knn.hip's: four waves own 64 rows of a (16 per wave, one 16 x 16 C tile per 16 rows of b); a tile of 64 rows of b
// is staged once in LDS, 64 feature columns at a time; the next chunk of b and the wave's own A operands of that chunk are loaded into
// registers under the current chunk's MFMAs.  There are no norms here: four MFMAs per step.  After the last column chunk each lane holds
// four complete dot products per 16 rows of b (C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg).
//
// The grid is (tiles of a) x (slabs of `slab` consecutive tiles of b): the outputs are partial sums, so b splits across workgroups and a
// launch with few rows of a still fills the chip.  Every sums[p][q] has one owning workgroup and is reduced in one fixed order - the lane's
// 16 values (C tile, then register), the wave's 64 lanes (an xor butterfly, 32 down to 1), the four waves in order - that does not know
// the slab length: the bits are the same for every grid shape and every run.  No atomics, no [m, n] array.  Rows past m / n and columns
// past d load 0; such a pair would still add coef0^3, so pairs are masked BY INDEX (i < m, j < n, i != j), never by value.
#include "common.h"

namespace {

constexpr int WAVES = 4;
constexpr int TPB = 64 * WAVES;
constexpr int TM = 16 * WAVES;    // rows of a per workgroup
constexpr int TN = 64;            // rows of b per staged tile
constexpr int SUB = TN / 16;      // C tiles per wave and staged tile
constexpr int DK = 64;            // feature columns per staged chunk
constexpr int LDB = DK + 4;       // row stride of the staged tile in floats: bank = 4 (lane & 15) + (lane >> 4), conflict-free
constexpr int PRE = TN * DK / TPB;
constexpr int DMAX = 1024;
constexpr int FILL = 512;         // workgroups asked for at least, when b has the tiles: 256 compute units twice over
constexpr int SLAB_MAX = 8;       // tiles of b per workgroup at most: the tail of a large launch stays a few percent of it
constexpr long long GRID_Y_MAX = 65535;
constexpr long long ROWS_MAX = 1LL << 30;
static_assert(TM == TN, "a tile of sums is square: the same tile size names the rows of both operands");

typedef double double4_t __attribute__((ext_vector_type(4)));

// Compiles to 157 VGPRs, no AGPRs, no scratch, 17 KB of LDS: three waves per SIMD.
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(2, 8))) void kernel_tile_sums_kernel(
    const float* __restrict__ a, long long m, const float* __restrict__ b, long long n, int d, double gamma, double coef0, bool exclude_diag,
    bool vec4, int slab, double* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) float stage[TN][LDB];
    __shared__ double wsum[WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const long long row0 = (long long)blockIdx.x * TM + 16 * wave;
    const long long arow = row0 + lc;                   // the row of a this lane loads as the A operand
    const bool arow_ok = arow < m;
    const float* ap = a + (arow_ok ? arow : m - 1) * d;      // a row past m reads the last one and is masked

    const int nchunk = (d + DK - 1) / DK;
    const long long ntile = (n + TN - 1) / TN;
    const long long tile0 = (long long)blockIdx.y * slab;
    const long long tile1 = tile0 + slab < ntile ? tile0 + slab : ntile;      // the host launches no empty slab: tile0 < ntile
    // the next chunk in registers: float4 e = tid + TPB u of the [TN][DK / 4] chunk of b (a row of the chunk per 16 lanes) and this lane's A
    // operands of the chunk's 16 steps.  A chunk wholly inside b, with 16-byte aligned rows, is loaded without a test per element.
    float pre[PRE], apre[DK / 4], acur[DK / 4];
    auto fetch = [&](long long tile, int c) {
        const bool k_full = (c + 1) * DK <= d;
        if (vec4 && k_full && (tile + 1) * TN <= n) {
            const float* src = b + (tile * TN + (tid >> 4)) * d + c * DK + 4 * (tid & 15);
#pragma unroll
            for (int u = 0; u < PRE / 4; ++u) {
                const float4 v = *reinterpret_cast<const float4*>(src + (long long)(TPB / 16) * u * d);
                pre[4 * u] = v.x, pre[4 * u + 1] = v.y, pre[4 * u + 2] = v.z, pre[4 * u + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int u = 0; u < PRE; ++u) {
                const int e = tid + TPB * (u / 4);
                const long long j = tile * TN + (e >> 4);
                const int kg = c * DK + 4 * (e & 15) + (u & 3);
                pre[u] = (j < n && kg < d) ? b[j * d + kg] : 0.f;
            }
        }
        if (k_full) {
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) apre[u] = ap[c * DK + 4 * u + lq];
        } else {
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) {
                const int kg = c * DK + 4 * u + lq;
                apre[u] = kg < d ? ap[kg] : 0.f;
            }
        }
    };
    fetch(tile0, 0);
    for (long long tile = tile0; tile < tile1; ++tile) {
        double4_t acc[SUB];
#pragma unroll
        for (int s = 0; s < SUB; ++s) acc[s] = double4_t{0., 0., 0., 0.};
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();      // the previous chunk's reads (and the previous tile's read of wsum) are done
#pragma unroll
            for (int u = 0; u < PRE / 4; ++u) {
                const int e = tid + TPB * u;
                *reinterpret_cast<float4*>(&stage[e >> 4][4 * (e & 15)]) = make_float4(pre[4 * u], pre[4 * u + 1], pre[4 * u + 2], pre[4 * u + 3]);
            }
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) acur[u] = arow_ok ? apre[u] : 0.f;
            __syncthreads();
            if (c + 1 < nchunk) fetch(tile, c + 1);
            else if (tile + 1 < tile1) fetch(tile + 1, 0);
            const int left = d - c * DK;      // a step past d adds exactly 0 and may be left out
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) {
                if (4 * u < left) {
                    const int kk = 4 * u;
                    const double av = (double)acur[u];
                    double bv[SUB];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) bv[s] = (double)stage[16 * s + lc][kk + lq];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[s], acc[s], 0, 0, 0);
                }
            }
        }

        // this lane's 16 kernel values, masked by index, in the order (C tile, register)
        const long long jt = tile * TN;
        double part = 0.;
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            const long long j = jt + 16 * s + lc;
            const bool j_ok = j < n;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long i = row0 + lq + 4 * r;
                const double v = gamma * acc[s][r] + coef0;
                const double k3 = (v * v) * v;
                const bool keep = j_ok && i < m && !(exclude_diag && i == j);
                part += keep ? k3 : 0.;
            }
        }
        // the wave's 64 lanes: every lane ends with the same sum; then the four waves in order
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
        if (lane == 0) wsum[wave] = part;
        __syncthreads();
        if (tid == 0) sums[(long long)blockIdx.x * ntile + tile] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

inline hipStream_t S(ctgan_stream_t s) { return static_cast<hipStream_t>(s); }

// can a row of the streamed array be read as float4s?
inline bool rows_vec4(const float* p, int d) { return d % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool misaligned8(const void* p) { return reinterpret_cast<uintptr_t>(p) & 7; }

// Tiles of b per workgroup: as many slabs per tile of a as fill the chip once (FILL workgroups in all, when b has the tiles), never more
// than SLAB_MAX tiles each unless the grid's second dimension would overflow.
inline int slab_length(long long mt, long long nt) {
    const long long want = (FILL + mt - 1) / mt;
    const long long slabs = want < nt ? want : nt;
    long long slab = (nt + slabs - 1) / slabs;
    if (slab > SLAB_MAX) slab = SLAB_MAX;
    const long long least = (nt + GRID_Y_MAX - 1) / GRID_Y_MAX;
    return (int)(slab < least ? least : slab);
}

}  // namespace

extern "C" {

int ctgan_kernel_tile(void) { return TM; }

int ctgan_kernel_tile_sums(const float* a, int64_t m, const float* b, int64_t n, int32_t d, double gamma, double coef0, int32_t exclude_diag,
                           double* sums, ctgan_stream_t stream) {
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "kernel_tile_sums: %d features (at most %d)", d, DMAX);
    if (d < 1 || m < 1 || n < 1 || m > ROWS_MAX || n > ROWS_MAX)
        return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums: bad argument (m %lld n %lld d %d)", (long long)m, (long long)n, d);
    if (exclude_diag && m != n)
        return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums: exclude_diag is for a set against itself (m %lld n %lld)", (long long)m, (long long)n);
    if (!a || !b || !sums) return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums: a null pointer");
    if (misaligned8(sums)) return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums: sums not 8-byte aligned");
    const long long mt = (m + TM - 1) / TM, nt = (n + TN - 1) / TN;
    const int slab = slab_length(mt, nt);
    hipLaunchKernelGGL(kernel_tile_sums_kernel, dim3((unsigned)mt, (unsigned)((nt + slab - 1) / slab)), dim3(TPB), 0, S(stream), a, (long long)m, b,
                       (long long)n, d, gamma, coef0, exclude_diag != 0, rows_vec4(b, d), slab, sums);
    return ctgan_check_launch("kernel_tile_sums");
}

}  // extern "C"
