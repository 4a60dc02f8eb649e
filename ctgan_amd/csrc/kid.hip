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
constexpr int SEG_MAX_CLASSES = 32;      // the grouped kernel: moments.hip's limit
static_assert(TM == TN, "a tile of sums is square: the same tile size names the rows of both operands");

typedef double double4_t __attribute__((ext_vector_type(4)));

// Compiles to 157 VGPRs, no AGPRs, no scratch, 17 KB of LDS: three waves per SIMD.
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(2, 8))) void kernel_tile_sums_kernel(
    const float* __restrict__ a, long long m, const float* __restrict__ b, long long n, int d, double gamma, double coef0, bool exclude_diag,
    bool vec4, int slab, double* __restrict__ sums) {
#define KID_BLK (long long)blockIdx.x
#define KID_SLAB (long long)blockIdx.y
#include "kid_tile_loop.h"
#undef KID_BLK
#undef KID_SLAB
}

// ---- the grouped (per-class) kernel: class-sorted operands with device-resident segment starts seg[classes + 1] ----------------------
// Segment start c of an operand of `rows` rows, clamped into [0, rows]: whatever the array holds, no row outside the operand is touched.
__device__ __forceinline__ long long seg_at(const int* __restrict__ seg, int c, long long rows) {
    const long long v = seg[c];
    return v < 0 ? 0 : (v > rows ? rows : v);
}

// One launch for every class.  grid.x = ceil(m / 64) + classes >= sum_c ceil(m_c / 64): workgroup x -> (class, tile of the class's rows of a)
// by a scan of seg_a (at most 33 scalar loads, uniform over the workgroup); grid.y = the slabs at the pooled bound ceil(n / 64).  A surplus
// workgroup, and one whose slab starts past its class's tiles of b, returns before the loop's first barrier.  The pooled kernel's loop
// (kid_tile_loop.h, the same text) then runs on the segment's bases and counts into the class's tile matrix at sums + toff[c]: the bits
// kernel_tile_sums_kernel leaves from the gathered rows, for every slab length.  toff is the caller's (the exclusive prefix sums of
// ceil(m_c / 64) ceil(n_c / 64)).  157 VGPRs, no scratch: the pooled kernel's three waves per SIMD.
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(2, 8))) void kernel_tile_sums_seg_kernel(
    const float* __restrict__ a, const int* __restrict__ seg_a, long long m, const float* __restrict__ b, const int* __restrict__ seg_b, long long n,
    int classes, int d, double gamma, double coef0, bool exclude_diag, bool vec4, int slab, const long long* __restrict__ toff,
    double* __restrict__ sums) {
    const long long wg = blockIdx.x;
    long long first = 0, a0 = seg_at(seg_a, 0, m), ma = 0, seg_tile = 0;
    int cls = -1;
    for (int c = 0; c < classes; ++c) {
        const long long a1 = seg_at(seg_a, c + 1, m);
        const long long cnt = a1 > a0 ? a1 - a0 : 0;
        const long long t = (cnt + TM - 1) / TM;
        if (wg < first + t) {
            cls = c, seg_tile = wg - first, ma = cnt;
            break;
        }
        first += t;
        a0 = a1 > a0 ? a1 : a0;
    }
    if (cls < 0) return;
    const long long b0 = seg_at(seg_b, cls, n), b1 = seg_at(seg_b, cls + 1, n);
    const long long nb = b1 > b0 ? b1 - b0 : 0;
    if ((long long)blockIdx.y * slab >= (nb + TN - 1) / TN) return;
    a += a0 * d, b += b0 * d, m = ma, n = nb, sums += toff[cls];
#define KID_BLK seg_tile
#define KID_SLAB (long long)blockIdx.y
#include "kid_tile_loop.h"
#undef KID_BLK
#undef KID_SLAB
}

// out[s] = the fp64 sum of vals[off[s] : off[s + 1]]: one workgroup per segment, thread t adds elements t, t + 256, ... in index order, then
// an LDS tree in a fixed order.  Nothing of the order depends on the grid: the same bits on every run.  An empty segment gives 0.
constexpr int SEG_TPB = 256;
__global__ __launch_bounds__(SEG_TPB) void segment_sums_kernel(const double* __restrict__ vals, const long long* __restrict__ off, double* __restrict__ out) {
    __shared__ double part[SEG_TPB];
    const long long lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
    double acc = 0.;
    for (long long i = lo + threadIdx.x; i < hi; i += SEG_TPB) acc += vals[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int w = SEG_TPB / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = part[0];
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

int ctgan_kernel_tile_sums_seg(const float* a, const int32_t* seg_a, int64_t m, const float* b, const int32_t* seg_b, int64_t n, int32_t classes,
                               int32_t d, double gamma, double coef0, int32_t exclude_diag, const int64_t* toff, double* sums, ctgan_stream_t stream) {
    if (classes > SEG_MAX_CLASSES) return ctgan_fail(CTGAN_E_UNSUPPORTED, "kernel_tile_sums_seg: %d classes (at most %d)", classes, SEG_MAX_CLASSES);
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "kernel_tile_sums_seg: %d features (at most %d)", d, DMAX);
    if (classes < 1 || d < 1 || m < 1 || n < 1 || m > ROWS_MAX || n > ROWS_MAX)
        return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums_seg: bad argument (classes %d m %lld n %lld d %d)", classes, (long long)m, (long long)n, d);
    if (exclude_diag && (a != b || seg_a != seg_b || m != n))
        return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums_seg: exclude_diag is for a set against itself (the same operand and segments twice)");
    if (!a || !b || !seg_a || !seg_b || !toff || !sums) return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums_seg: a null pointer");
    if (misaligned8(sums) || misaligned8(toff)) return ctgan_fail(CTGAN_E_BADARG, "kernel_tile_sums_seg: sums or toff not 8-byte aligned");
    const long long mt = (m + TM - 1) / TM + classes, nt = (n + TN - 1) / TN;
    const int slab = slab_length(mt, nt);
    hipLaunchKernelGGL(kernel_tile_sums_seg_kernel, dim3((unsigned)mt, (unsigned)((nt + slab - 1) / slab)), dim3(TPB), 0, S(stream), a, seg_a, (long long)m, b,
                       seg_b, (long long)n, classes, d, gamma, coef0, exclude_diag != 0, rows_vec4(b, d), slab,
                       reinterpret_cast<const long long*>(toff), sums);
    return ctgan_check_launch("kernel_tile_sums_seg");
}

int ctgan_segment_sums(const double* vals, const int64_t* off, int32_t segments, double* out, ctgan_stream_t stream) {
    if (segments < 0) return ctgan_fail(CTGAN_E_BADARG, "segment_sums: %d segments", segments);
    if (segments == 0) return CTGAN_OK;
    if (!vals || !off || !out) return ctgan_fail(CTGAN_E_BADARG, "segment_sums: a null pointer");
    if (misaligned8(vals) || misaligned8(off) || misaligned8(out)) return ctgan_fail(CTGAN_E_BADARG, "segment_sums: arrays not 8-byte aligned");
    hipLaunchKernelGGL(segment_sums_kernel, dim3((unsigned)segments), dim3(SEG_TPB), 0, S(stream), vals, reinterpret_cast<const long long*>(off), out);
    return ctgan_check_launch("segment_sums");
}

}  // extern "C"
