// moments.hip - the streaming first and second raw moments of a feature layer, for the Frechet distance of score_cifar.py:
//   s1[a] += sum_i f[i, a],   s2[a, b] += sum_i f[i, a] f[i, b]   (fp64 state, fp32 features [m, d])
// An fp32 value converts to fp64 exactly and the fp64 product of two of them is exact (48 significand bits): the only roundings are
// those of the sums.  One workgroup per upper-triangular pair (ti <= tj) of 16-column tiles owns the block s2[16 ti.., 16 tj..] and its
// mirror image, the diagonal workgroups also own s1 of their 16 columns: every state element has one owner per launch, which adds to it
// with a plain load / add / store.  Four waves take a fixed quarter of the rows each, four rows per v_mfma_f64_16x16x4_f64; their partial
// tiles are folded through LDS in wave order.  No atomics, every sum in a fixed order - the same bits on every run with the same chunks.
// ctgan_class_moments_accum runs the same loop per class of an int32 label column, in one launch (below); ctgan_confusion_accum counts
// label x predicted class from the logits of the same pass.
#include "argmax.h"
#include "common.h"

namespace {

constexpr int TILE = 16;
constexpr int WAVES = 4;
constexpr int TPB = 64 * WAVES;
constexpr int DMAX = 1024;
constexpr int UNROLL = 4;     // MFMA steps (of four rows) per loop iteration

typedef double double4_t __attribute__((ext_vector_type(4)));

// The accumulation of `m` rows into the state (s1, s2) by one workgroup, the one of tile pair `pair`.  INDEXED: logical row r is row
// rows[r] of f (the class kernel's compacted list, in LDS), otherwise row r itself; nothing else differs between the two kernels, so
// the same rows in the same order leave the same bits.
template <bool INDEXED>
__device__ __forceinline__ void moments_body(const float* __restrict__ f, const unsigned short* rows, long long m, int d, int pair,
                                             double* __restrict__ s1, double* __restrict__ s2, double (*part)[TILE][TILE + 1],
                                             double (*colsum)[64]) {
    const int T = (d + TILE - 1) / TILE;
    int ti = 0, rest = pair;                             // pair -> (ti, tj), ti <= tj, row-major over the upper triangle
    while (rest >= T - ti) { rest -= T - ti; ++ti; }
    const int tj = ti + rest;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ca = TILE * ti + (lane & 15), cb = TILE * tj + (lane & 15);
    const bool in_a = ca < d, in_b = cb < d, diag = ti == tj;
    const long long quarter = (m + 4 * WAVES - 1) / (4 * WAVES) * 4;      // rows per wave, a multiple of the MFMA's k = 4
    const long long lo = wave * quarter, hi = lo + quarter < m ? lo + quarter : m;

    // A[i = lane & 15][k = lane >> 4] = f[row + k][16 ti + i], B[k = lane >> 4][j = lane & 15] = f[row + k][16 tj + j]: D = A B
    double4_t acc = {0., 0., 0., 0.};
    double cs = 0.;                                      // this lane's share of column ca's sum (the diagonal workgroups' s1)
    for (long long k = lo; k < hi; k += 4 * UNROLL) {    // UNROLL steps' loads in flight; a row past the end loads 0 and adds exactly 0
        double a[UNROLL], b[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long long r = k + 4 * u + (lane >> 4);
            const bool in_r = r < hi;
            const long long row = INDEXED ? (in_r ? (long long)rows[r] : 0) : r;
            a[u] = (in_r && in_a) ? (double)f[row * d + ca] : 0.;
            b[u] = diag ? a[u] : ((in_r && in_b) ? (double)f[row * d + cb] : 0.);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
            cs += a[u];
        }
    }
    // C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][(lane >> 4) + 4 * r][lane & 15] = acc[r];
    colsum[wave][lane] = cs;
    __syncthreads();

    const int i = tid >> 4, j = tid & 15;                // one thread per element of the 16 x 16 block
    const int ga = TILE * ti + i, gb = TILE * tj + j;
    if (ga < d && gb < d && (!diag || i <= j)) {         // a diagonal block's lower half is written as the mirror of its upper half
        double v = part[0][i][j];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) v += part[w][i][j];
        double* p = s2 + (long long)ga * d + gb;
        *p += v;
        if (ga != gb) {
            double* q = s2 + (long long)gb * d + ga;
            *q += v;
        }
    }
    if (diag && tid < TILE && TILE * ti + tid < d) {     // column sums: the four row groups of each wave, waves in order
        double v = 0.;
        for (int w = 0; w < WAVES; ++w)
            for (int g = 0; g < 4; ++g) v += colsum[w][16 * g + tid];
        s1[TILE * ti + tid] += v;
    }
}

__global__ __launch_bounds__(TPB) void moments_accum_kernel(const float* __restrict__ f, long long m, int d, double* __restrict__ s1,
                                                            double* __restrict__ s2) {
    __shared__ double part[WAVES][TILE][TILE + 1];
    __shared__ double colsum[WAVES][64];
    moments_body<false>(f, nullptr, m, d, (int)blockIdx.x, s1, s2, part, colsum);
}

// ---- the same accumulation segmented by a label column: grid (tile pairs, classes).  Workgroup (pair, c) first builds the list of
// the chunk's rows with label c, in ascending row order, in LDS: 256 rows per step, a ballot per wave, the waves' counts exchanged
// through LDS (double-buffered: one barrier per step), every row written at (rows so far) + (earlier waves') + (lower lanes').  Every
// workgroup of a class builds the same list (the label column is m * 4 bytes, read from L2).  Then the shared body runs over the list
// into the class's slice of the state.  A label outside [0, classes) matches no workgroup.  Workgroup (0, c) owns cnt[c].
constexpr int MAX_ROWS = 8192;     // the list is MAX_ROWS * 2 bytes of LDS (16 KB) beside the 10.5 KB of fold buffers
constexpr int CMAX = 32;

__global__ __launch_bounds__(TPB) void class_moments_accum_kernel(const float* __restrict__ f, const int32_t* __restrict__ labels, int m,
                                                                  int d, long long* __restrict__ cnt, double* __restrict__ s1,
                                                                  double* __restrict__ s2) {
    __shared__ double part[WAVES][TILE][TILE + 1];
    __shared__ double colsum[WAVES][64];
    __shared__ unsigned short rows[MAX_ROWS];
    __shared__ int wcount[2][WAVES];
    const int c = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int total = 0;                                       // (uniform) rows of class c before this step
    for (int base = 0, step = 0; base < m; base += TPB, step ^= 1) {
        const int r = base + tid;
        const bool mine = r < m && labels[r] == c;
        const unsigned long long mask = __ballot(mine);
        if (lane == 0) wcount[step][wave] = __popcll(mask);
        __syncthreads();
        int before = total;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int n = wcount[step][w];
            if (w < wave) before += n;
            total += n;
        }
        if (mine) rows[before + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)r;
    }
    if (total == 0) return;                              // (uniform) an absent class: its state stays untouched
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) cnt[c] += total;
    moments_body<true>(f, rows, total, d, (int)blockIdx.x, s1 + (long long)c * d, s2 + (long long)c * d * d, part, colsum);
}

// ---- conf[label, argmax] += 1: LDS integer counters per workgroup, then integer adds into the caller's matrix (exact in any order)
constexpr int CONF_BLOCKS = 64;

__global__ __launch_bounds__(TPB) void confusion_accum_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, long long m,
                                                              int K, unsigned long long* __restrict__ conf) {
    __shared__ int local[CMAX * CMAX];
    for (int i = threadIdx.x; i < K * K; i += TPB) local[i] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * TPB;
    for (long long row = (long long)blockIdx.x * TPB + threadIdx.x; row < m; row += stride) {
        const int lab = labels[row];
        if (lab < 0 || lab >= K) continue;
        float best;
        atomicAdd(&local[lab * K + ctgan_argmax_first(logits + row * K, K, best)], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * K; i += TPB)
        if (local[i]) atomicAdd(&conf[i], (unsigned long long)local[i]);
}

inline hipStream_t S(ctgan_stream_t s) { return static_cast<hipStream_t>(s); }

}  // namespace

extern "C" {

int ctgan_moments_accum(const float* f, int64_t m, int32_t d, double* s1, double* s2, ctgan_stream_t stream) {
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "moments_accum: %d features (at most %d)", d, DMAX);
    if (d < 1 || m < 0 || m > (1LL << 40) || (m > 0 && (!f || !s1 || !s2)))
        return ctgan_fail(CTGAN_E_BADARG, "moments_accum: bad argument (m %lld d %d), or a null pointer", (long long)m, d);
    if ((reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 7) return ctgan_fail(CTGAN_E_BADARG, "moments_accum: state not 8-byte aligned");
    if (m == 0) return CTGAN_OK;
    const int T = (d + TILE - 1) / TILE;
    hipLaunchKernelGGL(moments_accum_kernel, dim3((unsigned)(T * (T + 1) / 2)), dim3(TPB), 0, S(stream), f, (long long)m, d, s1, s2);
    return ctgan_check_launch("moments_accum");
}

int ctgan_class_moments_max_rows(void) { return MAX_ROWS; }

int ctgan_class_moments_accum(const float* f, const int32_t* labels, int64_t m, int32_t d, int32_t classes, int64_t* cnt, double* s1,
                              double* s2, ctgan_stream_t stream) {
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "class_moments_accum: %d features (at most %d)", d, DMAX);
    if (classes > CMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "class_moments_accum: %d classes (at most %d)", classes, CMAX);
    if (m > MAX_ROWS) return ctgan_fail(CTGAN_E_UNSUPPORTED, "class_moments_accum: %lld rows in one call (at most %d)", (long long)m, MAX_ROWS);
    if (d < 1 || classes < 1 || m < 0 || (m > 0 && (!f || !labels || !cnt || !s1 || !s2)))
        return ctgan_fail(CTGAN_E_BADARG, "class_moments_accum: bad argument (m %lld d %d classes %d), or a null pointer", (long long)m, d, classes);
    if ((reinterpret_cast<uintptr_t>(cnt) | reinterpret_cast<uintptr_t>(s1) | reinterpret_cast<uintptr_t>(s2)) & 7)
        return ctgan_fail(CTGAN_E_BADARG, "class_moments_accum: state not 8-byte aligned");
    if (m == 0) return CTGAN_OK;
    const int T = (d + TILE - 1) / TILE;
    hipLaunchKernelGGL(class_moments_accum_kernel, dim3((unsigned)(T * (T + 1) / 2), (unsigned)classes), dim3(TPB), 0, S(stream), f, labels, (int)m, d,
                       reinterpret_cast<long long*>(cnt), s1, s2);
    return ctgan_check_launch("class_moments_accum");
}

int ctgan_confusion_accum(const float* logits, const int32_t* labels, int64_t m, int32_t classes, int64_t* conf, ctgan_stream_t stream) {
    if (classes > CMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "confusion_accum: %d classes (at most %d)", classes, CMAX);
    if (classes < 1 || m < 0 || m > (1LL << 31) || (m > 0 && (!logits || !labels || !conf)))      // (a workgroup's LDS counters are int)
        return ctgan_fail(CTGAN_E_BADARG, "confusion_accum: bad argument (m %lld classes %d), or a null pointer", (long long)m, classes);
    if (reinterpret_cast<uintptr_t>(conf) & 7) return ctgan_fail(CTGAN_E_BADARG, "confusion_accum: matrix not 8-byte aligned");
    if (m == 0) return CTGAN_OK;
    hipLaunchKernelGGL(confusion_accum_kernel, dim3(ctgan_blocks(m, TPB, CONF_BLOCKS)), dim3(TPB), 0, S(stream), logits, labels, (long long)m, classes,
                       reinterpret_cast<unsigned long long*>(conf));
    return ctgan_check_launch("confusion_accum");
}

}  // extern "C"
