// knn.hip - the k-nearest-neighbour manifold estimate of score_cifar.py (precision, recall, nearest reference row) in a feature space:
//   d2(i, j) = max(0, |a_i|^2 + |b_j|^2 - 2 a_i . b_j)   (fp64 over fp32 features [m, d] and [n, d], widened exactly)
//   knn_radii: r2[i] = the k-th smallest d2(i, j) over j != i of one set against itself
//   knn_cover: covered[i] = any_j d2(i, j) <= r2_b[j],  nn_d2[i] = min_j d2(i, j),  nn_idx[i] = the lowest j attaining it
// An fp32 value converts to fp64 exactly and the fp64 product of two of them is exact: the only roundings are those of the sums.  The dot
// products AND both row norms run on v_mfma_f64_16x16x4_f64 over the same k-ordered accumulation chain (the norms are the diagonal of a
// tile against itself), so for two bit-identical rows the three numbers are one and the same x, and (x + x) - 2 x == 0.0 exactly: a copy
// of a reference row is at distance 0, inside a ball of radius 0, and bit-identical rows of b give bit-identical distances.  Steps whose
// products are all 0 (columns past d) add exactly 0, so a chain may stop at the last step that holds a column.
//
// One workgroup owns 64 rows of a (16 per wave, one 16 x 16 C tile per 16 rows of b) and streams all of b in tiles of 64 rows; a tile is
// staged once in LDS, 64 feature columns at a time; the next chunk of b and the wave's own A operands of that chunk are loaded into
// registers under the current chunk's MFMAs, so the MFMA loop itself reads LDS and registers only.  Wave w also
// takes the norms of the tile's rows 16 w .. 16 w + 15.  After the last column chunk each lane holds four complete dot products per 16
// rows of b (C/D of the f64 form: col = lane & 15, row = (lane >> 4) + 4 reg) and folds them into its running selection: the sorted
// KNN_MAX_K smallest (radii), or the minimum with its index and the coverage flag (cover).  The 16 lanes that share a row are merged
// through LDS by one lane, in lane order.  No [m, n] array, no atomics, one owner per output element; a selection is a function of the
// multiset of a row's distances, so every run gives the same bits.  Rows past m / n and columns past d load 0 and are masked out of the
// selection by index.
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
constexpr int KNN_MAX_K = 8;
constexpr int SEG_MAX_CLASSES = 32;      // the grouped kernels: moments.hip's limit

typedef double double4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void insert_sorted(double (&top)[KNN_MAX_K], double v) {
#pragma unroll
    for (int t = 0; t < KNN_MAX_K; ++t)
        if (v < top[t]) {
            const double o = top[t];
            top[t] = v;
            v = o;
        }
}

// RADII: b == a, n == m, r2out [m].  Otherwise: r2b [n] or null, covered / nn_d2 / nn_idx [m].  The workgroup owns tile blockIdx.x of
// 64 rows of a; SEG (the grouped kernels): tile blk inside a class's segment, with the segment's bases and counts as a, m, b, n and the
// outputs.  The flag is a template parameter so that the pooled kernels compile to the instructions they had before it existed.
// n == 0 (cover, SEG only): nothing of b or r2b is read and the selection stays at its start - not covered, +inf, -1.
template <bool RADII, bool SEG = false>
__device__ __forceinline__ void knn_body(long long blk, const float* __restrict__ a, long long m, const float* __restrict__ b, long long n, int d, int k, bool vec4,
                                         const double* __restrict__ r2b, double* __restrict__ r2out, int* __restrict__ covered,
                                         double* __restrict__ nn_d2, int* __restrict__ nn_idx) {
    __shared__ __attribute__((aligned(16))) float stage[TN][LDB];
    __shared__ double nbs[TN];
    __shared__ double nas[TM];
    __shared__ double mrg_v[WAVES][64][RADII ? KNN_MAX_K : SUB];      // radii: [lane][t] per reg; cover: [lane][reg]
    __shared__ int mrg_j[RADII ? 1 : WAVES][64][4];
    __shared__ int mrg_c[RADII ? 1 : WAVES][64][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 15, lq = lane >> 4;
    const long long row0 = (SEG ? blk : (long long)blockIdx.x) * TM + 16 * wave;
    const long long arow = row0 + lc;                   // the row of a this lane loads as the A operand
    const bool arow_ok = arow < m;
    const float* ap = a + (arow_ok ? arow : m - 1) * d;      // a row past m reads the last one and is masked
    const bool diag[4] = {lq == lc, lq + 4 == lc, lq + 8 == lc, lq + 12 == lc};      // does reg r of this lane hold D[i][i]?

    // |a_i|^2 of the wave's 16 rows: the tile against itself, the same chain as a dot product
    {
        double4_t acc = {0., 0., 0., 0.};
        for (int k0 = 0; k0 < d; k0 += 4) {
            const int kg = k0 + lq;
            const double av = (arow_ok && kg < d) ? (double)ap[kg] : 0.;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, av, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (diag[r]) nas[16 * wave + lc] = acc[r];
    }
    __syncthreads();
    double na[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) na[r] = nas[16 * wave + lq + 4 * r];

    // the running selection of rows row0 + lq + 4 r over this lane's columns
    double top[4][KNN_MAX_K];      // radii: ascending
    double best[4];                // cover
    int bestj[4], cov[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int t = 0; t < KNN_MAX_K; ++t) top[r][t] = __builtin_inf();
        best[r] = __builtin_inf();
        bestj[r] = -1;
        cov[r] = 0;
    }

    const int nchunk = (d + DK - 1) / DK;
    const long long ntile = (n + TN - 1) / TN;
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
    fetch(0, 0);
    for (long long tile = 0; tile < ntile; ++tile) {
        double4_t acc[SUB];
#pragma unroll
        for (int s = 0; s < SUB; ++s) acc[s] = double4_t{0., 0., 0., 0.};
        double4_t nacc = {0., 0., 0., 0.};
        for (int c = 0; c < nchunk; ++c) {
            __syncthreads();      // the previous chunk's reads (and the previous tile's reads of nbs) are done
#pragma unroll
            for (int u = 0; u < PRE / 4; ++u) {
                const int e = tid + TPB * u;
                *reinterpret_cast<float4*>(&stage[e >> 4][4 * (e & 15)]) = make_float4(pre[4 * u], pre[4 * u + 1], pre[4 * u + 2], pre[4 * u + 3]);
            }
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) acur[u] = arow_ok ? apre[u] : 0.f;
            __syncthreads();
            if (c + 1 < nchunk) fetch(tile, c + 1);
            else if (tile + 1 < ntile) fetch(tile + 1, 0);
            const int left = d - c * DK;      // a step past d adds exactly 0 and may be left out
#pragma unroll
            for (int u = 0; u < DK / 4; ++u) {
                if (4 * u < left) {
                    const int kk = 4 * u;
                    const double av = (double)acur[u];
                    double bv[SUB];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) bv[s] = (double)stage[16 * s + lc][kk + lq];
                    const double bn = (double)stage[16 * wave + lc][kk + lq];
#pragma unroll
                    for (int s = 0; s < SUB; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[s], acc[s], 0, 0, 0);
                    nacc = __builtin_amdgcn_mfma_f64_16x16x4f64(bn, bn, nacc, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (diag[r]) nbs[16 * wave + lc] = nacc[r];
        __syncthreads();

        const long long jt = tile * TN;
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            const long long j = jt + 16 * s + lc;
            const bool j_ok = j < n;      // a padded row of b never becomes a neighbour
            const double nb = nbs[16 * s + lc];
            double rj = -1.;
            if (!RADII && r2b) {
                const double v = r2b[j_ok ? j : n - 1];
                rj = j_ok ? v : -1.;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double d2 = (na[r] + nb) - 2. * acc[s][r];
                d2 = d2 < 0. ? 0. : d2;      // (a NaN stays a NaN: it compares false below)
                if (RADII) {
                    if (j_ok && j != row0 + lq + 4 * r && d2 < top[r][KNN_MAX_K - 1]) insert_sorted(top[r], d2);
                } else {
                    cov[r] |= (j_ok && d2 <= rj) ? 1 : 0;
                    const bool nearer = j_ok && d2 < best[r];      // this lane's columns come in increasing order: the lowest j stays
                    best[r] = nearer ? d2 : best[r];
                    bestj[r] = nearer ? (int)j : bestj[r];
                }
            }
        }
    }

    // the 16 lanes 16 lq .. 16 lq + 15 hold the same rows over different columns: merged in lane order
    if (RADII) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            __syncthreads();
#pragma unroll
            for (int t = 0; t < KNN_MAX_K; ++t) mrg_v[wave][lane][t] = top[r][t];
            __syncthreads();
            if (lc == 0) {
                for (int c = 1; c < 16; ++c)
                    for (int t = 0; t < KNN_MAX_K; ++t) {
                        const double v = mrg_v[wave][lane + c][t];
                        if (!(v < top[r][KNN_MAX_K - 1])) break;      // ascending: nothing further of this lane's enters
                        insert_sorted(top[r], v);
                    }
                const long long gi = row0 + lq + 4 * r;
                if (gi < m) {
                    double out = top[r][0];
#pragma unroll
                    for (int t = 1; t < KNN_MAX_K; ++t)
                        if (t == k - 1) out = top[r][t];
                    r2out[gi] = out;
                }
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mrg_v[wave][lane][r] = best[r];
            mrg_j[wave][lane][r] = bestj[r];
            mrg_c[wave][lane][r] = cov[r];
        }
        __syncthreads();
        if (lane < 16) {                                 // lane i takes row row0 + i: reg i >> 2 of lanes 16 (i & 3) ..
            const int r = lane >> 2, l0 = 16 * (lane & 3);
            double v = mrg_v[wave][l0][r];
            int vj = mrg_j[wave][l0][r], vc = mrg_c[wave][l0][r];
            for (int c = 1; c < 16; ++c) {
                const double w = mrg_v[wave][l0 + c][r];
                const int wj = mrg_j[wave][l0 + c][r];
                vc |= mrg_c[wave][l0 + c][r];
                if (w < v || (w == v && wj < vj)) {
                    v = w;
                    vj = wj;
                }
            }
            const long long gi = row0 + lane;
            if (gi < m) {
                if (covered) covered[gi] = vc;
                nn_d2[gi] = v;
                nn_idx[gi] = vj;
            }
        }
    }
}

// Two entry kernels over one body.  Both compile to two waves per SIMD (the radii kernel by itself: 213 VGPRs + 40 AGPRs with its 64
// registers of sorted top-k state; the cover kernel is held to it: 179 VGPRs), no scratch, 34 KB of LDS.
__global__ __launch_bounds__(TPB) void knn_radii_kernel(const float* __restrict__ f, long long n, int d, int k, bool vec4, double* __restrict__ r2) {
    knn_body<true>(0, f, n, f, n, d, k, vec4, nullptr, r2, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(2, 8))) void knn_cover_kernel(
    const float* __restrict__ a, long long m, const float* __restrict__ b, long long n, int d, bool vec4, const double* __restrict__ r2b,
    int* __restrict__ covered, double* __restrict__ nn_d2, int* __restrict__ nn_idx) {
    knn_body<false>(0, a, m, b, n, d, 0, vec4, r2b, nullptr, covered, nn_d2, nn_idx);
}

// ---- the grouped (per-class) kernels: class-sorted operands with device-resident segment starts seg[classes + 1] ----------------------
// Segment start c of an operand of `rows` rows, clamped into [0, rows]: whatever the array holds, no row outside the operand is touched.
__device__ __forceinline__ long long seg_at(const int* __restrict__ seg, int c, long long rows) {
    const long long v = seg[c];
    return v < 0 ? 0 : (v > rows ? rows : v);
}

// Workgroup wg of a grid of ceil(rows / TM) + classes -> its class and its tile of TM rows inside the class's segment, by a scan of the
// segment starts (at most 33 scalar loads; uniform over the workgroup).  false: a surplus workgroup, sum_c ceil(rows_c / TM) <= wg.
__device__ __forceinline__ bool seg_locate(const int* __restrict__ seg, int classes, long long rows, long long wg, int& cls, long long& tile,
                                           long long& start, long long& count) {
    long long first = 0, s0 = seg_at(seg, 0, rows);
    for (int c = 0; c < classes; ++c) {
        const long long s1 = seg_at(seg, c + 1, rows);
        const long long cnt = s1 > s0 ? s1 - s0 : 0;
        const long long t = (cnt + TM - 1) / TM;
        if (wg < first + t) {
            cls = c, tile = wg - first, start = s0, count = cnt;
            return true;
        }
        first += t;
        s0 = s1 > s0 ? s1 : s0;
    }
    return false;
}

// One launch for every class: workgroup -> (class, tile of the class's rows), then the pooled body on the segment's bases and counts, so
// class c receives the bits knn_radii_kernel / knn_cover_kernel leave from the gathered rows.  A surplus workgroup returns before the
// body's first barrier.  Two waves per SIMD as the pooled kernels, no scratch: 249 VGPRs (radii), 179 (cover); DESIGN 27.
__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(2, 8))) void knn_radii_seg_kernel(
    const float* __restrict__ f, const int* __restrict__ seg, int classes, long long n, int d, int k, bool vec4, double* __restrict__ r2) {
    int cls;
    long long tile, s0, cnt;
    if (!seg_locate(seg, classes, n, blockIdx.x, cls, tile, s0, cnt)) return;
    const float* base = f + s0 * d;
    knn_body<true, true>(tile, base, cnt, base, cnt, d, k, vec4, nullptr, r2 + s0, nullptr, nullptr, nullptr);
}

__global__ __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(2, 8))) void knn_cover_seg_kernel(
    const float* __restrict__ a, const int* __restrict__ seg_a, long long m, const float* __restrict__ b, const int* __restrict__ seg_b,
    long long n, int classes, int d, bool vec4, const double* __restrict__ r2b, int* __restrict__ covered, double* __restrict__ nn_d2,
    int* __restrict__ nn_idx) {
    int cls;
    long long tile, a0, ma;
    if (!seg_locate(seg_a, classes, m, blockIdx.x, cls, tile, a0, ma)) return;
    const long long b0 = seg_at(seg_b, cls, n), b1 = seg_at(seg_b, cls + 1, n);
    const long long nb = b1 > b0 ? b1 - b0 : 0;
    knn_body<false, true>(tile, a + a0 * d, ma, b + b0 * d, nb, d, 0, vec4, r2b ? r2b + b0 : nullptr, nullptr, covered ? covered + a0 : nullptr,
                    nn_d2 + a0, nn_idx + a0);
}

inline hipStream_t S(ctgan_stream_t s) { return static_cast<hipStream_t>(s); }

// can a row of the streamed array be read as float4s?
inline bool rows_vec4(const float* p, int d) { return d % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool misaligned8(const void* p) { return reinterpret_cast<uintptr_t>(p) & 7; }

}  // namespace

extern "C" {

int ctgan_knn_max_k(void) { return KNN_MAX_K; }

int ctgan_knn_radii(const float* f, int64_t n, int32_t d, int32_t k, double* r2, ctgan_stream_t stream) {
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_radii: %d features (at most %d)", d, DMAX);
    if (k > KNN_MAX_K) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_radii: k = %d (at most %d)", k, KNN_MAX_K);
    if (k < 1 || n < (int64_t)k + 1) return ctgan_fail(CTGAN_E_BADARG, "knn_radii: %lld rows have no %d-th other neighbour", (long long)n, k);
    if (d < 1 || n > 0x7fffffffLL || !f || !r2 || misaligned8(r2))
        return ctgan_fail(CTGAN_E_BADARG, "knn_radii: bad argument (n %lld d %d), a null pointer, or radii not 8-byte aligned", (long long)n, d);
    hipLaunchKernelGGL(knn_radii_kernel, dim3((unsigned)((n + TM - 1) / TM)), dim3(TPB), 0, S(stream), f, (long long)n, d, k, rows_vec4(f, d), r2);
    return ctgan_check_launch("knn_radii");
}

int ctgan_knn_cover(const float* a, int64_t m, const float* b, int64_t n, int32_t d, const double* r2_b, int32_t* covered, double* nn_d2,
                    int32_t* nn_idx, ctgan_stream_t stream) {
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_cover: %d features (at most %d)", d, DMAX);
    if (d < 1 || m < 0 || n < 1 || m > 0x7fffffffLL || n > 0x7fffffffLL)
        return ctgan_fail(CTGAN_E_BADARG, "knn_cover: bad argument (m %lld n %lld d %d)", (long long)m, (long long)n, d);
    if (m == 0) return CTGAN_OK;
    if (!a || !b || !nn_d2 || !nn_idx || (r2_b && !covered)) return ctgan_fail(CTGAN_E_BADARG, "knn_cover: a null pointer");
    if (misaligned8(r2_b) || misaligned8(nn_d2)) return ctgan_fail(CTGAN_E_BADARG, "knn_cover: fp64 arrays not 8-byte aligned");
    hipLaunchKernelGGL(knn_cover_kernel, dim3((unsigned)((m + TM - 1) / TM)), dim3(TPB), 0, S(stream), a, (long long)m, b, (long long)n, d, rows_vec4(b, d), r2_b,
                       r2_b ? covered : (int*)nullptr, nn_d2, nn_idx);
    return ctgan_check_launch("knn_cover");
}

int ctgan_knn_radii_seg(const float* f, const int32_t* seg, int32_t classes, int64_t n, int32_t d, int32_t k, double* r2, ctgan_stream_t stream) {
    if (classes > SEG_MAX_CLASSES) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_radii_seg: %d classes (at most %d)", classes, SEG_MAX_CLASSES);
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_radii_seg: %d features (at most %d)", d, DMAX);
    if (k > KNN_MAX_K) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_radii_seg: k = %d (at most %d)", k, KNN_MAX_K);
    if (classes < 1 || k < 1 || d < 1 || n < 0 || n > 0x7fffffffLL)
        return ctgan_fail(CTGAN_E_BADARG, "knn_radii_seg: bad argument (classes %d n %lld d %d k %d)", classes, (long long)n, d, k);
    if (n == 0) return CTGAN_OK;
    if (!f || !seg || !r2 || misaligned8(r2)) return ctgan_fail(CTGAN_E_BADARG, "knn_radii_seg: a null pointer, or radii not 8-byte aligned");
    hipLaunchKernelGGL(knn_radii_seg_kernel, dim3((unsigned)((n + TM - 1) / TM + classes)), dim3(TPB), 0, S(stream), f, seg, classes, (long long)n, d, k,
                       rows_vec4(f, d), r2);
    return ctgan_check_launch("knn_radii_seg");
}

int ctgan_knn_cover_seg(const float* a, const int32_t* seg_a, int64_t m, const float* b, const int32_t* seg_b, int64_t n, int32_t classes, int32_t d,
                        const double* r2_b, int32_t* covered, double* nn_d2, int32_t* nn_idx, ctgan_stream_t stream) {
    if (classes > SEG_MAX_CLASSES) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_cover_seg: %d classes (at most %d)", classes, SEG_MAX_CLASSES);
    if (d > DMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "knn_cover_seg: %d features (at most %d)", d, DMAX);
    if (classes < 1 || d < 1 || m < 0 || n < 0 || m > 0x7fffffffLL || n > 0x7fffffffLL)
        return ctgan_fail(CTGAN_E_BADARG, "knn_cover_seg: bad argument (classes %d m %lld n %lld d %d)", classes, (long long)m, (long long)n, d);
    if (m == 0) return CTGAN_OK;
    if (!a || !seg_a || !seg_b || (n > 0 && !b) || !nn_d2 || !nn_idx || (r2_b && !covered)) return ctgan_fail(CTGAN_E_BADARG, "knn_cover_seg: a null pointer");
    if (misaligned8(r2_b) || misaligned8(nn_d2)) return ctgan_fail(CTGAN_E_BADARG, "knn_cover_seg: fp64 arrays not 8-byte aligned");
    hipLaunchKernelGGL(knn_cover_seg_kernel, dim3((unsigned)((m + TM - 1) / TM + classes)), dim3(TPB), 0, S(stream), a, seg_a, (long long)m, b, seg_b,
                       (long long)n, classes, d, rows_vec4(b, d), r2_b, r2_b ? covered : (int*)nullptr, nn_d2, nn_idx);
    return ctgan_check_launch("knn_cover_seg");
}

}  // extern "C"
