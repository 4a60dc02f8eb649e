// moments.hip - the streaming first and second raw moments of a feature layer, for the Frechet distance of score_cifar.py:
//   s1[a] += sum_i f[i, a],   s2[a, b] += sum_i f[i, a] f[i, b]   (fp64 state, fp32 features [m, d])
// An fp32 value converts to fp64 exactly and the fp64 product of two of them is exact (48 significand bits): the only roundings are
// those of the sums.  One workgroup per upper-triangular pair (ti <= tj) of 16-column tiles owns the block s2[16 ti.., 16 tj..] and its
// mirror image, the diagonal workgroups also own s1 of their 16 columns: every state element has one owner per launch, which adds to it
// with a plain load / add / store.  Four waves take a fixed quarter of the rows each, four rows per v_mfma_f64_16x16x4_f64; their partial
// tiles are folded through LDS in wave order.  No atomics, every sum in a fixed order - the same bits on every run with the same chunks.
#include "common.h"

namespace {

constexpr int TILE = 16;
constexpr int WAVES = 4;
constexpr int TPB = 64 * WAVES;
constexpr int DMAX = 1024;
constexpr int UNROLL = 4;     // MFMA steps (of four rows) per loop iteration

typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(TPB) void moments_accum_kernel(const float* __restrict__ f, long long m, int d, double* __restrict__ s1,
                                                            double* __restrict__ s2) {
    __shared__ double part[WAVES][TILE][TILE + 1];
    __shared__ double colsum[WAVES][64];
    const int T = (d + TILE - 1) / TILE;
    int ti = 0, rest = (int)blockIdx.x;                  // blockIdx -> (ti, tj), ti <= tj, row-major over the upper triangle
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
            const long long row = k + 4 * u + (lane >> 4);
            const bool in_r = row < hi;
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

}  // extern "C"
