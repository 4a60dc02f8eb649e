// score_cifar.hip - the device path between a generator and its classifier score (score_cifar.py): generator output -> the CT
// classifier's input in one launch, and the streaming score statistic of tflib.inception_score.score_from_probabilities over the
// logits of successive chunks - no [n, K] prediction array exists anywhere.
//   mean_i sum_j p_ij (log p_ij - log m_j) = (1/n) sum_i sum_j p_ij log p_ij - sum_j m_j log m_j,   m = mean_i p_i
//   reductions: per-thread fp64 partials, an LDS tree in a fixed order, one thread adds to the caller's state with plain loads and
//   stores; no float atomics - the same bits on every run.  The class counts are integers (LDS / global integer adds: exact in any order).
#include "argmax.h"
#include "common.h"
#include "pixel_u8.h"

namespace {

constexpr int TPB = 256;
constexpr int KMAX = 32;      // classes: a row's accumulators live in registers
constexpr int GRP = 8;        // accumulators that share one pass of the LDS tree

// x [n, C, S, S] (NCHW) -> out [n, S, S, C] rotated by 180 degrees: physical pixel p of an image holds reference pixel S S - 1 - p.
__global__ void score_input_kernel(const float* __restrict__ x, const float* __restrict__ lut, float* __restrict__ out, long long pixels, int C,
                                   int hw, float scale) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pixels; i += stride) {
        const long long img = i / hw;
        const int p = (int)(i - img * hw);
        const float* src = x + img * C * hw + (hw - 1 - p);
        float* o = out + i * C;
        for (int c = 0; c < C; ++c) o[c] = lut[pixel_u8(src[(long long)c * hw], scale)];
    }
}

__device__ __forceinline__ long long split_begin(long long k, long long n, int splits) { return k * n / splits; }

// One workgroup per split; its rows inside the chunk [r0, r0 + m) are strided over the threads.
__global__ __launch_bounds__(TPB) void score_accum_kernel(const float* __restrict__ logits, long long m, int K, long long r0, long long n,
                                                          int splits, const int32_t* __restrict__ labels, double* __restrict__ acc,
                                                          unsigned long long* __restrict__ cnt) {
    __shared__ double red[GRP][TPB];
    __shared__ int hist[2 * KMAX];
    const int k = blockIdx.x, tid = threadIdx.x;
    const long long lo = split_begin(k, n, splits), hi = split_begin(k + 1, n, splits);
    const long long a = (lo > r0 ? lo : r0) - r0, b = (hi < r0 + m ? hi : r0 + m) - r0;
    if (a >= b) return;                                  // (uniform over the workgroup) none of this split's rows in this chunk
    if (tid < 2 * KMAX) hist[tid] = 0;
    __syncthreads();
    double s[KMAX + GRP], ent = 0.;                      // (the tail beyond KMAX only keeps the unrolled tree's indices static)
#pragma unroll
    for (int j = 0; j < KMAX + GRP; ++j) s[j] = 0.;
    for (long long row = a + tid; row < b; row += TPB) {
        const float* z = logits + row * K;
        float best;
        const int arg = ctgan_argmax_first(z, K, best);  // numpy.argmax: the first maximum, a NaN counting as one
        const double mx = (double)best;
        double se = 0.;
        for (int j = 0; j < K; ++j) se += exp((double)z[j] - mx);
        const double lse = log(se);
        double t = 0.;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < K) {
                const double lp = (double)z[j] - mx - lse;
                const double p = exp(lp);
                s[j] += p;
                t += (p == 0. && isfinite(lp)) ? 0. : p * lp;      // an underflowed p adds exactly 0; a non-finite logit stays NaN
            }
        }
        ent += t;
        atomicAdd(&hist[arg], 1);
        if (labels && labels[row] == arg) atomicAdd(&hist[K + arg], 1);
    }
    double* mine = acc + (long long)k * (K + 1);
#pragma unroll
    for (int j0 = 0; j0 <= KMAX; j0 += GRP) {
        if (j0 <= K) {                                   // (uniform) accumulator j < K: class j, accumulator K: sum_j p_j lp_j
#pragma unroll
            for (int g = 0; g < GRP; ++g) {
                const int j = j0 + g;
                red[g][tid] = j < K ? s[j] : (j == K ? ent : 0.);
            }
            __syncthreads();
            for (int w = TPB / 2; w > 0; w >>= 1) {
                if (tid < w) {
#pragma unroll
                    for (int g = 0; g < GRP; ++g) red[g][tid] += red[g][tid + w];
                }
                __syncthreads();
            }
            if (tid == 0) {
                for (int g = 0; g < GRP && j0 + g <= K; ++g) mine[j0 + g] += red[g][0];
            }
            __syncthreads();
        }
    }
    if (tid < 2 * K && hist[tid]) atomicAdd(&cnt[tid], (unsigned long long)hist[tid]);
}

__global__ __launch_bounds__(TPB) void score_finish_kernel(const double* __restrict__ acc, long long n, int splits, int K, double* __restrict__ out) {
    for (int k = threadIdx.x; k < splits; k += TPB) {
        const double nk = (double)(split_begin(k + 1, n, splits) - split_begin(k, n, splits));
        const double* a = acc + (long long)k * (K + 1);
        double h = 0.;
        for (int j = 0; j < K; ++j) {
            const double mj = a[j] / nk;
            h += (mj == 0.) ? 0. : mj * log(mj);
        }
        out[2 + k] = exp(a[K] / nk - h);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {                              // mean and population std over the splits, in index order
        double sum = 0.;
        for (int k = 0; k < splits; ++k) sum += out[2 + k];
        const double mean = sum / splits;
        double var = 0.;
        for (int k = 0; k < splits; ++k) {
            const double d = out[2 + k] - mean;
            var += d * d;
        }
        out[0] = mean;
        out[1] = sqrt(var / splits);
    }
}

inline hipStream_t S(ctgan_stream_t s) { return static_cast<hipStream_t>(s); }

}  // namespace

extern "C" {

int ctgan_score_input(const float* x, int64_t n, int32_t channels, int32_t size, float scale, const float* lut, float* out,
                      ctgan_stream_t stream) {
    if (n < 0 || channels <= 0 || channels > 16 || size <= 0 || size > 1024 || !(scale > 0.f) || n > (1LL << 40) / ((long long)channels * size * size) ||
        !lut || (n > 0 && (!x || !out)))
        return ctgan_fail(CTGAN_E_BADARG, "score_input: bad argument (n %lld c %d size %d scale %g)", (long long)n, channels, size, scale);
    if (n == 0) return CTGAN_OK;
    const long long pixels = (long long)n * size * size;
    hipLaunchKernelGGL(score_input_kernel, dim3(ctgan_blocks(pixels, TPB)), dim3(TPB), 0, S(stream), x, lut, out, pixels, channels, size * size,
                       scale);
    return ctgan_check_launch("score_input");
}

static int score_shape_ok(const char* what, int64_t n, int32_t splits, int32_t classes) {
    if (classes > KMAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "%s: %d classes (at most %d)", what, classes, KMAX);
    if (classes <= 0 || splits <= 0 || splits > (1 << 16) || n < splits || n > (1LL << 40))
        return ctgan_fail(CTGAN_E_BADARG, "%s: bad shape n %lld splits %d classes %d", what, (long long)n, splits, classes);
    return CTGAN_OK;
}

int ctgan_score_accum(const float* logits, int64_t m, int32_t classes, int64_t r0, int64_t n, int32_t splits, const int32_t* labels,
                      double* acc, int64_t* cnt, ctgan_stream_t stream) {
    const int rc = score_shape_ok("score_accum", n, splits, classes);
    if (rc) return rc;
    if (m < 0 || r0 < 0 || r0 + m > n || !acc || !cnt || (m > 0 && !logits))
        return ctgan_fail(CTGAN_E_BADARG, "score_accum: rows [%lld, %lld) outside [0, %lld), or a null pointer", (long long)r0, (long long)(r0 + m),
                          (long long)n);
    if ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(cnt)) & 7) return ctgan_fail(CTGAN_E_BADARG, "score_accum: state not 8-byte aligned");
    if (m == 0) return CTGAN_OK;
    hipLaunchKernelGGL(score_accum_kernel, dim3((unsigned)splits), dim3(TPB), 0, S(stream), logits, (long long)m, classes, (long long)r0, (long long)n,
                       splits, labels, acc, reinterpret_cast<unsigned long long*>(cnt));
    return ctgan_check_launch("score_accum");
}

int ctgan_score_finish(const double* acc, int64_t n, int32_t splits, int32_t classes, double* out, ctgan_stream_t stream) {
    const int rc = score_shape_ok("score_finish", n, splits, classes);
    if (rc) return rc;
    if (!acc || !out || ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(out)) & 7))
        return ctgan_fail(CTGAN_E_BADARG, "score_finish: null or misaligned pointer");
    hipLaunchKernelGGL(score_finish_kernel, dim3(1), dim3(TPB), 0, S(stream), acc, (long long)n, splits, classes, out);
    return ctgan_check_launch("score_finish");
}

}  // extern "C"
