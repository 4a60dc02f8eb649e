// score.hip - the memory-bound kernels of the self-trained MNIST score classifier (LS/inception_score.py; LS/ = the reference's
// tensorflow_generative_model/LSUN_bedrooms): ELU (:38-39) and the global-norm gradient clip of LS/tflib/train_loop_2.py:76-79.
// The batch-norm entry points of that network (moving statistics, blend forward, fused residual epilogue) live in bn.hip.
//   elementwise kernels: grid-stride, 16 bytes per lane with a scalar tail (scalar throughout when a pointer is not 16-byte aligned)
//   reductions: two-stage, fp64 partials combined in a fixed order - no atomics, the same bits on every run
#include "common.h"

namespace {

constexpr int TPB = 256;

__device__ __forceinline__ float elu_f(float x) { return x > 0.f ? x : expm1f(x); }
// from the forward OUTPUT: y > 0 <=> x > 0, and for x <= 0  d/dx expm1(x) = exp(x) = y + 1
__device__ __forceinline__ float elu_b(float g, float y) { return y > 0.f ? g : g * (y + 1.f); }

__global__ void elu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0) {
        const long long n4 = n >> 2;
        for (long long v = i; v < n4; v += stride) {
            float4 a = reinterpret_cast<const float4*>(x)[v];
            a.x = elu_f(a.x); a.y = elu_f(a.y); a.z = elu_f(a.z); a.w = elu_f(a.w);
            reinterpret_cast<float4*>(y)[v] = a;
        }
        for (long long t = (n4 << 2) + i; t < n; t += stride) y[t] = elu_f(x[t]);
    } else {
        for (; i < n; i += stride) y[i] = elu_f(x[i]);
    }
}

// gx = [add +] elu'(y) * gy
template <bool ADD>
__global__ void elu_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y, const float* __restrict__ add,
                               float* __restrict__ gx, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    uintptr_t al = reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gx);
    if (ADD) al |= reinterpret_cast<uintptr_t>(add);
    if ((al & 15) == 0) {
        const long long n4 = n >> 2;
        for (long long v = i; v < n4; v += stride) {
            const float4 g = reinterpret_cast<const float4*>(gy)[v];
            const float4 r = reinterpret_cast<const float4*>(y)[v];
            float4 o;
            o.x = elu_b(g.x, r.x); o.y = elu_b(g.y, r.y); o.z = elu_b(g.z, r.z); o.w = elu_b(g.w, r.w);
            if (ADD) {
                const float4 a = reinterpret_cast<const float4*>(add)[v];
                o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
            }
            reinterpret_cast<float4*>(gx)[v] = o;
        }
        for (long long t = (n4 << 2) + i; t < n; t += stride) gx[t] = ADD ? add[t] + elu_b(gy[t], y[t]) : elu_b(gy[t], y[t]);
    } else {
        for (; i < n; i += stride) gx[i] = ADD ? add[i] + elu_b(gy[i], y[i]) : elu_b(gy[i], y[i]);
    }
}

// ---- global norm: part[b] = sum of g^2 over block b's grid-stride share (fp64), then one workgroup sums the partials in index order
constexpr int NORM_BLOCKS = 256;

__device__ __forceinline__ double block_sum(double v, double* red) {      // fixed-order tree over the workgroup's TPB values
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(TPB) void sumsq_partial_kernel(const float* __restrict__ g, long long n, double* __restrict__ part) {
    __shared__ double red[TPB];
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    double acc = 0.;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const long long n4 = n >> 2;
        for (long long v = i; v < n4; v += stride) {
            const float4 a = reinterpret_cast<const float4*>(g)[v];
            acc += (double)a.x * a.x; acc += (double)a.y * a.y; acc += (double)a.z * a.z; acc += (double)a.w * a.w;
        }
        for (long long t = (n4 << 2) + i; t < n; t += stride) acc += (double)g[t] * g[t];
    } else {
        for (long long t = i; t < n; t += stride) acc += (double)g[t] * g[t];
    }
    const double tot = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(TPB) void norm_final_kernel(const double* __restrict__ part, int nblocks, float* __restrict__ norm) {
    __shared__ double red[TPB];
    double acc = 0.;
    for (int k = threadIdx.x; k < nblocks; k += TPB) acc += part[k];
    const double tot = block_sum(acc, red);
    if (threadIdx.x == 0) norm[0] = (float)sqrt(tot);
}

// g *= clip / max(norm, clip): tf.clip_by_global_norm with use_norm (1 exactly while the norm is within the clip)
__global__ void clip_scale_kernel(float* __restrict__ g, long long n, const float* __restrict__ norm, float clip) {
    const float f = clip / fmaxf(norm[0], clip);
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const long long n4 = n >> 2;
        for (long long v = i; v < n4; v += stride) {
            float4 a = reinterpret_cast<float4*>(g)[v];
            a.x *= f; a.y *= f; a.z *= f; a.w *= f;
            reinterpret_cast<float4*>(g)[v] = a;
        }
        for (long long t = (n4 << 2) + i; t < n; t += stride) g[t] *= f;
    } else {
        for (; i < n; i += stride) g[i] *= f;
    }
}

int norm_blocks(long long n) { return (int)ctgan_blocks((n + 3) / 4, TPB, NORM_BLOCKS); }

}  // namespace

extern "C" {

int ctgan_elu_fwd(const float* x, float* y, int64_t n, ctgan_stream_t stream) {
    if (n < 0 || (n > 0 && (!x || !y))) return ctgan_fail(CTGAN_E_BADARG, "elu_fwd: bad argument");
    if (n == 0) return CTGAN_OK;
    hipLaunchKernelGGL(elu_fwd_kernel, dim3(ctgan_blocks((n + 3) / 4, TPB, 2048)), dim3(TPB), 0, static_cast<hipStream_t>(stream), x, y,
                       (long long)n);
    return ctgan_check_launch("elu_fwd");
}

int ctgan_elu_bwd(const float* gy, const float* y, const float* add, float* gx, int64_t n, ctgan_stream_t stream) {
    if (n < 0 || (n > 0 && (!gy || !y || !gx))) return ctgan_fail(CTGAN_E_BADARG, "elu_bwd: bad argument");
    if (n == 0) return CTGAN_OK;
    const dim3 grid(ctgan_blocks((n + 3) / 4, TPB, 2048));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (add)
        hipLaunchKernelGGL(elu_bwd_kernel<true>, grid, dim3(TPB), 0, st, gy, y, add, gx, (long long)n);
    else
        hipLaunchKernelGGL(elu_bwd_kernel<false>, grid, dim3(TPB), 0, st, gy, y, add, gx, (long long)n);
    return ctgan_check_launch("elu_bwd");
}

size_t ctgan_global_norm_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    return (size_t)norm_blocks(n) * sizeof(double);
}

int ctgan_global_norm(const float* g, int64_t n, float* norm, void* ws, size_t ws_bytes, ctgan_stream_t stream) {
    if (n <= 0 || !g || !norm || !ws) return ctgan_fail(CTGAN_E_BADARG, "global_norm: bad argument");
    if (ws_bytes < ctgan_global_norm_workspace_bytes(n)) return ctgan_fail(CTGAN_E_BADARG, "global_norm: workspace too small");
    if (reinterpret_cast<uintptr_t>(ws) & 7) return ctgan_fail(CTGAN_E_BADARG, "global_norm: workspace not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = norm_blocks(n);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(TPB), 0, st, g, (long long)n, static_cast<double*>(ws));
    int rc = ctgan_check_launch("global_norm_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(TPB), 0, st, static_cast<const double*>(ws), nb, norm);
    return ctgan_check_launch("global_norm_final");
}

int ctgan_clip_by_norm(float* g, int64_t n, const float* norm, float clip, ctgan_stream_t stream) {
    if (n <= 0 || !g || !norm || !(clip > 0.f)) return ctgan_fail(CTGAN_E_BADARG, "clip_by_norm: bad argument");
    hipLaunchKernelGGL(clip_scale_kernel, dim3(ctgan_blocks((n + 3) / 4, TPB, 2048)), dim3(TPB), 0, static_cast<hipStream_t>(stream), g,
                       (long long)n, norm, clip);
    return ctgan_check_launch("clip_by_norm");
}

}  // extern "C"
