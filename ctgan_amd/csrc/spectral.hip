// spectral.hip - spectral normalisation of the weight matrices of one flat parameter bucket (Miyato et al., ICLR 2018; NOT in the
// reference).  A normalised parameter is the stored layout read as M[K, N], N the last axis; its state is u[N], v[K], sigma.
//
//   normalise (one power iteration):  t = M u;  v = t / max(|t|, eps);  s = M^T v;  sigma = |s|;  u <- s / max(sigma, eps);
//                                     Mbar = M / max(sigma, eps)         (segments of the bucket no job owns are copied)
//   gradient (u, v constants):        G = (Gbar - <Gbar, Mbar> v u^T) / max(sigma, eps)   written over Gbar in the gradient bucket
//
// Launch shape.  A job's rows are cut into slices of rows_per_slice(N) rows - a function of N alone - and the (job, slice) pairs of
// the whole bucket are flattened into one grid by the prefix column of the job table.
//   normalise: 1. slice_kernel     per (job, slice): its rows of t (raw, into v), its partial sum of t^2, its partial M^T t
//              2. finish_kernel    per job: the partials in ascending slice order -> v, sigma, u
//              3. rescale_kernel   over the whole bucket: Mbar                      (iterate == 0 runs this one alone)
//   gradient:  1. dot_kernel       per (job, slice): its partial <Gbar, Mbar>
//              2. apply_kernel     per (job, slice): the partials in ascending slice order, then G over its rows
// Every reduction has one fixed order that is relative to the job (lane-strided serial sums, xor butterflies, LDS trees over a fixed
// width): no atomics, and a job's bits do not depend on its offset in the bucket or on what else the table holds.  The per-job kernels
// use 4-byte loads only (segment offsets are only 4-byte aligned); the rescale walks the BUCKET in 16-byte items, which are aligned
// whatever the segments are.  Stores are plain.
//
// Under a dynamic loss scale (`scaler`, the device float[4] of optim_rng.hip: [1] is the flag of a non-finite gradient) an update may be
// dropped on the device.  A dropped update makes no new weight version, so the normalise that follows it must not iterate: dot_kernel
// copies the flag into `hold[0]` (the end-of-step launch clears the flag before normalise runs), and slice_kernel / finish_kernel return
// at once when hold[0] is set - u, v, sigma keep their bits and the rescale rewrites the same theta_bar.  No host code is involved.
#include <math.h>
#include <stdint.h>

#include "common.h"

namespace {

constexpr int TPB = 256;               // threads per workgroup of every kernel here
constexpr int WAVE = 64;
constexpr int N_MAX = 4096;            // widest matrix (u and s are staged in LDS: 16 KiB)
constexpr int ROWS_MAX = 256;          // rows per slice at most: one per thread
constexpr int SLICE_ELEMS = 16384;     // rows_per_slice * N at most (64 KiB of weights per workgroup)
constexpr int THIN_N = 16;             // N <= THIN_N: a thread takes a whole row of t
constexpr float EPS = 1e-12f;
constexpr int HDR = 4, JOB = 8;        // table: int64 {njobs, nslices, scratch floats, tt0} then per job
enum { J_OFF, J_K, J_N, J_UOFF, J_VOFF, J_ROWS, J_SLICE0, J_POFF };   // tt0 / J_POFF: offsets into the scratch, in floats

inline hipStream_t S(ctgan_stream_t s) { return static_cast<hipStream_t>(s); }

inline int rows_per_slice(long long N) {
    long long r = SLICE_ELEMS / N;
    return (int)(r > ROWS_MAX ? ROWS_MAX : r);       // (N <= N_MAX: at least 4)
}

__device__ inline float wave_sum(float x) {          // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int m = WAVE / 2; m > 0; m >>= 1) x += __shfl_xor(x, m, WAVE);
    return x;
}

// fixed-width LDS tree over TPB values; the total is returned to every thread
__device__ inline float block_sum(float x, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
#pragma unroll
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// the job that owns workgroup b of the flattened (job, slice) grid: the last one whose first slice is <= b
__device__ inline int job_of_slice(const long long* tab, long long b) {
    int lo = 0, hi = (int)tab[0] - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[HDR + mid * JOB + J_SLICE0] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// sum of cnt floats at p in one fixed order: lane l of the first wave adds l, l + 64, ... serially, then a butterfly.  Every thread
// gets the total (through *slot, one LDS float).
__device__ inline float ordered_sum(const float* p, long long cnt, float* slot) {
    if (threadIdx.x < WAVE) {
        float a = 0.f;
        for (long long i = threadIdx.x; i < cnt; i += WAVE) a += p[i];
        a = wave_sum(a);
        if (threadIdx.x == 0) *slot = a;
    }
    __syncthreads();
    return *slot;
}

__global__ __launch_bounds__(TPB) void slice_kernel(const float* __restrict__ theta, const long long* __restrict__ tab,
                                                    const float* __restrict__ u, float* __restrict__ v, float* __restrict__ scratch,
                                                    const float* __restrict__ hold) {
    if (hold && hold[0] != 0.f) return;          // (uniform: the update before this call was dropped)
    __shared__ float u_s[N_MAX];
    __shared__ float t_s[ROWS_MAX];
    __shared__ float part_s[TPB];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const long long b = blockIdx.x;
    const long long* job = tab + HDR + job_of_slice(tab, b) * JOB;
    const long long K = job[J_K], sl = b - job[J_SLICE0];
    const int N = (int)job[J_N], R = (int)job[J_ROWS];
    const long long r0 = sl * R;
    const int rows = (int)(K - r0 < R ? K - r0 : R);
    const float* M = theta + job[J_OFF] + r0 * N;
    for (int n = tid; n < N; n += TPB) u_s[n] = u[job[J_UOFF] + n];
    __syncthreads();
    // t = M u over the slice's rows
    if (N <= THIN_N) {
        if (tid < rows) {
            float a = 0.f;
            for (int n = 0; n < N; ++n) a = fmaf(M[(long long)tid * N + n], u_s[n], a);
            t_s[tid] = a;
        }
    } else {
        for (int r = wave; r < rows; r += TPB / WAVE) {
            float a = 0.f;
            for (int n = lane; n < N; n += WAVE) a = fmaf(M[(long long)r * N + n], u_s[n], a);
            a = wave_sum(a);
            if (lane == 0) t_s[r] = a;
        }
    }
    __syncthreads();
    if (tid < rows) v[job[J_VOFF] + r0 + tid] = t_s[tid];
    if (wave == 0) {
        float a = 0.f;
        for (int r = lane; r < rows; r += WAVE) a = fmaf(t_s[r], t_s[r], a);
        a = wave_sum(a);
        if (lane == 0) scratch[tab[3] + b] = a;
    }
    // partial M^T t: CW columns side by side, the slice's rows cut into Q runs; the runs are added in ascending order
    int CW = 1;
    while (CW < N && CW < TPB) CW <<= 1;
    const int Q = TPB / CW, q = tid / CW, c = tid % CW;
    const int rq = (R + Q - 1) / Q;
    const int ra = q * rq, rb = (ra + rq < rows) ? ra + rq : rows;
    float* out = scratch + job[J_POFF] + sl * N;
    for (int n0 = 0; n0 < N; n0 += CW) {
        const int n = n0 + c;
        float a = 0.f;
        if (n < N)
            for (int r = ra; r < rb; ++r) a = fmaf(M[(long long)r * N + n], t_s[r], a);
        __syncthreads();
        part_s[tid] = a;
        __syncthreads();
        if (q == 0 && n < N) {
            float s = part_s[c];
            for (int k = 1; k < Q; ++k) s += part_s[k * CW + c];
            out[n] = s;
        }
    }
}

__global__ __launch_bounds__(TPB) void finish_kernel(const long long* __restrict__ tab, float* __restrict__ u, float* __restrict__ v,
                                                     float* __restrict__ sigma, const float* __restrict__ scratch,
                                                     const float* __restrict__ hold) {
    if (hold && hold[0] != 0.f) return;
    __shared__ float s_s[N_MAX];
    __shared__ float red[TPB];
    __shared__ float slot;
    const int tid = threadIdx.x, j = blockIdx.x;
    const long long* job = tab + HDR + j * JOB;
    const long long K = job[J_K];
    const int N = (int)job[J_N], R = (int)job[J_ROWS];
    const long long slices = (K + R - 1) / R;
    const float tt = ordered_sum(scratch + tab[3] + job[J_SLICE0], slices, &slot);
    const float nt = fmaxf(sqrtf(tt), EPS);
    const float* part = scratch + job[J_POFF];
    float ss = 0.f;
    for (int n = tid; n < N; n += TPB) {
        float a = 0.f;
        for (long long s = 0; s < slices; ++s) a += part[s * N + n];
        a = a / nt;
        s_s[n] = a;
        ss = fmaf(a, a, ss);
    }
    const float sg = sqrtf(block_sum(ss, red));
    const float d = fmaxf(sg, EPS);
    if (tid == 0) sigma[j] = sg;
    for (int n = tid; n < N; n += TPB) u[job[J_UOFF] + n] = s_s[n] / d;
    float* vj = v + job[J_VOFF];
    for (long long r = tid; r < K; r += TPB) vj[r] = vj[r] / nt;
}

// job owning bucket element i, or -1: jobs are sorted by offset and do not overlap
__device__ inline int job_of_elem(const long long* tab, int nj, long long i) {
    int lo = -1, hi = nj - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[HDR + mid * JOB + J_OFF] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(TPB) void rescale_kernel(const float* __restrict__ theta, float* __restrict__ bar, long long total,
                                                      const long long* __restrict__ tab, const float* __restrict__ sigma) {
    const int nj = (int)tab[0];
    const long long items = (total + 3) >> 2;
    for (long long it = (long long)blockIdx.x * TPB + threadIdx.x; it < items; it += (long long)gridDim.x * TPB) {
        const long long i0 = it * 4;
        int j = job_of_elem(tab, nj, i0);
        long long end = -1, next = total;                 // the current job's end; the next job's start
        float d = 1.f;
        auto enter = [&](int jj) {
            const long long* job = tab + HDR + jj * JOB;
            end = job[J_OFF] + job[J_K] * job[J_N];
            d = fmaxf(sigma[jj], EPS);
        };
        if (j >= 0) enter(j);
        if (j + 1 < nj) next = tab[HDR + (j + 1) * JOB + J_OFF];
        float x[4], y[4];
        const bool full = i0 + 3 < total;
        if (full) {
            const float4 q = *reinterpret_cast<const float4*>(theta + i0);
            x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
        } else {
            for (int k = 0; k < 4; ++k) x[k] = i0 + k < total ? theta[i0 + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = i0 + k;
            if (i >= next && i < total) {
                ++j;
                enter(j);
                next = j + 1 < nj ? tab[HDR + (j + 1) * JOB + J_OFF] : total;
            }
            y[k] = i < end ? x[k] / d : x[k];
        }
        if (full) {
            *reinterpret_cast<float4*>(bar + i0) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (i0 + k < total) bar[i0 + k] = y[k];
        }
    }
}

__global__ __launch_bounds__(TPB) void dot_kernel(const float* __restrict__ g, const float* __restrict__ bar, const long long* __restrict__ tab,
                                                  float* __restrict__ scratch, const float* __restrict__ scaler, float* __restrict__ hold) {
    __shared__ float red[TPB];
    const long long b = blockIdx.x;
    if (hold && b == 0 && threadIdx.x == 0) hold[0] = scaler[1];
    const long long* job = tab + HDR + job_of_slice(tab, b) * JOB;
    const long long K = job[J_K], sl = b - job[J_SLICE0];
    const int N = (int)job[J_N], R = (int)job[J_ROWS];
    const long long r0 = sl * R;
    const int cnt = (int)(K - r0 < R ? K - r0 : R) * N;
    const long long base = job[J_OFF] + r0 * N;
    float a = 0.f;
    for (int e = threadIdx.x; e < cnt; e += TPB) a = fmaf(g[base + e], bar[base + e], a);
    a = block_sum(a, red);
    if (threadIdx.x == 0) scratch[b] = a;
}

__global__ __launch_bounds__(TPB) void apply_kernel(float* __restrict__ g, const long long* __restrict__ tab, const float* __restrict__ u,
                                                    const float* __restrict__ v, const float* __restrict__ sigma,
                                                    const float* __restrict__ scratch) {
    __shared__ float slot;
    const long long b = blockIdx.x;
    const int j = job_of_slice(tab, b);
    const long long* job = tab + HDR + j * JOB;
    const long long K = job[J_K], sl = b - job[J_SLICE0];
    const int N = (int)job[J_N], R = (int)job[J_ROWS];
    const long long r0 = sl * R;
    const int cnt = (int)(K - r0 < R ? K - r0 : R) * N;
    const float dot = ordered_sum(scratch + job[J_SLICE0], (K + R - 1) / R, &slot);
    const float d = fmaxf(sigma[j], EPS);
    float* gj = g + job[J_OFF] + r0 * N;
    const float* uj = u + job[J_UOFF];
    const float* vj = v + job[J_VOFF] + r0;
    for (int e = threadIdx.x; e < cnt; e += TPB) {
        const int r = e / N, n = e - r * N;
        gj[e] = (gj[e] - (dot * vj[r]) * uj[n]) / d;
    }
}

int check_table_args(const char* what, const void* tab, int32_t njobs, int64_t nslices) {
    if (!tab || njobs < 1 || nslices < njobs || nslices > 0x7fffffffLL)
        return ctgan_fail(CTGAN_E_BADARG, "%s: no job table, or njobs %d / nslices %lld out of range", what, njobs, (long long)nslices);
    if (reinterpret_cast<uintptr_t>(tab) & 7) return ctgan_fail(CTGAN_E_BADARG, "%s: the job table is not 8-byte aligned", what);
    return CTGAN_OK;
}

}  // namespace

extern "C" {

int ctgan_spectral_max_n(void) { return N_MAX; }

int64_t ctgan_spectral_table_words(int32_t njobs) { return njobs < 0 ? 0 : HDR + (int64_t)JOB * njobs; }

int ctgan_spectral_table_fill(const int64_t* off, const int64_t* K, const int64_t* N, int32_t njobs, int64_t total, int64_t* table) {
    const char* what = "spectral_table_fill";
    if (!off || !K || !N || !table || njobs < 1 || total < 1) return ctgan_fail(CTGAN_E_BADARG, "%s: bad argument", what);
    for (int j = 0; j < njobs; ++j)
        if (N[j] > N_MAX) return ctgan_fail(CTGAN_E_UNSUPPORTED, "%s: job %d is %lld columns wide (at most %d)", what, j, (long long)N[j], N_MAX);
    long long prev_end = 0, uoff = 0, voff = 0, slice0 = 0, poff = 0;
    for (int j = 0; j < njobs; ++j) {
        if (K[j] < 1 || N[j] < 1 || off[j] < prev_end || K[j] > (total - off[j]) / N[j])
            return ctgan_fail(CTGAN_E_BADARG, "%s: job %d (offset %lld, %lld x %lld) is empty, out of order, overlaps its neighbour or leaves the bucket of %lld",
                              what, j, (long long)off[j], (long long)K[j], (long long)N[j], (long long)total);
        const int R = rows_per_slice(N[j]);
        const long long slices = (K[j] + R - 1) / R;
        int64_t* job = table + HDR + (long long)j * JOB;
        job[J_OFF] = off[j]; job[J_K] = K[j]; job[J_N] = N[j]; job[J_UOFF] = uoff; job[J_VOFF] = voff; job[J_ROWS] = R;
        job[J_SLICE0] = slice0; job[J_POFF] = poff;
        prev_end = off[j] + K[j] * N[j];
        uoff += N[j]; voff += K[j]; slice0 += slices; poff += slices * N[j];
        if (slice0 > 0x7fffffffLL) return ctgan_fail(CTGAN_E_UNSUPPORTED, "%s: more than 2^31 - 1 row slices", what);
    }
    table[0] = njobs; table[1] = slice0; table[2] = poff + slice0; table[3] = poff;
    return CTGAN_OK;
}

size_t ctgan_spectral_scratch_bytes(const int64_t* table) { return table && table[2] > 0 ? (size_t)table[2] * sizeof(float) : 0; }

int ctgan_spectral_normalize(const float* theta, float* theta_bar, int64_t total, const int64_t* table, int32_t njobs, int64_t nslices,
                             float* u, float* v, float* sigma, float* scratch, int32_t iterate, const float* hold, ctgan_stream_t stream) {
    const char* what = "spectral_normalize";
    if (int rc = check_table_args(what, table, njobs, nslices)) return rc;
    if (!theta || !theta_bar || !u || !v || !sigma || !scratch || total < 1) return ctgan_fail(CTGAN_E_BADARG, "%s: bad argument", what);
    if ((reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(theta_bar)) & 15)
        return ctgan_fail(CTGAN_E_BADARG, "%s: theta / theta_bar not 16-byte aligned", what);
    if (theta == theta_bar) return ctgan_fail(CTGAN_E_BADARG, "%s: theta_bar is theta", what);
    const long long* tab = reinterpret_cast<const long long*>(table);
    if (iterate) {
        hipLaunchKernelGGL(slice_kernel, dim3((unsigned)nslices), dim3(TPB), 0, S(stream), theta, tab, u, v, scratch, hold);
        hipLaunchKernelGGL(finish_kernel, dim3((unsigned)njobs), dim3(TPB), 0, S(stream), tab, u, v, sigma, scratch, hold);
    }
    hipLaunchKernelGGL(rescale_kernel, dim3(ctgan_blocks((total + 3) >> 2, TPB, 2048)), dim3(TPB), 0, S(stream), theta, theta_bar,
                       (long long)total, tab, sigma);
    return ctgan_check_launch(what);
}

int ctgan_spectral_grad(float* gbar, const float* theta_bar, const int64_t* table, int32_t njobs, int64_t nslices, const float* u,
                        const float* v, const float* sigma, float* scratch, const float* scaler, float* hold, ctgan_stream_t stream) {
    const char* what = "spectral_grad";
    if (int rc = check_table_args(what, table, njobs, nslices)) return rc;
    if (!gbar || !theta_bar || !u || !v || !sigma || !scratch) return ctgan_fail(CTGAN_E_BADARG, "%s: bad argument", what);
    if ((scaler == nullptr) != (hold == nullptr)) return ctgan_fail(CTGAN_E_BADARG, "%s: scaler and hold come together or not at all", what);
    const long long* tab = reinterpret_cast<const long long*>(table);
    hipLaunchKernelGGL(dot_kernel, dim3((unsigned)nslices), dim3(TPB), 0, S(stream), gbar, theta_bar, tab, scratch, scaler, hold);
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)nslices), dim3(TPB), 0, S(stream), gbar, tab, u, v, sigma, scratch);
    return ctgan_check_launch(what);
}

int ctgan_debug_spectral_launches(int which) { return which == 0 ? 3 : which == 1 ? 1 : which == 2 ? 2 : 0; }

}  // extern "C"
