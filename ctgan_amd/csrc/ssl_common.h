// ssl_common.h - what the three semi-supervised CT classifiers' kernel files (ssl.hip, ssl_conv.hip, ssl_te.hip) share: the row
// softmax pieces, the fixed-order reductions and the feature-matching forward.  These fix the rounding of every loss scalar
// (max-subtracted softmax, fixed reduction order, no float atomics - a replayed graph is bit-stable), so each is stated once.
#pragma once
#include "common.h"

namespace ctgan_ssl {

inline hipStream_t S(ctgan_stream_t s) { return static_cast<hipStream_t>(s); }

__device__ __forceinline__ float softplus_f(float t) { return fmaxf(t, 0.f) + log1pf(expf(-fabsf(t))); }
__device__ __forceinline__ float sigmoid_f(float t) {
    const float e = expf(-fabsf(t));
    return t >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
__device__ __forceinline__ float nan_f() { return __int_as_float(0x7fc00000); }

// ------------------------------------------------------------------------------------------------ rows of logits
struct RowStat { float mx, rse, lse; };      // rse = 1 / sum exp(l - mx);  lse = mx + log(sum exp(l - mx))
__device__ __forceinline__ RowStat row_stat(const float* __restrict__ l, int nc) {
    float mx = l[0];
    for (int k = 1; k < nc; ++k) mx = fmaxf(mx, l[k]);
    float se = 0.f;
    for (int k = 0; k < nc; ++k) se += expf(l[k] - mx);
    return {mx, 1.f / se, mx + logf(se)};
}
// softmax(l)_k: from the max-subtracted exponent, not from lse (whose rounding at |l| ~ 80 is 4e-6 relative to a probability)
__device__ __forceinline__ float prob(float l, RowStat s) { return expf(l - s.mx) * s.rse; }
// consistency term of one unlabelled row: ct = mean_k (softmax(u)_k - softmax(u2)_k)^2
__device__ __forceinline__ float row_ct(const float* __restrict__ u, const float* __restrict__ u2, RowStat su, RowStat s2, int nc) {
    float acc = 0.f;
    for (int k = 0; k < nc; ++k) { const float d = prob(u[k], su) - prob(u2[k], s2); acc += d * d; }
    return acc / (float)nc;
}

// ------------------------------------------------------------------------------------------------ column reductions
// Lanes along the contiguous axis (RED_COLS columns per workgroup), RED_SL row slices down the reduced axis.
// 16 columns x 32 row slices: a [784, 1000] weight gives 63 workgroups of 512 threads with 25 rows per thread (64 columns x 16 slices
// left it on 16 workgroups with 49 dependent iterations each: 15 us a launch); a wave covers 16 columns (64 B) of four rows.
constexpr int RED_COLS = 16;      // lanes along the contiguous axis
constexpr int RED_SL = 32;        // row slices per workgroup
constexpr int RED_THREADS = RED_COLS * RED_SL;

// sum of the SL slice partials of column cx, in slice order
template <int SL, int COLS>
__device__ __forceinline__ float combine_slices(float (&part)[SL][COLS], int cx) {
    float t = 0.f;
#pragma unroll
    for (int s = 0; s < SL; ++s) t += part[s][cx];
    return t;
}

// Two passes over column j of the row-major y [rows, cols]: mean_j, then ssd = sum_i (y_ij - mean_j)^2, by thread
// (cx, sl) = (threadIdx.x % COLS, threadIdx.x / COLS) of a COLS x SL workgroup.  A column with j >= cols reads nothing and takes
// part in every barrier.  Row: the type the row index runs in.
template <typename Row, int SL, int COLS>
__device__ __forceinline__ void col_mean_ssd(const float* y, Row rows, int cols, long long j, float (&part)[SL][COLS], float& mean,
                                             float& ssd) {
    const int cx = threadIdx.x % COLS, sl = threadIdx.x / COLS;
    const bool on = j < cols;
    float acc = 0.f;
    if (on) for (Row i = sl; i < rows; i += SL) acc += y[(long long)i * cols + j];
    part[sl][cx] = acc;
    __syncthreads();
    mean = combine_slices(part, cx) / (float)rows;
    __syncthreads();
    acc = 0.f;
    if (on) for (Row i = sl; i < rows; i += SL) { const float d = y[(long long)i * cols + j] - mean; acc += d * d; }
    part[sl][cx] = acc;
    __syncthreads();
    ssd = combine_slices(part, cx);
}

// ------------------------------------------------------------------------------------------------ workgroup tree
// red[q][0] <- the sum of acc[q] over the WG threads of the workgroup, by halving, for each of the NQ quantities
template <int NQ, int WG>
__device__ __forceinline__ void block_tree(float (&red)[NQ][WG], const float (&acc)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int w = WG / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int q = 0; q < NQ; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ feature matching, forward
// f [2B, C] = [f(G(z)) ; f(x)];  diff_j = mean_i f_ij (i < B) - mean_i f_ij (i >= B);  loss = mean_j (L1 ? |diff_j| : diff_j^2).
// ONE workgroup (the loss is a sum over all columns) of 64 columns x 16 row slices that walks the column tiles.
constexpr int FM_COLS = 64, FM_SL = 16, FM_THREADS = FM_COLS * FM_SL;
template <bool L1>
__device__ __forceinline__ void featmatch_fwd_body(const float* __restrict__ f, int B, int C, float* __restrict__ loss,
                                                   float* __restrict__ diff) {
    __shared__ float pg[FM_SL][FM_COLS], pr[FM_SL][FM_COLS];
    __shared__ float sq[FM_COLS];
    const int cx = threadIdx.x % FM_COLS, sl = threadIdx.x / FM_COLS;
    float acc2 = 0.f;
    for (int j0 = 0; j0 < C; j0 += FM_COLS) {
        const int j = j0 + cx;
        float ag = 0.f, ar = 0.f;
        if (j < C)
            for (int i = sl; i < B; i += FM_SL) { ag += f[(long long)i * C + j]; ar += f[(long long)(B + i) * C + j]; }
        pg[sl][cx] = ag; pr[sl][cx] = ar;
        __syncthreads();
        if (sl == 0 && j < C) {
            float tg = 0.f, tr = 0.f;
#pragma unroll
            for (int s = 0; s < FM_SL; ++s) { tg += pg[s][cx]; tr += pr[s][cx]; }
            const float d = tg / (float)B - tr / (float)B;
            diff[j] = d;
            acc2 += L1 ? fabsf(d) : d * d;
        }
        __syncthreads();
    }
    if (sl == 0) sq[cx] = acc2;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < FM_COLS; ++k) t += sq[k];
        loss[0] = t / (float)C;
    }
}

}  // namespace ctgan_ssl
