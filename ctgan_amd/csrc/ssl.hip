// ssl.hip - kernels of the semi-supervised CT classifier (ct_mnist.py; TH/ = CT-GANs/Theano_classifier of the reference):
// weight-normalised dense layers (TH/nn.py:398-430, :250-264), the Gaussian-noise epilogue (TH/nn.py:232-244), the data-dependent
// init (TH/nn.py:421-426), the K-class loss head with the consistency term on softmax outputs (TH/CT_MNIST.py:70-90), the
// feature-matching head (:92-94), the generator's 2-D batch norm + softplus (TH/nn.py:176-216) and Theano-form Adam with the
// parameter average fused (TH/nn.py:30-47, TH/CT_MNIST.py:104-105).
//
// Every reduction runs in a fixed order (per-thread strided partial sums, then a fixed LDS combine): no float atomics, so a
// replayed graph is bit-stable.  Column reductions put lanes along the contiguous `out` axis (RED_COLS columns per workgroup) and
// RED_SL row slices down the reduced axis; they, the row softmax pieces and the feature-matching forward are ssl_common.h's.
#include "common.h"
#include "philox.h"
#include "ssl_common.h"

namespace {
using namespace ctgan_philox;
using namespace ctgan_ssl;

// ------------------------------------------------------------------------------------------------ weight norm
// W[i,j] = theta[i,j] * s[j] / sqrt(eps + sum_i theta[i,j]^2)
__global__ void __launch_bounds__(RED_THREADS) wn_fwd_kernel(const float* __restrict__ theta, const float* __restrict__ s, int in, int out,
                                                             float eps, float* __restrict__ W, float* __restrict__ rnorm) {
    __shared__ float part[RED_SL][RED_COLS];
    const int cx = threadIdx.x % RED_COLS, sl = threadIdx.x / RED_COLS;
    const long long j = (long long)blockIdx.x * RED_COLS + cx;
    float acc = 0.f;
    if (j < out)
        for (int i = sl; i < in; i += RED_SL) { const float t = theta[(long long)i * out + j]; acc += t * t; }
    part[sl][cx] = acc;
    __syncthreads();
    if (j >= out) return;
    const float rn = 1.f / sqrtf(eps + combine_slices(part, cx));
    if (sl == 0) rnorm[j] = rn;
    const float sc = s[j] * rn;
    for (int i = sl; i < in; i += RED_SL) W[(long long)i * out + j] = theta[(long long)i * out + j] * sc;
}
// d_j = sum_i gW_ij theta_ij;  gs_j = d_j rn_j;  gtheta_ij = s_j rn_j (gW_ij - theta_ij d_j rn_j^2)
__global__ void __launch_bounds__(RED_THREADS) wn_bwd_kernel(const float* __restrict__ gW, const float* __restrict__ theta,
                                                             const float* __restrict__ s, const float* __restrict__ rnorm, int in, int out,
                                                             float* __restrict__ gtheta, float* __restrict__ gs) {
    __shared__ float part[RED_SL][RED_COLS];
    const int cx = threadIdx.x % RED_COLS, sl = threadIdx.x / RED_COLS;
    const long long j = (long long)blockIdx.x * RED_COLS + cx;
    float acc = 0.f;
    if (j < out)
        for (int i = sl; i < in; i += RED_SL) acc += gW[(long long)i * out + j] * theta[(long long)i * out + j];
    part[sl][cx] = acc;
    __syncthreads();
    if (j >= out) return;
    const float d = combine_slices(part, cx);
    const float rn = rnorm[j];
    if (sl == 0 && gs) gs[j] = d * rn;
    const float sc = s[j] * rn, dr2 = d * rn * rn;
    for (int i = sl; i < in; i += RED_SL) {
        const long long e = (long long)i * out + j;
        gtheta[e] = sc * (gW[e] - theta[e] * dr2);
    }
}

// ------------------------------------------------------------------------------------------------ dense epilogue
// a = relu ? max(y + b, 0) : y + b;  h = a + sigma * N(0,1).  Element (r, c) of the [rows, cols] tensor draws value
// (row_offset + r) * cols + c of the normal stream (seed, sid, step) - exactly what ctgan_rng_normal writes there - so a pass
// that is one row block of a stacked batch sees the numbers a launch of its own with that row offset would.
__global__ void dense_noise_fwd_kernel(const float* __restrict__ y, const float* __restrict__ bias, long long n, int cols, int relu, float sigma,
                                       uint64_t seed, uint32_t sid, const uint64_t* __restrict__ ctr, long long first,
                                       float* __restrict__ h, float* __restrict__ a_out) {
    const uint64_t step = ctr ? ctr[0] : 0;
    const long long b0 = first >> 2, nblk = ((first + n + 3) >> 2) - b0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const bool noisy = sigma != 0.f;
    for (long long bb = (long long)blockIdx.x * blockDim.x + threadIdx.x; bb < nblk; bb += stride) {
        const long long b = b0 + bb;
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (noisy) {
            uint32_t c[4];
            draw4(seed, sid, step, (uint32_t)b, c);
#pragma unroll
            for (int k = 0; k < 2; ++k) {   // Box-Muller on (c[2k], c[2k+1]), as rng_normal_kernel
                const float u1 = ((float)(c[2 * k] >> 8) + 0.5f) * (1.0f / 16777216.0f);
                const float u2 = u01(c[2 * k + 1]);
                const float r = sqrtf(-2.f * logf(u1));
                float sn, cs;
                sincosf(6.283185307179586f * u2, &sn, &cs);
                z[2 * k] = r * cs; z[2 * k + 1] = r * sn;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = b * 4 + k - first;
            if (i < 0 || i >= n) continue;
            float v = y[i];
            if (bias) v += bias[i % cols];
            if (relu) v = fmaxf(v, 0.f);
            if (a_out) a_out[i] = v;
            h[i] = noisy ? v + sigma * z[k] : v;
        }
    }
}
// gz = (gh + ga) where y + b > 0 (relu) else gh + ga;  gb_j = sum_i gz_ij.  No noise tensor exists: the noise is additive.
__global__ void __launch_bounds__(RED_THREADS) dense_noise_bwd_kernel(const float* __restrict__ gh, const float* __restrict__ ga,
                                                                      const float* __restrict__ y, const float* __restrict__ bias, long long rows,
                                                                      int cols, int relu, float* __restrict__ gz, float* __restrict__ gb) {
    __shared__ float part[RED_SL][RED_COLS];
    const int cx = threadIdx.x % RED_COLS, sl = threadIdx.x / RED_COLS;
    const long long j = (long long)blockIdx.x * RED_COLS + cx;
    float acc = 0.f;
    if (j < cols) {
        const float bj = bias ? bias[j] : 0.f;
        for (long long i = sl; i < rows; i += RED_SL) {
            const long long e = i * cols + j;
            float g = (gh ? gh[e] : 0.f) + (ga ? ga[e] : 0.f);
            if (relu && !(y[e] + bj > 0.f)) g = 0.f;
            gz[e] = g;
            acc += g;
        }
    }
    part[sl][cx] = acc;
    __syncthreads();
    if (j < cols && sl == 0 && gb) gb[j] = combine_slices(part, cx);
}

// ------------------------------------------------------------------------------------------------ data-dependent init
// y <- (y - mean_j) / stdv_j [relu], stdv_j = sqrt(mean_i (y_ij - mean_j)^2);  s_j <- s_j / stdv_j;  b_j <- -mean_j / stdv_j
__global__ void __launch_bounds__(RED_THREADS) wn_init_kernel(float* __restrict__ y, long long rows, int cols, int relu, float* __restrict__ s,
                                                              float* __restrict__ b) {
    __shared__ float part[RED_SL][RED_COLS];
    const int cx = threadIdx.x % RED_COLS, sl = threadIdx.x / RED_COLS;
    const long long j = (long long)blockIdx.x * RED_COLS + cx;
    float mean, ssd;
    col_mean_ssd(y, rows, cols, j, part, mean, ssd);
    if (j >= cols) return;
    const float stdv = sqrtf(ssd / (float)rows);
    for (long long i = sl; i < rows; i += RED_SL) {
        float v = (y[i * cols + j] - mean) / stdv;
        if (relu) v = fmaxf(v, 0.f);
        y[i * cols + j] = v;
    }
    if (sl == 0) { s[j] = s[j] / stdv; b[j] = -mean / stdv; }
}

// ------------------------------------------------------------------------------------------------ semi-supervised loss head
constexpr int HEAD_THREADS = 256;
// logits [4B, nc] = [lab ; unl ; unl2 ; fake];  out = {loss_lab, loss_unl, CT, train_err};  one workgroup
__global__ void __launch_bounds__(HEAD_THREADS) ssl_head_fwd_kernel(const float* __restrict__ lg, const int32_t* __restrict__ labels, int B, int nc,
                                                                    float lam2, float M, float* __restrict__ out, float* __restrict__ ct_i) {
    __shared__ float red[5][HEAD_THREADS];
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < B; i += HEAD_THREADS) {
        const float* l = lg + (long long)i * nc;
        const float* u = lg + (long long)(B + i) * nc;
        const float* u2 = lg + (long long)(2 * B + i) * nc;
        const float* f = lg + (long long)(3 * B + i) * nc;
        const RowStat sl = row_stat(l, nc), su = row_stat(u, nc), s2 = row_stat(u2, nc), sf = row_stat(f, nc);
        const int yi = labels[i];
        const float ly = (yi >= 0 && yi < nc) ? l[yi] : nan_f();      // a label outside [0, nc) poisons the loss, reads nothing
        int am = 0;
        for (int k = 1; k < nc; ++k) if (l[k] > l[am]) am = k;                               // first maximum, as argmax
        const float ct = row_ct(u, u2, su, s2, nc);
        ct_i[i] = ct;
        acc[0] += sl.lse - ly;
        acc[1] += fmaxf(lam2 * ct - M, 0.f);
        acc[2] += softplus_f(su.lse) - su.lse;
        acc[3] += softplus_f(sf.lse);
        acc[4] += am != yi ? 1.f : 0.f;
    }
    block_tree(red, acc);
    if (threadIdx.x == 0) {
        const float inv = 1.f / (float)B;
        const float CT = red[1][0] * inv;
        out[0] = red[0][0] * inv;
        out[1] = 0.5f * (CT + red[2][0] * inv + red[3][0] * inv);
        out[2] = CT;
        out[3] = red[4][0] * inv;
    }
}
// glogits [4B, nc] of gout[0] * loss_lab + gout[1] * loss_unl; one thread per row of the stacked batch
__global__ void ssl_head_bwd_kernel(const float* __restrict__ lg, const int32_t* __restrict__ labels, const float* __restrict__ gout, int B, int nc,
                                    float lam2, float M, float* __restrict__ gl) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 4LL * B) return;
    const int p = (int)(r / B), i = (int)(r % B);
    const float g_lab = gout[0] / (float)B, g_unl = 0.5f * gout[1] / (float)B;
    const float* l = lg + r * nc;
    float* o = gl + r * nc;
    const RowStat sr = row_stat(l, nc);
    if (p == 0) {
        const int yi = labels[i];
        for (int k = 0; k < nc; ++k) o[k] = g_lab * (prob(l[k], sr) - (k == yi ? 1.f : 0.f));
    } else if (p == 3) {
        const float sg = g_unl * sigmoid_f(sr.lse);
        for (int k = 0; k < nc; ++k) o[k] = sg * prob(l[k], sr);
    } else {
        const float* u = lg + (long long)(B + i) * nc;
        const float* u2 = lg + (long long)(2 * B + i) * nc;
        const RowStat su = row_stat(u, nc), s2 = row_stat(u2, nc);
        const float ct = row_ct(u, u2, su, s2, nc);
        const float w = (lam2 * ct - M > 0.f) ? g_unl * lam2 * 2.f / (float)nc : 0.f;       // d hinge / d (p_k - q_k) = w (p_k - q_k)
        const float sign = p == 1 ? 1.f : -1.f;
        float dot = 0.f;                                                                     // sum_m (p_m - q_m) * own_m
        for (int k = 0; k < nc; ++k) { const float pk = prob(u[k], su), qk = prob(u2[k], s2); dot += (pk - qk) * (p == 1 ? pk : qk); }
        const float slse = p == 1 ? g_unl * (sigmoid_f(su.lse) - 1.f) : 0.f;               // d (softplus(lse) - lse) / d lse
        for (int k = 0; k < nc; ++k) {
            const float pk = prob(u[k], su), qk = prob(u2[k], s2);
            const float own = p == 1 ? pk : qk;
            o[k] = slse * own + sign * w * own * ((pk - qk) - dot);
        }
    }
}

// ------------------------------------------------------------------------------------------------ feature matching
// loss = mean_j diff_j^2 (ssl_common.h's body)
__global__ void __launch_bounds__(FM_THREADS) featmatch_fwd_kernel(const float* __restrict__ f, int B, int C, float* __restrict__ loss,
                                                                   float* __restrict__ diff) {
    featmatch_fwd_body<false>(f, B, C, loss, diff);
}
__global__ void featmatch_bwd_kernel(const float* __restrict__ diff, const float* __restrict__ gout, int B, int C, float* __restrict__ gf) {
    const long long n = 2LL * B * C;
    const float sc = gout[0] * 2.f / ((float)C * (float)B);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const float g = sc * diff[e % C];
        gf[e] = e < (long long)B * C ? g : -g;
    }
}

// ------------------------------------------------------------------------------------------------ 2-D batch norm (+ softplus)
// xhat = (x - mean_j) * rstd_j, rstd_j = 1 / sqrt(eps + mean_i (x_ij - mean_j)^2);  t = xhat + offset_j;  y = act ? softplus(t) : t
__global__ void __launch_bounds__(RED_THREADS) bn2d_fwd_kernel(const float* __restrict__ x, const float* __restrict__ offset, int B, int C, float eps,
                                                               int act, float* __restrict__ y, float* __restrict__ xhat, float* __restrict__ rstd) {
    __shared__ float part[RED_SL][RED_COLS];
    const int cx = threadIdx.x % RED_COLS, sl = threadIdx.x / RED_COLS;
    const long long j = (long long)blockIdx.x * RED_COLS + cx;
    float mean, ssd;
    col_mean_ssd(x, B, C, j, part, mean, ssd);
    if (j >= C) return;
    const float rs = 1.f / sqrtf(eps + ssd / (float)B);
    if (sl == 0) rstd[j] = rs;
    const float bj = offset ? offset[j] : 0.f;
    for (int i = sl; i < B; i += RED_SL) {
        const long long e = (long long)i * C + j;
        const float xh = (x[e] - mean) * rs;
        xhat[e] = xh;
        const float t = xh + bj;
        y[e] = act ? softplus_f(t) : t;
    }
}
// gt = gy * (act ? sigmoid(t) : 1);  goffset_j = sum_i gt_ij;  gx = rstd_j (gt - mean_i gt - xhat mean_i (gt xhat))
__global__ void __launch_bounds__(RED_THREADS) bn2d_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ xhat,
                                                               const float* __restrict__ offset, const float* __restrict__ rstd, int B, int C, int act,
                                                               float* __restrict__ gx, float* __restrict__ goffset) {
    __shared__ float p1[RED_SL][RED_COLS], p2[RED_SL][RED_COLS];
    const int cx = threadIdx.x % RED_COLS, sl = threadIdx.x / RED_COLS;
    const long long j = (long long)blockIdx.x * RED_COLS + cx;
    const bool on = j < C;
    const float bj = (on && offset) ? offset[j] : 0.f;
    float a1 = 0.f, a2 = 0.f;
    if (on)
        for (int i = sl; i < B; i += RED_SL) {
            const long long e = (long long)i * C + j;
            const float xh = xhat[e];
            const float gt = act ? gy[e] * sigmoid_f(xh + bj) : gy[e];
            a1 += gt; a2 += gt * xh;
        }
    p1[sl][cx] = a1; p2[sl][cx] = a2;
    __syncthreads();
    if (!on) return;
    const float s1 = combine_slices(p1, cx), s2 = combine_slices(p2, cx);
    if (sl == 0 && goffset) goffset[j] = s1;
    const float m1 = s1 / (float)B, m2 = s2 / (float)B, rs = rstd[j];
    for (int i = sl; i < B; i += RED_SL) {
        const long long e = (long long)i * C + j;
        const float xh = xhat[e];
        const float gt = act ? gy[e] * sigmoid_f(xh + bj) : gy[e];
        gx[e] = rs * (gt - m1 - xh * m2);
    }
}

// ------------------------------------------------------------------------------------------------ Theano-form Adam + average
// m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr (m / (1-b1^t)) / sqrt(v / (1-b2^t) + eps);  avg += rate (p - avg)
// state = {lr, b1^t, b2^t, skipped} as adam_kernel's; a non-finite gradient leaves its element's p, m, v untouched and is counted.
__global__ void adam_theano_kernel(float* __restrict__ th, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                   float* __restrict__ avg, long long n, float* state, float b1, float b2, float eps, float rate) {
#pragma clang fp contract(off)
    const float lr = state[0], c1 = 1.f - state[1], c2 = 1.f - state[2];
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        float p = th[i];
        if (!(fabsf(gi) <= 3.0e38f)) {
            atomicAdd(state + 3, 1.0f);
        } else {
            const float mi = b1 * m[i] + (1.f - b1) * gi;
            const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
            m[i] = mi; v[i] = vi;
            p = p - lr * (mi / c1) / sqrtf(vi / c2 + eps);
            th[i] = p;
        }
        if (avg) { const float a = avg[i]; avg[i] = a + rate * (p - a); }
    }
}

inline unsigned col_blocks(long long cols) { return (unsigned)((cols + RED_COLS - 1) / RED_COLS); }
constexpr long long MAX_COLS = 1LL << 21;      // grid.x of the column kernels stays far below the launch limit

}  // namespace

extern "C" {

int ctgan_wn_fwd(const float* theta, const float* s, int32_t in, int32_t out, float eps, float* w, float* rnorm, ctgan_stream_t stream) {
    if (!theta || !s || !w || !rnorm) return ctgan_fail(CTGAN_E_BADARG, "wn_fwd: null pointer");
    if (in <= 0 || out <= 0 || out > MAX_COLS || !(eps >= 0.f)) return ctgan_fail(CTGAN_E_BADARG, "wn_fwd: bad shape [%d,%d] or eps %g", in, out, eps);
    hipLaunchKernelGGL(wn_fwd_kernel, dim3(col_blocks(out)), dim3(RED_THREADS), 0, S(stream), theta, s, in, out, eps, w, rnorm);
    return ctgan_check_launch("wn_fwd");
}

int ctgan_wn_bwd(const float* gw, const float* theta, const float* s, const float* rnorm, int32_t in, int32_t out, float* gtheta, float* gs,
                 ctgan_stream_t stream) {
    if (!gw || !theta || !s || !rnorm || !gtheta) return ctgan_fail(CTGAN_E_BADARG, "wn_bwd: null pointer");
    if (in <= 0 || out <= 0 || out > MAX_COLS) return ctgan_fail(CTGAN_E_BADARG, "wn_bwd: bad shape [%d,%d]", in, out);
    hipLaunchKernelGGL(wn_bwd_kernel, dim3(col_blocks(out)), dim3(RED_THREADS), 0, S(stream), gw, theta, s, rnorm, in, out, gtheta, gs);
    return ctgan_check_launch("wn_bwd");
}

int ctgan_dense_noise_fwd(const float* y, const float* bias, int64_t rows, int32_t cols, int32_t relu, float sigma, uint64_t seed,
                          uint64_t stream_id, const uint64_t* ctr, int64_t row_offset, float* h, float* a, ctgan_stream_t stream) {
    if (!y || !h) return ctgan_fail(CTGAN_E_BADARG, "dense_noise_fwd: null pointer");
    if (rows <= 0 || cols <= 0 || row_offset < 0 || !(sigma >= 0.f)) return ctgan_fail(CTGAN_E_BADARG, "dense_noise_fwd: bad shape or sigma");
    const long long n = (long long)rows * cols, first = (long long)row_offset * cols;
    if (rows > (1LL << 40) / cols || row_offset > (1LL << 40) / cols || ((first + n + 3) >> 2) > 0xffffffffLL || stream_id > 0xffffffffULL)
        return ctgan_fail(CTGAN_E_BADARG, "dense_noise_fwd: stream position out of range");
    const long long nblk = ((first + n + 3) >> 2) - (first >> 2);
    hipLaunchKernelGGL(dense_noise_fwd_kernel, dim3(ctgan_blocks(nblk, 256, 2048)), dim3(256), 0, S(stream), y, bias, n, cols, relu, sigma, seed,
                       (uint32_t)stream_id, ctr, first, h, a);
    return ctgan_check_launch("dense_noise_fwd");
}

int ctgan_dense_noise_bwd(const float* gh, const float* ga, const float* y, const float* bias, int64_t rows, int32_t cols, int32_t relu, float* gz,
                          float* gb, ctgan_stream_t stream) {
    if ((!gh && !ga) || !gz || (relu && !y)) return ctgan_fail(CTGAN_E_BADARG, "dense_noise_bwd: null pointer");
    if (rows <= 0 || cols <= 0 || cols > MAX_COLS || rows > (1LL << 40) / cols) return ctgan_fail(CTGAN_E_BADARG, "dense_noise_bwd: bad shape");
    hipLaunchKernelGGL(dense_noise_bwd_kernel, dim3(col_blocks(cols)), dim3(RED_THREADS), 0, S(stream), gh, ga, y, bias, (long long)rows, cols,
                       relu, gz, gb);
    return ctgan_check_launch("dense_noise_bwd");
}

int ctgan_wn_init(float* y, int64_t rows, int32_t cols, int32_t relu, float* s, float* b, ctgan_stream_t stream) {
    if (!y || !s || !b) return ctgan_fail(CTGAN_E_BADARG, "wn_init: null pointer");
    if (rows <= 0 || cols <= 0 || cols > MAX_COLS || rows > (1LL << 40) / cols) return ctgan_fail(CTGAN_E_BADARG, "wn_init: bad shape");
    hipLaunchKernelGGL(wn_init_kernel, dim3(col_blocks(cols)), dim3(RED_THREADS), 0, S(stream), y, (long long)rows, cols, relu, s, b);
    return ctgan_check_launch("wn_init");
}

int ctgan_ssl_head_fwd(const float* logits, const int32_t* labels, int32_t b, int32_t nc, float lam2, float m, float* out4, float* ct_i,
                       ctgan_stream_t stream) {
    if (!logits || !labels || !out4 || !ct_i) return ctgan_fail(CTGAN_E_BADARG, "ssl_head_fwd: null pointer");
    if (b <= 0 || nc <= 0 || b > (1 << 24) || nc > (1 << 16)) return ctgan_fail(CTGAN_E_BADARG, "ssl_head_fwd: bad shape b %d nc %d", b, nc);
    hipLaunchKernelGGL(ssl_head_fwd_kernel, dim3(1), dim3(HEAD_THREADS), 0, S(stream), logits, labels, b, nc, lam2, m, out4, ct_i);
    return ctgan_check_launch("ssl_head_fwd");
}

int ctgan_ssl_head_bwd(const float* logits, const int32_t* labels, const float* gout, int32_t b, int32_t nc, float lam2, float m, float* glogits,
                       ctgan_stream_t stream) {
    if (!logits || !labels || !gout || !glogits) return ctgan_fail(CTGAN_E_BADARG, "ssl_head_bwd: null pointer");
    if (b <= 0 || nc <= 0 || b > (1 << 24) || nc > (1 << 16)) return ctgan_fail(CTGAN_E_BADARG, "ssl_head_bwd: bad shape b %d nc %d", b, nc);
    hipLaunchKernelGGL(ssl_head_bwd_kernel, dim3((unsigned)((4LL * b + 63) / 64)), dim3(64), 0, S(stream), logits, labels, gout, b, nc, lam2, m,
                       glogits);
    return ctgan_check_launch("ssl_head_bwd");
}

int ctgan_featmatch_fwd(const float* f, int32_t b, int32_t c, float* loss, float* diff, ctgan_stream_t stream) {
    if (!f || !loss || !diff) return ctgan_fail(CTGAN_E_BADARG, "featmatch_fwd: null pointer");
    if (b <= 0 || c <= 0 || b > (1 << 24) || c > (1 << 24)) return ctgan_fail(CTGAN_E_BADARG, "featmatch_fwd: bad shape b %d c %d", b, c);
    hipLaunchKernelGGL(featmatch_fwd_kernel, dim3(1), dim3(FM_THREADS), 0, S(stream), f, b, c, loss, diff);
    return ctgan_check_launch("featmatch_fwd");
}

int ctgan_featmatch_bwd(const float* diff, const float* gout, int32_t b, int32_t c, float* gf, ctgan_stream_t stream) {
    if (!diff || !gout || !gf) return ctgan_fail(CTGAN_E_BADARG, "featmatch_bwd: null pointer");
    if (b <= 0 || c <= 0 || b > (1 << 24) || c > (1 << 24)) return ctgan_fail(CTGAN_E_BADARG, "featmatch_bwd: bad shape b %d c %d", b, c);
    hipLaunchKernelGGL(featmatch_bwd_kernel, dim3(ctgan_blocks(2LL * b * c, 256, 2048)), dim3(256), 0, S(stream), diff, gout, b, c, gf);
    return ctgan_check_launch("featmatch_bwd");
}

int ctgan_bn2d_fwd(const float* x, const float* offset, int32_t b, int32_t c, float eps, int32_t act, float* y, float* xhat, float* rstd,
                   ctgan_stream_t stream) {
    if (!x || !y || !xhat || !rstd) return ctgan_fail(CTGAN_E_BADARG, "bn2d_fwd: null pointer");
    if (b <= 0 || c <= 0 || c > MAX_COLS || !(eps >= 0.f) || (act != 0 && act != 1)) return ctgan_fail(CTGAN_E_BADARG, "bn2d_fwd: bad argument");
    hipLaunchKernelGGL(bn2d_fwd_kernel, dim3(col_blocks(c)), dim3(RED_THREADS), 0, S(stream), x, offset, b, c, eps, act, y, xhat, rstd);
    return ctgan_check_launch("bn2d_fwd");
}

int ctgan_bn2d_bwd(const float* gy, const float* xhat, const float* offset, const float* rstd, int32_t b, int32_t c, int32_t act, float* gx,
                   float* goffset, ctgan_stream_t stream) {
    if (!gy || !xhat || !rstd || !gx) return ctgan_fail(CTGAN_E_BADARG, "bn2d_bwd: null pointer");
    if (b <= 0 || c <= 0 || c > MAX_COLS || (act != 0 && act != 1)) return ctgan_fail(CTGAN_E_BADARG, "bn2d_bwd: bad argument");
    hipLaunchKernelGGL(bn2d_bwd_kernel, dim3(col_blocks(c)), dim3(RED_THREADS), 0, S(stream), gy, xhat, offset, rstd, b, c, act, gx, goffset);
    return ctgan_check_launch("bn2d_bwd");
}

int ctgan_adam_theano_step(float* theta, const float* g, float* m, float* v, float* avg, int64_t n, float* state, float beta1, float beta2,
                           float eps, float avg_rate, ctgan_stream_t stream) {
    if (!theta || !g || !m || !v || !state || n < 0) return ctgan_fail(CTGAN_E_BADARG, "adam_theano_step: bad argument");
    if (n == 0) return CTGAN_OK;
    hipLaunchKernelGGL(adam_theano_kernel, dim3(ctgan_blocks(n, 256, 2048)), dim3(256), 0, S(stream), theta, g, m, v, avg, (long long)n, state,
                       beta1, beta2, eps, avg_rate);
    return ctgan_check_launch("adam_theano_step");
}

}  // extern "C"
