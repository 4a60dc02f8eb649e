// ssl_conv.hip - what the convolutional semi-supervised CT classifier (ct_cifar.py; TH/ = CT-GANs/Theano_classifier of the reference,
// TH/CT_CIFAR.py) needs beyond ssl.hip: the weight norm of a transposed-conv filter whose output axis is not the trailing one
// (TH/nn.py:70-81), the data-dependent init on a channels-last map with a nonlinearity and init_stdv (TH/nn.py:85-95), the feature
// consistency term and train_err2 (TH/CT_CIFAR.py:120, :128), the L1 feature matching (:152-156) and the augmenting gather that
// replaces the script's per-image host loop (:48, :211-265).
//
// As in ssl.hip every reduction runs in a fixed order (strided per-thread partial sums, then a fixed LDS combine) and there are no
// float atomics, so a replayed graph is bit-stable.
#include "common.h"
#include "philox.h"
#include "ssl_common.h"

namespace {
using namespace ctgan_philox;
using namespace ctgan_ssl;

constexpr int WG = 256;
// sum over the workgroup in a fixed tree order; every thread receives it
__device__ __forceinline__ float block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = WG / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float t = red[0];
    __syncthreads();
    return t;
}

// ------------------------------------------------------------------------------------------------ weight norm, middle axis
// theta [outer, out, inner] (a [k,k,out,in] transposed-conv filter: outer = k k, inner = in):
// W[a,o,i] = theta[a,o,i] * s[o] / sqrt(eps + sum_{a,i} theta[a,o,i]^2).  One workgroup per output channel; lanes run along `inner`.
__global__ void __launch_bounds__(WG) wn_mid_fwd_kernel(const float* __restrict__ theta, const float* __restrict__ s, int outer, int out, int inner,
                                                        float eps, float* __restrict__ W, float* __restrict__ rnorm) {
    __shared__ float red[WG];
    const int o = blockIdx.x;
    const long long n = (long long)outer * inner;
    float acc = 0.f;
    for (long long e = threadIdx.x; e < n; e += WG) {
        const float t = theta[((e / inner) * out + o) * inner + e % inner];
        acc += t * t;
    }
    const float rn = 1.f / sqrtf(eps + block_sum(acc, red));
    if (threadIdx.x == 0) rnorm[o] = rn;
    const float sc = s[o] * rn;
    for (long long e = threadIdx.x; e < n; e += WG) {
        const long long a = ((e / inner) * out + o) * inner + e % inner;
        W[a] = theta[a] * sc;
    }
}
// d_o = sum gW theta;  gs_o = d_o rn_o;  gtheta = s_o rn_o (gW - theta d_o rn_o^2)   (the contract of wn_bwd_kernel)
__global__ void __launch_bounds__(WG) wn_mid_bwd_kernel(const float* __restrict__ gW, const float* __restrict__ theta, const float* __restrict__ s,
                                                        const float* __restrict__ rnorm, int outer, int out, int inner,
                                                        float* __restrict__ gtheta, float* __restrict__ gs) {
    __shared__ float red[WG];
    const int o = blockIdx.x;
    const long long n = (long long)outer * inner;
    float acc = 0.f;
    for (long long e = threadIdx.x; e < n; e += WG) {
        const long long a = ((e / inner) * out + o) * inner + e % inner;
        acc += gW[a] * theta[a];
    }
    const float d = block_sum(acc, red);
    const float rn = rnorm[o];
    if (threadIdx.x == 0 && gs) gs[o] = d * rn;
    const float sc = s[o] * rn, dr2 = d * rn * rn;
    for (long long e = threadIdx.x; e < n; e += WG) {
        const long long a = ((e / inner) * out + o) * inner + e % inner;
        gtheta[a] = sc * (gW[a] - theta[a] * dr2);
    }
}

// ------------------------------------------------------------------------------------------------ data-dependent init on a map
// y [rows = N H W, C] channels-last, in place: m_c = mean, inv_c = init_stdv / sqrt(mean (y - m_c)^2);  y <- act((y - m_c) inv_c)
// (no b is added in the init pass);  g_c <- g_c inv_c;  b_c <- -m_c inv_c.  act: 0 identity, 1 LeakyReLU(slope), 2 tanh.
__global__ void __launch_bounds__(RED_THREADS) wn_init_map_kernel(float* __restrict__ y, long long rows, int cols, int act, float slope,
                                                                 float init_stdv, float* __restrict__ g, float* __restrict__ b) {
    __shared__ float part[RED_SL][RED_COLS];
    const int cx = threadIdx.x % RED_COLS, sl = threadIdx.x / RED_COLS;
    const long long j = (long long)blockIdx.x * RED_COLS + cx;
    float mean, ssd;
    col_mean_ssd(y, rows, cols, j, part, mean, ssd);
    if (j >= cols) return;
    const float inv = init_stdv / sqrtf(ssd / (float)rows);
    for (long long i = sl; i < rows; i += RED_SL) {
        float v = (y[i * cols + j] - mean) * inv;
        if (act == 1) v = v > 0.f ? v : slope * v;
        else if (act == 2) v = tanhf(v);
        y[i * cols + j] = v;
    }
    if (sl == 0) { g[j] = g[j] * inv; b[j] = -mean * inv; }
}

// ------------------------------------------------------------------------------------------------ feature consistency + train_err2
// f [4B, F] = the features of [lab ; unl ; unl2 ; fake]:  out2[0] = mean_{i,j} (f[B+i,j] - f[2B+i,j])^2;  with logits [4B, nc]:
// out2[1] = mean_{i<B} (max_k logits[i,k] <= 0).  ONE workgroup.
__global__ void __launch_bounds__(WG) featcons_fwd_kernel(const float* __restrict__ f, const float* __restrict__ logits, int B, int F, int nc,
                                                          float* __restrict__ out2) {
    __shared__ float red[WG];
    const long long n = (long long)B * F;
    const float* u = f + n;
    const float* u2 = f + 2 * n;
    float acc = 0.f;
    for (long long e = threadIdx.x; e < n; e += WG) { const float d = u[e] - u2[e]; acc += d * d; }
    const float sq = block_sum(acc, red);
    float cnt = 0.f;
    if (logits)
        for (int i = threadIdx.x; i < B; i += WG) {
            const float* l = logits + (long long)i * nc;
            float mx = l[0];
            for (int k = 1; k < nc; ++k) mx = fmaxf(mx, l[k]);
            cnt += mx <= 0.f ? 1.f : 0.f;
        }
    const float c = block_sum(cnt, red);
    if (threadIdx.x == 0) { out2[0] = sq / (float)n; out2[1] = logits ? c / (float)B : 0.f; }
}
// gf [4B, F] of gout[0] * out2[0]: +-gout[0] * 2 (u - u2) / (B F) on the two unlabelled blocks, zero on the other two
__global__ void featcons_bwd_kernel(const float* __restrict__ f, const float* __restrict__ gout, int B, int F, float* __restrict__ gf) {
    const long long n = (long long)B * F;
    const float sc = gout[0] * 2.f / (float)n;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < 4 * n; e += stride) {
        const long long p = e / n, q = e % n;
        float g = 0.f;
        if (p == 1 || p == 2) { g = sc * (f[n + q] - f[2 * n + q]); if (p == 2) g = -g; }
        gf[e] = g;
    }
}

// ------------------------------------------------------------------------------------------------ L1 feature matching
// f [2B, C]:  diff_j = mean_i f_ij (i < B) - mean_i f_ij (i >= B);  loss = mean_j |diff_j|  (ssl_common.h's body, as ssl.hip's
// featmatch_fwd_kernel)
__global__ void __launch_bounds__(FM_THREADS) featmatch_l1_fwd_kernel(const float* __restrict__ f, int B, int C, float* __restrict__ loss,
                                                                      float* __restrict__ diff) {
    featmatch_fwd_body<true>(f, B, C, loss, diff);
}
// gf = +-gout sign(diff_j) / (C B), zero where diff_j is zero
__global__ void featmatch_l1_bwd_kernel(const float* __restrict__ diff, const float* __restrict__ gout, int B, int C, float* __restrict__ gf) {
    const long long n = 2LL * B * C;
    const float sc = gout[0] / ((float)C * (float)B);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
        const float d = diff[e % C];
        const float g = d > 0.f ? sc : (d < 0.f ? -sc : 0.f);
        gf[e] = e < (long long)B * C ? g : -g;
    }
}

// ------------------------------------------------------------------------------------------------ augmenting gather
// Row r of the output is a win x win window of image idx[r] of the uint8 set [n_data, C, S, S], reflect-padded by `pad` through
// index arithmetic (no padded copy), horizontally flipped or not, converted through the 256-entry table `lut`.  augment != 0: the
// flip is u[3r] > 0.5 and the window offsets are min(int((2 pad + 1) u[3r+1]), 2 pad) (rows) and the same of u[3r+2] (columns), u the
// uniform stream (seed, sid, step) ctgan_rng_uniform writes; augment == 0: the given flip and offsets.  In the reference's
// orientation  out[c, y, x] = P'[c, oy + y, ox + x],  P' the padded image after the flip.  rot != 0 writes the window rotated by 180
// degrees (position (y, x) holds reference position (win-1-y, win-1-x)); cl != 0 writes [win, win, C] per row, else [C, win, win].
// An index outside [0, n_data) reads nothing and writes NaN.  One workgroup per output row.
__device__ __forceinline__ int reflect(int t, int S) { return t < 0 ? -t : (t >= S ? 2 * (S - 1) - t : t); }
__global__ void __launch_bounds__(WG) aug_gather_kernel(const uint8_t* __restrict__ data, const int32_t* __restrict__ idx, int n_data, int C, int S,
                                                        int pad, int win, int augment, int oy0, int ox0, int flip0, int rot, int cl,
                                                        const float* __restrict__ lut, uint64_t seed, uint32_t sid,
                                                        const uint64_t* __restrict__ ctr, float* __restrict__ out) {
    __shared__ int sh[3];
    const long long r = blockIdx.x;
    if (threadIdx.x == 0) {
        int flip = flip0, oy = oy0, ox = ox0;
        if (augment) {
            const uint64_t step = ctr ? ctr[0] : 0;
            float u[3];
            uint32_t c[4];
            long long have = -1;
            for (int k = 0; k < 3; ++k) {
                const long long e = 3 * r + k;
                if ((e >> 2) != have) { have = e >> 2; draw4(seed, sid, step, (uint32_t)have, c); }
                u[k] = u01(c[e & 3]);
            }
            const int noff = 2 * pad + 1;
            flip = u[0] > 0.5f ? 1 : 0;
            oy = min((int)((float)noff * u[1]), noff - 1);
            ox = min((int)((float)noff * u[2]), noff - 1);
        }
        sh[0] = flip; sh[1] = oy; sh[2] = ox;
    }
    __syncthreads();
    const int flip = sh[0], oy = sh[1], ox = sh[2];
    const int src = idx[r];
    const bool bad = src < 0 || src >= n_data;
    const int Wp = S + 2 * pad, n = C * win * win;
    float* o = out + r * n;
    const uint8_t* img = data + (long long)(bad ? 0 : src) * C * S * S;
    for (int e = threadIdx.x; e < n; e += WG) {
        int c, y, x;
        if (cl) { c = e % C; x = (e / C) % win; y = e / (C * win); }
        else { x = e % win; y = (e / win) % win; c = e / (win * win); }
        if (rot) { y = win - 1 - y; x = win - 1 - x; }
        int X = ox + x;
        if (flip) X = Wp - 1 - X;
        const int sy = reflect(oy + y - pad, S), sx = reflect(X - pad, S);
        o[e] = bad ? nan_f() : lut[img[(c * S + sy) * S + sx]];
    }
}

}  // namespace

extern "C" {

int ctgan_wn_mid_fwd(const float* theta, const float* s, int32_t outer, int32_t out, int32_t inner, float eps, float* w, float* rnorm,
                     ctgan_stream_t stream) {
    if (!theta || !s || !w || !rnorm) return ctgan_fail(CTGAN_E_BADARG, "wn_mid_fwd: null pointer");
    if (outer <= 0 || out <= 0 || inner <= 0 || out > (1 << 20) || (long long)outer * out > (1LL << 31) / inner || !(eps >= 0.f))
        return ctgan_fail(CTGAN_E_BADARG, "wn_mid_fwd: bad shape [%d,%d,%d] or eps %g", outer, out, inner, eps);
    hipLaunchKernelGGL(wn_mid_fwd_kernel, dim3((unsigned)out), dim3(WG), 0, S(stream), theta, s, outer, out, inner, eps, w, rnorm);
    return ctgan_check_launch("wn_mid_fwd");
}

int ctgan_wn_mid_bwd(const float* gw, const float* theta, const float* s, const float* rnorm, int32_t outer, int32_t out, int32_t inner,
                     float* gtheta, float* gs, ctgan_stream_t stream) {
    if (!gw || !theta || !s || !rnorm || !gtheta) return ctgan_fail(CTGAN_E_BADARG, "wn_mid_bwd: null pointer");
    if (outer <= 0 || out <= 0 || inner <= 0 || out > (1 << 20) || (long long)outer * out > (1LL << 31) / inner)
        return ctgan_fail(CTGAN_E_BADARG, "wn_mid_bwd: bad shape [%d,%d,%d]", outer, out, inner);
    hipLaunchKernelGGL(wn_mid_bwd_kernel, dim3((unsigned)out), dim3(WG), 0, S(stream), gw, theta, s, rnorm, outer, out, inner, gtheta, gs);
    return ctgan_check_launch("wn_mid_bwd");
}

int ctgan_wn_init_map(float* y, int64_t rows, int32_t cols, int32_t act, float slope, float init_stdv, float* g, float* b,
                      ctgan_stream_t stream) {
    if (!y || !g || !b) return ctgan_fail(CTGAN_E_BADARG, "wn_init_map: null pointer");
    if (rows <= 0 || cols <= 0 || cols > (1 << 21) || rows > (1LL << 40) / cols || act < 0 || act > 2 || !(init_stdv > 0.f))
        return ctgan_fail(CTGAN_E_BADARG, "wn_init_map: bad argument");
    hipLaunchKernelGGL(wn_init_map_kernel, dim3((unsigned)((cols + RED_COLS - 1) / RED_COLS)), dim3(RED_THREADS), 0, S(stream), y, (long long)rows,
                       cols, act, slope, init_stdv, g, b);
    return ctgan_check_launch("wn_init_map");
}

int ctgan_featcons_fwd(const float* f, const float* logits, int32_t b, int32_t fdim, int32_t nc, float* out2, ctgan_stream_t stream) {
    if (!f || !out2) return ctgan_fail(CTGAN_E_BADARG, "featcons_fwd: null pointer");
    if (b <= 0 || fdim <= 0 || b > (1 << 24) || fdim > (1 << 24) || (logits && (nc <= 0 || nc > (1 << 16))))
        return ctgan_fail(CTGAN_E_BADARG, "featcons_fwd: bad shape b %d f %d nc %d", b, fdim, nc);
    hipLaunchKernelGGL(featcons_fwd_kernel, dim3(1), dim3(WG), 0, S(stream), f, logits, b, fdim, nc, out2);
    return ctgan_check_launch("featcons_fwd");
}

int ctgan_featcons_bwd(const float* f, const float* gout, int32_t b, int32_t fdim, float* gf, ctgan_stream_t stream) {
    if (!f || !gout || !gf) return ctgan_fail(CTGAN_E_BADARG, "featcons_bwd: null pointer");
    if (b <= 0 || fdim <= 0 || b > (1 << 24) || fdim > (1 << 24)) return ctgan_fail(CTGAN_E_BADARG, "featcons_bwd: bad shape b %d f %d", b, fdim);
    hipLaunchKernelGGL(featcons_bwd_kernel, dim3(ctgan_blocks(4LL * b * fdim, 256, 2048)), dim3(256), 0, S(stream), f, gout, b, fdim, gf);
    return ctgan_check_launch("featcons_bwd");
}

int ctgan_featmatch_l1_fwd(const float* f, int32_t b, int32_t c, float* loss, float* diff, ctgan_stream_t stream) {
    if (!f || !loss || !diff) return ctgan_fail(CTGAN_E_BADARG, "featmatch_l1_fwd: null pointer");
    if (b <= 0 || c <= 0 || b > (1 << 24) || c > (1 << 24)) return ctgan_fail(CTGAN_E_BADARG, "featmatch_l1_fwd: bad shape b %d c %d", b, c);
    hipLaunchKernelGGL(featmatch_l1_fwd_kernel, dim3(1), dim3(FM_THREADS), 0, S(stream), f, b, c, loss, diff);
    return ctgan_check_launch("featmatch_l1_fwd");
}

int ctgan_featmatch_l1_bwd(const float* diff, const float* gout, int32_t b, int32_t c, float* gf, ctgan_stream_t stream) {
    if (!diff || !gout || !gf) return ctgan_fail(CTGAN_E_BADARG, "featmatch_l1_bwd: null pointer");
    if (b <= 0 || c <= 0 || b > (1 << 24) || c > (1 << 24)) return ctgan_fail(CTGAN_E_BADARG, "featmatch_l1_bwd: bad shape b %d c %d", b, c);
    hipLaunchKernelGGL(featmatch_l1_bwd_kernel, dim3(ctgan_blocks(2LL * b * c, 256, 2048)), dim3(256), 0, S(stream), diff, gout, b, c, gf);
    return ctgan_check_launch("featmatch_l1_bwd");
}

int ctgan_aug_gather(const uint8_t* data, const int32_t* idx, int32_t n_data, int32_t rows, int32_t channels, int32_t size, int32_t pad,
                     int32_t win, int32_t augment, int32_t off_y, int32_t off_x, int32_t flip, int32_t rot180, int32_t channels_last,
                     const float* lut, uint64_t seed, uint64_t stream_id, const uint64_t* ctr, float* out, ctgan_stream_t stream) {
    if (!data || !idx || !lut || !out) return ctgan_fail(CTGAN_E_BADARG, "aug_gather: null pointer");
    if (n_data <= 0 || rows <= 0 || rows > (1 << 24) || channels <= 0 || channels > 16 || size <= 0 || size > 1024 || pad < 0 || pad >= size ||
        win <= 0 || (long long)n_data * channels * size * size > (1LL << 40) || stream_id > 0xffffffffULL)
        return ctgan_fail(CTGAN_E_BADARG, "aug_gather: bad shape n %d rows %d c %d size %d pad %d win %d", n_data, rows, channels, size, pad, win);
    const int wp = size + 2 * pad;
    if (augment ? win > size : (off_y < 0 || off_x < 0 || off_y + win > wp || off_x + win > wp))      // augment: offsets reach 2 pad
        return ctgan_fail(CTGAN_E_BADARG, "aug_gather: window %d at (%d,%d) leaves the padded %d image", win, off_y, off_x, wp);
    hipLaunchKernelGGL(aug_gather_kernel, dim3((unsigned)rows), dim3(WG), 0, S(stream), data, idx, n_data, channels, size, pad, win, augment ? 1 : 0,
                       off_y, off_x, flip ? 1 : 0, rot180 ? 1 : 0, channels_last ? 1 : 0, lut, seed, (uint32_t)stream_id, ctr, out);
    return ctgan_check_launch("aug_gather");
}

}  // extern "C"
