// diffaug.hip - Differentiable Augmentation (Zhao et al., NeurIPS 2020; NOT in the reference) of the critic's inputs: the policy
// `color,translation,cutout` on flat NCHW fp32 images [n, c, h, w], forward and adjoint in one templated kernel.
//
// Per image r the transformation T is affine:  y = Mask . Shift . Colour(x + b),  Colour = (q I + (1-q) P_img)(s I + (1-s) P_chan),
// P_chan the mean over the channels of a pixel, P_img the mean over the whole image.  Both colour maps are symmetric and commute
// (P_img P_chan = P_chan P_img = P_img), so the adjoint is  gx = Colour(Shift^T Mask g): the same colour arithmetic without b, applied
// AFTER the inverse gather.  Both directions therefore read "gather a source pixel's channels, zero them or not, run the colour
// arithmetic on them"; they differ in the sign of the shift, in where the cut rectangle is tested (forward: at the output position,
// and the zero is written after the colour map; adjoint: at the source position, before it) and in b.
//
// Draws: image r takes values 8r .. 8r+7 of the uniform stream (seed, stream_id, ctr[0]) - blocks 2r, 2r+1 of draw4 through u01, the
// values ctgan_rng_uniform writes there.  With S_h = int(h/8 + .5), k_h = int(h/2 + .5), n_h = h + (1 - k_h % 2) (and the same of w):
//   b = u0 - .5    s = 2 u1    q = u2 + .5
//   ty = min(int((2 S_h + 1) u3), 2 S_h) - S_h               tx the same of u4, w
//   oy = min(int(n_h u5), n_h - 1), rows [oy - k_h/2, oy - k_h/2 + k_h) n [0, h) are cut      columns the same of u6, w
// all in fp32.  A policy bit that is off fixes its parameters at the identity whatever the draws.
//
// Image mean (COLOR only; fixed order, no atomics, the same bits on every run) - the shape the tests derive their tolerance from:
//   lane t of the 256 sums its elements serially in fp32 in ascending address order - scalar path: elements t, t+256, t+512, ...;
//   16-byte path (w % 4 == 0, aligned pointers): quads t, t+256, ... of four consecutive elements, each quad's elements added one by
//   one - at most ceil(n / 1024) * 4 <= n / 256 + 4 additions per lane; then a binary tree over the 256 partials in LDS (8 levels:
//   red[t] += red[t + 128], then 64, ... 1); then ONE division by n.  Depth: ceil(n / 256) + 3 + 8 + 1 roundings.
//   The forward sums the raw input (the image mean of x2 equals that of x1 = x + b: m = mean(x) + b, one more rounding); the adjoint
//   sums the gathered, masked gradient by walking g itself and dropping the elements no output reads.
// The channel mean of a pixel is the serial sum over c = 0 .. C-1 of the (brightened) values, divided by C.
// Per element then  x2 = s x1 + (1 - s) mean_c,  y = q x2 + (1 - q) m.
//
// One workgroup per image.  A 3 x 128 x 128 image (192 KB) does not fit LDS: the second pass reads global memory again, which the first
// pass has just pulled through L2.  16-byte stores whenever w % 4 == 0; 16-byte loads when the shift keeps the source quad aligned
// (tx % 4 == 0), four scalar loads otherwise.  Up to four channels stay in registers between the channel sum and the output; more
// are read a second time (L1 / L2).
#include "common.h"
#include "philox.h"

namespace {
using namespace ctgan_philox;

constexpr int WG = 256;
constexpr uint32_t COLOR = 1, TRANSLATION = 2, CUTOUT = 4;
constexpr int CREG = 4;          // channels kept in registers between the two channel loops

struct Geo {
    float b, s, q;
    int ty, tx;                  // the shift
    int y0, y1, x0, x1;          // the cut rectangle [y0, y1) x [x0, x1), clipped; empty: y0 = y1 = h, x0 = x1 = w
};

__device__ __forceinline__ int half_up(int v, float div) { return (int)((float)v / div + .5f); }

// one element of the input: fp32, or int32 pixels through real_prep_kernel's own expression
template <bool INT>
__device__ __forceinline__ float ld1(const float* __restrict__ x, const int32_t* __restrict__ xi, long long i, float denom) {
    if (INT) return 2.f * (((float)xi[i] / denom) - .5f);
    return x[i];
}
template <bool INT>
__device__ __forceinline__ float4 ld4(const float* __restrict__ x, const int32_t* __restrict__ xi, long long i, float denom) {
    float4 v;
    if (INT) {
        const int4 t = *reinterpret_cast<const int4*>(xi + i);
        v.x = 2.f * (((float)t.x / denom) - .5f); v.y = 2.f * (((float)t.y / denom) - .5f);
        v.z = 2.f * (((float)t.z / denom) - .5f); v.w = 2.f * (((float)t.w / denom) - .5f);
    } else {
        v = *reinterpret_cast<const float4*>(x + i);
    }
    return v;
}

// ADJ: the adjoint; INT: int32 input (forward only); VEC: w % 4 == 0 and 16-byte aligned pointers
template <bool ADJ, bool INT, bool VEC>
__global__ void __launch_bounds__(WG) diffaug_kernel(const float* __restrict__ x, const int32_t* __restrict__ xi, float denom,
                                                     float* __restrict__ y, int C, int H, int W, uint32_t policy, int nobright,
                                                     uint64_t seed, uint32_t sid, const uint64_t* __restrict__ ctr,
                                                     float* __restrict__ params) {
    __shared__ Geo sg;
    __shared__ float red[WG];
    const int tid = threadIdx.x;
    const long long r = blockIdx.x;
    if (tid == 0) {
        const uint64_t step = ctr ? ctr[0] : 0;
        uint32_t c0[4], c1[4];
        draw4(seed, sid, step, (uint32_t)(2 * r), c0);
        draw4(seed, sid, step, (uint32_t)(2 * r + 1), c1);
        Geo g;
        g.b = 0.f; g.s = 1.f; g.q = 1.f; g.ty = 0; g.tx = 0; g.y0 = g.y1 = H; g.x0 = g.x1 = W;
        if (policy & COLOR) {
            g.b = u01(c0[0]) - .5f; g.s = 2.f * u01(c0[1]); g.q = u01(c0[2]) + .5f;
        }
        if (policy & TRANSLATION) {
            const int sh = half_up(H, 8.f), sw = half_up(W, 8.f);
            g.ty = min((int)((float)(2 * sh + 1) * u01(c0[3])), 2 * sh) - sh;
            g.tx = min((int)((float)(2 * sw + 1) * u01(c1[0])), 2 * sw) - sw;
        }
        if (policy & CUTOUT) {
            const int kh = half_up(H, 2.f), kw = half_up(W, 2.f);
            const int nh = H + (1 - kh % 2), nw = W + (1 - kw % 2);
            const int oy = min((int)((float)nh * u01(c1[1])), nh - 1), ox = min((int)((float)nw * u01(c1[2])), nw - 1);
            g.y0 = max(oy - kh / 2, 0); g.y1 = min(oy - kh / 2 + kh, H);
            g.x0 = max(ox - kw / 2, 0); g.x1 = min(ox - kw / 2 + kw, W);
        }
        if (params) {
            float* p = params + r * 8;
            p[0] = g.b; p[1] = g.s; p[2] = g.q; p[3] = (float)g.ty; p[4] = (float)g.tx; p[5] = (float)g.y0; p[6] = (float)g.x0;
            p[7] = (float)policy;
        }
        if (ADJ || nobright) g.b = 0.f;          // (params reports the drawn brightness; the linear part runs without it)
        sg = g;
    }
    __syncthreads();
    const Geo g = sg;
    const bool color = (policy & COLOR) != 0;
    const int HW = H * W, n = C * HW;
    const long long base = r * n;
    // forward: output (i, j) reads source (i - ty, j - tx); adjoint: output (i, j) reads g at (i + ty, j + tx)
    const int dy = ADJ ? g.ty : -g.ty, dx = ADJ ? g.tx : -g.tx;

    float add = 0.f;             // (1 - q) * image mean
    if (color) {
        float acc = 0.f;
        if (VEC) {
            for (int e4 = tid; e4 < (n >> 2); e4 += WG) {
                const int e = e4 << 2;
                const float4 v = ld4<INT>(x, xi, base + e, denom);
                const float vv[4] = {v.x, v.y, v.z, v.w};
                const int p = e % HW, i = p / W, j0 = p % W;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    bool keep = true;
                    if (ADJ) {       // g at (i, j) is read by output (i - ty, j - tx) unless it is cut or that output does not exist
                        const int j = j0 + k;
                        keep = !(i >= g.y0 && i < g.y1 && j >= g.x0 && j < g.x1) && (unsigned)(i - g.ty) < (unsigned)H &&
                               (unsigned)(j - g.tx) < (unsigned)W;
                    }
                    acc += keep ? vv[k] : 0.f;
                }
            }
        } else {
            for (int e = tid; e < n; e += WG) {
                const float v = ld1<INT>(x, xi, base + e, denom);
                bool keep = true;
                if (ADJ) {
                    const int p = e % HW, i = p / W, j = p % W;
                    keep = !(i >= g.y0 && i < g.y1 && j >= g.x0 && j < g.x1) && (unsigned)(i - g.ty) < (unsigned)H &&
                           (unsigned)(j - g.tx) < (unsigned)W;
                }
                acc += keep ? v : 0.f;
            }
        }
        red[tid] = acc;
        __syncthreads();
#pragma unroll
        for (int s = WG / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        const float mean = red[0] / (float)n;
        add = (1.f - g.q) * (mean + g.b);
    }
    const float oms = 1.f - g.s, rc = (float)C;

    // value of one output element from its gathered source value v, the pixel's channel mean mc and the zeroing flags
    auto finish = [&](float v, float mc, bool src_zero, bool out_zero) -> float {
        if (!color) return (src_zero || out_zero) ? 0.f : v;
        if (ADJ) return g.q * (g.s * v + oms * mc) + add;       // v, mc are already zero where the gather found nothing
        return out_zero ? 0.f : g.q * (g.s * v + oms * mc) + add;
    };

    if (VEC) {
        const int W4 = W >> 2, Q = HW >> 2;
        const bool aligned = (dx & 3) == 0;
        for (int q4 = tid; q4 < Q; q4 += WG) {
            const int i = q4 / W4, j0 = (q4 - i * W4) << 2;
            const int si = i + dy, sj0 = j0 + dx;
            const bool rowok = (unsigned)si < (unsigned)H;
            bool zero[4], cut_out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = j0 + k, sj = sj0 + k;
                const bool inb = rowok && (unsigned)sj < (unsigned)W;
                const bool cut_o = i >= g.y0 && i < g.y1 && j >= g.x0 && j < g.x1;
                const bool cut_s = si >= g.y0 && si < g.y1 && sj >= g.x0 && sj < g.x1;
                zero[k] = !inb || (ADJ && cut_s);          // the gather found nothing: the value entering the colour map is 0
                cut_out[k] = !inb || (!ADJ && cut_o);      // forward: the output itself is 0
            }
            const long long soff = base + (long long)si * W + sj0;
            auto load = [&](int c, float (&v)[4]) {
                const long long o = soff + (long long)c * HW;
                if (aligned) {
                    // w % 4 == 0 and dx % 4 == 0: the source quad lies wholly inside the row or wholly outside
                    if (rowok && (unsigned)sj0 < (unsigned)W) {
                        const float4 t = ld4<INT>(x, xi, o, denom);
                        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                    } else {
                        v[0] = v[1] = v[2] = v[3] = 0.f;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = (rowok && (unsigned)(sj0 + k) < (unsigned)W) ? ld1<INT>(x, xi, o + k, denom) : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = zero[k] ? 0.f : (ADJ ? v[k] : v[k] + g.b);
            };
            auto store = [&](int c, const float (&v)[4], const float (&mc)[4]) {
                float4 o;
                o.x = finish(v[0], mc[0], zero[0], cut_out[0]); o.y = finish(v[1], mc[1], zero[1], cut_out[1]);
                o.z = finish(v[2], mc[2], zero[2], cut_out[2]); o.w = finish(v[3], mc[3], zero[3], cut_out[3]);
                *reinterpret_cast<float4*>(y + base + (long long)c * HW + (long long)i * W + j0) = o;
            };
            float mc[4] = {0.f, 0.f, 0.f, 0.f};
            if (C <= CREG) {
                float v[CREG][4];
#pragma unroll
                for (int c = 0; c < CREG; ++c)
                    if (c < C) {
                        load(c, v[c]);
#pragma unroll
                        for (int k = 0; k < 4; ++k) mc[k] += v[c][k];
                    }
#pragma unroll
                for (int k = 0; k < 4; ++k) mc[k] = mc[k] / rc;
#pragma unroll
                for (int c = 0; c < CREG; ++c)
                    if (c < C) store(c, v[c], mc);
            } else {
                float v[4];
                if (color) {
                    for (int c = 0; c < C; ++c) {
                        load(c, v);
#pragma unroll
                        for (int k = 0; k < 4; ++k) mc[k] += v[k];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) mc[k] = mc[k] / rc;
                }
                for (int c = 0; c < C; ++c) {
                    load(c, v);
                    store(c, v, mc);
                }
            }
        }
    } else {
        for (int p = tid; p < HW; p += WG) {
            const int i = p / W, j = p - i * W;
            const int si = i + dy, sj = j + dx;
            const bool inb = (unsigned)si < (unsigned)H && (unsigned)sj < (unsigned)W;
            const bool cut_o = i >= g.y0 && i < g.y1 && j >= g.x0 && j < g.x1;
            const bool cut_s = si >= g.y0 && si < g.y1 && sj >= g.x0 && sj < g.x1;
            const bool zero = !inb || (ADJ && cut_s), cut_out = !inb || (!ADJ && cut_o);
            const long long soff = base + (long long)si * W + sj;
            auto load = [&](int c) -> float {
                if (zero) return 0.f;
                const float v = ld1<INT>(x, xi, soff + (long long)c * HW, denom);
                return ADJ ? v : v + g.b;
            };
            float mc = 0.f;
            if (C <= CREG) {
                float v[CREG];
#pragma unroll
                for (int c = 0; c < CREG; ++c)
                    if (c < C) { v[c] = load(c); mc += v[c]; }
                mc = mc / rc;
#pragma unroll
                for (int c = 0; c < CREG; ++c)
                    if (c < C) y[base + (long long)c * HW + p] = finish(v[c], mc, zero, cut_out);
            } else {
                if (color) {
                    for (int c = 0; c < C; ++c) mc += load(c);
                    mc = mc / rc;
                }
                for (int c = 0; c < C; ++c) y[base + (long long)c * HW + p] = finish(load(c), mc, zero, cut_out);
            }
        }
    }
}

template <bool ADJ, bool INT>
void launch(bool vec, int n, hipStream_t st, const float* x, const int32_t* xi, float denom, float* y, int C, int H, int W, uint32_t policy,
            int nobright, uint64_t seed, uint32_t sid, const uint64_t* ctr, float* params) {
    if (vec)
        hipLaunchKernelGGL((diffaug_kernel<ADJ, INT, true>), dim3((unsigned)n), dim3(WG), 0, st, x, xi, denom, y, C, H, W, policy, nobright, seed,
                           sid, ctr, params);
    else
        hipLaunchKernelGGL((diffaug_kernel<ADJ, INT, false>), dim3((unsigned)n), dim3(WG), 0, st, x, xi, denom, y, C, H, W, policy, nobright, seed,
                           sid, ctr, params);
}

}  // namespace

extern "C" {

int ctgan_diffaug(const float* x, const int32_t* x_int, float denom, float* y, int32_t n, int32_t c, int32_t h, int32_t w, uint32_t policy,
                  int32_t adjoint, uint64_t seed, uint64_t stream_id, const uint64_t* ctr, float* params, ctgan_stream_t stream) {
    if (!y) return ctgan_fail(CTGAN_E_BADARG, "diffaug: null pointer");
    if ((x != nullptr) == (x_int != nullptr)) return ctgan_fail(CTGAN_E_BADARG, "diffaug: exactly one of x and x_int is given");
    if (adjoint < 0 || adjoint > 2) return ctgan_fail(CTGAN_E_BADARG, "diffaug: adjoint %d is not 0, 1 or 2", adjoint);
    if (x_int && adjoint == 1) return ctgan_fail(CTGAN_E_BADARG, "diffaug: the adjoint takes no integer input");
    if (n < 1 || c < 1 || h < 1 || w < 1 || c > 16 || n > (1 << 24) || h > (1 << 14) || w > (1 << 14) || (long long)c * h * w > (1LL << 28))
        return ctgan_fail(CTGAN_E_BADARG, "diffaug: bad shape [%d,%d,%d,%d]", n, c, h, w);
    if (policy > 7u) return ctgan_fail(CTGAN_E_BADARG, "diffaug: policy mask %u has bits outside color | translation | cutout", policy);
    if (stream_id > 0xffffffffULL) return ctgan_fail(CTGAN_E_BADARG, "diffaug: stream id does not fit 32 bits");
    if (denom == 0.f) return ctgan_fail(CTGAN_E_BADARG, "diffaug: denom is 0");
    const void* in = x ? (const void*)x : (const void*)x_int;
    const bool vec = w % 4 == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nobright = adjoint == 2 ? 1 : 0;
    if (adjoint == 1)
        launch<true, false>(vec, n, st, x, x_int, denom, y, c, h, w, policy, 0, seed, (uint32_t)stream_id, ctr, params);
    else if (x_int)
        launch<false, true>(vec, n, st, x, x_int, denom, y, c, h, w, policy, nobright, seed, (uint32_t)stream_id, ctr, params);
    else
        launch<false, false>(vec, n, st, x, x_int, denom, y, c, h, w, policy, nobright, seed, (uint32_t)stream_id, ctr, params);
    return ctgan_check_launch("diffaug");
}

}  // extern "C"
