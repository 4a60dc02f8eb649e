// bn_act.hip - training-mode batch normalisation with the activation that follows it folded into the apply pass and into both passes
// of the backward, and the gated nonlinearity on its own.  The hidden layers of the DCGAN-style 64x64 nets:
//   conv -> Batchnorm -> { LeakyReLU | tanh | sigmoid(a) * tanh(b) }     (TF/CT_gan_64x64.py:237-273, :325-353, :375-399, :435-467)
// x is channels-last [n, hw, c]; the statistics come from ctgan_bn_stats (bn.hip: `groups`, fp64 partial sums, fixed order).
//   z = (x - mean) * rstd * scale + offset
//   CTGAN_ACT_LRELU: y = z > 0 ? z : alpha z          CTGAN_ACT_TANH: y = tanh(z)
//   CTGAN_ACT_GATE : y[.., j] = sigmoid(z[.., 2j]) * tanh(z[.., 2j+1])  - c/2 output channels, the pair adjacent in memory (:95-96, :333)
// Backward: g = act'(z) * gy is recomputed from x and the coefficients in the reduction pass and again in the apply pass (nothing but x,
// mean and rstd is kept from the forward); the partial sums have bn.hip's layout, so its finalisation kernel serves unchanged.
// ReLU stays in bn.hip.  tanhf / expf as elementwise.hip uses them.
#include "common.h"

namespace {

constexpr int CB = 64;      // channels per workgroup of the scalar reduction (bn.hip)
constexpr int RL = 4;       // its row lanes

struct Shape { int n, hw, c, groups, hc, pos; };      // hc / pos: bn.hip's chunk plan (ctgan_bn_plan)

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// y of one element (LRELU / TANH)
template <int ACT>
__device__ __forceinline__ float act1(float z, float alpha) {
    return ACT == CTGAN_ACT_LRELU ? (z > 0.f ? z : alpha * z) : tanhf(z);
}
// g = act'(z) gy of one element (LRELU / TANH)
template <int ACT>
__device__ __forceinline__ float dact1(float z, float gy, float alpha) {
    if (ACT == CTGAN_ACT_LRELU) return z > 0.f ? gy : alpha * gy;
    const float t = tanhf(z);
    return gy * (1.f - t * t);
}
// the gate's two gradients: y = s(a) t(b);  ga = gy s (1 - s) t,  gb = gy s (1 - t^2)
__device__ __forceinline__ void dgate(float a, float b, float gy, float& ga, float& gb) {
    const float s = sigm(a), t = tanhf(b);
    ga = gy * s * (1.f - s) * t;
    gb = gy * s * (1.f - t * t);
}

// the four pre-activations of a thread's channel quad
__device__ __forceinline__ void z4(const float4& v, const float4& mu, const float4& rs, const float4& ga, const float4& be, float xh[4],
                                   float z[4]) {
    xh[0] = (v.x - mu.x) * rs.x; xh[1] = (v.y - mu.y) * rs.y; xh[2] = (v.z - mu.z) * rs.z; xh[3] = (v.w - mu.w) * rs.w;
    z[0] = xh[0] * ga.x + be.x; z[1] = xh[1] * ga.y + be.y; z[2] = xh[2] * ga.z + be.z; z[3] = xh[3] * ga.w + be.w;
}

// g of a channel quad; gyp points at the quad's gradient (4 floats, or the 2 of its two gated outputs)
template <int ACT>
__device__ __forceinline__ void g4(const float z[4], const float* __restrict__ gyp, float alpha, float g[4]) {
    if (ACT == CTGAN_ACT_GATE) {
        const float2 gy = *reinterpret_cast<const float2*>(gyp);
        dgate(z[0], z[1], gy.x, g[0], g[1]);
        dgate(z[2], z[3], gy.y, g[2], g[3]);
    } else {
        const float4 gy = *reinterpret_cast<const float4*>(gyp);
        g[0] = dact1<ACT>(z[0], gy.x, alpha); g[1] = dact1<ACT>(z[1], gy.y, alpha);
        g[2] = dact1<ACT>(z[2], gy.z, alpha); g[3] = dact1<ACT>(z[3], gy.w, alpha);
    }
}

// ---- forward apply --------------------------------------------------------------------------------------------------------------------
// Vector form (c % 4 == 0, (c/4) divides 256): one workgroup per (sample, `apos` positions), a thread owns 4 consecutive channels = two
// gated pairs and keeps their coefficients in registers.  16-byte loads; 16-byte stores (8-byte for the gate's two outputs).
template <int ACT>
__global__ __launch_bounds__(256) void bn_act_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ scale,
                                                               const float* __restrict__ offset, float* __restrict__ y, Shape s, int apos,
                                                               float alpha) {
    const int c4n = s.c >> 2, c4 = threadIdx.x % c4n, pl = threadIdx.x / c4n, pstep = 256 / c4n;
    const int sample = blockIdx.x, p0 = blockIdx.y * apos, p1 = min(s.hw, p0 + apos);
    const int g = sample / (s.n / s.groups);
    const float4 mu = *reinterpret_cast<const float4*>(mean + g * s.c + c4 * 4), rs = *reinterpret_cast<const float4*>(rstd + g * s.c + c4 * 4);
    const float4 ga = *reinterpret_cast<const float4*>(scale + c4 * 4), be = *reinterpret_cast<const float4*>(offset + c4 * 4);
    const long long row0 = (long long)sample * s.hw;
    for (int p = p0 + pl; p < p1; p += pstep) {
        const float4 v = *reinterpret_cast<const float4*>(x + (row0 + p) * s.c + c4 * 4);
        float xh[4], z[4];
        z4(v, mu, rs, ga, be, xh, z);
        if (ACT == CTGAN_ACT_GATE) {
            float2 o;
            o.x = sigm(z[0]) * tanhf(z[1]); o.y = sigm(z[2]) * tanhf(z[3]);
            *reinterpret_cast<float2*>(y + (row0 + p) * (s.c >> 1) + c4 * 2) = o;
        } else {
            float4 o;
            o.x = act1<ACT>(z[0], alpha); o.y = act1<ACT>(z[1], alpha); o.z = act1<ACT>(z[2], alpha); o.w = act1<ACT>(z[3], alpha);
            *reinterpret_cast<float4*>(y + (row0 + p) * s.c + c4 * 4) = o;
        }
    }
}

// Scalar form: one OUTPUT element per step of a grid-stride loop.  The gate's output j of the flat [n hw c/2] result reads the flat
// inputs 2j and 2j+1 (c is even, so a pair never straddles a row).
template <int ACT>
__global__ void bn_act_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                    const float* __restrict__ scale, const float* __restrict__ offset, float* __restrict__ y, Shape s,
                                    float alpha) {
    constexpr int W = ACT == CTGAN_ACT_GATE ? 2 : 1;
    const long long total = (long long)s.n * s.hw * s.c / W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int per = s.n / s.groups;
    const long long hwc = (long long)s.hw * s.c;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
        const long long i = j * W;
        const int c = i % s.c;
        const int g = (int)(i / hwc) / per;
        const float z = (x[i] - mean[g * s.c + c]) * rstd[g * s.c + c] * scale[c] + offset[c];
        if (ACT == CTGAN_ACT_GATE) {
            const float zb = (x[i + 1] - mean[g * s.c + c + 1]) * rstd[g * s.c + c + 1] * scale[c + 1] + offset[c + 1];
            y[j] = sigm(z) * tanhf(zb);
        } else {
            y[j] = act1<ACT>(z, alpha);
        }
    }
}

// ---- backward, pass 1: part[(sample*hc + chunk)][2][c] (double) = sum g, sum g xhat over the chunk's positions (bn.hip's layout) --------
template <int ACT>
__global__ __launch_bounds__(256) void bn_act_bwd_partial_vec_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                     const float* __restrict__ scale, const float* __restrict__ offset,
                                                                     Shape s, float alpha, double* __restrict__ part) {
    __shared__ double red[2][256][4];
    constexpr int GW = ACT == CTGAN_ACT_GATE ? 2 : 1;
    const int c4n = s.c >> 2, rls = 256 / c4n;
    const int c4 = threadIdx.x % c4n, rl = threadIdx.x / c4n;
    const int sample = blockIdx.x / s.hc, chunk = blockIdx.x - sample * s.hc;
    const int p0 = chunk * s.pos, p1 = min(s.hw, p0 + s.pos);
    const int g = sample / (s.n / s.groups);
    const float4 mu = *reinterpret_cast<const float4*>(mean + g * s.c + c4 * 4), rs = *reinterpret_cast<const float4*>(rstd + g * s.c + c4 * 4);
    const float4 ga = *reinterpret_cast<const float4*>(scale + c4 * 4), be = *reinterpret_cast<const float4*>(offset + c4 * 4);
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};      // short per-thread sums in fp32, lanes combined in fp64 (bn.hip)
    const long long row0 = (long long)sample * s.hw;
#pragma unroll 2
    for (int p = p0 + rl; p < p1; p += rls) {
        const float4 v = *reinterpret_cast<const float4*>(x + (row0 + p) * s.c + c4 * 4);
        float xh[4], z[4], gg[4];
        z4(v, mu, rs, ga, be, xh, z);
        g4<ACT>(z, gy + (row0 + p) * (s.c / GW) + c4 * (4 / GW), alpha, gg);
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] += gg[k]; b[k] += gg[k] * xh[k]; }
    }
    double* ra = red[0][threadIdx.x]; double* rb = red[1][threadIdx.x];
#pragma unroll
    for (int k = 0; k < 4; ++k) { ra[k] = a[k]; rb[k] = b[k]; }
    __syncthreads();
    if (rl == 0) {
        double sa[4] = {0., 0., 0., 0.}, sb[4] = {0., 0., 0., 0.};
        for (int r = 0; r < rls; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) { sa[k] += red[0][r * c4n + c4][k]; sb[k] += red[1][r * c4n + c4][k]; }
        double* o = part + (long long)blockIdx.x * 2 * s.c;
#pragma unroll
        for (int k = 0; k < 4; ++k) { o[c4 * 4 + k] = sa[k]; o[s.c + c4 * 4 + k] = sb[k]; }
    }
}

// g and xhat of channel c at row `row` (scalar kernels): the gate reads its partner channel c ^ 1 too
template <int ACT>
__device__ __forceinline__ float g1(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, const float* __restrict__ scale, const float* __restrict__ offset,
                                    long long row, int c, int g, const Shape& s, float alpha, float& xh) {
    const int m = g * s.c + c;
    xh = (x[row * s.c + c] - mean[m]) * rstd[m];
    const float z = xh * scale[c] + offset[c];
    if (ACT != CTGAN_ACT_GATE) return dact1<ACT>(z, gy[row * s.c + c], alpha);
    const int cp = c ^ 1, mp = g * s.c + cp;
    const float zp = (x[row * s.c + cp] - mean[mp]) * rstd[mp] * scale[cp] + offset[cp];
    float da, db;
    const float gv = gy[row * (s.c >> 1) + (c >> 1)];
    if (c & 1) { dgate(zp, z, gv, da, db); return db; }
    dgate(z, zp, gv, da, db);
    return da;
}

template <int ACT>
__global__ __launch_bounds__(CB * RL) void bn_act_bwd_partial_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    const float* __restrict__ scale, const float* __restrict__ offset,
                                                                    Shape s, float alpha, double* __restrict__ part) {
    __shared__ double red[2][RL][CB];
    const int cl = threadIdx.x % CB, rl = threadIdx.x / CB;
    const int c = blockIdx.y * CB + cl;
    const int sample = blockIdx.x / s.hc, chunk = blockIdx.x - sample * s.hc;
    const int p0 = chunk * s.pos, p1 = min(s.hw, p0 + s.pos);
    double a = 0., b = 0.;
    if (c < s.c) {
        const int g = sample / (s.n / s.groups);
        const long long row0 = (long long)sample * s.hw;
        for (int p = p0 + rl; p < p1; p += RL) {
            float xh;
            const float gg = g1<ACT>(gy, x, mean, rstd, scale, offset, row0 + p, c, g, s, alpha, xh);
            a += gg; b += (double)gg * xh;
        }
    }
    red[0][rl][cl] = a; red[1][rl][cl] = b;
    __syncthreads();
    if (rl == 0 && c < s.c) {
        double sa = 0., sb = 0.;
#pragma unroll
        for (int r = 0; r < RL; ++r) { sa += red[0][r][cl]; sb += red[1][r][cl]; }
        double* o = part + (long long)blockIdx.x * 2 * s.c;
        o[c] = sa; o[s.c + c] = sb;
    }
}

// ---- backward, pass 2: gx = rstd (g scale - s1 - xhat s2), s12 = the per-group means of g scale and g scale xhat (bn.hip's finalisation) -
template <int ACT>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_vec_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                                   const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                   const float* __restrict__ scale, const float* __restrict__ offset,
                                                                   const float* __restrict__ s12, float* __restrict__ gx, Shape s, int apos,
                                                                   float alpha) {
    constexpr int GW = ACT == CTGAN_ACT_GATE ? 2 : 1;
    const int c4n = s.c >> 2, c4 = threadIdx.x % c4n, pl = threadIdx.x / c4n, pstep = 256 / c4n;
    const int sample = blockIdx.x, p0 = blockIdx.y * apos, p1 = min(s.hw, p0 + apos);
    const int g = sample / (s.n / s.groups);
    const float4 mu = *reinterpret_cast<const float4*>(mean + g * s.c + c4 * 4), rs = *reinterpret_cast<const float4*>(rstd + g * s.c + c4 * 4);
    const float4 ga = *reinterpret_cast<const float4*>(scale + c4 * 4), be = *reinterpret_cast<const float4*>(offset + c4 * 4);
    const float4 s1 = *reinterpret_cast<const float4*>(s12 + (g * 2 + 0) * s.c + c4 * 4), s2 = *reinterpret_cast<const float4*>(s12 + (g * 2 + 1) * s.c + c4 * 4);
    const long long row0 = (long long)sample * s.hw;
    for (int p = p0 + pl; p < p1; p += pstep) {
        const long long o = (row0 + p) * s.c + c4 * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + o);
        float xh[4], z[4], gg[4];
        z4(v, mu, rs, ga, be, xh, z);
        g4<ACT>(z, gy + (row0 + p) * (s.c / GW) + c4 * (4 / GW), alpha, gg);
        float4 r;
        r.x = rs.x * (gg[0] * ga.x - s1.x - xh[0] * s2.x); r.y = rs.y * (gg[1] * ga.y - s1.y - xh[1] * s2.y);
        r.z = rs.z * (gg[2] * ga.z - s1.z - xh[2] * s2.z); r.w = rs.w * (gg[3] * ga.w - s1.w - xh[3] * s2.w);
        *reinterpret_cast<float4*>(gx + o) = r;
    }
}

template <int ACT>
__global__ void bn_act_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ mean,
                                        const float* __restrict__ rstd, const float* __restrict__ scale, const float* __restrict__ offset,
                                        const float* __restrict__ s12, float* __restrict__ gx, Shape s, float alpha) {
    const long long total = (long long)s.n * s.hw * s.c;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int per = s.n / s.groups;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = i % s.c;
        const long long row = i / s.c;
        const int g = (int)(row / s.hw) / per;
        float xh;
        const float gg = g1<ACT>(gy, x, mean, rstd, scale, offset, row, c, g, s, alpha, xh);
        gx[i] = rstd[g * s.c + c] * (gg * scale[c] - s12[(g * 2 + 0) * s.c + c] - xh * s12[(g * 2 + 1) * s.c + c]);
    }
}

// ---- the gate without a normalisation: flat pairs (x[2j], x[2j+1]) -> y[j] -----------------------------------------------------------------
// quads = n_out / 2 float4 loads; the odd last pair (n_out odd) goes through the scalar tail of the first thread
__global__ void gate_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n_out, int vec) {
    const long long stride = (long long)gridDim.x * blockDim.x, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long quads = vec ? n_out >> 1 : 0;
    for (long long q = t; q < quads; q += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[q];
        float2 o;
        o.x = sigm(v.x) * tanhf(v.y); o.y = sigm(v.z) * tanhf(v.w);
        reinterpret_cast<float2*>(y)[q] = o;
    }
    for (long long j = quads * 2 + t; j < n_out; j += stride) y[j] = sigm(x[2 * j]) * tanhf(x[2 * j + 1]);
}
__global__ void gate_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x, float* __restrict__ gx, long long n_out, int vec) {
    const long long stride = (long long)gridDim.x * blockDim.x, t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long quads = vec ? n_out >> 1 : 0;
    for (long long q = t; q < quads; q += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[q];
        const float2 g = reinterpret_cast<const float2*>(gy)[q];
        float4 r;
        dgate(v.x, v.y, g.x, r.x, r.y);
        dgate(v.z, v.w, g.y, r.z, r.w);
        reinterpret_cast<float4*>(gx)[q] = r;
    }
    for (long long j = quads * 2 + t; j < n_out; j += stride) dgate(x[2 * j], x[2 * j + 1], gy[j], gx[2 * j], gx[2 * j + 1]);
}

bool aligned16(const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}
// the condition of bn.hip's vector kernels (bn_vec_ok): whole channel quads, (c/4) lanes dividing the workgroup
bool vec_ok(const Shape& s) {
    const int c4n = s.c >> 2;
    return (s.c % 4 == 0) && c4n >= 1 && c4n <= 256 && (256 % c4n == 0) && s.hw >= 8;
}
// positions per workgroup of the vector apply passes: 128 as bn.hip's, halved while the grid stays under 1024 workgroups (hw = 16 with a
// few dozen rows would otherwise leave most of the chip idle), never below one step of the workgroup's row lanes
int apply_pos(const Shape& s) {
    const int pstep = 256 / (s.c >> 2);
    int apos = 128;
    while (apos > pstep && (long long)s.n * ((s.hw + apos - 1) / apos) < 1024) apos >>= 1;
    return apos < pstep ? pstep : apos;
}

int check_args(int n, int hw, int c, int groups, int act, const char* who) {
    if (n <= 0 || hw <= 0 || c <= 0 || groups <= 0 || n % groups) return ctgan_fail(CTGAN_E_BADARG, "%s: bad shape", who);
    if (act != CTGAN_ACT_LRELU && act != CTGAN_ACT_TANH && act != CTGAN_ACT_GATE) return ctgan_fail(CTGAN_E_BADARG, "%s: unknown activation %d", who, act);
    if (act == CTGAN_ACT_GATE && (c & 1)) return ctgan_fail(CTGAN_E_BADARG, "%s: the gate pairs channels - c must be even", who);
    return 0;
}
Shape mk(int n, int hw, int c, int groups) {
    Shape s{n, hw, c, groups, 0, 0};
    ctgan_bn_plan(n, hw, &s.hc, &s.pos);
    return s;
}

template <int ACT>
int apply_t(const float* x, const float* mean, const float* rstd, const float* scale, const float* offset, float* y, const Shape& s,
            float alpha, hipStream_t st) {
    if (vec_ok(s) && aligned16(x, mean, rstd) && aligned16(scale, offset, y)) {
        const int apos = apply_pos(s);
        hipLaunchKernelGGL(bn_act_apply_vec_kernel<ACT>, dim3(s.n, (s.hw + apos - 1) / apos), dim3(256), 0, st, x, mean, rstd, scale, offset, y,
                           s, apos, alpha);
        return ctgan_check_launch("bn_act_apply_vec");
    }
    const long long outs = (long long)s.n * s.hw * s.c / (ACT == CTGAN_ACT_GATE ? 2 : 1);
    hipLaunchKernelGGL(bn_act_apply_kernel<ACT>, dim3(ctgan_blocks(outs, 256)), dim3(256), 0, st, x, mean, rstd, scale, offset, y, s, alpha);
    return ctgan_check_launch("bn_act_apply");
}

template <int ACT>
int bwd_t(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale, const float* offset, float* gx,
          float* gscale, float* goffset, const Shape& s, float alpha, double* part, float* s12, hipStream_t st) {
    const bool vec = vec_ok(s) && aligned16(gy, x, mean) && aligned16(rstd, scale, offset) && aligned16(gx, s12, s12);
    if (vec)
        hipLaunchKernelGGL(bn_act_bwd_partial_vec_kernel<ACT>, dim3(s.n * s.hc), dim3(256), 0, st, gy, x, mean, rstd, scale, offset, s, alpha, part);
    else
        hipLaunchKernelGGL(bn_act_bwd_partial_kernel<ACT>, dim3(s.n * s.hc, (s.c + CB - 1) / CB), dim3(CB * RL), 0, st, gy, x, mean, rstd, scale,
                           offset, s, alpha, part);
    int rc = ctgan_check_launch("bn_act_bwd_partial");
    if (rc) return rc;
    rc = ctgan_bn_bwd_finalize(part, scale, s.n, s.hw, s.c, s.groups, gscale, goffset, s12, st);
    if (rc) return rc;
    if (vec) {
        const int apos = apply_pos(s);
        hipLaunchKernelGGL(bn_act_bwd_apply_vec_kernel<ACT>, dim3(s.n, (s.hw + apos - 1) / apos), dim3(256), 0, st, gy, x, mean, rstd, scale,
                           offset, s12, gx, s, apos, alpha);
        return ctgan_check_launch("bn_act_bwd_apply_vec");
    }
    hipLaunchKernelGGL(bn_act_bwd_apply_kernel<ACT>, dim3(ctgan_blocks((long long)s.n * s.hw * s.c, 256)), dim3(256), 0, st, gy, x, mean, rstd,
                       scale, offset, s12, gx, s, alpha);
    return ctgan_check_launch("bn_act_bwd_apply");
}

}  // namespace

extern "C" {

int ctgan_bn_act_apply(const float* x, const float* mean, const float* rstd, const float* scale, const float* offset, float* y, int32_t n,
                       int32_t hw, int32_t c, int32_t groups, int32_t act, float alpha, ctgan_stream_t stream) {
    int rc = check_args(n, hw, c, groups, act, "bn_act_apply");
    if (rc) return rc;
    if (!x || !mean || !rstd || !scale || !offset || !y) return ctgan_fail(CTGAN_E_BADARG, "bn_act_apply: null");
    const Shape s = mk(n, hw, c, groups);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (act == CTGAN_ACT_LRELU) return apply_t<CTGAN_ACT_LRELU>(x, mean, rstd, scale, offset, y, s, alpha, st);
    if (act == CTGAN_ACT_TANH) return apply_t<CTGAN_ACT_TANH>(x, mean, rstd, scale, offset, y, s, alpha, st);
    return apply_t<CTGAN_ACT_GATE>(x, mean, rstd, scale, offset, y, s, alpha, st);
}

int ctgan_bn_act_bwd(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale, const float* offset,
                     float* gx, float* gscale, float* goffset, int32_t n, int32_t hw, int32_t c, int32_t groups, int32_t act, float alpha,
                     void* ws, size_t ws_bytes, ctgan_stream_t stream) {
    int rc = check_args(n, hw, c, groups, act, "bn_act_bwd");
    if (rc) return rc;
    if (!gy || !x || !mean || !rstd || !scale || !offset || !gx || !gscale || !goffset || !ws) return ctgan_fail(CTGAN_E_BADARG, "bn_act_bwd: null");
    const size_t need = ctgan_bn_workspace_bytes(n, hw, c, groups, 1);
    if (ws_bytes < need) return ctgan_fail(CTGAN_E_BADARG, "bn_act_bwd: workspace too small");
    const Shape s = mk(n, hw, c, groups);
    double* part = static_cast<double*>(ws);
    float* s12 = reinterpret_cast<float*>(static_cast<char*>(ws) + need - (size_t)groups * 2 * c * sizeof(float));      // bn.hip's place for it
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (act == CTGAN_ACT_LRELU) return bwd_t<CTGAN_ACT_LRELU>(gy, x, mean, rstd, scale, offset, gx, gscale, goffset, s, alpha, part, s12, st);
    if (act == CTGAN_ACT_TANH) return bwd_t<CTGAN_ACT_TANH>(gy, x, mean, rstd, scale, offset, gx, gscale, goffset, s, alpha, part, s12, st);
    return bwd_t<CTGAN_ACT_GATE>(gy, x, mean, rstd, scale, offset, gx, gscale, goffset, s, alpha, part, s12, st);
}

int ctgan_gate_fwd(const float* x, float* y, int64_t n_out, ctgan_stream_t stream) {
    if (n_out <= 0 || !x || !y) return ctgan_fail(CTGAN_E_BADARG, "gate_fwd: bad argument");
    const int vec = aligned16(x, x, x) && ((reinterpret_cast<uintptr_t>(y) & 7) == 0);
    hipLaunchKernelGGL(gate_fwd_kernel, dim3(ctgan_blocks((n_out + 1) / 2, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y,
                       (long long)n_out, vec);
    return ctgan_check_launch("gate_fwd");
}

int ctgan_gate_bwd(const float* gy, const float* x, float* gx, int64_t n_out, ctgan_stream_t stream) {
    if (n_out <= 0 || !gy || !x || !gx) return ctgan_fail(CTGAN_E_BADARG, "gate_bwd: bad argument");
    const int vec = aligned16(x, gx, gx) && ((reinterpret_cast<uintptr_t>(gy) & 7) == 0);
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(ctgan_blocks((n_out + 1) / 2, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gy, x, gx,
                       (long long)n_out, vec);
    return ctgan_check_launch("gate_bwd");
}

}  // extern "C"
