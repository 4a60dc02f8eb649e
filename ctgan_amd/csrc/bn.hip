// bn.hip - training-mode batch normalisation for the generator.
//   cond_batchnorm.Batchnorm (TF/tflib/ops/cond_batchnorm.py:10-16): moments over (n,h,w),
//     per-sample scale/offset gathered by label from [n_labels, C]
//   batchnorm.Batchnorm fused path (TF/tflib/ops/batchnorm.py:29-30) and axes=[0] path (:77-84)
// x is channels-last [n, hw, c].  `groups` splits the batch into independent statistic groups
// (the reference evaluates one generator tower per device, each with its own batch statistics).
// Reductions are two-stage and fixed-order (deterministic); sums are carried in fp64 because
// E[x^2]-E[x]^2 cancels catastrophically in fp32 for |mean| >> std.
#include "common.h"

namespace {

constexpr int CB = 64;      // channels per workgroup (one 256-byte row segment per wave load)
constexpr int RL = 4;       // row lanes per workgroup
// spatial positions per workgroup of the partial reductions (one partial row each) = BnShape::pos: 256 when that still
// leaves >= 512 workgroups (fewer rows for the finalisation), else 64

struct BnShape { int n, hw, c, groups, hc, pos; };


// part[(sample*hc + chunk)][2][c] (double): sum x, sum x^2 over the chunk's positions
__global__ __launch_bounds__(CB * RL) void bn_stats_partial_kernel(const float* __restrict__ x, BnShape s,
                                                                  double* __restrict__ part) {
    __shared__ double red[2][RL][CB];
    const int cl = threadIdx.x % CB, rl = threadIdx.x / CB;
    const int c = blockIdx.y * CB + cl;
    const int sample = blockIdx.x / s.hc, chunk = blockIdx.x - sample * s.hc;
    const int p0 = chunk * s.pos, p1 = min(s.hw, p0 + s.pos);
    double a = 0., b = 0.;
    if (c < s.c) {
        const float* base = x + ((long long)sample * s.hw) * s.c + c;
        for (int p = p0 + rl; p < p1; p += RL) {
            const double v = base[(long long)p * s.c];
            a += v; b += v * v;
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

constexpr int FL = 16;      // partial-row lanes of the finalisation workgroups
__global__ __launch_bounds__(CB * FL) void bn_stats_final_kernel(const double* __restrict__ part, BnShape s, float eps,
                                                              float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ double red[2][FL][CB];
    const int cl = threadIdx.x % CB, fl = threadIdx.x / CB;
    const int c = blockIdx.x * CB + cl;
    const int g = blockIdx.y;
    const int per = s.n / s.groups;
    double a = 0., b = 0.;
    if (c < s.c) {
        int i = g * per * s.hc + fl;
        const int i1 = (g + 1) * per * s.hc;
        for (; i + 3 * FL < i1; i += 4 * FL) {                 // four independent row loads in flight, summed in the same fixed order
            double va[4], vb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                va[u] = part[(long long)(i + u * FL) * 2 * s.c + c];
                vb[u] = part[(long long)(i + u * FL) * 2 * s.c + s.c + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { a += va[u]; b += vb[u]; }
        }
        for (; i < i1; i += FL) {
            a += part[(long long)i * 2 * s.c + c];
            b += part[(long long)i * 2 * s.c + s.c + c];
        }
    }
    red[0][fl][cl] = a; red[1][fl][cl] = b;
    __syncthreads();
    if (fl != 0 || c >= s.c) return;
    a = 0.; b = 0.;
#pragma unroll
    for (int r = 0; r < FL; ++r) { a += red[0][r][cl]; b += red[1][r][cl]; }
    const double cnt = (double)per * s.hw;
    const double m = a / cnt;
    double var = b / cnt - m * m;
    if (var < 0.) var = 0.;
    mean[g * s.c + c] = (float)m;
    rstd[g * s.c + c] = (float)(1.0 / sqrt(var + (double)eps));
}

__global__ void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                const float* __restrict__ scale, const float* __restrict__ offset,
                                const int32_t* __restrict__ labels, float* __restrict__ y, BnShape s, int relu) {
    const long long total = (long long)s.n * s.hw * s.c;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int per = s.n / s.groups;
    const long long hwc = (long long)s.hw * s.c;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = i % s.c;
        const int sample = i / hwc;
        const int g = sample / per;
        const int lab = labels ? labels[sample] : 0;
        float v = (x[i] - mean[g * s.c + c]) * rstd[g * s.c + c] * scale[lab * s.c + c] + offset[lab * s.c + c];
        if (relu) v = fmaxf(v, 0.f);
        y[i] = v;
    }
}

// part[(sample*hc+chunk)][2][c] (double): sum g, sum g*xhat, with g = relu-masked gy
__global__ __launch_bounds__(CB * RL) void bn_bwd_partial_kernel(
    const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ scale, const float* __restrict__ offset,
    const int32_t* __restrict__ labels, BnShape s, int relu, double* __restrict__ part) {
    __shared__ double red[2][RL][CB];
    const int cl = threadIdx.x % CB, rl = threadIdx.x / CB;
    const int c = blockIdx.y * CB + cl;
    const int sample = blockIdx.x / s.hc, chunk = blockIdx.x - sample * s.hc;
    const int p0 = chunk * s.pos, p1 = min(s.hw, p0 + s.pos);
    double a = 0., b = 0.;
    if (c < s.c) {
        const int g = sample / (s.n / s.groups);
        const int lab = labels ? labels[sample] : 0;
        const float mu = mean[g * s.c + c], rs = rstd[g * s.c + c];
        const float ga = scale[lab * s.c + c], be = offset[lab * s.c + c];
        const long long base = ((long long)sample * s.hw) * s.c + c;
        for (int p = p0 + rl; p < p1; p += RL) {
            const long long o = base + (long long)p * s.c;
            const float xh = (x[o] - mu) * rs;
            float gg = gy[o];
            if (relu && !(xh * ga + be > 0.f)) gg = 0.f;
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

// per-sample totals: tot[sample][2][c] = sum over the sample's chunks   (grid = (n, c/64))
__global__ __launch_bounds__(CB * RL) void bn_bwd_sample_kernel(const double* __restrict__ part, BnShape s,
                                                               double* __restrict__ tot) {
    __shared__ double red[2][RL][CB];
    const int cl = threadIdx.x % CB, rl = threadIdx.x / CB;
    const int c = blockIdx.y * CB + cl, sample = blockIdx.x;
    double a = 0., b = 0.;
    if (c < s.c)
        for (int k = rl; k < s.hc; k += RL) {
            const long long i = (long long)(sample * s.hc + k) * 2 * s.c;
            a += part[i + c]; b += part[i + s.c + c];
        }
    red[0][rl][cl] = a; red[1][rl][cl] = b;
    __syncthreads();
    if (rl == 0 && c < s.c) {
#pragma unroll
        for (int r = 1; r < RL; ++r) { a += red[0][r][cl]; b += red[1][r][cl]; }
        tot[(long long)sample * 2 * s.c + c] = a;
        tot[(long long)sample * 2 * s.c + s.c + c] = b;
    }
}

// Finalisation of the BN backward reductions.  grid = (c/64, n_labels + groups), 64 channels x 16 sample lanes:
//   blockIdx.y <  n_labels : label bin l:  goffset[l][c] = sum_{labels[s]==l} a_s, gscale[l][c] = sum b_s
//   blockIdx.y >= n_labels : group g:      s12[g][{0,1}][c] = sum_s {a_s, b_s} * scale[labels[s]][c] / count
// lanes are combined through LDS in a fixed order (deterministic).
__global__ __launch_bounds__(64 * 16) void bn_bwd_final_kernel(const double* __restrict__ tot, const float* __restrict__ scale,
                                                             const int32_t* __restrict__ labels, BnShape s, int n_labels,
                                                             float* __restrict__ gscale, float* __restrict__ goffset,
                                                             float* __restrict__ s12) {
    __shared__ double red[2][16][64];
    const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int job = blockIdx.y;
    const int per = s.n / s.groups;
    double a = 0., b = 0.;
    if (c < s.c) {
        if (job < n_labels) {
            for (int sample = sl; sample < s.n; sample += 16) {
                const int lab = labels ? labels[sample] : 0;
                if (lab != job) continue;
                for (int k = 0; k < s.hc; ++k) {          // `tot` = the per-chunk partials: hc (<= 4 on this path) rows per sample
                    const long long i = (long long)(sample * s.hc + k) * 2 * s.c;
                    a += tot[i + c]; b += tot[i + s.c + c];
                }
            }
        } else {
            const int g = job - n_labels;
            for (int sample = g * per + sl; sample < (g + 1) * per; sample += 16) {
                const int lab = labels ? labels[sample] : 0;
                const double ga = scale[lab * s.c + c];
                for (int k = 0; k < s.hc; ++k) {
                    const long long i = (long long)(sample * s.hc + k) * 2 * s.c;
                    a += tot[i + c] * ga; b += tot[i + s.c + c] * ga;
                }
            }
        }
    }
    red[0][sl][cl] = a; red[1][sl][cl] = b;
    __syncthreads();
    if (sl != 0 || c >= s.c) return;
    a = 0.; b = 0.;
#pragma unroll
    for (int r = 0; r < 16; ++r) { a += red[0][r][cl]; b += red[1][r][cl]; }
    if (job < n_labels) {
        goffset[job * s.c + c] = (float)a; gscale[job * s.c + c] = (float)b;
    } else {
        const int g = job - n_labels;
        const double cnt = (double)per * s.hw;
        s12[(g * 2 + 0) * s.c + c] = (float)(a / cnt); s12[(g * 2 + 1) * s.c + c] = (float)(b / cnt);
    }
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                    const float* __restrict__ scale, const float* __restrict__ offset,
                                    const int32_t* __restrict__ labels, const float* __restrict__ s12,
                                    float* __restrict__ gx, BnShape s, int relu) {
    const long long total = (long long)s.n * s.hw * s.c;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int per = s.n / s.groups;
    const long long hwc = (long long)s.hw * s.c;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = i % s.c;
        const int sample = i / hwc;
        const int g = sample / per;
        const int lab = labels ? labels[sample] : 0;
        const float rs = rstd[g * s.c + c];
        const float xh = (x[i] - mean[g * s.c + c]) * rs;
        const float ga = scale[lab * s.c + c];
        float gg = gy[i];
        if (relu && !(xh * ga + offset[lab * s.c + c] > 0.f)) gg = 0.f;
        gx[i] = rs * (gg * ga - s12[(g * 2 + 0) * s.c + c] - xh * s12[(g * 2 + 1) * s.c + c]);
    }
}

// Vector variants for c % 4 == 0 with (c/4) dividing 256: one workgroup per (sample, chunk of APOS positions), a thread
// owns 4 consecutive channels and keeps their per-channel coefficients in registers - no index division and no
// parameter gather per element (the scalar kernels above spend more time on 64-bit div/mod than on memory).
constexpr int APOS = 128;
__global__ __launch_bounds__(256) void bn_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ scale,
                                                           const float* __restrict__ offset, const int32_t* __restrict__ labels,
                                                           float* __restrict__ y, BnShape s, int relu) {
    const int c4n = s.c >> 2, c4 = threadIdx.x % c4n, pl = threadIdx.x / c4n, pstep = 256 / c4n;
    const int sample = blockIdx.x, p0 = blockIdx.y * APOS, p1 = min(s.hw, p0 + APOS);
    const int g = sample / (s.n / s.groups), lab = labels ? labels[sample] : 0;
    const float4 mu = *reinterpret_cast<const float4*>(mean + g * s.c + c4 * 4), rs = *reinterpret_cast<const float4*>(rstd + g * s.c + c4 * 4);
    const float4 ga = *reinterpret_cast<const float4*>(scale + lab * s.c + c4 * 4), be = *reinterpret_cast<const float4*>(offset + lab * s.c + c4 * 4);
    const long long base = ((long long)sample * s.hw) * s.c + c4 * 4;
    for (int p = p0 + pl; p < p1; p += pstep) {
        const float4 v = *reinterpret_cast<const float4*>(x + base + (long long)p * s.c);
        float4 o;     // same operation order as the scalar kernel: ((x - mean) * rstd) * scale + offset
        o.x = (v.x - mu.x) * rs.x * ga.x + be.x; o.y = (v.y - mu.y) * rs.y * ga.y + be.y;
        o.z = (v.z - mu.z) * rs.z * ga.z + be.z; o.w = (v.w - mu.w) * rs.w * ga.w + be.w;
        if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        *reinterpret_cast<float4*>(y + base + (long long)p * s.c) = o;
    }
}
__global__ __launch_bounds__(256) void bn_bwd_apply_vec_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ scale, const float* __restrict__ offset,
                                                               const int32_t* __restrict__ labels, const float* __restrict__ s12,
                                                               float* __restrict__ gx, BnShape s, int relu) {
    const int c4n = s.c >> 2, c4 = threadIdx.x % c4n, pl = threadIdx.x / c4n, pstep = 256 / c4n;
    const int sample = blockIdx.x, p0 = blockIdx.y * APOS, p1 = min(s.hw, p0 + APOS);
    const int g = sample / (s.n / s.groups), lab = labels ? labels[sample] : 0;
    const float4 mu = *reinterpret_cast<const float4*>(mean + g * s.c + c4 * 4), rs = *reinterpret_cast<const float4*>(rstd + g * s.c + c4 * 4);
    const float4 ga = *reinterpret_cast<const float4*>(scale + lab * s.c + c4 * 4), be = *reinterpret_cast<const float4*>(offset + lab * s.c + c4 * 4);
    const float4 s1 = *reinterpret_cast<const float4*>(s12 + (g * 2 + 0) * s.c + c4 * 4), s2 = *reinterpret_cast<const float4*>(s12 + (g * 2 + 1) * s.c + c4 * 4);
    const long long base = ((long long)sample * s.hw) * s.c + c4 * 4;
    for (int p = p0 + pl; p < p1; p += pstep) {
        const long long o = base + (long long)p * s.c;
        const float4 v = *reinterpret_cast<const float4*>(x + o);
        float4 gg = *reinterpret_cast<const float4*>(gy + o);
        const float xh0 = (v.x - mu.x) * rs.x, xh1 = (v.y - mu.y) * rs.y, xh2 = (v.z - mu.z) * rs.z, xh3 = (v.w - mu.w) * rs.w;
        if (relu) {
            if (!(xh0 * ga.x + be.x > 0.f)) gg.x = 0.f;
            if (!(xh1 * ga.y + be.y > 0.f)) gg.y = 0.f;
            if (!(xh2 * ga.z + be.z > 0.f)) gg.z = 0.f;
            if (!(xh3 * ga.w + be.w > 0.f)) gg.w = 0.f;
        }
        float4 r;
        r.x = rs.x * (gg.x * ga.x - s1.x - xh0 * s2.x); r.y = rs.y * (gg.y * ga.y - s1.y - xh1 * s2.y);
        r.z = rs.z * (gg.z * ga.z - s1.z - xh2 * s2.z); r.w = rs.w * (gg.w * ga.w - s1.w - xh3 * s2.w);
        *reinterpret_cast<float4*>(gx + o) = r;
    }
}
// Vector partial reductions (same layout of `part`): 16-B loads, each thread sums <= pos*c4n/256 positions of its 4 channels
// in fp32 (a few dozen values), the row lanes are then combined in fp64.  blockDim = 256 = (c/4) channel lanes x row lanes.
// Acc = double (ctgan_bn_stats_f64): the per-thread sums run in fp64 too - sum x^2 - mean^2 of a channel whose spread is far below its
// mean (variance ~ eps = 1e-6 at mean 0.5) loses the variance to the fp32 rounding of a sum of eight 0.25s.
template <typename Acc>
__global__ __launch_bounds__(256) void bn_stats_partial_vec_kernel(const float* __restrict__ x, BnShape s, double* __restrict__ part) {
    __shared__ double red[2][256][4];
    const int c4n = s.c >> 2, rls = 256 / c4n;
    const int c4 = threadIdx.x % c4n, rl = threadIdx.x / c4n;
    const int sample = blockIdx.x / s.hc, chunk = blockIdx.x - sample * s.hc;
    const int p0 = chunk * s.pos, p1 = min(s.hw, p0 + s.pos);
    Acc a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    const float* base = x + ((long long)sample * s.hw) * s.c + c4 * 4;
#pragma unroll 4
    for (int p = p0 + rl; p < p1; p += rls) {
        const float4 v = *reinterpret_cast<const float4*>(base + (long long)p * s.c);
        const Acc x0 = v.x, x1 = v.y, x2 = v.z, x3 = v.w;
        a0 += x0; a1 += x1; a2 += x2; a3 += x3;
        b0 += x0 * x0; b1 += x1 * x1; b2 += x2 * x2; b3 += x3 * x3;
    }
    double* ra = red[0][threadIdx.x]; double* rb = red[1][threadIdx.x];
    ra[0] = a0; ra[1] = a1; ra[2] = a2; ra[3] = a3;
    rb[0] = b0; rb[1] = b1; rb[2] = b2; rb[3] = b3;
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
__global__ __launch_bounds__(256) void bn_bwd_partial_vec_kernel(
    const float* __restrict__ gy, const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ scale, const float* __restrict__ offset, const int32_t* __restrict__ labels, BnShape s, int relu,
    double* __restrict__ part) {
    __shared__ double red[2][256][4];
    const int c4n = s.c >> 2, rls = 256 / c4n;
    const int c4 = threadIdx.x % c4n, rl = threadIdx.x / c4n;
    const int sample = blockIdx.x / s.hc, chunk = blockIdx.x - sample * s.hc;
    const int p0 = chunk * s.pos, p1 = min(s.hw, p0 + s.pos);
    const int g = sample / (s.n / s.groups);
    const int lab = labels ? labels[sample] : 0;
    const float4 mu = *reinterpret_cast<const float4*>(mean + g * s.c + c4 * 4), rs = *reinterpret_cast<const float4*>(rstd + g * s.c + c4 * 4);
    const float4 ga = *reinterpret_cast<const float4*>(scale + lab * s.c + c4 * 4), be = *reinterpret_cast<const float4*>(offset + lab * s.c + c4 * 4);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    const long long base = ((long long)sample * s.hw) * s.c + c4 * 4;
#pragma unroll 4
    for (int p = p0 + rl; p < p1; p += rls) {
        const long long o = base + (long long)p * s.c;
        const float4 xv = *reinterpret_cast<const float4*>(x + o);
        float4 gg = *reinterpret_cast<const float4*>(gy + o);
        const float hx = (xv.x - mu.x) * rs.x, hy = (xv.y - mu.y) * rs.y, hz = (xv.z - mu.z) * rs.z, hw_ = (xv.w - mu.w) * rs.w;
        if (relu) {
            if (!(hx * ga.x + be.x > 0.f)) gg.x = 0.f;
            if (!(hy * ga.y + be.y > 0.f)) gg.y = 0.f;
            if (!(hz * ga.z + be.z > 0.f)) gg.z = 0.f;
            if (!(hw_ * ga.w + be.w > 0.f)) gg.w = 0.f;
        }
        a.x += gg.x; a.y += gg.y; a.z += gg.z; a.w += gg.w;
        b.x += gg.x * hx; b.y += gg.y * hy; b.z += gg.z * hz; b.w += gg.w * hw_;
    }
    double* ra = red[0][threadIdx.x]; double* rb = red[1][threadIdx.x];
    ra[0] = a.x; ra[1] = a.y; ra[2] = a.z; ra[3] = a.w;
    rb[0] = b.x; rb[1] = b.y; rb[2] = b.z; rb[3] = b.w;
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

inline bool bn_vec_ok(const BnShape& s, const void* a, const void* b, const void* c) {
    const int c4n = s.c >> 2;
    return (s.c % 4 == 0) && c4n >= 1 && c4n <= 256 && (256 % c4n == 0) && s.hw >= 8 &&
           (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0);
}

int check_shape(int n, int hw, int c, int groups, const char* who) {
    if (n <= 0 || hw <= 0 || c <= 0 || groups <= 0 || n % groups) return ctgan_fail(CTGAN_E_BADARG, "%s: bad shape", who);
    return 0;
}
BnShape mk(int n, int hw, int c, int groups) {
    const int pos = (long long)n * ((hw + 255) / 256) >= 512 ? 256 : 64;
    return BnShape{n, hw, c, groups, (hw + pos - 1) / pos, pos};
}
size_t part_bytes(const BnShape& s) { return (size_t)s.n * s.hc * 2 * s.c * sizeof(double); }
size_t tot_bytes(const BnShape& s) { return (size_t)s.n * 2 * s.c * sizeof(double); }
size_t bins_bytes(const BnShape& s, int n_labels) { return (size_t)n_labels * 2 * s.c * sizeof(double); }

}  // namespace

extern "C" {

size_t ctgan_bn_workspace_bytes(int32_t n, int32_t hw, int32_t c, int32_t groups, int32_t n_labels) {
    if (n <= 0 || hw <= 0 || c <= 0 || groups <= 0) return 0;
    if (n_labels < 1) n_labels = 1;
    const BnShape s = mk(n, hw, c, groups);
    return part_bytes(s) + tot_bytes(s) + bins_bytes(s, n_labels) + (size_t)groups * 2 * c * sizeof(float);
}

static int bn_stats_impl(const float* x, int32_t n, int32_t hw, int32_t c, int32_t groups, float eps, float* mean, float* rstd, void* ws,
                         size_t ws_bytes, bool f64, ctgan_stream_t stream) {
    int rc = check_shape(n, hw, c, groups, "bn_stats");
    if (rc) return rc;
    if (!x || !mean || !rstd || !ws) return ctgan_fail(CTGAN_E_BADARG, "bn_stats: null");
    const BnShape s = mk(n, hw, c, groups);
    if (ws_bytes < part_bytes(s)) return ctgan_fail(CTGAN_E_BADARG, "bn_stats: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (bn_vec_ok(s, x, x, x) && f64)
        hipLaunchKernelGGL(bn_stats_partial_vec_kernel<double>, dim3(n * s.hc), dim3(256), 0, st, x, s, static_cast<double*>(ws));
    else if (bn_vec_ok(s, x, x, x))
        hipLaunchKernelGGL(bn_stats_partial_vec_kernel<float>, dim3(n * s.hc), dim3(256), 0, st, x, s, static_cast<double*>(ws));
    else
        hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(n * s.hc, (c + CB - 1) / CB), dim3(CB * RL), 0, st, x, s,
                           static_cast<double*>(ws));
    rc = ctgan_check_launch("bn_stats_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((c + CB - 1) / CB, groups), dim3(CB * FL), 0, st,
                       static_cast<const double*>(ws), s, eps, mean, rstd);
    return ctgan_check_launch("bn_stats_final");
}

int ctgan_bn_stats(const float* x, int32_t n, int32_t hw, int32_t c, int32_t groups, float eps, float* mean, float* rstd,
                   void* ws, size_t ws_bytes, ctgan_stream_t stream) {
    return bn_stats_impl(x, n, hw, c, groups, eps, mean, rstd, ws, ws_bytes, false, stream);
}

int ctgan_bn_stats_f64(const float* x, int32_t n, int32_t hw, int32_t c, int32_t groups, float eps, float* mean, float* rstd,
                       void* ws, size_t ws_bytes, ctgan_stream_t stream) {
    return bn_stats_impl(x, n, hw, c, groups, eps, mean, rstd, ws, ws_bytes, true, stream);
}

int ctgan_bn_apply(const float* x, const float* mean, const float* rstd, const float* scale, const float* offset,
                   const int32_t* labels, float* y, int32_t n, int32_t hw, int32_t c, int32_t groups, int32_t relu,
                   ctgan_stream_t stream) {
    int rc = check_shape(n, hw, c, groups, "bn_apply");
    if (rc) return rc;
    if (!x || !mean || !rstd || !scale || !offset || !y) return ctgan_fail(CTGAN_E_BADARG, "bn_apply: null");
    const BnShape s = mk(n, hw, c, groups);
    if (bn_vec_ok(s, x, y, mean) && bn_vec_ok(s, rstd, scale, offset)) {
        hipLaunchKernelGGL(bn_apply_vec_kernel, dim3(n, (hw + APOS - 1) / APOS), dim3(256), 0, static_cast<hipStream_t>(stream), x, mean, rstd,
                           scale, offset, labels, y, s, relu);
        return ctgan_check_launch("bn_apply_vec");
    }
    hipLaunchKernelGGL(bn_apply_kernel, dim3(ctgan_blocks((long long)n * hw * c, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, mean, rstd, scale, offset, labels, y, s, relu);
    return ctgan_check_launch("bn_apply");
}

int ctgan_bn_bwd(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale,
                 const float* offset, const int32_t* labels, float* gx, float* gscale, float* goffset, int32_t n,
                 int32_t hw, int32_t c, int32_t groups, int32_t n_labels, int32_t relu, void* ws, size_t ws_bytes,
                 ctgan_stream_t stream) {
    int rc = check_shape(n, hw, c, groups, "bn_bwd");
    if (rc) return rc;
    if (!gy || !x || !mean || !rstd || !scale || !offset || !gx || !gscale || !goffset || !ws || n_labels <= 0)
        return ctgan_fail(CTGAN_E_BADARG, "bn_bwd: bad argument");
    const BnShape s = mk(n, hw, c, groups);
    if (ws_bytes < ctgan_bn_workspace_bytes(n, hw, c, groups, n_labels))
        return ctgan_fail(CTGAN_E_BADARG, "bn_bwd: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* wsb = static_cast<char*>(ws);
    double* part = reinterpret_cast<double*>(wsb);
    double* tot = reinterpret_cast<double*>(wsb + part_bytes(s));
    double* bins = reinterpret_cast<double*>(wsb + part_bytes(s) + tot_bytes(s));
    float* s12 = reinterpret_cast<float*>(wsb + part_bytes(s) + tot_bytes(s) + bins_bytes(s, n_labels));
    if (bn_vec_ok(s, gy, x, mean) && bn_vec_ok(s, rstd, scale, offset))
        hipLaunchKernelGGL(bn_bwd_partial_vec_kernel, dim3(n * s.hc), dim3(256), 0, st, gy, x, mean, rstd, scale, offset, labels, s, relu, part);
    else
        hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(n * s.hc, (c + CB - 1) / CB), dim3(CB * RL), 0, st, gy, x, mean, rstd,
                           scale, offset, labels, s, relu, part);
    rc = ctgan_check_launch("bn_bwd_partial");
    if (rc) return rc;
    (void)bins; (void)tot;
    // the finalisation sums the (<= 4) chunk partials of a sample itself: no per-sample totals pass
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((c + 63) / 64, n_labels + groups), dim3(64 * 16), 0, st, part, scale, labels, s,
                       n_labels, gscale, goffset, s12);
    rc = ctgan_check_launch("bn_bwd_final");
    if (rc) return rc;
    if (bn_vec_ok(s, gy, x, gx) && bn_vec_ok(s, mean, rstd, scale) && bn_vec_ok(s, offset, s12, s12)) {
        hipLaunchKernelGGL(bn_bwd_apply_vec_kernel, dim3(n, (hw + APOS - 1) / APOS), dim3(256), 0, st, gy, x, mean, rstd, scale, offset, labels,
                           s12, gx, s, relu);
        return ctgan_check_launch("bn_bwd_apply_vec");
    }
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ctgan_blocks((long long)n * hw * c, 256)), dim3(256), 0, st, gy, x, mean,
                       rstd, scale, offset, labels, s12, gx, s, relu);
    return ctgan_check_launch("bn_bwd_apply");
}

}  // extern "C"
