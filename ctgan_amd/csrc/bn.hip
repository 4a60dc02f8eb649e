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
                                                             float* __restrict__ s12, double gys, float* __restrict__ sga) {
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
    // gys: the incoming gradient is gys * gy (ctgan_bn_bwd_scaled; 1 elsewhere - exact).  Every sum is linear in gy, so the factor
    // goes on the totals, and the apply pass reads the gain from sga = gys * scale instead of scaling gy per element.
    a *= gys; b *= gys;
    if (job < n_labels) {
        goffset[job * s.c + c] = (float)a; gscale[job * s.c + c] = (float)b;
    } else {
        const int g = job - n_labels;
        const double cnt = (double)per * s.hw;
        s12[(g * 2 + 0) * s.c + c] = (float)(a / cnt); s12[(g * 2 + 1) * s.c + c] = (float)(b / cnt);
        if (sga) sga[c] = (float)gys * scale[c];
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

// ---- the score classifier's batch norm (LS/tflib/ops/batchnorm.py:30-69; LS/ = tensorflow_generative_model/LSUN_bedrooms) ----------
// Finalisation of the training statistics (one group) that also moves the moving statistics (:62-65):
//   moving <- (it/(it+1)) moving + (1/(it+1)) batch     in fp32, `it` read from device memory (a replayed graph sees the current value)
// batch_var is what tf.nn.fused_batch_norm returns in training: the biased variance * cnt/max(cnt-1, 1), taken from the fp64 sums.
// Same summation order as bn_stats_final_kernel.  moving_mean == NULL: no update.
__global__ __launch_bounds__(CB * FL) void bn_stats_final_moving_kernel(const double* __restrict__ part, BnShape s, float eps,
                                                                       float* __restrict__ mean, float* __restrict__ rstd,
                                                                       float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                                       const float* __restrict__ it) {
    __shared__ double red[2][FL][CB];
    const int cl = threadIdx.x % CB, fl = threadIdx.x / CB;
    const int c = blockIdx.x * CB + cl;
    double a = 0., b = 0.;
    if (c < s.c) {
        const int i1 = s.n * s.hc;
        for (int i = fl; i < i1; i += FL) {
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
    const double cnt = (double)s.n * s.hw;
    const double m = a / cnt;
    double var = b / cnt - m * m;
    if (var < 0.) var = 0.;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (moving_mean) {
        const float bm = (float)m, bv = (float)(var * (cnt / fmax(cnt - 1., 1.)));
        const float fi = it[0];
        const float wa = fi / (fi + 1.f), wb = 1.f / (fi + 1.f);
        moving_mean[c] = wa * moving_mean[c] + wb * bm;
        moving_var[c] = wa * moving_var[c] + wb * bv;
    }
}

// Per-sample finalisation of the inference-mode "blend" (:32-38): the biased moments of sample n's plane c over h*w, from that sample's
// rows of `part`, blended in fp32 with the moving statistics by the row count B = n of the call:
//   mean = m/B + ((B-1)/B) moving_mean[c]   (the variance alike)  ->  mean[n][c], rstd[n][c] = 1/sqrt(var + eps)
// workgroup = 64 channels x 4 samples.
__global__ __launch_bounds__(CB * RL) void bn_blend_final_kernel(const double* __restrict__ part, BnShape s, float eps,
                                                                const float* __restrict__ moving_mean, const float* __restrict__ moving_var,
                                                                float* __restrict__ mean, float* __restrict__ rstd) {
    const int cl = threadIdx.x % CB, sl = threadIdx.x / CB;
    const int c = blockIdx.y * CB + cl, sample = blockIdx.x * RL + sl;
    if (c >= s.c || sample >= s.n) return;
    double a = 0., b = 0.;
    for (int k = 0; k < s.hc; ++k) {
        const long long i = ((long long)sample * s.hc + k) * 2 * s.c;
        a += part[i + c]; b += part[i + s.c + c];
    }
    const double m = a / s.hw;
    double var = b / s.hw - m * m;
    if (var < 0.) var = 0.;
    const float B = (float)s.n;
    const float wa = 1.f / B, wb = (B - 1.f) / B;
    const float mu = wa * (float)m + wb * moving_mean[c];
    const float v = wa * (float)var + wb * moving_var[c];
    mean[(long long)sample * s.c + c] = mu;
    rstd[(long long)sample * s.c + c] = (float)(1.0 / sqrt((double)v + (double)eps));
}

__device__ __forceinline__ float bn_elu(float x) { return x > 0.f ? x : expm1f(x); }

// y = [shortcut +] alpha * [relu]( (x - mean) * rstd * scale + offset ),  elu_out = elu(y)   in one pass.
// sstride: 0 = mean / rstd per channel (training statistics), c = per (sample, channel) (the blend).  shortcut / elu_out may be NULL.
__global__ void bn_apply_ex_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd, int sstride,
                                   const float* __restrict__ scale, const float* __restrict__ offset, const float* __restrict__ shortcut,
                                   float alpha, float* __restrict__ y, float* __restrict__ elu_out, BnShape s, int relu) {
    const long long total = (long long)s.n * s.hw * s.c;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long hwc = (long long)s.hw * s.c;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int c = i % s.c;
        const long long st = (i / hwc) * sstride + c;
        float v = (x[i] - mean[st]) * rstd[st] * scale[c] + offset[c];
        if (relu) v = fmaxf(v, 0.f);
        v = shortcut ? shortcut[i] + alpha * v : alpha * v;
        y[i] = v;
        if (elu_out) elu_out[i] = bn_elu(v);
    }
}
// vector form, as bn_apply_vec_kernel: a thread owns 4 consecutive channels of one sample and keeps their coefficients in registers
__global__ __launch_bounds__(256) void bn_apply_ex_vec_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, int sstride, const float* __restrict__ scale,
                                                              const float* __restrict__ offset, const float* __restrict__ shortcut, float alpha,
                                                              float* __restrict__ y, float* __restrict__ elu_out, BnShape s, int relu) {
    const int c4n = s.c >> 2, c4 = threadIdx.x % c4n, pl = threadIdx.x / c4n, pstep = 256 / c4n;
    const int sample = blockIdx.x, p0 = blockIdx.y * APOS, p1 = min(s.hw, p0 + APOS);
    const long long st = (long long)sample * sstride + c4 * 4;
    const float4 mu = *reinterpret_cast<const float4*>(mean + st), rs = *reinterpret_cast<const float4*>(rstd + st);
    const float4 ga = *reinterpret_cast<const float4*>(scale + c4 * 4), be = *reinterpret_cast<const float4*>(offset + c4 * 4);
    const long long base = ((long long)sample * s.hw) * s.c + c4 * 4;
    for (int p = p0 + pl; p < p1; p += pstep) {
        const long long o = base + (long long)p * s.c;
        const float4 v = *reinterpret_cast<const float4*>(x + o);
        float4 r;     // the operation order of bn_apply_kernel, then the residual sum
        r.x = (v.x - mu.x) * rs.x * ga.x + be.x; r.y = (v.y - mu.y) * rs.y * ga.y + be.y;
        r.z = (v.z - mu.z) * rs.z * ga.z + be.z; r.w = (v.w - mu.w) * rs.w * ga.w + be.w;
        if (relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
        if (shortcut) {
            const float4 sc = *reinterpret_cast<const float4*>(shortcut + o);
            r.x = sc.x + alpha * r.x; r.y = sc.y + alpha * r.y; r.z = sc.z + alpha * r.z; r.w = sc.w + alpha * r.w;
        } else {
            r.x *= alpha; r.y *= alpha; r.z *= alpha; r.w *= alpha;
        }
        *reinterpret_cast<float4*>(y + o) = r;
        if (elu_out) {
            float4 e;
            e.x = bn_elu(r.x); e.y = bn_elu(r.y); e.z = bn_elu(r.z); e.w = bn_elu(r.w);
            *reinterpret_cast<float4*>(elu_out + o) = e;
        }
    }
}

// the fp64 partial sums of the two entry points above (rows per (sample, chunk): what the blend needs per sample)
int launch_partial_f64(const float* x, const BnShape& s, double* part, hipStream_t st) {
    if (bn_vec_ok(s, x, x, x))
        hipLaunchKernelGGL(bn_stats_partial_vec_kernel<double>, dim3(s.n * s.hc), dim3(256), 0, st, x, s, part);
    else
        hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(s.n * s.hc, (s.c + CB - 1) / CB), dim3(CB * RL), 0, st, x, s, part);
    return ctgan_check_launch("bn_stats_partial");
}

}  // namespace

void ctgan_bn_plan(int n, int hw, int* hc, int* pos) {
    const BnShape s = mk(n, hw, 1, 1);
    *hc = s.hc; *pos = s.pos;
}

int ctgan_bn_bwd_finalize(const double* part, const float* scale, int n, int hw, int c, int groups, float* gscale, float* goffset,
                          float* s12, hipStream_t st) {
    const BnShape s = mk(n, hw, c, groups);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((c + 63) / 64, 1 + groups), dim3(64 * 16), 0, st, part, scale,
                       static_cast<const int32_t*>(nullptr), s, 1, gscale, goffset, s12, 1.0, static_cast<float*>(nullptr));
    return ctgan_check_launch("bn_bwd_final");
}

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

// scaled: the gradient is gys * gy (no labels, one group, no ReLU); the gain of the apply pass is then sga, written by the finalisation
static int bn_bwd_impl(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale,
                       const float* offset, const int32_t* labels, float* gx, float* gscale, float* goffset, int32_t n,
                       int32_t hw, int32_t c, int32_t groups, int32_t n_labels, int32_t relu, void* ws, size_t ws_bytes,
                       bool scaled, double gys, ctgan_stream_t stream) {
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
    (void)tot;
    float* sga = scaled ? reinterpret_cast<float*>(bins) : nullptr;      // c floats of the (otherwise unused) label-bin region
    // the finalisation sums the (<= 4) chunk partials of a sample itself: no per-sample totals pass
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((c + 63) / 64, n_labels + groups), dim3(64 * 16), 0, st, part, scale, labels, s,
                       n_labels, gscale, goffset, s12, gys, sga);
    rc = ctgan_check_launch("bn_bwd_final");
    if (rc) return rc;
    if (scaled) scale = sga;
    if (bn_vec_ok(s, gy, x, gx) && bn_vec_ok(s, mean, rstd, scale) && bn_vec_ok(s, offset, s12, s12)) {
        hipLaunchKernelGGL(bn_bwd_apply_vec_kernel, dim3(n, (hw + APOS - 1) / APOS), dim3(256), 0, st, gy, x, mean, rstd, scale, offset, labels,
                           s12, gx, s, relu);
        return ctgan_check_launch("bn_bwd_apply_vec");
    }
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ctgan_blocks((long long)n * hw * c, 256)), dim3(256), 0, st, gy, x, mean,
                       rstd, scale, offset, labels, s12, gx, s, relu);
    return ctgan_check_launch("bn_bwd_apply");
}

int ctgan_bn_bwd(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale,
                 const float* offset, const int32_t* labels, float* gx, float* gscale, float* goffset, int32_t n,
                 int32_t hw, int32_t c, int32_t groups, int32_t n_labels, int32_t relu, void* ws, size_t ws_bytes,
                 ctgan_stream_t stream) {
    return bn_bwd_impl(gy, x, mean, rstd, scale, offset, labels, gx, gscale, goffset, n, hw, c, groups, n_labels, relu, ws, ws_bytes,
                       false, 1.0, stream);
}

int ctgan_bn_bwd_scaled(const float* gy, const float* x, const float* mean, const float* rstd, const float* scale,
                        const float* offset, float gy_scale, float* gx, float* gscale, float* goffset, int32_t n, int32_t hw,
                        int32_t c, void* ws, size_t ws_bytes, ctgan_stream_t stream) {
    return bn_bwd_impl(gy, x, mean, rstd, scale, offset, nullptr, gx, gscale, goffset, n, hw, c, 1, 1, 0, ws, ws_bytes, true,
                       (double)gy_scale, stream);
}

int ctgan_bn_stats_moving(const float* x, int32_t n, int32_t hw, int32_t c, float eps, float* mean, float* rstd, float* moving_mean,
                          float* moving_var, const float* it, void* ws, size_t ws_bytes, ctgan_stream_t stream) {
    int rc = check_shape(n, hw, c, 1, "bn_stats_moving");
    if (rc) return rc;
    if (!x || !mean || !rstd || !ws) return ctgan_fail(CTGAN_E_BADARG, "bn_stats_moving: null");
    if ((moving_mean != nullptr) != (moving_var != nullptr) || (moving_mean && !it))
        return ctgan_fail(CTGAN_E_BADARG, "bn_stats_moving: the update needs moving_mean, moving_var and it");
    const BnShape s = mk(n, hw, c, 1);
    if (ws_bytes < part_bytes(s)) return ctgan_fail(CTGAN_E_BADARG, "bn_stats_moving: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_partial_f64(x, s, static_cast<double*>(ws), st);
    if (rc) return rc;
    hipLaunchKernelGGL(bn_stats_final_moving_kernel, dim3((c + CB - 1) / CB), dim3(CB * FL), 0, st, static_cast<const double*>(ws), s, eps,
                       mean, rstd, moving_mean, moving_var, it);
    return ctgan_check_launch("bn_stats_final_moving");
}

int ctgan_bn_blend_stats(const float* x, int32_t n, int32_t hw, int32_t c, float eps, const float* moving_mean, const float* moving_var,
                         float* mean, float* rstd, void* ws, size_t ws_bytes, ctgan_stream_t stream) {
    int rc = check_shape(n, hw, c, 1, "bn_blend_stats");
    if (rc) return rc;
    if (!x || !mean || !rstd || !moving_mean || !moving_var || !ws) return ctgan_fail(CTGAN_E_BADARG, "bn_blend_stats: null");
    const BnShape s = mk(n, hw, c, 1);
    if (ws_bytes < part_bytes(s)) return ctgan_fail(CTGAN_E_BADARG, "bn_blend_stats: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_partial_f64(x, s, static_cast<double*>(ws), st);
    if (rc) return rc;
    hipLaunchKernelGGL(bn_blend_final_kernel, dim3((n + RL - 1) / RL, (c + CB - 1) / CB), dim3(CB * RL), 0, st,
                       static_cast<const double*>(ws), s, eps, moving_mean, moving_var, mean, rstd);
    return ctgan_check_launch("bn_blend_final");
}

int ctgan_bn_apply_ex(const float* x, const float* mean, const float* rstd, int32_t per_sample, const float* scale, const float* offset,
                      const float* shortcut, float alpha, float* y, float* elu_out, int32_t relu, int32_t n, int32_t hw, int32_t c,
                      ctgan_stream_t stream) {
    int rc = check_shape(n, hw, c, 1, "bn_apply_ex");
    if (rc) return rc;
    if (!x || !mean || !rstd || !scale || !offset || !y) return ctgan_fail(CTGAN_E_BADARG, "bn_apply_ex: null");
    const BnShape s = mk(n, hw, c, 1);
    const int sstride = per_sample ? c : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (bn_vec_ok(s, x, y, mean) && bn_vec_ok(s, rstd, scale, offset) && bn_vec_ok(s, shortcut, elu_out, x)) {
        hipLaunchKernelGGL(bn_apply_ex_vec_kernel, dim3(n, (hw + APOS - 1) / APOS), dim3(256), 0, st, x, mean, rstd, sstride, scale, offset,
                           shortcut, alpha, y, elu_out, s, relu);
        return ctgan_check_launch("bn_apply_ex_vec");
    }
    hipLaunchKernelGGL(bn_apply_ex_kernel, dim3(ctgan_blocks((long long)n * hw * c, 256)), dim3(256), 0, st, x, mean, rstd, sstride, scale,
                       offset, shortcut, alpha, y, elu_out, s, relu);
    return ctgan_check_launch("bn_apply_ex");
}

}  // extern "C"
