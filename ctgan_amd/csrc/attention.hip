// attention.hip - the self-attention core of attention.py (Zhang et al. 2019; NOT in the reference) and its gated residual:
//   out[b, i, :] = sum_j softmax_j(q[b, i] . k[b, j]) v[b, j, :]         q, k [n, N, dk], v, out [n, N, dv] dense rows, no 1 / sqrt(dk) scale
//   lse[b, i]    = log sum_j exp(q[b, i] . k[b, j])                      (the row statistic the backward recomputes P = exp(S - lse) from)
// The [N, N] score matrix of an image exists in registers and LDS only, one 64 x 64 tile at a time (the structure of knn.hip / kid.hip):
// four waves own 64 rows (16 per wave), a block of 64 rows of the other operand is staged in LDS, the products run on the exact-fp32
// v_mfma_f32_16x16x4_f32 (A[l & 15][l >> 4], B[l >> 4][l & 15], C/D col = l & 15, row = 4 (l >> 4) + reg) whatever the convs' mma mode is.
// A tile of P leaves the accumulator layout through a wave-private LDS tile and comes back in the A-operand layout for the second product.
//
//   forward      grid = images x blocks of 64 queries; online softmax (running max and sum per row, the accumulator rescaled per key block).
//   backward gq  grid = images x blocks of 64 queries: delta_i = gout_i . out_i (also written to delta [n, N] for the second launch),
//                dS = P o (gout v^T - delta), gq = dS k.
//   backward gk, gv  grid = images x blocks of 64 keys: the transposed tiles S^T, P^T, dS^T; gk = dS^T q, gv = P^T gout.
// Every output element has one owning lane and one summation order that knows nothing of the grid or of the other images: no atomics,
// the same bits on every run, an image's rows the same whatever shares the launch.  No workspace grows with N^2 (delta is [n, N]).
// N is a multiple of 16, not of 64: keys past N of the last block are masked BY INDEX (a staged zero row would still score exp(0 - max)).
#include <math.h>

#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int TM = 64;            // rows per workgroup (16 per wave)
constexpr int TN = 64;            // rows of the other operand per staged block
constexpr int LDP = TN + 4;       // row stride of a wave's P tile: bank = 4 (l & 15) + (l >> 4) on the read, 16 (l >> 4) + (l & 15) on the write
constexpr int PTILE = 16 * LDP;
constexpr int RES_PARTS = 256;    // partial sums of the gate's gradient: the grid of attn_residual_bwd_kernel, whatever the size

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// row stride (floats, a multiple of 4) of a staged tile of `w` columns read with the row on the lane's low bits: stride / 4 odd
__host__ __device__ __forceinline__ int ld_rows(int w) { return ((w >> 2) & 1) ? w : w + 4; }
// ... read with the row on the lane's high bits (16 consecutive columns per row): stride = 16 mod 32
__host__ __device__ __forceinline__ int ld_cols(int w) { return (w & 31) == 16 ? w : w + 16; }

// dst[r][0 : w] = src[r][0 : d] (then zeros to w) for r < valid, zeros for valid <= r < 64.  d, w, ld multiples of 4; src 16-byte aligned.
__device__ __forceinline__ void stage(float* __restrict__ dst, int ld, int w, const float* __restrict__ src, int valid, int d) {
    const int w4 = w >> 2;
    for (int i = threadIdx.x; i < TN * w4; i += TPB) {
        const int r = i / w4, c = (i - r * w4) << 2;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < valid && c < d) val = *reinterpret_cast<const float4*>(src + (size_t)r * d + c);
        *reinterpret_cast<float4*>(dst + r * ld + c) = val;
    }
}

// the sum / maximum over the 16 lanes that hold one accumulator row (lanes of equal l >> 4), in one fixed order
__device__ __forceinline__ float row_sum(float x) {
    for (int o = 1; o < 16; o <<= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float row_max(float x) {
    for (int o = 1; o < 16; o <<= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}

#define ATT_IDS                                                                               \
    const int nb = (N + TM - 1) / TM;                                                         \
    const int b = blockIdx.x / nb, r0 = (blockIdx.x - b * nb) * TM;                           \
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lg = lane >> 4; \
    const size_t base = (size_t)b * N;                                                        \
    const int arow = min(r0 + 16 * wave + li, N - 1);          /* the A-operand row of this lane (clamped: rows past N are not stored) */

// ------------------------------------------------------------------------------------------------------------------ forward
template <int DVT>
__global__ __launch_bounds__(TPB) void attention_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            float* __restrict__ out, float* __restrict__ lse, int N, int dk, int dv) {
    extern __shared__ __align__(16) float smem[];
    ATT_IDS
    const int ldk = ld_rows(dk), ldv = ld_cols(dv);
    float* sK = smem;
    float* sV = sK + TN * ldk;
    float* sP = sV + TN * ldv + wave * PTILE;
    const float* qp = q + (base + arow) * dk + lg;
    f32x4 o[DVT];
    float m[4], l[4];
#pragma unroll
    for (int c = 0; c < DVT; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = -INFINITY, l[r] = 0.f;

    for (int j0 = 0; j0 < N; j0 += TN) {
        __syncthreads();                                  // the previous block's readers are done
        const int valid = min(TN, N - j0);
        stage(sK, ldk, dk, k + (base + j0) * dk, valid, dk);
        stage(sV, ldv, dv, v + (base + j0) * dv, valid, dv);
        __syncthreads();
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < dk; kk += 4) {
            const float a = qp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = MFMA4(a, sK[(li + 16 * t) * ldk + lg + kk], s[t]);
        }
        float mx[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[r] = m[r];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool in = j0 + li + 16 * t < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!in) s[t][r] = -INFINITY;
                mx[r] = fmaxf(mx[r], s[t][r]);
            }
        }
        float sum[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            mx[r] = row_max(mx[r]);                       // finite: every block holds at least one key
            const float sc = expf(m[r] - mx[r]);          // exp(-inf) = 0 on the first block
            m[r] = mx[r];
            l[r] *= sc;
#pragma unroll
            for (int c = 0; c < DVT; ++c) o[c][r] *= sc;
            sum[r] = 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(s[t][r] - mx[r]);
                sum[r] += p;
                sP[(4 * lg + r) * LDP + li + 16 * t] = p;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) l[r] += row_sum(sum[r]);
        __syncthreads();                                  // P: accumulator layout -> operand layout
        for (int kk = 0; kk < TN; kk += 4) {
            const float a = sP[li * LDP + lg + kk];
#pragma unroll
            for (int c = 0; c < DVT; ++c)
                if (16 * c < dv) o[c] = MFMA4(a, sV[(lg + kk) * ldv + li + 16 * c], o[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wave + 4 * lg + r;
        if (row >= N) continue;
        const float inv = 1.f / l[r];
#pragma unroll
        for (int c = 0; c < DVT; ++c)
            if (16 * c < dv) out[(base + row) * dv + li + 16 * c] = o[c][r] * inv;
        if (lse && li == 0) lse[base + row] = m[r] + logf(l[r]);
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward: gq
template <int DKT>
__global__ __launch_bounds__(TPB) void attention_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                              const float* __restrict__ out, const float* __restrict__ lse,
                                                              const float* __restrict__ gout, float* __restrict__ gq, float* __restrict__ delta,
                                                              int N, int dk, int dv) {
    extern __shared__ __align__(16) float smem[];
    ATT_IDS
    constexpr int KW = 16 * DKT, LDK = KW + 4;            // k is read both ways: zero columns up to the accumulator's width
    const int ldv = ld_rows(dv);
    float* sK = smem;
    float* sV = sK + TN * LDK;
    float* sP = sV + TN * ldv + wave * PTILE;
    const float* qp = q + (base + arow) * dk + lg;
    const float* gp = gout + (base + arow) * dv + lg;
    float ls[4], dl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wave + 4 * lg + r, rc = min(row, N - 1);
        float acc = 0.f;
        for (int c = li; c < dv; c += 16) acc += gout[(base + rc) * dv + c] * out[(base + rc) * dv + c];
        dl[r] = row_sum(acc);
        ls[r] = lse[base + rc];
        if (li == 0 && row < N) delta[base + row] = dl[r];
    }
    f32x4 g[DKT];
#pragma unroll
    for (int c = 0; c < DKT; ++c) g[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j0 = 0; j0 < N; j0 += TN) {
        __syncthreads();
        const int valid = min(TN, N - j0);
        stage(sK, LDK, KW, k + (base + j0) * dk, valid, dk);
        stage(sV, ldv, dv, v + (base + j0) * dv, valid, dv);
        __syncthreads();
        f32x4 s[4], dp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < dk; kk += 4) {
            const float a = qp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = MFMA4(a, sK[(li + 16 * t) * LDK + lg + kk], s[t]);
        }
        for (int kk = 0; kk < dv; kk += 4) {
            const float a = gp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) dp[t] = MFMA4(a, sV[(li + 16 * t) * ldv + lg + kk], dp[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool in = j0 + li + 16 * t < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = in ? expf(s[t][r] - ls[r]) : 0.f;
                sP[(4 * lg + r) * LDP + li + 16 * t] = p * (dp[t][r] - dl[r]);
            }
        }
        __syncthreads();
        for (int kk = 0; kk < TN; kk += 4) {
            const float a = sP[li * LDP + lg + kk];
#pragma unroll
            for (int c = 0; c < DKT; ++c) g[c] = MFMA4(a, sK[(lg + kk) * LDK + li + 16 * c], g[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wave + 4 * lg + r;
        if (row >= N) continue;
#pragma unroll
        for (int c = 0; c < DKT; ++c)
            if (li + 16 * c < dk) gq[(base + row) * dk + li + 16 * c] = g[c][r];
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward: gk, gv
template <int DKT, int DVT>
__global__ __launch_bounds__(TPB) void attention_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               const float* __restrict__ gout, float* __restrict__ gk, float* __restrict__ gv,
                                                               int N, int dk, int dv) {
    extern __shared__ __align__(16) float smem[];
    ATT_IDS
    constexpr int QW = 16 * DKT, LDQ = QW + 4, GW = 16 * DVT, LDG = GW + 4;      // q and gout are read both ways
    float* sQ = smem;
    float* sG = sQ + TN * LDQ;
    float* sL = sG + TN * LDG;
    float* sD = sL + TN;
    float* sP = sD + TN + wave * 2 * PTILE;
    float* sS = sP + PTILE;
    const float* kp = k + (base + arow) * dk + lg;        // this workgroup's rows are keys
    const float* vp = v + (base + arow) * dv + lg;
    f32x4 ak[DKT], av[DVT];
#pragma unroll
    for (int c = 0; c < DKT; ++c) ak[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DVT; ++c) av[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int i0 = 0; i0 < N; i0 += TN) {
        __syncthreads();
        const int valid = min(TN, N - i0);
        stage(sQ, LDQ, QW, q + (base + i0) * dk, valid, dk);
        stage(sG, LDG, GW, gout + (base + i0) * dv, valid, dv);
        if (threadIdx.x < TN) {
            const bool in = (int)threadIdx.x < valid;
            sL[threadIdx.x] = in ? lse[base + i0 + threadIdx.x] : 0.f;
            sD[threadIdx.x] = in ? delta[base + i0 + threadIdx.x] : 0.f;
        }
        __syncthreads();
        f32x4 s[4], dp[4];                                // [key 4 lg + r of the wave][query li + 16 t of the block]
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < dk; kk += 4) {
            const float a = kp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) s[t] = MFMA4(a, sQ[(li + 16 * t) * LDQ + lg + kk], s[t]);
        }
        for (int kk = 0; kk < dv; kk += 4) {
            const float a = vp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) dp[t] = MFMA4(a, sG[(li + 16 * t) * LDG + lg + kk], dp[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool in = i0 + li + 16 * t < N;
            const float L = sL[li + 16 * t], D = sD[li + 16 * t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = in ? expf(s[t][r] - L) : 0.f;
                sP[(4 * lg + r) * LDP + li + 16 * t] = p;
                sS[(4 * lg + r) * LDP + li + 16 * t] = p * (dp[t][r] - D);
            }
        }
        __syncthreads();
        for (int kk = 0; kk < TN; kk += 4) {
            const float ap = sP[li * LDP + lg + kk], as = sS[li * LDP + lg + kk];
#pragma unroll
            for (int c = 0; c < DKT; ++c) ak[c] = MFMA4(as, sQ[(lg + kk) * LDQ + li + 16 * c], ak[c]);
#pragma unroll
            for (int c = 0; c < DVT; ++c) av[c] = MFMA4(ap, sG[(lg + kk) * LDG + li + 16 * c], av[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wave + 4 * lg + r;
        if (row >= N) continue;
#pragma unroll
        for (int c = 0; c < DKT; ++c)
            if (li + 16 * c < dk) gk[(base + row) * dk + li + 16 * c] = ak[c][r];
#pragma unroll
        for (int c = 0; c < DVT; ++c)
            if (li + 16 * c < dv) gv[(base + row) * dv + li + 16 * c] = av[c][r];
    }
}

// ------------------------------------------------------------------------------------------------------------------ second derivative
// The backward of the backward above: a, b, c are the cotangents of gq, gk, gv.  With T = a k^T + q b^T (the cotangent of dS), dP = gout v^T,
//   tau_i = sum_j P T,   Pc = P c,   rho_i = sum_j P T dP - 2 tau_i delta_i + gout_i . (Pc)_i              (row statistics: a full key sweep)
//   W = P o (T - tau),   Sbar = P o (T o dP - dP tau - T delta + gout c^T - rho),   dS = P o (dP - delta)
//   d q = Sbar k + dS b,  d gout = W v + Pc          (grid = images x blocks of 64 queries: sweep 1 the statistics, sweep 2 the two outputs)
//   d k = Sbar^T q + dS^T a,  d v = W^T gout         (grid = images x blocks of 64 keys, on the transposed tiles; reads tau, rho [n, N])
// Every tile quantity is in the accumulator layout [row 4 lg + r of the wave][column li + 16 t of the staged block]; three of them (Sbar, dS,
// W) cross a wave-private LDS tile each into the A-operand layout.  The staged operands are read both ways (zero columns up to the
// accumulator's width).  Keys past N have P = 0 by index, so every product with them vanishes; rows past N are clamped and not stored.
template <int DKT, int DVT>
__global__ __launch_bounds__(TPB) void attention_bwd2_q_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               const float* __restrict__ gout, const float* __restrict__ a,
                                                               const float* __restrict__ b_, const float* __restrict__ c_,
                                                               float* __restrict__ dq, float* __restrict__ dgout, float* __restrict__ tau_out,
                                                               float* __restrict__ rho_out, int N, int dk, int dv) {
    extern __shared__ __align__(16) float smem[];
    ATT_IDS
    constexpr int KW = 16 * DKT, LDK = KW + 4, VW = 16 * DVT, LDV = VW + 4;
    float* sK = smem;
    float* sB = sK + TN * LDK;
    float* sV = sB + TN * LDK;
    float* sC = sV + TN * LDV;
    float* sX = sC + TN * LDV + wave * 3 * PTILE;         // P (sweep 1), Sbar (sweep 2)
    float* sY = sX + PTILE;                               // dS
    float* sZ = sY + PTILE;                               // W
    const float* qp = q + (base + arow) * dk + lg;
    const float* ap = a + (base + arow) * dk + lg;
    const float* gp = gout + (base + arow) * dv + lg;
    float ls[4], dl[4], tau[4], rho[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int rc = min(r0 + 16 * wave + 4 * lg + r, N - 1);
        ls[r] = lse[base + rc];
        dl[r] = delta[base + rc];
        tau[r] = rho[r] = 0.f;
    }
    f32x4 pc[DVT];                                        // Pc, then d gout = Pc + W v
#pragma unroll
    for (int c = 0; c < DVT; ++c) pc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- sweep 1: tau, rho, Pc
    for (int j0 = 0; j0 < N; j0 += TN) {
        __syncthreads();
        const int valid = min(TN, N - j0);
        stage(sK, LDK, KW, k + (base + j0) * dk, valid, dk);
        stage(sB, LDK, KW, b_ + (base + j0) * dk, valid, dk);
        stage(sV, LDV, VW, v + (base + j0) * dv, valid, dv);
        stage(sC, LDV, VW, c_ + (base + j0) * dv, valid, dv);
        __syncthreads();
        f32x4 s[4], tt[4], dp[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = tt[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < dk; kk += 4) {
            const float qa = qp[kk], aa = ap[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float kb = sK[(li + 16 * t) * LDK + lg + kk];
                s[t] = MFMA4(qa, kb, s[t]);
                tt[t] = MFMA4(aa, kb, tt[t]);
                tt[t] = MFMA4(qa, sB[(li + 16 * t) * LDK + lg + kk], tt[t]);
            }
        }
        for (int kk = 0; kk < dv; kk += 4) {
            const float ga = gp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) dp[t] = MFMA4(ga, sV[(li + 16 * t) * LDV + lg + kk], dp[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool in = j0 + li + 16 * t < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = in ? expf(s[t][r] - ls[r]) : 0.f;
                const float pt = p * tt[t][r];
                tau[r] += pt;
                rho[r] += pt * dp[t][r];
                sX[(4 * lg + r) * LDP + li + 16 * t] = p;
            }
        }
        __syncthreads();
        for (int kk = 0; kk < TN; kk += 4) {
            const float ax = sX[li * LDP + lg + kk];
#pragma unroll
            for (int c = 0; c < DVT; ++c)
                if (16 * c < dv) pc[c] = MFMA4(ax, sC[(lg + kk) * LDV + li + 16 * c], pc[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wave + 4 * lg + r, rc = min(row, N - 1);
        float gpc = 0.f;
#pragma unroll
        for (int c = 0; c < DVT; ++c)
            if (16 * c < dv) gpc += gout[(base + rc) * dv + li + 16 * c] * pc[c][r];
        tau[r] = row_sum(tau[r]);
        rho[r] = row_sum(rho[r]) - 2.f * tau[r] * dl[r] + row_sum(gpc);
        if (li == 0 && row < N) {
            tau_out[base + row] = tau[r];
            rho_out[base + row] = rho[r];
        }
    }
    f32x4 g[DKT];
#pragma unroll
    for (int c = 0; c < DKT; ++c) g[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- sweep 2: d q, d gout
    for (int j0 = 0; j0 < N; j0 += TN) {
        __syncthreads();
        const int valid = min(TN, N - j0);
        stage(sK, LDK, KW, k + (base + j0) * dk, valid, dk);
        stage(sB, LDK, KW, b_ + (base + j0) * dk, valid, dk);
        stage(sV, LDV, VW, v + (base + j0) * dv, valid, dv);
        stage(sC, LDV, VW, c_ + (base + j0) * dv, valid, dv);
        __syncthreads();
        f32x4 s[4], tt[4], dp[4], gc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = tt[t] = dp[t] = gc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < dk; kk += 4) {
            const float qa = qp[kk], aa = ap[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float kb = sK[(li + 16 * t) * LDK + lg + kk];
                s[t] = MFMA4(qa, kb, s[t]);
                tt[t] = MFMA4(aa, kb, tt[t]);
                tt[t] = MFMA4(qa, sB[(li + 16 * t) * LDK + lg + kk], tt[t]);
            }
        }
        for (int kk = 0; kk < dv; kk += 4) {
            const float ga = gp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                dp[t] = MFMA4(ga, sV[(li + 16 * t) * LDV + lg + kk], dp[t]);
                gc[t] = MFMA4(ga, sC[(li + 16 * t) * LDV + lg + kk], gc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool in = j0 + li + 16 * t < N;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = in ? expf(s[t][r] - ls[r]) : 0.f;
                const float T = tt[t][r], d = dp[t][r];
                const float pbar = T * d - d * tau[r] - T * dl[r] + gc[t][r];
                const int at = (4 * lg + r) * LDP + li + 16 * t;
                sX[at] = p * (pbar - rho[r]);
                sY[at] = p * (d - dl[r]);
                sZ[at] = p * (T - tau[r]);
            }
        }
        __syncthreads();
        for (int kk = 0; kk < TN; kk += 4) {
            const float ax = sX[li * LDP + lg + kk], ay = sY[li * LDP + lg + kk], az = sZ[li * LDP + lg + kk];
#pragma unroll
            for (int c = 0; c < DKT; ++c) {
                g[c] = MFMA4(ax, sK[(lg + kk) * LDK + li + 16 * c], g[c]);
                g[c] = MFMA4(ay, sB[(lg + kk) * LDK + li + 16 * c], g[c]);
            }
#pragma unroll
            for (int c = 0; c < DVT; ++c)
                if (16 * c < dv) pc[c] = MFMA4(az, sV[(lg + kk) * LDV + li + 16 * c], pc[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wave + 4 * lg + r;
        if (row >= N) continue;
#pragma unroll
        for (int c = 0; c < DKT; ++c)
            if (li + 16 * c < dk) dq[(base + row) * dk + li + 16 * c] = g[c][r];
#pragma unroll
        for (int c = 0; c < DVT; ++c)
            if (li + 16 * c < dv) dgout[(base + row) * dv + li + 16 * c] = pc[c][r];
    }
}

template <int DKT, int DVT>
__global__ __launch_bounds__(TPB) void attention_bwd2_kv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                const float* __restrict__ lse, const float* __restrict__ delta,
                                                                const float* __restrict__ tau, const float* __restrict__ rho,
                                                                const float* __restrict__ gout, const float* __restrict__ a,
                                                                const float* __restrict__ b_, const float* __restrict__ c_,
                                                                float* __restrict__ dkey, float* __restrict__ dval, int N, int dk, int dv) {
    extern __shared__ __align__(16) float smem[];
    ATT_IDS
    constexpr int QW = 16 * DKT, LDQ = QW + 4, GW = 16 * DVT, LDG = GW + 4;
    float* sQ = smem;
    float* sA = sQ + TN * LDQ;
    float* sG = sA + TN * LDQ;
    float* sL = sG + TN * LDG;
    float* sD = sL + TN;
    float* sT = sD + TN;
    float* sR = sT + TN;
    float* sX = sR + TN + wave * 3 * PTILE;               // Sbar^T
    float* sY = sX + PTILE;                               // dS^T
    float* sZ = sY + PTILE;                               // W^T
    const float* kp = k + (base + arow) * dk + lg;        // this workgroup's rows are keys
    const float* bp = b_ + (base + arow) * dk + lg;
    const float* vp = v + (base + arow) * dv + lg;
    const float* cp = c_ + (base + arow) * dv + lg;
    f32x4 ak[DKT], av[DVT];
#pragma unroll
    for (int c = 0; c < DKT; ++c) ak[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DVT; ++c) av[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int i0 = 0; i0 < N; i0 += TN) {
        __syncthreads();
        const int valid = min(TN, N - i0);
        stage(sQ, LDQ, QW, q + (base + i0) * dk, valid, dk);
        stage(sA, LDQ, QW, a + (base + i0) * dk, valid, dk);
        stage(sG, LDG, GW, gout + (base + i0) * dv, valid, dv);
        if (threadIdx.x < TN) {
            const bool in = (int)threadIdx.x < valid;
            sL[threadIdx.x] = in ? lse[base + i0 + threadIdx.x] : 0.f;
            sD[threadIdx.x] = in ? delta[base + i0 + threadIdx.x] : 0.f;
            sT[threadIdx.x] = in ? tau[base + i0 + threadIdx.x] : 0.f;
            sR[threadIdx.x] = in ? rho[base + i0 + threadIdx.x] : 0.f;
        }
        __syncthreads();
        f32x4 s[4], tt[4], dp[4], gc[4];                  // [key 4 lg + r of the wave][query li + 16 t of the block]
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = tt[t] = dp[t] = gc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < dk; kk += 4) {
            const float ka = kp[kk], ba = bp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float qb = sQ[(li + 16 * t) * LDQ + lg + kk];
                s[t] = MFMA4(ka, qb, s[t]);
                tt[t] = MFMA4(ka, sA[(li + 16 * t) * LDQ + lg + kk], tt[t]);
                tt[t] = MFMA4(ba, qb, tt[t]);
            }
        }
        for (int kk = 0; kk < dv; kk += 4) {
            const float va = vp[kk], ca = cp[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float gb = sG[(li + 16 * t) * LDG + lg + kk];
                dp[t] = MFMA4(va, gb, dp[t]);
                gc[t] = MFMA4(ca, gb, gc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool in = i0 + li + 16 * t < N;
            const float L = sL[li + 16 * t], D = sD[li + 16 * t], Tau = sT[li + 16 * t], Rho = sR[li + 16 * t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = in ? expf(s[t][r] - L) : 0.f;
                const float T = tt[t][r], d = dp[t][r];
                const float pbar = T * d - d * Tau - T * D + gc[t][r];
                const int at = (4 * lg + r) * LDP + li + 16 * t;
                sX[at] = p * (pbar - Rho);
                sY[at] = p * (d - D);
                sZ[at] = p * (T - Tau);
            }
        }
        __syncthreads();
        for (int kk = 0; kk < TN; kk += 4) {
            const float ax = sX[li * LDP + lg + kk], ay = sY[li * LDP + lg + kk], az = sZ[li * LDP + lg + kk];
#pragma unroll
            for (int c = 0; c < DKT; ++c) {
                ak[c] = MFMA4(ax, sQ[(lg + kk) * LDQ + li + 16 * c], ak[c]);
                ak[c] = MFMA4(ay, sA[(lg + kk) * LDQ + li + 16 * c], ak[c]);
            }
#pragma unroll
            for (int c = 0; c < DVT; ++c) av[c] = MFMA4(az, sG[(lg + kk) * LDG + li + 16 * c], av[c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 16 * wave + 4 * lg + r;
        if (row >= N) continue;
#pragma unroll
        for (int c = 0; c < DKT; ++c)
            if (li + 16 * c < dk) dkey[(base + row) * dk + li + 16 * c] = ak[c][r];
#pragma unroll
        for (int c = 0; c < DVT; ++c)
            if (li + 16 * c < dv) dval[(base + row) * dv + li + 16 * c] = av[c][r];
    }
}

// ------------------------------------------------------------------------------------------------------------------ gated residual
__global__ __launch_bounds__(TPB) void attn_residual_fwd_kernel(const float* __restrict__ x, const float* __restrict__ o,
                                                                const float* __restrict__ gamma, float* __restrict__ y, long long n) {
    const float g = gamma[0];
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) y[i] = x[i] + g * o[i];
}

// go = gamma gy; part[block] = the block's share of sum gy o: thread t adds its elements in index order (fp64), then an LDS tree.  The grid
// is RES_PARTS workgroups for every size, so the order depends on n alone.
__global__ __launch_bounds__(TPB) void attn_residual_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ o,
                                                                const float* __restrict__ gamma, float* __restrict__ go,
                                                                double* __restrict__ part, long long n) {
    __shared__ double red[TPB];
    const float g = gamma[0];
    double acc = 0.;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)RES_PARTS * TPB) {
        const float d = gy[i];
        go[i] = g * d;
        acc += (double)d * (double)o[i];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = TPB / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// The backward of the backward above, cgo / cgg the cotangents of go / ggamma: dgy = gamma cgo + cgg o, dO = cgg gy,
// part[block] = the block's share of d gamma = sum cgo gy (the order of attn_residual_bwd_kernel).  cgg may be NULL (zero: dO is not written).
__global__ __launch_bounds__(TPB) void attn_residual_bwd2_kernel(const float* __restrict__ cgo, const float* __restrict__ gy,
                                                                 const float* __restrict__ o, const float* __restrict__ gamma,
                                                                 const float* __restrict__ cgg, float* __restrict__ dgy, float* __restrict__ dO,
                                                                 double* __restrict__ part, long long n) {
    __shared__ double red[TPB];
    const float g = gamma[0];
    const float s = cgg ? cgg[0] : 0.f;
    double acc = 0.;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)RES_PARTS * TPB) {
        const float x = cgo[i], d = gy[i];
        if (cgg) {
            dgy[i] = g * x + s * o[i];
            dO[i] = s * d;
        } else {
            dgy[i] = g * x;
        }
        acc += (double)x * (double)d;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = TPB / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// ggamma = the sum of the RES_PARTS partial sums: one workgroup, an LDS tree, a plain store
__global__ __launch_bounds__(RES_PARTS) void attn_residual_finish_kernel(const double* __restrict__ part, float* __restrict__ ggamma) {
    __shared__ double red[RES_PARTS];
    red[threadIdx.x] = part[threadIdx.x];
    __syncthreads();
    for (int w = RES_PARTS / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) ggamma[0] = (float)red[0];
}

inline hipStream_t S(ctgan_stream_t s) { return static_cast<hipStream_t>(s); }
inline bool misaligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

// LDS of a launch, in bytes (the layouts of the three kernels above)
inline size_t fwd_lds(int dk, int dv) { return sizeof(float) * ((size_t)TN * ld_rows(dk) + (size_t)TN * ld_cols(dv) + 4 * PTILE); }
inline size_t bwd_q_lds(int dkt, int dv) { return sizeof(float) * ((size_t)TN * (16 * dkt + 4) + (size_t)TN * ld_rows(dv) + 4 * PTILE); }
inline size_t bwd_kv_lds(int dkt, int dvt) { return sizeof(float) * ((size_t)TN * (16 * dkt + 4) + (size_t)TN * (16 * dvt + 4) + 2 * TN + 8 * PTILE); }

// a launch with more than the default 64 KB of dynamic LDS asks for it first (once per kernel and size)
template <class Kern>
int grant_lds(Kern kern, size_t bytes, size_t* granted, const char* what) {
    if (bytes <= 64 * 1024 || bytes <= *granted) return CTGAN_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        return ctgan_fail(CTGAN_E_LAUNCH, "%s: %zu bytes of LDS refused", what, bytes);
    }
    *granted = bytes;
    return CTGAN_OK;
}

int check_shape(const char* what, int64_t n, int32_t N, int32_t dk, int32_t dv) {
    if (n < 1 || (long long)n * ((N + TM - 1) / TM) > 0x7fffffffLL) return ctgan_fail(CTGAN_E_BADARG, "%s: n = %lld images", what, (long long)n);
    if (N < 16 || N % 16) return ctgan_fail(CTGAN_E_BADARG, "%s: N = %d tokens (a multiple of 16, at least 16)", what, N);
    if (dk < 4 || dk > 64 || dk % 4) return ctgan_fail(CTGAN_E_BADARG, "%s: dk = %d (a multiple of 4 in [4, 64])", what, dk);
    if (dv < 16 || dv > 128 || dv % 16) return ctgan_fail(CTGAN_E_BADARG, "%s: dv = %d (a multiple of 16 in [16, 128])", what, dv);
    return CTGAN_OK;
}

template <int DVT>
int launch_fwd(const float* q, const float* k, const float* v, float* out, float* lse, unsigned grid, int N, int dk, int dv, hipStream_t st) {
    static size_t granted = 0;
    const size_t lds = fwd_lds(dk, dv);
    if (int rc = grant_lds(attention_fwd_kernel<DVT>, lds, &granted, "attention_fwd")) return rc;
    hipLaunchKernelGGL(attention_fwd_kernel<DVT>, dim3(grid), dim3(TPB), lds, st, q, k, v, out, lse, N, dk, dv);
    return ctgan_check_launch("attention_fwd");
}

template <int DKT>
int launch_bwd_q(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout, float* gq, float* delta,
                 unsigned grid, int N, int dk, int dv, hipStream_t st) {
    static size_t granted = 0;
    const size_t lds = bwd_q_lds(DKT, dv);
    if (int rc = grant_lds(attention_bwd_q_kernel<DKT>, lds, &granted, "attention_bwd (gq)")) return rc;
    hipLaunchKernelGGL(attention_bwd_q_kernel<DKT>, dim3(grid), dim3(TPB), lds, st, q, k, v, out, lse, gout, gq, delta, N, dk, dv);
    return ctgan_check_launch("attention_bwd (gq)");
}

template <int DKT, int DVT>
int launch_bwd_kv(const float* q, const float* k, const float* v, const float* lse, const float* delta, const float* gout, float* gk, float* gv,
                  unsigned grid, int N, int dk, int dv, hipStream_t st) {
    static size_t granted = 0;
    const size_t lds = bwd_kv_lds(DKT, DVT);
    if (int rc = grant_lds(attention_bwd_kv_kernel<DKT, DVT>, lds, &granted, "attention_bwd (gk, gv)")) return rc;
    hipLaunchKernelGGL((attention_bwd_kv_kernel<DKT, DVT>), dim3(grid), dim3(TPB), lds, st, q, k, v, lse, delta, gout, gk, gv, N, dk, dv);
    return ctgan_check_launch("attention_bwd (gk, gv)");
}

template <int DKT>
int launch_bwd_kv_dv(int dvt, const float* q, const float* k, const float* v, const float* lse, const float* delta, const float* gout, float* gk,
                     float* gv, unsigned grid, int N, int dk, int dv, hipStream_t st) {
    if (dvt <= 1) return launch_bwd_kv<DKT, 1>(q, k, v, lse, delta, gout, gk, gv, grid, N, dk, dv, st);
    if (dvt <= 2) return launch_bwd_kv<DKT, 2>(q, k, v, lse, delta, gout, gk, gv, grid, N, dk, dv, st);
    if (dvt <= 4) return launch_bwd_kv<DKT, 4>(q, k, v, lse, delta, gout, gk, gv, grid, N, dk, dv, st);
    return launch_bwd_kv<DKT, 8>(q, k, v, lse, delta, gout, gk, gv, grid, N, dk, dv, st);
}

// the operands of ctgan_attention_bwd2 behind one name each (nine inputs, two [n, N] scratch rows, four outputs)
struct Bwd2Args {
    const float *q, *k, *v, *lse, *delta, *gout, *a, *b, *c;
    float *dq, *dkey, *dval, *dgout, *tau, *rho;
};

inline size_t bwd2_q_lds(int dkt, int dvt) {
    return sizeof(float) * (2 * (size_t)TN * (16 * dkt + 4) + 2 * (size_t)TN * (16 * dvt + 4) + 12 * PTILE);
}
inline size_t bwd2_kv_lds(int dkt, int dvt) {
    return sizeof(float) * (2 * (size_t)TN * (16 * dkt + 4) + (size_t)TN * (16 * dvt + 4) + 4 * TN + 12 * PTILE);
}

template <int DKT, int DVT>
int launch_bwd2(const Bwd2Args& p, unsigned grid, int N, int dk, int dv, hipStream_t st) {
    static size_t granted_q = 0, granted_kv = 0;
    const size_t lds_q = bwd2_q_lds(DKT, DVT), lds_kv = bwd2_kv_lds(DKT, DVT);
    if (int rc = grant_lds(attention_bwd2_q_kernel<DKT, DVT>, lds_q, &granted_q, "attention_bwd2 (dq, dgout)")) return rc;
    if (int rc = grant_lds(attention_bwd2_kv_kernel<DKT, DVT>, lds_kv, &granted_kv, "attention_bwd2 (dk, dv)")) return rc;
    hipLaunchKernelGGL((attention_bwd2_q_kernel<DKT, DVT>), dim3(grid), dim3(TPB), lds_q, st, p.q, p.k, p.v, p.lse, p.delta, p.gout, p.a, p.b, p.c,
                       p.dq, p.dgout, p.tau, p.rho, N, dk, dv);
    if (int rc = ctgan_check_launch("attention_bwd2 (dq, dgout)")) return rc;
    hipLaunchKernelGGL((attention_bwd2_kv_kernel<DKT, DVT>), dim3(grid), dim3(TPB), lds_kv, st, p.q, p.k, p.v, p.lse, p.delta, p.tau, p.rho, p.gout,
                       p.a, p.b, p.c, p.dkey, p.dval, N, dk, dv);
    return ctgan_check_launch("attention_bwd2 (dk, dv)");
}

template <int DKT>
int launch_bwd2_dv(int dvt, const Bwd2Args& p, unsigned grid, int N, int dk, int dv, hipStream_t st) {
    if (dvt <= 1) return launch_bwd2<DKT, 1>(p, grid, N, dk, dv, st);
    if (dvt <= 2) return launch_bwd2<DKT, 2>(p, grid, N, dk, dv, st);
    if (dvt <= 4) return launch_bwd2<DKT, 4>(p, grid, N, dk, dv, st);
    return launch_bwd2<DKT, 8>(p, grid, N, dk, dv, st);
}

}  // namespace

extern "C" {

int ctgan_attention_fwd(const float* q, const float* k, const float* v, float* out, float* lse, int64_t n, int32_t N, int32_t dk, int32_t dv,
                        ctgan_stream_t stream) {
    if (int rc = check_shape("attention_fwd", n, N, dk, dv)) return rc;
    if (!q || !k || !v || !out) return ctgan_fail(CTGAN_E_BADARG, "attention_fwd: a null pointer (q, k, v, out; only lse may be NULL)");
    if (misaligned16(q) || misaligned16(k) || misaligned16(v) || misaligned16(out))
        return ctgan_fail(CTGAN_E_BADARG, "attention_fwd: q, k, v, out not 16-byte aligned");
    const unsigned grid = (unsigned)(n * ((N + TM - 1) / TM));
    const int dvt = dv / 16;
    if (dvt <= 1) return launch_fwd<1>(q, k, v, out, lse, grid, N, dk, dv, S(stream));
    if (dvt <= 2) return launch_fwd<2>(q, k, v, out, lse, grid, N, dk, dv, S(stream));
    if (dvt <= 4) return launch_fwd<4>(q, k, v, out, lse, grid, N, dk, dv, S(stream));
    return launch_fwd<8>(q, k, v, out, lse, grid, N, dk, dv, S(stream));
}

int ctgan_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* gout, float* gq,
                        float* gk, float* gv, float* delta, int64_t n, int32_t N, int32_t dk, int32_t dv, ctgan_stream_t stream) {
    if (int rc = check_shape("attention_bwd", n, N, dk, dv)) return rc;
    if (!q || !k || !v || !out || !lse || !gout || !gq || !gk || !gv || !delta)
        return ctgan_fail(CTGAN_E_BADARG, "attention_bwd: a null pointer (q, k, v, out, lse, gout, gq, gk, gv, delta)");
    if (misaligned16(q) || misaligned16(k) || misaligned16(v) || misaligned16(gout))
        return ctgan_fail(CTGAN_E_BADARG, "attention_bwd: q, k, v, gout not 16-byte aligned");
    const unsigned grid = (unsigned)(n * ((N + TM - 1) / TM));
    const int dkt = (dk + 15) / 16, dvt = dv / 16;
    int rc;
    if (dkt <= 1) rc = launch_bwd_q<1>(q, k, v, out, lse, gout, gq, delta, grid, N, dk, dv, S(stream));
    else if (dkt <= 2) rc = launch_bwd_q<2>(q, k, v, out, lse, gout, gq, delta, grid, N, dk, dv, S(stream));
    else rc = launch_bwd_q<4>(q, k, v, out, lse, gout, gq, delta, grid, N, dk, dv, S(stream));
    if (rc) return rc;
    if (dkt <= 1) return launch_bwd_kv_dv<1>(dvt, q, k, v, lse, delta, gout, gk, gv, grid, N, dk, dv, S(stream));
    if (dkt <= 2) return launch_bwd_kv_dv<2>(dvt, q, k, v, lse, delta, gout, gk, gv, grid, N, dk, dv, S(stream));
    return launch_bwd_kv_dv<4>(dvt, q, k, v, lse, delta, gout, gk, gv, grid, N, dk, dv, S(stream));
}

int ctgan_attention_bwd2(const float* q, const float* k, const float* v, const float* lse, const float* delta, const float* gout, const float* a,
                         const float* b, const float* c, float* dq, float* dkey, float* dval, float* dgout, float* tau, float* rho, int64_t n,
                         int32_t N, int32_t dk, int32_t dv, ctgan_stream_t stream) {
    if (int rc = check_shape("attention_bwd2", n, N, dk, dv)) return rc;
    if (!q || !k || !v || !lse || !delta || !gout || !a || !b || !c || !dq || !dkey || !dval || !dgout || !tau || !rho)
        return ctgan_fail(CTGAN_E_BADARG, "attention_bwd2: a null pointer (q, k, v, lse, delta, gout, a, b, c, dq, dk, dv, dgout, tau, rho)");
    if (misaligned16(q) || misaligned16(k) || misaligned16(v) || misaligned16(gout) || misaligned16(a) || misaligned16(b) || misaligned16(c))
        return ctgan_fail(CTGAN_E_BADARG, "attention_bwd2: q, k, v, gout, a, b, c not 16-byte aligned");
    const unsigned grid = (unsigned)(n * ((N + TM - 1) / TM));
    const int dkt = (dk + 15) / 16, dvt = dv / 16;
    const Bwd2Args p = {q, k, v, lse, delta, gout, a, b, c, dq, dkey, dval, dgout, tau, rho};
    if (dkt <= 1) return launch_bwd2_dv<1>(dvt, p, grid, N, dk, dv, S(stream));
    if (dkt <= 2) return launch_bwd2_dv<2>(dvt, p, grid, N, dk, dv, S(stream));
    return launch_bwd2_dv<4>(dvt, p, grid, N, dk, dv, S(stream));
}

int ctgan_attn_residual_parts(void) { return RES_PARTS; }

int ctgan_attn_residual_fwd(const float* x, const float* o, const float* gamma, float* y, int64_t n, ctgan_stream_t stream) {
    if (n < 1) return ctgan_fail(CTGAN_E_BADARG, "attn_residual_fwd: n = %lld elements", (long long)n);
    if (!x || !o || !gamma || !y) return ctgan_fail(CTGAN_E_BADARG, "attn_residual_fwd: a null pointer (x, o, gamma, y)");
    hipLaunchKernelGGL(attn_residual_fwd_kernel, dim3(ctgan_blocks(n, TPB * 4)), dim3(TPB), 0, S(stream), x, o, gamma, y, (long long)n);
    return ctgan_check_launch("attn_residual_fwd");
}

int ctgan_attn_residual_bwd(const float* gy, const float* o, const float* gamma, float* go, float* ggamma, double* part, int64_t n,
                            ctgan_stream_t stream) {
    if (n < 1) return ctgan_fail(CTGAN_E_BADARG, "attn_residual_bwd: n = %lld elements", (long long)n);
    if (!gy || !o || !gamma || !go || !ggamma || !part) return ctgan_fail(CTGAN_E_BADARG, "attn_residual_bwd: a null pointer (gy, o, gamma, go, ggamma, part)");
    if (reinterpret_cast<uintptr_t>(part) & 7) return ctgan_fail(CTGAN_E_BADARG, "attn_residual_bwd: part not 8-byte aligned");
    hipLaunchKernelGGL(attn_residual_bwd_kernel, dim3(RES_PARTS), dim3(TPB), 0, S(stream), gy, o, gamma, go, part, (long long)n);
    if (int rc = ctgan_check_launch("attn_residual_bwd")) return rc;
    hipLaunchKernelGGL(attn_residual_finish_kernel, dim3(1), dim3(RES_PARTS), 0, S(stream), part, ggamma);
    return ctgan_check_launch("attn_residual_bwd (finish)");
}

int ctgan_attn_residual_bwd2(const float* cgo, const float* gy, const float* o, const float* gamma, const float* cgg, float* dgy, float* d_o,
                             float* dgamma, double* part, int64_t n, ctgan_stream_t stream) {
    if (n < 1) return ctgan_fail(CTGAN_E_BADARG, "attn_residual_bwd2: n = %lld elements", (long long)n);
    if (!cgo || !gy || !o || !gamma || !dgy || !dgamma || !part || (cgg && !d_o))
        return ctgan_fail(CTGAN_E_BADARG, "attn_residual_bwd2: a null pointer (cgo, gy, o, gamma, dgy, dgamma, part; d_o with cgg; only cgg may be NULL)");
    if (reinterpret_cast<uintptr_t>(part) & 7) return ctgan_fail(CTGAN_E_BADARG, "attn_residual_bwd2: part not 8-byte aligned");
    hipLaunchKernelGGL(attn_residual_bwd2_kernel, dim3(RES_PARTS), dim3(TPB), 0, S(stream), cgo, gy, o, gamma, cgg, dgy, d_o, part, (long long)n);
    if (int rc = ctgan_check_launch("attn_residual_bwd2")) return rc;
    hipLaunchKernelGGL(attn_residual_finish_kernel, dim3(1), dim3(RES_PARTS), 0, S(stream), part, dgamma);
    return ctgan_check_launch("attn_residual_bwd2 (finish)");
}

}  // extern "C"
