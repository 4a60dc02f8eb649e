// ssl_te.hip - what the temporal-ensembling CT classifier (ct_cifar_te.py; TH/ = CT-GANs/Theano_classifier of the reference,
// TH/CT_CIFAR-10_TE.py) needs beyond ssl.hip and ssl_conv.hip: the loss head whose consistency term is taken against per-example
// TARGET rows (:116-122) - read from the device-resident tables by index, with this pass's unlabelled logits and features scattered
// into the epoch's prediction tables in the same launch (:300-302) - its backward, and the epoch-end ensemble update (:305-309).
//
// As in ssl.hip every reduction runs in a fixed order (strided per-lane partial sums, a fixed butterfly inside a 16-lane row group,
// a fixed LDS tree over the workgroup) and there are no float atomics, so a replayed graph is bit-stable.
#include "common.h"
#include "ssl_common.h"

namespace {
using namespace ctgan_ssl;

constexpr int WG = 256;
constexpr int LPR = 16;             // lanes of one row group: a wave holds four rows, a workgroup RPB
constexpr int RPB = WG / LPR;
constexpr int NQ = 8;               // quantities the forward reduces over the batch

// sum over the LPR lanes of a row group in a fixed butterfly order; every lane of the group receives it.  Called by whole waves.
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int w = LPR / 2; w > 0; w >>= 1) v += __shfl_xor(v, w, LPR);
    return v;
}
// sum_j (f_j - t2_j)^2 / F of one row: lane `sub` takes columns sub, sub + LPR, ..; t2 == nullptr (row inactive or index out of
// range): 0 from every lane.  The forward and the backward both call this, so both see the same hinge.
__device__ __forceinline__ float row_ctf(const float* __restrict__ f, const float* __restrict__ t2, int F, int sub) {
    float acc = 0.f;
    if (t2)
        for (int j = sub; j < F; j += LPR) { const float d = f[j] - t2[j]; acc += d * d; }
    return group_sum(acc) / (float)F;
}

// ------------------------------------------------------------------------------------------------ head, forward
// logits [3B, nc], feat [3B, F] = [lab ; unl ; fake];  targets [N, nc] (raw ensembled logits), targets2 [N, F];  idx [B] rows of
// the unlabelled examples.  out8 = {loss_lab, loss_unl, CT_, train_err, train_err2, mean ct, mean ctf, 0};  pred[idx[i]] <- logits
// row B + i, pred2[idx[i]] <- feature row B + i (plain stores: duplicate indices are memory-safe, the surviving row unspecified).
// ONE workgroup (the scalars are sums over the batch).  Row i belongs to the 16-lane group i % RPB: the group strides the F feature
// columns (the squared distance to the target row and the copy into pred2) and the nc logit columns of the copy into pred; then
// its lane 0 takes the unlabelled row's logit terms, lane 1 the labelled row's and lane 2 the generated row's.
__global__ void __launch_bounds__(WG) te_head_fwd_kernel(const float* __restrict__ lg, const float* __restrict__ ft, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ idx, const float* __restrict__ tg, const float* __restrict__ tg2,
                                                         int B, int nc, int F, int N, float lam2, float feat_w, float M, float* __restrict__ out,
                                                         float* __restrict__ pred, float* __restrict__ pred2) {
    __shared__ float red[NQ][WG];
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    for (int i0 = 0; i0 < B; i0 += RPB) {               // uniform trip count: group_sum is reached by whole waves
        const int i = i0 + grp;
        const bool on = i < B;
        const int src = on ? idx[i] : -1;
        const bool ok = on && src >= 0 && src < N;
        const float* u = lg + (long long)(B + (on ? i : 0)) * nc;
        const float* fu = ft + (long long)(B + (on ? i : 0)) * F;
        const float* t2 = ok ? tg2 + (long long)src * F : nullptr;
        const float ctf = row_ctf(fu, t2, F, sub);
        if (ok) {
            float* p2 = pred2 + (long long)src * F;
            for (int j = sub; j < F; j += LPR) p2[j] = fu[j];
            float* p1 = pred + (long long)src * nc;
            for (int k = sub; k < nc; k += LPR) p1[k] = u[k];
        }
        if (!on) continue;
        if (sub == 0) {
            const RowStat su = row_stat(u, nc);
            if (ok) {
                const float* t = tg + (long long)src * nc;
                const float ct = row_ct(u, t, su, row_stat(t, nc), nc);
                acc[1] += fmaxf(lam2 * (ct + feat_w * ctf) - M, 0.f);
                acc[6] += ct;
                acc[7] += ctf;
            } else {                                    // an index outside [0, N) poisons loss_unl, reads and writes nothing
                acc[1] += nan_f(); acc[6] += nan_f(); acc[7] += nan_f();
            }
            acc[2] += softplus_f(su.lse) - su.lse;
        } else if (sub == 1) {
            const float* l = lg + (long long)i * nc;
            const RowStat sl = row_stat(l, nc);
            const int yi = labels[i];
            const float ly = (yi >= 0 && yi < nc) ? l[yi] : nan_f();       // a label outside [0, nc) poisons loss_lab, reads nothing
            int am = 0;
            for (int k = 1; k < nc; ++k) if (l[k] > l[am]) am = k;          // first maximum, as argmax
            acc[0] += sl.lse - ly;
            acc[4] += am != yi ? 1.f : 0.f;
            acc[5] += sl.mx <= 0.f ? 1.f : 0.f;
        } else if (sub == 2) {
            acc[3] += softplus_f(row_stat(lg + (long long)(2 * B + i) * nc, nc).lse);
        }
    }
    block_tree(red, acc);
    if (threadIdx.x == 0) {
        const float inv = 1.f / (float)B;
        const float CT = red[1][0] * inv;
        out[0] = red[0][0] * inv;
        out[1] = 0.5f * (CT + red[2][0] * inv + red[3][0] * inv);
        out[2] = CT;
        out[3] = red[4][0] * inv;
        out[4] = red[5][0] * inv;
        out[5] = red[6][0] * inv;
        out[6] = red[7][0] * inv;
        out[7] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ head, backward
// glogits [3B, nc] and gfeat [3B, F] of gout[0] * loss_lab + gout[1] * loss_unl, recomputed from the logits, the features and the
// target rows.  One 16-lane group per row of the stacked batch, RPB rows per workgroup.  With p = softmax(u), q = softmax(t),
// w_i = [CT_i > 0] gout[1] lam2 / (2B):   d/du_k = gout[1] / (2B) (sigmoid(lse) - 1) p_k + w_i (2 / nc) p_k ((p_k - q_k) - sum_m (p_m - q_m) p_m)
// and d/df_j = w_i feat_w 2 (f_j - t2_j) / F;  gfeat is exactly 0 on the labelled and generated rows.  An unlabelled row whose
// index lies outside [0, N) reads no table and gets NaN (its loss is NaN).
__global__ void __launch_bounds__(WG) te_head_bwd_kernel(const float* __restrict__ lg, const float* __restrict__ ft, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ idx, const float* __restrict__ tg, const float* __restrict__ tg2,
                                                         const float* __restrict__ gout, int B, int nc, int F, int N, float lam2, float feat_w,
                                                         float M, float* __restrict__ gl, float* __restrict__ gf) {
    const int sub = threadIdx.x % LPR;
    const long long r = (long long)blockIdx.x * RPB + threadIdx.x / LPR;
    const bool on = r < 3LL * B;
    const int p = on ? (int)(r / B) : -1, i = on ? (int)(r % B) : 0;
    const int src = p == 1 ? idx[i] : -1;
    const bool ok = p == 1 && src >= 0 && src < N;
    const float* l = lg + (on ? r : 0) * nc;
    const float* f = ft + (on ? r : 0) * F;
    const float* t2 = ok ? tg2 + (long long)src * F : nullptr;
    const float ctf = row_ctf(f, t2, F, sub);           // reached by every lane of the workgroup
    if (!on) return;
    float* o = gl + r * nc;
    float* of = gf + r * F;
    const float g_lab = gout[0] / (float)B, g_unl = 0.5f * gout[1] / (float)B;
    const RowStat sr = row_stat(l, nc);
    if (p == 0) {
        const int yi = labels[i];
        for (int k = sub; k < nc; k += LPR) o[k] = g_lab * (prob(l[k], sr) - (k == yi ? 1.f : 0.f));
        for (int j = sub; j < F; j += LPR) of[j] = 0.f;
    } else if (p == 2) {
        const float sg = g_unl * sigmoid_f(sr.lse);
        for (int k = sub; k < nc; k += LPR) o[k] = sg * prob(l[k], sr);
        for (int j = sub; j < F; j += LPR) of[j] = 0.f;
    } else if (!ok) {
        for (int k = sub; k < nc; k += LPR) o[k] = nan_f();
        for (int j = sub; j < F; j += LPR) of[j] = nan_f();
    } else {
        const float* t = tg + (long long)src * nc;
        const RowStat st = row_stat(t, nc);
        const float ct = row_ct(l, t, sr, st, nc);
        const float w = (lam2 * (ct + feat_w * ctf) - M > 0.f) ? g_unl * lam2 : 0.f;
        float dot = 0.f;                                                       // sum_m (p_m - q_m) p_m
        for (int k = 0; k < nc; ++k) { const float pk = prob(l[k], sr); dot += (pk - prob(t[k], st)) * pk; }
        const float slse = g_unl * (sigmoid_f(sr.lse) - 1.f);                 // d (softplus(lse) - lse) / d lse
        const float wl = w * 2.f / (float)nc, wf = w * feat_w * 2.f / (float)F;
        for (int k = sub; k < nc; k += LPR) {
            const float pk = prob(l[k], sr);
            o[k] = slse * pk + wl * pk * ((pk - prob(t[k], st)) - dot);
        }
        for (int j = sub; j < F; j += LPR) of[j] = wf * (f[j] - t2[j]);
    }
}

// ------------------------------------------------------------------------------------------------ ensemble update
// ens = decay ens + (1 - decay) pred;  targets = ens inv_corr;  pred = 0   (TH/CT_CIFAR-10_TE.py:305-309, :273-274).  The float4
// body and the scalar tail round alike (no contraction).
__device__ __forceinline__ float ens_elem(float e, float p, float decay, float omd) {
#pragma clang fp contract(off)
    return decay * e + omd * p;
}
__global__ void te_ensemble_kernel(float* __restrict__ ens, float* __restrict__ tg, float* __restrict__ pred, long long n, long long n4,
                                   float decay, float inv_corr) {
    const float omd = 1.f - decay;
    const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float4* e4 = reinterpret_cast<float4*>(ens);
    float4* t4 = reinterpret_cast<float4*>(tg);
    float4* p4 = reinterpret_cast<float4*>(pred);
    for (long long v = t0; v < n4; v += stride) {
        float4 e = e4[v];
        const float4 p = p4[v];
        e.x = ens_elem(e.x, p.x, decay, omd); e.y = ens_elem(e.y, p.y, decay, omd);
        e.z = ens_elem(e.z, p.z, decay, omd); e.w = ens_elem(e.w, p.w, decay, omd);
        e4[v] = e;
        t4[v] = make_float4(e.x * inv_corr, e.y * inv_corr, e.z * inv_corr, e.w * inv_corr);
        p4[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long k = 4 * n4 + t0; k < n; k += stride) {       // scalar tail (everything, when the pointers are not 16-byte aligned)
        const float e = ens_elem(ens[k], pred[k], decay, omd);
        ens[k] = e;
        tg[k] = e * inv_corr;
        pred[k] = 0.f;
    }
}

inline bool bad_head_shape(int32_t b, int32_t nc, int32_t fdim, int32_t n) {
    return b <= 0 || nc <= 0 || fdim <= 0 || n <= 0 || b > (1 << 24) || nc > (1 << 16) || fdim > (1 << 24);
}

}  // namespace

extern "C" {

int ctgan_te_head_fwd(const float* logits, const float* feat, const int32_t* labels, const int32_t* idx, const float* targets,
                      const float* targets2, int32_t b, int32_t nc, int32_t fdim, int32_t n, float lam2, float feat_w, float m, float* out8,
                      float* pred, float* pred2, ctgan_stream_t stream) {
    if (!logits || !feat || !labels || !idx || !targets || !targets2 || !out8 || !pred || !pred2)
        return ctgan_fail(CTGAN_E_BADARG, "te_head_fwd: null pointer");
    if (bad_head_shape(b, nc, fdim, n)) return ctgan_fail(CTGAN_E_BADARG, "te_head_fwd: bad shape b %d nc %d f %d n %d", b, nc, fdim, n);
    hipLaunchKernelGGL(te_head_fwd_kernel, dim3(1), dim3(WG), 0, S(stream), logits, feat, labels, idx, targets, targets2, b, nc, fdim, n, lam2,
                       feat_w, m, out8, pred, pred2);
    return ctgan_check_launch("te_head_fwd");
}

int ctgan_te_head_bwd(const float* logits, const float* feat, const int32_t* labels, const int32_t* idx, const float* targets,
                      const float* targets2, const float* gout, int32_t b, int32_t nc, int32_t fdim, int32_t n, float lam2, float feat_w, float m,
                      float* glogits, float* gfeat, ctgan_stream_t stream) {
    if (!logits || !feat || !labels || !idx || !targets || !targets2 || !gout || !glogits || !gfeat)
        return ctgan_fail(CTGAN_E_BADARG, "te_head_bwd: null pointer");
    if (bad_head_shape(b, nc, fdim, n)) return ctgan_fail(CTGAN_E_BADARG, "te_head_bwd: bad shape b %d nc %d f %d n %d", b, nc, fdim, n);
    hipLaunchKernelGGL(te_head_bwd_kernel, dim3((unsigned)((3LL * b + RPB - 1) / RPB)), dim3(WG), 0, S(stream), logits, feat, labels, idx, targets,
                       targets2, gout, b, nc, fdim, n, lam2, feat_w, m, glogits, gfeat);
    return ctgan_check_launch("te_head_bwd");
}

int ctgan_te_ensemble_update(float* ens, float* targets, float* pred, int64_t n, float decay, float inv_corr, ctgan_stream_t stream) {
    if (!ens || !targets || !pred) return ctgan_fail(CTGAN_E_BADARG, "te_ensemble_update: null pointer");
    if (n < 0 || !(decay >= 0.f && decay < 1.f) || !(inv_corr > 0.f))
        return ctgan_fail(CTGAN_E_BADARG, "te_ensemble_update: bad n %lld, decay %g or correction %g", (long long)n, decay, inv_corr);
    if (n == 0) return CTGAN_OK;
    const bool aligned = (((uintptr_t)ens | (uintptr_t)targets | (uintptr_t)pred) & 15) == 0;
    const long long n4 = aligned ? n / 4 : 0;
    hipLaunchKernelGGL(te_ensemble_kernel, dim3(ctgan_blocks(n4 ? n4 : n, 256, 2048)), dim3(256), 0, S(stream), ens, targets, pred, (long long)n,
                       n4, decay, inv_corr);
    return ctgan_check_launch("te_ensemble_update");
}

}  // extern "C"
