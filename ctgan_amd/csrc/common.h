// common.h - shared host-side helpers of libctgan_hip.so (error reporting, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/ctgan_hip.h"
#include "../../include/ctgan_hip_debug.h"

// thread-local last-error message (no exception crosses the C ABI)
int ctgan_fail(int code, const char* fmt, ...);
// hipGetLastError() after a launch -> CTGAN_E_LAUNCH with the HIP error string
int ctgan_check_launch(const char* what);
// split-K plan of the weight-gradient GEMM (shared by the launcher and the workspace query)
void ctgan_wgrad_split(int tiles, int Kg, int* splits, int* chunk);

static inline unsigned ctgan_blocks(long long n, int per_block, int cap = 4096) {
    long long b = (n + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// ---- ctgan_epilogue_ext -> the kernels' dropout parameters (igemm.hip FwdParams, igemm16.hip P16) ----
// a tensor of C channels on an H x W grid with these (n, c, h, w) element strides is dense channels-last
static inline bool dense_channels_last(const int64_t* s, int C, int H, int W) {
    return s[1] == 1 && s[3] == C && s[2] == (int64_t)W * C && s[0] == (int64_t)H * W * C;
}
static inline bool keep_drops(float keep) { return keep > 0.f && keep < 1.f; }
// ext asks for a dropout that drops something: one keep in (0,1), or a range with one
static inline bool ext_wants_drop(const ctgan_epilogue_ext* ext) {
    if (!ext) return false;
    if (ext->n_ranges > 0) {
        for (int i = 0; i < ext->n_ranges && i < CTGAN_DROP_RANGES; ++i)
            if (keep_drops(ext->range_keep[i])) return true;
        return false;
    }
    return keep_drops(ext->drop_keep);
}
// Fills the drop* fields of a kernel parameter struct: everything off unless `on`, then the seed / counter and either the one keep /
// stream or, with n_ranges > 0, per range its end (first row past it, written to `ends` - the struct's drop_mend with rows_per_sample =
// pixels per sample, or its drop_nend with rows_per_sample = 1), keep (outside (0,1) = 1: none), stream and the offset of its first
// element (sample_elems = elements of one sample of the dense result).  Validation - range count, boundaries, layout - is the caller's.
template <class P>
static void set_drop(P& p, int (&ends)[CTGAN_DROP_RANGES], const ctgan_epilogue_ext* ext, bool on, long long rows_per_sample, long long sample_elems) {
    p.drop = 0; p.drop_keep = 1.f; p.drop_seed = 0; p.drop_sid = 0; p.drop_ctr = nullptr; p.drop_nr = 0;
    for (int i = 0; i < CTGAN_DROP_RANGES; ++i) { ends[i] = 0x7fffffff; p.drop_rkeep[i] = 1.f; p.drop_rsid[i] = 0; p.drop_roff[i] = 0; }
    if (!on) return;
    p.drop = 1; p.drop_seed = ext->drop_seed;
    p.drop_ctr = reinterpret_cast<const unsigned long long*>(ext->drop_ctr);
    if (ext->n_ranges > 0) {
        p.drop_nr = ext->n_ranges < CTGAN_DROP_RANGES ? ext->n_ranges : CTGAN_DROP_RANGES;
        long long start = 0;
        for (int i = 0; i < p.drop_nr; ++i) {
            ends[i] = (int)(ext->range_end[i] * rows_per_sample);
            p.drop_rkeep[i] = keep_drops(ext->range_keep[i]) ? ext->range_keep[i] : 1.f;
            p.drop_rsid[i] = (unsigned)ext->range_stream_id[i];
            p.drop_roff[i] = start * sample_elems;
            start = ext->range_end[i];
        }
    } else if (keep_drops(ext->drop_keep)) {
        p.drop_keep = ext->drop_keep; p.drop_sid = (unsigned)ext->drop_stream_id;
    }
}

// bn.hip, for bn_act.hip: the chunk plan of the partial reductions (part[(sample*hc + chunk)][2][c], `pos` positions per chunk) and the
// finalisation of the backward's sums (no labels): part -> gscale, goffset [c] and s12 [groups][2][c] = mean(g scale), mean(g scale xhat)
void ctgan_bn_plan(int n, int hw, int* hc, int* pos);
int ctgan_bn_bwd_finalize(const double* part, const float* scale, int n, int hw, int c, int groups, float* gscale, float* goffset,
                          float* s12, hipStream_t st);

// skinny.hip: small-N linear layers (critic heads)
bool ctgan_is_small_linear(const ctgan_conv_desc* d);
int ctgan_small_linear_fwd(const ctgan_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int relu,
                           hipStream_t st);
int ctgan_small_linear_dgrad(const ctgan_conv_desc* d, const float* gy, const float* w, const float* bias, float* gx,
                             hipStream_t st);
int ctgan_small_linear_wgrad(const ctgan_conv_desc* d, const float* x, const float* gy, float* gw, float* gb, hipStream_t st);
// per-thread name of the kernel variant the last conv call dispatched to
void ctgan_set_last_kernel(const char* name);
// ... and the device symbol of that launch as rocprofv3 prints it (template arguments spelled the compiler's way), so that
// bench.py's per-kernel table can be looked up in a committed rocprof summary.  ctgan_set_last_kernel clears it.
void ctgan_set_last_symbol(const char* fmt, ...);

// fewch.hip: direct kernels for convs with <= 4 channels on one side.  fwd / dgrad / wgrad return 1 when they
// handled the call, 0 when the caller should fall through to the GEMM kernels, < 0 on error.
bool ctgan_fewch_handles(const ctgan_conv_desc* d);
int ctgan_fewch_fwd(const ctgan_conv_desc* d, const float* x, const float* w, const float* bias, const float* mask, const float* resid,
                    float* y, int relu, int relu_in, hipStream_t st);
int ctgan_fewch_fwd_bn(const ctgan_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int relu_in, const float* mean,
                       const float* rstd, const float* scale, const float* offset, int groups, int tanh_out, hipStream_t st);
int ctgan_fewch_dgrad(const ctgan_conv_desc* d, const float* dy, const float* w, const float* bias, float* dx, hipStream_t st);
size_t ctgan_fewch_wgrad_workspace(const ctgan_conv_desc* d);
int ctgan_fewch_wgrad(const ctgan_conv_desc* d, const float* x, const float* dy, float* dw, float* db, void* ws, size_t ws_bytes,
                      int relu_x, hipStream_t st);
int ctgan_fewch_wgrad2(const ctgan_conv_desc* d, const float* x, const float* dy, int N0, int relu_x, int bias0, const float* x1,
                       const float* dy1, int N1, int relu_x1, int bias1, float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t st);
