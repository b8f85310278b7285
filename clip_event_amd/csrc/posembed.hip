// Resampling of the image tower's positional table to another patch grid, and the text tower's table at another
// context length (ce_pos_stretch_fwd / ce_pos_stretch_bwd, further down).
//
//   ce_pos_resample_fwd   out  [g_out^2 + 1, D] = class row copied, grid rows (Wy (x) Wx) pos
//   ce_pos_resample_bwd   dpos [g_in^2 + 1, D] (+)= the transpose applied to dout, in gather form
//
// The separable bicubic, antialiased weights Wy, Wx (dense fp32 [g_out, g_in], device memory) are the caller's: host arithmetic
// (clip_event_amd/posembed.py).  A zero weight is a tap outside the row's support and is skipped.  One 64-lane workgroup owns one
// table row and 256 of its columns, four columns (16 bytes) per lane; the row index is the block index, so every weight a
// workgroup reads is wave-uniform (scalar loads).  Both sums of an element run in ascending index order in fp32 and every element
// has one writer: no atomics, the same bits every run and under any launch geometry.
#include "common.hpp"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// out[1 + i g_out + j, :] = sum_a wy[i,a] (sum_b wx[j,b] pos[1 + a g_in + b, :]);  out[0, :] = pos[0, :]
__global__ __launch_bounds__(64) void pos_resample_fwd_kernel(const float* __restrict__ pos, int g_in,
                                                              const float* __restrict__ wy, const float* __restrict__ wx,
                                                              float* __restrict__ out, int g_out, int D) {
    const int r = blockIdx.x;                                  // output row, < g_out^2 + 1
    const int c = (blockIdx.y * 64 + threadIdx.x) * 4;
    if (c >= D) return;
    if (r == 0) {
        st4(out + c, ld4(pos + c));
        return;
    }
    const int i = (r - 1) / g_out, j = (r - 1) % g_out;
    const float* wyi = wy + (long)i * g_in;
    const float* wxj = wx + (long)j * g_in;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < g_in; ++a) {
        const float wa = wyi[a];
        if (wa == 0.f) continue;
        const float* src = pos + (1 + (long)a * g_in) * D + c;
        f32x4 inner = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < g_in; ++b) {
            const float wb = wxj[b];
            if (wb == 0.f) continue;
            inner += wb * ld4(src + (long)b * D);
        }
        acc += wa * inner;
    }
    st4(out + (long)r * D + c, acc);
}

// dpos[1 + a g_in + b, :] (+)= sum_i wy[i,a] (sum_j wx[j,b] dout[1 + i g_out + j, :]);  dpos[0, :] (+)= dout[0, :]
__global__ __launch_bounds__(64) void pos_resample_bwd_kernel(const float* __restrict__ dout, int g_out,
                                                              const float* __restrict__ wy, const float* __restrict__ wx,
                                                              float* __restrict__ dpos, int g_in, int D, int accumulate) {
    const int r = blockIdx.x;                                  // parameter row, < g_in^2 + 1
    const int c = (blockIdx.y * 64 + threadIdx.x) * 4;
    if (c >= D) return;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (r == 0) {
        acc = ld4(dout + c);
    } else {
        const int a = (r - 1) / g_in, b = (r - 1) % g_in;
        for (int i = 0; i < g_out; ++i) {
            const float wa = wy[(long)i * g_in + a];
            if (wa == 0.f) continue;
            const float* src = dout + (1 + (long)i * g_out) * D + c;
            f32x4 inner = {0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < g_out; ++j) {
                const float wb = wx[(long)j * g_in + b];
                if (wb == 0.f) continue;
                inner += wb * ld4(src + (long)j * D);
            }
            acc += wa * inner;
        }
    }
    float* dst = dpos + (long)r * D + c;
    st4(dst, accumulate ? ld4(dst) + acc : acc);
}

// ---- the text tower's positional table at another context length ----
// A run row is one or two scaled native rows: out[j, :] = w[j][0] pos[i0[j], :] + w[j][1] pos[min(i0[j] + 1, t_in - 1), :], the second
// term skipped when its weight is zero (a unit row is a copy, bit for bit).  The weights are the host's fp64 values and the two
// products and their sum are formed in fp64, rounded to fp32 once: the table is the fp32 rounding of the host's W @ pos, which is
// what a checkpoint resized on the host (posembed.resize_text_state_dict) carries.  Same geometry as above: one 64-lane workgroup
// per row and 256 columns, the row's table entries wave-uniform.  Every index read from a table is clamped into its buffer.
__global__ __launch_bounds__(64) void pos_stretch_fwd_kernel(const float* __restrict__ pos, int t_in, const int* __restrict__ i0,
                                                             const double* __restrict__ w, float* __restrict__ out, int D) {
#pragma clang fp contract(off)      // two rounded products and their rounded sum, never a fused multiply-add: the host's arithmetic
    const int j = blockIdx.x;                                  // run row, < t_out
    const int c = (blockIdx.y * 64 + threadIdx.x) * 4;
    if (c >= D) return;
    const int a = min(max(i0[j], 0), t_in - 1), b = min(a + 1, t_in - 1);
    const double wa = w[2 * j], wb = w[2 * j + 1];
    const f32x4 pa = ld4(pos + (long)a * D + c);
    f32x4 r;
    if (wb == 0.0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (float)(wa * (double)pa[e]);
    } else {
        const f32x4 pb = ld4(pos + (long)b * D + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (float)(wa * (double)pa[e] + wb * (double)pb[e]);
    }
    st4(out + (long)j * D + c, r);
}

// The transpose in gather form: native row i adds, in ascending order, the run rows span[i][0] .. span[i][1] - 1 -- the contiguous
// range whose i0 is i - 1 or i (i0 ascends with the row) -- each with the weight it gave row i, in fp64, rounded to fp32 once (with
// `accumulate`, after the old value has been added).  One writer per element, no atomics.
__global__ __launch_bounds__(64) void pos_stretch_bwd_kernel(const float* __restrict__ dout, int t_out, const int* __restrict__ i0,
                                                             const double* __restrict__ w, const int* __restrict__ span,
                                                             float* __restrict__ dpos, int t_in, int D, int accumulate) {
    const int i = blockIdx.x;                                  // native row, < t_in
    const int c = (blockIdx.y * 64 + threadIdx.x) * 4;
    if (c >= D) return;
    const int lo = max(span[2 * i], 0), hi = min(span[2 * i + 1], t_out);
    float* dst = dpos + (long)i * D + c;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (accumulate) {
        const f32x4 old = ld4(dst);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = (double)old[e];
    }
    for (int j = lo; j < hi; ++j) {
        const int a = min(max(i0[j], 0), t_in - 1);
        double wt = 0.0;                                       // what run row j gave native row i (forward: rows a and min(a + 1, t_in - 1))
        if (a == i) wt += w[2 * j];
        if (min(a + 1, t_in - 1) == i) wt += w[2 * j + 1];
        if (wt == 0.0) continue;
        const f32x4 d = ld4(dout + (long)j * D + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += wt * (double)d[e];
    }
    st4(dst, f32x4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]});
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_stretch(const char* who, const void* x, const void* i0, const void* w, const void* y, int t_in, int t_out, int D) {
    CE_CHECK_ARG(x && i0 && w && y, "%s: null buffer", who);
    CE_CHECK_ARG(t_in >= 1 && t_in <= 1024 && t_out >= 1 && t_out <= 1024, "%s: lengths must lie in 1..1024 (got %d -> %d)", who, t_in, t_out);
    CE_CHECK_ARG(D > 0 && D % 4 == 0, "%s: D must be a positive multiple of 4 (got %d)", who, D);
    CE_CHECK_ARG(aligned16(x) && aligned16(y), "%s: the tables must be 16-byte aligned", who);
    return 0;
}

int check_args(const char* who, const void* x, const void* wy, const void* wx, const void* y, int g_in, int g_out, int D) {
    CE_CHECK_ARG(x && wy && wx && y, "%s: null buffer", who);
    CE_CHECK_ARG(g_in >= 1 && g_in <= 63 && g_out >= 1 && g_out <= 63, "%s: grids must lie in 1..63 (got %d -> %d)", who, g_in, g_out);
    CE_CHECK_ARG(D > 0 && D % 4 == 0, "%s: D must be a positive multiple of 4 (got %d)", who, D);
    CE_CHECK_ARG(aligned16(x) && aligned16(y), "%s: the tables must be 16-byte aligned", who);
    return 0;
}

}  // namespace

extern "C" int ce_pos_resample_fwd(const float* pos, int g_in, const float* wy, const float* wx, float* out, int g_out, int D,
                                   void* stream) {
    if (int rc = check_args("ce_pos_resample_fwd", pos, wy, wx, out, g_in, g_out, D)) return rc;
    hipLaunchKernelGGL(pos_resample_fwd_kernel, dim3(g_out * g_out + 1, (D / 4 + 63) / 64), dim3(64), 0, (hipStream_t)stream, pos,
                       g_in, wy, wx, out, g_out, D);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_pos_resample_bwd(const float* dout, int g_out, const float* wy, const float* wx, float* dpos, int g_in, int D,
                                   int accumulate, void* stream) {
    if (int rc = check_args("ce_pos_resample_bwd", dout, wy, wx, dpos, g_in, g_out, D)) return rc;
    CE_CHECK_ARG(accumulate == 0 || accumulate == 1, "ce_pos_resample_bwd: accumulate must be 0 or 1 (got %d)", accumulate);
    hipLaunchKernelGGL(pos_resample_bwd_kernel, dim3(g_in * g_in + 1, (D / 4 + 63) / 64), dim3(64), 0, (hipStream_t)stream, dout,
                       g_out, wy, wx, dpos, g_in, D, accumulate);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_pos_stretch_fwd(const float* pos, int t_in, const int* i0, const double* w, float* out, int t_out, int D,
                                  void* stream) {
    if (int rc = check_stretch("ce_pos_stretch_fwd", pos, i0, w, out, t_in, t_out, D)) return rc;
    hipLaunchKernelGGL(pos_stretch_fwd_kernel, dim3(t_out, (D / 4 + 63) / 64), dim3(64), 0, (hipStream_t)stream, pos, t_in, i0, w,
                       out, D);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_pos_stretch_bwd(const float* dout, int t_out, const int* i0, const double* w, const int* span, float* dpos,
                                  int t_in, int D, int accumulate, void* stream) {
    if (int rc = check_stretch("ce_pos_stretch_bwd", dout, i0, w, dpos, t_in, t_out, D)) return rc;
    CE_CHECK_ARG(span, "ce_pos_stretch_bwd: null buffer");
    CE_CHECK_ARG(accumulate == 0 || accumulate == 1, "ce_pos_stretch_bwd: accumulate must be 0 or 1 (got %d)", accumulate);
    hipLaunchKernelGGL(pos_stretch_bwd_kernel, dim3(t_in, (D / 4 + 63) / 64), dim3(64), 0, (hipStream_t)stream, dout, t_out, i0, w,
                       span, dpos, t_in, D, accumulate);
    CE_LAUNCH_CHECK();
    return 0;
}
