// On-device image preprocessing: the reference's
//   Compose([Resize(n, BICUBIC), CenterCrop(n), convert("RGB"), ToTensor(), Normalize(mean, std)])   clip.py:62-69
// and the object-patch variant (image.crop(bbox) first, dataset_voa.py:222-233), for a batch of uint8 HWC images of
// different sizes, bit for bit: the resampling is Pillow's (Resample.c): separable, horizontal pass first, 8-bit
// intermediate, taps computed in double, normalised, rounded to 22-bit fixed point.  HBM-bound byte work:
//   coeff kernel : one thread per (output, axis, index) -> taps + bounds of the n cropped columns / rows
//   pass 1       : thread per (output, needed source row, column, channel) -> uint8 [rows][n][3]
//   pass 2       : thread per (output, row, column) -> vertical taps, /255, (x - mean) / std -> fp32 [3][n][n]
#include "common.hpp"
#include "../../include/clip_event_hip.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

// Resample.c bicubic_filter, a = -0.5.  No FMA contraction: the taps must round like Pillow's (plain x86-64 doubles).
__device__ double bicubic(double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * -0.5;
    return 0.0;
}

// taps[o][axis][i][k], bounds[o][axis][i] = {first source index, tap count} for cropped output index i
__global__ void preproc_coeff_kernel(const ce_preproc_desc* __restrict__ descs, int n_out, int n_px, int kmax,
                                     int* __restrict__ taps, int* __restrict__ bounds) {
#pragma clang fp contract(off)
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= (long)n_out * 2 * n_px) return;
    const int i = (int)(idx % n_px), axis = (int)((idx / n_px) & 1), o = (int)(idx / (2L * n_px));
    const ce_preproc_desc d = descs[o];
    const int in_size = axis ? d.h : d.w, out_size = axis ? d.oh : d.ow, first = axis ? d.top : d.left;
    int* k = taps + idx * kmax;
    int* b = bounds + idx * 2;
    const int xx = first + i;
    if (in_size == out_size) {          // Pillow skips the pass: identity
        k[0] = 1 << PRECISION_BITS;
        b[0] = xx; b[1] = 1;
        return;
    }
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    if (xmax > kmax) xmax = kmax;       // host sized kmax from the largest scale: never taken
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double w = bicubic((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
    }
    b[0] = xmin; b[1] = xmax;
}

__device__ __forceinline__ unsigned char clip8(int v) {
    v >>= PRECISION_BITS;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// tmp[o][r][x][c] = horizontal resample of ROI row (row0 + r), cropped columns, r < rows
__global__ void preproc_h_kernel(const ce_preproc_desc* __restrict__ descs, int n_px, int kmax,
                                 const int* __restrict__ taps, const int* __restrict__ bounds,
                                 unsigned char* __restrict__ tmp) {
    const int o = blockIdx.y;
    const ce_preproc_desc d = descs[o];
    const long total = (long)d.rows * n_px * 3;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % 3), x = (int)((idx / 3) % n_px), r = (int)(idx / (3L * n_px));
        const long t = ((long)o * 2 + 0) * n_px + x;
        const int x0 = bounds[t * 2], cnt = bounds[t * 2 + 1];
        const int* k = taps + t * kmax;
        const unsigned char* src = d.src + (long)(d.y0 + d.row0 + r) * d.pitch + (long)(d.x0 + x0) * 3 + c;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int j = 0; j < cnt; ++j) acc += (int)src[j * 3] * k[j];
        tmp[d.tmp_off + idx] = clip8(acc);
    }
}

__global__ void preproc_v_kernel(const ce_preproc_desc* __restrict__ descs, int n_px, int kmax,
                                 const int* __restrict__ taps, const int* __restrict__ bounds,
                                 const unsigned char* __restrict__ tmp, float* __restrict__ out, float m0, float m1,
                                 float m2, float s0, float s1, float s2) {
    const int o = blockIdx.y;
    const ce_preproc_desc d = descs[o];
    const long total = (long)n_px * n_px;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % n_px), y = (int)(idx / n_px);
        const long t = ((long)o * 2 + 1) * n_px + y;
        const int y0 = bounds[t * 2], cnt = bounds[t * 2 + 1];
        const int* k = taps + t * kmax;
        const unsigned char* src = tmp + d.tmp_off + ((long)(y0 - d.row0) * n_px + x) * 3;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < cnt; ++j) {
            const unsigned char* p = src + (long)j * n_px * 3;
            a0 += (int)p[0] * k[j];
            a1 += (int)p[1] * k[j];
            a2 += (int)p[2] * k[j];
        }
        // ToTensor (/255) and Normalize ((x - mean) / std), both correctly rounded fp32 like torch's div / sub / div
        float* dst = out + (long)o * 3 * total + idx;
        dst[0] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(a0), 255.0f), m0), s0);
        dst[total] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(a1), 255.0f), m1), s1);
        dst[2 * total] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)clip8(a2), 255.0f), m2), s2);
    }
}

}  // namespace

extern "C" size_t ce_preprocess_table_bytes(int n_out, int n_px, int kmax) {
    if (n_out <= 0 || n_px <= 0 || kmax <= 0) return 0;
    return ((size_t)n_out * 2 * n_px * kmax + (size_t)n_out * 2 * n_px * 2) * sizeof(int);
}

extern "C" int ce_preprocess(const ce_preproc_desc* descs_device, int n_out, int n_px, int kmax, int max_rows,
                             void* table, void* tmp, float* out, const float* mean, const float* std, void* stream) {
    CE_CHECK_ARG(descs_device && table && tmp && out && mean && std, "ce_preprocess: null buffer");
    CE_CHECK_ARG(n_out > 0 && n_px > 0 && kmax > 0 && kmax <= 4096 && max_rows > 0, "ce_preprocess: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    int* taps = reinterpret_cast<int*>(table);
    int* bounds = taps + (size_t)n_out * 2 * n_px * kmax;
    const long nc = (long)n_out * 2 * n_px;
    hipLaunchKernelGGL(preproc_coeff_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, descs_device, n_out, n_px,
                       kmax, taps, bounds);
    long bx = ((long)max_rows * n_px * 3 + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(preproc_h_kernel, dim3((unsigned)bx, n_out), dim3(256), 0, s, descs_device, n_px, kmax, taps, bounds,
                       reinterpret_cast<unsigned char*>(tmp));
    long bv = ((long)n_px * n_px + 255) / 256;
    hipLaunchKernelGGL(preproc_v_kernel, dim3((unsigned)bv, n_out), dim3(256), 0, s, descs_device, n_px, kmax, taps, bounds,
                       reinterpret_cast<const unsigned char*>(tmp), out, mean[0], mean[1], mean[2], std[0], std[1], std[2]);
    CE_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Training augmentation: RandomResizedCrop, horizontal flip, ColorJitter, RandomGrayscale, bit for bit with
// torchvision's PIL path.  The crop is the descriptor's region with ow = oh = n, so the coefficient kernel and pass 1 above
// are launched as they are; then
//   pass 2a : thread per (output, row, column) -> vertical taps -> uint8 [n][n][3]; zeroes the output's luma sum
//   luma sum: only the outputs whose list has contrast: the ops before it, L, workgroup reduction, one integer atomic
//   apply   : thread per (output, row, column) -> op list, greyscale, /255, (x - mean) / std -> fp32 [3][n][n], flipped store
// Pillow's arithmetic (Blend.c, Convert.c) is float32 / double on plain x86-64: no FMA contraction anywhere below.
namespace {

constexpr int AUG_BLOCK = 256;

struct rgb8 { int r, g, b; };

__device__ __forceinline__ int aug_luma(rgb8 p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 0x8000) >> 16; }

// Blend.c: (UINT8)(deg + f * (px - deg)) for 0 <= f <= 1 (t stays in [0, 255]: the clip below is then the truncation)
__device__ __forceinline__ int aug_blend(int deg, int px, float f) {
#pragma clang fp contract(off)
    const float t = (float)deg + f * (float)(px - deg);
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int aug_clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int aug_round(float x) { return aug_clip255((int)floor((double)x + 0.5)); }

// Convert.c rgb2hsv_row, H += shift (mod 256), hsv2rgb
__device__ rgb8 aug_hue(rgb8 p, int shift) {
#pragma clang fp contract(off)
    const int maxc = max(p.r, max(p.g, p.b)), minc = min(p.r, min(p.g, p.b));
    int H = 0, S = 0;
    const int V = maxc;
    if (maxc != minc) {
        const float cr = (float)(maxc - minc);
        const float s = __fdiv_rn(cr, (float)maxc);
        const float rc = __fdiv_rn((float)(maxc - p.r), cr), gc = __fdiv_rn((float)(maxc - p.g), cr), bc = __fdiv_rn((float)(maxc - p.b), cr);
        float h;
        if (p.r == maxc) h = bc - gc;
        else if (p.g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double turn = (double)h / 6.0 + 1.0;       // in [5/6, 11/6]: fmod(turn, 1.0) is turn - floor(turn), exactly
        h = (float)(turn - floor(turn));
        H = aug_clip255((int)((double)h * 255.0));
        S = aug_clip255((int)((double)s * 255.0));
    }
    H = (H + shift) & 255;
    if (S == 0) return rgb8{V, V, V};
    const float fh = __fdiv_rn((float)H * 6.0f, 255.0f);
    const float fi = floorf(fh);
    const float f = fh - fi;
    const float fs = __fdiv_rn((float)S, 255.0f);
    const float v = (float)V;
    const int pp = aug_round(v * (1.0f - fs));
    const int q = aug_round(v * (1.0f - fs * f));
    const int t = aug_round(v * (1.0f - fs * (1.0f - f)));
    switch ((int)fi % 6) {
        case 0: return rgb8{V, t, pp};
        case 1: return rgb8{q, V, pp};
        case 2: return rgb8{pp, V, t};
        case 3: return rgb8{pp, q, V};
        case 4: return rgb8{t, pp, V};
        default: return rgb8{V, pp, q};
    }
}

// ops [first, last) of the list; `mean` = the contrast op's degenerate grey (unused when the range holds no contrast)
__device__ rgb8 aug_ops(rgb8 p, const ce_augment_desc& a, int first, int last, int mean) {
    for (int i = first; i < last; ++i) {
        const float f = a.factor[i];
        switch (a.op[i]) {
            case 0: p = rgb8{aug_blend(0, p.r, f), aug_blend(0, p.g, f), aug_blend(0, p.b, f)}; break;
            case 1: p = rgb8{aug_blend(mean, p.r, f), aug_blend(mean, p.g, f), aug_blend(mean, p.b, f)}; break;
            case 2: {
                const int L = aug_luma(p);
                p = rgb8{aug_blend(L, p.r, f), aug_blend(L, p.g, f), aug_blend(L, p.b, f)};
                break;
            }
            default: p = aug_hue(p, (int)f); break;
        }
    }
    return p;
}

__device__ __forceinline__ int aug_n_ops(const ce_augment_desc& a) { return a.n_ops < 0 ? 0 : (a.n_ops > 4 ? 4 : a.n_ops); }

// position of the contrast op in the list, or -1
__device__ __forceinline__ int aug_contrast_at(const ce_augment_desc& a) {
    const int n = aug_n_ops(a);
    for (int i = 0; i < n; ++i)
        if (a.op[i] == 1) return i;
    return -1;
}

// img[o][y][x][c] = vertical resample of tmp (pass 2 of ce_preprocess up to its clip8); sums[o] = 0
__global__ void augment_v_kernel(const ce_preproc_desc* __restrict__ descs, int n_px, int kmax,
                                 const int* __restrict__ taps, const int* __restrict__ bounds,
                                 const unsigned char* __restrict__ tmp, unsigned char* __restrict__ img,
                                 int* __restrict__ sums) {
    const int o = blockIdx.y;
    const ce_preproc_desc d = descs[o];
    const long total = (long)n_px * n_px;
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[o] = 0;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % n_px), y = (int)(idx / n_px);
        const long t = ((long)o * 2 + 1) * n_px + y;
        const int y0 = bounds[t * 2], cnt = bounds[t * 2 + 1];
        const int* k = taps + t * kmax;
        const unsigned char* src = tmp + d.tmp_off + ((long)(y0 - d.row0) * n_px + x) * 3;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int j = 0; j < cnt; ++j) {
            const unsigned char* p = src + (long)j * n_px * 3;
            a0 += (int)p[0] * k[j];
            a1 += (int)p[1] * k[j];
            a2 += (int)p[2] * k[j];
        }
        unsigned char* dst = img + ((long)o * total + idx) * 3;
        dst[0] = clip8(a0);
        dst[1] = clip8(a1);
        dst[2] = clip8(a2);
    }
}

// sums[o] += luma of every pixel as it stands when contrast is applied; outputs without contrast leave at once
__global__ void augment_sum_kernel(const ce_augment_desc* __restrict__ augs, int n_px,
                                   const unsigned char* __restrict__ img, int* __restrict__ sums) {
    __shared__ int part[AUG_BLOCK / CE_WAVE];
    const int o = blockIdx.y;
    const ce_augment_desc a = augs[o];
    const int at = aug_contrast_at(a);
    if (at < 0) return;                                  // uniform over the workgroup
    const long total = (long)n_px * n_px;
    int acc = 0;
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const unsigned char* s = img + ((long)o * total + idx) * 3;
        acc += aug_luma(aug_ops(rgb8{s[0], s[1], s[2]}, a, 0, at, 0));
    }
    for (int off = CE_WAVE / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, CE_WAVE);
    if ((threadIdx.x & (CE_WAVE - 1)) == 0) part[threadIdx.x / CE_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < AUG_BLOCK / CE_WAVE; ++w) s += part[w];
        atomicAdd(sums + o, s);
    }
}

__global__ void augment_apply_kernel(const ce_augment_desc* __restrict__ augs, int n_px,
                                     const unsigned char* __restrict__ img, const int* __restrict__ sums,
                                     float* __restrict__ out, float m0, float m1, float m2, float s0, float s1, float s2) {
    const int o = blockIdx.y;
    const ce_augment_desc a = augs[o];
    const long total = (long)n_px * n_px;
    const int n_ops = aug_n_ops(a);
    int mean = 0;
    if (aug_contrast_at(a) >= 0) mean = (int)((2L * sums[o] + total) / (2L * total));     // int(sum / n^2 + 0.5)
    for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % n_px), y = (int)(idx / n_px);
        const unsigned char* s = img + ((long)o * total + idx) * 3;
        rgb8 p = aug_ops(rgb8{s[0], s[1], s[2]}, a, 0, n_ops, mean);
        if (a.grey) {
            const int L = aug_luma(p);
            p = rgb8{L, L, L};
        }
        // the flip commutes with every pointwise step (and with the image-wide luma sum): done at the store
        float* dst = out + (long)o * 3 * total + (long)y * n_px + (a.flip ? n_px - 1 - x : x);
        dst[0] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p.r, 255.0f), m0), s0);
        dst[total] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p.g, 255.0f), m1), s1);
        dst[2 * total] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p.b, 255.0f), m2), s2);
    }
}

constexpr size_t AUG_ALIGN = 256;
__host__ size_t aug_up(size_t v) { return (v + AUG_ALIGN - 1) / AUG_ALIGN * AUG_ALIGN; }

}  // namespace

// workspace = [taps table | per-output luma sums | 8-bit n x n x 3 images | pass-1 scratch (tmp_bytes)]
extern "C" size_t ce_augment_workspace_bytes(int n_out, int n_px, int kmax, long tmp_bytes) {
    if (n_out <= 0 || n_px <= 0 || kmax <= 0 || tmp_bytes < 0) return 0;
    return aug_up(ce_preprocess_table_bytes(n_out, n_px, kmax)) + aug_up((size_t)n_out * sizeof(int)) +
           aug_up((size_t)n_out * n_px * n_px * 3) + aug_up((size_t)tmp_bytes);
}

extern "C" int ce_augment(const ce_preproc_desc* descs_device, const ce_augment_desc* augs_device, const ce_augment_desc* augs_host,
                          int n_out, int n_px, int kmax, int max_rows, void* workspace, float* out,
                          const float* mean, const float* std, void* stream) {
    CE_CHECK_ARG(descs_device && augs_device && augs_host && workspace && out && mean && std, "ce_augment: null buffer");
    CE_CHECK_ARG(n_out > 0 && n_px > 0 && kmax > 0 && kmax <= 4096 && max_rows > 0 && n_out <= 65535, "ce_augment: bad sizes");
    CE_CHECK_ARG(n_px <= 2896, "ce_augment: n_px %d: the per-image luma sum 255 * n_px^2 must fit in int32 (n_px <= 2896)", n_px);
    bool any_contrast = false;
    for (int o = 0; o < n_out; ++o) {
        const ce_augment_desc& a = augs_host[o];
        CE_CHECK_ARG(a.n_ops >= 0 && a.n_ops <= 4, "ce_augment: output %d has %d ops (0..4)", o, a.n_ops);
        CE_CHECK_ARG((a.flip == 0 || a.flip == 1) && (a.grey == 0 || a.grey == 1), "ce_augment: output %d: flip / grey must be 0 or 1", o);
        int contrasts = 0;
        for (int i = 0; i < a.n_ops; ++i) {
            CE_CHECK_ARG(a.op[i] >= 0 && a.op[i] <= 3, "ce_augment: output %d op %d: unknown op %d", o, i, a.op[i]);
            CE_CHECK_ARG(a.factor[i] >= 0.0f, "ce_augment: output %d op %d: negative factor", o, i);
            CE_CHECK_ARG(a.op[i] != 3 || (a.factor[i] <= 255.0f && a.factor[i] == (float)(int)a.factor[i]),
                         "ce_augment: output %d op %d: the hue shift must be an integer 0..255", o, i);
            contrasts += a.op[i] == 1;
        }
        CE_CHECK_ARG(contrasts <= 1, "ce_augment: output %d lists contrast %d times (at most once)", o, contrasts);
        any_contrast |= contrasts == 1;
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    int* taps = reinterpret_cast<int*>(ws);
    int* bounds = taps + (size_t)n_out * 2 * n_px * kmax;
    ws += aug_up(ce_preprocess_table_bytes(n_out, n_px, kmax));
    int* sums = reinterpret_cast<int*>(ws);
    ws += aug_up((size_t)n_out * sizeof(int));
    unsigned char* img = reinterpret_cast<unsigned char*>(ws);
    ws += aug_up((size_t)n_out * n_px * n_px * 3);
    unsigned char* tmp = reinterpret_cast<unsigned char*>(ws);
    const long nc = (long)n_out * 2 * n_px;
    hipLaunchKernelGGL(preproc_coeff_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, descs_device, n_out, n_px,
                       kmax, taps, bounds);
    long bx = ((long)max_rows * n_px * 3 + 255) / 256;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(preproc_h_kernel, dim3((unsigned)bx, n_out), dim3(256), 0, s, descs_device, n_px, kmax, taps, bounds, tmp);
    long bv = ((long)n_px * n_px + AUG_BLOCK - 1) / AUG_BLOCK;
    if (bv > 1024) bv = 1024;
    hipLaunchKernelGGL(augment_v_kernel, dim3((unsigned)bv, n_out), dim3(AUG_BLOCK), 0, s, descs_device, n_px, kmax, taps, bounds,
                       tmp, img, sums);
    if (any_contrast)
        hipLaunchKernelGGL(augment_sum_kernel, dim3((unsigned)bv, n_out), dim3(AUG_BLOCK), 0, s, augs_device, n_px, img, sums);
    hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)bv, n_out), dim3(AUG_BLOCK), 0, s, augs_device, n_px, img, sums, out,
                       mean[0], mean[1], mean[2], std[0], std[1], std[2]);
    CE_LAUNCH_CHECK();
    return 0;
}
