// Fused optimiser step over the flat fp32 parameter / gradient buffers (gfx950, HBM-bound).
//
// Replaces engine.py:89-90: torch.nn.utils.clip_grad_norm_(params, 1) followed by
// torch.optim.Adam(lr, weight_decay).step() (L2 weight decay, not AdamW; engine.py:141-146).
// Two launches per step instead of ~900: a sum-of-squares reduction into a device scalar,
// then one Adam pass that reads the scalar (no host sync) and applies the clip coefficient
// max_norm / (norm + 1e-6) (clamped to 1) on the fly.
#include <stdlib.h>

#include <type_traits>

#include "common.hpp"
#include "../../include/clip_event_hip.h"

// CE_ADAM_NT (compile time): cache policy of the p / m / v streams (each element is touched once per step): 0 plain,
// 1 nt stores, 2 (default) nt loads and stores -- tools/bench_hbm.py adam: 914 / 920 / 861 us (4.97 / 4.93 / 5.27 TB/s)
#ifndef CE_ADAM_NT
#define CE_ADAM_NT 2
#endif
#if CE_ADAM_NT >= 1
#define CE_ADAM_ST(val, ptr) __builtin_nontemporal_store(val, ptr)
#else
#define CE_ADAM_ST(val, ptr) (*(ptr) = (val))
#endif
#if CE_ADAM_NT >= 2
#define CE_ADAM_LD(ptr) __builtin_nontemporal_load(ptr)
#else
#define CE_ADAM_LD(ptr) (*(ptr))
#endif

namespace {

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    const long stride = gridDim.x * 1024L;
    for (long i = blockIdx.x * 1024L + threadIdx.x * 4; i < n; i += stride) {
        if (i + 3 < n) {
            f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
            s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        } else {
            for (long k = i; k < n; ++k) s += g[k] * g[k];
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, (red[0] + red[1]) + (red[2] + red[3]));
}

// out += sum g^2 over [table[2b], table[2b+1]) for chunk b (multiples of 4, at most 65536 long): sumsq_kernel's rounding chain per
// chunk, and no load outside the table (the gradient slices of frozen parameters are never read)
__global__ __launch_bounds__(256) void sumsq_segments_kernel(const float* __restrict__ g, const long* __restrict__ table,
                                                             float* __restrict__ out) {
    __shared__ float red[4];
    const long lo = table[2 * blockIdx.x], hi = table[2 * blockIdx.x + 1];
    float s = 0.f;
    for (long i = lo + threadIdx.x * 4; i < hi; i += 1024) {
        f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
        s += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, (red[0] + red[1]) + (red[2] + red[3]));
}

// One element of clip + Adam.  Every kernel of this file updates through this function, with the contraction of a * b + c into
// fused multiply-adds spelled out, so that the flat kernel, the tile kernel and the segment kernel give the same bits.
// `decay` != 0 is the decoupled form (AdamW): p is first scaled by 1 - decay (decay = lr * weight_decay, one multiply-add) and the
// caller passes wd = 0, so the gradient gets no decay term.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float coef, float wd, float b1, float b2,
                                          float lr_bc1, float bc2_sqrt, float eps, float decay) {
#pragma clang fp contract(off)
    if (decay != 0.f) p = __builtin_fmaf(p, -decay, p);
    g = g * coef;
    if (wd != 0.f) g = __builtin_fmaf(p, wd, g);
    m = __builtin_fmaf(m, b1, g * (1.0f - b1));
    v = __builtin_fmaf(v, b2, (g * g) * (1.0f - b2));
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = __builtin_fmaf(-lr_bc1, m / denom, p);
}

// One element of clip + SGD with momentum (torch.optim.SGD: engine.py:136-140 behind engine.py:89's clip).  As adam_elem:
// every kernel form updates through this function with the multiply-adds spelled out, so that the flat, the tile and the segment
// kernel give the same bits.  `first`: no momentum buffer yet -- it becomes a copy of the decayed gradient
// whatever the dampening is (torch).  mu == 0: `buf` is neither read nor written.
__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, float coef, float wd, float mu, float one_minus_damp,
                                         float lr, bool first, bool nesterov) {
#pragma clang fp contract(off)
    g = g * coef;
    if (wd != 0.f) g = __builtin_fmaf(p, wd, g);
    float upd = g;
    if (mu != 0.f) {
        buf = first ? g : __builtin_fmaf(buf, mu, g * one_minus_damp);
        upd = nesterov ? __builtin_fmaf(buf, mu, g) : buf;
    }
    p = __builtin_fmaf(-lr, upd, p);
}

// One element of clip + Lion (Chen et al. 2023): c = b1 m + (1 - b1) g is formed from the OLD momentum, the master moves by exactly
// lr against c's sign, and only then the momentum becomes b2 m + (1 - b2) g.  As adam_elem / sgd_elem: every kernel form updates
// through this function -- here every product and sum is an instruction of its own (two products and one sum for c and for m, no
// multiply-add) -- so that the flat, the tile and the segment kernel give the same bits.  `decay` = lr * weight_decay: always the
// decoupled form, p <- p - decay p in front of the step, skipped when it is 0 (p - 0 * p is not p for p = -0).  The sign is
// (c > 0) - (c < 0): 0 for c == 0, and 0 for a NaN c as well (both comparisons are false), so that a NaN gradient leaves the master
// to the decay alone and shows in the momentum, which becomes NaN.  No bias correction, no step counter: zero momentum is the start.
__device__ __forceinline__ void lion_elem(float& p, float g, float& m, float coef, float b1, float one_minus_b1, float b2,
                                          float one_minus_b2, float lr, float decay) {
#pragma clang fp contract(off)
    g = g * coef;
    const float mb1 = m * b1, gb1 = g * one_minus_b1;
    const float c = mb1 + gb1;
    const float u = (c > 0.f ? 1.0f : 0.f) - (c < 0.f ? 1.0f : 0.f);
    if (decay != 0.f) {
        const float dp = decay * p;
        p = p - dp;
    }
    const float step = lr * u;
    p = p - step;
    const float mb2 = m * b2, gb2 = g * one_minus_b2;
    m = mb2 + gb2;
}

// One element of the weight average, e <- e + rate (p_new - e) with rate = 1 - decay, in torch's lerp_ form: below a weight of 0.5
// fma(p_new - e, rate, e), from 0.5 on p_new - (p_new - e) (1 - rate), so that rate 1 gives p_new itself (the branch is uniform
// over the launch).  p_new is the fp32 master exactly as the rule just wrote it.  As adam_elem / sgd_elem: the subtraction and the
// multiply-add are spelled out, so that every traversal gives the same bits.
__device__ __forceinline__ void ema_elem(float& e, float p_new, float rate) {
#pragma clang fp contract(off)
    const float d = p_new - e;
    e = rate < 0.5f ? __builtin_fmaf(d, rate, e) : p_new - d * (1.0f - rate);
}

__device__ __forceinline__ float clip_coef(const float* __restrict__ sumsq, float max_norm) {
    return sumsq ? fminf(1.0f, max_norm / (sqrtf(*sumsq) + 1e-6f)) : 1.0f;
}

// ---- update rules ----------------------------------------------------------------------------------------------------------------
// A rule is what the three traversals below are instantiated with: NS, the number of fp32 state streams beside p and g; Args, the
// by-value kernel argument; a device constructor (args, group id) that derives the per-launch scalars (the clip coefficient among
// them); GROUPED, whether lr / weight decay come from a table of parameter groups -- the tile and the segment traversal then hand the
// constructor the group of their workgroup (block-uniform, looked up once), otherwise 0 -- and elem(p, g, state), one element.  `state` has max(NS, 1) slots, so that a rule without state still has something to pass on.
struct AdamRule {
    static constexpr int NS = 2;                   // m, v
    static constexpr bool GROUPED = false;
    struct Args {
        const float* sumsq;
        float max_norm, lr, b1, b2, eps, wd, bc1, bc2_sqrt;
    };
    float coef, wd, b1, b2, lr_bc1, bc2_sqrt, eps;
    __device__ AdamRule(const Args& a, int)
        : coef(clip_coef(a.sumsq, a.max_norm)), wd(a.wd), b1(a.b1), b2(a.b2), lr_bc1(a.lr / a.bc1), bc2_sqrt(a.bc2_sqrt), eps(a.eps) {}
    __device__ __forceinline__ void elem(float& p, float g, float (&s)[2]) const {
        adam_elem(p, g, s[0], s[1], coef, wd, b1, b2, lr_bc1, bc2_sqrt, eps, 0.f);
    }
};

// The parameter groups of a grouped launch, by value in the kernel argument; `segment_group` (device, nullable) names the group of
// every segment, a tile job names its own in ce_transpose_job.pad_.
constexpr int kMaxGroups = 8;
struct group_table {
    const int* segment_group;
    int ngroups;
    ce_optim_group g[kMaxGroups];
};
__device__ __forceinline__ ce_optim_group pick_group(const group_table& t, int id) {
    id = id < 0 || id >= t.ngroups ? t.ngroups - 1 : id;      // block-uniform; never outside the table
    return t.g[id];
}

struct AdamGroupRule {
    static constexpr int NS = 2;
    static constexpr bool GROUPED = true;
    struct Args {
        const float* sumsq;
        float max_norm, b1, b2, eps, bc1, bc2_sqrt;
        group_table groups;
    };
    float coef, wd, b1, b2, lr_bc1, bc2_sqrt, eps, decay;
    __device__ AdamGroupRule(const Args& a, int group)
        : coef(clip_coef(a.sumsq, a.max_norm)), b1(a.b1), b2(a.b2), bc2_sqrt(a.bc2_sqrt), eps(a.eps) {
        set_group(a, group);
    }
    __device__ __forceinline__ void set_group(const Args& a, int group) {
#pragma clang fp contract(off)
        const ce_optim_group gr = pick_group(a.groups, group);
        lr_bc1 = gr.lr / a.bc1;
        wd = gr.decoupled ? 0.f : gr.weight_decay;
        decay = gr.decoupled ? gr.lr * gr.weight_decay : 0.f;
    }
    __device__ __forceinline__ void elem(float& p, float g, float (&s)[2]) const {
        adam_elem(p, g, s[0], s[1], coef, wd, b1, b2, lr_bc1, bc2_sqrt, eps, decay);
    }
};

struct sgd_args {
    const float* sumsq;
    float max_norm, lr, mu, one_minus_damp, wd;
    int first, nesterov;
};
// MOM = false: momentum 0, no momentum buffer and no momentum traffic (flat form: 8 B read + 6 B written per parameter);
// MOM = true: 12 B read + 10 B written
template <bool MOM>
struct SgdRule {
    static constexpr int NS = MOM ? 1 : 0;         // the momentum buffer
    static constexpr bool GROUPED = false;
    using Args = sgd_args;
    float coef, wd, mu, one_minus_damp, lr;
    bool first, nesterov;
    __device__ SgdRule(const Args& a, int)
        : coef(clip_coef(a.sumsq, a.max_norm)), wd(a.wd), mu(MOM ? a.mu : 0.f), one_minus_damp(a.one_minus_damp), lr(a.lr),
          first(a.first != 0), nesterov(a.nesterov != 0) {}
    __device__ __forceinline__ void elem(float& p, float g, float (&s)[1]) const {
        sgd_elem(p, g, s[0], coef, wd, mu, one_minus_damp, lr, first, nesterov);
    }
};

struct sgd_group_args {
    const float* sumsq;
    float max_norm, mu, one_minus_damp;
    int first, nesterov;
    group_table groups;
};
template <bool MOM>
struct SgdGroupRule {
    static constexpr int NS = MOM ? 1 : 0;
    static constexpr bool GROUPED = true;
    using Args = sgd_group_args;
    float coef, wd, mu, one_minus_damp, lr;
    bool first, nesterov;
    __device__ SgdGroupRule(const Args& a, int group)
        : coef(clip_coef(a.sumsq, a.max_norm)), mu(MOM ? a.mu : 0.f), one_minus_damp(a.one_minus_damp), first(a.first != 0),
          nesterov(a.nesterov != 0) {
        set_group(a, group);
    }
    __device__ __forceinline__ void set_group(const Args& a, int group) {
        const ce_optim_group gr = pick_group(a.groups, group);
        lr = gr.lr;
        wd = gr.weight_decay;
    }
    __device__ __forceinline__ void elem(float& p, float g, float (&s)[1]) const {
        sgd_elem(p, g, s[0], coef, wd, mu, one_minus_damp, lr, first, nesterov);
    }
};

// Lion: one state stream, the streams of SGD with momentum (flat form: 12 B read + 10 B written per parameter).  1 - b1, 1 - b2 and
// lr * weight_decay are rounded once here, in fp32.
struct LionRule {
    static constexpr int NS = 1;                   // the momentum (exp_avg)
    static constexpr bool GROUPED = false;
    struct Args {
        const float* sumsq;
        float max_norm, lr, b1, b2, wd;
    };
    float coef, b1, one_minus_b1, b2, one_minus_b2, lr, decay;
    __device__ LionRule(const Args& a, int)
        : coef(clip_coef(a.sumsq, a.max_norm)), b1(a.b1), one_minus_b1(1.0f - a.b1), b2(a.b2), one_minus_b2(1.0f - a.b2), lr(a.lr),
          decay(a.lr * a.wd) {}
    __device__ __forceinline__ void elem(float& p, float g, float (&s)[1]) const {
        lion_elem(p, g, s[0], coef, b1, one_minus_b1, b2, one_minus_b2, lr, decay);
    }
};

// lr and weight decay per group; ce_optim_group.decoupled is not read (Lion's decay is always decoupled)
struct LionGroupRule {
    static constexpr int NS = 1;
    static constexpr bool GROUPED = true;
    struct Args {
        const float* sumsq;
        float max_norm, b1, b2;
        group_table groups;
    };
    float coef, b1, one_minus_b1, b2, one_minus_b2, lr, decay;
    __device__ LionGroupRule(const Args& a, int group)
        : coef(clip_coef(a.sumsq, a.max_norm)), b1(a.b1), one_minus_b1(1.0f - a.b1), b2(a.b2), one_minus_b2(1.0f - a.b2) {
        set_group(a, group);
    }
    __device__ __forceinline__ void set_group(const Args& a, int group) {
        const ce_optim_group gr = pick_group(a.groups, group);
        lr = gr.lr;
        decay = gr.lr * gr.weight_decay;
    }
    __device__ __forceinline__ void elem(float& p, float g, float (&s)[1]) const {
        lion_elem(p, g, s[0], coef, b1, one_minus_b1, b2, one_minus_b2, lr, decay);
    }
};

template <class Rule>
constexpr int kSlots = Rule::NS > 0 ? Rule::NS : 1;

// the four lanes of a 16-byte chunk through Rule::elem
template <class Rule>
__device__ __forceinline__ void elem4(const Rule& rule, f32x4& p, f32x4 g, f32x4 (&s)[kSlots<Rule>]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], se[kSlots<Rule>];
#pragma unroll
        for (int k = 0; k < kSlots<Rule>; ++k) se[k] = s[k][e];
        rule.elem(pe, g[e], se);
        p[e] = pe;
#pragma unroll
        for (int k = 0; k < kSlots<Rule>; ++k) s[k][e] = se[k];
    }
}

// the four lanes of a 16-byte chunk of the average through ema_elem
__device__ __forceinline__ void ema4(f32x4& e, const f32x4& p_new, float rate) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float ek = e[k];
        ema_elem(ek, p_new[k], rate);
        e[k] = ek;
    }
}

// ---- the traversals --------------------------------------------------------------------------------------------------------------
// Each is one kernel template over the rule.  The state streams are the kernel parameters s0, s1 (NULL beyond Rule::NS; parameters
// rather than an array so that they keep __restrict__) and are named only under `k < Rule::NS`: a rule with NS == 0 issues no
// state traffic at all.  Cache policy: p and the state through CE_ADAM_LD / CE_ADAM_ST, g always nontemporal.
// EMA (compile time): the traversal also carries the weight average `ema` -- one more stream, requested with the others, updated
// from the new master in registers (ema_elem) and stored like the state.  Without it `ema` / `ema_rate` are never named.

// the request for one 16-byte chunk of every stream at element offset `at`: p, g, then the state streams, then the average
template <class Rule, bool EMA>
__device__ __forceinline__ void load_chunk(float* p, const float* g, float* const (&st)[2], float* ema, long at, f32x4& pv, f32x4& gv,
                                           f32x4 (&sv)[kSlots<Rule>], f32x4& ev) {
    pv = CE_ADAM_LD(reinterpret_cast<f32x4*>(p + at));
    gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + at));
#pragma unroll
    for (int k = 0; k < Rule::NS; ++k) sv[k] = CE_ADAM_LD(reinterpret_cast<f32x4*>(st[k] + at));
    if constexpr (EMA) ev = CE_ADAM_LD(reinterpret_cast<f32x4*>(ema + at));
}
// the average of one chunk from its new masters, and its store
template <bool EMA>
__device__ __forceinline__ void update_ema(float* ema, long at, f32x4& ev, const f32x4& p_new, float rate) {
    if constexpr (EMA) {
        ema4(ev, p_new, rate);
        CE_ADAM_ST(ev, reinterpret_cast<f32x4*>(ema + at));
    }
}
template <class Rule>
__device__ __forceinline__ void store_state(float* const (&st)[2], long at, const f32x4 (&sv)[kSlots<Rule>]) {
#pragma unroll
    for (int k = 0; k < Rule::NS; ++k) CE_ADAM_ST(sv[k], reinterpret_cast<f32x4*>(st[k] + at));
}
__device__ __forceinline__ u32x2 pack_bf4(const f32x4& v) { return u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])}; }

// Flat: grid-stride over [0, n).  Two 16-byte chunks per lane and iteration, every load issued before the first use: the pass is
// pure streaming (Adam: 16 B read + 14 B written per parameter) and wants as many bytes in flight as the registers allow.
template <class Rule, bool EMA>
__global__ __launch_bounds__(256) void optim_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                         float* __restrict__ s1, bf16_t* __restrict__ p16, long n,
                                                         typename Rule::Args a, float* __restrict__ ema, float ema_rate) {
    const Rule rule(a, 0);
    float* const st[2] = {s0, s1};
    const long stride = gridDim.x * 2048L;
    for (long i0 = blockIdx.x * 2048L + threadIdx.x * 4; i0 < n; i0 += stride) {
        const long i1 = i0 + 1024;
        if (i1 + 3 < n) {
            f32x4 pv[2], gv[2], sv[2][kSlots<Rule>] = {}, ev[2] = {};
#pragma unroll
            for (int u = 0; u < 2; ++u) load_chunk<Rule, EMA>(p, g, st, ema, u ? i1 : i0, pv[u], gv[u], sv[u], ev[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const long i = u ? i1 : i0;
                elem4(rule, pv[u], gv[u], sv[u]);
                CE_ADAM_ST(pv[u], reinterpret_cast<f32x4*>(p + i));
                if (p16) *reinterpret_cast<u32x2*>(p16 + i) = pack_bf4(pv[u]);
                store_state<Rule>(st, i, sv[u]);
                update_ema<EMA>(ema, i, ev[u], pv[u], ema_rate);
            }
        } else {
            for (int u = 0; u < 2; ++u) {
                const long ib = u ? i1 : i0;
                for (long k = ib; k < n && k < ib + 4; ++k) {
                    float pk = p[k], sk[kSlots<Rule>] = {};
#pragma unroll
                    for (int q = 0; q < Rule::NS; ++q) sk[q] = st[q][k];
                    rule.elem(pk, g[k], sk);
                    p[k] = pk;
#pragma unroll
                    for (int q = 0; q < Rule::NS; ++q) st[q][k] = sk[q];
                    if (p16) p16[k] = f2bf(pk);
                    if constexpr (EMA) {
                        float ek = ema[k];
                        ema_elem(ek, pk, ema_rate);
                        ema[k] = ek;
                    }
                }
            }
        }
    }
}

// base[table[2b] .. table[2b+1]) = 0 for chunk b (element offsets, multiples of 4): the step's gradient zero-fill minus the
// tensors whose first gradient contribution is a store (ce_gemm_tn_grouped_ex overwrite)
__global__ __launch_bounds__(256) void zero_segments_kernel(float* __restrict__ base, const long* __restrict__ table) {
    const long lo = table[2 * blockIdx.x], hi = table[2 * blockIdx.x + 1];
    for (long i = lo + threadIdx.x * 4; i < hi; i += 1024)
        __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(base + i));
}

// ---- 64 x 64 tiles of a table of bf16 matrices -----------------------------------------------------------------------------------
// The tile a workgroup owns: its job and the tile's first row and column.
struct tile_at {
    ce_transpose_job job;
    int r0, c0;
};
__device__ __forceinline__ tile_at find_tile(const ce_transpose_job* __restrict__ jobs, int njobs) {
    int j = 0;
    const int b = blockIdx.x;
    while (j + 1 < njobs && b >= jobs[j + 1].tile_start) ++j;      // block-uniform
    const ce_transpose_job job = jobs[j];
    const int t = b - job.tile_start;
    const int tiles_c = (job.cols + 63) / 64;
    return {job, (t / tiles_c) * 64, (t % tiles_c) * 64};
}

// The LDS tile ([source row][source column]; row stride 66 elements = 33 dwords: the 8 rows a lane gathers for one 16-byte
// transposed store sit in 8 different banks) written to job.dst ([cols][rows]), 16 bytes per lane.  rows, cols multiples of 8.
template <bool NT>
__device__ __forceinline__ void store_tile_transposed(const bf16_t (&tile)[64][66], const tile_at& t) {
    bf16_t* dst = reinterpret_cast<bf16_t*>(t.job.dst);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = threadIdx.x + k * 256;                 // 64 output rows (source columns) x 8 chunks of 8 source rows
        const int c = idx >> 3, ch = idx & 7;
        if (t.c0 + c < t.job.cols && t.r0 + ch * 8 < t.job.rows) {
            uint32_t w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                w[e] = (uint32_t)tile[ch * 8 + 2 * e][c] | ((uint32_t)tile[ch * 8 + 2 * e + 1][c] << 16);
            const u32x4 v = {w[0], w[1], w[2], w[3]};
            u32x4* out = reinterpret_cast<u32x4*>(dst + (long)(t.c0 + c) * t.job.rows + t.r0 + ch * 8);
            if (NT) __builtin_nontemporal_store(v, out);
            else *out = v;
        }
    }
}

// dst[c][r] = src[r][c] for a table of bf16 matrices, one launch: the transposed operand copies of every
// weight (input-gradient GEMMs read W^T) are rebuilt from the bf16 mirror the optimiser kernels wrote.
__global__ __launch_bounds__(256) void multi_transpose_kernel(const ce_transpose_job* __restrict__ jobs, int njobs) {
    // 64 x 64 tile through LDS; global accesses are 16 bytes per lane on both sides when rows/cols are multiples
    // of 8 (every weight here), 2 bytes per lane otherwise.
    __shared__ bf16_t tile[64][66];
    const tile_at t = find_tile(jobs, njobs);
    const ce_transpose_job& job = t.job;
    const int r0 = t.r0, c0 = t.c0;
    const bf16_t* src = reinterpret_cast<const bf16_t*>(job.src);
    bf16_t* dst = reinterpret_cast<bf16_t*>(job.dst);
    const bool wide = (job.rows % 8 == 0) && (job.cols % 8 == 0) &&
                      ((reinterpret_cast<size_t>(src) | reinterpret_cast<size_t>(dst)) % 16 == 0);
    if (wide) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int idx = threadIdx.x + k * 256;                 // 64 rows x 8 chunks
            const int r = idx >> 3, ch = idx & 7;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (r0 + r < job.rows && c0 + ch * 8 < job.cols)
                v = *reinterpret_cast<const u32x4*>(src + (long)(r0 + r) * job.cols + c0 + ch * 8);
            uint32_t* trow = reinterpret_cast<uint32_t*>(&tile[r][ch * 8]);
            trow[0] = v[0]; trow[1] = v[1]; trow[2] = v[2]; trow[3] = v[3];
        }
        __syncthreads();
        store_tile_transposed<false>(tile, t);
        return;
    }
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;        // 64 x 4
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int r = r0 + ty + 4 * k, c = c0 + tx;
        tile[ty + 4 * k][tx] = (r < job.rows && c < job.cols) ? src[(long)r * job.cols + c] : (bf16_t)0;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int c = c0 + ty + 4 * k, r = r0 + tx;
        if (r < job.rows && c < job.cols) dst[(long)c * job.rows + r] = tile[tx][ty + 4 * k];
    }
}

// Tiles: the update over a table of bf16-mirrored MATRICES, one 64 x 64 tile per workgroup: the flat kernel's update element for
// element, and with it BOTH operand copies of the new weights -- the row-major bf16 mirror and, through an LDS transpose of the
// tile, the W^T copy the input-gradient GEMMs read (`job.dst`, [cols][rows]) -- so that no separate transpose pass re-reads the
// mirror (`multi_transpose_kernel`: 0.17 GB read + a launch beside the next forward's first kernels).  `job.src` points into the
// flat mirror `p16`: its offset there is the matrix's offset in every flat buffer.  rows, cols multiples of 8.
template <class Rule, bool EMA>
__global__ __launch_bounds__(256) void optim_tiles_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                          float* __restrict__ s1, bf16_t* __restrict__ p16,
                                                          const ce_transpose_job* __restrict__ jobs, int njobs, typename Rule::Args a,
                                                          float* __restrict__ ema, float ema_rate) {
    __shared__ bf16_t tile[64][66];
    Rule rule(a, 0);
    float* const st[2] = {s0, s1};
    const tile_at t = find_tile(jobs, njobs);
    if constexpr (Rule::GROUPED) rule.set_group(a, t.job.pad_);
    const long off = reinterpret_cast<const bf16_t*>(t.job.src) - p16;
    // 64 rows x 16 four-element chunks; all loads of a thread (Adam: sixteen, with the average twenty) in flight before the first use
    f32x4 pv[4] = {}, gv[4] = {}, sv[4][kSlots<Rule>] = {}, ev[4] = {};
    bool ok[4];
    long at[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = threadIdx.x + k * 256;
        const int r = idx >> 4, ch = idx & 15;
        ok[k] = t.r0 + r < t.job.rows && t.c0 + ch * 4 < t.job.cols;
        at[k] = off + (long)(t.r0 + r) * t.job.cols + t.c0 + ch * 4;
        if (ok[k]) load_chunk<Rule, EMA>(p, g, st, ema, at[k], pv[k], gv[k], sv[k], ev[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = threadIdx.x + k * 256;
        const int r = idx >> 4, ch = idx & 15;
        elem4(rule, pv[k], gv[k], sv[k]);
        const u32x2 pk = pack_bf4(pv[k]);
        uint32_t* trow = reinterpret_cast<uint32_t*>(&tile[r][ch * 4]);
        trow[0] = pk[0]; trow[1] = pk[1];
        if (ok[k]) {
            CE_ADAM_ST(pv[k], reinterpret_cast<f32x4*>(p + at[k]));
            __builtin_nontemporal_store(pk, reinterpret_cast<u32x2*>(p16 + at[k]));       // (nt on the mirror and on W^T: 1034 -> 986 us for
                                                                                          //  the ViT-B/32 Adam step in a loop of its own)
            store_state<Rule>(st, at[k], sv[k]);
            update_ema<EMA>(ema, at[k], ev[k], pv[k], ema_rate);
        }
    }
    __syncthreads();
    store_tile_transposed<true>(tile, t);
}

// Segments: the same update over a table of [lo, hi) chunks of the flat buffers (everything that is not one of the matrices
// above): one workgroup per chunk of at most 2048 elements, both 16-byte pieces of a thread requested before the first use
template <class Rule, bool EMA>
__global__ __launch_bounds__(256) void optim_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                             float* __restrict__ s1, bf16_t* __restrict__ p16,
                                                             const long* __restrict__ table, typename Rule::Args a,
                                                             float* __restrict__ ema, float ema_rate) {
    int group = 0;
    if constexpr (Rule::GROUPED) group = a.groups.segment_group ? a.groups.segment_group[blockIdx.x] : 0;
    const Rule rule(a, group);
    float* const st[2] = {s0, s1};
    const long lo = table[2 * blockIdx.x], hi = table[2 * blockIdx.x + 1];
    f32x4 pv[2] = {}, gv[2] = {}, sv[2][kSlots<Rule>] = {}, ev[2] = {};
    long at[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        at[u] = lo + threadIdx.x * 4 + u * 1024;
        ok[u] = at[u] + 3 < hi;
        if (ok[u]) load_chunk<Rule, EMA>(p, g, st, ema, at[u], pv[u], gv[u], sv[u], ev[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (!ok[u]) continue;
        elem4(rule, pv[u], gv[u], sv[u]);
        CE_ADAM_ST(pv[u], reinterpret_cast<f32x4*>(p + at[u]));
        if (p16) *reinterpret_cast<u32x2*>(p16 + at[u]) = pack_bf4(pv[u]);
        store_state<Rule>(st, at[u], sv[u]);
        update_ema<EMA>(ema, at[u], ev[u], pv[u], ema_rate);
    }
}

// a <-> b element for element, and a16 = the bf16 mirror (f2bf, as ce_cast_bf16) of what lands in a: the swap between the masters
// and their average in one pass (16 B read + 18 B written per element), 16-byte chunks and a scalar tail
__global__ __launch_bounds__(256) void swap_cast_kernel(float* __restrict__ a, float* __restrict__ b, bf16_t* __restrict__ a16, long n) {
    const long stride = gridDim.x * 1024L;
    for (long i = blockIdx.x * 1024L + threadIdx.x * 4; i < n; i += stride) {
        if (i + 3 < n) {
            const f32x4 av = CE_ADAM_LD(reinterpret_cast<f32x4*>(a + i));
            const f32x4 bv = CE_ADAM_LD(reinterpret_cast<f32x4*>(b + i));
            CE_ADAM_ST(bv, reinterpret_cast<f32x4*>(a + i));
            CE_ADAM_ST(av, reinterpret_cast<f32x4*>(b + i));
            *reinterpret_cast<u32x2*>(a16 + i) = pack_bf4(bv);
        } else {
            for (long k = i; k < n; ++k) {
                const float ak = a[k], bk = b[k];
                a[k] = bk;
                b[k] = ak;
                a16[k] = f2bf(bk);
            }
        }
    }
}

// torch.optim.SGD's argument rules (plus: a momentum buffer must exist when momentum is used); 0 or -EINVAL with a message
int sgd_check(const char* who, const float* buf, float momentum, float dampening, int nesterov) {
    CE_CHECK_ARG(momentum >= 0.f, "%s: invalid momentum value %g", who, (double)momentum);
    CE_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f), "%s: nesterov momentum requires a momentum and zero dampening", who);
    CE_CHECK_ARG(momentum == 0.f || buf, "%s: momentum %g needs a momentum buffer", who, (double)momentum);
    return 0;
}

// Bias corrections in double, rounded once to fp32 -- as torch.optim.Adam takes them (Python floats).  In fp32, 1 - powf(beta2,
// step) cancels: at step 2 (1 - 0.998) the rounding of powf is up to 1.5e-5 of the result, and the update inherits it.
float adam_bc1(float beta1, int step) { return (float)(1.0 - pow((double)beta1, (double)step)); }
float adam_bc2_sqrt(float beta2, int step) { return (float)sqrt(1.0 - pow((double)beta2, (double)step)); }

// the by-value group table of a grouped launch; 0 or -EINVAL with a message
int fill_groups(const char* who, group_table& t, const ce_optim_group* groups, int ngroups, const int* segment_group, bool decoupled_ok) {
    CE_CHECK_ARG(groups && ngroups >= 1 && ngroups <= kMaxGroups, "%s: need 1..%d groups (got %d, table %s)", who, kMaxGroups, ngroups,
                 groups ? "given" : "NULL");
    t.segment_group = segment_group;
    t.ngroups = ngroups;
    for (int i = 0; i < kMaxGroups; ++i) t.g[i] = groups[i < ngroups ? i : ngroups - 1];
    for (int i = 0; i < ngroups; ++i)
        CE_CHECK_ARG(decoupled_ok || !groups[i].decoupled, "%s: group %d is decoupled; decoupled weight decay is Adam's (AdamW)", who, i);
    return 0;
}

unsigned flat_blocks(long n) {
    static const long cap = getenv("CE_ADAM_BLOCKS") ? atol(getenv("CE_ADAM_BLOCKS")) : 4096;
    const long blocks = (n + 2047) / 2048;
    return (unsigned)(blocks > cap ? cap : blocks);
}

// what every _ema entry point asks of its two extra arguments; 0 or -EINVAL with a message
int ema_check(const char* who, const float* ema, float ema_rate) {
    CE_CHECK_ARG(ema, "%s: ema is NULL", who);
    CE_CHECK_ARG(ema_rate > 0.f && ema_rate <= 1.f, "%s: ema_rate %g is outside (0, 1]", who, (double)ema_rate);
    return 0;
}

}  // namespace

extern "C" int ce_multi_transpose_bf16(const ce_transpose_job* jobs_device, int njobs, int total_tiles, void* stream) {
    CE_CHECK_ARG(jobs_device && njobs > 0 && total_tiles > 0, "ce_multi_transpose_bf16: empty");
    hipLaunchKernelGGL(multi_transpose_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, jobs_device, njobs);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_zero_segments(float* base, const long* table_device, int nchunks, void* stream) {
    CE_CHECK_ARG(base && table_device && nchunks > 0, "ce_zero_segments: empty");
    hipLaunchKernelGGL(zero_segments_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, base, table_device);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_sumsq(const float* g, long n, float* out, void* stream) {
    CE_CHECK_ARG(n > 0, "ce_sumsq: empty");
    long blocks = (n + 1023) / 1024;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, g, n, out);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_sumsq_segments(const float* g, const long* table_device, int nchunks, float* out, void* stream) {
    CE_CHECK_ARG(g && table_device && out && nchunks > 0, "ce_sumsq_segments: empty");
    hipLaunchKernelGGL(sumsq_segments_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, g, table_device, out);
    CE_LAUNCH_CHECK();
    return 0;
}

// ---- the optimiser step: entry point -> the rule's host part -> run_step -----------------------------------------------------------
// An entry point (extern "C", at the end) only fills a StepCall from its arguments.  The host part of its rule (run_adam, run_sgd,
// run_lion and their grouped forms) checks the rule's scalars and builds Rule::Args.  run_step checks what no rule decides and
// launches.  That is also the order of the checks, which decides the message when several arguments are bad at once:
//   1. the rule's own -- Adam: step >= 1; SGD: sgd_check (momentum, nesterov, a momentum buffer when momentum > 0); Lion: lion_check
//      (m, the betas), then lr / weight decay; the grouped forms then the group table (fill_groups; Lion: every group's lr / weight decay)
//   2. the form: n > 0 (flat), or a table with something in it (tiles / groups)
//   3. the buffers: p and g, every state stream the rule has (Rule::NS), and in the table forms p_bf16, which the tiles are located
//      in; the flat form takes p_bf16 == NULL (no mirror is written)
//   4. the weight average (ema_check), when the _ema twin was called
namespace {

struct StepCall {
    const char* who;                  // the entry point that was called: every message starts with it
    float* p;
    const float* g;
    float* state[2];                  // Adam: m, v; SGD: buf; Lion: m.  Only the first Rule::NS reach a kernel
    void* p_bf16;
    const float* sumsq;
    float max_norm;
    void* stream;
    bool flat = false;                // [0, n); otherwise the table forms: `jobs` in tiles, then `segments`
    long n = 0;
    const ce_transpose_job* jobs = nullptr;
    int njobs = 0, total_tiles = 0;
    const long* segments = nullptr;
    int nsegments = 0;
    const int* segment_group = nullptr;      // the grouped forms (what fill_groups reads)
    const ce_optim_group* groups = nullptr;
    int ngroups = 0;
    bool with_ema = false;            // the _ema twin was called
    float* ema = nullptr;
    float ema_rate = 0.f;
};

StepCall flat_call(const char* who, float* p, const float* g, float* s0, float* s1, void* p_bf16, long n, const float* sumsq,
                   float max_norm, void* stream) {
    StepCall c = {who, p, g, {s0, s1}, p_bf16, sumsq, max_norm, stream};
    c.flat = true, c.n = n;
    return c;
}
StepCall table_call(const char* who, float* p, const float* g, float* s0, float* s1, void* p_bf16, const ce_transpose_job* jobs,
                    int njobs, int total_tiles, const long* segments, int nsegments, const float* sumsq, float max_norm, void* stream) {
    StepCall c = {who, p, g, {s0, s1}, p_bf16, sumsq, max_norm, stream};
    c.jobs = jobs, c.njobs = njobs, c.total_tiles = total_tiles, c.segments = segments, c.nsegments = nsegments;
    return c;
}
StepCall with_groups(StepCall c, const int* segment_group, const ce_optim_group* groups, int ngroups) {
    c.segment_group = segment_group, c.groups = groups, c.ngroups = ngroups;
    return c;
}
StepCall with_ema(StepCall c, float* ema, float ema_rate) {
    c.with_ema = true, c.ema = ema, c.ema_rate = ema_rate;
    return c;
}

// f(std::true_type) or f(std::false_type): the one place where the EMA instantiation of a traversal is chosen
template <class F>
void pick_ema(bool on, F&& f) {
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

template <class Rule>
int run_step(const StepCall& c, const typename Rule::Args& a) {
    const bool tiles = c.jobs && c.njobs > 0 && c.total_tiles > 0, segments = c.segments && c.nsegments > 0;      // either table may be empty
    if (c.flat) CE_CHECK_ARG(c.n > 0, "%s: need n>0", c.who);
    else CE_CHECK_ARG(tiles || segments, "%s: nothing to update", c.who);
    bool buffers = c.p && c.g && (c.flat || c.p_bf16);
    for (int k = 0; k < Rule::NS; ++k) buffers = buffers && c.state[k];
    CE_CHECK_ARG(buffers, "%s: null buffer", c.who);
    if (c.with_ema)
        if (int rc = ema_check(c.who, c.ema, c.ema_rate)) return rc;
    float* const s0 = Rule::NS > 0 ? c.state[0] : nullptr;
    float* const s1 = Rule::NS > 1 ? c.state[1] : nullptr;
    bf16_t* const p16 = (bf16_t*)c.p_bf16;
    const hipStream_t s = (hipStream_t)c.stream;
    pick_ema(c.with_ema, [&](auto on) {
        // without the average the kernels never name the pointer: NULL and rate 0
        constexpr bool EMA = decltype(on)::value;
        float* const ema = EMA ? c.ema : nullptr;
        const float ema_rate = EMA ? c.ema_rate : 0.f;
        if constexpr (!Rule::GROUPED) {      // (no entry point is flat and grouped: those kernels are not instantiated)
            if (c.flat)
                hipLaunchKernelGGL((optim_flat_kernel<Rule, EMA>), dim3(flat_blocks(c.n)), dim3(256), 0, s, c.p, c.g, s0, s1, p16, c.n, a,
                                   ema, ema_rate);
        }
        if (!c.flat && tiles)
            hipLaunchKernelGGL((optim_tiles_kernel<Rule, EMA>), dim3((unsigned)c.total_tiles), dim3(256), 0, s, c.p, c.g, s0, s1, p16,
                               c.jobs, c.njobs, a, ema, ema_rate);
        if (!c.flat && segments)
            hipLaunchKernelGGL((optim_segments_kernel<Rule, EMA>), dim3((unsigned)c.nsegments), dim3(256), 0, s, c.p, c.g, s0, s1, p16,
                               c.segments, a, ema, ema_rate);
    });
    CE_LAUNCH_CHECK();
    return 0;
}

int run_adam(const StepCall& c, float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
    CE_CHECK_ARG(step >= 1, "%s: need step>=1", c.who);
    return run_step<AdamRule>(c, {c.sumsq, c.max_norm, lr, beta1, beta2, eps, weight_decay, adam_bc1(beta1, step), adam_bc2_sqrt(beta2, step)});
}
int run_adam_groups(const StepCall& c, float beta1, float beta2, float eps, int step) {
    CE_CHECK_ARG(step >= 1, "%s: need step>=1", c.who);
    AdamGroupRule::Args a = {c.sumsq, c.max_norm, beta1, beta2, eps, adam_bc1(beta1, step), adam_bc2_sqrt(beta2, step), {}};
    if (int rc = fill_groups(c.who, a.groups, c.groups, c.ngroups, c.segment_group, true)) return rc;
    return run_step<AdamGroupRule>(c, a);
}

// SGD: momentum 0 is the instantiation without a momentum stream (`buf` is then not looked at, NULL or not)
int run_sgd(const StepCall& c, float lr, float momentum, float dampening, float weight_decay, int nesterov, int first_step) {
    if (int rc = sgd_check(c.who, c.state[0], momentum, dampening, nesterov)) return rc;
    const sgd_args a = {c.sumsq, c.max_norm, lr, momentum, 1.0f - dampening, weight_decay, first_step != 0, nesterov != 0};
    return momentum > 0.f ? run_step<SgdRule<true>>(c, a) : run_step<SgdRule<false>>(c, a);
}
int run_sgd_groups(const StepCall& c, float momentum, float dampening, int nesterov, int first_step) {
    if (int rc = sgd_check(c.who, c.state[0], momentum, dampening, nesterov)) return rc;
    sgd_group_args a = {c.sumsq, c.max_norm, momentum, 1.0f - dampening, first_step != 0, nesterov != 0, {}};
    if (int rc = fill_groups(c.who, a.groups, c.groups, c.ngroups, c.segment_group, false)) return rc;
    return momentum > 0.f ? run_step<SgdGroupRule<true>>(c, a) : run_step<SgdGroupRule<false>>(c, a);
}

// what every Lion entry point asks of its momentum and its hyper-parameters (the grouped forms: of every group's lr / weight decay,
// checked in run_lion_groups); 0 or -EINVAL with a message
int lion_check(const char* who, const float* m, float beta1, float beta2) {
    CE_CHECK_ARG(m, "%s: the momentum buffer m is NULL", who);
    CE_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f, "%s: invalid beta1 value %g (outside [0, 1))", who, (double)beta1);
    CE_CHECK_ARG(beta2 >= 0.f && beta2 < 1.f, "%s: invalid beta2 value %g (outside [0, 1))", who, (double)beta2);
    return 0;
}
int lion_scalars_check(const char* who, float lr, float weight_decay) {
    CE_CHECK_ARG(lr >= 0.f, "%s: invalid learning rate %g", who, (double)lr);
    CE_CHECK_ARG(weight_decay >= 0.f, "%s: invalid weight_decay value %g", who, (double)weight_decay);
    return 0;
}
int run_lion(const StepCall& c, float lr, float beta1, float beta2, float weight_decay) {
    if (int rc = lion_check(c.who, c.state[0], beta1, beta2)) return rc;
    if (int rc = lion_scalars_check(c.who, lr, weight_decay)) return rc;
    return run_step<LionRule>(c, {c.sumsq, c.max_norm, lr, beta1, beta2, weight_decay});
}
int run_lion_groups(const StepCall& c, float beta1, float beta2) {
    if (int rc = lion_check(c.who, c.state[0], beta1, beta2)) return rc;
    LionGroupRule::Args a = {c.sumsq, c.max_norm, beta1, beta2, {}};
    if (int rc = fill_groups(c.who, a.groups, c.groups, c.ngroups, c.segment_group, true)) return rc;      // (`decoupled` is not read)
    for (int i = 0; i < c.ngroups; ++i)
        if (int rc = lion_scalars_check(c.who, c.groups[i].lr, c.groups[i].weight_decay)) return rc;
    return run_step<LionGroupRule>(c, a);
}

}  // namespace

// ---- the eighteen entry points: flat, tiles and groups for each rule, each with its _ema twin ----------------------------------------
extern "C" int ce_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* sumsq,
                            float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                            void* stream) {
    const StepCall c = flat_call("ce_adam_step", p, g, m, v, p_bf16, n, sumsq, max_norm, stream);
    return run_adam(c, lr, beta1, beta2, eps, weight_decay, step);
}
extern "C" int ce_adam_step_ema(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* sumsq,
                                float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                float* ema, float ema_rate, void* stream) {
    const StepCall c = flat_call("ce_adam_step_ema", p, g, m, v, p_bf16, n, sumsq, max_norm, stream);
    return run_adam(with_ema(c, ema, ema_rate), lr, beta1, beta2, eps, weight_decay, step);
}
extern "C" int ce_adam_step_tiles(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device,
                                  int njobs, int total_tiles, const long* segments_device, int nsegments, const float* sumsq,
                                  float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                  void* stream) {
    const StepCall c = table_call("ce_adam_step_tiles", p, g, m, v, p_bf16, jobs_device, njobs, total_tiles, segments_device, nsegments,
                                  sumsq, max_norm, stream);
    return run_adam(c, lr, beta1, beta2, eps, weight_decay, step);
}
extern "C" int ce_adam_step_tiles_ema(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device,
                                      int njobs, int total_tiles, const long* segments_device, int nsegments, const float* sumsq,
                                      float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                      float* ema, float ema_rate, void* stream) {
    const StepCall c = table_call("ce_adam_step_tiles_ema", p, g, m, v, p_bf16, jobs_device, njobs, total_tiles, segments_device, nsegments,
                                  sumsq, max_norm, stream);
    return run_adam(with_ema(c, ema, ema_rate), lr, beta1, beta2, eps, weight_decay, step);
}
extern "C" int ce_adam_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device,
                                   int njobs, int total_tiles, const long* segments_device, int nsegments, const int* segment_group,
                                   const float* sumsq, float max_norm, const ce_optim_group* groups, int ngroups, float beta1,
                                   float beta2, float eps, int step, void* stream) {
    const StepCall c = table_call("ce_adam_step_groups", p, g, m, v, p_bf16, jobs_device, njobs, total_tiles, segments_device, nsegments,
                                  sumsq, max_norm, stream);
    return run_adam_groups(with_groups(c, segment_group, groups, ngroups), beta1, beta2, eps, step);
}
extern "C" int ce_adam_step_groups_ema(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device,
                                       int njobs, int total_tiles, const long* segments_device, int nsegments, const int* segment_group,
                                       const float* sumsq, float max_norm, const ce_optim_group* groups, int ngroups, float beta1,
                                       float beta2, float eps, int step, float* ema, float ema_rate, void* stream) {
    const StepCall c = table_call("ce_adam_step_groups_ema", p, g, m, v, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_adam_groups(with_ema(with_groups(c, segment_group, groups, ngroups), ema, ema_rate), beta1, beta2, eps, step);
}

extern "C" int ce_sgd_step(float* p, const float* g, float* buf, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                           float momentum, float dampening, float weight_decay, int nesterov, int first_step, void* stream) {
    const StepCall c = flat_call("ce_sgd_step", p, g, buf, nullptr, p_bf16, n, sumsq, max_norm, stream);
    return run_sgd(c, lr, momentum, dampening, weight_decay, nesterov, first_step);
}
extern "C" int ce_sgd_step_ema(float* p, const float* g, float* buf, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                               float momentum, float dampening, float weight_decay, int nesterov, int first_step, float* ema,
                               float ema_rate, void* stream) {
    const StepCall c = flat_call("ce_sgd_step_ema", p, g, buf, nullptr, p_bf16, n, sumsq, max_norm, stream);
    return run_sgd(with_ema(c, ema, ema_rate), lr, momentum, dampening, weight_decay, nesterov, first_step);
}
extern "C" int ce_sgd_step_tiles(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                 int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm,
                                 float lr, float momentum, float dampening, float weight_decay, int nesterov, int first_step,
                                 void* stream) {
    const StepCall c = table_call("ce_sgd_step_tiles", p, g, buf, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_sgd(c, lr, momentum, dampening, weight_decay, nesterov, first_step);
}
extern "C" int ce_sgd_step_tiles_ema(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                     int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm,
                                     float lr, float momentum, float dampening, float weight_decay, int nesterov, int first_step,
                                     float* ema, float ema_rate, void* stream) {
    const StepCall c = table_call("ce_sgd_step_tiles_ema", p, g, buf, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_sgd(with_ema(c, ema, ema_rate), lr, momentum, dampening, weight_decay, nesterov, first_step);
}
extern "C" int ce_sgd_step_groups(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                  int total_tiles, const long* segments_device, int nsegments, const int* segment_group,
                                  const float* sumsq, float max_norm, const ce_optim_group* groups, int ngroups, float momentum,
                                  float dampening, int nesterov, int first_step, void* stream) {
    const StepCall c = table_call("ce_sgd_step_groups", p, g, buf, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_sgd_groups(with_groups(c, segment_group, groups, ngroups), momentum, dampening, nesterov, first_step);
}
extern "C" int ce_sgd_step_groups_ema(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                      int total_tiles, const long* segments_device, int nsegments, const int* segment_group,
                                      const float* sumsq, float max_norm, const ce_optim_group* groups, int ngroups, float momentum,
                                      float dampening, int nesterov, int first_step, float* ema, float ema_rate, void* stream) {
    const StepCall c = table_call("ce_sgd_step_groups_ema", p, g, buf, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_sgd_groups(with_ema(with_groups(c, segment_group, groups, ngroups), ema, ema_rate), momentum, dampening, nesterov,
                          first_step);
}

extern "C" int ce_lion_step(float* p, const float* g, float* m, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                            float beta1, float beta2, float weight_decay, void* stream) {
    const StepCall c = flat_call("ce_lion_step", p, g, m, nullptr, p_bf16, n, sumsq, max_norm, stream);
    return run_lion(c, lr, beta1, beta2, weight_decay);
}
extern "C" int ce_lion_step_ema(float* p, const float* g, float* m, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                                float beta1, float beta2, float weight_decay, float* ema, float ema_rate, void* stream) {
    const StepCall c = flat_call("ce_lion_step_ema", p, g, m, nullptr, p_bf16, n, sumsq, max_norm, stream);
    return run_lion(with_ema(c, ema, ema_rate), lr, beta1, beta2, weight_decay);
}
extern "C" int ce_lion_step_tiles(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                  int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm,
                                  float lr, float beta1, float beta2, float weight_decay, void* stream) {
    const StepCall c = table_call("ce_lion_step_tiles", p, g, m, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_lion(c, lr, beta1, beta2, weight_decay);
}
extern "C" int ce_lion_step_tiles_ema(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                      int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm,
                                      float lr, float beta1, float beta2, float weight_decay, float* ema, float ema_rate,
                                      void* stream) {
    const StepCall c = table_call("ce_lion_step_tiles_ema", p, g, m, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_lion(with_ema(c, ema, ema_rate), lr, beta1, beta2, weight_decay);
}
extern "C" int ce_lion_step_groups(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                   int total_tiles, const long* segments_device, int nsegments, const int* segment_group,
                                   const float* sumsq, float max_norm, const ce_optim_group* groups, int ngroups, float beta1,
                                   float beta2, void* stream) {
    const StepCall c = table_call("ce_lion_step_groups", p, g, m, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_lion_groups(with_groups(c, segment_group, groups, ngroups), beta1, beta2);
}
extern "C" int ce_lion_step_groups_ema(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                                       int total_tiles, const long* segments_device, int nsegments, const int* segment_group,
                                       const float* sumsq, float max_norm, const ce_optim_group* groups, int ngroups, float beta1,
                                       float beta2, float* ema, float ema_rate, void* stream) {
    const StepCall c = table_call("ce_lion_step_groups_ema", p, g, m, nullptr, p_bf16, jobs_device, njobs, total_tiles, segments_device,
                                  nsegments, sumsq, max_norm, stream);
    return run_lion_groups(with_ema(with_groups(c, segment_group, groups, ngroups), ema, ema_rate), beta1, beta2);
}

extern "C" int ce_swap_cast_bf16(float* a, float* b, void* a_bf16, long n, void* stream) {
    CE_CHECK_ARG(a && b && a_bf16 && a != b && n > 0, "ce_swap_cast_bf16: null or identical buffers, or n <= 0");
    CE_CHECK_ARG((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b)) % 16 == 0 && reinterpret_cast<size_t>(a_bf16) % 8 == 0,
                 "ce_swap_cast_bf16: a and b must be 16-byte aligned, a_bf16 8-byte aligned");
    hipLaunchKernelGGL(swap_cast_kernel, dim3(flat_blocks(2 * n)), dim3(256), 0, (hipStream_t)stream, a, b, (bf16_t*)a_bf16, n);
    CE_LAUNCH_CHECK();
    return 0;
}
