// Scoring without the logits matrix: the best k keys of every query with their scores, the log-sum-exp over all keys and
// the rank of one target key per query (zero-shot top-k, retrieval R@k / median rank), on the similarity sweep of
// infonce.hip (MODE_FWD) -- the [nq, nk] matrix (10 GB at 50 k x 50 k) is never written.
//
//   score(r, c) = s <q_r, keys_c>,  s = exp(*logit_scale) or 1;   order: score descending, then key index ascending
//   top_val / top_idx [nq, k]: the first k keys in that order (padded with -inf / -1 past nk)
//   lse[r] = log sum_c exp(score(r, c));   rank[r] = number of keys before target[r] in that order (-1: no valid target)
//
// Skeleton: a workgroup (4 waves, or 8 where E is a multiple of 256 up to 768) keeps 32 RESIDENT queries in LDS and sweeps
// 32-key STREAMED blocks of its split of the keys; the tile S^T[i][j] = <key_i, query_j> comes from v_mfma_f32_32x32x2_f32
// (exact fp32 FMA chains), each wave over its slice of E, the partial tiles summed through LDS in wave order.  One
// device function (sim_tile) produces every score, so a (query, key) pair gets the same bits wherever it falls in a tile,
// a split or the grid: bit-identical key rows tie exactly, and nothing below depends on the number of splits.
//   * selection: after the LDS sum the 32 x 32 tile is shared out over ALL lanes of the workgroup (16 / NW rows per lane
//     instead of every wave repeating the whole tile).  A lane sees its keys in ascending index order, so "strictly
//     greater than my k-th best" is the whole threshold test, and the insertion behind it is a compare-exchange chain over
//     registers with compile-time indices (k buckets 1, 8, 16).
//   * target rank: a pre-pass runs the same tile code with the resident queries' target rows gathered as the streamed block
//     and keeps the diagonal: the target's score with the sweep's own arithmetic.  The sweep then counts, per lane, the keys
//     that come before (score, index) of the target.
//   * per split: the 2 NW lane lists of a query are merged in LDS (position of an element = its place in its own list +
//     binary searches in the others), and the split's top-k, (max, sum) and count go to the workspace; a small kernel merges
//     the splits the same way and writes the outputs.
// Plain vector stores only; no allocation, no synchronisation.
#include <mutex>

#include "common.hpp"
#include "head_sweep.hpp"
#include "../../include/clip_event_hip.h"

using namespace head_sweep;

namespace {

struct TopkArgs {
    const float* q; long ldq; int nq;              // resident matrix: queries
    const float* keys; long ldk; int nk;           // streamed matrix: keys
    const float* logit_scale;                      // nullable: scale 1
    const long* target;                            // nullable, [nq]
    float* tscore;                                 // [nq] score of the target (pre-pass -> sweep)
    float* p_ms;                                   // [splits][nq][2] partial (max, sum)
    int* p_cnt;                                    // [splits][nq] keys before the target
    float* p_val; int* p_idx;                      // [splits][nq][KB] partial top-k
    int E, splits, blocks_per_split;
};

// (yv, yi) comes before (xv, xi): score descending, then index ascending
__device__ __forceinline__ bool before(float yv, int yi, float xv, int xi) { return yv > xv || (yv == xv && yi < xi); }

// how many entries of a list sorted in that order come before (xv, xi); padding (-inf, -1) sits at the end and never does
__device__ __forceinline__ int count_before(const float* v, const int* i, int n, float xv, int xi) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (before(v[mid], i[mid], xv, xi)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One 32 x 32 tile of scores.  arow: this lane's streamed row (lane & 31) at its wave's slice of E, brow likewise for the
// resident row in LDS.  Returns in S[t] the score of streamed row row_of(wave * R + t, h) against resident row j.  The ONLY
// place a score is computed: the MFMA chain over the wave's slice, the NW partial tiles added in wave order, one multiply.
template <int NW>
__device__ __forceinline__ void sim_tile(const float* arow, bool ivalid, const float* brow, int E, float* part_l, int wave,
                                         int j, int h, float scale, float (&S)[16 / NW]) {
    constexpr int R = 16 / NW;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 4
    for (int u = 0; u < E / (8 * NW); ++u) {
        f32x4 av = {0.f, 0.f, 0.f, 0.f};
        if (ivalid) av = *reinterpret_cast<const f32x4*>(arow + 8 * u);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(brow + 8 * u);
#pragma unroll
        for (int x = 0; x < 4; ++x) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[x], bv[x], acc, 0, 0, 0);
    }
    __syncthreads();          // the previous tile's readers of part_l are done
#pragma unroll
    for (int r = 0; r < 16; ++r) part_l[(wave * HB + row_of(r, h)) * 33 + j] = acc[r];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int i = row_of(wave * R + t, h);
        float sum = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += part_l[(w * HB + i) * 33 + j];
        S[t] = scale * sum;
    }
}

// pre-pass: tscore[r] = score(r, target[r]) from sim_tile, the target rows gathered as the streamed block (diagonal)
template <int NW>
__global__ __launch_bounds__(64 * NW) void target_score_kernel(TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = 16 / NW;
    const int E = a.E, pitch = E + 4;
    float* res_l = reinterpret_cast<float*>(smem);                       // [32][E+4]
    float* part_l = res_l + HB * pitch;                                  // [NW][32][33]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * HB;
    const float scale = a.logit_scale ? __expf(*a.logit_scale) : 1.f;
    load_residents<NW>(a.q, a.ldq, a.nq, nullptr, E, res_l, r0, tid);
    const bool jvalid = r0 + j < a.nq;
    const long tgt = jvalid ? a.target[r0 + j] : -1;
    const bool tvalid = tgt >= 0 && tgt < a.nk;                          // anything else is never dereferenced
    __syncthreads();
    const int e_lo = wave * (E / NW);
    float S[R];
    sim_tile<NW>(a.keys + (tvalid ? tgt : 0) * a.ldk + e_lo + 4 * h, tvalid, res_l + j * pitch + e_lo + 4 * h, E, part_l, wave,
                 j, h, scale, S);
#pragma unroll
    for (int t = 0; t < R; ++t)
        if (row_of(wave * R + t, h) == j && jvalid) a.tscore[r0 + j] = S[t];
}

template <int NW, int KB>
__global__ __launch_bounds__(64 * NW) void topk_sweep_kernel(TopkArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = 16 / NW, L = 2 * NW;                               // rows per lane and tile; lane lists per query
    const int E = a.E, pitch = E + 4;
    float* res_l = reinterpret_cast<float*>(smem);                       // [32][E+4]
    float* part_l = res_l + HB * pitch;                                  // [NW][32][33]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * HB;
    const float scale = a.logit_scale ? __expf(*a.logit_scale) : 1.f;
    load_residents<NW>(a.q, a.ldq, a.nq, nullptr, E, res_l, r0, tid);
    const bool jvalid = r0 + j < a.nq;
    const long tgt64 = (a.target && jvalid) ? a.target[r0 + j] : -1;
    const bool tvalid = tgt64 >= 0 && tgt64 < a.nk;
    const int tgt = tvalid ? (int)tgt64 : -1;
    const float ts = tvalid ? a.tscore[r0 + j] : 0.f;
    __syncthreads();

    float run_m = -INFINITY, run_l = 0.f;                 // online log-sum-exp of query j over this lane's keys
    int cnt = 0;                                          // this lane's keys that come before the target
    float lv[KB];                                         // this lane's best KB, sorted; its keys arrive in index order,
    int li[KB];                                           // so a later key never displaces an equal score
#pragma unroll
    for (int p = 0; p < KB; ++p) { lv[p] = -INFINITY; li[p] = -1; }
    const int e_lo = wave * (E / NW);
    const float* brow = res_l + j * pitch + e_lo + 4 * h;

    const int sb0 = blockIdx.y * a.blocks_per_split;
    const int sb1 = min(sb0 + a.blocks_per_split, (a.nk + HB - 1) / HB);
    for (int sb = sb0; sb < sb1; ++sb) {
        const int c0 = sb * HB;
        const bool ivalid = c0 + j < a.nk;
        float S[R];
        sim_tile<NW>(a.keys + (long)(c0 + j) * a.ldk + e_lo + 4 * h, ivalid, brow, E, part_l, wave, j, h, scale, S);
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < R; ++t)
            if (c0 + row_of(wave * R + t, h) < a.nk) mx = fmaxf(mx, S[t]);
        if (mx > -INFINITY) {
            const float m_new = fmaxf(run_m, mx);
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < R; ++t)
                if (c0 + row_of(wave * R + t, h) < a.nk) sum += __expf(S[t] - m_new);
            run_l = run_l * __expf(run_m - m_new) + sum;                  // run_m = -inf at first: exp(-inf) = 0
            run_m = m_new;
        }
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int c = c0 + row_of(wave * R + t, h);
            if (c >= a.nk) continue;
            const float v = S[t];
            if (tvalid && before(v, c, ts, tgt)) ++cnt;
            if (v > lv[KB - 1]) {
                lv[KB - 1] = v;
                li[KB - 1] = c;
#pragma unroll
                for (int p = KB - 1; p > 0; --p) {
                    const bool sw = lv[p] > lv[p - 1];
                    const float v0 = lv[p - 1], v1 = lv[p];
                    const int i0 = li[p - 1], i1 = li[p];
                    lv[p - 1] = sw ? v1 : v0; lv[p] = sw ? v0 : v1;
                    li[p - 1] = sw ? i1 : i0; li[p] = sw ? i0 : i1;
                }
            }
        }
    }

    // ---- merge the L lane lists of every query in LDS (the sweep's buffers are free now) ----
    __syncthreads();
    float* lst_v = reinterpret_cast<float*>(smem);                       // [32][L][KB]
    int* lst_i = reinterpret_cast<int*>(lst_v + HB * L * KB);            // [32][L][KB]
    float* ms_l = reinterpret_cast<float*>(lst_i + HB * L * KB);         // [32][L][2]
    int* cnt_l = reinterpret_cast<int*>(ms_l + HB * L * 2);              // [32][L]
    float* out_v = reinterpret_cast<float*>(cnt_l + HB * L);             // [32][KB]
    int* out_i = reinterpret_cast<int*>(out_v + HB * KB);                // [32][KB]
    const int mine = j * L + wave * 2 + h;
#pragma unroll
    for (int p = 0; p < KB; ++p) { lst_v[mine * KB + p] = lv[p]; lst_i[mine * KB + p] = li[p]; }
    ms_l[mine * 2] = run_m;
    ms_l[mine * 2 + 1] = run_l;
    cnt_l[mine] = cnt;
    __syncthreads();
    const int n_split = min(a.nk, sb1 * HB) - sb0 * HB;                  // valid keys of this split (>= 1)
    for (int e = tid; e < HB * KB; e += 64 * NW)                         // positions no key reaches: padding
        if (e % KB >= n_split) { out_v[e] = -INFINITY; out_i[e] = -1; }
    for (int e = tid; e < HB * L * KB; e += 64 * NW) {
        const int qi = e / (L * KB), rem = e - qi * (L * KB), la = rem / KB;
        const float xv = lst_v[e];
        const int xi = lst_i[e];
        if (xi < 0) continue;
        int pos = rem - la * KB;                                         // its own list is sorted: that many come before it
        for (int lb = 0; lb < L && pos < KB; ++lb)
            if (lb != la) pos += count_before(lst_v + (qi * L + lb) * KB, lst_i + (qi * L + lb) * KB, KB, xv, xi);
        if (pos < KB) { out_v[qi * KB + pos] = xv; out_i[qi * KB + pos] = xi; }
    }
    if (tid < HB && r0 + tid < a.nq) {
        float m = -INFINITY;
        for (int l = 0; l < L; ++l) m = fmaxf(m, ms_l[(tid * L + l) * 2]);
        float s = 0.f;
        int c = 0;
        for (int l = 0; l < L; ++l) {
            s += ms_l[(tid * L + l) * 2 + 1] * __expf(ms_l[(tid * L + l) * 2] - m);      // a lane without keys: 0 * exp(-inf)
            c += cnt_l[tid * L + l];
        }
        const long o = (long)blockIdx.y * a.nq + r0 + tid;
        a.p_ms[o * 2] = m;
        a.p_ms[o * 2 + 1] = s;
        a.p_cnt[o] = c;
    }
    __syncthreads();
    for (int e = tid; e < HB * KB; e += 64 * NW) {
        const int qi = e / KB;
        if (r0 + qi < a.nq) {
            const long o = ((long)blockIdx.y * a.nq + r0 + qi) * KB + (e - qi * KB);
            a.p_val[o] = out_v[e];
            a.p_idx[o] = out_i[e];
        }
    }
}

// merge the splits: one wave per query
__global__ __launch_bounds__(256) void topk_merge_kernel(TopkArgs a, int KB, int k, float* __restrict__ top_val,
                                                         int64_t* __restrict__ top_idx, float* __restrict__ lse,
                                                         int64_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.nq) return;
    const long stride = (long)a.nq * KB;                                 // between the lists of two splits
    const float* v = a.p_val + (long)r * KB;
    const int* ix = a.p_idx + (long)r * KB;
    for (int p = a.nk + lane; p < k; p += 64) {                          // nk < k: padding
        top_val[(long)r * k + p] = -INFINITY;
        top_idx[(long)r * k + p] = -1;
    }
    for (int e = lane; e < a.splits * KB; e += 64) {
        const int la = e / KB;
        const float xv = v[la * stride + (e - la * KB)];
        const int xi = ix[la * stride + (e - la * KB)];
        if (xi < 0) continue;
        int pos = e - la * KB;
        for (int lb = 0; lb < a.splits && pos < k; ++lb)
            if (lb != la) pos += count_before(v + lb * stride, ix + lb * stride, KB, xv, xi);
        if (pos < k) {
            top_val[(long)r * k + pos] = xv;
            top_idx[(long)r * k + pos] = xi;
        }
    }
    if (lane == 0) {
        if (lse) {
            float m, l;
            merge_max_sum(a.p_ms + 2L * r, 2L * a.nq, a.splits, m, l);
            lse[r] = m + __logf(l);
        }
        if (rank) {
            const long t = a.target[r];
            long c = -1;
            if (t >= 0 && t < a.nk) {
                c = 0;
                for (int s = 0; s < a.splits; ++s) c += a.p_cnt[(long)s * a.nq + r];
            }
            rank[r] = c;
        }
    }
}

size_t merge_lds_bytes(int nw, int kb) { return (size_t)(HB * 2 * nw * (2 * kb + 3) + 2 * HB * kb) * 4; }
size_t topk_lds_bytes(int E, int nw, int kb) {
    const size_t s = lds_bytes(E, nw), m = merge_lds_bytes(nw, kb);
    return s > m ? s : m;
}

int bucket_of(int k) { return k == 1 ? 1 : (k <= 8 ? 8 : 16); }

// rows of per-split partials the workspace holds.  splits = 0: a bound on nq * (the launcher's choice) that grows with nq
// (the choice itself falls as nq grows): nq * ceil(512 / rb) <= 32 rb (512 / rb + 1)
long partial_rows(int nq, int nk, int splits) {
    if (splits == 0) return 32L * (512 + ce_div_up(nq, HB));
    const int sblocks = ce_div_up(nk, HB);
    return (long)nq * (splits < sblocks ? splits : sblocks);
}

template <int NW, int KB>
void launch_sweep(const TopkArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((topk_sweep_kernel<NW, KB>), dim3(ce_div_up(a.nq, HB), a.splits), dim3(64 * NW), topk_lds_bytes(a.E, NW, KB),
                       s, a);
}
template <int NW>
void launch_sweep_k(const TopkArgs& a, int kb, hipStream_t s) {
    if (kb == 1) launch_sweep<NW, 1>(a, s);
    else if (kb == 8) launch_sweep<NW, 8>(a, s);
    else launch_sweep<NW, 16>(a, s);
}

template <typename K>
void allow_lds(K kernel, size_t bytes) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

extern "C" size_t ce_score_topk_workspace_bytes(int nq, int nk, int k, int splits) {
    if (nq < 1 || nk < 1 || k < 1 || k > CE_TOPK_MAX || splits < 0 || splits > CE_INFONCE_MAX_SPLITS) return 0;
    return sizeof(float) * ((size_t)nq + (size_t)partial_rows(nq, nk, splits) * (3 + 2 * bucket_of(k)));
}

extern "C" int ce_score_topk(const float* q, long ldq, int nq, const float* keys, long ldk, int nk, int E,
                             const float* logit_scale, const int64_t* target, int k, int splits, float* top_val,
                             int64_t* top_idx, float* lse, int64_t* rank, void* workspace, void* stream) {
    CE_CHECK_ARG(nq > 0 && nk > 0, "ce_score_topk: empty problem (nq = %d, nk = %d)", nq, nk);
    CE_CHECK_ARG(k >= 1 && k <= CE_TOPK_MAX, "ce_score_topk: k must be in 1..%d (got %d)", CE_TOPK_MAX, k);
    CE_CHECK_ARG(splits >= 0 && splits <= CE_INFONCE_MAX_SPLITS, "ce_score_topk: splits must be 0 or 1..%d (got %d)",
                 CE_INFONCE_MAX_SPLITS, splits);
    if (int rc = check_features("ce_score_topk", "E", q, ldq, E)) return rc;
    if (int rc = check_features("ce_score_topk", "E", keys, ldk, E)) return rc;
    CE_CHECK_ARG(top_val && top_idx && workspace, "ce_score_topk: null output");
    CE_CHECK_ARG(!rank || target, "ce_score_topk: rank needs target");
    const int kb = bucket_of(k);
    const long rows = partial_rows(nq, nk, splits);
    TopkArgs a{};
    a.q = q; a.ldq = ldq; a.nq = nq; a.keys = keys; a.ldk = ldk; a.nk = nk; a.E = E;
    a.logit_scale = logit_scale;
    a.target = rank ? (const long*)target : nullptr;          // without rank nobody reads the count
    // splits of the key range: the caller's, or about two workgroups per CU when the queries alone do not fill the chip
    const Splits sp = split_choice(nq, nk, splits, CE_INFONCE_MAX_SPLITS);
    a.splits = sp.splits;
    a.blocks_per_split = sp.blocks_per_split;
    a.tscore = (float*)workspace;
    a.p_ms = a.tscore + nq;
    a.p_cnt = (int*)(a.p_ms + 2 * rows);
    a.p_val = (float*)(a.p_cnt + rows);
    a.p_idx = (int*)(a.p_val + rows * kb);
    static std::once_flag flag;
    std::call_once(flag, [] {
        allow_lds(target_score_kernel<4>, lds_bytes(1024, 4));
        allow_lds(target_score_kernel<8>, lds_bytes(768, 8));
        allow_lds(topk_sweep_kernel<4, 1>, topk_lds_bytes(1024, 4, 1));
        allow_lds(topk_sweep_kernel<4, 8>, topk_lds_bytes(1024, 4, 8));
        allow_lds(topk_sweep_kernel<4, 16>, topk_lds_bytes(1024, 4, 16));
        allow_lds(topk_sweep_kernel<8, 1>, topk_lds_bytes(768, 8, 1));
        allow_lds(topk_sweep_kernel<8, 8>, topk_lds_bytes(768, 8, 8));
        allow_lds(topk_sweep_kernel<8, 16>, topk_lds_bytes(768, 8, 16));
    });
    hipStream_t s = (hipStream_t)stream;
    const bool eight = eight_waves(E, E);
    if (a.target) {
        if (eight) hipLaunchKernelGGL(target_score_kernel<8>, dim3(ce_div_up(nq, HB)), dim3(512), lds_bytes(E, 8), s, a);
        else hipLaunchKernelGGL(target_score_kernel<4>, dim3(ce_div_up(nq, HB)), dim3(256), lds_bytes(E, 4), s, a);
        CE_LAUNCH_CHECK();
    }
    if (eight) launch_sweep_k<8>(a, kb, s);
    else launch_sweep_k<4>(a, kb, s);
    CE_LAUNCH_CHECK();
    hipLaunchKernelGGL(topk_merge_kernel, dim3(ce_div_up(nq, 4)), dim3(256), 0, s, a, kb, k, top_val, top_idx, lse, rank);
    CE_LAUNCH_CHECK();
    return 0;
}
