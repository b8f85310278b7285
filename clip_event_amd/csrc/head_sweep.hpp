// What a similarity sweep is, said once for the kernels that run one: the loss heads (infonce.hip) and top-k scoring
// (retrieval.hip).
//
// A workgroup of NW waves (4, or 8: eight_waves) keeps one block of HB = 32 RESIDENT rows in LDS and sweeps HB-row STREAMED
// blocks of the other matrix; the streamed blocks are cut into `splits` ranges (grid.y) so that few resident blocks still fill
// the chip.  The tile S^T[i][j] = <streamed_i, resident_j> comes from v_mfma_f32_32x32x2_f32, each wave over its 1 / NW of the
// width E, the NW partial tiles added through LDS in wave order: a similarity summed by eight waves differs in its last bits
// from the same one summed by four, so every sweep that must reproduce another's scores takes its wave count from the same rule.
// Here: the block size, the accumulator layout, the resident-block load, the LDS footprint, the wave rule, the split choice, the
// merge of the splits' (max, sum) pairs and the argument check of a feature matrix.  The tile arithmetic itself is written out
// in infonce_kernel and in retrieval.hip's sim_tile (DESIGN.md "Head sweep skeleton": one shared tile function cost
// infonce_kernel<DQ, 8, distill> a third of its occupancy).
#pragma once
#include "common.hpp"

namespace head_sweep {

constexpr int HB = 32;          // rows per resident / streamed block

__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }   // 32x32 C/D row of reg r

// The resident block -> LDS: rows r0 .. r0 + 31 of the [n, E] matrix m (row r0 + r is row gather[r0 + r] of m where a gather is
// given), zeros behind row n, row pitch E + 4 floats (conflict-free ds_read_b128)
template <int NW>
__device__ __forceinline__ void load_residents(const float* m, long ld, int n, const long* gather, int E, float* res_l, int r0,
                                               int tid) {
    const int pitch = E + 4;
    for (int idx = tid; idx < HB * (E / 4); idx += 64 * NW) {
        const int r = idx / (E / 4), c = (idx - r * (E / 4)) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < n) {
            const long src = gather ? gather[r0 + r] : (long)(r0 + r);
            v = *reinterpret_cast<const f32x4*>(m + src * ld + c);
        }
        *reinterpret_cast<f32x4*>(res_l + r * pitch + c) = v;
    }
}

// Log-sum-exp statistics of one row from its per-split (max, sum) pairs, `stride` floats apart: m = the largest max, l = the
// sums brought to it, in split order (a split without keys: 0 * exp(-inf) = 0).  The row's log-sum-exp is m + __logf(l).
__device__ __forceinline__ void merge_max_sum(const float* p, long stride, int splits, float& m, float& l) {
    m = -INFINITY;
    for (int s = 0; s < splits; ++s) m = fmaxf(m, p[s * stride]);
    l = 0.f;
    for (int s = 0; s < splits; ++s) l += p[s * stride + 1] * __expf(p[s * stride] - m);
}

// resident block [32][E+4] + the waves' partial tiles [NW][32][33] (also the output transpose of the gradient sweeps)
inline size_t lds_bytes(int E, int nw) { return (size_t)(HB * (E + 4) + nw * HB * 33) * 4; }

// Eight waves split BOTH widths in eight: the similarity's E and the width Eval of the values a gradient product streams
// (a 128-wide value matrix under a 256-wide similarity would get no e-tile); a sweep without values passes Eval = E.
// E = 1024 with eight partial tiles exceeds 160 KiB of LDS.
inline bool eight_waves(int E, int Eval) { return E % 256 == 0 && E <= 768 && Eval % 256 == 0; }

struct Splits {
    int splits, blocks_per_split;
};

// Ranges of the streamed blocks before rounding: `requested`, or (0) about two workgroups per CU when the resident blocks
// alone do not fill the chip; never more than `cap` or than there are blocks.  An upper bound of split_choice().splits.
inline int split_bound(int nres, int nstr, int requested, int cap) {
    const int rb = ce_div_up(nres, HB), sblocks = ce_div_up(nstr, HB);
    int splits = requested ? requested : ce_div_up(512, rb);
    if (splits > sblocks) splits = sblocks;
    if (splits > cap) splits = cap;
    return splits < 1 ? 1 : splits;
}

// The launch's choice: equal ranges of blocks_per_split blocks, `splits` the number of ranges that are not empty
inline Splits split_choice(int nres, int nstr, int requested, int cap) {
    const int sblocks = ce_div_up(nstr, HB);
    const int bps = ce_div_up(sblocks, split_bound(nres, nstr, requested, cap));
    return {ce_div_up(sblocks, bps), bps};
}

// A feature matrix of the entry point `what`: [rows, E] fp32 with leading dimension ld, rows read 16 bytes at a time; `name`
// is what the entry point calls the width (E, Es, Et)
inline int check_features(const char* what, const char* name, const float* p, long ld, int E) {
    CE_CHECK_ARG(p, "%s: null buffer", what);
    CE_CHECK_ARG(E >= 128 && E % 128 == 0 && E <= 1024, "%s: %s must be a multiple of 128 in 128..1024 (got %d)", what, name, E);
    CE_CHECK_ARG(ld >= E && ld % 4 == 0, "%s: leading dimensions must be >= %s and multiples of 4 (got %ld)", what, name, ld);
    return 0;
}

}  // namespace head_sweep
