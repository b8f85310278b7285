// Launch policy of the TN GEMM family: see tn_plan.hpp.
#include "tn_plan.hpp"

#include <stdlib.h>

namespace {

inline int div_up(long a, long b) { return (int)((a + b - 1) / b); }

// The M split every kernel gets: whole 64-row contraction tiles per split, and no split left without rows.
inline void set_splits(TNPlan& p, int M, int splits) {
    const int m_tiles = div_up(M, TN_PLAN_BM);
    if (splits > m_tiles) splits = m_tiles;
    if (splits < 1) splits = 1;
    p.m_per_split = div_up(m_tiles, splits) * TN_PLAN_BM;
    p.splits = div_up(M, p.m_per_split);
}

inline int env_int(const char* name, int otherwise) {
    const char* e = getenv(name);
    return e ? atoi(e) : otherwise;
}

}  // namespace

TNKnobs tn_knobs_from_env() {
    TNKnobs k;
    k.variant = env_int("CE_GEMM_TN", k.variant);
    k.force_splits = env_int("CE_TN3_SPLITS", k.force_splits);
    k.depth = env_int("CE_TN3_DEPTH", k.depth);
    k.rows = env_int("CE_TN3_ROWS", k.rows);
    k.loader_waves = env_int("CE_TN3_LW", k.loader_waves);
    return k;
}

TNPlan tn_plan(int M, int count, const int* Nn, const int* Kk, int splits_arg, bool overwrite, const TNKnobs& knobs) {
    TNPlan p = {};
    // v3 (256x256 tiles, one workgroup per CU) when every problem is a multiple of 256 both ways and the contraction is
    // long enough to amortise the 64 KB prologue
    bool can3 = knobs.variant == 3;
    for (int i = 0; i < count; ++i) can3 = can3 && tn_tiles_256(M, Nn[i], Kk[i]);
    const int edge = can3 ? 256 : 128;
    int tiles = 0;
    for (int i = 0; i < count; ++i) {
        p.tiles_n[i] = div_up(Nn[i], edge);
        p.tiles_k[i] = div_up(Kk[i], edge);
        tiles += p.tiles_n[i] * p.tiles_k[i];
        p.tile_end[i] = tiles;
    }
    for (int i = count; i < CE_TN_MAX_GROUP; ++i) p.tile_end[i] = tiles;
    p.tiles = tiles;
    p.depth = knobs.depth < 1 ? 1 : (knobs.depth > 3 ? 3 : knobs.depth);
    const int m_tiles = div_up(M, TN_PLAN_BM);

    if (!can3) {
        // v1, v2: one resident round (at most 2 workgroups per CU = 512 slots), never a ragged second round of SPLIT tiles
        p.form = knobs.variant == 1 ? TN_V1 : TN_V2;
        p.rows = TN_PLAN_BM;
        p.stages = 2;
        p.lds_bytes = p.form == TN_V1 ? TN_PLAN_LDS_V1 : TN_PLAN_LDS_128;
        set_splits(p, M, splits_arg > 0 ? splits_arg : 512 / tiles);
        p.prof_class = CE_PROF_GEMM_TN2;
    } else {
        // M split by a cost model fitted to tools/bench_tn_group.py (us): a workgroup spends 1.7 per 64-row contraction
        // tile + 3 of prologue; rounds of 256 workgroups; only the LAST round's epilogue is exposed -- 0.20 per tile with
        // float atomics (256 KB at 1.3 TB/s chip-wide), 0.105 as a plain read-modify-write when nothing is split
        auto cost = [&](int sp) {
            const long wgs = (long)tiles * sp;
            const long rounds = (wgs + 255) / 256;
            const long tail = wgs - (rounds - 1) * 256;
            return rounds * (div_up(m_tiles, sp) * 1.7 + 3.0) + tail * (sp == 1 ? 0.105 : 0.20);
        };
        int sp = 1;
        if (splits_arg > 0) sp = splits_arg;
        else if (knobs.force_splits > 0) sp = knobs.force_splits;
        else {
            double best = cost(1);
            for (int c = 2; c <= 16 && c <= m_tiles && (long)tiles * c <= 256; ++c)     // split only within one resident round:
                if (cost(c) < best) { best = cost(c); sp = c; }                        // every split tile costs atomic bandwidth
        }
        set_splits(p, M, sp);
        // 48-row stages x 3 slots (default; in the step 993 TF/s) or 32-row stages x 4 slots (CE_TN3_ROWS=32: 935): one
        // stage less in flight costs nothing (prefetch depth 2 = depth 3 above), a third fewer barriers per FLOP pays
        p.rows = knobs.rows == 32 ? 32 : 48;
        p.stages = p.rows == 48 ? 3 : 4;
        p.form = knobs.loader_waves ? TN_V3LW : TN_V3;      // loader-wave form: 1127 -> 1188 TF/s in the step
        p.lds_bytes = tn_plan_lds_256(p.rows, p.stages);
        // overwrite: out = product.  Unsplit 256x256 tiles store their accumulators; every other form (split tiles, the
        // 128x128 kernels) has the outputs zero-filled first and accumulates as usual.
        p.kernel_overwrites = overwrite && p.splits == 1;
        p.prof_class = CE_PROF_GEMM_TN;
    }
    p.zero_fill_first = overwrite && !p.kernel_overwrites;
    p.block = TN_PLAN_BLOCK[p.form];
    p.workgroups = tiles * p.splits;
    return p;
}

// A launch of T unsplit tiles takes ceil(T / slots) rounds of the chip and every round costs a full tile time, so the cuts
// minimise the total number of rounds, then the number of launches: a small dynamic programme over the blocks.
int tn_group_cuts(int n_blocks, int width, int M, long extra_tiles, int force_group, int* sizes_out) {
    const int n = n_blocks;
    // The one case this function defines that the programme it came from did not: a forced group above the 8 blocks one
    // launch takes left a range of more than 8 blocks without any admissible group (cost -1, `take` never written).
    if (force_group > TN_GROUP_MAX_BLOCKS) force_group = TN_GROUP_MAX_BLOCKS;
    const long t = 12 * tn_problem_tiles(M, width, width);     // qkv 3 + out-projection 1 + c_fc 4 + c_proj 4
    const long slots = tn_round_slots(M, width, width);
    long cost[TN_CUT_MAX_BLOCKS + 1];
    int take[TN_CUT_MAX_BLOCKS + 1];
    cost[0] = 0;
    for (int k = 1; k <= n; ++k) {                               // k blocks, counted from the BOTTOM of the range
        cost[k] = -1;
        for (int g = 1; g <= TN_GROUP_MAX_BLOCKS && g <= k; ++g) {     // the topmost group of those k has g blocks
            if (force_group >= 1 && g != force_group && g != k) continue;
            const long tiles = g * t + (k == n ? extra_tiles : 0);   // the group that starts the range inherits the queue
            const long c = cost[k - g] + (tiles + slots - 1) / slots * 1000 + 1;   // rounds first, then fewer launches
            if (cost[k] < 0 || c < cost[k]) { cost[k] = c; take[k] = g; }
        }
    }
    int groups = 0;
    for (int k = n; k > 0; k -= take[k]) sizes_out[groups++] = take[k];
    return groups;
}
