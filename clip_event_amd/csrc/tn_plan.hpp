// Launch policy of the TN (weight-gradient) GEMM family (gemm.hip) and of the tower's grouping of blocks into TN launches
// (tower.cpp): which kernel, how many M splits, which grid, overwrite or zero-fill, where to cut.  Plain C++17: no HIP call,
// no global, no allocation, so it runs (and is tested, tests/test_tn_plan_cpu.py) without a GPU.
#pragma once
#include "../../include/clip_event_hip.h"

// the values of ce_tn_plan.form
enum TNForm {
    TN_V1 = 0,      // gemm_tn_kernel: 128 x 128, register staged, one launch per problem
    TN_V2 = 1,      // gemm_tn2_kernel: 128 x 128, LDS-DMA, two workgroups per CU
    TN_V3 = 2,      // gemm_tn3_kernel<rows, stages>: 256 x 256 ring, one workgroup per CU
    TN_V3LW = 3     // gemm_tn3lw_kernel<rows, stages>: its loader-wave form
};

// block size and dynamic LDS bytes of each form (gemm.hip checks them against the kernels' own constants)
constexpr int TN_PLAN_BLOCK[4] = {256, 256, 1024, 768};
constexpr int TN_PLAN_LDS_128 = 65536;                       // v2; v1 pads its rows:
constexpr int TN_PLAN_LDS_V1 = 81920;
constexpr int tn_plan_lds_256(int rows, int stages) { return stages * rows * 1024; }   // v3: 3 x 48 KiB or 4 x 32 KiB

constexpr int TN_PLAN_BM = 64;            // rows of one contraction tile: an M split is a whole number of them
constexpr int TN_PLAN_MIN_M_256 = 2048;   // the 256 x 256 kernels' 64 KB prologue pays from this contraction length

// The shape rule alone (whatever CE_GEMM_TN says): 256 x 256 tiles, one workgroup per CU, when the problem is a multiple of
// 256 both ways and the contraction is long enough; 128 x 128 tiles, two workgroups per CU, otherwise.
constexpr bool tn_tiles_256(int M, int Nn, int Kk) { return M >= TN_PLAN_MIN_M_256 && Nn % 256 == 0 && Kk % 256 == 0; }
// tiles the problem contributes to a launch
constexpr long tn_problem_tiles(int M, int Nn, int Kk) {
    return tn_tiles_256(M, Nn, Kk) ? (long)(Nn / 256) * (Kk / 256) : (long)((Nn + 127) / 128) * ((Kk + 127) / 128);
}
// workgroups the chip holds at once (one round)
constexpr int tn_round_slots(int M, int Nn, int Kk) { return tn_tiles_256(M, Nn, Kk) ? 256 : 512; }

// The environment's switches (tuning / tests), as written: tn_plan applies the parsing rules.
struct TNKnobs : ce_tn_knobs {
    constexpr TNKnobs() : ce_tn_knobs{3, 0, 3, 48, 1} {}
    constexpr TNKnobs(const ce_tn_knobs& k) : ce_tn_knobs(k) {}
};
TNKnobs tn_knobs_from_env();              // the one place that reads CE_GEMM_TN and CE_TN3_*
const TNKnobs& tn_process_knobs();        // runtime.cpp: tn_knobs_from_env(), once per process

using TNPlan = ce_tn_plan;

// count problems [Nn[i], Kk[i]] sharing the contraction length M; splits_arg > 0: the caller's M split
TNPlan tn_plan(int M, int count, const int* Nn, const int* Kk, int splits_arg, bool overwrite, const TNKnobs& knobs);

constexpr int TN_CUT_MAX_BLOCKS = 64;     // blocks tn_group_cuts takes
constexpr int TN_GROUP_MAX_BLOCKS = 8;    // blocks per grouped launch (x 4 problems <= CE_TN_MAX_GROUP)

// Cuts n_blocks residual blocks of `width` (four weight gradients each, queued top-down) into grouped launches; extra_tiles
// are already queued and go out with the first group.  force_group >= 1: groups of that many blocks.  Writes the group sizes
// top-down and returns their number.
int tn_group_cuts(int n_blocks, int width, int M, long extra_tiles, int force_group, int* sizes_out);
