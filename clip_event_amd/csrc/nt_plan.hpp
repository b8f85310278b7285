// Launch policy of the NT GEMM family (gemm.hip): which kernel, which tile heights, which grid.  Plain C++17 integer
// arithmetic: no HIP call, no global, no allocation, so it runs (and is tested, tests/test_nt_plan_cpu.py) without a GPU.
// The bf16 launcher and the e4m3 launcher on the loader-wave kernels share it.
#pragma once
#include "../../include/clip_event_hip.h"

#ifndef CE_N4_LOADERS      // loader waves of the loader-wave kernels: the same compile-time switch as gemm.hip's
#define CE_N4_LOADERS 4
#endif

// the values of ce_nt_plan.kernel
enum NTKernel {
    NT_NT128 = 0,        // gemm_nt_kernel: 128 x 128, register staged
    NT_NT256x2 = 1,      // gemm_nt256_kernel<., TM, 2>: (32 TM) x 128, 4 waves, two workgroups per CU
    NT_NT256x4 = 2,      // gemm_nt256_kernel<., TM, 4>: (32 TM) x 256, 8 waves
    NT_NT32 = 3,         // gemm_nt32_kernel: 160 x 256 x 32, two workgroups per CU
    NT_NT160_RING = 4,   // gemm_nt160_kernel: 160 x 256, three-stage ring
    NT_LW = 5,           // gemm_nt160lw_kernel<., TM>: (32 TM) x 256, loader waves, one tile per workgroup
    NT_PERSIST = 6,      // gemm_nt160p_kernel<., TM, ., TS>: its persistent form, one or two tile heights
    NT_SKINNY = 7        // gemm_nt_skinny_kernel: 64 x 64, M <= 512
};

// block size and dynamic LDS bytes of each kernel (gemm.hip checks them against the kernels' own constants)
constexpr int NT_PLAN_BLOCK[8] = {256, 256, 512, 512, 512, 64 * (8 + CE_N4_LOADERS), 64 * (8 + CE_N4_LOADERS), 512};
constexpr int NT_PLAN_LDS[8] = {65536, 73728, 139264, 53248, 159744, 159744, 159744 + 64, 139264};

struct NTShape {
    int M, N, K;
    long lda, ldb, ldo, ldo2, ldaux, ldr;
};

// Everything the setters and the environment can change about the policy.
struct NTKnobs {
    int force_tile = 0;      // ce_gemm_nt_tune(): 0 auto, else the forced tile code (include/clip_event_hip.h)
    int force_chunk = -2;    // ce_gemm_nt_tune(1000 + ...): walk of the persistent kernel (-2: env_chunk)
    // CU budget (ce_gemm_set_cu_budget / CE_GEMM_CUS, default 256 = the whole chip).  Every NT kernel here puts ONE 156 KiB
    // workgroup on a CU and sizes its grid to fill the chip exactly once (one-round launches: 226-240 tiles; persistent
    // launches: 256 workgroups), so a single CU held by another stream's kernel -- an RCCL channel during a gradient
    // all-reduce -- leaves one workgroup without a home until a whole tile list has finished: measured with a 1-CU "hog"
    // (ce_cu_hog) every such launch takes 1.6-1.75x as long.  A budget below 256 sizes the one-round and the
    // persistent grids for that many CUs, so that the rest may be taken.
    int cus = 256;
    // ce_gemm_set_dynamic_tiles / CE_NT_DYNAMIC: the persistent kernel's DYNAMIC tile list (off by default)
    int dynamic = 0;
    // XCD-owned walk (persist_walk): CE_NT_CHUNK = 0 (default) the launch-wide walk, -1 = chunks of tiles_m / 8 row panels,
    // n > 0 = chunks of n.  OFF: with sc1 output stores it takes the c_fc GEMM's fetch from 166.8 to 68.3 MB (algorithmic
    // 24.4; the floor of any 8-way partition is 57) and qkv's from 105.5 to 53.5 MB (profiles/r03_pmc_fetch_xcd_walk.txt)
    // and the kernels do not get faster: BIAS_GELU 1.30 -> 1.32 ms/step, qkv 0.945 -> 0.96; with plain stores 1.37 -> 1.46
    // and 0.92 -> 1.00.  These launches are not bound by operand re-fetch.
    int env_chunk = 0;
    // CE_NT_PGRID workgroups walk the persistent tile list (0: one per budgeted CU).  More, shorter lists = finer scheduling
    // granularity when some CUs are held by another stream's kernels (or by RCCL): a workgroup that starts late then delays
    // the launch by a shorter list.
    int env_pgrid = 0;
    int env_mixed = 1;       // CE_NT_MIXED=0 switches the two tile heights off

    int budget() const { return cus >= 32 && cus <= 256 ? cus : 256; }
};

struct NTPlan {
    bool taken = true;           // false (fp8 only): not a shape the loader-wave kernels take; the caller falls back
    NTKernel kernel = NT_NT128;
    int tm = 0, ts = 0;          // tile height in 32-row units; ts > 0: the height of the panels after the first tall_panels
    int tiles_m = 0, tiles_n = 0, tall_panels = 0, tile_chunk = 0;      // the NTArgs tiling fields
    int workgroups = 0, block = 0, lds_bytes = 0;
    bool wants_tile_queue = false;    // persistent kernel: hand its tiles out through a device counter (NTArgs.tile_queue)
    bool needs_colsum_pass = false;   // the 128^2 kernel has no fused column sums: GELUGRAD's come from a second launch
    int family = 0;              // profiler class offset (CE_PROF_GEMM_NT0 + ...), 0..7
};

// epilogues for which the persistent kernel is also built with two tile heights
constexpr bool nt_two_heights(int epi) {
    return epi == CE_EPI_BIAS_GELU || epi == CE_EPI_GELUGRAD_BF16 || epi == CE_EPI_BIAS_BF16 || epi == CE_EPI_BF16 ||
           epi == CE_EPI_BIAS_RESID_F16 || epi == CE_EPI_BIAS_RESID_F32 || epi == CE_EPI_BIAS_QGELU_BF16;
}

NTPlan nt_plan(const NTShape& s, int epilogue, bool fp8, const NTKnobs& knobs);
