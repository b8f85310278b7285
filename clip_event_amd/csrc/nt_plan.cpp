// Launch policy of the NT GEMM family: see nt_plan.hpp.
#include "nt_plan.hpp"

#include <algorithm>

namespace {

inline long div_up(long a, long b) { return (a + b - 1) / b; }

// Tile-variant cost model, fitted to tools/tune_nt.py sweeps (M 8k..20k, both towers' N/K; unit = 0.137 us at
// K = 512, scales with K): one round of 32*TM-row tiles on the budgeted CUs costs 28 + 10*TM (the K loop is
// LDS-read bound: a fixed share for the 256-column B fragments plus TM A fragments per k-step); the
// 160x256x32 kernel keeps two workgroups per CU: a co-resident pair costs 146, a lone one 78.
inline long nt256_cost(long tiles, int tm, long cus) { return div_up(tiles, cus) * (28 + 10 * tm); }
inline long nt32_cost(long tiles) {
    const long n = div_up(tiles, 256);
    return (n / 2) * 146 + (n % 2) * 78;
}

// Persistent kernel, one tile height: the height in tm_max .. 3 with the cheapest longest per-workgroup tile list over G
// workgroups -- rows of tile work + ~48 rows' worth of epilogue per tile (the taller height wins a tie).
struct Height { int tm; long cost; };
inline Height cheapest_height(long M, long tiles_n, long G, int tm_max) {
    Height best{tm_max, -1};
    for (int tm = tm_max; tm >= 3; --tm) {
        const long cost = div_up(div_up(M, 32 * tm) * tiles_n, G) * (32 * tm + 48);
        if (best.cost < 0 || cost < best.cost) best = {tm, cost};
    }
    return best;
}

// One-round loader-wave kernel: the shortest tile whose launch still fits one round of the budgeted CUs (the text tower's
// N = 512 has two tile columns).
inline int shortest_one_round_height(long M, long tiles_n, long cus) {
    int ltm = 5;
    for (int tm = 4; tm >= 3; --tm)
        if (div_up(M, 32 * tm) * tiles_n <= cus) ltm = tm;
    return ltm;
}

// Two tile heights for one persistent launch (gemm_nt160p_kernel<EPI, TM, F8, TS>): n_tall row panels of 32 TM rows, the rest in panels
// of 32 TS, chosen so that the longest per-workgroup list (tall tiles first, round-robin over G workgroups) is shortest under the
// launch policy's cost model (32 tm + 48 per tile).  `uniform` = the best single height's cost; true when a split beats it by >=
// min_gain per cent.
inline bool two_height_plan(long M, long tn, long G, int TM, long uniform, int min_gain, long& b_tall, long& b_short, int& b_ts) {
    const long ct = 32 * TM + 48;
    auto span = [&](long n_tall, int ts, long n_short) {      // cost of the longest list
        const long T = n_tall * tn, S = n_short * tn, q = T / G, r = T % G;
        auto shorts = [&](long d) { return d < S ? (S - 1 - d) / G + 1 : 0; };   // short tiles of the workgroup d places behind r
        const long cs = 32 * ts + 48;
        long worst = q * ct + shorts(0) * cs;                  // workgroup r: q tall tiles, the most short ones
        if (r > 0) worst = std::max(worst, (q + 1) * ct + shorts(G - r) * cs);   // workgroup 0: q + 1 tall
        return worst;
    };
    long best = uniform;
    b_tall = -1; b_short = 0; b_ts = 0;
    for (int ts = TM - 1; ts >= 1; --ts)
        for (long n_tall = M / (32 * TM); n_tall >= 1; --n_tall) {
            const long rest = M - n_tall * 32 * TM;
            if (rest <= 0) continue;
            const long n_short = (rest + 32 * ts - 1) / (32 * ts);
            const long c = span(n_tall, ts, n_short);
            if (c < best || (c == best && b_tall < 0)) { best = c; b_tall = n_tall; b_short = n_short; b_ts = ts; }
        }
    return b_tall > 0 && best * 100 <= uniform * (100 - min_gain);
}

constexpr int epi_out_bytes(int epi) {
    return (epi == CE_EPI_F32 || epi == CE_EPI_BIAS_F32 || epi == CE_EPI_BIAS_RESID_F32) ? 4 : 2;
}

}  // namespace

NTPlan nt_plan(const NTShape& s, int epilogue, bool fp8, const NTKnobs& knobs) {
    NTPlan p;
    const long M = s.M;
    const bool aligned8 = s.N % 8 == 0 && s.ldo % 8 == 0 && s.ldo2 % 8 == 0 && s.ldaux % 8 == 0;
    // the loader-wave kernels address their epilogue operands with 32-bit buffer offsets (EpiBuf): every one must span < 2 GiB
    const auto span = [&](long ld, long esz) { return M * ld * esz; };
    const bool fits31 = span(s.ldo, epi_out_bytes(epilogue)) < (1l << 31) && span(s.ldo2, 2) < (1l << 31) &&
                        span(s.ldaux, 2) < (1l << 31) && span(s.ldr, 4) < (1l << 31);

    // The e4m3 path has the two loader-wave families only, so a shape they do not take is "not taken".  Where it differs
    // from the bf16 path below, each difference is one of these values:
    //   - forced codes and the forced walk of ce_gemm_nt_tune, the chunked walk, CE_NT_PGRID and the tile queue are bf16 only;
    //   - the persistent heights are {4, 3}: 160-row tiles spill in the e4m3 form (32-byte fragments).
    if (fp8) {
        p.taken = s.M >= 1024 && s.N >= 256 && s.K % 128 == 0 && s.K >= 256 && aligned8 && s.lda % 16 == 0 && s.ldb % 16 == 0 && fits31 &&
                  epilogue != CE_EPI_F32 && epilogue != CE_EPI_BIAS_F32;      // (the two epilogues without an e4m3 form)
        if (!p.taken) return p;
    }
    const int f = fp8 ? 0 : knobs.force_tile;
    const int tall_tm = fp8 ? 4 : 5;
    const long cus = knobs.budget();
    const long pgrid = !fp8 && knobs.env_pgrid > 0 ? knobs.env_pgrid : cus;
    const int walk = fp8 ? 0 : (knobs.force_chunk > -2 ? knobs.force_chunk : knobs.env_chunk);
    const bool dynamic = !fp8 && knobs.dynamic;
    // `kernel` on tiles of 32 tm x cols, one workgroup per tile (the e4m3 launches report one profiler family, 4)
    const auto tiled = [&](NTKernel kernel, int family, int tm, int cols) {
        p.kernel = kernel;
        p.family = fp8 ? 4 : family;
        p.tm = tm;
        p.tiles_m = (int)div_up(M, 32 * tm);
        p.tiles_n = (int)div_up(s.N, cols);
        p.workgroups = p.tiles_m * p.tiles_n;
        p.block = NT_PLAN_BLOCK[kernel];
        p.lds_bytes = NT_PLAN_LDS[kernel];
        return p;
    };

    if (!(s.K % 64 == 0 && aligned8 && s.M >= 1024 && s.N >= 256)) {
        if (s.M <= 512 && s.K % 256 == 0 && aligned8 && s.ldr % 4 == 0) return tiled(NT_SKINNY, 7, 2, 64);
        p.needs_colsum_pass = epilogue == CE_EPI_GELUGRAD_BF16;
        return tiled(NT_NT128, 0, 4, 128);
    }

    // the 64-column-K families, 256 output columns wide (NT256x2: 128)
    const long tiles_n = div_up(s.N, 256);
    // 8-wave tile: the height by wave quantisation, cost ~ (rounds over the CUs) x (cost of one tile-round)
    int best = 8;
    long best_cost = -1;
    if (f >= 3 && f <= 8) {
        best = f;
    } else {
        for (int tm = 8; tm >= 3; --tm) {
            const long cost = nt256_cost(div_up(M, 32 * tm) * tiles_n, tm, cus);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = tm; }
        }
    }
    const bool use32 = f == 32 || (f == 0 && !fp8 && nt32_cost(div_up(M, 160) * tiles_n) < best_cost);
    // Where the cost model picks a 256-column tile with one workgroup per CU and the tiles fit one resident round
    // (N = width GEMMs: 240 tiles of 160x256), use the loader-wave kernel (gemm_nt160lw_kernel: -2.7 % on the step
    // against the 160x128 pair, which was itself 0.5-2 % ahead of the plain 8-wave tile because a workgroup of
    // the OTHER tower's GEMM could share the CU).  Where an epilogue operand spans 2 GiB or more the 160x128 pair takes its place.
    const bool one_resident_round = div_up(M, 160) * div_up(s.N, 128) <= 2 * cus;
    const bool half = f == 104 || (f >= 203 && f <= 205) || (f == 0 && one_resident_round && !use32);
    const bool lw = fits31 && (f == 161 || (half && f == 0));
    // multi-round launches: the persistent loader-wave kernel, for the light epilogues (qkv forward: 726 -> 810 TF/s) and
    // for the GELU epilogues (as kernels about equal to the two-workgroup 160x256x32 kernel since their epilogues lost the
    // division and the backward's transcendentals): B = 256 step 14.15 -> 14.00 (light) -> 13.96 ms (both), config 4 at
    // B = 64 32.3 -> 31.9 -> 31.5 ms.
    // (A two-group "ping-pong" persistent kernel -- 128x256x64 tiles, one group of four waves multiplying while the other
    //  issues the ring's LDS-DMAs and works through the previous tile's epilogue -- was built, parity-tested and measured in
    //  round 3: BIAS_GELU 63.1 vs 55.4 us per launch, qkv 41.0 vs 35.3, step 12.77 vs 12.40 ms, slower in both versions; it
    //  was removed in round 4.  DESIGN 6b keeps the post-mortem.)
    const bool pers = !lw && fits31 && s.K >= 128 && ((f >= 162 && f <= 165) || (f == 0 && !half));

    if (pers) {
        const int ptm = f >= 163 && f <= 165 ? f - 160 : cheapest_height(M, tiles_n, cus, tall_tm).tm;
        tiled(NT_PERSIST, 6, ptm, 256);
        p.tile_chunk = walk < 0 ? (p.tiles_m >= 8 ? p.tiles_m / 8 : 1) : walk;   // floor: a chunk never spans three XCDs
        // TWO TILE HEIGHTS: n_tall row panels of 32 tall_tm rows, the rest in panels of 32 ts, chosen so that the longest
        // per-workgroup list (tall tiles first, round-robin over the grid) is shortest under the same cost model; taken when
        // it beats the best single height by >= 3 %, from two tall panels' worth of rows.  12800 x 3072: 960 tiles of 160
        // rows = 3.75 rounds -> 3 rounds of 160 + one of 128.
        if (nt_two_heights(epilogue) && knobs.env_mixed && f == 0 && p.tile_chunk == 0 && M >= 64 * tall_tm) {
            const long uniform = cheapest_height(M, tiles_n, pgrid, tall_tm).cost;
            long n_tall, n_short;
            int ts;
            if (two_height_plan(M, tiles_n, pgrid, tall_tm, uniform, 3, n_tall, n_short, ts)) {
                p.tm = tall_tm;
                p.ts = ts;
                p.tall_panels = (int)n_tall;
                p.tiles_m = (int)(n_tall + n_short);
            }
        }
        const long tiles = (long)p.tiles_m * p.tiles_n;
        p.workgroups = (int)std::min(tiles, pgrid);
        // dynamic tile list: only where a workgroup walks more than one tile, with >= 3 K iterations (the fetched id is
        // published by the barrier of iteration 1 and needed from iteration nk - 2) on the launch-wide walk
        p.wants_tile_queue = dynamic && tiles > p.workgroups && s.K >= 3 * 64 && p.tile_chunk == 0;
        return p;
    }
    if (lw) return tiled(NT_LW, 5, shortest_one_round_height(M, tiles_n, cus), 256);
    // 160x128, two workgroups per CU: measured equal to the 8-wave 160x256 tile, kept as an option
    if (half) return tiled(NT_NT256x2, 1, f >= 203 && f <= 205 ? f - 200 : 5, 128);
    if (use32) return tiled(NT_NT32, 3, 5, 256);
    // three-stage ring: measured 6 % slower than the two-stage loop (the K loop is LDS-bandwidth bound, not DMA-latency
    // bound); kept as an option.  It reports the 8-wave tile's profiler family.
    if (f == 160) return tiled(NT_NT160_RING, 2, 5, 256);
    return tiled(NT_NT256x4, 2, best, 256);
}
