// Fused contrastive head at global-batch scale: scaled similarity tiles, online log-sum-exp, label pick and the
// backward from the saved log-sum-exp, WITHOUT the [B, N*K] logits matrix in HBM (336 MB at N = 4096,
// K = 5).  Replaces, for the 'ce' criterion over the batch, model_clip.py:496-521 (logits) + :633-662 (cross entropy).
//
//   loss += mean_r ( lse_r - s <q_r, k_{y_r}> ),   lse_r = log sum_c exp(s <q_r, k_c>)          q, k already L2-normalised
//   G[r,c] = g/n (exp(s <q_r,k_c> - lse_r) - [c == y_r]);  dq_r = s sum_c G[r,c] k_c;  dk_c = s sum_r G[r,c] q_r;
//   dlogit_scale = sum G[r,c] s <q_r,k_c>
//
// fp32 throughout, products on the fp32 matrix instruction v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains, 16x below the
// bf16 rate but 3x an LDS-tiled VALU kernel; MI355X_MICROARCH.md "Matrix cores").  One kernel skeleton, three modes:
// a workgroup (4 waves) keeps one 32-row RESIDENT block in LDS and sweeps 32-row STREAMED blocks of the other matrix.
//   * similarity tile: S^T[i][j] = <streamed_i, resident_j>, the streamed rows as the A operand straight from global
//     memory (16 B per lane, L1-resident over the four MFMAs that consume them), the resident rows as the B operand from
//     LDS (row pitch E+4 floats: conflict-free ds_read_b128).  Each wave takes a quarter of E; the four partial tiles are
//     summed through LDS.  Resident index j sits on the lane, streamed index i in the 16 accumulator registers.
//   * mode FWD (resident = queries): online max / sum per lane, partial (max, sum) per split, merged by a second tiny
//     kernel that also picks s <q_r, k_{y_r}> and adds the mean loss.
//   * modes DQ (resident = queries) / DK (resident = keys): G^T in registers is directly the B operand of the gradient
//     product  dres^T[e][j] += sum_i streamed[i][e] G^T[i][j]  (contraction over the accumulator's register index needs no
//     lane movement: cdna_hip_programming.md "An accumulator tile as the next MFMA's operand"); each wave owns a quarter of
//     E; the result leaves through an LDS transpose as whole rows (plain stores when the streamed range is not split,
//     float atomics otherwise).
//
// Two loss policies share the skeleton (template parameter LOSS).  LOSS_SOFTMAX is the above.  LOSS_SIGMOID is the pairwise
// sigmoid loss of SigLIP over queries x keys, one direction:
//   x[r,c] = s <q_r, k_c> + b,  z[r,c] = +1 if c == y_r else -1,  loss = -(1/nq) sum_r sum_c log sigma(z x)
//   G[r,c] = -(g/nq) z sigma(-z x);  dq, dk as above;  db = sum G;  dlogit_scale = sum G (x - b)
// Every pair is an independent term: no row statistic, no merge by maximum, nothing saved for the backward.  Three sites differ:
//   * FWD sums stable softplus terms, each wave taking 16 / NW of the tile's accumulator rows (the softmax FWD lets every wave
//     reduce the whole tile); one partial per workgroup goes to a workspace and a one-workgroup kernel adds the partials in a
//     fixed order and applies 1/nq: the loss is bit-identical from run to run (no float atomics on it).
//   * G in DQ / DK; qinfo carries the label only.
//   * zero-padded tile positions are NOT neutral (softplus(0) = log 2): every term is masked by row and column validity.
// LOSS_DISTILL (cross entropy against a teacher's softmax; the entry points at the end of the file compose it from sweeps):
// FWD leaves the log-sum-exp partials only; in DQ / DK G = c exp(x - lse) with no label, the gradient product streams a VALUE
// matrix of its own width (HeadArgs::val) in place of the streamed operand, and the write has a scale of its own.
// Group-id targets (several positives per query): every query source row and every key row carries a 64-bit id, and key c is a
// positive of query r when the ids are equal and not negative.  LOSS_MULTIPOS is the softmax loss against the uniform
// distribution over the row's positives P(r), n_r = |P(r)|:
//   loss = (1/nq) sum_{n_r > 0} (lse_r - (1/n_r) sum_{c in P(r)} x[r,c]),   G[r,c] = g/nq (exp(x - lse_r) - [c in P(r)] / n_r)
// FWD counts the positives and sums their x in the SAME sweep (partials (max, sum, count, possum) per split), the merge leaves
// lse and invpos = 1 / n_r (0: a row without positives, which G then skips).  LOSS_SIGMOID_GROUP is LOSS_SIGMOID with z = +1
// on every positive.  The ids of the 32 streamed rows sit in LDS (qinfo) in every mode; a padded streamed row has id -1 and a
// padded resident lane id -1, so neither is ever a positive.
#include <stdlib.h>

#include <mutex>

#include "common.hpp"
#include "head_sweep.hpp"
#include "../../include/clip_event_hip.h"

using namespace head_sweep;

namespace {

enum { MODE_FWD = 0, MODE_DQ = 1, MODE_DK = 2 };
enum { LOSS_SOFTMAX = 0, LOSS_SIGMOID = 1, LOSS_DISTILL = 2, LOSS_MULTIPOS = 3, LOSS_SIGMOID_GROUP = 4 };
constexpr bool is_sigmoid(int loss) { return loss == LOSS_SIGMOID || loss == LOSS_SIGMOID_GROUP; }
constexpr bool is_group(int loss) { return loss == LOSS_MULTIPOS || loss == LOSS_SIGMOID_GROUP; }

struct HeadArgs {
    const float* res; long ldres; int nres;       // resident matrix (queries for FWD / DQ, keys for DK)
    const float* str; long ldstr; int nstr;       // streamed matrix
    const long* sel;                              // query row gather (nullable): query r = row sel[r] of its matrix
    const long* labels;                           // key index per query SOURCE row (labels[sel[r]])
    const float* lse;                             // [nq]            (DQ / DK; LOSS_DISTILL: [nq][2] = (max, log sum), see lse_merge_kernel)
    const float* logit_scale;
    const float* grad;                            // upstream scalar (DQ / DK)
    float* part;                                  // FWD: [splits][nq][2] partial (max, sum)
    float* dres;                                  // DQ / DK: gradient of the resident matrix [rows, E] (+=)
    float* dls;                                   // DQ: logit_scale gradient (+=)
    int E, nq, splits, blocks_per_split;
    // LOSS_SIGMOID only
    const float* logit_bias;
    float* dbias;                                 // DQ: logit_bias gradient (+=)
    float* loss_part;                             // FWD: [splits][row blocks] loss partial of each workgroup
    // LOSS_DISTILL only
    const float* val; long ldval; int Eval;       // DQ / DK: value matrix of the gradient product (rows gathered as the streamed rows)
    const long* osel;                             // DQ: row of dres that resident r adds to (nullable: row r)
    const float* out_logit_scale;                 // DQ / DK: the write multiplies by exp(*out_logit_scale) (nullable: by 1)
    const float* sub;                             // DQ: [nres, Eval], the write also subtracts c exp(*out_logit_scale) sub[r] (nullable)
    const float* dot; long lddot;                 // DQ: part[split][r] = <dot[sel[r]], this split's share of output row r> (nullable)
    float csign;                                  // c = csign * (grad ? *grad / nq : 1)
    // group-id targets only (LOSS_MULTIPOS: part is [splits][nq][4] = (max, sum, count, possum))
    const long* qgroup;                           // id per query SOURCE row (qgroup[sel[r]])
    const long* kgroup;                           // id per key row
    const float* invpos;                          // [nq] 1 / n_r, 0 for a row without positives (DQ / DK of LOSS_MULTIPOS)
};

// log(1 + e) for 0 <= e <= 1, accurate where e is tiny (with the usual bias near -10 a negative pair's term is ~ 4.5e-5 and
// log(1.f + e) alone keeps four of its digits): u = fl(1 + e) carries the rounding of the sum, and log(u) * e / (u - 1) takes it
// out again (the classic log1p correction); u == 1 leaves e itself.  One v_log_f32, one v_rcp_f32.
__device__ __forceinline__ float log1p_unit(float e) {
    const float u = 1.f + e, d = u - 1.f;
    return d == 0.f ? e : __logf(u) * (e * __frcp_rn(d));
}
// -log sigma(y) = softplus(-y) = max(-y, 0) + log1p(exp(-|y|)): exp never sees a positive argument
__device__ __forceinline__ float neg_log_sigmoid(float y) { return fmaxf(-y, 0.f) + log1p_unit(__expf(-fabsf(y))); }
// sigma(-y) = e / (1 + e) for y >= 0, 1 / (1 + e) for y < 0, e = exp(-|y|)
__device__ __forceinline__ float sigmoid_neg(float y) {
    const float e = __expf(-fabsf(y));
    return (y >= 0.f ? e : 1.f) * __frcp_rn(1.f + e);
}

// NW waves per workgroup: 4 (E a multiple of 128) or 8 (E a multiple of 256: two waves per SIMD cover the global operand
// loads that feed the MFMAs; each wave then owns an eighth of E)
template <int MODE, int NW, int LOSS = LOSS_SOFTMAX>
__global__ __launch_bounds__(64 * NW) void infonce_kernel(HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int E = a.E, pitch = E + 4;
    float* res_l = reinterpret_cast<float*>(smem);                       // [32][E+4]
    float* part_l = res_l + HB * pitch;                                  // [NW][32][33]: partial tiles / output transpose
    float* qinfo = part_l + NW * HB * 33;                                 // [2][32]: lse, label (as float bits) of the streamed queries (DK)
                                                                          //          (sigmoid: label only; FWD: the waves' loss sums)
    // group ids: the 64-bit ids of the 32 streamed rows, every mode -- behind [2][32] (lse, invpos; DK) for LOSS_MULTIPOS
    long* const sid = reinterpret_cast<long*>(qinfo + (LOSS == LOSS_MULTIPOS ? 2 * HB : 0));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * HB;
    // distillation: the correctly rounded exp.  __expf(log 100) is off by 2e-7 of itself (the rounding of x log2(e)), which moves
    // logits near 40 by 1e-5, and the teacher's scale reshapes the target distribution
    const float scale = (LOSS == LOSS_DISTILL) ? expf(*a.logit_scale) : __expf(*a.logit_scale);

    // ---- resident block -> LDS (gathered through sel when the residents are queries) ----
    load_residents<NW>(a.res, a.ldres, a.nres, MODE != MODE_DK ? a.sel : nullptr, E, res_l, r0, tid);
    // per-lane facts about resident row j
    const bool jvalid = r0 + j < a.nres;
    long jsrc = 0, jlabel = -1;
    long jgroup = -1;                                     // group id of resident row j (a query's, or in DK a key's)
    float jlse = 0.f, jlse_lo = 0.f, jinv = 0.f;
    if (MODE != MODE_DK && jvalid) {
        jsrc = a.sel ? a.sel[r0 + j] : (long)(r0 + j);
        if (LOSS != LOSS_DISTILL && !is_group(LOSS)) jlabel = a.labels[jsrc];
        if (is_group(LOSS)) jgroup = a.qgroup[jsrc];
        if (MODE == MODE_DQ && (LOSS == LOSS_SOFTMAX || LOSS == LOSS_MULTIPOS)) jlse = a.lse[r0 + j];
        if (MODE == MODE_DQ && LOSS == LOSS_MULTIPOS) jinv = a.invpos[r0 + j];
        if (MODE == MODE_DQ && LOSS == LOSS_DISTILL) {
            jlse = a.lse[2 * (r0 + j)];
            jlse_lo = a.lse[2 * (r0 + j) + 1];
        }
    }
    if (is_group(LOSS) && MODE == MODE_DK && jvalid) jgroup = a.kgroup[r0 + j];
    // equal ids have the same sign: "both ids >= 0" is a fact about the resident row alone (false for a padded lane, id -1)
    const bool jlive = jgroup >= 0;
    const float bias = is_sigmoid(LOSS) ? *a.logit_bias : 0.f;
    const float coef = (MODE == MODE_FWD) ? 0.f
                       : (LOSS == LOSS_DISTILL) ? a.csign * (a.grad ? *a.grad / (float)a.nq : 1.f) : (*a.grad / (float)a.nq);
    __syncthreads();

    float run_m = -INFINITY, run_l = 0.f;                 // FWD: online statistics of query j over this split
    float dls_acc = 0.f;
    float loss_acc = 0.f, dbias_acc = 0.f;                // sigmoid: FWD loss terms / DQ bias gradient of this lane
    float pos_cnt = 0.f, pos_sum = 0.f;                   // LOSS_MULTIPOS FWD: positives of query j among this lane's rows, and their x
    constexpr int GT = 32 / NW;                           // gradient accumulators: up to 1024 / NW / 32 e-tiles of 32 per wave
    f32x16 gacc[MODE == MODE_FWD ? 1 : GT];
    // the gradient product runs over the value matrix: the streamed matrix itself, or (distillation) one of another width
    const int EV = (LOSS == LOSS_DISTILL && MODE != MODE_FWD) ? a.Eval : E;
    const float* const vmat = (LOSS == LOSS_DISTILL && MODE != MODE_FWD) ? a.val : a.str;
    const long ldv = (LOSS == LOSS_DISTILL && MODE != MODE_FWD) ? a.ldval : a.ldstr;
    const int etiles = EV / (32 * NW);                    // e-tiles of 32 columns per wave (EV/NW columns per wave)
    const int ev_lo = wave * (EV / NW);
    if (MODE != MODE_FWD) {
#pragma unroll
        for (int t = 0; t < GT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) gacc[t][r] = 0.f;
    }
    const int e_lo = wave * (E / NW);

    const int sb0 = blockIdx.y * a.blocks_per_split;
    const int sb1 = min(sb0 + a.blocks_per_split, (a.nstr + HB - 1) / HB);
    for (int sb = sb0; sb < sb1; ++sb) {
        const int c0 = sb * HB;
        // streamed row of this lane for the similarity A operand: i = lane & 31
        const bool ivalid = c0 + j < a.nstr;
        long isrc = c0 + j;
        if (MODE == MODE_DK && a.sel && ivalid) isrc = a.sel[c0 + j];
        const float* arow = a.str + isrc * a.ldstr + e_lo + 4 * h;
        // ---- similarity tile, this wave's quarter of E ----
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* brow = res_l + j * pitch + e_lo + 4 * h;
#pragma unroll 4
        for (int u = 0; u < E / (8 * NW); ++u) {
            f32x4 av = {0.f, 0.f, 0.f, 0.f};
            if (ivalid) av = *reinterpret_cast<const f32x4*>(arow + 8 * u);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(brow + 8 * u);
#pragma unroll
            for (int x = 0; x < 4; ++x) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[x], bv[x], acc, 0, 0, 0);
        }
        // ---- sum the four partial tiles through LDS: part_l[w][row i][col j] ----
        __syncthreads();          // previous iteration's readers of part_l / qinfo writers are done
#pragma unroll
        for (int r = 0; r < 16; ++r) part_l[(wave * HB + row_of(r, h)) * 33 + j] = acc[r];
        if (MODE == MODE_DK && tid < HB) {                // lse / label of the 32 streamed queries
            const bool v = c0 + tid < a.nstr;
            const long src = v ? (a.sel ? a.sel[c0 + tid] : (long)(c0 + tid)) : 0;
            if (LOSS == LOSS_SOFTMAX) qinfo[tid] = v ? a.lse[c0 + tid] : 0.f;
            if (LOSS == LOSS_SOFTMAX || LOSS == LOSS_SIGMOID)
                qinfo[HB + tid] = v ? (float)a.labels[src] : -1.f;                                // key indices < 2^24: exact in fp32
            if (LOSS == LOSS_MULTIPOS) {
                qinfo[tid] = v ? a.lse[c0 + tid] : 0.f;
                qinfo[HB + tid] = v ? a.invpos[c0 + tid] : 0.f;
            }
            if (is_group(LOSS)) sid[tid] = v ? a.qgroup[src] : -1L;
            if (LOSS == LOSS_DISTILL) {                   // no label: the second slot carries the low part of the log-sum-exp
                qinfo[tid] = v ? a.lse[2 * (c0 + tid)] : 0.f;
                qinfo[HB + tid] = v ? a.lse[2 * (c0 + tid) + 1] : 0.f;
            }
        }
        if (is_group(LOSS) && MODE != MODE_DK && tid < HB)       // ids of the 32 streamed keys (-1 behind nk: never a positive)
            sid[tid] = c0 + tid < a.nstr ? a.kgroup[c0 + tid] : -1L;
        __syncthreads();
        if (MODE == MODE_FWD && is_sigmoid(LOSS)) {
            // pairs are independent: wave w takes the accumulator rows r = w * 16 / NW ... of every lane's column
            constexpr int RPW = 16 / NW;
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr) {
                const int i = row_of(wave * RPW + rr, h);
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) t += part_l[(w * HB + i) * 33 + j];
                const float x = scale * t + bias;
                // a zero-padded row or column would add softplus(0) = log 2
                if (jvalid && c0 + i < a.nstr) {
                    const bool pos = is_group(LOSS) ? (jlive && sid[i] == jgroup) : (long)(c0 + i) == jlabel;
                    loss_acc += neg_log_sigmoid(pos ? x : -x);
                }
            }
            continue;
        }
        float S[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = row_of(r, h);
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += part_l[(w * HB + i) * 33 + j];
            S[r] = scale * t;
        }
        if (MODE == MODE_FWD) {
            float mx = run_m;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (c0 + row_of(r, h) < a.nstr) mx = fmaxf(mx, S[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (c0 + row_of(r, h) < a.nstr) sum += __expf(S[r] - mx);
            sum += __shfl_xor(sum, 32, 64);
            run_l = run_l * __expf(run_m - mx) + sum;      // run_m = -inf on the first block: exp(-inf) = 0
            run_m = mx;
            if (LOSS == LOSS_MULTIPOS) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = row_of(r, h);
                    if (jlive && c0 + i < a.nstr && sid[i] == jgroup) {
                        pos_cnt += 1.f;
                        pos_sum += S[r];
                    }
                }
            }
        } else {
            // G^T[i][j] for this lane's resident j and its 16 streamed rows
            float G[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = row_of(r, h);
                float g = 0.f;
                if (is_sigmoid(LOSS)) {
                    if (jvalid && c0 + i < a.nstr) {
                        const bool pos = is_group(LOSS)     ? (jlive && sid[i] == jgroup)
                                         : (MODE == MODE_DQ) ? (long)(c0 + i) == jlabel
                                                             : (float)(r0 + j) == qinfo[HB + i];
                        const float x = S[r] + bias;
                        g = (pos ? -coef : coef) * sigmoid_neg(pos ? x : -x);
                    }
                    if (MODE == MODE_DQ) dbias_acc += g;
                } else if (LOSS == LOSS_DISTILL) {                      // no label term: c softmax
                    if (jvalid && c0 + i < a.nstr)
                        g = coef * __expf((S[r] - (MODE == MODE_DQ ? jlse : qinfo[i])) - (MODE == MODE_DQ ? jlse_lo : qinfo[HB + i]));
                } else if (LOSS == LOSS_MULTIPOS) {                     // uniform over the row's positives; no positive: no row
                    const float inv = (MODE == MODE_DQ) ? jinv : qinfo[HB + i];
                    if (jvalid && c0 + i < a.nstr && inv > 0.f)
                        g = coef * (__expf(S[r] - (MODE == MODE_DQ ? jlse : qinfo[i])) - (jlive && sid[i] == jgroup ? inv : 0.f));
                } else if (MODE == MODE_DQ) {
                    if (jvalid && c0 + i < a.nstr) g = coef * (__expf(S[r] - jlse) - ((long)(c0 + i) == jlabel ? 1.f : 0.f));
                } else {
                    if (jvalid && c0 + i < a.nstr)
                        g = coef * (__expf(S[r] - qinfo[i]) - ((float)(r0 + j) == qinfo[HB + i] ? 1.f : 0.f));
                }
                G[r] = g;
                if (MODE == MODE_DQ && LOSS != LOSS_DISTILL) dls_acc += g * S[r];
            }
            // ---- gradient product: dres^T[e][j] += sum_i streamed[i][e] G^T[i][j]; A = streamed[i(r,h)][e0 + (lane&31)] ----
#pragma unroll
            for (int t = 0; t < GT; ++t) {
                if (t < etiles) {
                const int e0 = ev_lo + 32 * t + j;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = c0 + row_of(r, h);
                    float av = 0.f;
                    if (i < a.nstr) {
                        const long src = (MODE == MODE_DK && a.sel) ? a.sel[i] : (long)i;
                        av = vmat[src * ldv + e0];
                    }
                    gacc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, G[r], gacc[t], 0, 0, 0);
                }
                }
            }
        }
    }

    if (MODE == MODE_FWD && is_sigmoid(LOSS)) {
        loss_acc = wave_sum(loss_acc);
        __syncthreads();                                  // the last tile's readers of part_l are done (qinfo sits behind it)
        if (lane == 0) qinfo[wave] = loss_acc;
        __syncthreads();
        if (tid == 0) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += qinfo[w];
            a.loss_part[(long)blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
        return;
    }
    if (MODE == MODE_FWD && LOSS == LOSS_MULTIPOS) {      // every wave holds the same tile sums: wave 0 writes
        pos_cnt += __shfl_xor(pos_cnt, 32, 64);
        pos_sum += __shfl_xor(pos_sum, 32, 64);
        if (wave == 0 && h == 0 && jvalid)
            *reinterpret_cast<f32x4*>(a.part + ((long)blockIdx.y * a.nq + r0 + j) * 4) = f32x4{run_m, run_l, pos_cnt, pos_sum};
        return;
    }
    if (MODE == MODE_FWD) {
        if (wave == 0 && h == 0 && jvalid) {
            float* o = a.part + ((long)blockIdx.y * a.nq + r0 + j) * 2;
            o[0] = run_m;
            o[1] = run_l;
        }
        return;
    }
    // ---- gradient out: transpose each 32(e) x 32(j) tile through LDS, then whole 128-byte row segments ----
    if (MODE == MODE_DQ && LOSS != LOSS_DISTILL) {
        dls_acc = wave_sum(dls_acc);
        if (lane == 0 && wave == 0) atomicAdd(a.dls, dls_acc);        // every wave holds the same tile sums: count once
        if (is_sigmoid(LOSS)) {
            dbias_acc = wave_sum(dbias_acc);
            if (lane == 0 && wave == 0) atomicAdd(a.dbias, dbias_acc);
        }
    }
    if (LOSS == LOSS_DISTILL && MODE == MODE_DQ && a.dot) {
        // <dot_j, this split's share of row j>, one plain store per (split, row): the caller adds the splits in index order,
        // so what is built on it repeats bit for bit although the rows themselves are accumulated by float atomics.
        // gacc[t][r] is element e = ev_lo + 32 t + row_of(r, h) of resident row j.
        float d = 0.f;
        if (jvalid) {
            const float* drow = a.dot + jsrc * a.lddot + ev_lo;
#pragma unroll
            for (int t = 0; t < GT; ++t) {
                if (t >= etiles) continue;
#pragma unroll
                for (int r = 0; r < 16; ++r) d += gacc[t][r] * drow[32 * t + row_of(r, h)];
            }
        }
        d += __shfl_xor(d, 32, 64);
        __syncthreads();                                              // the last tile's readers of part_l are done
        if (h == 0) part_l[wave * HB + j] = d;
        __syncthreads();
        if (tid < HB && r0 + tid < a.nres) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += part_l[w * HB + tid];
            a.part[(long)blockIdx.y * a.nq + r0 + tid] = t;
        }
    }
    __syncthreads();
    float* tile = part_l + wave * HB * 33;                            // [j][e'] for this wave
    // the factor at the write: the similarity's scale, or (distillation) the student's whatever the similarity was
    const float oscale = (LOSS == LOSS_DISTILL) ? (a.out_logit_scale ? expf(*a.out_logit_scale) : 1.f) : scale;
    const long* const osel = (LOSS == LOSS_DISTILL) ? a.osel : a.sel;
#pragma unroll
    for (int t = 0; t < GT; ++t) {
        if (t >= etiles) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[j * 33 + row_of(r, h)] = gacc[t][r] * oscale;
        // lanes: 2 rows per pass (row = pass*2 + h), 32 columns
        for (int pass = 0; pass < 16; ++pass) {
            const int jr = pass * 2 + h;
            if (r0 + jr < a.nres) {
                const long dst = (MODE == MODE_DQ && osel) ? osel[r0 + jr] : (long)(r0 + jr);
                float* o = a.dres + dst * (long)EV + ev_lo + 32 * t + j;
                float v = tile[jr * 33 + j];
                if (LOSS == LOSS_DISTILL && MODE == MODE_DQ && a.sub && blockIdx.y == 0)          // once per row: the first split
                    v -= coef * oscale * a.sub[(long)(r0 + jr) * EV + ev_lo + 32 * t + j];
                if (a.splits == 1) *o += v;
                else atomicAdd(o, v);
            }
        }
    }
}

// merge the per-split (max, sum), pick the labelled logit, add the mean loss: one wave per query
__global__ __launch_bounds__(256) void infonce_merge_kernel(HeadArgs a, float* __restrict__ lse_out, float* __restrict__ loss) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.nq) return;
    float m, l;
    merge_max_sum(a.part + 2L * r, 2L * a.nq, a.splits, m, l);
    const float lse = m + __logf(l);
    const long src = a.sel ? a.sel[r] : (long)r;
    const long y = a.labels[src];
    const float* q = a.res + src * a.ldres;
    const float* k = a.str + y * a.ldstr;
    float d = 0.f;
    for (int c = lane; c < a.E; c += 64) d += q[c] * k[c];
    d = wave_sum(d);
    if (lane == 0) {
        lse_out[r] = lse;
        atomicAdd(loss, (lse - __expf(*a.logit_scale) * d) / (float)a.nq);
    }
}

// sum the workgroups' loss partials in index order and apply 1/nq: one workgroup, a fixed tree, no atomics
__global__ __launch_bounds__(256) void sigmoid_loss_sum_kernel(const float* __restrict__ part, int n, int nq, float* __restrict__ loss) {
    __shared__ float red[256];
    float t = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) t += part[i];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = red[0] / (float)nq;
}

size_t head_lds_bytes(int E, int nw) { return lds_bytes(E, nw) + 2 * HB * 4; }      // + qinfo
// LOSS_MULTIPOS keeps (lse, invpos) AND the 64-bit ids of the 32 streamed rows: [2][32] floats more than qinfo
constexpr size_t group_lds_extra(int loss) { return loss == LOSS_MULTIPOS ? 2 * HB * 4 : 0; }

struct Side {      // one matrix of a sweep: [n, E] fp32 rows, ld floats apart
    const float* p; long ld; int n;
};
constexpr int NO_CAP = 1 << 20;          // splits of a sweep whose partials need no workspace

// One sweep of the skeleton: `res` resident, `str` streamed, both E wide, the streamed blocks split under `cap`.
// The wave count follows head_sweep::eight_waves -- for FWD too, with Eval = the width of the values its log-sum-exp will later
// weigh: exp(x - max) of a row's largest entry is exactly 1 only when the sweep that rebuilds x adds it up as FWD did.
template <int MODE, int LOSS = LOSS_SOFTMAX>
int sweep(HeadArgs& a, Side res, Side str, int E, int cap, hipStream_t s) {
    static std::once_flag flag;
    std::call_once(flag, [] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(infonce_kernel<MODE, 4, LOSS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(head_lds_bytes(1024, 4) + group_lds_extra(LOSS)));
        hipFuncSetAttribute(reinterpret_cast<const void*>(infonce_kernel<MODE, 8, LOSS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)(head_lds_bytes(768, 8) + group_lds_extra(LOSS)));
    });
    a.res = res.p; a.ldres = res.ld; a.nres = res.n;
    a.str = str.p; a.ldstr = str.ld; a.nstr = str.n;
    a.E = E;
    const Splits sp = split_choice(res.n, str.n, 0, cap);
    a.splits = sp.splits;
    a.blocks_per_split = sp.blocks_per_split;
    const int rb = ce_div_up(res.n, HB);
    static const int force_nw = getenv("CE_HEAD_WAVES") ? atoi(getenv("CE_HEAD_WAVES")) : 0;
    if (eight_waves(E, LOSS == LOSS_DISTILL ? a.Eval : E) && force_nw != 4)
        hipLaunchKernelGGL((infonce_kernel<MODE, 8, LOSS>), dim3(rb, a.splits), dim3(512), head_lds_bytes(E, 8) + group_lds_extra(LOSS), s,
                           a);
    else
        hipLaunchKernelGGL((infonce_kernel<MODE, 4, LOSS>), dim3(rb, a.splits), dim3(256), head_lds_bytes(E, 4) + group_lds_extra(LOSS), s,
                           a);
    CE_LAUNCH_CHECK();
    return 0;
}

int check_common(const char* what, const float* q, long ldq, int nq, const float* k, long ldk, int nk, int E,
                 const float* logit_scale, const int64_t* labels) {
    if (int rc = check_features(what, "E", q, ldq, E)) return rc;
    if (int rc = check_features(what, "E", k, ldk, E)) return rc;
    CE_CHECK_ARG(logit_scale && labels, "%s: null buffer", what);
    CE_CHECK_ARG(nq > 0 && nk > 0, "%s: empty problem", what);
    CE_CHECK_ARG(nk < (1 << 24), "%s: more than 2^24 keys", what);
    return 0;
}

}  // namespace

extern "C" size_t ce_infonce_workspace_bytes(int nq) { return (size_t)CE_INFONCE_MAX_SPLITS * nq * 2 * sizeof(float); }

extern "C" int ce_infonce_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                              const float* logit_scale, const int64_t* labels, float* lse, float* loss, void* workspace,
                              void* stream) {
    if (int rc = check_common("ce_infonce_fwd", q, ldq, nq, k, ldk, nk, E, logit_scale, labels)) return rc;
    CE_CHECK_ARG(lse && loss && workspace, "ce_infonce_fwd: null output");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.labels = (const long*)labels; a.logit_scale = logit_scale; a.nq = nq;
    // per-split (max, sum) of every query, then the merge that also picks the labelled logit
    a.part = (float*)workspace;
    if (int rc = sweep<MODE_FWD>(a, Q, K, E, CE_INFONCE_MAX_SPLITS, s)) return rc;
    hipLaunchKernelGGL(infonce_merge_kernel, dim3(ce_div_up(nq, 4)), dim3(256), 0, s, a, lse, loss);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_infonce_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                              const float* logit_scale, const int64_t* labels, const float* lse, const float* grad, float* dq,
                              float* dk, float* dlogit_scale, void* stream) {
    if (int rc = check_common("ce_infonce_bwd", q, ldq, nq, k, ldk, nk, E, logit_scale, labels)) return rc;
    CE_CHECK_ARG(lse && grad && dq && dk && dlogit_scale, "ce_infonce_bwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.labels = (const long*)labels; a.logit_scale = logit_scale; a.lse = lse; a.grad = grad;
    a.nq = nq; a.dls = dlogit_scale;
    // dq: resident = queries, streamed = keys
    a.dres = dq;
    if (int rc = sweep<MODE_DQ>(a, Q, K, E, NO_CAP, s)) return rc;
    // dk: resident = keys, streamed = queries
    a.dres = dk;
    return sweep<MODE_DK>(a, K, Q, E, NO_CAP, s);
}

// ---- sigmoid pairwise loss (SigLIP) on the same sweep ----------------------------------------------------------------

extern "C" size_t ce_sigmoid_head_workspace_bytes(int nq, int nk) {
    if (nq <= 0 || nk <= 0) return 0;
    return (size_t)ce_div_up(nq, HB) * split_bound(nq, nk, 0, CE_INFONCE_MAX_SPLITS) * sizeof(float);
}

extern "C" int ce_sigmoid_head_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                                   const float* logit_scale, const float* logit_bias, const int64_t* labels, float* loss,
                                   void* workspace, void* stream) {
    if (int rc = check_common("ce_sigmoid_head_fwd", q, ldq, nq, k, ldk, nk, E, logit_scale, labels)) return rc;
    CE_CHECK_ARG(logit_bias && loss && workspace, "ce_sigmoid_head_fwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.labels = (const long*)labels; a.logit_scale = logit_scale; a.logit_bias = logit_bias; a.nq = nq;
    // one loss partial per workgroup (never more splits than the workspace was sized for), then their sum in index order
    a.loss_part = (float*)workspace;
    if (int rc = sweep<MODE_FWD, LOSS_SIGMOID>(a, Q, K, E, CE_INFONCE_MAX_SPLITS, s)) return rc;
    hipLaunchKernelGGL(sigmoid_loss_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, ce_div_up(nq, HB) * a.splits, nq,
                       loss);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_sigmoid_head_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                                   const float* logit_scale, const float* logit_bias, const int64_t* labels, const float* grad,
                                   float* dq, float* dk, float* dlogit_scale, float* dlogit_bias, void* stream) {
    if (int rc = check_common("ce_sigmoid_head_bwd", q, ldq, nq, k, ldk, nk, E, logit_scale, labels)) return rc;
    CE_CHECK_ARG(logit_bias && grad && dq && dk && dlogit_scale && dlogit_bias, "ce_sigmoid_head_bwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.labels = (const long*)labels; a.logit_scale = logit_scale; a.logit_bias = logit_bias; a.grad = grad;
    a.nq = nq; a.dls = dlogit_scale; a.dbias = dlogit_bias;
    // dq: resident = queries, streamed = keys (also the scale and bias gradients)
    a.dres = dq;
    if (int rc = sweep<MODE_DQ, LOSS_SIGMOID>(a, Q, K, E, NO_CAP, s)) return rc;
    // dk: resident = keys, streamed = queries
    a.dres = dk;
    return sweep<MODE_DK, LOSS_SIGMOID>(a, K, Q, E, NO_CAP, s);
}

// ---- group-id targets: several positives per query, softmax and sigmoid ------------------------------------------------

namespace {

// merge the per-split (max, sum, count, possum): lse, invpos = 1 / n_r (0 without positives), and the row's term of the mean loss
// lse - possum / n_r (rows without positives add nothing; the divisor stays nq).  One thread per query, one atomic per wave.
__global__ __launch_bounds__(256) void multipos_merge_kernel(const float* __restrict__ part, int splits, int nq,
                                                             float* __restrict__ lse_out, float* __restrict__ invpos_out,
                                                             float* __restrict__ loss) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    float term = 0.f;
    if (r < nq) {
        float m, l;
        merge_max_sum(part + 4L * r, 4L * nq, splits, m, l);
        float cnt = 0.f, ps = 0.f;
        for (int s = 0; s < splits; ++s) {
            cnt += part[4L * ((long)s * nq + r) + 2];
            ps += part[4L * ((long)s * nq + r) + 3];
        }
        const float lse = m + __logf(l), inv = cnt > 0.f ? 1.f / cnt : 0.f;
        lse_out[r] = lse;
        invpos_out[r] = inv;
        if (cnt > 0.f) term = (lse - ps * inv) / (float)nq;
    }
    term = wave_sum(term);
    if ((threadIdx.x & 63) == 0 && term != 0.f) atomicAdd(loss, term);
}

int check_groups(const char* what, const float* q, long ldq, int nq, const float* k, long ldk, int nk, int E,
                 const float* logit_scale, const int64_t* qgroup, const int64_t* kgroup) {
    if (int rc = check_features(what, "E", q, ldq, E)) return rc;
    if (int rc = check_features(what, "E", k, ldk, E)) return rc;
    CE_CHECK_ARG(logit_scale && qgroup && kgroup, "%s: null buffer", what);
    CE_CHECK_ARG(nq > 0 && nk > 0, "%s: empty problem", what);
    CE_CHECK_ARG(nk < (1 << 24), "%s: more than 2^24 keys", what);          // a row's positive count is kept in fp32
    return 0;
}

}  // namespace

extern "C" size_t ce_multipos_head_workspace_bytes(int nq) {
    return nq > 0 ? (size_t)CE_INFONCE_MAX_SPLITS * nq * 4 * sizeof(float) : 0;
}

extern "C" int ce_multipos_head_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                                    const float* logit_scale, const int64_t* qgroup, const int64_t* kgroup, float* lse,
                                    float* invpos, float* loss, void* workspace, void* stream) {
    if (int rc = check_groups("ce_multipos_head_fwd", q, ldq, nq, k, ldk, nk, E, logit_scale, qgroup, kgroup)) return rc;
    CE_CHECK_ARG(lse && invpos && loss && workspace, "ce_multipos_head_fwd: null output");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.qgroup = (const long*)qgroup; a.kgroup = (const long*)kgroup; a.logit_scale = logit_scale;
    a.nq = nq;
    // per-split (max, sum, count, possum) of every query from ONE sweep, then the merge
    a.part = (float*)workspace;
    if (int rc = sweep<MODE_FWD, LOSS_MULTIPOS>(a, Q, K, E, CE_INFONCE_MAX_SPLITS, s)) return rc;
    hipLaunchKernelGGL(multipos_merge_kernel, dim3(ce_div_up(nq, 256)), dim3(256), 0, s, (const float*)workspace, a.splits, nq, lse,
                       invpos, loss);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_multipos_head_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                                    const float* logit_scale, const int64_t* qgroup, const int64_t* kgroup, const float* lse,
                                    const float* invpos, const float* grad, float* dq, float* dk, float* dlogit_scale,
                                    void* stream) {
    if (int rc = check_groups("ce_multipos_head_bwd", q, ldq, nq, k, ldk, nk, E, logit_scale, qgroup, kgroup)) return rc;
    CE_CHECK_ARG(lse && invpos && grad && dq && dk && dlogit_scale, "ce_multipos_head_bwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.qgroup = (const long*)qgroup; a.kgroup = (const long*)kgroup; a.logit_scale = logit_scale;
    a.lse = lse; a.invpos = invpos; a.grad = grad; a.nq = nq; a.dls = dlogit_scale;
    a.dres = dq;
    if (int rc = sweep<MODE_DQ, LOSS_MULTIPOS>(a, Q, K, E, NO_CAP, s)) return rc;
    a.dres = dk;
    return sweep<MODE_DK, LOSS_MULTIPOS>(a, K, Q, E, NO_CAP, s);
}

extern "C" int ce_sigmoid_head_group_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                                         const float* logit_scale, const float* logit_bias, const int64_t* qgroup,
                                         const int64_t* kgroup, float* loss, void* workspace, void* stream) {
    if (int rc = check_groups("ce_sigmoid_head_group_fwd", q, ldq, nq, k, ldk, nk, E, logit_scale, qgroup, kgroup)) return rc;
    CE_CHECK_ARG(logit_bias && loss && workspace, "ce_sigmoid_head_group_fwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.qgroup = (const long*)qgroup; a.kgroup = (const long*)kgroup; a.logit_scale = logit_scale;
    a.logit_bias = logit_bias; a.nq = nq;
    // the partial-sum loss path of ce_sigmoid_head_fwd (workspace of ce_sigmoid_head_workspace_bytes): the same bits every run
    a.loss_part = (float*)workspace;
    if (int rc = sweep<MODE_FWD, LOSS_SIGMOID_GROUP>(a, Q, K, E, CE_INFONCE_MAX_SPLITS, s)) return rc;
    hipLaunchKernelGGL(sigmoid_loss_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, ce_div_up(nq, HB) * a.splits, nq,
                       loss);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_sigmoid_head_group_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                                         const float* logit_scale, const float* logit_bias, const int64_t* qgroup,
                                         const int64_t* kgroup, const float* grad, float* dq, float* dk, float* dlogit_scale,
                                         float* dlogit_bias, void* stream) {
    if (int rc = check_groups("ce_sigmoid_head_group_bwd", q, ldq, nq, k, ldk, nk, E, logit_scale, qgroup, kgroup)) return rc;
    CE_CHECK_ARG(logit_bias && grad && dq && dk && dlogit_scale && dlogit_bias, "ce_sigmoid_head_group_bwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.qgroup = (const long*)qgroup; a.kgroup = (const long*)kgroup; a.logit_scale = logit_scale;
    a.logit_bias = logit_bias; a.grad = grad; a.nq = nq; a.dls = dlogit_scale; a.dbias = dlogit_bias;
    a.dres = dq;
    if (int rc = sweep<MODE_DQ, LOSS_SIGMOID_GROUP>(a, Q, K, E, NO_CAP, s)) return rc;
    a.dres = dk;
    return sweep<MODE_DK, LOSS_SIGMOID_GROUP>(a, K, Q, E, NO_CAP, s);
}

// ---- distillation: cross entropy against a teacher's softmax, on sweeps of the same skeleton --------------------------
//   S = s <q^_r, k^_c> (student, width Es), T = st <tq^_r, tk^_c> (teacher, width Et, constants), P_t = softmax_c T, P_s = softmax_c S
//   loss = (1/nq) sum_r (lse_s[r] - sum_c P_t S),   G = (g/nq)(P_s - P_t)
// With v_r = sum_c P_t[r,c] k^_c ([nq, Es]): sum_c P_t S = s <q^_r, v_r> and dq^_r = (g/nq) s (sum_c P_s k^_c - v_r), so no sweep ever
// needs a student and a teacher resident block in LDS at once (512 + 768 wide: 165 KB at 32 rows).  A sweep of LOSS_DISTILL
// has G = c exp(x - lse) with no label term, streams a value matrix that is not the similarity operand through the gradient
// product (its own width: accumulators and output transpose run over Eval) and writes with a scale of its own.

namespace {

// log-sum-exp from the per-split (max, sum), one thread per query, kept as the pair (max, log sum): one float holds a
// log-sum-exp near 40 to 2e-6 only, and a softmax rebuilt as exp(x - lse) would be off by that factor in EVERY entry of the
// row -- up to 2e-6 x sum_c P S ~ 1e-4 in a row term whose value is ~ 1 when both distributions are peaked.  exp((x - max)
// - log sum) is normalised to fp32 rounding -- provided the sweep rebuilds x bit for bit as FWD saw it (sweep()'s wave rule).
__global__ __launch_bounds__(256) void lse_merge_kernel(const float* __restrict__ part, int splits, int nq, float* __restrict__ lse_out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nq) return;
    float m, l;
    merge_max_sum(part + 2L * r, 2L * nq, splits, m, l);
    lse_out[2 * r] = m;
    lse_out[2 * r + 1] = __logf(l);
}

// term[r] = lse_s[r] - s <q^_r, v_r>, the dot product as the sum of the v sweep's per-split shares in index order
__global__ __launch_bounds__(256) void distill_row_term_kernel(const float* __restrict__ dotpart, int splits,
                                                               const float* __restrict__ lse_s,
                                                               const float* __restrict__ logit_scale, int nq,
                                                               float* __restrict__ term) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nq) return;
    float d = 0.f;
    for (int s = 0; s < splits; ++s) d += dotpart[(long)s * nq + r];
    term[r] = (lse_s[2 * r] - expf(*logit_scale) * d) + lse_s[2 * r + 1];
}

// *out += sum_r <x_r, y_r>: one wave per row
__global__ __launch_bounds__(256) void rowdot_sum_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy,
                                                         int n, int E, float* __restrict__ out) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float d = 0.f;
    for (int r = blockIdx.x * 4 + w; r < n; r += gridDim.x * 4) {
        const float* xr = x + (long)r * ldx;
        const float* yr = y + (long)r * ldy;
        for (int c = lane; c < E; c += 64) d += xr[c] * yr[c];
    }
    d = wave_sum(d);
    if (lane == 0) red[w] = d;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, (red[0] + red[1]) + (red[2] + red[3]));
}

int check_distill(const char* what, const float* q, long ldq, int nq, const float* k, long ldk, int nk, int Es,
                  const float* logit_scale, const float* tq, long ldtq, const float* tk, long ldtk, int Et,
                  const float* teacher_logit_scale) {
    if (int rc = check_features(what, "Es", q, ldq, Es)) return rc;
    if (int rc = check_features(what, "Es", k, ldk, Es)) return rc;
    if (int rc = check_features(what, "Et", tq, ldtq, Et)) return rc;
    if (int rc = check_features(what, "Et", tk, ldtk, Et)) return rc;
    CE_CHECK_ARG(logit_scale && teacher_logit_scale, "%s: null buffer", what);
    CE_CHECK_ARG(nq > 0 && nk > 0, "%s: empty problem", what);
    return 0;
}

}  // namespace

extern "C" size_t ce_distill_head_workspace_bytes(int nq) { return ce_infonce_workspace_bytes(nq); }

extern "C" int ce_distill_head_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int Es,
                                   const float* logit_scale, const float* tq, long ldtq, const float* tk, long ldtk, int Et,
                                   const float* teacher_logit_scale, float* lse_s, float* lse_t, float* v, float* loss,
                                   void* workspace, void* stream) {
    if (int rc = check_distill("ce_distill_head_fwd", q, ldq, nq, k, ldk, nk, Es, logit_scale, tq, ldtq, tk, ldtk, Et,
                               teacher_logit_scale))
        return rc;
    CE_CHECK_ARG(lse_s && lse_t && v && loss && workspace, "ce_distill_head_fwd: null output");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk}, TQ{tq, ldtq, nq}, TK{tk, ldtk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.nq = nq; a.part = (float*)workspace;
    // log-sum-exp of the teacher's rows, then of the student's (the partials of one are merged before the other's are written)
    // (Eval = Es in both: the wave count of the sweeps that will read these statistics)
    a.Eval = Es;
    a.logit_scale = teacher_logit_scale;
    if (int rc = sweep<MODE_FWD, LOSS_DISTILL>(a, TQ, TK, Et, CE_INFONCE_MAX_SPLITS, s)) return rc;
    hipLaunchKernelGGL(lse_merge_kernel, dim3(ce_div_up(nq, 256)), dim3(256), 0, s, (const float*)workspace, a.splits, nq, lse_t);
    CE_LAUNCH_CHECK();
    a.logit_scale = logit_scale;
    if (int rc = sweep<MODE_FWD, LOSS_DISTILL>(a, Q, K, Es, CE_INFONCE_MAX_SPLITS, s)) return rc;
    hipLaunchKernelGGL(lse_merge_kernel, dim3(ce_div_up(nq, 256)), dim3(256), 0, s, (const float*)workspace, a.splits, nq, lse_s);
    CE_LAUNCH_CHECK();
    // v[r] += sum_c softmax(T)[r,c] k^_c: the teacher's similarity, the student's keys as values, c = 1, written unscaled
    a.logit_scale = teacher_logit_scale;
    // the same sweep leaves <q^_r, its share of v_r> per split in the workspace: the loss does not depend on the atomics' order
    a.lse = lse_t; a.val = k; a.ldval = ldk; a.csign = 1.f; a.dres = v; a.dot = q; a.lddot = ldq;
    if (int rc = sweep<MODE_DQ, LOSS_DISTILL>(a, TQ, TK, Et, CE_INFONCE_MAX_SPLITS, s)) return rc;
    // the rows' terms, then their sum in index order: no float atomic on the loss
    float* term = (float*)workspace + (size_t)CE_INFONCE_MAX_SPLITS * nq;
    hipLaunchKernelGGL(distill_row_term_kernel, dim3(ce_div_up(nq, 256)), dim3(256), 0, s, (const float*)workspace, a.splits,
                       (const float*)lse_s, logit_scale, nq, term);
    CE_LAUNCH_CHECK();
    hipLaunchKernelGGL(sigmoid_loss_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)term, nq, nq, loss);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" int ce_distill_head_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int Es,
                                   const float* logit_scale, const float* tq, long ldtq, const float* tk, long ldtk, int Et,
                                   const float* teacher_logit_scale, const float* lse_s, const float* lse_t, const float* v,
                                   const float* grad, float* dq, float* dk, void* stream) {
    if (int rc = check_distill("ce_distill_head_bwd", q, ldq, nq, k, ldk, nk, Es, logit_scale, tq, ldtq, tk, ldtk, Et,
                               teacher_logit_scale))
        return rc;
    CE_CHECK_ARG(lse_s && lse_t && v && grad && dq && dk, "ce_distill_head_bwd: null buffer");
    hipStream_t s = (hipStream_t)stream;
    const Side Q{q, ldq, nq}, K{k, ldk, nk}, TQ{tq, ldtq, nq}, TK{tk, ldtk, nk};
    HeadArgs a{};
    a.sel = (const long*)sel; a.nq = nq; a.grad = grad; a.out_logit_scale = logit_scale; a.Eval = Es;
    // dq[sel[r]] += (g/nq) s (sum_c P_s k^_c - v_r): student similarity, resident = queries; the first split's write takes v off
    a.logit_scale = logit_scale;
    a.lse = lse_s; a.val = k; a.ldval = ldk; a.csign = 1.f; a.dres = dq; a.osel = (const long*)sel; a.sub = v;
    if (int rc = sweep<MODE_DQ, LOSS_DISTILL>(a, Q, K, Es, NO_CAP, s)) return rc;
    // dk[c] += (g/nq) s sum_r P_s q^_r: student similarity, resident = keys
    a.val = q; a.ldval = ldq; a.dres = dk;
    a.osel = nullptr; a.sub = nullptr;
    if (int rc = sweep<MODE_DK, LOSS_DISTILL>(a, K, Q, Es, NO_CAP, s)) return rc;
    // dk[c] -= (g/nq) s sum_r P_t q^_r: the TEACHER's similarity, the student's queries as values, the student's scale at the write
    a.logit_scale = teacher_logit_scale; a.lse = lse_t;
    a.csign = -1.f;
    return sweep<MODE_DK, LOSS_DISTILL>(a, TK, TQ, Et, NO_CAP, s);
}

extern "C" int ce_rowdot_sum(const float* x, long ldx, const float* y, long ldy, int n, int E, float* out, void* stream) {
    CE_CHECK_ARG(x && y && out, "ce_rowdot_sum: null buffer");
    CE_CHECK_ARG(n > 0 && E > 0 && ldx >= E && ldy >= E, "ce_rowdot_sum: bad shape");
    int blocks = ce_div_up(n, 4);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(rowdot_sum_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, n, E, out);
    CE_LAUNCH_CHECK();
    return 0;
}
