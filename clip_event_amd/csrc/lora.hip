// Low-rank adapters (LoRA) in the merged-operand form (gfx950).
//
// The towers never see an adapter: before a forward, ce_lora_merge writes bf16(W0 + s B A) into the operand copies of the adapted
// matrices (the row-major mirror and the W^T copy); after the backward, ce_lora_grad turns the full fp32 weight gradient dW that
// the towers left in the flat gradient buffer into dA = s B^T dW and dB = s dW A^T.  Both are memory-bound passes; the products
// run on the fp32-input matrix instruction v_mfma_f32_32x32x2_f32 (an exact fmaf chain, as infonce.hip / retrieval.hip use it):
//   A operand: lane l holds A[i = l & 31][k = l >> 5], B operand: B[k = l >> 5][j = l & 31],
//   C/D: lane l holds column l & 31, register r row (r & 3) + 8 (r >> 2) + 4 (l >> 5).
#include "common.hpp"
#include "../../include/clip_event_hip.h"

namespace {

constexpr int kMaxRank = 64;
constexpr int kPitch = 68;            // floats per row of the fp32 LDS tile: 16-byte rows, and 17 (odd) 16-byte units apart

__device__ __forceinline__ int row_of(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// ---- merge ------------------------------------------------------------------------------------------------------------------------
// One 64 x 64 tile per workgroup (tile_start as ce_transpose_job's).  The four waves each form one 32 x 32 quadrant of t = B A in
// k order, the tile goes through LDS into the row-major chunk layout of optim_tiles_kernel (16 bytes of W0 per lane), and the bf16
// result leaves twice: to the mirror, and through a second LDS tile transposed to W^T.
template <bool MASTER>
__global__ __launch_bounds__(256) void lora_merge_kernel(const ce_lora_job* __restrict__ jobs, int njobs) {
    __shared__ float tl[64][kPitch];
    __shared__ bf16_t tile[64][66];
    int jn = 0;
    const int blk = blockIdx.x;
    while (jn + 1 < njobs && blk >= jobs[jn + 1].tile_start) ++jn;      // block-uniform
    const ce_lora_job job = jobs[jn];
    const int rows = job.rows, cols = job.cols, rank = job.rank;
    const int t = blk - job.tile_start;
    const int tiles_c = (cols + 63) / 64;
    const int r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;

    // the W0 tile: 64 rows x 16 four-element chunks, requested before the product
    f32x4 wv[4];
    bool ok[4];
    long at[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = threadIdx.x + k * 256;
        const int r = idx >> 4, ch = idx & 15;
        ok[k] = r0 + r < rows && c0 + ch * 4 < cols;
        at[k] = (long)(r0 + r) * cols + c0 + ch * 4;
        wv[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ok[k]) wv[k] = *reinterpret_cast<const f32x4*>(job.w0 + at[k]);
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int qr = 32 * (wave >> 1), qc = 32 * (wave & 1);
    const int orow = r0 + qr + j, ocol = c0 + qc + j;
    const bool rv = orow < rows, cv = ocol < cols;
    const float* brow = job.b + (long)orow * rank;
    const float* acol = job.a + ocol;
    f32x16 acc = zero16();
    for (int k0 = 0; k0 < rank; k0 += 16) {         // eight k-steps' operands requested together (one load latency per 16 of the
        float bv[8], av[8];                         // rank); the rank is padded with zeros to the instruction's k
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + 2 * u + h;
            const bool kv = k < rank;
            bv[u] = (rv && kv) ? brow[k] : 0.f;
            av[u] = (cv && kv) ? acol[(long)k * cols] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (k0 + 2 * u < rank) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[u], av[u], acc, 0, 0, 0);      // (wave-uniform)
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) tl[qr + row_of(r, h)][qc + j] = acc[r];
    __syncthreads();

    bf16_t* const w16 = reinterpret_cast<bf16_t*>(job.w16);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = threadIdx.x + k * 256;
        const int r = idx >> 4, ch = idx & 15;
        const f32x4 tv = *reinterpret_cast<const f32x4*>(&tl[r][ch * 4]);
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = __builtin_fmaf(job.scale, tv[e], wv[k][e]);
        const u32x2 pk = {pack_bf2(w[0], w[1]), pack_bf2(w[2], w[3])};
        uint32_t* trow = reinterpret_cast<uint32_t*>(&tile[r][ch * 4]);
        trow[0] = pk[0];
        trow[1] = pk[1];
        if (ok[k]) {
            __builtin_nontemporal_store(pk, reinterpret_cast<u32x2*>(w16 + at[k]));
            if (MASTER) *reinterpret_cast<f32x4*>(job.w0 + at[k]) = w;
        }
    }
    __syncthreads();
    if (!job.wt) return;
    bf16_t* const wt = reinterpret_cast<bf16_t*>(job.wt);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = threadIdx.x + k * 256;                 // 64 output rows (source columns) x 8 chunks of 8 source rows
        const int c = idx >> 3, ch = idx & 7;
        if (c0 + c < cols && r0 + ch * 8 < rows) {
            uint32_t w[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                w[e] = (uint32_t)tile[ch * 8 + 2 * e][c] | ((uint32_t)tile[ch * 8 + 2 * e + 1][c] << 16);
            const u32x4 v = {w[0], w[1], w[2], w[3]};
            __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(wt + (long)(c0 + c) * rows + r0 + ch * 8));
        }
    }
}

// ---- gradients --------------------------------------------------------------------------------------------------------------------
// One workgroup per strip of 64 rows of dW, walking the strip's 64-column tiles (the next tile's loads in flight while this one is
// multiplied).  A tile sits in LDS and serves both products:
//   dA share [rank, 64 cols] = B_strip^T dW_tile    (sum over the strip's 64 rows; stored to the workspace, complete per tile)
//   dB      [64 rows, rank] += dW_tile A_tile^T     (sum over the columns; accumulated in registers across the tiles)
// A wave owns one 32 x 32 output tile of each: rank <= 32 -> waves 0, 1 take the two column halves of dA and waves 2, 3 the two row
// halves of dB; rank > 32 -> wave w takes rank tile w >> 1 and half w & 1 of both.
__global__ __launch_bounds__(256) void lora_grad_kernel(const ce_lora_job* __restrict__ jobs, int njobs, float* __restrict__ ws) {
    __shared__ float tl[64][kPitch];
    int jn = 0;
    const int blk = blockIdx.x;
    while (jn + 1 < njobs && blk >= jobs[jn + 1].strip_start) ++jn;     // block-uniform
    const ce_lora_job job = jobs[jn];
    const int rows = job.rows, cols = job.cols, rank = job.rank;
    const int strip = blk - job.strip_start;
    const int r0 = strip * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const bool two = rank > 32;
    const int rt = two ? (wave >> 1) : 0, half = wave & 1;
    const bool do_a = two || wave < 2, do_b = two || wave >= 2;
    const int kk = rt * 32 + j;                        // the rank index on this lane, in both products
    const bool kvalid = kk < rank;

    // dA's A operand [m = rank index][k = strip row]: B[r0 + 2 step + h][kk], the same for every column tile
    float bs[32];
#pragma unroll
    for (int s = 0; s < 32; ++s) {
        const int o = r0 + 2 * s + h;
        bs[s] = (do_a && kvalid && o < rows) ? job.b[(long)o * rank + kk] : 0.f;
    }
    float* const part = ws + job.ws_start + (long)strip * rank * cols;
    f32x16 acc_b = zero16();

    f32x4 nx[4];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = threadIdx.x + k * 256;
            const int r = idx >> 4, ch = idx & 15;
            nx[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r0 + r < rows && c0 + ch * 4 < cols)
                nx[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(job.gw + (long)(r0 + r) * cols + c0 + ch * 4));
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < cols; c0 += 64) {
        __syncthreads();                               // the previous tile's readers are done
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = threadIdx.x + k * 256;
            *reinterpret_cast<f32x4*>(&tl[idx >> 4][(idx & 15) * 4]) = nx[k];
        }
        __syncthreads();
        if (c0 + 64 < cols) fetch(c0 + 64);
        if (do_a) {
            // B operand [k = strip row][n = column]: dW[2 step + h][half * 32 + j]
            f32x16 acc_a = zero16();
#pragma unroll
            for (int s = 0; s < 32; ++s)
                acc_a = __builtin_amdgcn_mfma_f32_32x32x2f32(bs[s], tl[2 * s + h][half * 32 + j], acc_a, 0, 0, 0);
            const int i = c0 + half * 32 + j;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = rt * 32 + row_of(r, h);
                if (k < rank && i < cols) part[(long)k * cols + i] = acc_a[r];
            }
        }
        if (do_b) {
            // A operand [m = strip row][k = column]: dW[half * 32 + j][.], B operand [k = column][n = rank index]: A[kk][.]; the
            // column of (step, h) is 8 (step >> 2) + 4 h + (step & 3) on both sides, so a lane reads 16 bytes per four steps
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 dv = *reinterpret_cast<const f32x4*>(&tl[half * 32 + j][8 * g + 4 * h]);
                const int i = c0 + 8 * g + 4 * h;
                f32x4 av = {0.f, 0.f, 0.f, 0.f};
                if (kvalid && i < cols) av = *reinterpret_cast<const f32x4*>(job.a + (long)kk * cols + i);
#pragma unroll
                for (int x = 0; x < 4; ++x) acc_b = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[x], av[x], acc_b, 0, 0, 0);
            }
        }
    }
    if (do_b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = r0 + half * 32 + row_of(r, h);
            if (o < rows && kvalid) job.gb[(long)o * rank + kk] = job.scale * acc_b[r];
        }
    }
}

// dA = scale * (the strips' shares added in ascending order): blockIdx.y = job, 1024 elements per workgroup
__global__ __launch_bounds__(256) void lora_fold_kernel(const ce_lora_job* __restrict__ jobs, const float* __restrict__ ws) {
    const ce_lora_job job = jobs[blockIdx.y];
    const long n = (long)job.rank * job.cols;          // a multiple of 8
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= n) return;
    const int strips = (job.rows + 63) / 64;
    const float* p = ws + job.ws_start + e;
    f32x4 s = *reinterpret_cast<const f32x4*>(p);
    for (int t = 1; t < strips; ++t) s += *reinterpret_cast<const f32x4*>(p + (long)t * n);
    *reinterpret_cast<f32x4*>(job.ga + e) = job.scale * s;
}

// ---- the host table, checked: 0 or -EINVAL with a message -------------------------------------------------------------------------
struct lora_totals {
    long tiles, strips, ws_floats, fold_blocks;
};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int lora_check(const char* who, const ce_lora_job* jobs, int njobs, lora_totals& t) {
    CE_CHECK_ARG(jobs && njobs > 0, "%s: the job table is NULL or empty (njobs %d)", who, njobs);
    t = {0, 0, 0, 1};
    for (int i = 0; i < njobs; ++i) {
        const ce_lora_job& q = jobs[i];
        CE_CHECK_ARG(q.rank >= 1 && q.rank <= kMaxRank, "%s: job %d has rank %d; the rank must lie in 1..%d", who, i, q.rank, kMaxRank);
        CE_CHECK_ARG(q.rows > 0 && q.cols > 0 && q.rows % 8 == 0 && q.cols % 8 == 0,
                     "%s: job %d is %d x %d; rows and cols must be positive multiples of 8", who, i, q.rows, q.cols);
        CE_CHECK_ARG(q.w0 && q.w16 && q.a && q.b && q.gw && q.ga && q.gb, "%s: job %d has a NULL pointer (only wt may be NULL)", who, i);
        CE_CHECK_ARG(aligned16(q.w0) && aligned16(q.w16) && aligned16(q.wt) && aligned16(q.a) && aligned16(q.b) && aligned16(q.gw) &&
                         aligned16(q.ga) && aligned16(q.gb), "%s: job %d has a pointer that is not 16-byte aligned", who, i);
        CE_CHECK_ARG(q.tile_start == t.tiles && q.strip_start == t.strips && q.ws_start == t.ws_floats,
                     "%s: job %d starts at tile %d, strip %d, workspace float %ld; the running counts are %ld, %ld, %ld", who, i,
                     q.tile_start, q.strip_start, q.ws_start, t.tiles, t.strips, t.ws_floats);
        const long strips = (q.rows + 63) / 64;
        t.tiles += strips * ((q.cols + 63) / 64);
        t.strips += strips;
        t.ws_floats += strips * q.rank * q.cols;
        const long fold = ((long)q.rank * q.cols + 1023) / 1024;
        if (fold > t.fold_blocks) t.fold_blocks = fold;
        CE_CHECK_ARG(t.tiles < (1L << 31) && t.strips < (1L << 31), "%s: the table has more than 2^31 tiles", who);
    }
    return 0;
}

}  // namespace

extern "C" int ce_lora_merge(const ce_lora_job* jobs_host, const void* jobs_device, int njobs, int total_tiles, int write_master,
                             void* stream) {
    lora_totals t;
    if (int rc = lora_check("ce_lora_merge", jobs_host, njobs, t)) return rc;
    CE_CHECK_ARG(jobs_device, "ce_lora_merge: the device copy of the job table is NULL");
    CE_CHECK_ARG(total_tiles == t.tiles, "ce_lora_merge: total_tiles is %d, the table has %ld", total_tiles, t.tiles);
    const ce_lora_job* jd = reinterpret_cast<const ce_lora_job*>(jobs_device);
    if (write_master)
        hipLaunchKernelGGL(lora_merge_kernel<true>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, jd, njobs);
    else
        hipLaunchKernelGGL(lora_merge_kernel<false>, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream, jd, njobs);
    CE_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t ce_lora_grad_workspace_bytes(const ce_lora_job* jobs_host, int njobs) {
    lora_totals t;
    if (lora_check("ce_lora_grad_workspace_bytes", jobs_host, njobs, t)) return 0;
    return (size_t)t.ws_floats * sizeof(float);
}

extern "C" int ce_lora_grad(const ce_lora_job* jobs_host, const void* jobs_device, int njobs, int total_strips, void* workspace,
                            size_t workspace_bytes, void* stream) {
    lora_totals t;
    if (int rc = lora_check("ce_lora_grad", jobs_host, njobs, t)) return rc;
    CE_CHECK_ARG(jobs_device, "ce_lora_grad: the device copy of the job table is NULL");
    CE_CHECK_ARG(total_strips == t.strips, "ce_lora_grad: total_strips is %d, the table has %ld", total_strips, t.strips);
    const size_t need = (size_t)t.ws_floats * sizeof(float);
    CE_CHECK_ARG(workspace && workspace_bytes >= need, "ce_lora_grad: the workspace of %zu bytes is too small (need %zu)",
                 workspace ? workspace_bytes : (size_t)0, need);
    CE_CHECK_ARG(aligned16(workspace), "ce_lora_grad: the workspace is not 16-byte aligned");
    const ce_lora_job* jd = reinterpret_cast<const ce_lora_job*>(jobs_device);
    float* ws = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(lora_grad_kernel, dim3((unsigned)total_strips), dim3(256), 0, (hipStream_t)stream, jd, njobs, ws);
    CE_LAUNCH_CHECK();
    hipLaunchKernelGGL(lora_fold_kernel, dim3((unsigned)t.fold_blocks, (unsigned)njobs), dim3(256), 0, (hipStream_t)stream, jd,
                       (const float*)ws);
    CE_LAUNCH_CHECK();
    return 0;
}
