/* clip_event_hip.h -- C ABI of libclip_event_hip.so (gfx950 / MI355X).
 *
 * The reference (limanling/clip-event) has no FFI: its hot path is a Python module API
 * (src/clip-event/model_clip.py) that reaches the device through torch.nn ops.  This
 * library is the device side of the drop-in: one entry point per op call site of that
 * path, each citing the reference lines it replaces.  The Python mirror of the reference
 * API (clip_event_amd.model.CLIP, CriterionContrastive, CriterionAlignment) calls these
 * through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions:
 *   - device pointers are borrowed, never freed or retained; workspaces are caller-provided;
 *   - every launch is asynchronous on `stream` (a hipStream_t passed as void*); no entry
 *     point synchronises the device or allocates device memory;
 *   - return 0 on success, a negative errno-style code on failure; ce_last_error() returns
 *     the message of the calling thread's last failure;
 *   - "bf16" = raw bfloat16 bits (uint16_t); "f32" = float; row-major, leading dimensions in
 *     ELEMENTS;
 *   - activations are token-major [rows = batch*tokens, width]; master weights / gradients are fp32, GEMM
 *     operands bf16, accumulation fp32; the residual stream is fp32 or IEEE fp16 (ce_tower_desc.stream16).
 */
#ifndef CLIP_EVENT_HIP_H
#define CLIP_EVENT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* ce_last_error(void);
int ce_version(void);

/* ---- GEMM epilogues (ce_gemm_nt) ---- */
enum {
    CE_EPI_BF16 = 0,          /* out(bf16) = acc                                            */
    CE_EPI_F32 = 1,           /* out(f32)  = acc                                            */
    CE_EPI_BIAS_BF16 = 2,     /* out(bf16) = acc + bias[n]                                  */
    CE_EPI_BIAS_F32 = 3,      /* out(f32)  = acc + bias[n]                                  */
    CE_EPI_BIAS_RESID_F32 = 4,/* out(f32)  = resid(f32) + acc + bias[n]     (x + proj(..))  */
    CE_EPI_BIAS_GELU = 5,     /* a = acc + bias; out(bf16) = dQuickGELU(a) = s + 1.702 a s (1 - s), s = sigmoid(1.702 a): the
                               * factor the backward needs, from the fp32 a; out2(bf16) = QuickGELU(a) = a s */
    CE_EPI_GELUGRAD_BF16 = 6, /* out(bf16) = acc * aux(bf16), aux = the derivative BIAS_GELU saved; out2 (nullable) is reused as
                               * a float[N] that receives += the column sums of out (bias gradient); where the launch
                               * policy picks the 128x128 kernel (ce_gemm_nt_plan) the sums are a second pass over out,
                               * which takes N % 8 == 0 and ldo % 8 == 0 only: refused otherwise, before anything is launched */
    CE_EPI_BIAS_RESID_F16 = 7,/* out(f16)  = resid(f16) + acc + bias[n]: the residual add on an fp16 stream (CE_T_F16;
                               * resid / out point at IEEE half data, ldr / ldo in elements; stores saturate at 65504) */
    CE_EPI_BIAS_QGELU_BF16 = 8/* out(bf16) = QuickGELU(acc + bias[n]): BIAS_GELU's out2 bit for bit (same tile variant at the same
                               * M, N, K), without the derivative -- the forward that no backward follows; out2 unused */
};

/* Element types of residual-stream operands (ce_layernorm_*_t, ce_token_embed_t, ce_cast_t, ce_tower_desc.stream16).
 * The reference keeps the stream in fp32 (model_clip.py:190-200).  It is read and written four times per block and
 * direction and never enters a matrix unit, so its storage format is a bandwidth choice: IEEE fp16 (11 significand bits;
 * bf16 has 8) leaves the gradient noise floor where the bf16 GEMM operands put it (tests/stream16_emulation.py: median
 * per-parameter error x 1.04 on BASELINE config 1; a bf16 stream: x 2.4).  fp16 stores saturate at +-65504, and a
 * GRADIENT stream holds gradient * scale, a power of two chosen per backward pass from the largest element of the
 * gradient that enters the tower (ce_grad_scale; gradients of a mean loss sit below fp16's normal range). */
#ifndef CE_T_F32
#define CE_T_F32 0
#define CE_T_BF16 1
#define CE_T_F16 2
#endif

/* C[M,N] = A[M,K] . B[N,K]^T, bf16 operands, fp32 accumulate, fused epilogue.
 * Replaces nn.Linear / MHA in_proj,out_proj / Conv2d(k=s=patch) forward and their
 * input-gradient GEMMs (model_clip.py:175-180, :188, :219, :230, :329, :415). */
int ce_gemm_nt(const void* A, long lda, const void* B, long ldb, int M, int N, int K, int epilogue,
               const float* bias, const void* resid, long ldr, void* out, long ldo, void* out2, long ldo2,
               const void* aux, long ldaux, void* stream);

/* out[Nn,Kk] (f32) += P[M,Nn]^T . Q[M,Kk]  (weight gradients; fp32 atomic accumulation, so the
 * caller zeroes `out` once per step).  splits<=0 picks the M split that fills the chip. */
int ce_gemm_tn(const void* P, long ldp, const void* Q, long ldq, int M, int Nn, int Kk, float* out, long ldo,
               int splits, void* stream);
/* same, plus the bias gradient bias_grad[n] (f32 [Nn], nullable) += sum_m P[m,n] */
int ce_gemm_tn_bias(const void* P, long ldp, const void* Q, long ldq, int M, int Nn, int Kk, float* out, long ldo,
                    float* bias_grad, int splits, void* stream);
/* 1..CE_TN_MAX_GROUP weight-gradient problems sharing M in one launch (the four Linear layers of a residual block, or of
 * several consecutive blocks: with about one resident round of tiles the launch needs no M split, and an unsplit tile is
 * added by plain read-modify-write instead of float atomics) */
#define CE_TN_MAX_GROUP 36
int ce_gemm_tn_grouped(int count, const void* const* P, const long* ldp, const void* const* Q, const long* ldq, int M,
                       const int* Nn, const int* Kk, float* const* out, const long* ldo, int splits, void* stream);
/* the same with overwrite != 0: out = P^T Q (whatever out held is discarded; the caller need not zero it).  A step's FIRST
 * contribution to a weight gradient: an unsplit tile then stores its accumulators instead of adding them with float
 * atomics (memory-side, 1.3 TB/s chip-wide), and the step's zero-fill of these tensors (85 % of the gradient buffer) goes away.
 * The outputs of one call must not overlap. */
int ce_gemm_tn_grouped_ex(int count, const void* const* P, const long* ldp, const void* const* Q, const long* ldq, int M,
                          const int* Nn, const int* Kk, float* const* out, const long* ldo, int splits, int overwrite,
                          void* stream);

/* ---- fp8 (OCP e4m3) operand path (gemm_fp8.hip; BASELINE config 5, tensors as convert_weights model_clip.py:554-575) ----
 * q[r,:] (e4m3 bytes) = x[r,:] (bf16) * 2^e_r with the power of two that puts the row's amax into (224, 448],
 * scale[r] = 2^-e_r (1 for an all-zero row); exact scaling, so the bytes are reproducible anywhere; K <= 4096 */
int ce_quant_rows_fp8(const void* x, long ldx, void* q, long ldq, float* scale, int M, int K, void* stream);
/* the same quantisation for a table of matrices in ONE launch (the per-step requantisation of every block weight and
 * its transpose: 288 launches of a few microseconds each otherwise).  jobs live in device memory; tile_start = first
 * 4-row group of the job in the launch's grid; K <= 4096. */
typedef struct ce_quant_job {
    const void* src; void* dst; float* scale;
    long lds_; long ldd;         /* leading dimensions: src in bf16 elements, dst in bytes */
    int rows, cols;
    int group_start, pad_;
} ce_quant_job;
int ce_quant_rows_fp8_multi(const ce_quant_job* jobs_device, int njobs, int total_groups, void* stream);
/* C[m,n] = sa[m] * sb[n] * sum_k A8[m,k] * B8[n,k] (e4m3 operands, one fp32 scale per row of each, fp32 accumulate on
 * v_mfma_scale_f32_16x16x128_f8f6f4) with the fused epilogues of ce_gemm_nt (BF16, BIAS_BF16, BIAS_RESID_F32, BIAS_GELU,
 * GELUGRAD_BF16).  K % 128 == 0; lda/ldb in bytes (= elements). */
int ce_gemm_nt_fp8(const void* A8, long lda, const float* sa, const void* B8, long ldb, const float* sb, int M, int N,
                   int K, int epilogue, const float* bias, const void* resid, long ldr, void* out, long ldo, void* out2,
                   long ldo2, const void* aux, long ldaux, void* stream);
/* MX form of the same path (round 3): one E8M0 scale byte per row and 32 contraction values -- the block the scaled MFMA
 * applies natively, so quantisation can be done by whoever PRODUCES the operand, block by block, with no row-wide pass.
 * q [M,K] e4m3 bytes, scale8 [M, K/32] bytes (lds_ = bytes per scale row); the block's amax is mapped into (224, 448];
 * K % 32 == 0 (ce_gemm_nt_mx8: K % 128 == 0, scale rows K/32 bytes apart and 4-byte aligned). */
int ce_quant_mx_fp8(const void* x, long ldx, void* q, long ldq, void* scale8, long lds_, int M, int K, void* stream);
/* job table as ce_quant_rows_fp8_multi; job.scale points at the [rows, cols/32] byte array of the job */
int ce_quant_mx_fp8_multi(const ce_quant_job* jobs_device, int njobs, int total_groups, void* stream);
int ce_gemm_nt_mx8(const void* A8, long lda, const void* sa8, const void* B8, long ldb, const void* sb8, int M, int N, int K,
                   int epilogue, const float* bias, const void* resid, long ldr, void* out, long ldo, void* out2, long ldo2,
                   const void* aux, long ldaux, void* stream);
/* y = LayerNorm(x[rows[r]] or x[r]) over D columns, fp32 statistics (eps inside the sqrt).
 * y is bf16 (out_f32=0: the next GEMM's operand) or fp32 (ln_pre: the residual stream).
 * Writes mean/rstd [M] for the backward.  Replaces LayerNorm.forward, model_clip.py:157-163. */
int ce_layernorm_fwd(const float* x, long ldx, const int* rows, const float* w, const float* b, void* y, long ldy,
                     int out_f32, float* mean, float* rstd, int M, int D, float eps, void* stream);
/* the same with typed operands: x_type CE_T_F32 / CE_T_F16 (the stream), y_type CE_T_BF16 (GEMM operand) / CE_T_F32 /
 * CE_T_F16 (ln_pre writing the stream) */
int ce_layernorm_fwd_t(const void* x, int x_type, long ldx, const int* rows, const float* w, const float* b, void* y,
                       int y_type, long ldy, float* mean, float* rstd, int M, int D, float eps, void* stream);

/* the same plus -- q8 != NULL, y bf16 -- an e4m3 copy of the output with one fp32 scale per row, written from the registers
 * that hold the row: q8[r,:] and qscale[r] equal ce_quant_rows_fp8 of y[r,:] bit for bit (fp8 operand path: the quantisation
 * pass of the GEMM that consumes y disappears) */
int ce_layernorm_fwd_q8(const void* x, int x_type, long ldx, const int* rows, const float* w, const float* b, void* y,
                        int y_type, long ldy, float* mean, float* rstd, int M, int D, float eps, void* q8, long ldq,
                        float* qscale, void* stream);

/* dx_out[dst] = (dx_in ? dx_in[dst] : 0) + dLN(dy[r]); dst = rows ? rows[r] : r; dxb = bf16 copy
 * (nullable); dw/db (f32 [D]) accumulate atomically (caller zeroes once per step); dxsum (f32 [D],
 * nullable) += column sums of dx_out = the bias gradient of the Linear that produced this stream. */
int ce_layernorm_bwd(const void* dy, long lddy, int dy_f32, const float* x, long ldx, const int* rows,
                     const float* mean, const float* rstd, const float* w, const float* dx_in, float* dx_out,
                     long lddx, void* dxb, long lddxb, float* dw, float* db, float* dxsum, int M, int D,
                     void* stream);
/* the same with typed operands: dy CE_T_BF16 / CE_T_F32 / CE_T_F16 (a gradient stream), x CE_T_F32 / CE_T_F16, dx_in and
 * dx_out CE_T_F32 / CE_T_F16.  An fp16 gradient operand holds gradient * *gscale (gscale: DEVICE pointer to the scale of
 * this backward pass, ce_grad_scale; it is read back / stored in those units; may be NULL when no operand is fp16);
 * dxb, dw, db, dxsum are always in true units. */
int ce_layernorm_bwd_t(const void* dy, int dy_type, long lddy, const void* x, int x_type, long ldx, const int* rows,
                       const float* mean, const float* rstd, const float* w, const void* dx_in, int dxin_type,
                       void* dx_out, int dx_type, long lddx, void* dxb, long lddxb, float* dw, float* db, float* dxsum,
                       const float* gscale, int M, int D, void* stream);

/* the same plus -- q8 != NULL -- the e4m3 copy (+ per-row scales, ce_quant_rows_fp8's rule) of dxb, indexed like dxb */
int ce_layernorm_bwd_q8(const void* dy, int dy_type, long lddy, const void* x, int x_type, long ldx, const int* rows,
                        const float* mean, const float* rstd, const float* w, const void* dx_in, int dxin_type,
                        void* dx_out, int dx_type, long lddx, void* dxb, long lddxb, float* dw, float* db, float* dxsum,
                        const float* gscale, int M, int D, void* q8, long ldq, float* qscale, void* stream);

/* The same backward WITHOUT atomics on the parameter gradients: the launch's workgroups (ce_layernorm_bwd_blocks(M, D) of them) each
 * write their partial column sums -- d gamma | d beta | (want_dxsum) column sums of dx -- as one row of partials[blocks][3][D], and
 * ce_layernorm_fold adds the rows of any number of such launches into their destinations in ONE launch (dw += ..., db += ...,
 * dxsum += ...).  Why: every workgroup of a launch adds into the same 2-3 rows, float atomics on one address serialise at the memory
 * side, and that phase is 3.7 us of a 23 us launch; the tower backward (48 LayerNorms per ViT-B/32 tower pass) folds once at its end. */
int ce_layernorm_bwd_blocks(int M, int D);
int ce_layernorm_bwd_partials(const void* dy, int dy_type, long lddy, const void* x, int x_type, long ldx, const int* rows,
                              const float* mean, const float* rstd, const float* w, const void* dx_in, int dxin_type,
                              void* dx_out, int dx_type, long lddx, void* dxb, long lddxb, int want_dxsum,
                              const float* gscale, int M, int D, void* q8, long ldq, float* qscale, float* partials,
                              void* stream);
#define CE_LN_FOLD_MAX 64
typedef struct ce_ln_fold_job {
    const float* partials; /* device: [blocks][3][D] */
    float *dw, *db, *dxsum; /* device destinations (dxsum nullable) */
    int blocks, D;
} ce_ln_fold_job;
int ce_layernorm_fold(const ce_ln_fold_job* jobs /* HOST array; no two jobs of a call may share a destination */, int njobs, void* stream);

/* Self-attention core on the packed in-projection output qkv[B*L, 3*H*64] (bf16; q | k | v column
 * blocks, head h at columns h*64): o[B*L, H*64] = softmax(q k^T / 8 + causal?) v, lse[B*H*L] (f32)
 * saved for the backward.  L <= 128: one workgroup per (sample, head); longer sequences (ViT-B/16, ViT-L/14): tiled
 * over 64-key blocks with an online softmax.  Replaces the core of nn.MultiheadAttention as called at
 * model_clip.py:188 (mask from model_clip.py:377-384).
 * cu_seqlens (int32 [B+1], nullable): variable-length batch, sample b owns rows cu_seqlens[b] ..
 * cu_seqlens[b+1]-1 (at most L of them); NULL = dense, sample b owns rows b*L .. b*L+L-1.  lse stays [B,H,L]. */
int ce_attention_fwd(const void* qkv, long ld, void* o, long ldo, float* lse, const int* cu_seqlens, int B, int L,
                     int H, int causal, void* stream);
/* bias_grad (f32 [3*H*64], nullable) += column sums of dqkv (the in_proj bias gradient) */
int ce_attention_bwd(const void* qkv, long ld, const void* o, long ldo, const void* dout, long lddo,
                     const float* lse, void* dqkv, long lddq, float* bias_grad, const int* cu_seqlens, int B, int L,
                     int H, int causal, void* stream);
/* The same backward (L <= 128 only) WITHOUT atomics on the bias gradient: workgroup (b, h) stores its 192 column sums as
 * partials[b][j][h*64 + c] (f32 [B][3][H*64]; j = dq | dk | dv), zeros for an empty sample of a packed batch, so every entry is
 * written by every call and the buffer needs no memset.  It is ce_layernorm_fold's job format: one job with blocks = B, D = H*64,
 * dw = bias_grad, db = bias_grad + D, dxsum = bias_grad + 2 D adds the rows into the gradient, in a fixed order (the atomic form's
 * order varies from run to run).  dqkv is bit-identical to ce_attention_bwd's. */
int ce_attention_bwd_partials(const void* qkv, long ld, const void* o, long ldo, const void* dout, long lddo,
                              const float* lse, void* dqkv, long lddq, float* partials, const int* cu_seqlens, int B,
                              int L, int H, int causal, void* stream);
/* Variable-length batches of any length: the signatures of ce_attention_fwd / ce_attention_bwd, cu_seqlens required
 * (NULL is -EINVAL before any launch), L = the longest sample the launch is sized for, 1 .. 4096.  L <= 128 IS ce_attention_fwd /
 * ce_attention_bwd (same kernels, same bits).  Longer: the tiled kernels with per-sample lengths -- sample b's own length (at most L)
 * bounds its key and query blocks, loads, clamps and masks, so no load reaches into the next sample's rows; the grid stays
 * (blocks of L, B H) and a workgroup whose block starts at or past its sample's length returns at once, an empty sample's
 * workgroups all do.  lse and the backward's delta scratch stay [B, H, L]; rows past a sample's length are not written.  bias_grad
 * is accumulated with atomics as in the dense long path.  The profiler scope charges B L^2 as the short packed path does, not the
 * live sum of squares. */
int ce_attention_fwd_packed(const void* qkv, long ld, void* o, long ldo, float* lse, const int* cu_seqlens, int B, int L,
                            int H, int causal, void* stream);
int ce_attention_bwd_packed(const void* qkv, long ld, const void* o, long ldo, const void* dout, long lddo,
                            const float* lse, void* dqkv, long lddq, float* bias_grad, const int* cu_seqlens, int B, int L,
                            int H, int causal, void* stream);

/* ---- input side, bookkeeping (embed.hip) ---- */
/* image f32 [B,3,R,R] -> patch rows bf16 [B*(R/p)^2, k_padded], columns ordered (c, py, px) like the
 * flattened conv1.weight; columns >= 3*p*p are zero.  Conv2d(k=s=p), model_clip.py:219,235. */
int ce_im2col(const float* image, void* patches, int B, int resolution, int patch, int k_padded, void* stream);
/* x0[b,t,:] = (t==0 ? class_embedding : patch_out[b*(T-1)+t-1,:]) + positional_embedding[t,:]
 * (model_clip.py:237-242); the backward emits the bf16 patch-row gradient for the conv wgrad. */
int ce_vision_assemble(const float* patch_out, const float* cls, const float* pos, float* x0, int B, int tokens,
                       int D, void* stream);
int ce_vision_assemble_bwd(const float* dx0, void* dpatch, int B, int tokens, int D, void* stream);
/* ---- patch dropout (FLIP): the image tower trains on `keep` of the N = (R/p)^2 patches of every image ----
 * ce_patch_keep chooses them.  The choice is counter-based (no generator state; a pass can be replayed exactly).  With
 * fmix32 the murmur3 finaliser on uint32, shifts and multiplies mod 2^32:
 *     h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 * the key of patch t of sample s = sample0 + b (b the row in the pass), for seed S and draw d (all taken mod 2^32), is
 *     a = fmix32(S + 0x9E3779B9);  b' = fmix32(a ^ d);  c = fmix32(b' ^ s);  key = fmix32(c ^ t)
 * fmix32 is a bijection, so the keys of one sample are pairwise different; the kept set is the `keep` patches with the
 * smallest keys.  One launch writes keep_idx [B,keep] (the kept patches in ascending patch order) and, when `inv` is not
 * NULL, inv [B,N] (slot j of patch t in keep_idx, or -1 for a dropped patch).  1 <= keep <= N <= 4095. */
int ce_patch_keep(long seed, long draw, long sample0, int B, int N, int keep, int* keep_idx, int* inv, void* stream);
/* The kernels below clamp every index they read from keep_idx / inv into range: a bad device-side list cannot make them
 * read outside their buffers.
 * ce_im2col's rows for the kept patches only: patches [B*keep, k_padded], row b*keep+j bit-identical to row
 * b*N + keep_idx[b,j] of ce_im2col (same 16-byte path for patch 8 / 16 / 32, same generic path, same zero padding). */
int ce_im2col_rows(const float* image, const int* keep_idx, void* patches, int B, int keep, int resolution, int patch,
                   int k_padded, void* stream);
/* x0 [B, keep+1, D]:  x0[b,0,:] = class_embedding + positional_embedding[0,:];
 * x0[b,1+j,:] = patch_out[b*keep+j,:] + positional_embedding[1 + keep_idx[b,j],:].  N bounds the index.  Its patch-row
 * backward is ce_vision_assemble_bwd at tokens = keep+1. */
int ce_vision_assemble_rows(const float* patch_out, const int* keep_idx, const float* cls, const float* pos, float* x0,
                            int B, int N, int keep, int D, void* stream);
/* dx0 [B, keep+1, D] -> dpos [N+1, D]:  dpos[0,:] += sum_b dx0[b,0,:];
 * dpos[1+t,:] += sum_{b : inv[b,t] >= 0} dx0[b, 1+inv[b,t], :].  b ascends and no atomics are used: bit-identical run to
 * run.  A row that no sample kept is not touched. */
int ce_pos_embed_bwd_rows(const float* dx0, const int* inv, float* dpos, int B, int N, int keep, int D, void* stream);
/* x0[r,:] = token_embedding[ids[e],:] + positional_embedding[e % tokens,:], e = src_rows ? src_rows[r] : r
 * (model_clip.py:400-403).  src_rows selects the LIVE tokens of a packed batch: under the causal mask
 * (model_clip.py:377-384) the rows after a caption's EOT can influence neither its feature (taken at the EOT,
 * model_clip.py:415) nor any gradient, so the text tower runs on the rows up to each EOT only.  The backward
 * skips exact-zero gradient elements (they change nothing and would serialise on the padding id). */
int ce_token_embed(const int64_t* ids, const int* src_rows, const float* table, const float* pos, float* x0, long rows,
                   int tokens, int D, int vocab, void* stream);
/* the same writing x0 in element type x0_type (CE_T_F32 / CE_T_F16) */
int ce_token_embed_t(const int64_t* ids, const int* src_rows, const float* table, const float* pos, void* x0, int x0_type,
                     long rows, int tokens, int D, int vocab, void* stream);
int ce_token_embed_bwd(const int64_t* ids, const int* src_rows, const float* dx0, float* dtable, long rows, int D,
                       int vocab, void* stream);
/* packed batch: dpos[t,:] += sum_{b : len_b > t} dx0[cu_seqlens[b] + t, :]   (cu_seqlens int32 [n+1]) */
int ce_pos_embed_bwd_packed(const float* dx0, const int* cu_seqlens, float* dpos, int n, int tokens, int D,
                            void* stream);
/* out[i] (+)= sum_b x[b*slab + i], i < n  (positional / class embedding gradients) */
int ce_batch_reduce(const float* x, float* out, int B, long slab, long n, int accumulate, void* stream);
/* ---- the image tower's positional table on another patch grid (posembed.hip) ----
 * pos [g_in^2 + 1, D] -> out [g_out^2 + 1, D]:  out[0,:] = pos[0,:] (class token);
 *     out[1 + i g_out + j, :] = sum_a wy[i,a] (sum_b wx[j,b] pos[1 + a g_in + b, :]),
 * both sums in ascending index order in fp32, a zero weight skipped.  wy, wx: dense fp32 [g_out, g_in] in device memory, the
 * caller's (the separable antialiased bicubic weights of clip_event_amd/posembed.py: host arithmetic).  The backward is the
 * transpose in gather form, one thread per dpos element, no atomics: bit-identical run to run;
 *     dpos[1 + a g_in + b, :] (+)= sum_i wy[i,a] (sum_j wx[j,b] dout[1 + i g_out + j, :]),   dpos[0,:] (+)= dout[0,:];
 * accumulate = 0 stores, 1 adds.  1 <= g_in, g_out <= 63, D a multiple of 4, 16-byte aligned tables; nothing is allocated. */
int ce_pos_resample_fwd(const float* pos, int g_in, const float* wy, const float* wx, float* out, int g_out, int D,
                        void* stream);
int ce_pos_resample_bwd(const float* dout, int g_out, const float* wy, const float* wx, float* dpos, int g_in, int D,
                        int accumulate, void* stream);
/* ---- the text tower's positional table at another context length (posembed.hip) ----
 * pos [t_in, D] -> out [t_out, D]:  out[j,:] = w[2j] pos[i0[j],:] + w[2j+1] pos[min(i0[j] + 1, t_in - 1),:], the second term skipped
 * when its weight is zero (a unit row is a bit-exact copy).  i0 int32 [t_out] ascending, w fp64 [t_out][2]: the caller's, device
 * memory (clip_event_amd/posembed.py text_weights: host arithmetic).  Products and sum are formed in fp64 and rounded to fp32 once,
 * so out is the fp32 rounding of the host's fp64 W pos -- the table a checkpoint resized on the host carries.  The backward is the
 * transpose in gather form, no atomics, bit-identical run to run: native row i adds the run rows span[2i] .. span[2i+1] - 1 (int32
 * [t_in][2], the contiguous range whose i0 is i - 1 or i) in ascending order in fp64, each with the weight it gave row i;
 * accumulate = 0 stores, 1 adds to the old value before the one rounding.  Indices read from the tables are clamped into the
 * buffers.  1 <= t_in, t_out <= 1024, D a multiple of 4, 16-byte aligned pos / out / dout / dpos; nothing is allocated. */
int ce_pos_stretch_fwd(const float* pos, int t_in, const int* i0, const double* w, float* out, int t_out, int D, void* stream);
int ce_pos_stretch_bwd(const float* dout, int t_out, const int* i0, const double* w, const int* span, float* dpos, int t_in,
                       int D, int accumulate, void* stream);
/* out[n] += sum_m x[m,n]  (bias gradients; atomics) */
int ce_colsum_bf16(const void* x, long ld, float* out, int M, int N, void* stream);
/* fp32 master weight [R,C] -> bf16 copy [R,C] (nullable) and bf16 transposed copy [C,R] (nullable) */
int ce_cast_transpose(const float* w, void* w16, long ld16, void* w16t, long ld16t, int R, int C, void* stream);
int ce_cast_bf16(const float* x, void* y, long n, void* stream);
/* y[i] (dst_type) = x[i] (src_type) * mul, element types CE_T_F32 / CE_T_BF16 / CE_T_F16; n a multiple of 4 */
int ce_cast_t(const void* x, int src_type, void* y, int dst_type, float mul, long n, void* stream);
/* the same with the factor in DEVICE memory: y = x * *scale, or x / *scale with divide != 0 */
int ce_cast_scaled(const void* x, int src_type, void* y, int dst_type, const float* scale, int divide, long n, void* stream);
/* *scale = the power of two s with s * max|x| in (target / 2, target] (1 when x is all zero or not finite): the scale of an
 * fp16 gradient stream whose top-of-tower gradient is x (fp32, n elements).  Stores saturate at 65504, so 65504 / target is
 * the growth the gradient may see on its way down the tower (target 64: 1024x; measured x17-34 in the ViT-B/32 text tower).  scratch: CE_GRAD_SCALE_SCRATCH floats. */
#define CE_GRAD_SCALE_SCRATCH 256
int ce_grad_scale(const float* x, long n, float target, float* scratch, float* scale, void* stream);
/* Saturation telemetry of the fp16 streams.  The reference keeps both streams in fp32 (model_clip.py:190-200) and stops on a
 * non-finite loss (engine.py:79-82); an fp16 store that clamps at +-65504 produces neither an inf nor a NaN, so the clamp is
 * made visible instead: register a DEVICE buffer of two unsigned counters (NULL switches it off; one buffer per process = per
 * GPU).  From then on every LayerNorm launch adds to them, sticky until the caller zeroes the buffer:
 *   [0] forward stream: LayerNorm-forward (wave, lane) slots that read a residual-stream element at the fp16 limit -- every
 *       stream row passes through a LayerNorm forward before anything else reads it, so no clamped store escapes;
 *   [1] gradient stream: LayerNorm-backward slots whose output gradient * scale reached the limit (or was not finite)
 *       before the clamping store.
 * Non-zero means the step computed with a clipped activation / gradient: lower CE_GRAD_TARGET, or run the stream in fp32. */
int ce_stream16_set_counters(unsigned int* device_counters);
/* dst[r,c] += src[r,c] for c < cols (rows with different strides: real columns of a column-padded gradient) */
int ce_add_cols(const float* src, long lds, float* dst, long ldd, int rows, int cols, void* stream);
/* gather / scatter whole rows: dst[dst_rows?dst_rows[i]:i] = src[src_rows?src_rows[i]:i], 16-byte granules */
int ce_copy_rows(const void* src, long src_stride_bytes, const int* src_rows, void* dst, long dst_stride_bytes,
                 const int* dst_rows, int n, int row_bytes, void* stream);
/* dst (M rows) = zeros except dst[dst_rows[i]] = src[i], i < n; dst_rows strictly ascending.  One pass instead of a
 * memset + ce_copy_rows (the pruned last block's backward hands the gradients of the B consumed rows to kernels that take
 * the dense [M, width] layout). */
int ce_scatter_rows_zero(const void* src, long src_stride_bytes, void* dst, long dst_stride_bytes, const int* dst_rows, int n,
                         int M, int row_bytes, void* stream);
/* rows[r] = r*tokens + argmax_t ids[r,t]  (EOT gather index, model_clip.py:415; first maximum) */
int ce_eot_rows(const int64_t* ids, int* rows, long n, int tokens, void* stream);

/* ---- image preprocessing (preprocess.hip) ---- */
/* One entry per OUTPUT image (several may share a source: whole image + object patches, dataset_voa.py:195-233).
 * Geometry is torchvision's Resize(n)/CenterCrop(n) on the region (x0,y0,w,h) of an HWC uint8 RGB image; the host
 * fills it (clip_event_amd/preprocess.py).  row0/rows = the region rows the vertical pass reads. */
typedef struct {
    const unsigned char* src;  /* device pointer, HWC uint8 RGB */
    long pitch;                /* bytes per source row */
    int x0, y0, w, h;          /* region = image.crop((x0, y0, x0+w, y0+h)), inside the image */
    int ow, oh;                /* size after Resize(n): shorter side n */
    int left, top;             /* CenterCrop offsets in the resized image */
    int row0, rows;            /* first region row and row count needed by the n cropped output rows */
    long tmp_off;              /* byte offset of this output's [rows][n][3] block in the scratch buffer */
} ce_preproc_desc;
size_t ce_preprocess_table_bytes(int n_out, int n_px, int kmax);
/* out[o] (f32 [3,n,n]) = Normalize(ToTensor(CenterCrop(Resize(region_o, BICUBIC)))), clip.py:62-69, bit-exact with
 * Pillow's resampling.  kmax >= 2*ceil(2*max_scale)+1 taps; table = ce_preprocess_table_bytes(); tmp = sum of
 * rows*n*3 bytes; mean/std = HOST pointers to 3 floats. */
int ce_preprocess(const ce_preproc_desc* descs_device, int n_out, int n_px, int kmax, int max_rows, void* table,
                  void* tmp, float* out, const float* mean, const float* std, void* stream);

/* ---- training augmentation (preprocess.hip) ---- */
/* What follows the crop + resize of one OUTPUT, in torchvision's order: RandomHorizontalFlip, ColorJitter (an op list in
 * its drawn order), RandomGrayscale.  The arithmetic is Pillow's (Blend.c, Convert.c), bit for bit. */
enum { CE_AUG_BRIGHTNESS = 0, CE_AUG_CONTRAST = 1, CE_AUG_SATURATION = 2, CE_AUG_HUE = 3 };
typedef struct {
    int flip;          /* 0/1: mirror left-right */
    int grey;          /* 0/1: replace the three channels by the luma, after the ops */
    int n_ops;         /* 0..4 */
    int op[4];         /* CE_AUG_*; contrast at most once */
    float factor[4];   /* >= 0: the enhancement factor (1 = unchanged); for hue the integer shift 0..255 of the 8-bit H */
} ce_augment_desc;
/* table, per-output luma sums, 8-bit n x n x 3 images and the pass-1 scratch (tmp_bytes = sum of rows*n*3) in one block */
size_t ce_augment_workspace_bytes(int n_out, int n_px, int kmax, long tmp_bytes);
/* out[o] (f32 [3,n,n]) = Normalize(ToTensor(grey(ops(flip(Resize(region_o -> n x n, BICUBIC)))))).  descs: as for
 * ce_preprocess with ow = oh = n_px and left = top = 0 (RandomResizedCrop: the region is the crop box; it may be smaller
 * than n_px).  augs_device / augs_host: the same n_out records on the device and on the host (the host copy is checked
 * and decides whether the contrast reduction is launched at all).  The contrast mean is an integer sum per output, so the
 * result does not depend on the launch shape; the sums are zeroed by the library's own kernels.  n_px <= 2896. */
int ce_augment(const ce_preproc_desc* descs_device, const ce_augment_desc* augs_device, const ce_augment_desc* augs_host,
               int n_out, int n_px, int kmax, int max_rows, void* workspace, float* out, const float* mean, const float* std,
               void* stream);

/* ---- contrastive head (head.hip) ---- */
int ce_l2norm_fwd(const float* f, long ldf, float* y, long ldy, float* inv_norm, int n, int E, void* stream);
int ce_l2norm_bwd(const float* dy, long lddy, const float* y, long ldy, const float* inv_norm, float* df, long lddf,
                  int n, int E, int accumulate, void* stream);
/* C[m,n] = alpha' * sum_k A[m*sam+k*sak] * B[k*sbk+n*sbn] + beta*C; alpha' = alpha * (alpha_ptr ?
 * (alpha_exp ? exp(*alpha_ptr) : *alpha_ptr) : 1).  fp32; logits and their gradients. */
int ce_sgemm(const float* A, long sam, long sak, const float* B, long sbk, long sbn, float* C, long ldc, int M,
             int N, int K, const float* alpha_ptr, float alpha, int alpha_exp, float beta, void* stream);
/* mean cross-entropy over the selected rows (sel = index_pos or NULL): *loss += mean(lse - logit[label]) */
int ce_xent_fwd(const float* logits, long ld, const int64_t* labels, const int64_t* sel, float* row_lse,
                float* loss, int nrows, int C, void* stream);
int ce_xent_bwd(const float* logits, long ld, const int64_t* labels, const int64_t* sel, const float* row_lse,
                const float* grad, float* dlogits, long ldd, int nrows, int C, void* stream);
/* the multi-positive cross entropy on materialised logits [., C], one wave per selected row (sel = index_pos or NULL): column c
 * is a positive of row src when kgroup[c] == qgroup[src] >= 0; row_lse / row_invpos [nrows] (1 / positives, 0 without) are kept
 * for the backward; *loss += (1/nrows) sum over rows with a positive of (lse - mean of the positives' logits);
 * dlogits[src, c] = grad / nrows (softmax_c - [c positive] invpos), zeros for a row without positives (rows not selected untouched) */
int ce_multipos_xent_fwd(const float* logits, long ld, const int64_t* qgroup, const int64_t* kgroup, const int64_t* sel,
                         float* row_lse, float* row_invpos, float* loss, int nrows, int C, void* stream);
int ce_multipos_xent_bwd(const float* logits, long ld, const int64_t* qgroup, const int64_t* kgroup, const int64_t* sel,
                         const float* row_lse, const float* row_invpos, const float* grad, float* dlogits, long ldd, int nrows, int C,
                         void* stream);
/* soft-target cross entropy over the selected rows: *loss += mean_r (lse(x_r) - sum_c softmax(t_r)_c x_r,c), x = logits,
 * t = teacher_logits (a constant; same shape, own leading dimension); row_lse / row_lse_t [nrows] are kept for the backward,
 * dlogits[src, c] = grad / nrows (softmax(x)_c - softmax(t)_c) (rows not selected untouched) */
int ce_soft_xent_fwd(const float* logits, long ld, const float* teacher_logits, long ldt, const int64_t* sel, float* row_lse,
                     float* row_lse_t, float* loss, int nrows, int C, void* stream);
int ce_soft_xent_bwd(const float* logits, long ld, const float* teacher_logits, long ldt, const int64_t* sel,
                     const float* row_lse, const float* row_lse_t, const float* grad, float* dlogits, long ldd, int nrows,
                     int C, void* stream);
int ce_dot(const float* a, const float* b, long n, float* out, void* stream);
/* per-instance logits_per_image (model_clip.py:509-521): lpi[b,k] = exp(*logit_scale) <In[b], Tn[b*K+k]> */
int ce_instance_logits(const float* In, const float* Tn, const float* logit_scale, float* lpi, int B, int K, int E,
                       void* stream);
int ce_instance_logits_bwd(const float* dlpi, const float* In, const float* Tn, const float* logit_scale, float* dIn,
                           float* dTn, int B, int K, int E, void* stream);
/* mean-reduced elementwise losses: mode 0 = BCEWithLogits, mode 1 = KLDiv (model_clip.py:626-629) */
int ce_elem_loss_fwd(const float* x, const float* y, long n, int mode, float* loss, void* stream);
int ce_elem_loss_bwd(const float* x, const float* y, long n, int mode, const float* grad, float* dx, void* stream);

/* ---- optimiser (optim.hip): clip_grad_norm_(.,max_norm) + Adam(L2 weight decay), engine.py:89-90 ---- */
int ce_sumsq(const float* g, long n, float* out, void* stream);
/* base[table[2b] .. table[2b+1]) = 0 for b < nchunks (element offsets, multiples of 4, in DEVICE memory): the gradient
 * zero-fill of a step restricted to the tensors that are accumulated into (ce_tower_desc.wgrad_overwrite) */
int ce_zero_segments(float* base, const long* table_device, int nchunks, void* stream);
/* p_bf16 (nullable): bf16 mirror of the updated parameters, same flat layout (the GEMM operand copies).  -EINVAL for step < 1,
 * n <= 0 and p, g, m or v NULL -- every step entry point below refuses NULL p / g / state buffers (and, in the tile and group forms,
 * NULL p_bf16) before any launch */
int ce_adam_step(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* sumsq, float max_norm,
                 float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* dst[c][r] = src[r][c] (bf16, dense) for a device table of matrices in one launch; tile_start = running
 * count of 64x64 tiles (jobs sorted by it) */
typedef struct ce_transpose_job {
    const void* src;
    void* dst;
    int rows, cols, tile_start, pad_;
} ce_transpose_job;
int ce_multi_transpose_bf16(const ce_transpose_job* jobs_device, int njobs, int total_tiles, void* stream);
/* clip + Adam (ce_adam_step's arithmetic, element for element) in a form that also leaves the TRANSPOSED bf16 copies of the weight
 * matrices behind: `jobs` lists matrices whose `src` points into the flat bf16 mirror `p_bf16` (same offset in p / g / m / v) and whose
 * `dst` receives W^T ([cols][rows]; rows, cols multiples of 8); one 64 x 64 tile per workgroup, `total_tiles` as for
 * ce_multi_transpose_bf16.  `segments` = [lo, hi) element ranges (multiples of 4, at most 2048 long: one workgroup each) of everything that is not one
 * of those matrices.  Replaces ce_adam_step + the ce_multi_transpose_bf16 pass of the next step (engine.py:87-95). */
int ce_adam_step_tiles(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                       int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* clip_grad_norm_(.,max_norm) + torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov).step(), engine.py:89-90 with
 * engine.py:136-140's optimiser: g = g * coef (coef as ce_adam_step: min(1, max_norm / (sqrt(*sumsq) + 1e-6)), 1 when sumsq is NULL),
 * g += weight_decay * p, buf = first_step ? g : momentum * buf + (1 - dampening) * g, p -= lr * (nesterov ? g + momentum * buf : buf);
 * with momentum == 0 the update is g, and buf may be NULL (it is neither read nor written).  first_step: no momentum buffer exists
 * yet (torch keeps no step counter): buf is overwritten.  p_bf16 as for ce_adam_step.  -EINVAL for n <= 0, momentum < 0, nesterov
 * with momentum <= 0 or dampening != 0 (torch's rule), buf == NULL with momentum > 0. */
int ce_sgd_step(float* p, const float* g, float* buf, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                float momentum, float dampening, float weight_decay, int nesterov, int first_step, void* stream);
/* the same update, element for element, in ce_adam_step_tiles' form (jobs / segments as there): also writes the W^T copies */
int ce_sgd_step_tiles(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                      int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm, float lr,
                      float momentum, float dampening, float weight_decay, int nesterov, int first_step, void* stream);
/* ---- partial fine-tuning: a gradient norm and an update over TABLES of what is trainable, with parameter groups ----
 * out += sum of g^2 over the [lo, hi) element ranges of `table_device` (2 x nchunks longs in DEVICE memory; multiples of 4, at
 * most 65536 long: one workgroup each, ce_sumsq's rounding chain per chunk).  Nothing outside the table is read: the gradient
 * slices of frozen parameters may hold anything. */
int ce_sumsq_segments(const float* g, const long* table_device, int nchunks, float* out, void* stream);
/* one parameter group: its learning rate and weight decay; decoupled != 0 (Adam only) = AdamW: p *= 1 - lr * weight_decay before the
 * update and no decay term in the gradient */
typedef struct ce_optim_group {
    float lr, weight_decay;
    int decoupled, pad_;
} ce_optim_group;
/* ce_adam_step_tiles / ce_sgd_step_tiles with per-group lr / weight_decay: `groups` is a HOST array of 1 <= ngroups <= 8 entries,
 * passed into the kernels by value.  A tile job names its group in ce_transpose_job.pad_, segment i in segment_group[i] (DEVICE
 * memory; NULL: every segment is of group 0); an id outside [0, ngroups) is taken as ngroups - 1.  What is in no table (a frozen
 * range) is neither read nor written: masters, state, bf16 mirror and W^T copy stay as they are.  One group that is not decoupled
 * gives ce_*_step_tiles' bits.  -EINVAL for ngroups outside 1..8, groups == NULL, empty tables, a decoupled group with SGD, and
 * whatever the ungrouped entry points refuse. */
int ce_adam_step_groups(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                        int total_tiles, const long* segments_device, int nsegments, const int* segment_group, const float* sumsq,
                        float max_norm, const ce_optim_group* groups, int ngroups, float beta1, float beta2, float eps, int step,
                        void* stream);
int ce_sgd_step_groups(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                       int total_tiles, const long* segments_device, int nsegments, const int* segment_group, const float* sumsq,
                       float max_norm, const ce_optim_group* groups, int ngroups, float momentum, float dampening, int nesterov,
                       int first_step, void* stream);
/* ---- weight EMA: every step entry point above with an exponential moving average of the weights carried along ----
 * `ema` (fp32, the flat layout of p) is one more stream of the same traversal: ema += ema_rate * (p_new - ema), ema_rate = 1 - decay,
 * in torch's lerp_ form (fma(p_new - ema, ema_rate, ema) below 0.5, p_new - (p_new - ema) (1 - ema_rate) from 0.5 on: ema_rate 1
 * copies), from the fp32 master exactly as the update wrote it.  p, the state, the bf16 mirror and the W^T copies get the bits of the
 * entry point without _ema; all forms give the same bits in ema.  In the grouped forms, what is in no table is neither read nor
 * written in ema.  -EINVAL for ema == NULL, ema_rate outside (0, 1], and whatever the parent refuses. */
int ce_adam_step_ema(float* p, const float* g, float* m, float* v, void* p_bf16, long n, const float* sumsq, float max_norm,
                     float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* ema, float ema_rate,
                     void* stream);
int ce_adam_step_tiles_ema(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                           int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm, float lr,
                           float beta1, float beta2, float eps, float weight_decay, int step, float* ema, float ema_rate,
                           void* stream);
int ce_adam_step_groups_ema(float* p, const float* g, float* m, float* v, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                            int total_tiles, const long* segments_device, int nsegments, const int* segment_group, const float* sumsq,
                            float max_norm, const ce_optim_group* groups, int ngroups, float beta1, float beta2, float eps, int step,
                            float* ema, float ema_rate, void* stream);
int ce_sgd_step_ema(float* p, const float* g, float* buf, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                    float momentum, float dampening, float weight_decay, int nesterov, int first_step, float* ema, float ema_rate,
                    void* stream);
int ce_sgd_step_tiles_ema(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                          int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm, float lr,
                          float momentum, float dampening, float weight_decay, int nesterov, int first_step, float* ema,
                          float ema_rate, void* stream);
int ce_sgd_step_groups_ema(float* p, const float* g, float* buf, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                           int total_tiles, const long* segments_device, int nsegments, const int* segment_group, const float* sumsq,
                           float max_norm, const ce_optim_group* groups, int ngroups, float momentum, float dampening, int nesterov,
                           int first_step, float* ema, float ema_rate, void* stream);
/* ---- Lion (Chen et al. 2023, "Symbolic Discovery of Optimization Algorithms") behind the same clip, in every form above ----
 * One state stream m (exp_avg; zeros are the initial state: no bias correction, no step counter, no first-step flag), the streams
 * and bytes of SGD with momentum.  Per element, in fp32, every product and sum rounded on its own (no multiply-add), in this order:
 *     gc = g * coef                        coef as ce_adam_step: min(1, max_norm / (sqrt(*sumsq) + 1e-6)), 1 when sumsq is NULL
 *     c  = beta1 * m + (1 - beta1) * gc    two products, one sum
 *     u  = (c > 0) - (c < 0)               the sign; 0 for c == 0, and 0 for a NaN c (both comparisons are false: the master then
 *                                          moves by the decay alone, and m becomes NaN)
 *     p  = p - (lr * weight_decay) * p     decoupled decay, always; skipped, bit for bit, when lr * weight_decay == 0
 *     p  = p - lr * u                      the master moves by exactly lr
 *     m  = beta2 * m + (1 - beta2) * gc    from the OLD m, after c was formed
 * 1 - beta1, 1 - beta2 and lr * weight_decay are rounded once to fp32.  All forms give the same bits; p_bf16, jobs, segments,
 * segment_group and groups are those of the Adam / SGD forms.  In the grouped form lr and weight_decay come from the group and
 * ce_optim_group.decoupled is IGNORED (Lion's decay is decoupled whatever it says); one group gives ce_lion_step_tiles' bits.
 * -EINVAL, each with a message of its own, for n <= 0 (flat), m == NULL, beta1 or beta2 outside [0, 1), lr < 0 or weight_decay < 0
 * (of any group), and for what the SGD form refuses: empty tables, ngroups outside 1..8, groups == NULL, p / g / p_bf16 NULL; the
 * _ema forms (as above: ema += ema_rate * (p_new - ema) in the same traversal) also for ema == NULL and ema_rate outside (0, 1]. */
int ce_lion_step(float* p, const float* g, float* m, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                 float beta1, float beta2, float weight_decay, void* stream);
int ce_lion_step_tiles(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                       int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm, float lr,
                       float beta1, float beta2, float weight_decay, void* stream);
int ce_lion_step_groups(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                        int total_tiles, const long* segments_device, int nsegments, const int* segment_group, const float* sumsq,
                        float max_norm, const ce_optim_group* groups, int ngroups, float beta1, float beta2, void* stream);
int ce_lion_step_ema(float* p, const float* g, float* m, void* p_bf16, long n, const float* sumsq, float max_norm, float lr,
                     float beta1, float beta2, float weight_decay, float* ema, float ema_rate, void* stream);
int ce_lion_step_tiles_ema(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                           int total_tiles, const long* segments_device, int nsegments, const float* sumsq, float max_norm, float lr,
                           float beta1, float beta2, float weight_decay, float* ema, float ema_rate, void* stream);
int ce_lion_step_groups_ema(float* p, const float* g, float* m, void* p_bf16, const ce_transpose_job* jobs_device, int njobs,
                            int total_tiles, const long* segments_device, int nsegments, const int* segment_group, const float* sumsq,
                            float max_norm, const ce_optim_group* groups, int ngroups, float beta1, float beta2, float* ema,
                            float ema_rate, void* stream);
/* a[i] <-> b[i] for i < n, and a_bf16[i] = bf16(new a[i]) (ce_cast_bf16's rounding): the masters and their average change places
 * and the bf16 mirror follows, in one pass.  a, b 16-byte aligned, a_bf16 8-byte aligned, a != b.  Calling it twice restores both. */
int ce_swap_cast_bf16(float* a, float* b, void* a_bf16, long n, void* stream);

/* ---- low-rank adapters in the merged-operand form (lora.hip) ----
 * An adapted matrix W0 [rows = out, cols = in] (fp32 master, frozen) has two fp32 parameters A [rank, cols] and B [rows, rank];
 * the towers run on bf16(W0 + scale * B A) and hand back the full fp32 weight gradient dW, from which the adapters' gradients
 * follow.  One job per adapted matrix; a table of jobs exists twice, as a HOST array (every call checks it: nothing is launched
 * on a table that could index out of bounds) and as a copy of the same bytes in DEVICE memory (what the kernels read).
 *   w0 fp32 [rows, cols]; w16 its bf16 operand copy; wt (nullable) the W^T copy [cols, rows], bf16; a, b the adapters;
 *   gw the dW slice; ga, gb the gradient slices of a and b.  All 16-byte aligned, rows and cols multiples of 8, 1 <= rank <= 64.
 *   tile_start / strip_start / ws_start: running counts over the table of 64 x 64 tiles ((rows+63)/64 * (cols+63)/64 per job), of
 *   64-row strips ((rows+63)/64) and of workspace floats (strips * rank * cols). */
typedef struct ce_lora_job {
    float* w0;
    void* w16;
    void* wt;
    const float* a;
    const float* b;
    const float* gw;
    float* ga;
    float* gb;
    int rows, cols, rank;
    float scale;
    int tile_start, strip_start;
    long ws_start;
} ce_lora_job;
/* Merge: t = sum_k b[o,k] a[k,i] (an fp32 fmaf chain in k order from 0, v_mfma_f32_32x32x2_f32), w = fmaf(scale, t, w0[o,i]),
 * w16[o,i] = bf16(w) (ce_cast_bf16's rounding), wt[i,o] the same bits; one 64 x 64 tile per workgroup.  w0 is read only unless
 * write_master != 0, which also stores w into w0 (folding the adapters into the masters for good).  ga, gb, gw are not touched. */
int ce_lora_merge(const ce_lora_job* jobs_host, const void* jobs_device, int njobs, int total_tiles, int write_master, void* stream);
/* Gradients: ga[k,i] = scale * sum_o b[o,k] gw[o,i], gb[o,k] = scale * sum_i gw[o,i] a[k,i], fp32 throughout, STORED (calling it
 * again gives the same bits).  One workgroup per 64-row strip reads its rows of gw once for both products: gb is complete there, the
 * strip's share of ga goes to `workspace` (ce_lora_grad_workspace_bytes(jobs_host, njobs) bytes, 16-byte aligned) and a second
 * launch adds the strips in ascending order.  No atomics: the same inputs give the same bits. */
int ce_lora_grad(const ce_lora_job* jobs_host, const void* jobs_device, int njobs, int total_strips, void* workspace,
                 size_t workspace_bytes, void* stream);
/* host arithmetic; 0 for a table the calls above would refuse */
size_t ce_lora_grad_workspace_bytes(const ce_lora_job* jobs_host, int njobs);

/* ---- transformer tower runner (tower.cpp): the 12x ResidualAttentionBlock loop of
 * Transformer.forward (model_clip.py:171-211) and its backward, all launches issued from C++ ---- */
typedef struct ce_block_params {
    /* fp32 master parameters (reference state-dict tensors, model_clip.py:175-182) */
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    const float *b_qkv, *b_out, *b_fc, *b_proj;
    /* bf16 GEMM operands: w_* = [out,in] as stored by the reference, wt_* = [in,out] transposed copy */
    const void *w_qkv, *w_out, *w_fc, *w_proj;
    const void *wt_qkv, *wt_out, *wt_fc, *wt_proj;
    /* fp32 gradients, accumulated (+=) */
    float *g_ln1_w, *g_ln1_b, *g_ln2_w, *g_ln2_b;
    float *g_b_qkv, *g_b_out, *g_b_fc, *g_b_proj;
    float *g_w_qkv, *g_w_out, *g_w_fc, *g_w_proj;
    /* fp8 path (read only when ce_tower_desc.fp8 != 0): e4m3 copies of w_* ([out,in], scale per out row) and of
     * wt_* ([in,out], scale per in row), see ce_quant_rows_fp8 */
    const void *w8_qkv, *w8_out, *w8_fc, *w8_proj;
    const float *s8_qkv, *s8_out, *s8_fc, *s8_proj;
    const void *wt8_qkv, *wt8_out, *wt8_fc, *wt8_proj;
    const float *st8_qkv, *st8_out, *st8_fc, *st8_proj;
} ce_block_params;

typedef struct ce_tower_desc {
    int layers, width, heads, tokens, causal;
    const ce_block_params* blocks; /* host array [layers] of device pointers */
    int fp8;                       /* bit 0: forward Linear GEMMs on the fp8 path, bit 1: the input-gradient GEMMs too
                                    * (activations / gradients are quantised per row on the fly; weight gradients,
                                    * attention, LayerNorm and the residual stream are unchanged) */
    int stream16;                  /* 0: fp32 residual stream and gradient stream (x0 / x_out / dx / dx_sel are float);
                                    * 1: both in IEEE fp16 (CE_T_F16): x0, x_out, dx point at half data, the stash keeps half
                                    * x_mid / x_out, dx holds gradient * *grad_scale.  dx_sel stays float. */
    int wgrad_overwrite;           /* backward: != 0 = this call makes the step's FIRST contribution to the four weight
                                    * gradients g_w_* of every block it covers: they are written (ce_gemm_tn_grouped_ex), not
                                    * accumulated, and need not have been zeroed.  Bias / LayerNorm gradients always accumulate. */
    const float* grad_scale;       /* backward with stream16: DEVICE pointer to the power of two the fp16 gradient stream of this
                                    * pass is stored multiplied by (ce_grad_scale of the top-of-tower gradient) */
} ce_tower_desc;

/* bytes of activation stash + backward scratch for `batch` samples */
size_t ce_tower_workspace_bytes(const ce_tower_desc* d, int batch);
/* x_out[B*T, width] (f32) = blocks(x0[B*T, width] (f32)); stash kept in `workspace` for the backward;
 * x0 must stay valid until ce_tower_backward has run.
 * sel_rows (int32 [B], strictly ascending, flat row index of the ONE token per sample whose output is consumed: CLS for the
 * image tower, model_clip.py:256; EOT for the text tower, :415) selects the pruned mode: the last block's
 * out-projection and MLP run on those B rows only (the other rows of the last block's output are never read
 * by the reference either) and x_out is [B, width].
 * rows / cu_seqlens: a dense batch has rows = batch*tokens and cu_seqlens NULL; a packed batch (text tower,
 * see ce_token_embed) has rows = cu_seqlens[batch] <= batch*tokens activation rows, sample b owning rows
 * cu_seqlens[b] .. cu_seqlens[b+1]-1; sel_rows then index the packed rows. */
int ce_tower_forward(const ce_tower_desc* d, int batch, int rows, const int* cu_seqlens, const void* x0,
                     void* workspace, void* x_out, const int* sel_rows, void* stream);
/* The same forward when NO backward follows (inference; the features-only first pass of a micro-batched step): the launches of
 * ce_tower_forward in the same order with the same shapes, so x_out is bit-identical, but nothing is stashed -- every buffer
 * is reused from block to block (two stream-typed buffers for x, one each of h, qkv, o, g, LayerNorm statistics, lse, the
 * compact buffers of the pruned block, the fp8 scratch) and mlp.c_fc runs CE_EPI_BIAS_QGELU_BF16.  The workspace is
 * ce_tower_infer_workspace_bytes(d, batch): 22 (fp16 stream) or 26 (fp32) x width bytes per row, 26 / 30 with the fp8 scratch,
 * whatever d->layers is -- against 32-36 x width per row AND block plus 162 x width per row of backward rings.  x0 is not written. */
size_t ce_tower_infer_workspace_bytes(const ce_tower_desc* d, int batch);
int ce_tower_forward_infer(const ce_tower_desc* d, int batch, int rows, const int* cu_seqlens, const void* x0,
                           void* workspace, void* x_out, const int* sel_rows, void* stream);
/* dx (f32 [B*T, width]) = gradient w.r.t. x0.  Full mode (sel_rows NULL): dx holds the gradient w.r.t. x_out on
 * entry (in place).  Pruned mode: dx_sel (f32 [B, width]) is the gradient w.r.t. the [B, width] output and dx is
 * output only.  Parameter gradients are accumulated into the g_* buffers. */
int ce_tower_backward(const ce_tower_desc* d, int batch, int rows, const int* cu_seqlens, const void* x0,
                      void* workspace, void* dx, const int* sel_rows, const float* dx_sel, void* stream);
/* the same backward for blocks layer_hi .. layer_lo only (both inclusive, top-down); successive calls covering
 * layers-1 .. 0 with the same buffers equal one ce_tower_backward.  After the call that ends at block l the
 * gradients of every block >= l are final, so a data-parallel caller can start reducing them
 * (clip_event_amd/distributed.py) while the lower blocks still run. */
int ce_tower_backward_range(const ce_tower_desc* d, int batch, int rows, const int* cu_seqlens, const void* x0,
                            void* workspace, void* dx, const int* sel_rows, const float* dx_sel, int layer_hi,
                            int layer_lo, void* stream);

/* ---- optimal-transport alignment + region pooling (ot.hip) ---- */
/* dist[b] = trace(C_b T_b): cosine cost between txt[b] (M rows) and img[b] (N rows), IPOT plan
 * (beta, `iters` outer iterations, 1 inner) computed without gradient; pads are uint8 [B,M]/[B,N].
 * Strides in elements: batch stride, row stride (unit column stride).  T [B,N,M] and the inverse row
 * norms are kept for the backward.  model_ot.py:8-83; M,N <= 64. */
int ce_ot_fwd(const float* txt, long tsb, long tsr, const float* img, long isb, long isr,
              const unsigned char* txt_pad, const unsigned char* img_pad, float* dist, float* T, float* txt_inv,
              float* img_inv, int B, int M, int N, int D, float beta, int iters, void* stream);
/* dtxt [B,M,D], dimg [B,N,D] (dense) for upstream grad[b] on dist[b] (gradient through the cost only) */
int ce_ot_bwd(const float* txt, long tsb, long tsr, const float* img, long isb, long isr, const float* T,
              const float* txt_inv, const float* img_inv, const float* grad, float* dtxt, float* dimg, int B, int M,
              int N, int D, void* stream);
/* out[i,:] = mean(grid[img_i, x0:x1, y0:y1, :]); boxes int32 [nbox,5] = {img,x0,y0,x1,y1}
 * (model_clip.py:438-443; strides of the grid view in elements); backward adds into dense dgrid [B,g,g,E] */
int ce_bbox_pool_fwd(const float* grid, long sb, long s0, long s1, const int* boxes, float* out, int nbox, int E,
                     void* stream);
int ce_bbox_pool_bwd(const float* dout, const int* boxes, float* dgrid, int g, int nbox, int E, void* stream);

/* Fused contrastive head for the 'ce' criterion over the batch (model_clip.py:496-521 logits + :633-662 cross entropy)
 * that never forms the [nq, nk] logits matrix (336 MB at N = 4096, K = 5): q [.,E], k [nk,E] are L2-NORMALISED fp32
 * features (ce_l2norm_fwd), query r = row sel[r] of q (sel nullable: row r), its target column labels[sel[r]].
 *   fwd: lse[r] = log sum_c exp(s <q_r, k_c>), *loss += mean_r (lse[r] - s <q_r, k_label>), s = exp(*logit_scale);
 *        workspace = ce_infonce_workspace_bytes(nq) bytes of scratch.
 *   bwd: for the upstream scalar *grad: dq[sel[r],:] += s sum_c G[r,c] k_c, dk[c,:] += s sum_r G[r,c] q_r,
 *        *dlogit_scale += sum G[r,c] s <q_r,k_c>, G = grad/nq (softmax_r - onehot); dq / dk are gradients w.r.t. the
 *        normalised features (feed ce_l2norm_bwd) and must be zero-filled (or hold earlier contributions).
 * fp32 on v_mfma_f32_32x32x2_f32; E a multiple of 128, 128..1024. */
#define CE_INFONCE_MAX_SPLITS 64
size_t ce_infonce_workspace_bytes(int nq);
int ce_infonce_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                   const float* logit_scale, const int64_t* labels, float* lse, float* loss, void* workspace, void* stream);
int ce_infonce_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                   const float* logit_scale, const int64_t* labels, const float* lse, const float* grad, float* dq, float* dk,
                   float* dlogit_scale, void* stream);

/* Sigmoid pairwise loss (SigLIP) on the same sweep, one direction, with a logit bias; q, k, sel, labels as ce_infonce_fwd:
 *   x[r,c] = s <q_r, k_c> + b,  z[r,c] = +1 if c == labels[sel[r]] else -1,  s = exp(*logit_scale), b = *logit_bias
 *   fwd: *loss = -(1/nq) sum_r sum_c log sigma(z x)   (WRITTEN, not added: the workgroups' partials go to `workspace`,
 *        ce_sigmoid_head_workspace_bytes(nq, nk) bytes, and are summed in a fixed order -- the same inputs give the same bits)
 *   bwd: G[r,c] = -(*grad / nq) z sigma(-z x); dq[sel[r],:] += s sum_c G k_c, dk[c,:] += s sum_r G q_r,
 *        *dlogit_scale += sum G (x - b), *dlogit_bias += sum G; nothing is saved by the forward.  dq and dk as for ce_infonce_bwd.
 * fp32 on v_mfma_f32_32x32x2_f32; E a multiple of 128, 128..1024; nk < 2^24.  No allocation, no synchronisation. */
size_t ce_sigmoid_head_workspace_bytes(int nq, int nk);
int ce_sigmoid_head_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                        const float* logit_scale, const float* logit_bias, const int64_t* labels, float* loss, void* workspace,
                        void* stream);
int ce_sigmoid_head_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                        const float* logit_scale, const float* logit_bias, const int64_t* labels, const float* grad, float* dq,
                        float* dk, float* dlogit_scale, float* dlogit_bias, void* stream);

/* Group-id targets on the same sweep (several positives per query), one direction.  q, k, sel, nq, nk as ce_infonce_fwd;
 * qgroup holds one 64-bit id per query SOURCE row (query r reads qgroup[sel[r]]), kgroup one per key row.  Key c is a positive of
 * query r when kgroup[c] == qgroup[sel[r]] over all 64 bits AND the id is >= 0: a negative id belongs to no group.
 *   P(r) the positives of row r, n_r = |P(r)|, x[r,c] = s <q_r, k_c>
 *   fwd: lse[r] = log sum_c exp(x[r,c]); invpos[r] = 1 / n_r, 0 where n_r = 0;
 *        *loss += (1/nq) sum_{n_r > 0} (lse[r] - (1/n_r) sum_{c in P(r)} x[r,c]) -- ONE sweep counts and sums the positives next
 *        to the log-sum-exp; workspace = ce_multipos_head_workspace_bytes(nq) bytes.
 *   bwd: G[r,c] = grad/nq (exp(x - lse[r]) - [c in P(r)] invpos[r]), a row with n_r = 0 contributes nothing;
 *        dq, dk, *dlogit_scale from G as in ce_infonce_bwd.
 * With one positive per row this is ce_infonce_fwd/bwd.  nk < 2^24.  No allocation, no synchronisation. */
size_t ce_multipos_head_workspace_bytes(int nq);
int ce_multipos_head_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                         const float* logit_scale, const int64_t* qgroup, const int64_t* kgroup, float* lse, float* invpos,
                         float* loss, void* workspace, void* stream);
int ce_multipos_head_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                         const float* logit_scale, const int64_t* qgroup, const int64_t* kgroup, const float* lse,
                         const float* invpos, const float* grad, float* dq, float* dk, float* dlogit_scale, void* stream);
/* ce_sigmoid_head_fwd / _bwd with z[r,c] = +1 on every positive of the row (group ids as above) in place of one label; the
 * workspace is ce_sigmoid_head_workspace_bytes(nq, nk) and *loss is WRITTEN from partials summed in a fixed order. */
int ce_sigmoid_head_group_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                              const float* logit_scale, const float* logit_bias, const int64_t* qgroup, const int64_t* kgroup,
                              float* loss, void* workspace, void* stream);
int ce_sigmoid_head_group_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int E,
                              const float* logit_scale, const float* logit_bias, const int64_t* qgroup, const int64_t* kgroup,
                              const float* grad, float* dq, float* dk, float* dlogit_scale, float* dlogit_bias, void* stream);

/* Distillation loss on the same sweep, one direction: cross entropy of the student's softmax against a teacher's, the
 * logits of neither materialised.  q, k, sel, nq, nk as ce_infonce_fwd (student, width Es, s = exp(*logit_scale)); tq / tk are
 * the teacher's L2-normalised features with the SAME row layout as q / k (query r = row sel[r] of tq), width Et (may differ
 * from Es), st = exp(*teacher_logit_scale); the teacher is a constant.
 *   S = s <q_r, k_c>, T = st <tq_r, tk_c>, loss = (1/nq) sum_r (lse_s[r] - sum_c softmax_c(T)[r,c] S[r,c])
 *   fwd: lse_s, lse_t [nq][2] (each row's log-sum-exp as the pair (max, log sum): one float would not normalise a peaked softmax
 *        closely enough) and v [nq, Es] = sum_c softmax_c(T)[r,c] k_c are written for the backward -- v is an accumulation
 *        target and must be ZERO-FILLED by the caller; *loss is WRITTEN (row terms summed in index order: the same inputs
 *        give the same bits); workspace = ce_distill_head_workspace_bytes(nq) bytes.
 *   bwd: G = (*grad / nq)(softmax(S) - softmax(T)); dq[sel[r],:] += s sum_c G k_c, dk[c,:] += s sum_r G q_r (dense, pitch Es,
 *        zero-filled or holding earlier contributions, as for ce_infonce_bwd).  The logit_scale gradient is not produced
 *        here: sum G S = sum_r <q_r, dq_r> = sum_c <k_c, dk_c>, so ce_rowdot_sum over a feature matrix and the gradient
 *        buffer this entry filled gives it -- for a pair of directions accumulated into one buffer, both at once.
 * Es and Et multiples of 128 in 128..1024.  No allocation, no synchronisation. */
size_t ce_distill_head_workspace_bytes(int nq);
int ce_distill_head_fwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int Es,
                        const float* logit_scale, const float* tq, long ldtq, const float* tk, long ldtk, int Et,
                        const float* teacher_logit_scale, float* lse_s, float* lse_t, float* v, float* loss, void* workspace,
                        void* stream);
int ce_distill_head_bwd(const float* q, long ldq, const int64_t* sel, int nq, const float* k, long ldk, int nk, int Es,
                        const float* logit_scale, const float* tq, long ldtq, const float* tk, long ldtk, int Et,
                        const float* teacher_logit_scale, const float* lse_s, const float* lse_t, const float* v,
                        const float* grad, float* dq, float* dk, void* stream);
/* *out += sum_r <x_r, y_r> over n rows of E columns */
int ce_rowdot_sum(const float* x, long ldx, const float* y, long ldy, int n, int E, float* out, void* stream);

/* Scoring without the [nq, nk] logits matrix (retrieval.hip): best-k keys per query, log-sum-exp and the rank of one target,
 * on the similarity sweep of ce_infonce_fwd.  q [nq,E], keys [nk,E] are used as given (the caller normalises them:
 * ce_l2norm_fwd).  score(r, c) = s <q_r, keys_c>, s = exp(*logit_scale) (logit_scale nullable: s = 1).  Candidates are
 * ordered by score descending, then key index ascending.
 *   top_val / top_idx [nq,k]: the first k keys in that order, padded with -inf / -1 when nk < k;  1 <= k <= CE_TOPK_MAX
 *   lse [nq] (nullable): log sum_c exp(score(r, c))
 *   rank [nq] (nullable; needs target): 0-based position of key target[r] in that order; a target outside 0..nk-1 gives -1
 *        and is never dereferenced
 * Every score comes from one instruction sequence whatever its place in a tile, a split or the grid: bit-identical key rows
 * tie exactly, rank[r] < k implies top_idx[r, rank[r]] == target[r], and top_val / top_idx / rank do not depend on `splits`
 * (0 = chosen by the launcher so that few queries still fill the chip, else 1..CE_INFONCE_MAX_SPLITS, clamped to the number
 * of 32-key blocks).  workspace = ce_score_topk_workspace_bytes(nq, nk, k, splits) bytes of scratch (0 for arguments
 * ce_score_topk refuses).  fp32 on v_mfma_f32_32x32x2_f32; E a multiple of 128, 128..1024.  No allocation, no
 * synchronisation. */
#define CE_TOPK_MAX 16
size_t ce_score_topk_workspace_bytes(int nq, int nk, int k, int splits);
int ce_score_topk(const float* q, long ldq, int nq, const float* keys, long ldk, int nk, int E, const float* logit_scale,
                  const int64_t* target, int k, int splits, float* top_val, int64_t* top_idx, float* lse, int64_t* rank,
                  void* workspace, void* stream);

/* Small-batch contrastive head in three launches: feature normalisation, logits_per_image / logits_per_text over the batch
 * (model_clip.py:496-521), CriterionContrastive 'ce' with index_pos (model_clip.py:633-662) and the whole backward down to the raw
 * features, in fp32 -- for the sizes where the head between the towers' forward and backward is pure launch latency (config 2:
 * 256 x 256 logits, 21 launches / 200 us in head.hip's form).  1 <= nI, nT <= 1024, nsel <= nT, E <= 1024 and a multiple of 4.
 *   fi [nI,E], ft [nT,E] raw features; labels_i [nI] target column of image row i; sel [nsel] (nullable: rows 0..nsel-1) the text rows
 *   that carry a loss, labels_t [nT] the target column of every text row (row sel[r] uses labels_t[sel[r]], as ce_xent_fwd does).
 * ce_head_small_fwd fills `workspace` (ce_head_small_workspace_floats floats): normalised features, P = (softmax - onehot) / rows
 * of both directions and, at ce_head_small_scalars_offset, four floats {loss_i, loss_t, sum P_i * lpi, sum P_t * lpt}.
 * ce_head_small_bwd takes the upstream gradients of the two losses as DEVICE scalars (nullable = 0) and writes dfi, dft and
 * *dlogit_scale (nullable). */
size_t ce_head_small_workspace_floats(int nI, int nT, int nsel, int E);
size_t ce_head_small_scalars_offset(int nI, int nT, int nsel, int E);
int ce_head_small_fwd(const float* fi, const float* ft, int nI, int nT, int E, const float* logit_scale, const int64_t* labels_i,
                      const int64_t* labels_t, const int64_t* sel, int nsel, float* workspace, void* stream);
int ce_head_small_bwd(int nI, int nT, int nsel, int E, const float* logit_scale, const float* g_i, const float* g_t,
                      const int64_t* sel, const float* workspace, float* dfi, float* dft, float* dlogit_scale, void* stream);

/* Region / argument InfoNCE of the train_arg branch (model_clip.py:456-488) for every image of the batch in one
 * launch.  region / desc / label: f32 [R,E] rows grouped per image, image g owning rows offsets[g] .. offsets[g+1]-1 (at
 * most 16; max_rows = the largest group, checked on the host); label may be NULL when use_label = 0.  Adds
 *   loss_bbox += sum_g CE(s r^ d^T) [+ CE(s r^ l^T)],  loss_arg += sum_g CE(s d^ r^T) [+ CE(s l^ r^T)] [+ CE(s d^ l^T)]
 * (x^ = x/|x|, s = exp(*logit_scale), targets arange(n), mean over the n rows; the l terms with use_label, the last with
 * role_text).  The backward takes the upstream scalars g_bbox / g_arg (device) and writes dregion / ddesc / dlabel (the
 * caller zero-fills them) and adds the logit_scale gradient. */
int ce_region_nce_fwd(const float* region, const float* desc, const float* label, const int* offsets, int groups,
                      int max_rows, int E, const float* logit_scale, int use_label, int role_text, float* loss_bbox,
                      float* loss_arg, void* stream);
int ce_region_nce_bwd(const float* region, const float* desc, const float* label, const int* offsets, int groups,
                      int max_rows, int E, const float* logit_scale, int use_label, int role_text, const float* g_bbox,
                      const float* g_arg, float* dregion, float* ddesc, float* dlabel, float* dlogit_scale, void* stream);

/* ==================================================================================================================
 * CE_DIAG -- diagnostics: profiler, tuning hooks and lane-map probes.  Used by bench.py's instrumented pass, tools/ and
 * tests/; the product path (clip_event_amd/*.py) calls none of them.
 * ================================================================================================================== */
/* ---- optional profiler: HIP events on the launch stream around every launch, summed per kernel
 * class.  ce_profile_collect fills out[class][4] = {launches, total ms, algorithmic FLOPs, algorithmic
 * bytes} and resets.  Used by bench.py for the `roofline` object; off by default. ---- */
#define CE_PROF_NT_FAMILIES 8
enum {
    CE_PROF_GEMM_NT0 = 0, /* + CE_PROF_NT_FAMILIES * epilogue id (0..7; CE_EPI_BIAS_QGELU_BF16: CE_PROF_GEMM_NT_QGELU) + kernel family: 0 gemm_nt_kernel (128x128, register
                           * staged), 1 gemm_nt256_kernel<.,.,2> (160x128, 4 waves), 2 gemm_nt256_kernel<.,.,4> (256 columns,
                           * 8 waves), 3 gemm_nt32_kernel (160x256x32), 4 gemm_nt8_kernel (fp8), 5 gemm_nt160lw_kernel (160x256,
                           * loader waves), 6 gemm_nt160p_kernel (its persistent form), 7 gemm_nt_skinny_kernel (M <= 512) -- one class per
                           * rocprofv3 kernel row */
    CE_PROF_GEMM_TN = 64, CE_PROF_ATTN_FWD = 65, CE_PROF_ATTN_BWD = 66, CE_PROF_LN_FWD = 67, CE_PROF_LN_BWD = 68,
    CE_PROF_COLSUM = 69, CE_PROF_OTHER = 70, CE_PROF_GEMM_TN2 = 71 /* gemm_tn2_kernel; CE_PROF_GEMM_TN = gemm_tn3_kernel */,
    CE_PROF_GEMM_NT_QGELU = 72, /* + kernel family: the NT kernels with CE_EPI_BIAS_QGELU_BF16 (the ids up to 71 keep their meaning) */
    CE_PROF_NCLASS = 80
};
void ce_profile_enable(int on);
int ce_profile_collect(double* out, int max_classes);
int ce_profile_num_classes(void);
const char* ce_profile_class_name(int cls);

/* tuning hook (tools/, tests/), the only way to force an NT tile variant (bf16 path; the e4m3 path ignores it) -- 0 auto,
 * 3..8 rows/32 of the 256-column kernel, 32 = 160x256x32 two-workgroup kernel, 104 = 160x128 four-wave (203..205: with
 * 96/128/160-row tiles), 160 = three-stage ring, 161 = loader waves (one tile per workgroup), 162 = persistent loader waves
 * (163..165: with 96/128/160-row tiles); 1000..1999 = tile walk of the persistent kernel: 1000 XCD-owned chunks of
 * tiles_m / 8 row panels, 1001 launch-wide (default, or CE_NT_CHUNK), 1001 + n chunks of n */
void ce_gemm_nt_tune(int variant);
/* the two-height tile plan of the most recent NT launch (tests): row panels of the tall height (160 rows; e4m3: 128), height of
 * the others in 32-row units; 0, 0 when the launch used one height */
int ce_gemm_nt_last_plan(int* tall_panels, int* short_tm);
/* What the NT launch policy does with a problem under the process's current knobs (ce_gemm_nt_tune, ce_gemm_set_cu_budget,
 * ce_gemm_set_dynamic_tiles, the environment): pure host arithmetic, launches nothing, needs no GPU.  kernel: 0 gemm_nt_kernel
 * (128x128), 1 gemm_nt256_kernel<.,tm,2>, 2 gemm_nt256_kernel<.,tm,4>, 3 gemm_nt32_kernel, 4 gemm_nt160_kernel (ring),
 * 5 gemm_nt160lw_kernel<.,tm>, 6 gemm_nt160p_kernel<.,tm,.,ts> (persistent), 7 gemm_nt_skinny_kernel; tm / ts: tile heights in
 * 32-row units, ts > 0 = row panels tall_panels.. are 32 ts rows; tiles_m, tiles_n, tall_panels, tile_chunk: the kernel's tiling
 * arguments; workgroups, block, lds_bytes: the launch; fp8 != 0: the e4m3 launcher, whose taken == 0 means that it falls back
 * to gemm_nt8_kernel (every other field is then 0). */
typedef struct { int kernel, tm, ts, tall_panels, tiles_m, tiles_n, tile_chunk,
                 workgroups, block, lds_bytes, wants_tile_queue, taken; } ce_nt_plan;
int ce_gemm_nt_plan(int M, int N, int K, int epilogue, int fp8,
                    long lda, long ldb, long ldo, long ldo2, long ldaux, long ldr,
                    ce_nt_plan* out);
/* The same for the weight-gradient (TN) launcher: what ce_gemm_tn_grouped_ex(count, ..., M, Nn, Kk, ..., splits, overwrite)
 * launches.  knobs: the environment's weight-gradient switches (csrc/tn_plan.cpp names them) as values -- variant [3],
 * force_splits [0], depth [3, clamped to 1..3], rows [48 unless exactly 32], loader_waves [1]; NULL: the process's, read from
 * the environment once.  form: 0 gemm_tn_kernel (v1: one launch per problem, `workgroups` in all),
 * 1 gemm_tn2_kernel (v2, 128x128 tiles), 2 gemm_tn3_kernel<rows,stages>, 3 gemm_tn3lw_kernel<rows,stages> (v3, 256x256 tiles);
 * workgroups = tiles * splits, every split m_per_split rows (a multiple of 64); kernel_overwrites: unsplit 256x256 tiles store
 * `out`; zero_fill_first: the launcher zeroes `out` before the launch (overwrite on any other form); tiles_n, tiles_k, tile_end
 * (cumulative, padded with `tiles`): the tiling per problem. */
typedef struct { int variant, force_splits, depth, rows, loader_waves; } ce_tn_knobs;
typedef struct { int form, rows, stages, block, lds_bytes, workgroups, splits, m_per_split, depth,
                 kernel_overwrites, zero_fill_first, tiles, prof_class;
                 int tiles_n[CE_TN_MAX_GROUP], tiles_k[CE_TN_MAX_GROUP], tile_end[CE_TN_MAX_GROUP]; } ce_tn_plan;
int ce_gemm_tn_plan(int count, const int* Nn, const int* Kk, int M, int splits, int overwrite,
                    const ce_tn_knobs* knobs, ce_tn_plan* out);
/* How ce_tower_backward groups the weight gradients of n_blocks (1..64) residual blocks of `width`, M rows, into grouped TN
 * launches: group sizes top-down into sizes_out[n_blocks], returns their number.  extra_tiles: tiles already queued (they go
 * out with the first group); force_group: CE_WGRAD_GROUP (0: planned). */
int ce_tower_wgrad_cuts(int n_blocks, int width, int M, long extra_tiles, int force_group, int* sizes_out);
/* tuning hook (tools/ only): 0 auto, 4/5/6/8 = tile height (x32 rows) of the 256-column kernel, 105 = 160x128 tile */
void ce_gemm_nt_fp8_tune(int variant);

/* CU budget of the NT GEMM launch policies: every kernel of the family puts ONE 156 KiB workgroup on a CU and sizes its grid to
 * fill the chip exactly once, so a CU held by another stream's kernel (an RCCL channel during the gradient all-reduce,
 * train.py:222-225's DDP) makes the launch wait for a second round.  `cus` < 256 sizes the one-round and the persistent grids
 * for that many CUs and leaves the rest to whoever holds them; 0 restores the default (CE_GEMM_CUS, else 256).  Process-wide;
 * call between steps. */
int ce_gemm_set_cu_budget(int cus);
/* DYNAMIC tile lists in the persistent NT kernel (off by default; CE_NT_DYNAMIC=1 or this call; -1 = back to the environment's
 * choice): a workgroup's first tile is its static one, every further tile comes from a per-launch device counter, fetched by
 * one wave while the current tile is multiplied.  A workgroup the dispatcher could not place -- its CU is held by another
 * stream's kernel, e.g. an RCCL channel during the gradient all-reduce -- then finds the list empty when it starts instead of
 * holding the launch up for a whole static tile list (measured: 1.2-1.4x per launch beside a resident foreign workgroup). */
int ce_gemm_set_dynamic_tiles(int on);

/* "CU hog" (bench.py --cu-hog): `blocks` workgroups that each occupy one CU (96 KiB of LDS, 256 threads) for
 * `microseconds` of wall time and do nothing -- what RCCL's channel kernels take away from the GEMM grids during a gradient
 * all-reduce, so that the 8-GPU contention risk can be sized on one GPU.  Bounded spin: every wave exits when the time is up. */
int ce_cu_hog(int blocks, float microseconds, void* stream);
/* shader clock in MHz that the last hog's first workgroup saw over its lifetime (s_memtime ticks per 100 MHz s_memrealtime
 * tick): what the chip clocked at under the load that ran beside the hog.  Synchronises the device. */
double ce_cu_hog_clock_mhz(void);

/* Debug probes: raw MFMA / transposed-LDS-read lane maps (tests/test_hip_probes.py). */
int ce_probe_mfma(int shape, const void* a_frags, const void* b_frags, float* out, void* stream);
/* one v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3): a_frags / b_frags 64 lanes x 32 bytes, scale_a / scale_b 64 ints (E8M0 in
 * byte 0), out 64 lanes x 4 floats */
int ce_probe_mfma_scale(const void* a_frags, const void* b_frags, const int* scale_a, const int* scale_b, float* out, void* stream);
int ce_probe_tr16(const void* image, int n_elems, const int* byte_off, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIP_EVENT_HIP_H */
