/*
 * animate3d_hip.h — C-ABI of libanimate3d_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary of this project is the Python call surface of the reference's
 * `MVUNetMotionModel.forward` (animatediff/models/unet_motion_mv_model.py:633-867); the
 * host side (animate3d_amd/unet.py) mirrors that class.  Everything arithmetic below that
 * surface is executed by the entry points declared here: plain pointers, sizes and a HIP
 * stream, no torch types.  Each entry point names the reference call it replaces.
 *
 * Conventions
 *   - activations / weights: bf16 (uint16_t storage), row-major, last dim contiguous
 *   - bias / norm affine / statistics: fp32
 *   - images are NHWC, flattened to rows: row = ((b*H + y)*W + x), image batch order is
 *     the reference's (b n f) order (unet_motion_mv_model.py:767)
 *   - ld* = leading dimension (elements between consecutive rows)
 *   - every function returns 0 on success, a negative A3D_E* code on bad arguments, or a
 *     positive hipError_t from the launch.  Nothing here allocates or synchronises.
 *   - the Gaussian side of the 4D-SDS stage (splat rasterizer, deformation field, ARAP rigidity loss and its k-NN graph) is fp32
 *     at the interface, with no storage twins; the ARAP entry points keep their rotations and per-sample energies in fp64
 *     buffers that the caller allocates
 */
#ifndef ANIMATE3D_HIP_H
#define ANIMATE3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* a3d_stream_t; /* hipStream_t */

enum {
  A3D_OK = 0,
  A3D_EINVAL = -1,      /* shape / alignment precondition violated */
  A3D_EUNSUPPORTED = -2 /* e.g. head_dim not in {40, 80, 160} */
};

/* dtype codes for the two layout-conversion entry points */
enum { A3D_F32 = 0, A3D_BF16 = 1, A3D_F16 = 2 };

/* Library / build identification ("animate3d_hip gfx950 <n kernels>"). */
const char* a3d_version(void);

/* ------------------------------------------------------------------------------------
 * Row addressing for the attention kernels.  Sequence position s of attention group g
 * lives at tensor row
 *     row(g, s) = (g / gdiv) * ga + (g % gdiv) * gb + (s / seg_len) * seg_stride + s % seg_len
 * This expresses the reference's einops regroupings as addressing instead of copies:
 *   "(b n f) l c -> (b f) (n l) c"   (attention_processor.py:54,340,557):
 *        g = b*F + f ; gdiv = F, ga = n*F*L, gb = L, seg_len = L, seg_stride = F*L
 *   first-frame K/V (attention_processor.py:389-397): same with gb = 0
 *   text / IP tokens shared by the F frames of a video (unet_motion_mv_model.py:754,763):
 *        g = image index ; gdiv = F, ga = T, gb = 0, seg_len = T
 * ------------------------------------------------------------------------------------ */
typedef struct a3d_rowmap {
  int64_t gdiv, ga, gb;
  int64_t seg_len, seg_stride;
  int64_t ld; /* elements per row of the underlying [rows, ld] tensor */
} a3d_rowmap;

/* Y[M,N] = alpha * (X[M,K] · W[N,K]^T + bias[N] + rowbias[m / rb_div][N]) + beta * R[M,N]
 * Replaces every nn.Linear / 1x1 nn.Conv2d on the path (diffusers Attention.to_q/k/v/out,
 * the processors' to_*_i2v / to_*_sp / to_*_ip Linear layers attention_processor.py:162-166,
 * 322-323,490-493; Transformer2D/Temporal proj_in/out; FeedForward; TimestepEmbedding;
 * ResnetBlock2D.time_emb_proj / conv_shortcut) with the residual add, AlphaBlender mix
 * (attention_processor.py:709) and time-embedding broadcast fused as epilogues.
 * bias, rowbias, R may be NULL.  Requires K % 64 == 0, N % 4 == 0, 16-byte aligned rows.
 * `flags` (also of a3d_gemm_geglu / a3d_conv3x3; 0 = defaults) is a per-call launch parameter — the library keeps no tuning state:
 *   bits 0-7   A3D_GEMM_RESERVED_CUS: compute units the persistent kernel's grid leaves free for concurrently running kernels
 *              (the sharded path passes the CUs an in-flight RCCL all-gather needs; at least 32 CUs are always used);
 *   bits 8-9   kernel choice: 0 = automatic (persistent 256-row-tile kernel for the big token matrices; round 6: the LDS-DMA ring kernel
 *              with 128-row tiles for the small ones — UNet levels 2 / 3 of a multi-GPU rank, the 4D-SDS shape —; 128 x 128 register-staged
 *              tiles for ragged shapes), A3D_GEMM_TILE128 = always the register-staged 128 x 128 kernel, A3D_GEMM_RING = the ring kernel
 *              whenever the shape allows it (a3d_gemm only; falls back to the automatic choice otherwise).  All kernels walk K in the same order with
 *              the same epilogue arithmetic: bit-identical results (A/B measurements and the parity tests).  The fourth value of the
 *              field (0x300) names no kernel, and other bits must be zero (A3D_EINVAL). */
#define A3D_GEMM_RESERVED_CUS_MASK 0xff
#define A3D_GEMM_KERNEL_MASK 0x300
#define A3D_GEMM_TILE128 0x100
#define A3D_GEMM_RING 0x200
int a3d_gemm_bf16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                  const float* bias, const void* rowbias, int64_t rb_div, const void* R, int64_t ldr,
                  void* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, float alpha, float beta, int flags);

/* a3d_gemm with a caller-owned workspace for SPLIT-K (round 5).  The persistent kernel works on 256-row tiles: at the small token
 * matrices of UNet levels 2 / 3 (M <= 8192 at the 4D-SDS shape, animatemv_guidance.py:339-346) a launch is 32-160 tiles on 256 compute
 * units.  With a workspace the K-tiles of one output tile are dealt to up to 16 work items that leave fp32 partial accumulators in `ws`;
 * a second kernel adds them in index order (deterministic) and applies the epilogue.  Results agree with a3d_gemm to fp32 summation
 * order (NOT bit for bit: callers that compare runs bit for bit use a3d_gemm).  Two calls: first with ws_needed != NULL — nothing is
 * launched, *ws_needed receives the bytes a split launch of exactly this call would use (0: the shape does not split, call a3d_gemm) —
 * then with ws (16-byte aligned, >= that many bytes) and ws_needed == NULL.  The library still never allocates. */
int a3d_gemm_ws_bf16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                     const float* bias, const void* rowbias, int64_t rb_div, const void* R, int64_t ldr,
                     void* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, float alpha, float beta, int flags,
                     void* ws, int64_t ws_bytes, int64_t* ws_needed);

/* Y[M,N] = [X | X2] W^T + bias with the A operand in two pieces: contraction columns [0, K1) are read from X (row stride ldx), [K1, K) from
 * X2 (row stride ldx2) — the 1x1 shortcut convolution of an up-block ResnetBlock2D over torch.cat([hidden, skip], dim=1)
 * (unet_motion_mv_model.py:826-827 / diffusers CrossAttnUpBlockMotion) without materialising the concatenation (round 5).  Served by the
 * persistent kernel only: A3D_EUNSUPPORTED (M % 256 != 0, too few tiles, ldx / ldx2 / ldw not multiples of 64) means "concatenate and call
 * a3d_gemm".  K1 % 64 == 0, K % 64 == 0, N % 8 == 0, 16-byte aligned rows.  Bit-identical to a3d_gemm on the concatenated operand. */
int a3d_gemm2_bf16(a3d_stream_t stream, const void* X, int64_t ldx, const void* X2, int64_t ldx2, int64_t K1,
                   const void* W, int64_t ldw, const float* bias, void* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, int flags);

/* Same contraction with an fp32 result: Y[M,N] (float, row stride ldy floats) = alpha * (X W^T + bias).  For logits that must
 * not be rounded to bf16: the single-head 512-wide self-attention of the VAE mid block (diffusers AutoencoderKL, used by
 * pipeline.py:566-579 decode_latents) computes S = Q K^T / sqrt(512) with this, a3d_softmax_rows_f32_bf16, and two more GEMMs.
 * Requires K % 64 == 0, N % 8 == 0, 16-byte aligned rows. */
int a3d_gemm_f32out_bf16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                         const float* bias, float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, float alpha);

/* Fused feed-forward input projection + GEGLU (diffusers FeedForward.net[0] = GEGLU: proj, chunk(2), h * gelu(gate)):
 *   Y[M, N2/2][m, j] = (X·Wh^T + bh)[m, j] * gelu_erf((X·Wg^T + bg)[m, j])
 * W / bias rows must be INTERLEAVED in blocks of 32: rows [64b, 64b+32) = h rows [32b, 32b+32),
 * rows [64b+32, 64b+64) = gate rows [32b, 32b+32), so h and gate of one output column land in the same
 * wave tile and the 2x wider intermediate never goes to HBM.  N2 % 64 == 0, K % 64 == 0, 16-byte aligned rows and bias (the persistent
 * kernel fetches the bias by 16-byte LDS-DMA, as a3d_gemm does). */
int a3d_gemm_geglu_bf16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                        const float* bias, void* Y, int64_t ldy, int64_t M, int64_t N2, int64_t K, int flags);

/* 3x3 convolution, padding 1, NHWC, as an implicit GEMM (K = 9*Cin):
 *   Y[b, yo, xo, co] = bias[co] + rowbias[(row) / rb_div][co] + R[...]
 *                      + sum_{ky,kx,ci} X[b, yo*stride+ky-1, xo*stride+kx-1, ci] * Wp[co][ky][kx][ci]
 * up2x bit 0 first applies nearest 2x upsampling to X (diffusers Upsample2D) by addressing; bits 1 / 2 crop the upsampled
 * image by its last row / column, which is what F.interpolate(size = (2H-1, 2W-1), mode = "nearest") yields: the forced
 * upsample size of latents that are not multiples of 8 (unet_motion_mv_model.py:690-698, 831-837).
 * Replaces cuDNN conv2d in diffusers ResnetBlock2D.conv1/conv2, Downsample2D, Upsample2D and
 * conv_out (unet_motion_mv_model.py:271,859).  Requires Cin % 64 == 0, Cout % 4 == 0. */
int a3d_conv3x3_bf16(a3d_stream_t stream, const void* X, const void* Wp, const float* bias,
                     const void* rowbias, int64_t rb_div, const void* R, void* Y,
                     int B, int H, int W, int Cin, int Cout, int stride, int up2x, int flags);

/* a3d_conv3x3 with a split-K workspace (see a3d_gemm_ws_bf16): the 8 x 8 and 4 x 4 feature maps of the mid block (K = 9 Cin = 11 520 ... 23 040 over
 * 128 or fewer output tiles; cuDNN under nn.Conv2d picks a split-K algorithm there too).  Work items hold whole 64-channel slices. */
int a3d_conv3x3_ws_bf16(a3d_stream_t stream, const void* X, const void* Wp, const float* bias,
                        const void* rowbias, int64_t rb_div, const void* R, void* Y,
                        int B, int H, int W, int Cin, int Cout, int stride, int up2x, int flags,
                        void* ws, int64_t ws_bytes, int64_t* ws_needed);

/* The up-sampling convolution (a3d_conv3x3 with up2x = 1: exact 2H x 2W output, no crop) in its 2x2 PHASE FORM over weights folded at
 * pack time.  The nine taps of output pixel (2i + a, 2j + b) read only the 2x2 window of source pixels whose top-left one is
 * (i - 1 + a, j - 1 + b); taps that hit the same source pixel are summed once by the caller:
 *   Wf[p = 2a + b][co][(r, c)][ci] = sum_{ky in R_a(r), kx in R_b(c)} Wp[co][ky][kx][ci],  R_0(0) = {0}, R_0(1) = {1, 2}, R_1(0) = {0, 1}, R_1(1) = {2}
 *   Y[b, 2i + a, 2j + b', co] = bias[co] + sum_{r, c, ci} X[b, i - 1 + a + r, j - 1 + b' + c, ci] * Wf[p][co][(r, c)][ci]
 * (source pixels outside the image read zero) — 16 MACs per output pixel instead of 36.  Wf is [4, Cout, 4 Cin], contiguous, summed in
 * float64 and rounded ONCE to the storage type (animate3d_amd.hip_ops.fold_up2x_weights), so the result differs from a3d_conv3x3's by
 * that one rounding of the weights; with weights whose tap sums are exact it is bit-identical.  X [B H W, Cin], Y [B 2H 2W, Cout].
 * One launch of the persistent kernel walks all four phases; nothing else serves this entry point, so every shape that kernel does not
 * take is A3D_EINVAL (keep a3d_conv3x3 for it): B H W % 256 != 0, Cin % 64 != 0, Cout a multiple of neither 320 nor 256, an input of
 * 4 GB or more, pointers that are not 16-byte aligned.  It takes no row bias and no residual — the up-samplers have neither —: rowbias
 * and R must be NULL (A3D_EINVAL otherwise).  bias may be NULL.  flags: A3D_GEMM_RESERVED_CUS only (a kernel choice is A3D_EINVAL).
 * No split-K: the result does not depend on the grid. */
int a3d_conv3x3_up2x_folded_bf16(a3d_stream_t stream, const void* X, const void* Wf, const float* bias,
                                 const void* rowbias, const void* R, void* Y,
                                 int B, int H, int W, int Cin, int Cout, int flags);

/* softmax(Q K^T * scale) V per (group, head), flash-style (no score matrix in memory).
 *   O[row_o(g,s), h*D + d] = out_scale * attn(...)   (+ previous O contents if accumulate)
 * Replaces xformers.ops.memory_efficient_attention at attention_processor.py:103,233,268,
 * 405,416,656.  head_dim in {40, 80, 160} (the SD1.5 UNet levels) and 64 (CLIP text tower of pipeline.py:345-524).  K and V share
 * kmap.  `accumulate` is a per-call flag word: bit 0 (A3D_ATTN_ACCUMULATE): add to the previous O contents; bit 1
 * (A3D_ATTN_CAUSAL): causal mask (key s visible to queries >= s of its group; head_dim 64 / 160 only) — transformers'
 * CLIPTextModel causal attention; bit 2 (A3D_ATTN_EXACT): skip the max-free first pass of the LDS-DMA staged kernels (head_dim
 * 40 / 80, long aligned K/V) and run their exact running-maximum pass directly — the pass a workgroup otherwise re-runs after an
 * overflow; bit 3 (A3D_ATTN_PLAIN): use the generic kernel that serves the short / ragged shapes (parity tests, A/B timing).
 * Results agree to rounding in every mode. */
#define A3D_ATTN_ACCUMULATE 1
#define A3D_ATTN_CAUSAL 2
#define A3D_ATTN_EXACT 4
#define A3D_ATTN_PLAIN 8
int a3d_flash_attn_bf16(a3d_stream_t stream, const void* Q, const void* K, const void* V, void* O,
                        const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* omap,
                        int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len,
                        float scale, float out_scale, int accumulate);

/* a3d_flash_attn plus diagnostics of the LDS-DMA staged kernels (head_dim 40 / 80 on long aligned K/V): `counters` = 3 caller-zeroed
 * device words; [0] += workgroups sent straight to the exact pass by the fp16 spread vote, [1] += workgroups that discarded a max-free
 * result and re-ran exactly (overflow), [2] += workgroups launched.  Launches of the other kernels leave the words alone.  The reference has
 * no counterpart (xformers.ops.memory_efficient_attention, attention_processor.py:405,416,656, always keeps a running maximum); this
 * exists so that parity tests on peaked softmax inputs can assert how much of a launch left the fast path.  Same results as a3d_flash_attn. */
int a3d_flash_attn_counted_bf16(a3d_stream_t stream, const void* Q, const void* K, const void* V, void* O,
                                const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* omap,
                                int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len,
                                float scale, float out_scale, int accumulate, unsigned int* counters);

/* Two key sets in one launch, each with its own softmax:
 *   O = out_scale * attn(Q, K, V) + out_scale2 * attn(Q, K2, V2)   (+ previous O contents if accumulate)
 * Replaces the text-token attention, the per-adapter image-token attention and `hidden_states = hidden_states + scale * ip` of the
 * IPAdapter processor (attention_processor.py:233, 254-283) with ONE pass over Q and O.  head_dim 40 or 80 (A3D_EUNSUPPORTED otherwise:
 * the caller then issues two a3d_flash_attn calls, the second with accumulate). */
int a3d_flash_attn2_bf16(a3d_stream_t stream, const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O,
                         const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* kmap2, const a3d_rowmap* omap,
                         int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len, int64_t kv_len2,
                         float scale, float out_scale, float out_scale2, int accumulate);

/* Temporal (AnimateDiff) self-attention over the F frames of every (video, pixel, head):
 * rows of Q/K/V/O are ((v*F + f)*L + l).  Replaces the unfused
 * get_attention_scores + torch.bmm of attention_processor.py:630-636.  frames <= 32. */
int a3d_temporal_attn_bf16(a3d_stream_t stream, const void* Q, const void* K, const void* V, int64_t ldqkv,
                           void* O, int64_t ldo, int videos, int frames, int64_t L, int heads,
                           int head_dim, float scale);

/* The same attention when the FRAMES of a video are sharded over ranks (frame-parallel denoise step): this
 * rank holds queries (and writes outputs) only for frames [q_f0, q_f0 + q_frames), rows ((v*q_frames + f - q_f0)*L + l); K / V
 * are the all-gathered tensors, kv_frames_per_block frames per rank block: frame f of video v sits at row
 * (f / kv_frames_per_block) * kv_block_stride + (v*kv_frames_per_block + f % kv_frames_per_block)*L + l.
 * Per-query arithmetic is that of a3d_temporal_attn_bf16 (reference: attention_processor.py:630-636 over all F frames). */
int a3d_temporal_attn_sharded_bf16(a3d_stream_t stream, const void* Q, int64_t ldq, const void* K, const void* V, int64_t ldkv,
                                   void* O, int64_t ldo, int videos, int frames, int64_t L, int heads,
                                   int head_dim, float scale, int q_f0, int q_frames, int kv_frames_per_block,
                                   int64_t kv_block_stride);

/* GroupNorm over `rows` consecutive rows x (C/groups) channels per instance, optional SiLU.
 * 2-D GroupNorm: B = images, rows = H*W.  The motion module's 3-D GroupNorm over
 * (C/32, F, H, W) (diffusers TransformerTemporalModel.norm): B = videos, rows = F*H*W.
 * ws: fp32 scratch of a3d_group_norm_ws_floats(B, rows, groups) elements. */
int64_t a3d_group_norm_ws_floats(int B, int64_t rows, int groups);
int a3d_group_norm_bf16(a3d_stream_t stream, const void* X, void* Y, const float* gamma, const float* beta,
                        float* ws, int B, int64_t rows, int C, int groups, float eps, int silu);

/* Host-only query (touches no GPU): how a3d_group_norm_{bf16,f16} runs a one-source instance of this geometry.  The launch decides from the
 * same code.  out[7] = { fused, sg, nx, ny, threads, rmax, stream }:
 *   fused 1: one launch, a workgroup keeps a slab of `sg` whole groups in registers: `threads` threads = nx 16-byte chunk columns x ny row
 *            lanes (a thread owns rows ry, ry + ny, ...: at most rmax = 11 or 21 of them); stream 1: non-temporal accesses (a two-source
 *            input, a3d_group_norm2, never streams);
 *   fused 0: three launches (partial sums, finalize, apply) of blocks (nx = C / 8, ny) over 128-row chunks; sg = rmax = 0, stream = 1.
 * Returns A3D_EINVAL for a geometry a3d_group_norm refuses (or out == NULL), 0 otherwise. */
int a3d_group_norm_plan(int64_t rows, int C, int groups, int* out);

/* a3d_group_norm_bf16 over a TWO-SOURCE input: channels [0, Ca) of a row come from Xa ([B*rows, Ca]), channels [Ca, Ca + Cb) from Xb
 * ([B*rows, Cb]); Y is the normalised [B*rows, Ca + Cb] tensor.  norm1 of an up-block ResnetBlock2D over torch.cat([hidden, skip], dim=1)
 * (diffusers CrossAttnUpBlockMotion / UpBlockMotion, unet_motion_mv_model.py:826-827) without the concatenation pass (round 5).  A group may
 * straddle the two sources (1280 + 640 channels in 32 groups of 60); Ca % 8 == 0.  ws as for a3d_group_norm_bf16 with C = Ca + Cb. */
int a3d_group_norm2_bf16(a3d_stream_t stream, const void* Xa, int Ca, const void* Xb, int Cb, void* Y, const float* gamma,
                         const float* beta, float* ws, int B, int64_t rows, int groups, float eps, int silu);

/* The two halves of a3d_group_norm_bf16 for a norm whose instance is spread over ranks (the motion module's 3-D GroupNorm of
 * diffusers TransformerTemporalModel.norm under frame sharding): `sums` receives fp64 [B][groups][2] = (sum, sum of squares)
 * of this rank's rows; the caller all-reduces them over the frame group, forms (mean, rstd) as fp32 [B][groups][2] and hands
 * them to the apply half.  ws as above. */
int a3d_group_norm_sums_bf16(a3d_stream_t stream, const void* X, float* ws, double* sums, int B, int64_t rows, int C, int groups);
int a3d_group_norm_apply_bf16(a3d_stream_t stream, const void* X, void* Y, const float* gamma, const float* beta,
                              const float* stats, int B, int64_t rows, int C, int groups, int silu);

/* LayerNorm over C, with the positional-embedding adds of the motion-module processor fused:
 *   Y1[m] = LN(X[m]) + pe1[(m / pe1_div) % pe1_mod]     (pe1 may be NULL)
 *   Y2[m] = LN(X[m]) + pe2[(m / pe2_div) % pe2_mod]     (Y2 may be NULL)
 * (time_pos_embed attention_processor.py:583-584; SinePositionalEncoding2D :561-563).
 * X, Y1, Y2, gamma, beta, pe1 and pe2 are accessed 16 bytes at a time: one that is not 16-byte aligned is A3D_EINVAL. */
int a3d_layer_norm_bf16(a3d_stream_t stream, const void* X, void* Y1, void* Y2, const float* gamma,
                        const float* beta, int64_t M, int C, float eps,
                        const void* pe1, int64_t pe1_div, int64_t pe1_mod,
                        const void* pe2, int64_t pe2_div, int64_t pe2_mod);

/* Y[m, j] = X[m, j] * gelu_erf(X[m, N + j])   (diffusers GEGLU). N % 8 == 0. */
int a3d_geglu_bf16(a3d_stream_t stream, const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t M, int64_t N);

/* Y = X * sigmoid(X), n elements (n % 8 == 0). */
int a3d_silu_bf16(a3d_stream_t stream, const void* X, void* Y, int64_t n);

/* Elementwise activation on n elements (n % 8 == 0): mode 0 SiLU, 1 QuickGELU x * sigmoid(1.702 x) (transformers CLIPTextModel of
 * pipeline.py:345-524 encode_prompt), 2 exact GELU (CLIP ViT-H image encoder of pipeline.py:527-538 encode_image). */
int a3d_activation_bf16(a3d_stream_t stream, const void* X, void* Y, int64_t n, int mode);

/* Y[m] = [A[m, 0:Ca] | B[m, 0:Cb]]  (torch.cat([x, skip], dim=1) of the up blocks). */
int a3d_concat_bf16(a3d_stream_t stream, const void* A, int64_t Ca, const void* Bsrc, int64_t Cb, void* Y, int64_t M);

/* diffusers Timesteps(dim, flip_sin_to_cos=True, shift 0): Y[v] = [cos(t_v f_j) | sin(t_v f_j)],
 * fp32 math, bf16 out (unet_motion_mv_model.py:723-728). */
int a3d_timestep_embed_bf16(a3d_stream_t stream, const float* t, void* Y, int V, int dim);

/* sample [V, C, F, H, W] (dtype code) -> im2col rows [(V F) H W, 64] bf16 with
 * k = (ky*3 + kx)*C + c for k < 9*C, zero above (3x3, pad 1).  Folds the
 * permute/reshape of unet_motion_mv_model.py:767 and conv_in's patch gather. 9*C <= 64. */
int a3d_im2col_in(a3d_stream_t stream, const void* sample, int dtype, void* Y, int V, int C, int F, int H, int W);

/* Adjoint of a3d_im2col_in: dCol rows [(V F) H W, 64] bf16 (columns k >= 9*C ignored) -> fp32 dX [V, C, F, H, W] =
 * scale * col2im(dCol).  The input gradient of conv_in on the fp32 RGB image of the VAE encoder (4D-SDS,
 * animatemv_guidance.py:365-373); `scale` folds the 2 of imgs * 2 - 1 and the removal of a gradient scale.  9*C <= 64;
 * dCol 2-byte and dX 4-byte aligned (A3D_EINVAL otherwise). */
int a3d_im2col_in_bwd(a3d_stream_t stream, const void* dCol, float* dX, int V, int C, int F, int H, int W, float scale);

/* rows [(V F) H W, C] bf16 -> [V, C, F, H, W] in `dtype` (unet_motion_mv_model.py:862). */
int a3d_unpack_out(a3d_stream_t stream, const void* X, void* Y, int dtype, int V, int C, int F, int H, int W);

/* Row softmax of fp32 logits X[M, N] (row stride ldx floats) -> bf16 probabilities Y[M, N] (row stride ldy elements);
 * the softmax of diffusers' AttnProcessor in the VAE mid block.  N % 4 == 0. */
int a3d_softmax_rows_f32_bf16(a3d_stream_t stream, const float* X, int64_t ldx, void* Y, int64_t ldy, int64_t M, int64_t N);

/* Backward of a3d_softmax_rows_f32_bf16 (the VAE encoder's mid-block attention on the 4D-SDS input-gradient path):
 *   dS[m, n] = alpha * P[m, n] * (dP[m, n] - sum_j P[m, j] dP[m, j])
 * with P the bf16 probabilities the forward multiplied by V (row stride ldp elements), dP fp32 (row stride lddp floats), dS bf16 (row
 * stride ldds elements); the row sum is fp32.  N % 4 == 0, ldp / lddp / ldds multiples of 4 and >= N, P / dS 8-byte and dP 16-byte aligned. */
int a3d_softmax_rows_bwd_bf16(a3d_stream_t stream, const void* P, int64_t ldp, const float* dP, int64_t lddp, void* dS, int64_t ldds,
                              int64_t M, int64_t N, float alpha);

/* Planar fp32 channel mix y[b, o, :] = scale * sum_c w[o, c] x[b, c, :] + bias[o] for <= 8 channels: the VAE's 1x1
 * post_quant_conv together with the 1 / scaling_factor of pipeline.py:567 (decode_latents). */
int a3d_channel_mix_f32(a3d_stream_t stream, const float* X, const float* W, const float* bias, float* Y,
                        int B, int Cin, int Cout, int64_t HW, float scale);

/* CFG combine + DDIM step + first-frame re-pin, one elementwise pass (pipeline.py:1023-1031):
 *   eps = e_uncond + s (e_text - e_uncond) ; x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t)
 *   x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps ; frame 0 <- first_frame
 * fp32 tensors [n, C, F, H, W]; eps_pair is [2n, C, F, H, W] in (uncond, text) order. */
int a3d_cfg_ddim_step_f32(a3d_stream_t stream, const float* eps_pair, const float* x, const float* first_frame,
                          float* x_prev, int64_t n, int C, int F, int64_t HW, float guidance,
                          float alpha_t, float alpha_prev);


/* ---------------------------------------------------------------------------------------------------------------------
 * Training path: the backward kernels behind `loss.backward()` of train.py:576-590 and the fused
 * optimiser step of train.py:583-596.  The matrix products of the backward pass (dgrad = dY W, wgrad = dY^T X) reuse
 * a3d_gemm / a3d_conv3x3 on transposed operands; what is declared here is everything else.
 * --------------------------------------------------------------------------------------------------------------------- */

/* Flash attention backward (the xformers memory_efficient_attention backward of attention_processor.py:103-105, 233-235, 405-418,
 * 656-658, 691-693).  Same row maps as a3d_flash_attn; dO rows through `domap`, dQ through `dqmap`, dK / dV through `dkmap`
 * (group index of the K/V maps: the first of the `q_per_kv` consecutive query groups that read that K/V, e.g. the F frames of a
 * video in the first-frame branch; groups % q_per_kv == 0).  dO is the gradient of the attention output scaled by `do_scale`
 * (the forward's out_scale).  lse2 / delta: fp32 scratch [groups * heads * q_len] each (log2-sum-exp and sum_k P dP per query
 * row, recomputed here: the forward keeps nothing).  dQ may be NULL (no query gradient wanted) or dK == dV == NULL (keys / values
 * of frozen text / image tokens); bit 0 of accumulate adds into dQ / dK / dV, bit 1: see a3d_flash_attn_lse below.  head_dim 40 / 64 / 80 / 160.
 * Q, K, V, dO, dQ, dK, dV 16-byte aligned (row strides multiples of 8 elements), lse2 / delta 4-byte aligned.  do_scale finite and either
 * 0 or normal (|do_scale| >= FLT_MIN): 0 gives zero gradients (with bit 0 of accumulate: dQ / dK / dV are left untouched); a subnormal
 * or non-finite do_scale is A3D_EINVAL. */
int a3d_flash_attn_bwd_bf16(a3d_stream_t stream, const void* Q, const void* K, const void* V, const void* dO,
                            void* dQ, void* dK, void* dV, float* lse2, float* delta,
                            const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* domap,
                            const a3d_rowmap* dqmap, const a3d_rowmap* dkmap,
                            int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len, int q_per_kv,
                            float scale, float do_scale, int accumulate);

/* The statistics of the backward without its statistics pass (a third of the attention backward's time at head_dim 40), for callers that
 * keep the forward's output: a3d_flash_attn_lse is a3d_flash_attn that also returns lse2 [groups][heads][q_len] (log2 of the softmax
 * denominator per query, out of the kernel's own row sums: one float store per query and head; xformers keeps the same tensor for its
 * backward); a3d_attn_delta computes delta[g][h][q] = sum_d dO[q][h, d] * O[q][h, d] (dO rows through `domap`, O rows through `omap`,
 * O = that forward's un-accumulated output; dO / O 16-byte, delta 4-byte aligned).  a3d_flash_attn_bwd with bit 1 of `accumulate` set
 * then reads lse2 / delta instead of recomputing them. */
int a3d_flash_attn_lse_bf16(a3d_stream_t stream, const void* Q, const void* K, const void* V, void* O,
                            const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* omap,
                            int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len,
                            float scale, float out_scale, int accumulate, float* lse2);
int a3d_attn_delta_bf16(a3d_stream_t stream, const void* dO, const void* O, const a3d_rowmap* domap, const a3d_rowmap* omap,
                        float* delta, int groups, int heads, int head_dim, int64_t q_len);

/* Temporal attention backward (attention_processor.py:630-636 under autograd): rows ((v*F + f)*L + l); Q / K / V share the row
 * stride ldqkv, dQ / dK / dV share ldd (e.g. the three column ranges of one [rows, 3C] gradient buffer).  frames <= 32; all seven
 * pointers 16-byte aligned, ldqkv / lddo / ldd multiples of 8. */
int a3d_temporal_attn_bwd_bf16(a3d_stream_t stream, const void* Q, const void* K, const void* V, int64_t ldqkv,
                               const void* dO, int64_t lddo, void* dQ, void* dK, void* dV, int64_t ldd,
                               int videos, int frames, int64_t L, int heads, int head_dim, float scale);

/* LayerNorm backward (diffusers BasicTransformerBlock.norm1/2/3): dX [M, C]; dgamma / dbeta fp32 [C] (both or neither;
 * accumulate == 0 zeroes them first; fp32 atomics: run-to-run equal to rounding).  C <= 2048; C = 320 / 640 / 1280 with 16-byte
 * aligned X, dY, dX, gamma take the 16-byte-access kernel (8 / 16 / 32 lanes per row). */
int a3d_layer_norm_bwd_bf16(a3d_stream_t stream, const void* X, const void* dY, const float* gamma, void* dX,
                            float* dgamma, float* dbeta, int64_t M, int C, float eps, int accumulate);

/* GroupNorm (+ fused SiLU) backward on channel-last [B][rows][C] (ResnetBlock2D.norm1/2, Transformer2DModel.norm, the 3-D norm of
 * TransformerTemporalModel): stats fp32 [B][groups][2] = (mean, rstd) as a3d_group_norm_apply takes them; ws fp32 [B*C*2] scratch;
 * dgamma / dbeta fp32 [C], ADDED to (both or neither).  C % 8 == 0, C <= 8192, X / dY / dX 16-byte aligned, the fp32 operands
 * 4-byte aligned (A3D_EINVAL otherwise). */
int a3d_group_norm_bwd_bf16(a3d_stream_t stream, const void* X, const void* dY, const float* gamma, const float* beta,
                            const float* stats, void* dX, float* ws, float* dgamma, float* dbeta,
                            int B, int64_t rows, int C, int groups, int silu);

/* GEGLU backward on the interleaved projection P [M, 2N] of a3d_gemm_geglu (column blocks [32 h | 32 gate]):
 * dP = [dY * gelu(gate) | dY * h * gelu'(gate)] in the same layout.  N % 32 == 0; P, dY, dP 16-byte aligned, row strides multiples of 8. */
int a3d_geglu_bwd_bf16(a3d_stream_t stream, const void* P, int64_t ldp, const void* dY, int64_t lddy, void* dP, int64_t lddp,
                       int64_t M, int64_t N);

/* Y[c][r] = X[r][c] (r < rows, c < cols), Y[c][rows .. rows_pad) = 0: operands of the weight-gradient GEMM dW = dY^T X, whose
 * contraction (the token rows) must be a multiple of 64, and W^T of the trainable weights for dX = dY W.  16-byte accesses when cols,
 * rows_pad, ldx and ldy are multiples of 8 and both pointers 16-byte aligned; any shape otherwise. */
int a3d_transpose_bf16(a3d_stream_t stream, const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t rows, int64_t cols,
                       int64_t rows_pad);

/* Weight gradient of a Linear: dW[N, K] (fp32, row stride lddw floats) (+)= alpha * dY[M, N]^T X[M, K], both operands in their natural
 * row-major layout.  The token axis M is split over the grid (the output is small, the contraction long): partial tiles go to the
 * fp32 workspace `ws` (a3d_wgrad_ws_floats(M, N, K) floats, 16-byte aligned) and a second kernel sums them.  accumulate != 0 adds
 * to dW.  N % 8 == 0, K % 8 == 0, 16-byte aligned rows. */
int64_t a3d_wgrad_ws_floats(int64_t M, int64_t N, int64_t K);
int a3d_wgrad_bf16(a3d_stream_t stream, const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, int64_t lddw,
                   float* ws, int64_t M, int64_t N, int64_t K, float alpha, int accumulate);

/* out[c] (+)= alpha * sum_r X[r][c]  (bias gradients), fp32 out (fp32 atomics over the row split).  cols % 320 == 0 with ldx % 8 == 0 and
 * a 16-byte aligned X reads 16 bytes per lane; any shape otherwise. */
int a3d_colsum_bf16(a3d_stream_t stream, const void* X, int64_t ldx, int64_t rows, int64_t cols, float* out, float alpha, int accumulate);

/* Y = a X + b Y over n elements (n % 8 == 0): sum of the gradients of two branches.  X, Y 16-byte aligned. */
int a3d_axpby_bf16(a3d_stream_t stream, const void* X, void* Y, int64_t n, float a, float b);

/* dgrad helper of the stride-2 down-sampling conv: Z [B, H, W, C] = dY [B, Ho, Wo, C] at the even positions, zero elsewhere
 * (Ho = (H-1)/2 + 1); the input gradient then is a stride-1 a3d_conv3x3 of Z with the flipped, transposed weight.  C % 8 == 0,
 * dY / Z 16-byte aligned. */
int a3d_zero_insert2x_bf16(a3d_stream_t stream, const void* dY, void* Z, int B, int H, int W, int C);

/* Backward of the nearest up-sampling in front of the up-sampler conv: dX [B, H, W, C] = sum of the <= 4 positions of
 * dU [B, He, We, C] each input pixel was copied to (He = 2H or 2H-1, likewise We: the forced sizes of unet_motion_mv_model.py:831-837).
 * C % 8 == 0, dU / dX 16-byte aligned. */
int a3d_upsample2x_bwd_bf16(a3d_stream_t stream, const void* dU, void* dX, int B, int H, int W, int He, int We, int C);

/* Optimiser over ONE flat fp32 buffer holding every trainable parameter (and flat gradient / moment buffers of the same length):
 *   a3d_sqnorm_f32     out[0] (+)= sum g^2
 *   a3d_clip_ctrl_f32  ctrl[0] = inv_loss_scale * min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_, train.py:586,593),
 *                      ctrl[1] = 1 if the norm is not finite (GradScaler: skip the step), ctrl[2] = the unscaled norm
 *   a3d_adamw_f32      torch.optim.AdamW step (decoupled weight decay) on g * ctrl[0], skipped when ctrl[1] != 0; ctrl may be NULL. */
int a3d_sqnorm_f32(a3d_stream_t stream, const float* g, int64_t n, float* out, int accumulate);
int a3d_clip_ctrl_f32(a3d_stream_t stream, const float* sqnorm, float max_norm, float inv_loss_scale, float* ctrl);
int a3d_adamw_f32(a3d_stream_t stream, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float bias_corr1, float bias_corr2, const float* ctrl);

/* Differentiable Gaussian splat rasterizer (csrc/splat.hip; contract in animate3d_amd/splat.py), fp32, B cameras per launch.
 * Per-Gaussian inputs are [*, N, k] contiguous; their *_bs argument is the element stride between images (0: one tensor shared
 * by all images).  Exactly one of shs ([*, N, M, 3], degree deg <= 3) / colors ([*, N, 3]) is non-NULL.  view / proj [B, 4, 4]
 * row-vector convention, campos [B, 3], tanfovx / tanfovy [B].  Per-(image, Gaussian) buffers are [B, N, ...]:
 *   a3d_gs_preprocess_f32      radii, xy [B, N, 2] (pixels), depth, conic_o [B, N, 4] (conic, opacity), rgb [B, N, 3], clamped (SH clamp bits),
 *                              tiles_touched
 *   a3d_gs_duplicate_f32       offsets = inclusive prefix sum of tiles_touched (int64); writes one key / value per touched tile:
 *                              key = (image * tiles + tile) << 32 | float bits of depth, value = Gaussian index
 *   a3d_gs_tile_ranges_f32     ranges [B * tiles, 2] = [start, end) of each (image, tile) in the L sorted keys (zeroed first)
 *   a3d_gs_render_f32          perm = the stable sort's permutation (sorted -> duplicated position, int64); image [B, 3, H, W], depth / alpha /
 *                              T_final [B, H, W], n_contrib [B, H, W]
 *   a3d_gs_render_bwd_f32      d_depth / d_alpha may be NULL (zero); rows [L, 12]: per instance, in duplicated order, the gradient w.r.t.
 *                              centre (2), conic (3), opacity, colour (3), depth, summed over the tile's pixels
 *   a3d_gs_preprocess_bwd_f32  per (image, Gaussian) input gradients [B, N, ...] (d_means2d: NDC centre, third component 0)
 *   a3d_gs_sum_batch_f32       dst[k] = sum over b of src[b * M + k], b in order
 * Preconditions, checked before anything is launched (A3D_EINVAL otherwise):
 *   - every pointer is required except d_depth / d_alpha, the colour source not in use with its gradient (d_shs / d_colors), and
 *     keys of a3d_gs_tile_ranges_f32 when L == 0; perm, vals and rows are required even when there are no instances (one element);
 *   - alignment: conic_o and rows 16 bytes; xy, ranges, keys, offsets and perm 8; every other float / int operand 4;
 *   - B, N, H, W > 0, B N <= 2^31 - 1, B * tiles <= 2^31 - 1 (tiles = ceil(W / 16) ceil(H / 16)); 0 <= deg <= 3 and
 *     M >= (deg + 1)^2 with shs; 0 <= L <= 2^31 - 1 and n_tiles > 0 for a3d_gs_tile_ranges_f32; B, M > 0 for a3d_gs_sum_batch_f32. */
int a3d_gs_preprocess_f32(a3d_stream_t stream, int B, int N, const float* means, int64_t means_bs, const float* scales, int64_t scales_bs,
                          const float* rots, int64_t rots_bs, const float* opac, int64_t opac_bs, const float* shs, int64_t shs_bs, int M,
                          int deg, const float* colors, int64_t colors_bs, const float* view, const float* proj, const float* campos,
                          const float* tanfovx, const float* tanfovy, int H, int W, float scale_mod, int* radii, float* xy, float* depth,
                          float* conic_o, float* rgb, int* clamped, int* tiles_touched);
int a3d_gs_duplicate_f32(a3d_stream_t stream, int B, int N, int H, int W, const float* xy, const float* depth, const int* radii,
                         const int64_t* offsets, int64_t* keys, int* vals);
int a3d_gs_tile_ranges_f32(a3d_stream_t stream, const int64_t* keys, int64_t L, int* ranges, int64_t n_tiles);
int a3d_gs_render_f32(a3d_stream_t stream, int B, int N, int H, int W, const int* ranges, const int64_t* perm, const int* vals,
                      const float* xy, const float* conic_o, const float* rgb, const float* depth, const float* bg,
                      float* out_img, float* out_depth, float* out_alpha, float* T_final, int* n_contrib);
int a3d_gs_render_bwd_f32(a3d_stream_t stream, int B, int N, int H, int W, const int* ranges, const int64_t* perm, const int* vals,
                          const float* xy, const float* conic_o, const float* rgb, const float* depth, const float* bg,
                          const float* T_final, const int* n_contrib, const float* d_img, const float* d_depth,
                          const float* d_alpha, float* rows);
int a3d_gs_preprocess_bwd_f32(a3d_stream_t stream, int B, int N, const float* means, int64_t means_bs, const float* scales, int64_t scales_bs,
                              const float* rots, int64_t rots_bs, const float* opac, int64_t opac_bs, const float* shs, int64_t shs_bs, int M,
                              int deg, const float* colors, int64_t colors_bs, const float* view, const float* proj, const float* campos,
                              const float* tanfovx, const float* tanfovy, int H, int W, float scale_mod, const int* radii,
                              const int* clamped, const int64_t* offsets, const int* tiles_touched, const float* rows,
                              float* d_means2d, float* d_means, float* d_scales, float* d_rots, float* d_opac, float* d_shs,
                              float* d_colors);
int a3d_gs_sum_batch_f32(a3d_stream_t stream, const float* src, float* dst, int B, int64_t M);

/* 4-D Gaussian deformation field: two-scale HexPlane grid + five 32-wide MLPs (csrc/deform4d.hip; contract in animate3d_amd/deform4d.py),
 * fp32, every frame of a step per call.  Replaces Gaussian4DModel.interpolate_ms_features / get_xyz / get_rotation / get_scaling
 * (custom/threestudio-animate3d/geometry/gaussian_4d.py:450-548) and their per-image loop (diff_gaussian_rasterizer_advanced_4d.py:77-135).
 * xyz [N, 3], scaling [N, 3], rotation [N, 4], timestamps [T].  grid: the twelve planes repacked texel-major ([H][W][16] each) in one
 * buffer; plane_desc is a HOST array [36] = float offset (multiple of 16) | W | H of plane k = 6 scale + pair, pairs in
 * itertools.combinations(range(4), 2) order, W the resolution of the pair's first coordinate (every resolution >= 2).
 * weights [5, 1152]: per network layers.0.weight [32, 32] then layers.2.weight zero-padded to [4, 32]; networks delta_xyz, delta_rot,
 * delta_scaling, global_rot, global_trans.  flags: 1 use_global_trans, 2 deform_scales, 4 first_frame_trainable.
 * img_start [T + 1] / img_list [B]: the images that show each frame, ascending (int32).
 *   a3d_dg_cells_f32           cells [12, N] int32: per plane the cell of each Gaussian (row-major (H - 1) x (W - 1) for a spatial plane,
 *                              the cell along the spatial axis for a time plane); the caller stable-sorts them into the plan
 *   a3d_dg_mean_partials       blocks per frame of the mean's first reduction stage (size of mpart)
 *   a3d_dg_forward_f32         sp [N, 32] (product of the spatial planes), mpart [T, partials, 32], gmean [T, 32], glob [T, 12] (R | trans)
 *                              (the last three only with use_global_trans); means / scales [B, N, 3], rots [B, N, 4]
 *   a3d_dg_backward_ws_floats  floats of the backward's workspace
 *   a3d_dg_backward_f32        order [12, N] / starts: the plan (per plane the Gaussians sorted by cell and each cell's first position,
 *                              cells + 1 entries per plane, planes back to back); d_means / d_scales / d_rots [B, N, ...];
 *                              d_grid in the packing of grid, d_weights [5, 1152], d_scaling [N, 3], d_rotation [N, 4].  No atomics:
 *                              every sum runs in a fixed order (images of a frame ascending, Gaussians in plan order, frames ascending) */
int a3d_dg_cells_f32(a3d_stream_t stream, int N, const float* xyz, const int64_t* plane_desc, int* cells);
int64_t a3d_dg_mean_partials(int N);
int a3d_dg_forward_f32(a3d_stream_t stream, int T, int N, int B, const float* xyz, const float* scaling, const float* rotation,
                       const float* timestamps, const float* grid, const int64_t* plane_desc, const float* weights, int flags,
                       const int* img_start, const int* img_list, float* sp, float* mpart, float* gmean, float* glob, float* means,
                       float* scales, float* rots);
int64_t a3d_dg_backward_ws_floats(int T, int N, const int64_t* plane_desc);
int a3d_dg_backward_f32(a3d_stream_t stream, int T, int N, int B, const float* xyz, const float* scaling, const float* rotation,
                        const float* timestamps, const float* grid, const int64_t* plane_desc, const float* weights, int flags,
                        const int* img_start, const int* img_list, const float* sp, const float* gmean, const float* glob,
                        const int* order, const int* starts, const float* d_means, const float* d_scales, const float* d_rots,
                        float* ws, float* d_grid, float* d_weights, float* d_scaling, float* d_rotation);

/* ARAP rigidity loss on the Gaussian trajectories and its k-NN graph (csrc/arap.hip; contract in animate3d_amd/arap.py), fp32 at the
 * interface.  Replaces cal_connectivity_from_points / estimate_rotation / cal_arap_error (custom/threestudio-animate3d/systems/util.py:58-215)
 * and the pytorch3d.ops.knn_points they are built on.
 *   a3d_knn_f32            exact K nearest other points of each of N points [N, 3] by dx*dx + dy*dy + dz*dz, ascending by (distance,
 *                          index); 1 <= K <= 16 (else A3D_EUNSUPPORTED), N > K.  Columns >= least_edge_num whose distance is not below
 *                          radius2 become index -1, distance +inf (least_edge_num >= K: no cut).  nn_idx [N, K] int32, nn_dist [N, K]
 *   a3d_arap_energy_f32    source [Nv, 3]; targets: F frames of [Nv, 3], frame f at targets + f * targets_bs floats; nn_idx [Nv, K] (-1: no
 *                          edge); weight [Nv, K] or NULL (1 on edges); sample_idx [S] int32.  rot [F, S, 9] fp64 (kept for the backward),
 *                          rot_f32 [F, S, 9] or NULL, energy [F * S] fp64 workspace, loss [1]: the sum over frames, samples and edges in a
 *                          fixed order
 *   a3d_arap_backward_f32  order [S (K + 1)] / starts [Nv + 1]: the (sample, slot) pairs s (K + 1) + c (slot 0: the sample's vertex, slot k + 1
 *                          its k-th neighbour) stable-sorted by vertex, absent ones last, and each vertex's first position; grad_out [1]
 *                          or NULL (zero); d_targets [F, Nv, 3] contiguous, d_source [Nv, 3] or NULL.  The rotations are constants.  No
 *                          atomics: each vertex sums its entries in list order, frames ascending; rows without entries are written 0
 *   a3d_mesh_sample_neighbours  the mesh branch's per-step draw (sample_matrix_vectorized, util.py:320-344) over a fixed CSR adjacency:
 *                          row_start [Nv + 1] and col [E] int32 (col may be NULL when E = 0), seed [1] int64 read on the device, nn_idx
 *                          [Nv, K] int32 out.  Row v has d = row_start[v + 1] - row_start[v] entries (bounds outside [0, E] or descending
 *                          are clamped: a short row, never an access out of bounds).  Its positions p = 0 .. d - 1 are walked once;
 *                          position p is kept iff mulhi32(r_p, d - p) < K - kept, where mulhi32 is the high word of the 32 x 32-bit
 *                          product and kept counts the positions kept so far (selection sampling, Knuth's Algorithm S: a uniformly
 *                          random subset of min(K, d) positions, in ascending position; bias at most d / 2^32 per decision);
 *                          nn_idx[v, kept] = col[row_start[v] + p]; the walk ends at kept = K; the rest of the row is -1.  A row with
 *                          d <= K is copied whole.  r_p is word p % 4 of Philox4x32-10 (Salmon et al. 2011, as in Random123: multipliers
 *                          0xD2511F53 on word 0 and 0xCD9E8D57 on word 2, key increments 0x9E3779B9 and 0xBB67AE85, round
 *                          (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key raised between
 *                          rounds) with key (low, high 32 bits of seed[0]) and counter (v, p / 4, 0, 0): a row depends on (seed, v) and
 *                          the graph alone.  Nv >= 1, E >= 0; pointers 4-byte aligned, seed 8-byte aligned (else A3D_EINVAL);
 *                          1 <= K <= 16 (else A3D_EUNSUPPORTED).  One launch, one thread per vertex, no workspace */
int a3d_knn_f32(a3d_stream_t stream, int N, const float* points, int K, int least_edge_num, float radius2, int* nn_idx, float* nn_dist);
int a3d_arap_energy_f32(a3d_stream_t stream, int F, int Nv, int K, int S, const float* source, const float* targets, int64_t targets_bs,
                        const int* nn_idx, const float* weight, const int* sample_idx, double* rot, float* rot_f32, double* energy,
                        float* loss);
int a3d_arap_backward_f32(a3d_stream_t stream, int F, int Nv, int K, int S, const float* source, const float* targets, int64_t targets_bs,
                          const int* nn_idx, const float* weight, const int* sample_idx, const double* rot, const int* order,
                          const int* starts, const float* grad_out, float* d_targets, float* d_source);
int a3d_mesh_sample_neighbours(a3d_stream_t stream, int Nv, int E, const int* row_start, const int* col, int K, const int64_t* seed,
                               int* nn_idx);

/* Mesh ingest (csrc/mesh_ingest.hip; contract in animate3d_amd/mesh.py), fp32 at the interface.  Replaces the Python loops of
 * tools/mesh_animation/mesh2gaussian.py and the transform of Gaussian4DModel.load_ply (geometry/gaussian_4d.py:177-260).  rot9 (R,
 * row-major) and quat4 (R's unit quaternion w, x, y, z) are HOST pointers to doubles, read before the launch; every other pointer is
 * device memory, 4-byte aligned.
 *   a3d_mesh_vertex_gaussians_f32  one thread per vertex of verts [Nv, 3] over the CSR adjacency row_start [Nv + 1] / col [E] (col and
 *                          edge_length may be NULL when E = 0): edge_length [E] = |x_v - x_col[e]| for e in v's row; mean_edge [Nv, 3] =
 *                          the sum over the row, in row order, of |x_u - x_v| per axis, divided by the degree (0 for an empty row);
 *                          colors [Nv, 3] = vertex_colors [Nv, 3] as they are, or the sum over v's corners, in the order of the list
 *                          corner_order [C] / corner_start [Nv + 1] (corner k is entry k of faces [F, 3] flattened, C = 3 F), of the
 *                          corner's colour, divided by their number: corner_colors [C, 3], or texture [Ht, Wt, 3] sampled bilinearly
 *                          at uvs [Nt, 2][corner_uv [C]] with the v axis flipped, pixel centres at the ends of [0, 1] and the
 *                          coordinates clamped to it (grid_sample with align_corners and border padding on the row-flipped texture).
 *                          xyz = scale_factor R x, scaling = log(mean_edge / shrink * scale_factor) (-inf for a zero), shs =
 *                          (colors - 0.5) / 0.28209479177387814.  Exactly one of vertex_colors, corner_colors and texture is not NULL.
 *                          A3D_EINVAL before any launch for: a NULL required pointer, Nv <= 0, E < 0, zero or several colour sources,
 *                          a corner source without its list or with C < 1, Ht / Wt / Nt < 1, shrink or scale_factor not a positive
 *                          finite number, a misaligned pointer.  Row bounds and the indices the kernel reads (col, corner_order,
 *                          corner_uv) are clamped to their arrays.  No atomics, no workspace, one launch
 *   a3d_gaussians_rigid_f32  N Gaussians: xyz = scale_factor R xyz_in, scaling = scaling_in + log(scale_factor), rotation =
 *                          q_R (x) rotation_in / |rotation_in| (Hamilton product, w first), in fp64 with one rounding.  A3D_EINVAL for
 *                          a NULL pointer, N <= 0, scale_factor not a positive finite number, a misaligned pointer.  In place is fine */
int a3d_mesh_vertex_gaussians_f32(a3d_stream_t stream, int Nv, int E, int C, const float* verts, const int* row_start, const int* col,
                                  const int* corner_order, const int* corner_start, const float* vertex_colors, const float* corner_colors,
                                  const float* texture, int Ht, int Wt, const float* uvs, int Nt, const int* corner_uv, const double* rot9,
                                  double scale_factor, double shrink, float* xyz, float* scaling, float* shs, float* colors,
                                  float* mean_edge, float* edge_length);
int a3d_gaussians_rigid_f32(a3d_stream_t stream, int N, const float* xyz_in, const float* scaling_in, const float* rotation_in,
                            const double* rot9, const double* quat4, double scale_factor, float* xyz, float* scaling, float* rotation);

/* Mesh export (csrc/mesh_export.hip; contract in animate3d_amd/mesh_export.py), fp32 at the interface.  The per-frame vertex normals of
 * the animated mesh that replaces tools/mesh_animation/export_animated_mesh.py (which leaves them to Blender).
 *   a3d_mesh_vertex_normals_f32  one thread per (frame t, vertex v) of pos [T, Nv, 3] over v's corner list order [C] / starts [Nv + 1]
 *                          (corner c is entry c of faces [F, 3] flattened, C = 3 F; the list a3d_mesh_vertex_gaussians_f32 reads):
 *                          nrm [T, Nv, 3] = normalize(sum over v's corners c, in the list's order, of u x w) with f = c / 3, k = c - 3 f,
 *                          a = faces[c], b = faces[3 f + (k + 1) % 3], d = faces[3 f + (k + 2) % 3], u = P_t[b] - P_t[a], w = P_t[d] -
 *                          P_t[a]: area-weighted, a face with two equal corners adds exactly 0.  Differences, products, the sum and
 *                          the normalisation are fp64 without contraction, the result is rounded to fp32 once; where the squared
 *                          length of the sum is not > 0 or not finite, nrm = (0, 0, 1).  A3D_EINVAL before any launch for: T < 1,
 *                          Nv < 1, C < 3, C % 3 != 0, T Nv 3 >= 2^31, a NULL pointer, a pointer that is not 4-byte aligned.  The
 *                          indices the kernel reads (starts, order, faces) are clamped to their arrays.  No atomics, no workspace,
 *                          no host synchronisation, one launch; bitwise reproducible and independent of the launch geometry */
int a3d_mesh_vertex_normals_f32(a3d_stream_t stream, int T, int Nv, int C, const float* pos, const int* faces, const int* order,
                                const int* starts, float* nrm);

/* Camera batches of the 4-D stage (csrc/camera_batch.hip; contract in animate3d_amd/cameras.py), fp32 at the interface.  Replace the
 * per-step CPU code of custom/threestudio-animate3d/data/uncond_hybrid.py (collate and the two eval datasets) and
 * data/simple_multi_image.py:91-131, and the two solver calls of get_cam_info_gaussian.  One thread per camera, fp64 arithmetic, every
 * output rounded to fp32 once; no atomics, no workspace, one launch.  Outputs per camera b, in the layout rasterize_gaussians takes:
 * c2w [B, 4, 4] = [right, up, -lookat | pos] with lookat = normalize(centre - pos), right = normalize(lookat x up), up = normalize(right x
 * lookat) (normalize: v / max(|v|, 1e-12)); w2c [B, 4, 4]: the inverse of c2w diag(1, -1, -1, 1), transposed (row-vector form);
 * full_proj [B, 4, 4] = w2c projT with get_projection_matrix_gaussian's matrix for fovx = fovy, znear, zfar; campos [B, 3] = pos;
 * tanfov [B] = tan(fovy / 2).
 *   a3d_cameras_spherical_f32  pos = distance (cos e cos a, cos e sin a, sin e) for elevation e, azimuth a; angles and fovy are given in
 *                          units of angle_unit radians (1: radians; pi / 180: degrees, converted in fp64).  perturb [B, 9] or NULL:
 *                          (offset added to pos, centre, offset added to the up vector (0, 0, 1)); NULL: centre 0, up (0, 0, 1)
 *   a3d_cameras_random_f32  collate (uncond_hybrid.py:195-304) on explicit draws for B = R n_view total_frame cameras, object-major, then
 *                          view, then frame: obj [R, 5] uniform (elevation, azimuth, fovy, distance, zoom), pert_u [B, 3] uniform,
 *                          pert_n [B, 6] normal (centre, up).  ranges10: HOST pointer to 10 doubles, (lo, hi) of elevation, azimuth and
 *                          fovy in degrees, of the distance and of the zoom.  elev_mode 0: elevation uniform in degrees; 1: uniform
 *                          on the sphere, asin(u (sin hi - sin lo) + sin lo).  azimuth of view v = (u + v) / n_view (hi - lo) + lo;
 *                          distance *= 1 / tan(fovy / 2) with relative_radius, before fovy *= zoom; pos += pert_u 2 camera_perturb -
 *                          camera_perturb, centre = pert_n[:3] center_perturb, up = (0, 0, 1) + pert_n[3:] up_perturb.  Also written:
 *                          elevation_deg, azimuth_deg, fovy (radians, after the zoom), camera_distances [B]
 *   a3d_cameras_from_c2w_f32  any invertible c2w [B, 4, 4] and fovy [B] (radians): the 4 x 4 inverse by the adjugate; campos = c2w[:3, 3]
 * A3D_EINVAL before any launch for: a NULL pointer other than perturb, a pointer that is not 4-byte aligned, B or R or n_view or
 * total_frame <= 0, more than 2^24 cameras, elev_mode other than 0 / 1, a non-finite range or perturbation, angle_unit not a positive
 * finite number, znear / zfar not finite with 0 < znear < zfar. */
int a3d_cameras_spherical_f32(a3d_stream_t stream, int B, const float* elevation, const float* azimuth, const float* distance,
                              const float* fovy, const float* perturb, double angle_unit, double znear, double zfar, float* c2w, float* w2c,
                              float* full_proj, float* campos, float* tanfov);
int a3d_cameras_random_f32(a3d_stream_t stream, int R, int n_view, int total_frame, const float* obj, const float* pert_u,
                           const float* pert_n, const double* ranges10, int elev_mode, int relative_radius, double camera_perturb,
                           double center_perturb, double up_perturb, double znear, double zfar, float* c2w, float* w2c, float* full_proj,
                           float* campos, float* tanfov, float* elevation_deg, float* azimuth_deg, float* fovy, float* camera_distances);
int a3d_cameras_from_c2w_f32(a3d_stream_t stream, int B, const float* c2w, const float* fovy, double znear, double zfar, float* w2c,
                             float* full_proj, float* campos, float* tanfov);

/* Reconstruction loss of the 4-D stage (csrc/recon_loss.hip; contract in animate3d_amd/stage4d.py, masked_recon_loss), fp32.  Replaces the
 * val[sampled_idx] copies, the mask compositing and the two F.mse_loss of custom/threestudio-animate3d/systems/animate3d.py:160-184 and the
 * clamp of diff_gaussian_rasterizer_advanced_4d.py:180.  image [B, 3, H, W] planar and unclamped, alpha [B, H, W], gt_rgb [S, H, W, 3]
 * interleaved, gt_mask [S, H, W] bytes (non-zero: inside), index [B] int32 or NULL (identity): image b is compared with frame index[b],
 * which the kernels do not range-check.  bg: the background of all three channels.
 *   a3d_recon_loss_f32      out [3] = {lambda_rgb mean_rgb + lambda_mask mean_mask, mean_rgb, mean_mask} with
 *                           mean_rgb = mean((clamp(image, 0, 1) - (m ? gt : bg))^2) over B H W 3 and mean_mask = mean((alpha - m)^2) over
 *                           B H W.  partials [2, n_partials] fp32 workspace, n_partials = B * ceil(H W / 2048) (anything else: A3D_EINVAL).
 *                           No atomics: per-thread runs of 8 pixels, a fixed tree per block, the partials added in index order
 *   a3d_recon_loss_bwd_f32  recomputes from the inputs: d_image = g coef_rgb (clamp(image) - (m ? gt : bg)) where 0 <= image <= 1 and
 *                           exactly 0 elsewhere, d_alpha = g coef_mask (alpha - m), g = grad_out[0] read on the device; the caller passes
 *                           coef_rgb = 2 lambda_rgb / (3 B H W), coef_mask = 2 lambda_mask / (B H W).  One of d_image / d_alpha may be NULL
 * Pointers are 4-byte aligned at least (A3D_EINVAL otherwise); where H W % 4 == 0 and every float pointer is 16-byte aligned the kernels
 * read and write 16 bytes at a time.  B, H, W > 0 and B H W < 2^40 (A3D_EINVAL), checked before the first HIP call. */
int a3d_recon_loss_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const float* gt_rgb,
                       const uint8_t* gt_mask, const int* index, float bg, double lambda_rgb, double lambda_mask, float* partials,
                       int64_t n_partials, float* out);
int a3d_recon_loss_bwd_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const float* gt_rgb,
                           const uint8_t* gt_mask, const int* index, float bg, float coef_rgb, float coef_mask, const float* grad_out,
                           float* d_image, float* d_alpha);

/* The same pair on 8-bit ground truth: gt_rgba8 [S, H, W, 4] bytes (r, g, b, a) in place of gt_rgb and gt_mask.  The kernels are the two
 * above with another reader of the ground truth, the only thing that differs: colour = (float)byte / 255.0f by IEEE division, inside =
 * alpha byte >= 128 (byte / 255.0f > 0.5f).  Against gt_rgb = byte / 255.0f and gt_mask = alpha byte >= 128 every output is bit-equal
 * to the pair above.  Geometry, partial count, summation order, index and every other rule are theirs.  gt_rgba8 is 4-byte aligned at
 * least (A3D_EINVAL otherwise, before the first HIP call); where H W % 4 == 0 and it and every float pointer are 16-byte aligned, four
 * pixels are read as one 16-byte load. */
int a3d_recon_loss_rgba8_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const uint8_t* gt_rgba8,
                             const int* index, float bg, double lambda_rgb, double lambda_mask, float* partials, int64_t n_partials,
                             float* out);
int a3d_recon_loss_rgba8_bwd_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, const uint8_t* gt_rgba8,
                                 const int* index, float bg, float coef_rgb, float coef_mask, const float* grad_out, float* d_image,
                                 float* d_alpha);

/* Frames of the 4-D stage (csrc/stage_frames.hip; contract in animate3d_amd/frames.py): 8-bit RGBA ground truth in, test renders out.
 * Replace the CPU arithmetic of custom/threestudio-animate3d/data/simple_multi_image.py:205-215 and systems/animate3d.py:441-445.
 *   a3d_frames_unpack_u8  rgba8 [S, h, w, 4] bytes and an integer reduction factor k, 1 <= k <= 16, h = k H, w = k W.  Per output pixel and
 *                         channel, alpha included: q = (2 sum + k^2) / (2 k^2) in integers over the k x k source bytes, the exact mean
 *                         rounded half up (k = 1: the byte itself).  Outputs, each may be NULL but not all: out8 [S, H, W, 4] the bytes q;
 *                         rgb [S, H, W, 3] fp32 = (float)q / 255.0f by IEEE division, never a multiply by a reciprocal; mask [S, H, W]
 *                         bytes 0 / 1 = q_alpha >= 128, which is q / 255.0f > 0.5f.  One thread per output pixel, one 4-byte load per
 *                         source pixel
 *   a3d_frames_pack_u8    image [B, 3, H, W] planar and alpha [B, H, W] fp32 -> rgba8 [B, H, W, 4] bytes: (uint8)(clamp(v, 0, 1) * 255.0f)
 *                         in fp32, truncating, what (rgba_img * 255).astype(np.uint8) gives for the clamped comp_rgb.  alpha is clamped
 *                         as well (comp_mask is not clamped in the reference; a rasterizer alpha lies in [0, 1]); a NaN gives 0
 * A3D_EINVAL before any launch for: a NULL input, no output, an extent <= 0, k outside 1 .. 16, h % k or w % k != 0, 2^39 pixels or more
 * (S h w, B H W), a pointer other than mask that is not 4-byte aligned.  No atomics, no workspace, no host synchronisation, one launch. */
int a3d_frames_unpack_u8(a3d_stream_t stream, int S, int h, int w, int k, const uint8_t* rgba8, uint8_t* out8, float* rgb, uint8_t* mask);
int a3d_frames_pack_u8(a3d_stream_t stream, int B, int H, int W, const float* image, const float* alpha, uint8_t* rgba8);

/* Regularisers of the 4-D stage's step (csrc/stage_reg.hip; contract in animate3d_amd/stage4d.py, image_regularizers and
 * gaussian_regularizers), fp32.  Replace the torch chains of custom/threestudio-animate3d/systems/animate3d.py:256-296 over tv_loss
 * (threestudio/utils/loss.py:8-16).  image [B, 3, H, W] planar and unclamped, depth and alpha [B, H, W]; means [B, N, 3]; scales: image b's
 * [N, 3] at scales + b scales_bs, scales_bs = 3 N or 0 (one [N, 3] counted B times); scaling [N, 3] log-scales; opacity [N].
 *   a3d_image_reg_f32         out [4] = {lambda_tv tv + lambda_depth_tv depth_tv + lambda_sparsity sparsity, tv, depth_tv, sparsity} with
 *                             tv = 2 (sum (x[y+1] - x[y])^2 / (3 (H-1) W) + sum (x[x+1] - x[x])^2 / (3 H (W-1))) / B of x = clamp(image, 0, 1),
 *                             depth_tv the same of depth (one channel, no clamp), sparsity = mean(sqrt(alpha^2 + 0.01)).  A term whose
 *                             lambda is 0 is neither read nor computed (0 in out) and its pointer may be NULL; all three 0: A3D_EINVAL.
 *                             partials [5, n_partials] fp32 workspace, n_partials = B * ceil(H W / 8192) (anything else: A3D_EINVAL).
 *                             No atomics: per-thread runs of 32 pixels, a fixed tree per block, the partials added in index order in fp64
 *   a3d_image_reg_bwd_f32     gather form, recomputed from the inputs; g = grad_out[0] read on the device.  d_image = g (coef_tv_h (into -
 *                             out of the pixel vertically) + coef_tv_w (the same horizontally)) of the clamped neighbours where
 *                             0 <= image <= 1 and exactly 0 elsewhere; d_depth likewise without a clamp; d_alpha = g coef_sparsity alpha /
 *                             sqrt(alpha^2 + 0.01).  The caller passes coef_tv_h = 4 lambda_tv / (3 (H-1) W B), coef_tv_w = 4 lambda_tv /
 *                             (3 H (W-1) B), the depth's without the 3, coef_sparsity = lambda_sparsity / (B H W).  Each of d_image / d_depth
 *                             / d_alpha may be NULL, not all; the input of a NULL output is not read and may be NULL
 *   a3d_gaussian_reg_f32      out [4] = {lambda_position position + lambda_scales scale_sum + lambda_opacity opacity_term, position,
 *                             scale_sum, opacity_term}: position = mean over (B, N) of |means|, scale_sum = sum of scales, opacity_term =
 *                             sum over N of |exp(scaling)| opacity.  Lambdas and NULLs as above.  partials [3, n_partials],
 *                             n_partials = ceil(B N / 1024)
 *   a3d_gaussian_reg_bwd_f32  d_means [B, N, 3] = g coef_position means / |means| (0 at |means| = 0), d_scales [B, N, 3] = g coef_scales,
 *                             d_opacity [N] = g coef_opacity |exp(scaling)|; the caller passes coef_position = lambda_position / (B N) and
 *                             the other two lambdas.  Each output may be NULL, not all
 * Pointers are 4-byte aligned at least (A3D_EINVAL otherwise); where W % 4 == 0 and every image pointer is 16-byte aligned the image kernels
 * read and write 16 bytes at a time.  B, H, W, N > 0, H W <= 2^30, B N <= 2^30, and H, W >= 2 with a TV term (A3D_EINVAL), checked before
 * the first HIP call. */
int a3d_image_reg_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* depth, const float* alpha, double lambda_tv,
                      double lambda_depth_tv, double lambda_sparsity, float* partials, int64_t n_partials, float* out);
int a3d_image_reg_bwd_f32(a3d_stream_t stream, int B, int H, int W, const float* image, const float* depth, const float* alpha,
                          float coef_tv_h, float coef_tv_w, float coef_depth_tv_h, float coef_depth_tv_w, float coef_sparsity,
                          const float* grad_out, float* d_image, float* d_depth, float* d_alpha);
int a3d_gaussian_reg_f32(a3d_stream_t stream, int B, int N, const float* means, const float* scales, int64_t scales_bs, const float* scaling,
                         const float* opacity, double lambda_position, double lambda_scales, double lambda_opacity, float* partials,
                         int64_t n_partials, float* out);
int a3d_gaussian_reg_bwd_f32(a3d_stream_t stream, int B, int N, const float* means, const float* scaling, float coef_position,
                             float coef_scales, float coef_opacity, const float* grad_out, float* d_means, float* d_scales,
                             float* d_opacity);

/* The SDS-side glue of the 4D-SDS step (csrc/sds_glue.hip; contract in animate3d_amd/sds.py, sds_recon_loss_fused): everything of
 * AnimateMVDiffusionGuidance.compute_mvdream_recon_loss (animatemv_guidance.py:415-503) but the UNet call.  b videos of n views of f >= 2
 * frames, c channels, P = h w.  latents, latents_noisy, latents_recon, noise_pred and grad are [(b n f), c, P] fp32; noise is
 * [b, n, f - 1, c, P] fp32; t [b] int64 and table [table_len] fp32 (alphas_cumprod) live on the device, a = table[t[b]] with t clamped into
 * the table.  sample and eps are the UNet's [2 b n, c, f, P] in (text, uncond) halves and timestep its [2 b n], all of `dtype`: A3D_F32, or
 * the storage type of the entry point (A3D_BF16 for _bf16, A3D_F16 for _f16; the other one: A3D_EINVAL).
 *   a3d_sds_pack          one launch: latents_noisy = frame 0 ? latents : sqrt(a) latents + sqrt(1 - a) noise; sample = latents_noisy in the
 *                         "(b n) c f P" layout, both halves; timestep = t[b] per (half, b, view)
 *   a3d_sds_epilogue      eps_cfg = eps_text + guidance_scale (eps_text - eps_uncond); x0(e) = (latents_noisy - sqrt(1 - a) e) / sqrt(a);
 *                         with r = recon_std_rescale != 0: factor[b] = (std x0(eps_text) + 1e-8) / (std x0(eps_cfg) + 1e-8), the unbiased
 *                         standard deviations over b's n (f - 1) c P diffused elements, and recon = r (x0 factor) + (1 - r) x0, else
 *                         recon = x0(eps_cfg); frame 0 of latents_recon is frame 0 of latents; out[0] = 0.5 sum (latents - recon)^2 /
 *                         (b n f) * f / (f - 1).  noise_pred (eps_cfg of every frame) may be NULL.  Three launches with r != 0, two without
 *                         (stats may then be NULL).  latents_recon and noise_pred are fp32 arithmetic that rounds where the torch ops
 *                         round.  The statistics and the loss are formed in fp64 from latents, noise and eps (noise: the tensor
 *                         a3d_sds_pack diffused with): the statistics per block of 2 048 elements in two passes (mean, then squared
 *                         deviations), merged per b in block order by the pairwise update of Chan, Golub and LeVeque, never as a
 *                         difference of sums; the loss's block sums through the fixed tree of csrc/loss_reduce.h in fp64, stored as
 *                         fp32 pairs (hi, lo) and added by one block in fp64, so out[0] carries one rounding.  stats [b, ceil(n (f - 1)
 *                         c P / 2048), 4] fp64 workspace, n_stats its length in doubles; partials [2, n_partials] fp32 workspace,
 *                         n_partials = b ceil(n f c P / 2048); anything else: A3D_EINVAL
 *   a3d_sds_epilogue_bwd_f32   grad = (latents - latents_recon) coef grad_out[0], exactly 0 in frame 0; grad_out is read on the device;
 *                         the caller passes coef = f / ((f - 1) b n f).  One launch, fp32 on both sides: no twin
 * No atomics, no host synchronisation; two calls are bitwise equal and b's rows do not depend on the rest of the batch.  A3D_EINVAL before
 * any launch for: a NULL required pointer, a size < 1, f < 2, b n f c P >= 2^40, a pointer not aligned to its element. */
int a3d_sds_pack_bf16(a3d_stream_t stream, int b, int n, int f, int c, int P, const float* latents, const float* noise, const int64_t* t,
                      const float* table, int table_len, int dtype, float* latents_noisy, void* sample, void* timestep);
int a3d_sds_epilogue_bf16(a3d_stream_t stream, int b, int n, int f, int c, int P, const void* eps, int dtype, const float* latents_noisy,
                          const float* latents, const float* noise, const int64_t* t, const float* table, int table_len,
                          double guidance_scale, double recon_std_rescale, double* stats, int64_t n_stats, float* latents_recon,
                          float* noise_pred, float* partials, int64_t n_partials, float* out);
int a3d_sds_epilogue_bwd_f32(a3d_stream_t stream, int b, int n, int f, int c, int P, const float* latents, const float* latents_recon,
                             float coef, const float* grad_out, float* grad);

/* The optimiser step of the 4-D stage (csrc/stage_optim.hip; contract in animate3d_amd/stage_optim.py, StageAdam), fp32.  Replaces
 * torch.optim.Adam(l, lr=0.0, eps=1e-15) of custom/threestudio-animate3d/geometry/gaussian_4d.py:391 and the step that Lightning's
 * GradScaler drops when a gradient holds an inf or a NaN.
 *   a3d_stage_adam_f32  table: HOST pointer to count entries, 1 <= count <= A3D_STAGE_ADAM_MAX_TENSORS; it is copied into the kernels'
 *                       arguments, nothing is copied to the device.  Entry t: parameter p, gradient g, moments m and v of n fp32
 *                       elements each, the tensor's own step (one fp32 on the device, an exact integer) and its own rate lr.  No two
 *                       entries may overlap.  flag: one int32 on the device.  phases, a sum of
 *                         A3D_STAGE_ADAM_BEGIN   flag = 0
 *                         A3D_STAGE_ADAM_CHECK   flag = 1 where any element of any g of the table is an inf or a NaN
 *                         A3D_STAGE_ADAM_UPDATE  where flag == 0: per element, with k = step + 1,
 *                                                  m' = beta1 m + (1 - beta1) g,  v' = beta2 v + (1 - beta2) g^2,
 *                                                  p' = p - (lr / (1 - beta1^k)) m' / (sqrt(v') / sqrt(1 - beta2^k) + eps)
 *                                                (torch.optim.Adam without amsgrad, weight decay or maximize) in fp64 on the fp32
 *                                                loads, without contraction, the update from the unrounded m' and v', each of p', m',
 *                                                v' rounded to fp32 once; then step += 1 for every tensor.  Where flag != 0: nothing
 *                                                is written, the steps included
 *                       run in this order.  All three in one call is the whole step of up to A3D_STAGE_ADAM_MAX_TENSORS tensors.  More
 *                       tensors: BEGIN | CHECK with the first table, CHECK with every other, then UPDATE with each, on one stream;
 *                       the check then covers every tensor before any is updated, and flag reads 1 (skipped) or 0 afterwards.
 *                       At most four launches per call, whatever count is; no atomics, no workspace but the flag, no host
 *                       synchronisation; no result depends on the order in which blocks run.  4-byte accesses.
 * A3D_EINVAL before any launch for: table or flag NULL, count < 1 or > A3D_STAGE_ADAM_MAX_TENSORS, phases 0 or with another bit, beta1 or
 * beta2 outside [0, 1), eps negative or not finite, and in any entry a NULL pointer, a pointer that is not 4-byte aligned, n < 1, lr
 * negative or not finite, or more than 2^31 - 1 blocks of 1 024 elements in all. */
#define A3D_STAGE_ADAM_MAX_TENSORS 32
#define A3D_STAGE_ADAM_BEGIN 1
#define A3D_STAGE_ADAM_CHECK 2
#define A3D_STAGE_ADAM_UPDATE 4
typedef struct a3d_stage_adam_entry {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* step;
  int64_t n;
  double lr;
} a3d_stage_adam_entry;
int a3d_stage_adam_f32(a3d_stream_t stream, const a3d_stage_adam_entry* table, int count, double beta1, double beta2, double eps,
                       int phases, int* flag);

/* CLIP image pre-processing of rendered frames (csrc/clip_preprocess.hip; contract in animate3d_amd/clip.py, preprocess_frames).
 * Replaces the device -> host -> PIL -> CLIPImageProcessor -> device round trip of animatemv_guidance.py:546-555 / utils/util.py:268-287,
 * bit-equal to it: (uint8)(v * 255.0f), Pillow's 8-bit bicubic resampler (integer, 22 precision bits, horizontal then vertical pass, a
 * clip to [0, 255] after each), the centre crop, and a [3, 256] table for /255 + mean / std.  One launch, one dtype code, no twins.
 *   rgb            n_src frames [in_h, in_w, 3] of fp32, element (n, y, x, c) at rgb + n s_img + y s_y + x s_x + c s_c
 *   image_index    [n_img] frames to take, or NULL (frame i); an index outside 0 .. n_src - 1 gives a frame of zero bytes
 *   coef_* / bounds_* / ksize_*   per axis (x: horizontal pass, y: vertical) the fixed-point coefficients [crop, ksize] and
 *                  (first input index, count) [crop, 2] of the crop x crop output window; ksize 0: the pass is skipped (equal sizes) and
 *                  output i copies input off_* + i.  off_* is read only then
 *   tile_rows      output rows per workgroup; max_rows: the most input rows the vertical pass of one such tile reads.  The tile's
 *                  intermediate, max_rows * 3 * crop bytes, lives in LDS: above a3d_clip_preprocess_lds_limit() -> A3D_EUNSUPPORTED
 *   table          [3, 256] fp32
 *   outputs (each may be NULL, not all): pixel_values [n_img, 3, crop, crop] and patch_rows [n_img (crop / patch)^2, kp] with columns
 *                  in (c, ky, kx) order and columns 3 patch^2 .. kp zero (needs tile_rows == patch, crop % patch == 0), both of `dtype`
 *                  (A3D_F32 / A3D_BF16 / A3D_F16: one round-to-nearest-even of the table value); u8 [n_img, crop, crop, 3] the bytes */
int64_t a3d_clip_preprocess_lds_limit(void);
int a3d_clip_preprocess(a3d_stream_t stream, const float* rgb, int n_src, int in_h, int in_w, int64_t s_img, int64_t s_y, int64_t s_x,
                        int64_t s_c, const int* image_index, int n_img, int crop, const int* coef_x, const int* bounds_x, int ksize_x,
                        int off_x, const int* coef_y, const int* bounds_y, int ksize_y, int off_y, int tile_rows, int max_rows,
                        const float* table, int dtype, void* pixel_values, void* patch_rows, int patch, int kp, uint8_t* u8);

/* The byte ends of MV-VDM generation (csrc/video_io.hip; host side in animate3d_amd/video.py, used by animate3d_amd/pipeline.py).  Elementwise,
 * one launch each, no workspace, no atomics; a result depends on its own input value only.  A3D_EINVAL before any launch: a NULL operand, an
 * extent <= 0, more than 2^31 - 1 pixels, a pixel size or channel count other than 3 or 4, a dtype code outside the enum, a misaligned pointer
 * or stride as stated per entry point.
 *   a3d_images_in_u8   images [n, H, W, cin] bytes (cin 3 or 4, a fourth channel is ignored; 4-byte aligned) -> planar [n, 3, H, W] fp32 =
 *                      (b / 255.0f - 0.5f) / 0.5f with IEEE division and subtraction as written: the bits of torch's uint8 / 255 and
 *                      Normalize(0.5, 0.5) on the CPU (animatediff/pipelines/pipeline.py:548-554).  unit (or NULL) [n, H, W, 3] fp32 = b / 255.0f:
 *                      the float image a3d_clip_preprocess reads, whose (uint8)(v * 255.0f) is b for all 256 bytes.  planar, unit: 16-byte aligned
 *   a3d_video_to_u8    video: dtype A3D_BF16 / A3D_F16: the VAE decoder's conv_out rows [(n F) H W, 4] (channel 3 is padding; needs W % 4 == 0,
 *                      video 16-byte aligned, dst and the three strides multiples of 4); dtype A3D_F32: a planar video [n, 3, F, H, W] (any W;
 *                      4-byte aligned; any dst and strides).  Pixel (v, f, y, x) goes to dst + v s_view + f s_frame + y s_row + x pixel as
 *                      `pixel` bytes r g b [255]; strides in bytes, >= 0, s_row >= W pixel.  Per value: widen to fp32, t = x / 2 + 0.5,
 *                      clamp to [0, 1], t * 255.0f rounded to fp32, round half to even: (images * 255).round().astype("uint8") of
 *                      VaeImageProcessor.postprocess's (x / 2 + 0.5).clamp(0, 1).  A NaN gives 0 (numpy's cast of a NaN is not defined) */
int a3d_images_in_u8(a3d_stream_t stream, const uint8_t* images, int n, int H, int W, int cin, float* planar, float* unit);
int a3d_video_to_u8(a3d_stream_t stream, const void* video, int dtype, int n, int F, int H, int W, uint8_t* dst, int64_t s_view,
                    int64_t s_frame, int64_t s_row, int pixel);

/* ---------------------------------------------------------------------------------------------------------------------
 * fp16-storage twins.  Every entry point above that reads or writes 16-bit activations / weights exists a second time with
 * IEEE fp16 as the storage type (same signature, same semantics, same fp32 accumulation / statistics / softmax; the MFMA is
 * v_mfma_f32_32x32x16_f16): the dtype the reference's 4D-SDS caller runs the UNet in (animatemv_guidance.py:339-346 casts
 * the model and every input to fp16; BASELINE.json configs 4 and 5).  Built from the same sources with -DA3D_STORAGE_F16:
 * animate3d_amd/build.py compiles a source twice unless its SINGLE_STORAGE tuple lists it, and the fp32-only entry points
 * (the 4-D stage, the optimiser, a3d_channel_mix_f32, a3d_cfg_ddim_step_f32, a3d_version) live in the listed sources and
 * have no twin; a3d_sds_epilogue_bwd_f32 lives in a twin source and is compiled into its bf16 build only.  a3d_im2col_in_f16 / a3d_unpack_out_f16: the CALLER tensor's dtype is still the `dtype` argument,
 * the activation side is fp16; a3d_im2col_in_bwd_f16 reads fp16 dCol rows and still writes fp32.
 * --------------------------------------------------------------------------------------------------------------------- */
int a3d_gemm_f16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                  const float* bias, const void* rowbias, int64_t rb_div, const void* R, int64_t ldr,
                  void* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, float alpha, float beta, int flags);
int a3d_gemm_ws_f16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                    const float* bias, const void* rowbias, int64_t rb_div, const void* R, int64_t ldr,
                    void* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, float alpha, float beta, int flags,
                    void* ws, int64_t ws_bytes, int64_t* ws_needed);
int a3d_gemm2_f16(a3d_stream_t stream, const void* X, int64_t ldx, const void* X2, int64_t ldx2, int64_t K1,
                  const void* W, int64_t ldw, const float* bias, void* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, int flags);
int a3d_gemm_f32out_f16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                         const float* bias, float* Y, int64_t ldy, int64_t M, int64_t N, int64_t K, float alpha);
int a3d_gemm_geglu_f16(a3d_stream_t stream, const void* X, int64_t ldx, const void* W, int64_t ldw,
                        const float* bias, void* Y, int64_t ldy, int64_t M, int64_t N2, int64_t K, int flags);
int a3d_conv3x3_f16(a3d_stream_t stream, const void* X, const void* Wp, const float* bias,
                     const void* rowbias, int64_t rb_div, const void* R, void* Y,
                     int B, int H, int W, int Cin, int Cout, int stride, int up2x, int flags);
int a3d_conv3x3_ws_f16(a3d_stream_t stream, const void* X, const void* Wp, const float* bias,
                       const void* rowbias, int64_t rb_div, const void* R, void* Y,
                       int B, int H, int W, int Cin, int Cout, int stride, int up2x, int flags,
                       void* ws, int64_t ws_bytes, int64_t* ws_needed);
int a3d_conv3x3_up2x_folded_f16(a3d_stream_t stream, const void* X, const void* Wf, const float* bias,
                                const void* rowbias, const void* R, void* Y,
                                int B, int H, int W, int Cin, int Cout, int flags);
int a3d_flash_attn_f16(a3d_stream_t stream, const void* Q, const void* K, const void* V, void* O,
                        const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* omap,
                        int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len,
                        float scale, float out_scale, int accumulate);
int a3d_flash_attn_counted_f16(a3d_stream_t stream, const void* Q, const void* K, const void* V, void* O,
                               const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* omap,
                               int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len,
                               float scale, float out_scale, int accumulate, unsigned int* counters);
int a3d_flash_attn2_f16(a3d_stream_t stream, const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O,
                        const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* kmap2, const a3d_rowmap* omap,
                        int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len, int64_t kv_len2,
                        float scale, float out_scale, float out_scale2, int accumulate);
int a3d_temporal_attn_f16(a3d_stream_t stream, const void* Q, const void* K, const void* V, int64_t ldqkv,
                           void* O, int64_t ldo, int videos, int frames, int64_t L, int heads,
                           int head_dim, float scale);
int a3d_temporal_attn_sharded_f16(a3d_stream_t stream, const void* Q, int64_t ldq, const void* K, const void* V, int64_t ldkv,
                                   void* O, int64_t ldo, int videos, int frames, int64_t L, int heads,
                                   int head_dim, float scale, int q_f0, int q_frames, int kv_frames_per_block,
                                   int64_t kv_block_stride);
int a3d_group_norm_f16(a3d_stream_t stream, const void* X, void* Y, const float* gamma, const float* beta,
                        float* ws, int B, int64_t rows, int C, int groups, float eps, int silu);
int a3d_group_norm2_f16(a3d_stream_t stream, const void* Xa, int Ca, const void* Xb, int Cb, void* Y, const float* gamma,
                        const float* beta, float* ws, int B, int64_t rows, int groups, float eps, int silu);
int a3d_group_norm_sums_f16(a3d_stream_t stream, const void* X, float* ws, double* sums, int B, int64_t rows, int C, int groups);
int a3d_group_norm_apply_f16(a3d_stream_t stream, const void* X, void* Y, const float* gamma, const float* beta,
                              const float* stats, int B, int64_t rows, int C, int groups, int silu);
int a3d_layer_norm_f16(a3d_stream_t stream, const void* X, void* Y1, void* Y2, const float* gamma,
                        const float* beta, int64_t M, int C, float eps,
                        const void* pe1, int64_t pe1_div, int64_t pe1_mod,
                        const void* pe2, int64_t pe2_div, int64_t pe2_mod);
int a3d_geglu_f16(a3d_stream_t stream, const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t M, int64_t N);
int a3d_silu_f16(a3d_stream_t stream, const void* X, void* Y, int64_t n);
int a3d_activation_f16(a3d_stream_t stream, const void* X, void* Y, int64_t n, int mode);
int a3d_concat_f16(a3d_stream_t stream, const void* A, int64_t Ca, const void* Bsrc, int64_t Cb, void* Y, int64_t M);
int a3d_timestep_embed_f16(a3d_stream_t stream, const float* t, void* Y, int V, int dim);
int a3d_im2col_in_f16(a3d_stream_t stream, const void* sample, int dtype, void* Y, int V, int C, int F, int H, int W);
int a3d_unpack_out_f16(a3d_stream_t stream, const void* X, void* Y, int dtype, int V, int C, int F, int H, int W);
int a3d_softmax_rows_f32_f16(a3d_stream_t stream, const float* X, int64_t ldx, void* Y, int64_t ldy, int64_t M, int64_t N);
int a3d_softmax_rows_bwd_f16(a3d_stream_t stream, const void* P, int64_t ldp, const float* dP, int64_t lddp, void* dS, int64_t ldds,
                             int64_t M, int64_t N, float alpha);
int a3d_im2col_in_bwd_f16(a3d_stream_t stream, const void* dCol, float* dX, int V, int C, int F, int H, int W, float scale);
int a3d_flash_attn_bwd_f16(a3d_stream_t stream, const void* Q, const void* K, const void* V, const void* dO,
                            void* dQ, void* dK, void* dV, float* lse2, float* delta,
                            const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* domap,
                            const a3d_rowmap* dqmap, const a3d_rowmap* dkmap,
                            int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len, int q_per_kv,
                            float scale, float do_scale, int accumulate);
int a3d_flash_attn_lse_f16(a3d_stream_t stream, const void* Q, const void* K, const void* V, void* O,
                           const a3d_rowmap* qmap, const a3d_rowmap* kmap, const a3d_rowmap* omap,
                           int groups, int heads, int head_dim, int64_t q_len, int64_t kv_len,
                           float scale, float out_scale, int accumulate, float* lse2);
int a3d_attn_delta_f16(a3d_stream_t stream, const void* dO, const void* O, const a3d_rowmap* domap, const a3d_rowmap* omap,
                       float* delta, int groups, int heads, int head_dim, int64_t q_len);
int a3d_temporal_attn_bwd_f16(a3d_stream_t stream, const void* Q, const void* K, const void* V, int64_t ldqkv,
                               const void* dO, int64_t lddo, void* dQ, void* dK, void* dV, int64_t ldd,
                               int videos, int frames, int64_t L, int heads, int head_dim, float scale);
int a3d_layer_norm_bwd_f16(a3d_stream_t stream, const void* X, const void* dY, const float* gamma, void* dX,
                            float* dgamma, float* dbeta, int64_t M, int C, float eps, int accumulate);
int a3d_group_norm_bwd_f16(a3d_stream_t stream, const void* X, const void* dY, const float* gamma, const float* beta,
                            const float* stats, void* dX, float* ws, float* dgamma, float* dbeta,
                            int B, int64_t rows, int C, int groups, int silu);
int a3d_geglu_bwd_f16(a3d_stream_t stream, const void* P, int64_t ldp, const void* dY, int64_t lddy, void* dP, int64_t lddp,
                       int64_t M, int64_t N);
int a3d_transpose_f16(a3d_stream_t stream, const void* X, int64_t ldx, void* Y, int64_t ldy, int64_t rows, int64_t cols,
                       int64_t rows_pad);
int a3d_colsum_f16(a3d_stream_t stream, const void* X, int64_t ldx, int64_t rows, int64_t cols, float* out, float alpha, int accumulate);
int a3d_axpby_f16(a3d_stream_t stream, const void* X, void* Y, int64_t n, float a, float b);
int a3d_zero_insert2x_f16(a3d_stream_t stream, const void* dY, void* Z, int B, int H, int W, int C);
int a3d_upsample2x_bwd_f16(a3d_stream_t stream, const void* dU, void* dX, int B, int H, int W, int He, int We, int C);
int a3d_wgrad_f16(a3d_stream_t stream, const void* dY, int64_t lddy, const void* X, int64_t ldx, float* dW, int64_t lddw,
                   float* ws, int64_t M, int64_t N, int64_t K, float alpha, int accumulate);
int a3d_sds_pack_f16(a3d_stream_t stream, int b, int n, int f, int c, int P, const float* latents, const float* noise, const int64_t* t,
                     const float* table, int table_len, int dtype, float* latents_noisy, void* sample, void* timestep);
int a3d_sds_epilogue_f16(a3d_stream_t stream, int b, int n, int f, int c, int P, const void* eps, int dtype, const float* latents_noisy,
                         const float* latents, const float* noise, const int64_t* t, const float* table, int table_len,
                         double guidance_scale, double recon_std_rescale, double* stats, int64_t n_stats, float* latents_recon,
                         float* noise_pred, float* partials, int64_t n_partials, float* out);

#ifdef __cplusplus
}
#endif
#endif /* ANIMATE3D_HIP_H */
