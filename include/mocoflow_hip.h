/*
 * mocoflow_hip.h -- C ABI of the MI355X (gfx950) volume-rendering path of MoCo-Flow.
 *
 * The reference (wyysf-98/MoCo_Flow) is pure Python/PyTorch and has NO native
 * boundary of its own; this ABI is the build-defined drop-in surface described in
 * SURVEY.md §8(b).  Every entry point below names the reference interface it
 * replaces (file:line relative to the reference repository).
 *
 * Conventions
 *   - extern "C", POD only: device pointers, 32/64-bit sizes, a hipStream_t passed
 *     as void*.  No torch types, no exceptions, no allocation, no ownership
 *     transfer: the caller allocates every output and workspace buffer.
 *   - All pointers are DEVICE pointers (fp32 / int32 as documented) unless marked
 *     "host".  Descriptor structs are read on the host during the call.
 *   - Return value: 0 = ok; <0 = error (MF_E_*), text via mf_last_error()
 *     (thread-local).  Work is enqueued on `stream`; nothing synchronises.
 *   - The library is stateless; "packed weights" are plain caller-owned device
 *     buffers produced by mf_*_pack from the PyTorch parameter tensors.
 */
#ifndef MOCOFLOW_HIP_H
#define MOCOFLOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: activation dump of the training forward; 4: mf_nerf_backward, mf_weight_grads; 5: NoF backward
 * (mf_nof_points_dump, mf_nof_backward); 6: mf_composite_backward, mf_image_compose;
 * 7: mf_nof_forward_dump; 8: mf_loss_partials, new packed layout of MF_PREC_BF16 (32x32x16 fragments);
 * 9: mf_valid_rays_mask, mf_nerf_backward_x (embedded-input gradient in the chain launch), mf_embedding_backward;
 * 10: mf_nerf_forward_dump, mf_render_args.dump_nof_* (+ mf_nof_emb_slot_features), mf_smpl_lbs,
 *     mf_smpl_frame_transforms, mf_apply_vertex_transforms
 * 12: MF_PREC_BF16 NoF takes its image-index block as a per-ray fp32 bias: mf_render_args.workspace(+_bytes),
 *     mf_render_workspace_bytes, mf_render_prepare, mf_loss_partials_backward, perturb arguments of mf_z_vals, mf_points_sigma_workspace_bytes, workspace arguments of mf_points_sigma_p
 * 13: MF_PREC_BF16X3 is the full three-product mode (own packed layout); mf_weight_grads_p, mf_weight_grads_scratch_bytes_p,
 *     mf_nerf_backward3 (+ mf_nerf_bwd3_packed_bytes, mf_nerf_pack_bwd3), MF_PREC_BF16X3 in mf_points_sigma_p and with the NeRF dump
 * 14: mf_embedding_forward_rows
 * 15: MF_PREC_BF16X3 packs the NoF in three-term operands (six products per k-step); mf_nof_backward3 (+ mf_nof_bwd3_packed_bytes,
 *     mf_nof_pack_bwd3); ReLU bit rows: four panels per word, written for NoF evaluations (behind T) and under NoF; mf_sample_pdf_eps
 * 16: MF_PREC_BF16X3 packs the NoF as IEEE-half (hi, lo) pairs at 2^5 x (three products per k-step on the f16 matrix
 *     instruction, biases at 2^10 x); MF_PREC_BF16X3 training forward under NoF (mf_render_args.dump_nof_acts / dump_nof_out without
 *     dump_nof_emb) + mf_nof_embed_rows
 * additive entries since, version unchanged: mf_mc_scratch_bytes / mf_mc_count / mf_mc_emit; mf_ssim, mf_sqerr (+ their
 *     _scratch_bytes); mf_depth_range, mf_depth_colormap, mf_frame_sheet; mf_points_radiance, mf_mc_normals;
 *     mf_mask_compact (+ mf_mask_compact_scratch_bytes), mf_ray_batch; mf_point_correspond, mf_point_loss_partials
 *     (+ mf_point_loss_partials_scratch_bytes), mf_point_loss_partials_backward; mf_nerf_fold_packed_bytes / mf_nerf_pack_fold
 *     + MF_F_FOLDED_FINAL (the fp32 inference stream with xyz_encoding_final folded into extra_encoding); mf_occ_build
 *     (+ mf_occ_build_scratch_bytes), mf_ray_clip; mf_mesh_label, mf_mesh_table_count / mf_mesh_table_emit, mf_mesh_filter_plan /
 *     mf_mesh_filter_emit (+ their _scratch_bytes), mf_gather_rows; mf_project_vertices, mf_rasterize (+ mf_raster_scratch_bytes),
 *     mf_raster_resolve, mf_raster_interpolate, mf_raster_shade; mf_resize_u8 (+ mf_resize_u8_scratch_bytes), mf_composite_rows,
 *     mf_background_plate; mf_lattice_select (+ mf_lattice_select_scratch_bytes), mf_lattice_points, mf_lattice_scatter;
 *     mf_mask_label (+ mf_mask_label_scratch_bytes), mf_mask_select, mf_mask_fill_holes, mf_mask_table_count / mf_mask_table_emit;
 *     mf_simplify_mesh_plan / mf_simplify_mesh_emit (+ mf_simplify_mesh_scratch_bytes); mf_rings_mesh_plan / mf_rings_mesh_emit
 *     (+ mf_rings_mesh_scratch_bytes), mf_smooth_mesh (+ mf_smooth_mesh_scratch_bytes); mf_voxel_mesh, mf_voxel_fill
 *     (+ mf_voxel_fill_scratch_bytes), mf_voxel_dilate (+ mf_voxel_dilate_scratch_bytes); mf_grid_edt
 *     (+ mf_grid_edt_scratch_bytes); mf_surface_records, mf_surface_closest, mf_surface_weights, mf_surface_sample, mf_surface_stats
 *     (+ mf_surface_stats_scratch_bytes); mf_surface_corners, mf_surface_cast */
#define MF_ABI_VERSION 16

enum {
  MF_OK = 0,
  MF_E_INVALID = -1,     /* bad argument / unsupported configuration */
  MF_E_LAUNCH = -2,      /* HIP launch or runtime failure            */
  MF_E_UNSUPPORTED = -3  /* valid for the reference, not built here  */
};

enum { MF_MAX_FREQS = 16, MF_MAX_LAYERS = 16 };

/* Arithmetic of the W-wide ("hidden") GEMMs of the fused pass.  F32: exact-fp32 MFMA everywhere
 * (the reference's arithmetic; BASELINE configs C1-C2).  BF16: hidden-layer weights and
 * activations rounded to bf16 (RNE), fp32 accumulate (v_mfma_f32_32x32x16_bf16, 32 samples per wave); the
 * embedded-input k-ranges and the NoF head use a two-term bf16 split (16 mantissa bits); biases, the NeRF
 * heads and the composite stay fp32 (BASELINE configs C3-C5).
 * BF16X3 (ABI v12; NoF in three-term bf16 operands in v15, in IEEE-half pairs since v16): the fp32 CONTRACT on the bf16 pipe (1e-4 max-rel on every per-ray
 * output, measured <= 4.6e-5 on the reference-generated golden vectors and <= 3.1e-5 through the MoCo chains at 4096 rays on two
 * weight draws).  The NeRF's matrix products as a two-term bf16 split of activations AND weights (hi + lo, 16 mantissa bits
 * each), three products hi*hi + hi*lo + lo*hi; the NoFs' -- whose output point feeds sin(512 x) -- as IEEE-half (hi, lo) pairs of
 * 2^5 x the value (22 significand bits), the same three products on v_mfma_f32_32x32x16_f16; fp32 accumulation; sigma / rgb heads as fp32 dot products on the fp32 accumulators; the
 * NoF's image index an exact fp32 per-ray bias.  Three matrix instructions per product where F32 costs sixteen:
 * 0.33-0.4 of F32's time.  Own packed layout (every k-step a (hi, lo) group pair: bf16 in the NeRF, halves in the NoF).  Render passes
 * (with the activation dumps of the training forward, v16: under NoF too) and mf_points_sigma_p (scalar
 * image index or no NoF). */
enum { MF_PREC_F32 = 0, MF_PREC_BF16 = 1, MF_PREC_BF16X3 = 2 };

/* ---- Embedding: models/embedding.py:4-47 ------------------------------------
 * out = [x, w0*sin(f0 x), w0*cos(f0 x), w1*sin(f1 x), ...]; freq[] are the module's
 * freq_bands (2^k or linear), weight[] its per-frequency weights (set_weights /
 * trainer_moco_flow.py:289,301).  n_freqs == 0 is legal (identity). */
typedef struct mf_embedding {
  int32_t in_channels;             /* 3 (xyz, dir) or 1 (ind)             */
  int32_t n_freqs;                 /* 0..MF_MAX_FREQS                     */
  float freq[MF_MAX_FREQS];
  float weight[MF_MAX_FREQS];
} mf_embedding;

/* ---- NeRF: models/nerf.py:5-102 ---------------------------------------------
 * Parameter pointers follow the reference's state_dict:
 *   trunk_w[i] / trunk_b[i]  = xyz_encoding_{i+1}.0.{weight,bias}
 *   final_w / final_b        = xyz_encoding_final.{weight,bias}
 *   extra_w / extra_b        = extra_encoding.0.{weight,bias}   (W/2, W+extra_feat_dim)
 *   sigma_w / sigma_b        = sigma.{weight,bias}              (1, W)
 *   rgb_w / rgb_b            = rgb.0.{weight,bias}              (3, W/2)
 * All row-major (out, in) fp32 as nn.Linear stores them. */
enum { MF_EXTRA_NONE = 0, MF_EXTRA_IND = 1, MF_EXTRA_DIR = 2 };

typedef struct mf_nerf_desc {
  int32_t D;                       /* trunk layers, 2..MF_MAX_LAYERS-1       */
  int32_t W;                       /* hidden width: 256 (bf16 modes, backward); the fp32 forward also takes 128 */
  int32_t in_channels_xyz;         /* 63 (= 3*(2*10+1)); narrower embeddings are zero-padded to it by the caller */
  uint32_t skip_mask;              /* bit i set <=> i in skips (nerf.py:84-86) */
  int32_t extra_feat_type;         /* MF_EXTRA_*                             */
  int32_t extra_feat_dim;          /* columns of extra_encoding beyond W     */
  const float* trunk_w[MF_MAX_LAYERS];
  const float* trunk_b[MF_MAX_LAYERS];
  const float* final_w; const float* final_b;
  const float* extra_w; const float* extra_b;
  const float* sigma_w; const float* sigma_b;
  const float* rgb_w;   const float* rgb_b;
} mf_nerf_desc;

/* ---- NoF: models/nof.py:6-85 --------------------------------------------------
 *   trunk_w[i] / trunk_b[i] = nof_encoding_{i+1}.0.{weight,bias}
 *   head_w / head_b         = nof_encoding_final.{weight,bias}  (9|3, W) */
typedef struct mf_nof_desc {
  int32_t D;                       /* trunk layers                           */
  int32_t W;                       /* hidden width: 128                      */
  int32_t in_channels_xyz;         /* 33                                     */
  int32_t extra_feat_dim;          /* 33 (ind embedding width)               */
  uint32_t skip_mask;
  int32_t use_quat;                /* nof.py:75-82                           */
  const float* trunk_w[MF_MAX_LAYERS];
  const float* trunk_b[MF_MAX_LAYERS];
  const float* head_w; const float* head_b;
} mf_nof_desc;

int32_t mf_version(void);
const char* mf_last_error(void);

/* Size in bytes of the packed-weights buffer for a network (0 on unsupported). */
int64_t mf_nerf_packed_bytes(const mf_nerf_desc* d);
int64_t mf_nof_packed_bytes(const mf_nof_desc* d);
/* Re-order the nn.Linear tensors into the kernels' MFMA fragment stream.
 * Must be re-run whenever the parameters change (optimizer.step). */
int32_t mf_nerf_pack(const mf_nerf_desc* d, void* packed, void* stream);
int32_t mf_nof_pack(const mf_nof_desc* d, void* packed, void* stream);
/* The same with an explicit MF_PREC_* (the plain forms are MF_PREC_F32).  A packed buffer can only
 * be used by a render pass of the same precision. */
int64_t mf_nerf_packed_bytes_p(const mf_nerf_desc* d, int32_t precision);
int64_t mf_nof_packed_bytes_p(const mf_nof_desc* d, int32_t precision);
int32_t mf_nerf_pack_p(const mf_nerf_desc* d, int32_t precision, void* packed, void* stream);
int32_t mf_nof_pack_p(const mf_nof_desc* d, int32_t precision, void* packed, void* stream);
/* The fp32 INFERENCE stream of a NeRF with xyz_encoding_final folded into extra_encoding (nerf.py:96-98: the final layer has
 * no activation and extra_encoding is its only consumer; sigma is read in front of it):
 *   extra_encoding(h) = relu(W' h + W_e[:, W:] ext + b'),  W' = W_e[:, :W] W_f,  b' = b_e + W_e[:, :W] b_f
 * for h = the last trunk layer's output.  The stream is mf_nerf_pack's without the final layer's panels (256 of 2320 groups for
 * the default NeRF); the resident block has the same size and offsets, its extra bias is b' and the final layer's bias slot is
 * unused.  A small kernel in front of the pack computes W' and b' -- float64 sums over ascending k, rounded to fp32 once, no
 * atomics: packs are bit-identical -- into a scratch area of round_up((W/2 * W + W/2) * 4, 1024) bytes (129 KiB) that is
 * appended behind the panels and counted by mf_nerf_fold_packed_bytes.  The extra block W_e[:, W:] ext is the same for every
 * sample of a ray: the stream's extra_encoding panels hold W' alone (32 groups each; 2048 groups in all for the default NeRF,
 * where they were 2064) and W_e[:, W:] follows the scratch area as W/2 rows of 32 (dir) | 16 (ind) | 0 (none) floats, natural
 * column order, zero-padded -- the bytes its k-quads took in the panels, so mf_nerf_fold_packed_bytes returns what it did.  The
 * pass adds it to b' once per ray.  The layout is private to the library (pack and pass must come from the same build); the
 * C ABI and MF_ABI_VERSION are unchanged.  fp32 and W = 256 only (0 / MF_E_UNSUPPORTED otherwise);
 * extra_feat_type dir, ind or none.  Read by mf_render_pass with MF_F_FOLDED_FINAL; every other entry point takes the
 * streams of mf_nerf_pack*.  Must be re-run whenever the parameters change. */
int64_t mf_nerf_fold_packed_bytes(const mf_nerf_desc* d);
int32_t mf_nerf_pack_fold(const mf_nerf_desc* d, void* packed, void* stream);

/* Embedding.forward, models/embedding.py:30-47:  x (B, in_channels) -> out (B, C*(2F+1)). */
int32_t mf_embedding_forward(const mf_embedding* e, const float* x, int64_t B, float* out, void* stream);
/* The same for B OUTPUT rows of `out_stride` >= C*(2F+1) floats (the columns past the embedding are written 0;
 * out_stride <= 0: the embedding's width), output row b embedding input row b / repeat (x has ceil(B / repeat)
 * rows): the embedded inputs as the weight-gradient launches read them (64 / 32-column operands of mf_weight_grads;
 * the per-ray `ind` / `dir` embedding of rendering.py:133-146 repeated for the ray's samples) in ONE launch
 * instead of embedding + repeat_interleave + zero pad. */
int32_t mf_embedding_forward_rows(const mf_embedding* e, const float* x, int64_t B, int32_t repeat, float* out,
                                  int64_t out_stride, void* stream);

/* NeRF.forward, models/nerf.py:61-102: inputs (B, in_channels_xyz [+ extra_feat_dim]) row
 * stride `in_stride` floats -> out (B,4) = [rgb, sigma], or (B,1) sigma when sigma_only. */
int32_t mf_nerf_forward(const mf_nerf_desc* d, const void* packed, const float* inputs,
                        int64_t in_stride, int64_t B, int32_t sigma_only, float* out, void* stream);

/* The same call when gradients are wanted (trainer_moco_flow.py:146-157 `forwarf_nerf`, :337-362: NeRF called on
 * embedded points with requires_grad inputs): the full forward (out (B,4)) that also writes the per-sample layer
 * outputs [h_0 .. h_{D-1} | xyz_encoding_final | extra_encoding] to dump_acts (B, dump_stride >= (D+1) W + W/2),
 * the layout mf_nerf_backward / mf_weight_grads consume -- the module-level counterpart of
 * mf_render_args.dump_acts.  (ABI v10) */
int32_t mf_nerf_forward_dump(const mf_nerf_desc* d, const void* packed, const float* inputs, int64_t in_stride,
                             int64_t B, float* out, float* dump_acts, int64_t dump_stride, void* stream);

/* NoF.forward, models/nof.py:55-85: inputs (B, in_channels_xyz+extra_feat_dim), xyz (B,3) -> (B,3). */
int32_t mf_nof_forward(const mf_nof_desc* d, const void* packed, const float* inputs,
                       int64_t in_stride, const float* xyz, int64_t B, float* out, void* stream);

/* ---- backward of NeRF.forward over the training forward's dump (ABI v4) -------------------
 * Replaces the autograd graph torch records for models/nerf.py:78-102 under loss.backward()
 * (trainer/base.py:188-197).  The input-gradient chain (nine W-wide contractions per sample) runs
 * on the same register-resident MFMA core as the forward, on the transposed weights:
 *   mf_nerf_bwd_packed_bytes / mf_nerf_pack_bwd : transposed fragment stream of a NeRF (fp32, W=256);
 *     re-run whenever the parameters change.
 *   mf_nerf_backward : g_out (P,4) = dL/d[rgb (after the sigmoid), sigma], acts (P,stride) and
 *     rgbsigma (P,4) = mf_render_args.dump_acts / dump_rgbsigma of the forward ->
 *       gpre  (round_up(P,128), stride): pre-activation gradients in the dump's layout
 *             [d z_0 .. d z_{D-1} | d xyz_encoding_final | d extra_encoding]  (rows >= P are scratch)
 *       ghead (P,4): [d rgb pre-sigmoid (3), d sigma]
 *     The weight gradients are then plain GEMMs on (acts, gpre):  dW_l = gpre_l^T in_l,  db_l = sum gpre_l. */
int64_t mf_nerf_bwd_packed_bytes(const mf_nerf_desc* d);
int32_t mf_nerf_pack_bwd(const mf_nerf_desc* d, void* packed, void* stream);
int32_t mf_nerf_backward(const mf_nerf_desc* d, const void* packed_bwd, int64_t P, const float* g_out,
                         const float* acts, int64_t stride, const float* rgbsigma, float* gpre,
                         float* ghead, void* stream);

/* The same launch, additionally producing the gradient of the EMBEDDED INPUT (ABI v9): g_emb (P,64), natural column
 * order of the 63-wide xyz embedding (column 63 = 0), = xyz_encoding_1[:, :63]^T d_z_0 + (one skip layer)
 * xyz_encoding_{skip+1}[:, :63]^T d_z_skip, as two more panels of the transposed stream behind the chain; NULL =
 * mf_nerf_backward.  mf_nerf_pack_bwd packs those panels; more than one skip layer: MF_E_UNSUPPORTED. */
int32_t mf_nerf_backward_x(const mf_nerf_desc* d, const void* packed_bwd, int64_t P, const float* g_out,
                           const float* acts, int64_t stride, const float* rgbsigma, float* gpre,
                           float* ghead, float* g_emb, void* stream);
/* The chain of mf_nerf_backward in three bf16 products (ABI v13; csrc/mf_backward_bf16.hip): gradients and transposed
 * weights as (hi, lo) bf16 pairs, fp32 accumulation, ReLU masks from the dump as in the fp32 chain (no unit changes side:
 * the result differs by the 2^-16 of the split operands).  Own packed stream (mf_nerf_bwd3_packed_bytes /
 * mf_nerf_pack_bwd3); same arguments and outputs as mf_nerf_backward_x (g_emb may be NULL).  `mask` (nullable): the
 * forward's mf_render_args.dump_mask rows -- the chain then reads no activation at all (`acts` may be NULL).  W = 256, D >= 2. */
int64_t mf_nerf_bwd3_packed_bytes(const mf_nerf_desc* d);
int32_t mf_nerf_pack_bwd3(const mf_nerf_desc* d, void* packed, void* stream);
int32_t mf_nerf_backward3(const mf_nerf_desc* d, const void* packed_bwd3, int64_t P, const float* g_out,
                          const float* acts, int64_t stride, const float* rgbsigma, float* gpre,
                          float* ghead, float* g_emb, const uint32_t* mask, int64_t mask_stride, void* stream);
/* Backward of Embedding.forward (models/embedding.py:42-46) through the embedded values themselves:
 * g_x[c] = g_emb[c] + sum_k f_k (emb[cos_kc] g_emb[sin_kc] - emb[sin_kc] g_emb[cos_kc]);  g_emb (P, >= C(2F+1))
 * with row stride g_stride, emb = the forward's output rows (stride e_stride), g_x (P, C). */
int32_t mf_embedding_backward(const mf_embedding* e, const float* g_emb, int64_t g_stride, const float* emb,
                              int64_t e_stride, int64_t P, float* g_x, void* stream);

/* Backward of the alpha-composite of nerf_inference (models/rendering.py:157-192) on per-sample planes:
 * g_rgb (N,3) / g_depth (N) / g_opacity (N) (any may be NULL) = dL/d of the pass's outputs ->
 * g_rgbsigma (N*S,4) = dL/d[rgb (after the sigmoid), raw sigma] per sample, ready for mf_nerf_backward.
 * rgbsigma = mf_render_args.dump_rgbsigma of the forward; z_vals / noise / activation / background as in
 * the forward.  Nothing flows to z_vals (rendering.py:323).  S <= 2048. */
int32_t mf_composite_backward(const float* rays, int64_t ray_stride, int64_t n_rays, int32_t S,
                              const float* z_vals, const float* rgbsigma, const float* noise,
                              int32_t activation, const float* background, const float* g_rgb,
                              const float* g_depth, const float* g_opacity, float* g_rgbsigma, void* stream);

/* Weight / bias gradients of a set of linear layers over P samples, ONE persistent launch:
 *     dW_i = G_i[:P]^T X_i[:P]   (n_out x n_in),      db_i = sum_s G_i[s]   (n_out)
 * G_i / X_i: fp32 row-major device matrices (column slices of the mf_nerf_backward gradient buffer, of
 * the forward's activation dump, or of the embedded inputs), 16-byte aligned, strides multiples of 4
 * floats.  Supported blocks (n_out x n_in): NeRF 256x256, 256x64, 128x256, 128x32 and 4x640 (the two heads
 * at once: G = ghead (P,4), X = dump columns [h_D | final | extra]; no head reads `final`: its 256 columns
 * are not fetched and columns 256..511 of this block's dW are returned as 0); NoF 128x128, 128x80 (embedded input,
 * 66 -> 80) and 12x128 (head, G = d T padded to 12 columns).  dW is written as a dense
 * (max(n_out,16), n_in) matrix, db (optional, may be NULL) as max(n_out,16) floats.  Deterministic
 * (fixed-order partial sums through `scratch`, no atomics).  Replaces the dW/db halves of torch's
 * addmm backward for models/nerf.py:78-102. */
#define MF_WG_MAX_ITEMS 32
typedef struct mf_wgrad_item {
  const float* G; int64_t g_stride; int32_t n_out;
  const float* X; int64_t x_stride; int32_t n_in;
  float* dW; float* db;
} mf_wgrad_item;
int64_t mf_weight_grads_scratch_bytes(const mf_wgrad_item* items, int32_t n_items, int64_t P);
int32_t mf_weight_grads(const mf_wgrad_item* items, int32_t n_items, int64_t P, void* scratch, void* stream);
/* The same with the arithmetic of the contraction chosen (ABI v13).  MF_PREC_F32: exact-fp32 MFMA (the two calls above).
 * MF_PREC_BF16X3: every block but the heads' 4x640 (round 5; before: 256x256 and 128x256 only) contracts G and X as two-term
 * bf16 splits, three bf16 products per 16-sample step with fp32 accumulation (16 mantissa bits per operand; a fifth of the
 * fp32 pipe's matrix time, the launch then runs against the HBM reads of its operands) -- 256x64 on a 256x128 block, the NoF's
 * 128x128 / 128x80 / 12x128 and 128x32 on a 128x128 block, columns beyond the operands' widths zero; dW keeps the (rows, n_in)
 * layout of the fp32 call, the operand strides must be even.  The heads block stays fp32.  The scratch size depends on the
 * precision. */
int64_t mf_weight_grads_scratch_bytes_p(int32_t precision, const mf_wgrad_item* items, int32_t n_items, int64_t P);
int32_t mf_weight_grads_p(int32_t precision, const mf_wgrad_item* items, int32_t n_items, int64_t P, void* scratch, void* stream);

/* ---- backward of one NoF evaluation on points (rendering.py:49-83 + nof.py:69-82; ABI v5) ---------
 * mf_nof_points_dump: pts (P,3), per-ray image index ind[ray * ind_stride] with ray = sample / S ->
 *   out (P,3) and the dump the backward reads: acts (P,stride) = [h_1 .. h_D | T padded to 16],
 *   emb (P,80) = the embedded input [xyz 33 | ind 33 | 0] in the reference's column order.
 * mf_nof_bwd_packed_bytes / mf_nof_pack_bwd: transposed fragment stream (W=128, at most one skip layer).
 * mf_nof_backward: g_out (P,3) = dL/d out -> g_pts (P,3, may be NULL) = dL/d pts and
 *   gpre (round_up(P,128), stride) = [d z_0 .. d z_{D-1} | d T padded to 16] for mf_weight_grads. */
int32_t mf_nof_points_dump(const mf_nof_desc* d, const void* packed, const mf_embedding* emb_xyz,
                           const mf_embedding* emb_ind, const float* pts, const float* ind,
                           int64_t ind_stride, int32_t S, int64_t P, float* out, float* acts,
                           int64_t stride, float* emb, void* stream);
/* NoF.forward (models/nof.py:55-85) on pre-embedded inputs, storing the same activation dump: the forward
 * half of the module-level training call (trainer_nof.py:85-112, trainer_moco_flow.py:159-187). */
int32_t mf_nof_forward_dump(const mf_nof_desc* d, const void* packed, const float* inputs, int64_t in_stride,
                            const float* xyz, int64_t B, float* out, float* acts, int64_t stride, void* stream);
int64_t mf_nof_bwd_packed_bytes(const mf_nof_desc* d);
int32_t mf_nof_pack_bwd(const mf_nof_desc* d, void* packed, void* stream);
int32_t mf_nof_backward(const mf_nof_desc* d, const void* packed_bwd, const mf_embedding* emb_xyz, int64_t P,
                        const float* pts, const float* acts, int64_t stride, const float* g_out,
                        float* gpre, float* g_pts, void* stream);
/* mf_nof_backward in three bf16 products (ABI v15; csrc/mf_nofgrad_bf16.hip): the hidden contractions and the embedded-input
 * layers on gradients and transposed weights as (hi, lo) bf16 pairs with fp32 accumulation, ReLU masks from the dump as in
 * the fp32 kernel (no unit changes side), the transform's backward / head product / sin-cos chain rule in fp32.  Own packed
 * stream (mf_nof_bwd3_packed_bytes / mf_nof_pack_bwd3); same arguments and outputs as mf_nof_backward; dump rows 16-byte
 * aligned.  Replaces the same autograd range: models/rendering.py:49-83 + models/nof.py:69-82 under loss.backward()
 * (trainer/base.py:188-197). */
int64_t mf_nof_bwd3_packed_bytes(const mf_nof_desc* d);
int32_t mf_nof_pack_bwd3(const mf_nof_desc* d, void* packed, void* stream);
int32_t mf_nof_backward3(const mf_nof_desc* d, const void* packed_bwd3, const mf_embedding* emb_xyz, int64_t P,
                         const float* pts, const float* acts, int64_t stride, const float* g_out,
                         float* gpre, float* g_pts, void* stream);

/* Fused point query: xyz (B,3) -> [backward NoF at image index ind] -> positional encoding -> NeRF
 * trunk -> raw sigma (B,), one launch.  Replaces the per-chunk module sequence forward_nof /
 * nerf_embedding_xyz / zero-pad / NeRF(sigma_only=True) of trainer_moco_flow.py:146-187 and the
 * lattice loop of visualize_mesh (trainer_moco_flow.py:500-526, trainer_nerf.py:215-245).
 * nof == NULL: canonical-space query.  ind: per-point indices (B,) or NULL -> ind_scalar for all.
 * canon (B,3), optional: the point after the backward flow. */
int32_t mf_points_sigma(const mf_nerf_desc* nerf, const void* nerf_packed, const mf_embedding* emb_xyz,
                        const mf_nof_desc* nof, const void* nof_packed, const mf_embedding* nof_emb_xyz,
                        const mf_embedding* nof_emb_ind, const float* xyz, const float* ind,
                        float ind_scalar, int64_t B, float* sigma, float* canon, void* stream);
/* The same query with the arithmetic of `precision` (MF_PREC_F32 | MF_PREC_BF16 | MF_PREC_BF16X3; the packed buffers must
 * have been packed for it): bf16 runs the hidden GEMMs of both networks on the bf16 matrix pipe like mf_render_pass does
 * (inference only; the 512^3 mesh-extraction lattice of test.py in ~0.15 s instead of ~0.9 s); bf16x3 (ABI v13) the
 * three-product kernels (fp32-class, ~0.3 s), with `ind` == NULL only (scalar image index, or no NoF): a per-point index
 * tensor returns MF_E_UNSUPPORTED.  (ABI v11) */
int32_t mf_points_sigma_p(int32_t precision, const mf_nerf_desc* nerf, const void* nerf_packed, const mf_embedding* emb_xyz,
                          const mf_nof_desc* nof, const void* nof_packed, const mf_embedding* nof_emb_xyz,
                          const mf_embedding* nof_emb_ind, const float* xyz, const float* ind,
                          float ind_scalar, int64_t B, float* sigma, float* canon, void* workspace,
                          int64_t workspace_bytes, void* stream);
/* Bytes of `workspace` the bf16 query needs when a NoF is given (ABI v12): the per-point (ind array) or single
 * (ind_scalar) fp32 bias  b_l + W_l[:, 33:66] emb(ind)  of the NoF layers that consume the embedded input -- in bf16 mode
 * the image index does not go through the matrix pipe (see mf_render_args.workspace).  0 for MF_PREC_F32 / no NoF. */
int64_t mf_points_sigma_workspace_bytes(int32_t precision, const mf_nof_desc* nof, int32_t per_point_ind, int64_t B);

/* Fused point radiance query, fp32: the whole of NeRF.forward on free points in one launch -- xyz (B,3) -> [backward NoF at
 * image index ind] -> positional encoding -> NeRF trunk -> sigma head, xyz_encoding_final, extra_encoding over the extra block
 * embedded in registers, rgb sigmoid.  out (B,4) = [rgb | raw sigma], the column order of NeRF.forward (models/nerf.py:101;
 * 16-byte aligned); canon (B,3), optional: the point after the backward flow (ignored without a NoF).  Replaces the module
 * sequence NoF -> Embedding -> zero-pad -> Embedding of the extra block -> NeRF.forward and its padded (B, 63 + extra) rows.
 * The extra block follows nerf_inference (models/rendering.py:133-142) by nerf->extra_feat_type:
 *   MF_EXTRA_DIR : view_dirs (B,3) through emb_extra (3 channels, <= 4 frequencies), embedded AS GIVEN (nothing normalises
 *                  it), zero-padded to extra_feat_dim;
 *   MF_EXTRA_IND : the image index -- ind (B,) or, ind == NULL, ind_scalar: the value that also drives the NoF, as ray
 *                  column 8 does in render_rays -- through emb_extra (1 channel, <= 2 frequencies);
 *   MF_EXTRA_NONE: no extra block; emb_extra and view_dirs are not read.
 * nof == NULL: canonical-space query.  Returns MF_E_INVALID for a null argument (emb_extra / view_dirs where the type needs
 * them) and for an extra embedding of the wrong channel count, with more frequencies than above or wider than
 * extra_feat_dim; MF_E_UNSUPPORTED for a NeRF the packed layout does not cover or with W != 256, an xyz embedding other than
 * (3, <= 10 frequencies), a NoF the layout does not cover.  B == 0: MF_OK, nothing launched. */
int32_t mf_points_radiance(const mf_nerf_desc* nerf, const void* nerf_packed, const mf_embedding* emb_xyz,
                           const mf_embedding* emb_extra, const mf_nof_desc* nof, const void* nof_packed,
                           const mf_embedding* nof_emb_xyz, const mf_embedding* nof_emb_ind, const float* xyz,
                           const float* view_dirs, const float* ind, float ind_scalar, int64_t B, float* out,
                           float* canon, void* stream);

/* ---- one rendering pass: nof_inference* + nerf_inference of models/rendering.py:49-192 as
 * called from render_rays (rendering.py:262-314 coarse, 329-373 fine) -------------------- */
enum {
  MF_ACT_RELU = 0, MF_ACT_SOFTPLUS = 1        /* rendering.py:169-172 */
};
enum {
  MF_F_SIGMA_ONLY   = 1 << 0,  /* weights_only=True: no rgb/depth (rendering.py:290-294)   */
  MF_F_CHAIN_LOCAL  = 1 << 1,  /* fw(bw(x,i),i) consensus (rendering.py:275-277)            */
  MF_F_CHAIN_GLOBAL = 1 << 2,  /* fw_i(bw_j(fw_j(bw_i(x)))) (rendering.py:279-282)          */
  MF_F_FOLDED_FINAL = 1 << 3   /* nerf_packed is the stream of mf_nerf_pack_fold: MF_PREC_F32 only (bf16 / bf16x3:
                                * MF_E_UNSUPPORTED), no dump_* pointer (MF_E_INVALID); results differ from the unfolded
                                * pass by the rounding of W' alone (rgb ~2e-7 max-rel; sigma, depth, opacity, weights: none) */
};

typedef struct mf_render_args {
  /* rays (N, ray_stride>=9|10): o(3) d(3) near far img_ind [chained_img_ind]
   * (rendering.py:237-242) */
  const float* rays; int64_t ray_stride; int64_t n_rays;
  const float* background;          /* (N,3) or NULL (rendering.py:189-190)              */
  int32_t n_samples;                /* S of this pass                                     */
  /* depths: either z_vals (N,S) explicit (perturbed / fine pass), or z_steps (S,)
   * = torch.linspace(0,1,S) with use_disp choosing rendering.py:247 vs :249 */
  const float* z_vals; const float* z_steps; int32_t use_disp;
  const float* noise;               /* (N,S) sigma noise already scaled by noise_std, or NULL */
  int32_t activation;               /* MF_ACT_*                                           */
  int32_t flags;                    /* MF_F_*                                             */
  /* canonical NeRF */
  const mf_nerf_desc* nerf; const void* nerf_packed;
  mf_embedding emb_xyz;             /* nerf_embeddings[0]                                 */
  mf_embedding emb_extra;           /* nerf_embeddings[1] (ind) or [2] (dir); ignored for none */
  /* neural motion flow (NULL => plain NeRF) */
  const mf_nof_desc* nof_bw; const void* nof_bw_packed;
  const mf_nof_desc* nof_fw; const void* nof_fw_packed;
  mf_embedding nof_emb_xyz, nof_emb_ind;
  /* outputs (any may be NULL) */
  float* rgb;                       /* (N,3) */
  float* depth;                     /* (N,)  */
  float* opacity;                   /* (N,)  weights.sum(1)                               */
  float* weights;                   /* (N,S) */
  float* alphas;                    /* (N,S) */
  float* disp_local;                /* (N,S) mean_c |xyz - recon|         (rendering.py:310-311) */
  float* disp_global;               /* (N,S) mean_c |xyz - chained_recon| (rendering.py:313-314) */
  int32_t precision;                /* MF_PREC_*: must match how every *_packed buffer was packed      */
  /* training forward (MF_PREC_F32 only; all optional): what the backward needs, written once by the
   * fused kernel instead of being recomputed.  dump_acts (N*S, dump_stride): per sample the NeRF's
   * post-activation layer outputs in natural feature order [h_0 | ... | h_{D-1} | xyz_encoding_final |
   * extra_encoding] (dump_stride >= (D+1)*W + W/2 floats); dump_rgbsigma (N*S, 4): per-sample rgb (after
   * the sigmoid) and raw sigma; dump_xyz (N*S, 3): the point fed to the NeRF (canonical under NoF). */
  float* dump_acts; int64_t dump_stride;
  float* dump_rgbsigma;
  float* dump_xyz;
  /* The same for the NoF evaluations of the chain program (rendering.py:270-282), one plane per step k in
   * [bw(x,i), fw(canon,i), fw(canon,j), bw(.,j), fw(.,i)] (as many as the flags run), each N*S rows:
   * dump_nof_acts (steps, N*S, dump_nof_stride): [h_1 | ... | h_D | T (9 | 3) zero-padded to 16]
   * (dump_nof_stride >= D*W + 16), dump_nof_emb (steps, N*S, 80): the embedded input [xyz 33 | ind 33] in the
   * kernel's register-slot order (column c holds reference column mf_nof_emb_slot_features()[c], -1 = zero pad: the
   * weight gradient taken against it is un-permuted once per launch, on 128 x 80 numbers),
   * dump_nof_out (steps, N*S, 3): the step's output points.  This is what mf_nof_points_dump writes for one
   * evaluation (there in natural column order); with it the backward needs no forward re-evaluation of the chains.
   * All three or none.  dump_nof_plane[k] = plane (0 .. steps-1, a permutation) that step k writes: lets the caller
   * keep the evaluations of one network adjacent (bw: steps 0, 3; fw: steps 1, 2, 4), so that its weight gradients
   * are one contraction over all of them. */
  float* dump_nof_acts; int64_t dump_nof_stride;
  float* dump_nof_emb;
  float* dump_nof_out;
  int32_t dump_nof_plane[5];
  /* MF_PREC_BF16 with NoF (ABI v12): caller-allocated device scratch of mf_render_workspace_bytes(a) bytes holding,
   * per ray and (network, image index) combination of the chain program, the fp32 vectors  b_l + W_l[:, 33:66] emb(ind)
   * of the NoF layers that consume the embedded input (models/rendering.py:73-75, models/nof.py:69-73: the index block
   * is constant along a ray).  mf_render_prepare fills it (one small launch); mf_render_pass reads it as those layers'
   * initial accumulator values.  Ignored (may be NULL) otherwise. */
  void* workspace; int64_t workspace_bytes;
  /* ReLU bit mask of the NeRF's dumped activations (ABI v13; with dump_acts; ABI v15: passes with NoF too; NULL = none): dump_mask (N*S, dump_mask_stride
   * >= 8 (D + 2) words): layer l owns words 8 l .. 8 l + 7; output 32 t + f (f < 32) of the layer sits in word
   * 8 l + 4 (t / 4) + (f % 16) / 4 at bit 8 (t % 4) + 4 (f / 16) + f % 4 (ABI v15: the forward kernels' lane order, one 4-byte store per lane
   * and four 32-row panels; v13 / v14 stored a byte per panel) -- for the trunk layers
   * l = 0 .. D-1 and extra_encoding (l = D + 1, 4 words; l = D, xyz_encoding_final, is not written: no activation) -- what
   * mf_nerf_backward3 needs of the activations: 32 bytes instead of 1 KiB per layer and sample. */
  uint32_t* dump_mask; int64_t dump_mask_stride;
} mf_render_args;

/* mf_render_prepare(a) must have run on the same stream with the same rays / NoFs / nof_emb_ind / chain flags whenever
 * mf_render_workspace_bytes(a) > 0; the coarse and the fine pass of one render_rays call share one prepared workspace
 * (same rays, same NoFs).  A no-op (MF_OK) when no workspace is needed. */
int32_t mf_render_prepare(const mf_render_args* a, void* stream);
int32_t mf_render_pass(const mf_render_args* a, void* stream);
int64_t mf_render_workspace_bytes(const mf_render_args* a);

/* Column map of mf_render_args.dump_nof_emb: features80[c] = column of the NoF's embedded input ([xyz 33 | ind 33])
 * stored at dump column c, or -1 (zero).  Host-side, no stream. */
int32_t mf_nof_emb_slot_features(int32_t* features80);

/* The embedded input of a NoF evaluation as rows, NATURAL column order (ABI v16): out (P, 80) = [emb_xyz(pts) zero-padded to 33 |
 * ind_emb[r / S] (ind_width <= 33 columns: the index embedding of the point's ray, embedded ONCE per ray by the caller,
 * mf_embedding_forward) | 0], row r belongs to ray r / S.  Reference: models/rendering.py:70-75, models/embedding.py:42-47.
 * The X operand of the NoF's 128 x 80 weight-gradient blocks for training forwards that do not write
 * mf_render_args.dump_nof_emb themselves (MF_PREC_BF16X3).  xyz embedding: 3 channels, <= 5 frequencies. */
int32_t mf_nof_embed_rows(const mf_embedding* emb_xyz, const float* pts, const float* ind_emb, int32_t ind_width, int32_t S,
                          int64_t P, float* out, void* stream);

/* ---- hierarchical resampling: sample_pdf (rendering.py:5-46) [+ cat + sort, :321-326] ------
 * General form.  Per ray: n_bins bin positions -- either explicit `bins` (N, n_bins), the
 * reference's first argument, or the mid-points of z_coarse (N, n_bins+1) (rendering.py:321) --
 * and n_bins-1 weights starting at weights + ray*w_stride.  u: uniform draws (N, M) with row
 * stride u_stride, or ONE shared row with u_stride = 0 (the deterministic linspace(0,1,M)).
 * cdf_in (N, n_bins), optional: use this cdf instead of normalising/summing the weights.
 * Outputs (each optional): z_new_out (N,M) the drawn samples; inds_out (N,M) int32 the
 * searchsorted(right=True) indices; z_sorted_out (N, n_bins+1+M) = sort(cat(z_coarse, samples))
 * (needs z_coarse). */
int32_t mf_sample_pdf(const float* bins, const float* z_coarse, const float* weights, int64_t w_stride,
                      int64_t n_rays, int32_t n_bins, int32_t M, const float* u, int64_t u_stride,
                      const float* cdf_in, float* z_new_out, int32_t* inds_out, float* z_sorted_out,
                      void* stream);
/* The same with sample_pdf's `eps` argument (rendering.py:5, :20, :41-42; ABI v15): mf_sample_pdf is eps = 1e-5, the value of
 * every call the reference makes. */
int32_t mf_sample_pdf_eps(const float* bins, const float* z_coarse, const float* weights, int64_t w_stride,
                          int64_t n_rays, int32_t n_bins, int32_t M, const float* u, int64_t u_stride,
                          const float* cdf_in, float* z_new_out, int32_t* inds_out, float* z_sorted_out,
                          float eps, void* stream);
/* render_rays' use of it: z_coarse (N,S), weights (N,S) of the coarse pass (the kernel takes
 * weights[:,1:-1]); u (N,M) draws; writes the sorted union z_out (N,S+M). */
int32_t mf_sample_pdf_merge(const float* z_coarse, const float* weights, int64_t n_rays,
                            int32_t S, int32_t M, const float* u, float* z_out,
                            int32_t* inds_out, float* z_new_out, void* stream);

/* ---- consensus compaction, rendering.py:306-314: mask = alphas >= 0.01 (all-true if none);
 * out[k] = vals[p_k] for masked positions in row-major (ray, sample) order.
 * count (device int64[1]) receives the number of outputs; scratch >= mf_compact_scratch_bytes. */
int64_t mf_compact_scratch_bytes(int64_t n_rays);
int32_t mf_compact_mask(const float* alphas, const float* vals_a, const float* vals_b,
                        int64_t n_rays, int32_t S, float* out_a, float* out_b,
                        int64_t* count, void* scratch, void* stream);

/* ---- fused loss partials (second half): the additive pieces of MSELoss over both passes
 * (models/losses.py:4-14) and of the consensus means over mask = alphas >= 0.01, all-true if none
 * (models/rendering.py:306-314, trainer/trainer_moco_flow.py:317-328), from the arrays a render pass already wrote:
 * no mask compaction, no data-dependent length, no host sync.  out12 (device, 12 doubles) = one (sum, count) pair
 * per term the reference averages separately:
 *   [0:4]  sum (rgb_coarse - target)^2, 3N | sum (rgb_fine - target)^2, 3N
 *   [4:8]  sum_masked disp_local_coarse, n_masked | ... fine        (disp_* = mf_render_args.disp_local/global planes)
 *   [8:12] sum_masked disp_global_coarse, n_masked | ... fine
 * A NULL array (or a NULL `fine`) leaves its pair at (0, 0).  loss terms = sum / count; the multi-GPU caller
 * all-reduces the 96 bytes first.  Deterministic (fixed-order partial sums through `scratch`). */
typedef struct mf_loss_pass {
  const float* rgb;          /* (N,3) rendered colour of the pass, or NULL            */
  const float* alphas;       /* (N,S) of the pass: the consensus mask source, or NULL */
  const float* disp_local;   /* (N,S) or NULL                                         */
  const float* disp_global;  /* (N,S) or NULL                                         */
  int32_t n_samples;         /* S of the pass                                         */
} mf_loss_pass;
int64_t mf_loss_partials_scratch_bytes(void);
/* means6 (device, 6 floats, optional; ABI v12): sum / count of each pair in fp32 -- what torch.mean of the corresponding
 * vector returns (nan for an empty one) -- so that a mean-only caller launches nothing else. */
int32_t mf_loss_partials(const mf_loss_pass* coarse, const mf_loss_pass* fine, const float* target, int64_t n_rays,
                         double* out12, float* means6, void* scratch, void* stream);

/* Backward of mf_loss_partials (ABI v12): the training-mode loss epilogue.  g12 (device, 12 doubles) = dL/d out12 (only the
 * six sums carry a gradient; out12 = the forward's result, its counts tell whether the consensus mask fell back to
 * all-true).  Writes the gradient seeds the backward nodes of the pass consume, each buffer whole:
 *   g_rgb (N,3)              = g12[2q] * 2 (rgb - target)                               models/losses.py:4-14
 *   g_recon_local  (N*S,3)   = g12[4+2q] * mask * (-sign(x - recon_local)) / 3           models/rendering.py:310-311
 *   g_recon_global (N*S,3)   = g12[8+2q] * mask * (-sign(x - recon_global)) / 3          models/rendering.py:313-314
 * x = o + d z (rays columns 0-5, z_vals (N,S)); recon_* = the output points of the chain's last forward-flow evaluation
 * (mf_render_args.dump_nof_out planes of steps 1 / 4).  Any output pointer may be NULL. */
typedef struct mf_loss_grad_pass {
  const float* rgb; float* g_rgb;
  const float* alphas; int32_t n_samples;
  const float* rays; int64_t ray_stride; const float* z_vals;
  const float* recon_local; float* g_recon_local;
  const float* recon_global; float* g_recon_global;
} mf_loss_grad_pass;
int32_t mf_loss_partials_backward(const mf_loss_grad_pass* coarse, const mf_loss_grad_pass* fine, const float* target,
                                  int64_t n_rays, const double* out12, const double* g12, void* stream);

/* The sample depths of a pass as render_rays materialises them when something outside the fused kernel needs them
 * (the resample, stratified jitter, the backward): z_out (N, S) = near*(1-t) + far*t, or 1/(1/near*(1-t) + 1/far*t)
 * with use_disp (models/rendering.py:245-251; near / far = columns 6 / 7 of the ray rows, t = z_steps (S) = linspace(0,1,S));
 * every product and sum separately rounded, bit-identical to the torch expression and to the fused pass's own z.
 * perturb_rand (N, S) uniform draws, or NULL (ABI v12): the stratified jitter of rendering.py:253-260 in the same launch,
 * z = lower + (upper - lower) * (perturb * rand) with lower / upper the neighbouring mid-points (the ray's ends at the
 * ends), again bit-identical to the torch expression. */
int32_t mf_z_vals(const float* rays, int64_t ray_stride, int64_t n_rays, const float* z_steps, int32_t n_samples,
                  int32_t use_disp, const float* perturb_rand, float perturb, float* z_out, void* stream);

/* ---- producers either side of the path -----------------------------
 * Camera.make_rays (utils/camera.py:134-148 with gen_ray_directions :29-50 and gen_rays :52-81):
 * rays_out (H*W, 9) = [o(3), unit d(3), near, far, idx], pixel order row-major; the direction is
 * ((i-cx)/focal, -(j-cy)/focal, -1) rotated by c2w[:, :3] (host pointer to the 3x4 row-major matrix, or
 * NULL for camera coordinates).  near/far/idx are the scalars make_rays broadcasts. */
int32_t mf_make_rays(int32_t H, int32_t W, float focal, float cx, float cy, const float* c2w_host,
                     float nearv, float farv, float idx, float* rays_out, void* stream);
/* Camera.get_valid_rays_mask (utils/camera.py:119-132): mask_out (H*W bytes, device, row-major) = 1 inside the filled
 * convex hull of the projected AABB corners pts_xy (host, n_pts x (x = column, y = row) int32: the output of
 * calculate_2d_projections, camera.py:83-103), else 0.  Hull on the host, fill on the device, one thread per pixel.
 * Rule = cv2.fillConvexPoly's scan-line fill (line_type 8) with exact intersections: row y in [ymin, ymax] sets
 * pixels round_half_up(XL(y)) .. round_half_up(XR(y)).  PARITY UNPINNED vs cv2 itself (absent from the image). */
int32_t mf_valid_rays_mask(int32_t H, int32_t W, const int32_t* pts_xy_host, int32_t n_pts, uint8_t* mask_out,
                           void* stream);
/* Foreground scatter-back of the full-image drivers (MoCoFlowTrainer.render trainer_moco_flow.py:249-266,
 * NeRFTrainer.render trainer_nerf.py:128-140), on the device: for every pixel b of the (B) image
 *   not rendered (rays_msk[b] == 0)            -> img = background[b], depth = 10
 *   rendered, opacity[rank[b]] > 0             -> img = rgb[rank[b]],  depth = depth[rank[b]]
 *   rendered, opacity == 0                     -> img = background[b], depth = 8
 * rays_msk (B) bytes or NULL (all rendered, rank may be NULL); rank (B) int64 = position of pixel b among
 * the rendered rays. */
int32_t mf_image_compose(const uint8_t* rays_msk, const int64_t* rank, int64_t B, const float* opacity,
                         const float* rgb, const float* depth, const float* background, float* img,
                         float* depth_out, void* stream);

/* knn_cuda.KNN(k=1, transpose_mode=True) of the vendored wheel (datasets/moco_flow_dataset.py:35,120):
 * ref (V,3), query (Q,3) -> dist (Q,) Euclidean distance to, and ind (Q,) int64 0-based index of, the
 * nearest reference point; first minimum on ties. */
int32_t mf_knn1(const float* ref, int64_t V, const float* query, int64_t Q, float* dist, int64_t* ind,
                void* stream);

/* ---- SMPL linear blend skinning + per-vertex frame transforms (ABI v10) ------------
 * The model arrays of utils/smpl/smpl_model.py:60-82 as device pointers (fp32, row-major):
 *   v_template (V,3), shapedirs (V*3,10) [= shapedirs[:, :, :10]], posedirs (V*3,207), j_regressor (24,V) dense,
 *   weights (V,24); parent[i] (i = 1..23) = index of joint i's parent (an earlier joint), parent[0] ignored. */
typedef struct mf_smpl_model {
  int32_t n_verts;
  const float* v_template;
  const float* shapedirs;
  const float* posedirs;
  const float* j_regressor;
  const float* weights;
  int32_t parent[24];
} mf_smpl_model;

/* SMPL.forward (smpl_model.py:96-139) and SMPL.get_vertex_transformation (:141-186) in one call:
 * pose (B,72) axis-angle, or (B,24,3,3) rotation matrices when pose_is_rotmat; betas (B,10) ->
 * verts (B,V,3) and / or T (B,V,4,4) (either may be NULL).  scratch: mf_smpl_scratch_bytes(V,B) bytes. */
int64_t mf_smpl_scratch_bytes(int64_t n_verts, int64_t B);
int32_t mf_smpl_lbs(const mf_smpl_model* m, const float* pose, int32_t pose_is_rotmat, const float* betas, int64_t B,
                    float* verts, float* T, void* scratch, void* stream);

/* datasets/moco_flow_dataset.py:96-99: trans (V,4,4) = T_tgt @ inverse(T_src), per vertex. */
int32_t mf_smpl_frame_transforms(const float* T_src, const float* T_tgt, int64_t V, float* trans, void* stream);

/* datasets/moco_flow_dataset.py:127-129: cano (Q,3) = (trans[ind] @ [query, 1])[:3]; ind (Q,) int64 into the V
 * transforms (mf_knn1's output).  An index outside [0, V - 1] is clamped to that range before any address is formed:
 * a negative one reads transform 0, one >= V reads transform V - 1. */
int32_t mf_apply_vertex_transforms(const float* trans, const int64_t* ind, int64_t V, const float* query, int64_t Q,
                                   float* cano, void* stream);

/* ---- marching cubes: mcubes.marching_cubes of visualize_mesh (trainer_moco_flow.py:528-532, trainer_nerf.py:247-251)
 * on the device.  vol: C-contiguous fp32 (n0, n1, n2), each side >= 2, at most 2^31 - 1 points (else MF_E_INVALID);
 * clamp_zero != 0 reads every value as v < 0 ? 0 : v (the reference's np.maximum(sigma, 0)).  A corner is below iff v < iso.
 * One vertex per crossing lattice edge (p, axis), at p + t e_axis in index coordinates of vol's axes, t = (iso - f(p)) /
 * (f(p + e_axis) - f(p)) in fp32; vertices sorted by 3 p + axis (p: C-order point index), triangles by the C-order index of
 * their cell, within a cell in the order of the case table (mf_mc_tables.hpp: classic Lorensen-Cline, scikit-image's
 * triangulation and raw winding).  Deterministic: bit-identical from run to run.
 * Bytes of the caller's scratch (or MF_E_INVALID on a bad shape): 4 per lattice point + 24 per 1024 points. */
int64_t mf_mc_scratch_bytes(int64_t n0, int64_t n1, int64_t n2);
/* Pass 1: classify the volume and write counts (device int64[2]) = [V, T]; scratch keeps what mf_mc_emit needs. */
int32_t mf_mc_count(const float* vol, int64_t n0, int64_t n1, int64_t n2, float iso, int32_t clamp_zero,
                    void* scratch, int64_t* counts, void* stream);
/* Pass 2, after mf_mc_count on the same stream with the same vol / shape / iso / clamp_zero / scratch: verts (V, 3) fp32 and
 * tris (T, 3) int64 vertex indices, sized by the counts pass 1 wrote (NULL only when that count is 0). */
int32_t mf_mc_emit(const float* vol, int64_t n0, int64_t n1, int64_t n2, float iso, int32_t clamp_zero,
                   const void* scratch, float* verts, int64_t* tris, void* stream);
/* Unit normals (V, 3) of vertices verts (V, 3) given in index coordinates of vol (mf_mc_emit's), from the volume's gradient;
 * one thread per vertex (tests/mesh_color_oracle.py restates it in numpy).  v = vol, or max(vol, 0) with clamp_zero.
 * Lattice gradient g(q): per axis the central difference (v(q + e_k) - v(q - e_k)) / 2, on a border face the one-sided
 * difference.  Vertex p: i_k = min(floor(p_k), n_k - 1) (0 for p_k < 0 or NaN), t_k = p_k - i_k; a = the axis of the largest
 * t_k (ties: the lowest axis), t = t_a; g(p) = (1 - t) g(i) + t g(i + e_a), or g(i) when t is 0 (a lattice point).  The
 * normal is -g / ||g||: toward decreasing density, out of the body; the zero vector where ||g|| is 0 or g is not finite.
 * fp32 throughout.  Shape rules of mf_mc_count; V == 0: MF_OK, nothing launched. */
int32_t mf_mc_normals(const float* vol, int64_t n0, int64_t n1, int64_t n2, int32_t clamp_zero, const float* verts, int64_t V,
                      float* normals, void* stream);

/* ---- mesh clean-up: connected components of an indexed triangle mesh, the table of the components, and the compaction of
 * the mesh to the components a caller keeps -- what a user of visualize_mesh's output (trainer_moco_flow.py:485-548) does
 * next, a fixed-threshold sigma isosurface being a body plus detached specks -- without the mesh leaving the device
 * (tests/mesh_components_oracle.py restates the contract in numpy).
 * tris: (T, 3) int64 over V vertices.  Two vertices are adjacent if some triangle names both; a triangle may name an index
 * twice or three times and may be repeated.  The label of a vertex is the smallest vertex index of its connected
 * component (a vertex in no triangle is its own component); a triangle belongs to the component of its column-0 vertex.
 * Every output is a pure function of the input: bit-identical from run to run, whatever the launch geometry and the order
 * in which atomics land.  32-bit internal indexing: V or T outside [0, 2^31) is MF_E_INVALID.  A triangle with an index
 * outside [0, V) is never dereferenced: it joins nothing, belongs to nothing and is counted into the entry's `bad`
 * counter -- the caller reads that counter with the counts it reads anyway and rejects the mesh.  Scratch is the caller's
 * (the *_scratch_bytes queries; MF_E_INVALID on a bad shape); nothing is allocated, everything runs on `stream`, nothing
 * synchronises.  V = 0 or T = 0 launches nothing that reads the missing array (which may be NULL).
 *
 * mf_mesh_label: labels (V) int64; bad (device int64[1]) = triangles with an index out of range.  Lock-free union-find on
 * 32-bit parents in scratch (4 V bytes): parent[v] = v; one grid-stride pass over the triangles unites (t0, t1) and (t1, t2)
 * -- find both roots (path splitting), hook the larger under the smaller with one compare-and-swap, and on a failed swap go
 * on from the value it returned (another thread has hooked that root, under a smaller index); one pass writes the roots.
 * A parent is never larger than its vertex, so the final root is the component's minimum whoever won which swap; no wave
 * ever waits for another (no flags, no grid barrier, no cooperative launch).  Three launches. */
int64_t mf_mesh_label_scratch_bytes(int64_t V, int64_t T);
int32_t mf_mesh_label(const int64_t* tris, int64_t T, int64_t V, int64_t* labels, int64_t* bad, void* scratch, void* stream);
/* The component table, in two steps around the caller's read of the component count.
 * mf_mesh_table_count: per label the number of triangles and of vertices (integer atomic adds, first summed over the lanes
 * of a wave that hit the same label and, for the label most of a wave shares, over the wave's whole share of the mesh: one
 * big component does not send every add to one address) and the root flags labels[v] == v, all kept in scratch; counts
 * (device int64[2]) =
 * [C = number of components, bad = triangles whose column-0 index, and vertices whose label, is outside [0, V)].
 * mf_mesh_table_emit, with the same V and scratch and the C read from counts: ids (C) = the labels in ascending order
 * (mf_mask_compact on the root flags), tri_counts (C), vert_counts (C), all int64.  C == 0: nothing launched. */
int64_t mf_mesh_table_scratch_bytes(int64_t V, int64_t T);
int32_t mf_mesh_table_count(const int64_t* tris, int64_t T, int64_t V, const int64_t* labels, int64_t* counts, void* scratch,
                            void* stream);
int32_t mf_mesh_table_emit(int64_t V, int64_t C, void* scratch, int64_t* ids, int64_t* tri_counts, int64_t* vert_counts,
                           void* stream);
/* The filter, in two steps around the caller's read of the kept counts.
 * mf_mesh_filter_plan: ids (C) and keep (C, uint8) are the table's labels and the caller's decision per component.  Flags
 * per vertex (its label's component is kept) and per triangle (its column-0 vertex is kept) go to scratch; counts (device
 * int64[3]) = [kept vertices, kept triangles, bad = triangles with an index, vertices with a label and ids entries
 * outside [0, V)]; a bad triangle is dropped.
 * mf_mesh_filter_emit, with the same tris / T / V / scratch and the two counts read: vert_inds (Vk) and tri_inds (Tk) = the
 * kept vertices and triangles by their old indices, ascending (stable: mf_mask_compact on the flags); tris_out (Tk, 3) = the
 * kept triangles with their indices rewritten through the old -> new vertex map (-1 for an index out of range, which the
 * bad counter has reported).  A pointer whose count is 0 may be NULL. */
int64_t mf_mesh_filter_scratch_bytes(int64_t V, int64_t T);
int32_t mf_mesh_filter_plan(const int64_t* tris, int64_t T, int64_t V, const int64_t* labels, const int64_t* ids,
                            const uint8_t* keep, int64_t C, int64_t* counts, void* scratch, void* stream);
int32_t mf_mesh_filter_emit(const int64_t* tris, int64_t T, int64_t V, int64_t Vk, int64_t Tk, void* scratch,
                            int64_t* vert_inds, int64_t* tri_inds, int64_t* tris_out, void* stream);
/* dst row k = src row inds[k] for k < n: rows of row_bytes contiguous bytes, copied as they are (vertices and any
 * per-vertex attribute of a filtered mesh stay bitwise equal); src has n_src rows, an index outside [0, n_src) gives a row
 * of zero bytes.  4-byte words where row_bytes and both pointers allow it, bytes otherwise.  n row_bytes == 0: nothing
 * launched. */
int32_t mf_gather_rows(const void* src, int64_t n_src, int64_t row_bytes, const int64_t* inds, int64_t n, void* dst,
                       void* stream);

/* ---- mesh simplification by vertex clustering: the triangle count of an isosurface (1.8 M triangles on a smooth field at
 * 512^3) brought down on the device, in one pass and as a pure function of the input (tests/mesh_simplify_oracle.py restates
 * the contract in numpy).  The reference has no counterpart: it writes the full mesh (trainer_moco_flow.py:535-548).
 * verts (V, 3) fp32, tris (T, 3) int64; lo, hi: HOST double[3]; cell > 0: the edge of a cubic cell in the vertices' units;
 * n_a = floor((hi_a - lo_a) / cell) + 1 cells per axis, computed by the caller in double and checked here; n0 n1 n2, V, T
 * below 2^31 (32-bit internal indexing), anything else MF_E_INVALID -- from mf_simplify_mesh_scratch_bytes already, before
 * anything is allocated.
 * Cell of a vertex, per axis in double: t = (double(v) - lo) / cell, c = floor(t), id = (c0 n1 + c1) n2 + c2.  A vertex that is
 * not finite or lies outside [lo, hi] on an axis, and a triangle with an index outside [0, V), are counted into `bad`: nothing
 * is clamped, a bad index is never dereferenced, the caller rejects the mesh.
 * A triangle is degenerate, and dropped, if two of its three cells are equal.  Two others are duplicates if their cell triples
 * are equal up to cyclic rotation (the opposite winding is another triangle); of a class the smallest triangle index
 * survives.  Survivors keep their order and their corner order.  A cell is used if a survivor names it; the new vertices
 * are the used cells, ascending by id; first[k] = the smallest vertex index in used cell k; cluster[v] = the new index of
 * v's cell, -1 for a vertex of an unused cell.
 * Duplicates are found in an open-addressing table of `slots` int32 entries -- a power of two above T, at most 2^31: an empty
 * slot always remains, every probe ends, and the probe loop is bounded by `slots` besides.  A slot holds a triangle index;
 * its key is recomputed from that triangle's cells.  Insert: linear probing from the hash of the rotation-canonical triple;
 * compare-and-swap into an empty slot, atomicMin into a slot of the same key, on to the next otherwise.  A taken slot never
 * changes its key class, so each class settles in one slot whatever the interleaving, and the slot ends as the class's minimum.
 * Every rank is mf_scan.hpp's (fixed order); sums, minima and counts over a cell's members are integer atomics: every output
 * is bit-identical from run to run.  Scratch is the caller's; nothing is allocated, everything runs on `stream`, nothing
 * synchronises.  V = 0 or T = 0 is legal (the missing array may be NULL).
 *
 * mf_simplify_mesh_plan: cell ids, the table, the survivor flags, the used-cell bit mask and its word prefixes go to scratch;
 * counts (device int64[3]) = [Vk = used cells, Tk = survivors, bad].  Up to six launches.
 * mf_simplify_mesh_emit, with the same mesh, grid and scratch and the two counts read: tris_k (Tk, 3) = the survivors, corners
 * rewritten to the new indices; first (Vk); cluster (V).  verts_k (Vk, 3) with sums (28 Vk bytes of the caller's, 8-byte
 * aligned) = the exact mean of each used cell's members in fixed point: per axis q = llrint((t - c) 2^20), S = the int64 sum of
 * q over the n members, verts_k = float(lo + cell (c + (double(S) / double(n)) / 2^20)), every operation rounded once in
 * double; both NULL: positions are the caller's (rows first[k] of verts through mf_gather_rows keep a vertex on its lattice
 * edge).  Tk == 0: cluster is filled with -1, nothing else is touched.  Up to three launches. */
int64_t mf_simplify_mesh_scratch_bytes(int64_t V, int64_t T, int64_t n0, int64_t n1, int64_t n2, int64_t slots);
int32_t mf_simplify_mesh_plan(const float* verts, int64_t V, const int64_t* tris, int64_t T, const double* lo, const double* hi,
                              double cell, int64_t n0, int64_t n1, int64_t n2, int64_t slots, int64_t* counts, void* scratch,
                              void* stream);
int32_t mf_simplify_mesh_emit(const float* verts, int64_t V, const int64_t* tris, int64_t T, const double* lo, const double* hi,
                              double cell, int64_t n0, int64_t n1, int64_t n2, int64_t Vk, int64_t Tk, void* scratch, void* sums,
                              float* verts_k, int64_t* tris_k, int64_t* first, int64_t* cluster, void* stream);

/* ---- vertex adjacency and smoothing: what follows an isosurface at a fixed threshold, whose lattice-scale ripple (and the
 * faceting a clustering grid leaves) a user otherwise removes on the host after copying the mesh there.  The reference has no
 * counterpart; tests/mesh_smooth_oracle.py restates both contracts in numpy.  Nothing is allocated, everything runs on `stream`,
 * nothing synchronises; every output is a pure function of the input, bit-identical from run to run. */
#define MF_MESH_MAX_TRIANGLES_PER_VERTEX 2048

/* mf_rings_mesh_plan (serves trainer_moco_flow.py:490-538, trainer_nerf.py:200-259: the mesh visualize_mesh extracts): the
 * one-ring of every vertex of tris (T, 3) int64 over V vertices.  A triangle that names a vertex outside [0, V) is counted into
 * `bad` and never dereferenced.  A triangle with two equal indices is skipped entirely and contributes no edge.  m(i, j) = the
 * number of remaining triangles that contain both i and j, i != j.  ring(i) = { j : m(i, j) >= 1 }, ascending by j, each j once
 * (the same triangle twice, or in both windings, changes m and not the ring).  boundary[i] = 1 iff some j has m(i, j) == 1: an
 * edge in three or more triangles does not make its ends boundary; a vertex in no kept triangle has an empty ring and is not
 * boundary.  V < 2^31 and 6 T < 2^31 (R <= 6 T), else MF_E_INVALID -- from mf_rings_mesh_scratch_bytes already, a host function,
 * before anything is allocated.  A vertex in more than MF_MESH_MAX_TRIANGLES_PER_VERTEX kept triangles is counted into
 * `over_cap` by the counting pass; with bad or over_cap non-zero no segment is sorted (no lane does work quadratic in an unbounded
 * degree), offsets and boundary hold nothing of use and the caller rejects the mesh.
 * Writes counts (device int64[3]) = [bad, over_cap, R], offsets (V + 1) int64 (offsets[V] = R) and boundary (V) uint8; the
 * sorted, de-duplicated segments stay in scratch.  Raw half-edges are counted and placed by integer atomics, each segment is
 * sorted before anything is read from it: the order in which the atomics land shows in no output.  V = 0 or T = 0 is legal
 * (offsets all zero; tris, boundary and scratch may be NULL where empty).  Up to ten launches. */
int64_t mf_rings_mesh_scratch_bytes(int64_t V, int64_t T);
int32_t mf_rings_mesh_plan(const int64_t* tris, int64_t T, int64_t V, int64_t* counts, int64_t* offsets, uint8_t* boundary,
                           void* scratch, void* stream);
/* mf_rings_mesh_emit (serves trainer_moco_flow.py:490-538, trainer_nerf.py:200-259): after mf_rings_mesh_plan on the same
 * stream with the same V, T, scratch and offsets, and with counts read (bad = over_cap = 0): ring (R) int64,
 * ring[offsets[i] .. offsets[i + 1]) = ring(i).  Nothing is written at or beyond R.  R = 0 launches nothing.  Two launches. */
int32_t mf_rings_mesh_emit(int64_t V, int64_t T, int64_t R, void* scratch, const int64_t* offsets, int64_t* ring, void* stream);

/* mf_smooth_mesh (serves trainer_moco_flow.py:490-538, trainer_nerf.py:200-259): Laplacian (taubin = 0: `iterations` steps with
 * factor lam) or Taubin lambda|mu smoothing (taubin = 1: `iterations` times a lam step, then a mu step) of verts (V, 3) fp32
 * over the rings mf_rings_mesh_* wrote (offsets (V + 1), ring (R), both int64) -> out (V, 3) fp32; out must not alias verts.
 * One step with factor f: every vertex reads the positions of the PREVIOUS step (Jacobi, two buffers).  A vertex that moves, with
 * ring j0 < j1 < ... < j(n-1), per component in fp32, every operation rounded once: s = p[j0]; s = s + p[jk] for k = 1 .. n-1 in
 * that order; m = s / float(n); d = m - p_i; p_i' = p_i + f d (the product rounded, then the sum).  A vertex that does not move
 * -- an empty ring, or boundary[i] != 0 where boundary is given (NULL: boundary vertices move like any other) -- is copied byte
 * for byte.  Positions that are not finite propagate by IEEE rules: nothing is checked, nothing is clamped.
 * The steps run on private copies in scratch (mf_smooth_mesh_scratch_bytes(V, R); V, R in [0, 2^31), else MF_E_INVALID):
 * positions as 16-byte rows, offsets and ring as int32.  While copying, offsets are clamped to [0, R] and a ring entry outside
 * [0, V) becomes 0, so rings that are not mf_rings_mesh_*'s give positions without meaning but no access outside the buffers.
 * iterations in [0, 2^20], lam (and mu with taubin) finite, else MF_E_INVALID.  iterations = 0 or R = 0: out = verts, a copy.
 * V = 0 launches nothing.  One call enqueues the packing, every step and the unpacking: 2 + the number of steps launches. */
int64_t mf_smooth_mesh_scratch_bytes(int64_t V, int64_t R);
int32_t mf_smooth_mesh(const float* verts, int64_t V, const int64_t* offsets, const int64_t* ring, int64_t R,
                       const uint8_t* boundary, int32_t iterations, float lam, float mu, int32_t taubin, float* out, void* scratch,
                       void* stream);

/* ---- validation metrics: models/metrics.py:4-22 (mse, psnr, ssim), called per validation image by val_step
 * (trainer_moco_flow.py:453-473).  The reference's ssim is kornia 0.6.5's kornia.metrics.ssim.ssim(img1, img2, window_size,
 * max_val=1.0, eps=1e-12); kornia is not available to this project: KORNIA RESTATED from the published algorithm (as
 * oracle/kornia_restated.py does for the quaternion functions), unpinned against kornia itself.
 *
 * mf_ssim: a, b = fp32 (B, C, H, W) images, each addressed through four ELEMENT strides (host int64[4]: B, C, H, W), so a
 * contiguous CHW tensor and the view rows.view(H, W, 3).permute(2, 0, 1)[None] of rendered (H W, 3) rows both work uncopied.
 * Window g[i] = exp(-(i - ws/2)^2 / (2 1.5^2)) normalised to sum 1 (float64 on the host), 2-D window g x g,
 * window_size odd in 3..11; border = reflect padding without repeating the edge by ws/2 (F.pad(mode='reflect'): needs
 * ws/2 < min(H, W), else MF_E_INVALID).  Per pixel, f = the windowed sum: mu1 = f(a), mu2 = f(b), s1 = f(a^2) - mu1^2,
 * s2 = f(b^2) - mu2^2, s12 = f(ab) - mu1 mu2, C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2,
 *   ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + eps)
 * (the moments are accumulated in float64 and the map is rounded to fp32 once: the formula's own fp32 evaluation is
 * 2e-4 .. 9e-4 off in flat regions through the cancellation in s1, s2).
 * map_out: (B, C, H, W) contiguous fp32 or NULL; sums: device double[2] = [sum of ssim, sum of (a - b)^2] over all B C H W
 * elements, reduced in a fixed order through scratch (mf_ssim_scratch_bytes bytes): bit-identical from run to run.
 * B C H W = 0 launches nothing and writes zeros to sums.  One kernel launch plus the finishing workgroup. */
int64_t mf_ssim_scratch_bytes(int64_t B, int64_t C, int64_t H, int64_t W);
int32_t mf_ssim(const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int64_t B, int64_t C,
                int64_t H, int64_t W, int32_t window_size, float max_val, float eps, float* map_out, double* sums,
                void* scratch, void* stream);
/* mf_sqerr: the reduction behind mse / psnr (metrics.py:4-13).  a, b: n contiguous fp32 elements; mask: one uint8 per row of
 * row_len elements (row_len = 1: elementwise; 3: the per-ray mask value[valid_mask] applies to (N, 3); row_len divides n), or
 * NULL = all.  out2: device double[2] = [sum of (a - b)^2 over the selected elements, their count]; same fixed-order
 * reduction through scratch (mf_sqerr_scratch_bytes(n) bytes).  n = 0 writes zeros. */
int64_t mf_sqerr_scratch_bytes(int64_t n);
int32_t mf_sqerr(const float* a, const float* b, int64_t n, const uint8_t* mask, int64_t row_len, double* out2,
                 void* scratch, void* stream);

/* ---- pictures: utils/vis_utils.py:28-43 (visualize_depth), reached through decode_results (trainer_moco_flow.py:475-482) by
 * val_step, visualize_frame, visualize_video and visualize_spherical_poses; and the sheet those assemble with torch.cat and
 * hand to torchvision's save_image (trainer_moco_flow.py:609-623, 644-659).  The reference copies the depth plane to the
 * host, normalises it with numpy, colours it with cv2.applyColorMap and copies it back; here everything stays on the device
 * and nothing synchronises.
 * The index arithmetic is vis_utils.py:34-40 in its own fp32, one rounding per operation:
 *   v = nan_to_num(d)   (NaN -> nan_value, +inf -> FLT_MAX, -inf -> -FLT_MAX: numpy's defaults)
 *   den = (ma - mi) + 1e-8     x = (v - mi) / den     i = (uint8) trunc(255 x)
 * ONE DEVIATION: where astype(np.uint8) is undefined -- 255 x outside [0, 256) or NaN, which takes a caller-given range
 * narrower than the data, or infinities in the data -- i is clamped to 0 .. 255 (NaN: 0).
 * lut: 768 device bytes, (256, 3); entry i colours index i, column c becomes channel c of the result.  The package's Jet
 * table (moco_flow_amd/vis.py: colormap_lut) is OPENCV RESTATED: cv2 is not available to this project, the table restates
 * OpenCV's COLORMAP_JET from its closed form (with applyColorMap's BGR order read as RGB, as the reference does) and is
 * UNPINNED AGAINST cv2 ITSELF; a caller who has cv2 passes its table.
 *
 * mf_depth_range: out2 = device fp32 [min, max] of nan_to_num(depth) over n contiguous fp32 elements, exact (min and max do
 * not depend on the order); per-workgroup partials in scratch (mf_depth_range_scratch_bytes(n) bytes), one launch plus the
 * finishing workgroup.  n = 0 writes [0, 0] and launches nothing else. */
int64_t mf_depth_range_scratch_bytes(int64_t n);
int32_t mf_depth_range(const float* depth, int64_t n, float nan_value, float* out2, void* scratch, void* stream);
/* mf_depth_colormap (vis_utils.py:39-43): range2 = device fp32 [mi, ma], written by mf_depth_range or by the caller;
 * out_planar[c n + p] = lut[3 i(p) + c] / 255.0f (fp32 division) for c = 0, 1, 2: the (3, H, W) tensor ToTensor returns. */
int32_t mf_depth_colormap(const float* depth, int64_t n, const float* range2, float nan_value, const uint8_t* lut,
                          float* out_planar, void* stream);
/* mf_frame_sheet: up to 8 panels of H x W pixels side by side along the width, one launch (the torch.cat(..., dim=-1) of
 * trainer_moco_flow.py:614-621, 650-655 and save_image's quantisation).
 *   kind 0  rgb rows (H W, 3) as render_rays / render_image return them, or the ground-truth rgbs: pixel p, channel c at
 *           rows[3 p + c]
 *   kind 1  a depth plane (H W), colour-mapped as mf_depth_colormap does with the range range2s[2 k], range2s[2 k + 1] of
 *           panel k and the panel's nan_value
 * out_u8: (H, n_panels W, 3) bytes, u = (uint8) clamp(v 255 + 0.5, 0, 255) in fp32 as torchvision.utils.save_image
 * quantises (NaN: 0); a colour-mapped pixel is its LUT byte.  out_planar: the float (3, H, n_panels W) stack (rgb values
 * as they are, colour-mapped ones lut / 255).  Either output may be NULL, not both.  range2s and lut may be NULL without a
 * depth panel.  32-bit indexing: H W n_panels 3 must be below 2^31, else MF_E_INVALID.  H W = 0 launches nothing. */
typedef struct mf_sheet_panel {
  const float* rows;
  int32_t kind;
  float nan_value;
} mf_sheet_panel;
int32_t mf_frame_sheet(const mf_sheet_panel* panels /* host */, int32_t n_panels, int64_t H, int64_t W, const float* range2s,
                       const uint8_t* lut, uint8_t* out_u8, float* out_planar, void* stream);

/* ---- the ray batch of a training step (trainer/trainer_moco_flow.py:407-417, the same lines of trainer/trainer_nerf.py; fed by
 * datasets/moco_flow_dataset.py:166-176, 190-196; the chain_global column of _shared_step, trainer_moco_flow.py:308-312).
 * The reference keeps per frame the (H W, 9) ray table, the composited (H W, 3) image and the (H W, 3) background, and draws
 * a batch with torch.nonzero, torch.randperm and three gathers.  The batch is a pure function of the camera, the hull mask,
 * the image and a permutation: these two entries build it from those, and none of the tables exists.
 *
 * mf_mask_compact (trainer_moco_flow.py:414: val_inds = torch.nonzero(rays_msk).squeeze(1)): inds_out[0 .. count) = the
 * positions of the non-zero bytes of mask (n bytes), ascending; count (device int64[1]) = how many.  inds_out has room for n
 * entries; entries from count on are not written.  mask == NULL: the identity, count = n (scratch may be NULL).  Per-workgroup
 * counts into scratch (mf_mask_compact_scratch_bytes(n) bytes), then every workgroup sums the counts in front of it and
 * scatters its share with wavefront ballots: no atomics, pixel order, bit-identical from run to run.  Two launches (one for the
 * identity), no host read; n = 0 only zeroes count. */
int64_t mf_mask_compact_scratch_bytes(int64_t n);
int32_t mf_mask_compact(const uint8_t* mask, int64_t n, int64_t* inds_out, int64_t* count, void* scratch, void* stream);

/* mf_ray_batch (trainer_moco_flow.py:415-416 with datasets/moco_flow_dataset.py:169-176, 196 and _shared_step :308-312): one
 * launch, one thread per row k < n_rows.  pixel = val_inds[perm[k]] (both device int64; the reference's
 * val_inds[torch.randperm(n_valid)[:N_rand]]), written to sel_out[k] when sel_out is given.
 *   rays_out (n_rows, 9), or (n_rows, 10) with has_chain: columns 0-8 are row `pixel` of mf_make_rays for the same H, W, focal,
 *       cx, cy, c2w, nearv, farv, idx, bit for bit (the same per-pixel device function); column 9 = chain_idx.  c2w travels BY
 *       VALUE (3x4 row-major, read when has_c2w).  Rows are stored in float4 pieces where rays_out is 16-byte aligned.
 *   rgbs_out (n_rows, 3), by image_kind:
 *       MF_IMAGE_NONE    nothing is written (rgbs_out may be NULL)
 *       MF_IMAGE_ROWS    image = fp32 (H W, 3): the row is gathered
 *       MF_IMAGE_U8_RGB  image = bytes (H, W, 3): v = u8 * (1.0f / 255.0f), which is what u8.float().div(255) (torchvision's
 *                        ToTensor) gives ON THE DEVICE, where torch multiplies by the fp32 reciprocal of a host scalar.  For
 *                        126 of the 256 byte values that is one ulp from the fp32 quotient the host computes.
 *       MF_IMAGE_U8_RGBA image = bytes (H, W, 4), 4-byte aligned: v_c a + bg_c (1 - a) with a = alpha * (1.0f / 255.0f) and bg the
 *                        pixel's background (moco_flow_dataset.py:174); the reciprocal, every product, difference and sum
 *                        rounded once, no fused multiply-add: bit-identical to the torch expression evaluated on the device.
 *                        Needs a background.
 *   background_out (n_rows, 3), optional, by background_kind:
 *       MF_BACKGROUND_NONE    none      MF_BACKGROUND_ROWS  background = fp32 (H W, 3): the row is gathered
 *       MF_BACKGROUND_COLOUR  background = 3 device floats, one colour for every pixel (bkgd_img, moco_flow_dataset.py:176)
 * perm[k] outside [0, n_valid), or a val_inds entry outside [0, H W), is NOT dereferenced: the row's outputs are NaN and
 * sel_out[k] = -1 (the caller cannot check a device permutation without a synchronisation).
 * 32-bit pixel indexing: H W and n_rows below 2^31, else MF_E_INVALID.  n_rows = 0 launches nothing. */
enum { MF_IMAGE_NONE = 0, MF_IMAGE_ROWS = 1, MF_IMAGE_U8_RGB = 2, MF_IMAGE_U8_RGBA = 3 };
enum { MF_BACKGROUND_NONE = 0, MF_BACKGROUND_ROWS = 1, MF_BACKGROUND_COLOUR = 2 };
typedef struct mf_ray_batch_args {
  int32_t H, W;
  float focal, cx, cy;             /* as mf_make_rays */
  int32_t has_c2w; float c2w[12];
  float nearv, farv, idx;
  int32_t has_chain; float chain_idx;
  const int64_t* val_inds; int64_t n_valid;     /* mf_mask_compact's output */
  const int64_t* perm; int64_t n_rows;          /* n_rows entries are read */
  const void* image; int32_t image_kind;
  const float* background; int32_t background_kind;
  float* rays_out; float* rgbs_out; float* background_out; int64_t* sel_out;
} mf_ray_batch_args;
int32_t mf_ray_batch(const mf_ray_batch_args* a /* host */, void* stream);

/* ---- SMPL point supervision of a training step (datasets/moco_flow_dataset.py:101-132; trainer/trainer_moco_flow.py:146-157,
 * 330-363; trainer/trainer_nof.py:115-125; csrc/mf_supervise.hip).  The reference compacts the query points into an inside and
 * an outside set (two host reads of data-dependent lengths) and takes three losses of them.  Here every tensor keeps all Q rows
 * in the queries' order, the split is the byte mask `inside`, and the losses are (sum, count) pairs: no compaction, no host read.
 *
 * mf_point_correspond: one launch.  Q = q_given + q_near queries: rows [0, q_given) are `query` (q_given, 3) as given; row
 * q_given + j is verts[pick[j]] + noise[j] * thickness (pick: q_near int64 in [0, V), clamped; noise (q_near, 3), a randn
 * draw), the product and the sum rounded once each -- near_surface_pts of moco_flow_dataset.py:110-111 without its gather.
 * verts (V, 3): the source-pose vertices; trans (V, 4, 4): mf_smpl_frame_transforms' output.
 *   pairs (Q, 6)  = [query | trans[ind] @ (query, 1)], mf_apply_vertex_transforms' expression
 *   inside (Q)    = dist < thickness ? 1 : 0 (strict, :123)
 *   dist (Q), ind (Q): the nearest vertex's distance and index; each may be NULL
 * The search is mf_knn1's arithmetic per candidate (fma(az, az, fma(ay, ay, ax ax)) on ref - query, sqrtf of the minimum) and
 * its tie rule (the lowest index among equal minima): dist, ind and pairs are bit-identical to mf_knn1 followed by
 * mf_apply_vertex_transforms.  lanes_per_query lanes of a wave share a query -- each takes the vertices v = lane (mod
 * lanes_per_query) of every tile, then the lanes take the lexicographic minimum of (d, index) -- so that a few thousand queries
 * still fill the chip; the result does not depend on it.  0 = chosen from Q (the fewest lanes that give every SIMD two waves);
 * anything but 0, 1, 4, 16, 64 is MF_E_INVALID, as are V < 1, V or Q >= 2^31 - 1, a negative count and a NULL that is needed.
 * Q = 0 launches nothing. */
int32_t mf_point_correspond(const float* verts, const float* trans, int64_t V, const float* query, int64_t q_given,
                            const int64_t* pick, const float* noise, int64_t q_near, float thickness, int32_t lanes_per_query,
                            float* pairs, uint8_t* inside, float* dist, int64_t* ind, void* stream);

/* mf_point_loss_partials: out6 (device, 6 doubles) = [sum, count] of
 *   nof_bw       sum |pred_bw - pairs[:, 3:6]| over the rows with inside = 1; count = 3 x those rows   (nn.L1Loss, :337-338)
 *   nof_fw       sum |pred_fw - pairs[:, 0:3]| over the same rows                                        (:340-341)
 *   alphas_mask  sum over the rows with inside = 0 and the n_nerfs (<= 2) NeRFs of -max(logf(1 - alpha), -100), alpha = 1 -
 *                expf(-delta softplus(sigma)), softplus(s) = s > 20 ? s : log1pf(expf(s)): nn.BCELoss against zeros of
 *                forwarf_nerf's alphas (:146-157, :348-363), every operation rounded where torch rounds it; count = outside
 *                rows x n_nerfs, the length of the reference's torch.cat (:359)
 * each |.| taken in fp32 and summed in float64.  inside == NULL or use_all != 0: the L1 terms take every row (stage 2,
 * trainer_nof.py:115-125); inside == NULL leaves no outside row.  pred_bw / pred_fw NULL: that term is (0, 0).
 * means3 (device, 3 floats, optional): sum / count in fp32, 0 where the count is 0 (the reference would give NaN).
 * Deterministic: per-workgroup partials in scratch (mf_point_loss_partials_scratch_bytes(Q) bytes), summed in a fixed order by
 * a second launch; no atomics.  Q = 0 writes zeros. */
typedef struct mf_point_loss_args {
  int64_t Q;
  const float* pairs;             /* (Q, 6) */
  const uint8_t* inside;          /* (Q) or NULL */
  int32_t use_all;
  const float* pred_bw;           /* (Q, 3) or NULL */
  const float* pred_fw;           /* (Q, 3) or NULL */
  int32_t n_nerfs;                /* 0 .. 2 */
  const float* sigma[2];          /* (Q) raw densities of each NeRF */
  float delta[2];
} mf_point_loss_args;
int64_t mf_point_loss_partials_scratch_bytes(int64_t Q);
int32_t mf_point_loss_partials(const mf_point_loss_args* a /* host */, double* out6, float* means3, void* scratch, void* stream);

/* Backward of the three means: seeds3 (device, 3 floats) = dL / d (sum / count) of each term, out6 the forward's partials (the
 * counts are read on the device).  Written whole, exact zeros on rows the mask drops and everywhere in a term whose count is 0:
 *   g_pred_bw, g_pred_fw (Q, 3) = seed / count * sign(pred - target), sign(0) = 0                      (nn.L1Loss)
 *   g_sigma0, g_sigma1 (Q)      = seed * alpha / max((1 - alpha) alpha, 1e-12) / count                  (nn.BCELoss)
 *                                 * expf(-delta softplus(sigma)) * delta, then (sigma > 20 ? a : a z / (z + 1)), z = expf(sigma)
 * Every product and quotient is rounded in the order of torch's device kernels for the same chain (binary_cross_entropy_backward,
 * exp, mul, softplus_backward, mean), `/ count` being their multiplication by the rounded reciprocal 1.f / count: the seeds are
 * bit-identical to the ones autograd hands the compacted rows.
 * Each output may be NULL.  One launch. */
int32_t mf_point_loss_partials_backward(const mf_point_loss_args* a /* host */, const double* out6, const float* seeds3,
                                        float* g_pred_bw, float* g_pred_fw, float* g_sigma0, float* g_sigma1, void* stream);

/* ---- occupancy grid: cull and clip test-time rays before the render pass.  The reference renders every ray of the projected
 * AABB's hull (MoCoFlowTrainer.render, trainer_moco_flow.py:226-268) from the nearest to the farthest AABB corner
 * (Camera.make_rays, utils/camera.py:134-148; the coarse z_vals of models/rendering.py:239-249 span that whole interval). ----
 *
 * mf_occ_build (serves trainer_moco_flow.py:226-268, utils/camera.py:134-148, rendering.py:239-249): sigma (nx, ny, nz) fp32,
 * z fastest, raw densities of the lattice as mf_points_sigma returns them -> a grid of (nx-1, ny-1, nz-1) cells, one bit per
 * cell, packed along z: row (i, j) holds ceil((nz-1) / 32) uint32 words, cell k is bit k % 32 of word k / 32, the unused bits
 * of a row's last word are 0.  Cell (i, j, k) is set iff some lattice point of [i-r, i+1+r] x [j-r, j+1+r] x [k-r, k+1+r]
 * (clipped to the lattice, r = dilate in {0, 1, 2}) has act(sigma) > tau -- strictly; a NaN counts as set.  act = MF_ACT_RELU
 * (sigma < 0 ? 0 : sigma) or MF_ACT_SOFTPLUS (sigma > 20 ? sigma : log1pf(expf(sigma))), as the render pass and
 * mf_point_loss_partials evaluate them.  count_out (device int64[1], optional): the number of set cells, through the fixed-order
 * reduction (scratch: mf_occ_build_scratch_bytes bytes, needed only with count_out).  Every word is written by one lane with a
 * plain store; no atomics; bit-identical from run to run.  Each side >= 2 and fewer than 2^31 cells, else MF_E_INVALID. */
int64_t mf_occ_build_scratch_bytes(int64_t nx, int64_t ny, int64_t nz);
int32_t mf_occ_build(const float* sigma, int64_t nx, int64_t ny, int64_t nz, int32_t activation, float tau, int32_t dilate,
                     uint32_t* bits_out, int64_t* count_out, void* scratch, void* stream);

/* mf_ray_clip (serves trainer_moco_flow.py:226-268, utils/camera.py:134-148, rendering.py:239-249): rays (n_rays, >= 8) fp32 with
 * a row stride in floats ([o, d, near, far, ...]: the 9- and 10-column tables both work) marched through the bit grid of
 * (gx, gy, gz) cells over the box lo .. hi (host float[3] each; inv_cell: host float[3], cells per world unit, passed so that the
 * kernel and a restatement use the same constants) in steps of dt world units -> t_first, t_last (n_rays) fp32, hit (n_rays)
 * uint8.  Per ray, every fp32 operation rounded once (no fused multiply-add):
 *   1. o, d, near or far NaN / inf: hit = 1, t_first = near, t_last = far (nothing is hidden: the ray renders NaN as before)
 *   2. tmin = near, tmax = far; per axis with d_a != 0: t1 = (lo_a - o_a) / d_a, t2 = (hi_a - o_a) / d_a, tmin = max(tmin,
 *      min(t1, t2)), tmax = min(tmax, max(t1, t2)); with d_a == 0 the ray misses if o_a < lo_a or o_a > hi_a; tmin > tmax misses
 *   3. t_k = tmin + float(k) * dt for k = 0, 1, .. while t_k <= tmax: p = o + d * t_k, cell c_a = clamp(int(floor((p_a - lo_a) *
 *      inv_cell_a)), 0, g_a - 1), the cell's bit is tested
 *   4. kf / kl the first / last k with a set bit: hit = 1, t_first = max(near, t_kf - dt), t_last = min(far, t_kl + dt)
 *   5. otherwise hit = 0, t_first = near, t_last = far
 * The march takes at most n = floor(|hi - lo| / dt) + 2 steps (float64, on the host), which covers every ray with |d| >= 1; n >
 * 65536, dt <= 0 or a box with lo_a >= hi_a is MF_E_INVALID.  A ray still inside [tmin, tmax] after n steps (|d| < 1) is kept
 * whole from there: hit = 1, t_last = far, t_first from step 4 if a bit was set, else near.  One lane per ray; the grid is read
 * through the vector caches.  n_rays = 0 launches nothing. */
int32_t mf_ray_clip(const float* rays, int64_t ray_stride, int64_t n_rays, const uint32_t* bits, int32_t gx, int32_t gy,
                    int32_t gz, const float* lo /* host */, const float* hi /* host */, const float* inv_cell /* host */, float dt,
                    float* t_first, float* t_last, uint8_t* hit, void* stream);

/* ---- occupancy grids from a mesh (csrc/mf_voxelize.hip): the bit grid of mf_occ_build's layout -- (gx, gy, gz) cells over the
 * box lo .. hi, row (i, j) holding ceil(gz / 32) uint32 words, cell k bit k % 32 of word k / 32, the unused bits of a row's last
 * word 0 -- built from triangles instead of densities.  The reference labels a point "inside" iff it lies within `thickness` of a
 * vertex of the posed SMPL mesh (datasets/moco_flow_dataset.py:87-142), derives the frame's AABB from that mesh
 * (datasets/moco_flow_dataset.py:144-154) and renders every ray of that box's hull (trainer_moco_flow.py:226-268).  All three
 * entries decide in integers: their results are bit-identical from run to run and equal to tests/voxelize_oracle.py.
 * mf_voxel_dilate thickens a grid by a box of cells, a superset of the Euclidean shell; mf_grid_edt (csrc/mf_distance.hip, below
 * the three) thickens it by the shell itself and gives the grid's squared-distance field, in integers again
 * (tests/distance_oracle.py). ----
 *
 * mf_voxel_mesh (serves datasets/moco_flow_dataset.py:87-142, datasets/moco_flow_dataset.py:144-154,
 * trainer_moco_flow.py:226-268): verts (V, 3) fp32 and tris (T, 3) int64 on the device -> the cells the triangles' surfaces meet.
 * lo, hi, inv_cell: host float[3] each, exactly as mf_ray_clip takes them.  Per vertex coordinate, every fp32 operation rounded
 * once (no fused multiply-add): u = (p - lo_a) * inv_cell_a (mf_ray_clip's cell rule), q = rintf(u * 64) saturated to
 * [-2^16, 2^17] -- 64 sub-cell units per cell, 1024 cells below the box to 2048 cells above its origin.  Cell (i, j, k) is set iff
 * the closed snapped triangle meets the closed box [64 i, 64 i + 64] x [64 j, 64 j + 64] x [64 k, 64 k + 64], decided exactly in
 * int64 (edge differences < 2^18, normal components < 2^37, a plane test against a box corner < 2^57): a triangle lying in a cell
 * face sets the cells on both sides, a vertex on a cell corner all eight.  A triangle with an index outside [0, V), a NaN or inf
 * vertex, or a zero integer normal after snapping is skipped, and counted in dropped_out (device int64[1], optional).  A triangle
 * that reaches more than 1024 cells outside the box is distorted by the saturation.  The entry clears bits_out itself and then
 * sets bits with atomic ORs (order-independent).  T = 0 or V = 0: an all-zero grid, only the clear is launched (V = 0: dropped =
 * T).  Each side 1 .. 1024 and fewer than 2^31 cells, V and T in [0, 2^31), lo_a < hi_a, else MF_E_INVALID. */
int32_t mf_voxel_mesh(const float* verts, int64_t V, const int64_t* tris, int64_t T, int32_t gx, int32_t gy, int32_t gz,
                      const float* lo /* host */, const float* hi /* host */, const float* inv_cell /* host */, uint32_t* bits_out,
                      int64_t* dropped_out, void* stream);

/* mf_voxel_fill (serves datasets/moco_flow_dataset.py:87-142, datasets/moco_flow_dataset.py:144-154,
 * trainer_moco_flow.py:226-268): a cell of bits_out is set iff it is set in bits, or it is an empty cell that is NOT 6-connected
 * through empty cells to the outside of the grid (everything beyond the grid counts as empty and connected): a union-find over
 * the empty cells with one virtual root for the outside (csrc/mf_unionfind.hpp); the result does not depend on the order of the
 * unions.  An open mesh, or one cut by the box, leaks and fills nothing; a torus's hole stays empty; a closed shell inside a
 * closed shell is filled through.  scratch: mf_voxel_fill_scratch_bytes bytes (4 per cell).  bits_out may be bits.  Each side
 * >= 1 and fewer than 2^31 cells, else MF_E_INVALID. */
int64_t mf_voxel_fill_scratch_bytes(int64_t gx, int64_t gy, int64_t gz);
int32_t mf_voxel_fill(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, uint32_t* bits_out, void* scratch, void* stream);

/* mf_voxel_dilate (serves datasets/moco_flow_dataset.py:87-142, datasets/moco_flow_dataset.py:144-154,
 * trainer_moco_flow.py:226-268): cell (i, j, k) of bits_out is set iff some cell of [i - rx, i + rx] x [j - ry, j + ry] x
 * [k - rz, k + rz], clipped to the grid, is set in bits.  Radii >= 0 of any size.  Separable: z on words (any radius, across
 * word boundaries), then y, then x; every output word is written by one lane with a plain store, padding bits stay 0.  bits_out
 * must not be bits.  count_out (device int64[1], optional): the number of set cells, through the fixed-order reduction.
 * scratch: mf_voxel_dilate_scratch_bytes bytes, always needed.  Each side >= 1 and fewer than 2^31 cells, else MF_E_INVALID. */
int64_t mf_voxel_dilate_scratch_bytes(int64_t gx, int64_t gy, int64_t gz);
int32_t mf_voxel_dilate(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, int32_t rx, int32_t ry, int32_t rz,
                        uint32_t* bits_out, int64_t* count_out, void* scratch, void* stream);

/* mf_grid_edt (serves datasets/moco_flow_dataset.py:87-142, trainer_moco_flow.py:226-268; csrc/mf_distance.hip): the exact
 * weighted squared distance field of a bit grid, capped, and the Euclidean dilation it decides.  With w (host int32[3], each in
 * [1, 65536]) and 0 <= R < 2^30:
 *   d2(i, j, k) = min(R + 1, min over the set cells (a, b, c) of bits of w[0] (i-a)^2 + w[1] (j-b)^2 + w[2] (k-c)^2)      int32
 * (an empty grid: R + 1 everywhere).  d2_out (optional): (gx, gy, gz) int32, dense, z fastest.  bits_out (optional): cell
 * (i, j, k) is set iff d2 <= R, padding bits written 0; count_out (device int64[1], optional, needs bits_out): the number of set
 * cells, through the fixed-order reduction.  At least one of d2_out / bits_out; bits_out must not be bits; the padding bits of
 * bits are 0.  The caller turns world units into integers (OccupancyGrid.euclid_metric): with cmax the longest cell edge and t
 * the world radius, w_a = floor(65536 (cell_a / cmax)^2) and R = ceil(65536 (t / cmax)^2) -- the floor and the ceil keep the
 * result a superset of the real-valued ellipsoid; cubic cells give w = 65536 on every axis and the plain Euclidean test in cell
 * units.  Three separable passes, exact because a pass drops only terms that exceed R on their own (r_a = isqrt(R / w_a) cells
 * is the reach along axis a; windows are clipped to the grid, a reach beyond the side works): z by bit scans on the row's words,
 * across word boundaries, then y, then x; a term w_a d^2 with |d| <= r_a is <= R and partial minima are capped at R + 1, so
 * every intermediate fits an int32.  No atomics: every output word or int is written by one lane with a plain store;
 * bit-identical from run to run.  scratch: mf_grid_edt_scratch_bytes bytes (6 per cell + 8 per workgroup), always needed.
 * Nothing allocates or synchronises.  Each side 1 .. 1024, else MF_E_INVALID. */
int64_t mf_grid_edt_scratch_bytes(int64_t gx, int64_t gy, int64_t gz);
int32_t mf_grid_edt(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, const int32_t* w /* host */, int32_t R,
                    int32_t* d2_out, uint32_t* bits_out, int64_t* count_out, void* scratch, void* stream);

/* ---- mesh-to-mesh distances: closest points on a triangle mesh, area-weighted surface samples and their statistics
 * (csrc/mf_mesh_distance.hip).  The reference has no such measure: it validates a `thickness` around the SMPL surface
 * by eye (datasets/moco_flow_dataset.py:101-132) and reports no geometry metric.  THE CONTRACT IS FIXED ARITHMETIC: every fp32
 * operation is rounded once, in the order written, without FMA, and dot(x, y) = (x0 y0 + x1 y1) + x2 y2; max / min ignore a NaN
 * operand (fmaxf / fminf).  tests/mesh_distance_oracle.py restates every output in np.float32.  No float atomics; every result
 * is bit-identical from run to run and independent of every order and launch shape below.  Nothing allocates or synchronises.
 *
 * mf_surface_records: verts (V, 3) fp32, tris (T, 3) int64, order (T) int32 or NULL (identity): slot s holds triangle order[s].
 * With a, b, c the triangle's vertices, ab = b - a, ac = c - a, bc = c - b, n = ab x ac (each component x y - z w: two rounded
 * products, one difference):
 *   records (Tp, 16)   a, ab, ac, r_ab = 1 / dot(ab, ab), r_ac = 1 / dot(ac, ac), r_bc = 1 / dot(bc, bc), d00 = dot(ab, ab),
 *                      d01 = dot(ab, ac), d11 = dot(ac, ac), rden = 1 / (d00 d11 - d01 d01); Tp = T rounded up to 64
 *   edges (Tp, 12)     b (the vertex as read), bc, and the triangle's exact min / max box lo, hi
 *   slot_tri (Tp)      int32: the caller's index of the slot's triangle, -1 for a slot without one (these never win)
 *   tile_box (Tp / 64, 8)   per tile of 64 slots: min lo, max hi over its kept slots (+inf / -inf for none), their number, 0
 *   tri_slot (T) int32 the slot of triangle t or -1; area2 (T) = sqrtf(dot(n, n)); normal (T, 3) = n (1 / area2);
 *   dropped (T) uint8; dropped_count (device int64[1])
 * A triangle is DROPPED -- never a candidate, never sampled, area2 = normal = 0 -- when an index lies outside [0, V) (tested
 * before an address is formed), when dot(n, n) is zero or not finite, when one of the 16 record fields is not finite, or when
 * no slot holds it: an entry of order outside [0, T) leaves its slot empty, and of equal entries the lowest slot keeps the
 * triangle (an integer atomic minimum), so a bad order cannot fault.  Every slot is written.
 *
 * The tile walk of a MeshIndex search (mf_surface_closest, mf_surface_cast): one row (a query, a ray) per lane.  Lane l of wave w
 * takes row qorder[64 w + l] (int32 (Q) or NULL: identity; an entry outside [0, Q) is skipped, a repeated one leaves another row
 * unwritten -- the caller passes a permutation).  Wave w visits the tiles start[w], +1, -1, +2, ... (int32 (ceil(Q / 64)) or NULL:
 * 0; clamped into the tiles).  Evaluating every tile is the sweep.  Under the cull the wave leaves the walk when no lane wants
 * anything more, and takes ONE decision per tile (one ballot, wave-uniform): the tile is skipped when it holds no kept slot or no
 * lane wants it -- by the search's own test of the tile's box, below.  Any other tile is evaluated whole, its 64 slots in order on
 * every lane, a slot's rows read at wave-uniform addresses (scalar loads).
 * visited (ceil(Q / 64)) int32, optional: the tiles wave w evaluated.  Q = 0 launches nothing.
 *
 * mf_surface_closest: query (Q, 3).  The value of a kept triangle at q is max(m, lb(q, lo, hi)) (lb > m ? lb : m), m the least, in
 * the order ab, ac, bc, face under strict < (the first minimum wins, a NaN never does), of dot(q - P, q - P) over
 *   edge ab  P = a + ab t, t = min(max(dot(q - a, ab) r_ab, 0), 1);   edge ac  the same with ac, r_ac
 *   edge bc  P = b + bc t, t = min(max(dot(q - b, bc) r_bc, 0), 1)
 *   face     d20 = dot(q - a, ab), d21 = dot(q - a, ac), v = min(max((d11 d20 - d01 d21) rden, 0), 1),
 *            w = min(max((d00 d21 - d01 d20) rden, 0), 1 - v), P = (a + ab v) + ac w
 * and lb(q, lo, hi) = dot(g, g), g = max(max(lo - q, q - hi), 0) per axis.  Per query: the lexicographic minimum of (value,
 * caller's index) over the kept triangles -> d2 (Q), tri (Q) int32, point (Q, 3) = the winning candidate's P, region (Q) uint8
 * (0 ab, 1 ac, 2 bc, 3 face; optional).  No kept triangle, or no value below +inf and no kept triangle at +inf: d2 = +inf,
 * tri = -1, point = 0, region = 0.  The rows are the queries of the tile walk above (qorder, start, visited).  mode: 0 = the sweep,
 * 1 = the cull: a lane wants a tile iff its row is a query and lb(q, tile box) <= best (best: the lane's least value so far, +inf
 * before).  Every operation of lb is monotone under rounding, so lb of a containing box <= lb of the triangle's own box <= the
 * value, in fp32: the skip needs no slack and both modes give the same bits.
 *
 * mf_surface_weights: weights (T) int64 = 0 for a dropped triangle, else max(1, (int64) floorf(area2 (1048576.f / amax[0]))), capped
 * at 2^22; amax: device fp32[1], the largest area2.  The caller takes their running sum `cum` (integers: exact in any order).
 * mf_surface_sample: r (n) int64, masked to [0, 2^53); u (n, 2) fp32 in [0, 1).  total = cum[T - 1]; target = floor(r total / 2^53)
 * by the 128-bit product; tri = the first t with cum[t] > target; s = sqrtf(u0), b0 = 1 - s, b1 = s (1 - u1), b2 = s u1;
 * point = (a b0 + b b1) + c b2.  total = 0, or a triangle whose indices lie outside [0, V): tri = -1, point = 0.
 *
 * mf_surface_stats: d2 (n) and optionally tri_src, tri_dst (n) int32 with the normal tables (T_src, 3), (T_dst, 3).  A row with a
 * negative tri_src or tri_dst is LEFT OUT; a row whose d2 is not in [0, +inf) is skipped; over the rest, d = sqrtf(d2):
 *   out_f64 (device, 4)  = [sum d, sum d d, max d, sum |dot(n_src[tri_src], n_dst[tri_dst])|] (the last needs all four; |.| in fp32)
 *   out_i64 (device, 10) = [rows with d <= thresholds[k], k < 8 (host fp32, n_thresholds <= 8; 0 beyond), finite rows, rows left out]
 * Sums in float64 through the fixed-order reduction (csrc/mf_reduce.hpp): per-workgroup partials in scratch
 * (mf_surface_stats_scratch_bytes(n) bytes), gathered by one workgroup.  n = 0 writes zeros.
 *
 * Every count (V, T, Q, n) in [0, 2^31 - 1), a NULL that is needed, a mode outside 0 .. 1 and an output that is an input are
 * MF_E_INVALID with an mf_last_error text, settled before any launch. ---- */
int32_t mf_surface_records(const float* verts, int64_t V, const int64_t* tris, int64_t T, const int32_t* order, float* records,
                        float* edges, int32_t* slot_tri, float* tile_box, int32_t* tri_slot, float* area2, float* normal,
                        uint8_t* dropped, int64_t* dropped_count, void* stream);
int32_t mf_surface_closest(const float* records, const float* edges, const int32_t* slot_tri, const float* tile_box, int64_t T,
                        const float* query, int64_t Q, const int32_t* qorder, const int32_t* start, int32_t mode, float* d2,
                        int32_t* tri, float* point, uint8_t* region, int32_t* visited, void* stream);
int32_t mf_surface_weights(const float* area2, const uint8_t* dropped, int64_t T, const float* amax, int64_t* weights, void* stream);
int32_t mf_surface_sample(const float* verts, int64_t V, const int64_t* tris, int64_t T, const int64_t* cum, const int64_t* r,
                       const float* u, int64_t n, float* points, int32_t* tri, void* stream);
int64_t mf_surface_stats_scratch_bytes(int64_t n);
int32_t mf_surface_stats(const float* d2, int64_t n, const int32_t* tri_src, const int32_t* tri_dst, const float* normal_src,
                         int64_t T_src, const float* normal_dst, int64_t T_dst, const float* thresholds /* host */,
                         int32_t n_thresholds, double* out_f64, int64_t* out_i64, void* scratch, void* stream);

/* ---- ray casts against a mesh: the first hit of a ray on the triangles of an mf_surface_records index, or whether it has one
 * (csrc/mf_mesh_rays.hip).  The reference has no ray-mesh code.  THE CONTRACT IS FIXED ARITHMETIC, as in the section
 * above: every fp32 operation is rounded once, in the order written, without FMA; min / max are fminf / fmaxf (a NaN operand is
 * ignored); a / b is the correctly rounded quotient.  tests/mesh_rays_oracle.py restates every output in np.float32.  No atomics;
 * every result is bit-identical from run to run.  Nothing allocates or synchronises.
 *
 * mf_surface_corners: verts, tris as given to mf_surface_records and the slot_tri (Tp) it wrote -> corners (Tp, 16), 16-byte
 * aligned: per slot the three vertices a, b, c AS READ (9 floats), the triangle's box lo, hi (6 floats, the values of
 * edges[6 .. 11]) and a zero.  A slot with slot_tri outside [0, T), or whose triangle has an index outside [0, V) (both tested
 * before an address is formed), gets 16 zeros.
 *
 * mf_surface_cast: ray i is origins + i ray_stride, dirs + i ray_stride (3 floats each; ray_stride >= 3, in floats) with the range
 * t_min[i bound_stride] .. t_max[i bound_stride] (bound_stride >= 0; 0: one pair for every ray).  The package's (Q, 8) ray rows
 * (o, d, near, far) are origins = rows, dirs = rows + 3, t_min = rows + 6, t_max = rows + 7 and both strides 8.
 * Per ray (o, d, t_min, t_max): the ray is DEAD -- it hits nothing -- if a component of o or d is not finite, if d is all zero,
 * or if !(t_min <= t_max).  Otherwise kz = the first axis of the largest |d|, kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky
 * swapped if d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
 * Per vertex p of a triangle, exactly as read from verts: q = p - o; x = q[kx] - Sx q[kz], y = q[ky] - Sy q[kz], z = Sz q[kz].
 * (A vertex shared by two triangles gets the same three numbers in both.)
 * Per triangle with the sheared corners A, B, C:
 *   U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax (each two rounded products and one difference);  det = (U + V) + W
 *   t_raw = ((U Az + V Bz) + W Cz) (1 / det);  t = min(max(t_raw, zmin), zmax), zmin / zmax = min / max((Az, Bz), Cz)
 * The triangle is ACCEPTED iff (U, V, W all >= 0, or all <= 0) and det != 0 and min((Ax, Bx), Cx) <= 0 <= max((Ax, Bx), Cx) and
 * the same in y and t_min <= t <= t_max.  Both faces count.
 *   mode 0 (first): the lexicographic minimum of (t, caller's index) over the accepted kept triangles -> t (Q) fp32, tri (Q)
 *     int32, bary (Q, 3) = (U, V, W) (1 / det) of the winner, recomputed from its slot: the hit is bary0 a + bary1 b + bary2 c.
 *     A miss: t = +inf, tri = -1, bary = 0.  hit may be NULL.
 *   mode 1 (any): hit (Q) uint8 = 1 iff some kept triangle is accepted.  t, tri, bary may be NULL.
 * The rows are the rays of the tile walk of a MeshIndex search (the section above: qorder, start, visited).  cull: 0 = the sweep;
 * 1 = the cull: with the tile box translated by o (l = lo - o, h = hi - o) and
 *   x0 = l[kx] - max(Sx l[kz], Sx h[kz]), x1 = h[kx] - min(Sx l[kz], Sx h[kz]); y0, y1 the same with ky, Sy;
 *   z0 = min(Sz l[kz], Sz h[kz]), z1 = max(Sz l[kz], Sz h[kz])
 * a lane WANTS the tile unless its ray is dead, or (mode 1) it has a hit already, or !(x0 <= 0 <= x1), or !(y0 <= 0 <= y1), or
 * z1 < t_min, or z0 > t_max, or !(z0 <= best) (best: the lane's least t so far, +inf before); a lane wants nothing more when
 * its ray is dead or (mode 1) has its hit.
 *   P1  Cull equals sweep, bit for bit.  Subtracting a fixed o, multiplying by a fixed S and min / max are monotone under
 *       rounding, so the intervals of a box that contains a vertex contain the vertex's computed x, y, z.  An accepted triangle
 *       has 0 inside its own computed x and y ranges (a condition of acceptance) and t >= zmin >= z0, t <= zmax <= z1 (the
 *       clamp), so its tile is wanted by every lane it could still serve.
 *   P2  Watertight.  Neighbours see the same sheared end points of a shared edge, so its edge function in one is exactly the
 *       negation of that in the other; and a rounded difference of two rounded products never has the sign opposite to the
 *       exact one (rounding is monotone: a b >= c d gives fl(a b) >= fl(c d)).  So on the closed planar mesh of sheared
 *       points, computed acceptance of the sign test contains exact acceptance; the own-range conditions hold trivially for a
 *       triangle that exactly contains the origin.  det = 0 needs U = V = W = 0 (numbers of one sign do not cancel): a triangle
 *       sheared to a segment or a point -- its neighbours across the edges through the origin contain the origin too -- or
 *       one so small that all six fp32 products round to the same values; the argument does not cover the latter.
 *   P3  Order independence: the result is a minimum over a set, so the order of the index, of the rays, the start tiles and
 *       the launch shape cannot change it.
 *   P4  No atomics; a dropped triangle, or a slot without one (slot_tri < 0), never wins.
 * Every store is a vector store.
 *
 * Every count (V, T, Q) in [0, 2^31 - 1), a NULL that is needed, a mode or cull outside 0 .. 1, ray_stride < 3, bound_stride < 0,
 * corners not 16-byte aligned and an output that is an input are MF_E_INVALID with an mf_last_error text, settled before any
 * launch. ---- */
int32_t mf_surface_corners(const float* verts, int64_t V, const int64_t* tris, int64_t T, const int32_t* slot_tri, float* corners,
                           void* stream);
int32_t mf_surface_cast(const float* corners, const int32_t* slot_tri, const float* tile_box, int64_t T, const float* origins,
                        const float* dirs, int64_t ray_stride, const float* t_min, const float* t_max, int64_t bound_stride,
                        int64_t Q, const int32_t* qorder, const int32_t* start, int32_t mode, int32_t cull, float* t, int32_t* tri,
                        float* bary, uint8_t* hit, int32_t* visited, void* stream);

/* ---- sparse lattice queries: sigma only where a bit grid is occupied.  visualize_mesh (trainer_moco_flow.py:490-538,
 * trainer_nerf.py:200-259) evaluates every point of its lattice, and so does the lattice behind mf_occ_build; a body fills about a
 * tenth of its box.  The lattice is (n0, n1, n2) points, axis 2 fastest, given by three ascending fp32 coordinate tables;
 * world_of_axis (host int32[3], a permutation of (0, 1, 2)) names the world coordinate -- and so the grid axis -- that volume
 * axis a carries ((1, 0, 2) for visualize_mesh's 'xy' meshgrid).  A BRICK is 8 x 8 x 8 lattice points: brick (b0, b1, b2) owns
 * the indices [8 b_a, min(8 b_a + 7, n_a - 1)] of every axis, nb_a = ceil(n_a / 8), linear brick index (b0 nb1 + b1) nb2 + b2.
 * Each side in [1, 2^31) and fewer than 2^31 bricks, else MF_E_INVALID.  Integer work and copies only; no atomics, every output
 * word has one writer, bit-identical from run to run.  No entry allocates or synchronises. ----
 *
 * mf_lattice_select (serves trainer_moco_flow.py:490-538, trainer_nerf.py:200-259): bits / (gx, gy, gz) as mf_occ_build writes
 * them (padding bits zero); range_a (device int32 (nb_a, 2)): per brick coordinate of volume axis a the inclusive first and last
 * grid cell, along grid axis world_of_axis[a], that the brick's grown index range touches, or an empty range (first > last) --
 * built by the caller (moco_flow_amd/points.py restates mf_ray_clip's cell rule on the host); a range is clipped to the grid
 * before it is used.  A brick is active iff its three ranges are non-empty and some bit of the cell box they span is set: one
 * lane per brick ORs the box's words.  slot (nb0 nb1 nb2) int32 = the brick's rank among the active ones in ascending linear
 * index, or -1; brick_ids int32, room for nb0 nb1 nb2 entries, the first K written, ascending; count (device int64[1]) = K.
 * Ranks through the ordered scan (mf_scan.hpp); scratch: mf_lattice_select_scratch_bytes bytes. */
int64_t mf_lattice_select_scratch_bytes(int64_t n0, int64_t n1, int64_t n2);
int32_t mf_lattice_select(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, const int32_t* range0, const int32_t* range1,
                          const int32_t* range2, int64_t n0, int64_t n1, int64_t n2, const int32_t* world_of_axis /* host */,
                          int32_t* slot, int32_t* brick_ids, int64_t* count, void* scratch, void* stream);
/* mf_lattice_points (serves trainer_moco_flow.py:490-538, trainer_nerf.py:200-259): brick_ids (K) int32 -> points (K 512, 3)
 * fp32, the input of mf_points_sigma: brick r has rows [512 r, 512 r + 512), local order (l0, l1, l2) with l2 fastest, and
 * column world_of_axis[a] of a row is axis_a[min(8 b_a + l_a, n_a - 1)] -- a partial brick repeats its last point (those rows are
 * evaluated and never stored).  An id outside [0, nb0 nb1 nb2) is clamped, never dereferenced.  K = 0 launches nothing. */
int32_t mf_lattice_points(const int32_t* brick_ids, int64_t K, const float* axis0, const float* axis1, const float* axis2, int64_t n0,
                          int64_t n1, int64_t n2, const int32_t* world_of_axis /* host */, float* points, void* stream);
/* mf_lattice_scatter (serves trainer_moco_flow.py:490-538, trainer_nerf.py:200-259): sigma (K 512) fp32 in the row order of
 * mf_lattice_points, slot as mf_lattice_select wrote it -> volume (n0, n1, n2) fp32: point (i0, i1, i2) = sigma[512 s + (i0 % 8)
 * 64 + (i1 % 8) 8 + i2 % 8] with s the slot of its brick, or `fill` where s is -1 (or not below K).  ONE pass writes every point
 * exactly once: no memset, no second writer.  K = 0 (sigma may be NULL) fills the volume. */
int32_t mf_lattice_scatter(const float* sigma, const int32_t* slot, int64_t K, int64_t n0, int64_t n1, int64_t n2, float fill,
                           float* volume, void* stream);

/* ---- triangle rasterizer (moco_flow_amd/csrc/mf_raster.hip, which writes out the fill rule and every operation order): the
 * pictures the reference draws with pyrender -- the stage-1 views of the posed SMPL mesh and the SMPL overlay,
 * scripts/data_utils.py:23-86, 273-336 -- through the camera of mf_make_rays (utils/camera.py:29-81): with p_cam = R^T (p - t)
 * and z = -p_cam.z, column x = cx + f p_cam.x / z and row y = cy - f p_cam.y / z, one focal length for both axes.  The sample
 * of pixel (row j, column i) sits at (x, y) = (i + pixel_offset, j + pixel_offset); pixel_offset = 0 is where mf_make_rays shoots
 * that pixel's ray, 0.5 is OpenGL's sample position, anything else is MF_E_INVALID.
 * PYRENDER NOT RESTATED: its metallic-roughness BRDF and the three point lights of data_utils.py:36-46 are third-party
 * arithmetic this project does not restate and is UNPINNED against (as kornia and cv2 are); colours are the interpolated vertex
 * colours, optionally times a headlight term.
 * No entry allocates or synchronises; V, T in [0, 2^31), H, W >= 1 and H W < 2^31, else MF_E_INVALID. */

/* mf_project_vertices (data_utils.py:23-86, 273-336; camera.py:29-81): verts (V, 3) fp32 world, c2w_host the 3x4 row-major
 * camera-to-world matrix (host) -> screen (V, 2) int32 = (rintf(256 x), rintf(256 y)), saturated at +-2^30, and inv_z (V) = 1 / z.
 * A vertex with z <= znear (znear > 0), or with a NaN position, gets screen = (INT32_MIN, INT32_MIN) and inv_z = 0.  xy (V, 2)
 * fp32, optional: the unsnapped (x, y) (NaN for a flagged vertex).  fp32, every operation rounded once. */
int32_t mf_project_vertices(const float* verts, int64_t V, const float* c2w_host, float focal, float cx, float cy, float znear,
                            int32_t* screen, float* inv_z, float* xy, void* stream);
/* Bytes of the scratch mf_rasterize fills and mf_raster_resolve / mf_raster_shade read: the (H W) plane of 64-bit keys and the
 * 8-byte counter of dropped triangles (data_utils.py:23-86, 273-336; camera.py:29-81). */
int64_t mf_raster_scratch_bytes(int64_t H, int64_t W);
/* mf_rasterize (data_utils.py:23-86, 273-336; camera.py:29-81): clears the scratch, then one wave per 64 triangles of tris (T, 3)
 * int64 writes min((bits(z) << 32) | triangle index) over the triangles covering each sample.  Coverage is decided in int64 on
 * the snapped coordinates with a top-left fill rule; winding does not matter; zero-area triangles cover nothing; a triangle with
 * a flagged vertex, a vertex beyond +-2^15 pixels or a vertex index outside [0, V) is dropped whole and counted (no clipping).
 * Bit-identical from run to run and under any permutation of tris (up to the index itself); an exact depth tie goes to the
 * lower index.  T = 0 only clears. */
int32_t mf_rasterize(const int32_t* screen, const float* inv_z, int64_t V, const int64_t* tris, int64_t T, int64_t H, int64_t W,
                     float pixel_offset, void* scratch, void* stream);
/* mf_raster_resolve (data_utils.py:23-86, 273-336; camera.py:29-81): the scratch of mf_rasterize, with the arguments it was
 * filled from -> face (H, W) int32 (-1 = none), depth (H, W) fp32 camera-axis z (+inf where none), bary (H, W, 3) fp32
 * perspective-correct (zeros where none), dropped_out (device int64[1]).  Any output may be NULL, not all. */
int32_t mf_raster_resolve(const void* scratch, const int32_t* screen, const float* inv_z, int64_t V, const int64_t* tris, int64_t T,
                          int64_t H, int64_t W, float pixel_offset, int32_t* face, float* depth, float* bary, int64_t* dropped_out,
                          void* stream);
/* mf_raster_interpolate (data_utils.py:23-86, 273-336; camera.py:29-81): out (n_pix, C) = (bary_0 a_0 + bary_1 a_1) + bary_2 a_2
 * of the rows a_k = attrs[tris[face][k]] of attrs (V, C) fp32, 1 <= C <= 16; zeros where face is outside [0, T) or names a
 * vertex outside [0, V) (nothing is dereferenced). */
int32_t mf_raster_interpolate(const float* attrs, int64_t V, int32_t C, const int64_t* tris, int64_t T, const int32_t* face,
                              const float* bary, int64_t n_pix, float* out, void* stream);
/* mf_raster_shade (data_utils.py:23-86, 273-336; camera.py:29-81): ONE launch from the scratch of mf_rasterize to a frame.
 *   rgba  (H, W, 4) uint8, 4-byte aligned: covered: alpha 255 and (uint8) clamp(c 255 + 0.5, 0, 255) in fp32, truncated (the
 *         rounding of mf_frame_sheet), of c = (bary_0 c_0 + bary_1 c_1) + bary_2 c_2 over colors (V, 3) fp32 (NULL: 1), times
 *         ambient + (1 - ambient) |n . v| with MF_RASTER_SHADE_HEADLIGHT (n: unit normal of the triangle's world vertices verts
 *         (V, 3), v: unit vector from the surface point to the camera); elsewhere alpha 0 and the background (none: 0, one
 *         colour by value, or the (H, W, 3) uint8 image)
 *   mask  (H W) bytes 1 / 0;  depth (H, W) fp32 z, +inf where none;  face (H, W) int32, -1 where none
 *   ray_t (H, W) fp32 = z |((x - cx) / f, -(y - cy) / f, -1)| at the sample position: with pixel_offset 0 the point of that
 *         pixel's mf_make_rays ray is o + ray_t d; +inf where none
 * c2w travels by value (3x4 row-major).  Any output may be NULL, not all. */
enum { MF_RASTER_SHADE_NONE = 0, MF_RASTER_SHADE_HEADLIGHT = 1 };
enum { MF_RASTER_BG_NONE = 0, MF_RASTER_BG_COLOUR = 1, MF_RASTER_BG_IMAGE = 2 };
typedef struct mf_raster_shade_args {
  const void* scratch;
  const int32_t* screen; const float* inv_z; const float* verts; const float* colors; int64_t V;
  const int64_t* tris; int64_t T;
  int64_t H, W;
  float focal, cx, cy, pixel_offset;
  float c2w[12];
  int32_t shading; float ambient;
  int32_t background_kind; uint8_t background_colour[4]; const uint8_t* background_image;
  uint8_t* rgba; uint8_t* mask; float* depth; float* ray_t; int32_t* face;
} mf_raster_shade_args;
int32_t mf_raster_shade(const mf_raster_shade_args* a, void* stream);

/* ---- frame ingest (moco_flow_amd/csrc/mf_frames.hip): from decoded 8-bit frames to the tensors mf_ray_batch, mf_ssim and
 * mf_frame_sheet take -- the resize of datasets/moco_flow_dataset.py:51-55, 169 (also :45, the background image), the composite
 * of :174-176 over the whole frame, and the background plate of scripts/data_utils.py:150-163.  Integer arithmetic on bytes, or
 * fp32 rounded once per operation: every result is pinned bit for bit.  No entry allocates or synchronises. */

/* Bytes of the scratch mf_resize_u8 needs (datasets/moco_flow_dataset.py:51-55, 169): the byte image between the two passes,
 * F H0 W C, or 0 where at most one axis changes size.  -1 on a negative size or C outside {1, 3, 4}. */
int64_t mf_resize_u8_scratch_bytes(int64_t F, int64_t H0, int64_t W0, int32_t C, int64_t H, int64_t W);
/* mf_resize_u8 (datasets/moco_flow_dataset.py:51-55, 169: T.Resize on a PIL image): in (F, H0, W0, C) bytes -> out (F, H, W, C)
 * bytes, C in {1, 3, 4}, equal to Image.fromarray(a).resize((W, H), Image.BILINEAR) of PIL 12 bit for bit: the antialiased
 * triangle filter in two passes, horizontal first, with 22-bit fixed-point coefficients.
 *   Per axis (x: W0 -> W, y: H0 -> H) the caller uploads bounds (out, 2) int32 = (first tap, tap count n <= ksize) and kk (out,
 *   ksize) int32, zeros past n (moco_flow_amd/frames.py builds them in float64 as PIL's precompute_coeffs does).  A pass computes
 *   clamp((2^21 + sum_t pixel[first + t] kk_t) >> 22, 0, 255) in int32 and writes bytes; the vertical pass reads the horizontal
 *   pass's bytes (scratch).  A pass whose axis keeps its size is skipped (its tables may be NULL); neither changes: a plain copy.
 *   C = 4 is resampled premultiplied (PIL's RGBA -> RGBa -> resize -> RGBA): the first pass that runs loads c' = (t + (t >> 8))
 *   >> 8, t = c a + 128; the last one stores c = c' where a' is 0 or 255, else min(255, 255 c' / a'); the plain copy does
 *   neither.  in, out and scratch must be 4-byte aligned for C = 4.
 * A table entry is never trusted with an address: first and n are clamped to the axis; a coefficient is read as a 24-bit unsigned
 * number (PIL's are at most 2^22 + 1).  32-bit indexing: F H0 W0 C, F H0 W C and
 * F H W C below 2^31, else MF_E_INVALID (the Python side chunks the frames).  An output of 0 bytes launches nothing; an empty input
 * axis with a non-empty output is MF_E_INVALID. */
int32_t mf_resize_u8(const uint8_t* in, int64_t F, int64_t H0, int64_t W0, int32_t C, int64_t H, int64_t W,
                     const int32_t* xbounds, const int32_t* xkk, int32_t xksize,
                     const int32_t* ybounds, const int32_t* ykk, int32_t yksize, uint8_t* out, void* scratch, void* stream);

/* mf_composite_rows (datasets/moco_flow_dataset.py:169-176, over every pixel: what mf_ray_batch does for the selected ones):
 * rows_out (H W, 3) fp32 from
 *   MF_IMAGE_U8_RGBA  image (H, W, 4) bytes, 4-byte aligned: v_c a + bg_c (1 - a), the expression of mf_ray_batch (the same device
 *                     function: a row equals the batch's row bit for bit); needs a background
 *   MF_IMAGE_U8_RGB   image (H, W, 3) bytes: u * (1.0f / 255.0f); takes no background
 * background_kind: MF_BACKGROUND_ROWS (fp32 (H W, 3)), MF_BACKGROUND_COLOUR (3 device floats) or MF_BACKGROUND_U8 ((H, W, 3)
 * bytes, read as u * (1.0f / 255.0f) -- the plate of mf_background_plate as it stands).  Any other kind, H W >= 2^31 / 4 or a
 * NULL that is needed: MF_E_INVALID.  H W = 0 launches nothing. */
enum { MF_BACKGROUND_U8 = 3 };
int32_t mf_composite_rows(const void* image, int32_t image_kind, int64_t H, int64_t W, const void* background,
                          int32_t background_kind, float* rows_out, void* stream);

/* mf_background_plate (scripts/data_utils.py:150-163, generate_background_image): frames (F, H, W, C) bytes, C in {3, 4}
 * (channel 3 is ignored), masks (F, H, W) bytes -> out (H, W, 3) bytes.  Per pixel and channel the key of frame f is u (255 - m),
 * 0 .. 65025; out = (key_k + 127) / 255 in integer division of the k-th smallest key, k 0-based from the caller (the reference's
 * int(num_images * 0.8)).  That is floor(255 x + 0.5) of the reference's float64 np.sort(img / 255. * (1 - msk / 255.), axis=0)[k]:
 * 255 is odd, so no value lies within 1 / 510 of a rounding boundary.
 * The k-th key is found by 16 bisection steps on its bits, counting keys below the trial value; no atomics, bit-identical from run
 * to run.  path: MF_PLATE_AUTO stages a workgroup's tile of keys in LDS -- every frame byte is read from memory once -- while F is
 * within the LDS bound (a named constant of the unit) and streams the frames from memory per step beyond it; MF_PLATE_STAGED /
 * MF_PLATE_STREAMED force one (STAGED beyond the bound is MF_E_INVALID).  1 <= F < 65536, 0 <= k < F, H W < 2^31 / 4, else
 * MF_E_INVALID.  H W = 0 launches nothing. */
enum { MF_PLATE_AUTO = 0, MF_PLATE_STAGED = 1, MF_PLATE_STREAMED = 2 };
int32_t mf_background_plate(const uint8_t* frames, const uint8_t* masks, int64_t F, int64_t H, int64_t W, int32_t C, int64_t k,
                            int32_t path, uint8_t* out, void* stream);

/* ---- matte clean-up (csrc/mf_regions.hip): the connected regions of a thresholded byte image, per frame of an (F, H, W) stack.
 * Contract: members are alpha >= thres (below != 0: alpha < thres), thres in [0, 256]; regions are the 8- or 4-connected
 * components of the members of one frame (frames never interact, rows do not wrap); the label of a member is the smallest
 * row-major index y W + x of its region within its frame, -1 for a non-member; area = pixel count.  Integers only, every output a
 * pure function of the input.  Every entry: F, H, W >= 0 and F H W < 2^31 (32-bit indexing), else MF_E_INVALID; all refusals come
 * before any launch; F H W = 0 launches nothing.  Not cv2: contourArea is a polygon area, not a pixel count, and RETR_TREE's hole
 * contours erase a one-pixel ring around every hole of the kept region. */

/* mf_mask_label_scratch_bytes (scripts/data_utils.py:102-114, :135-147): bytes of the scratch that the five entries below share:
 * parent int32 [F H W] | area int32 [F H W] | uint64 [F] | int64 [launch constant].  -1 on a refused shape. */
int64_t mf_mask_label_scratch_bytes(int64_t F, int64_t H, int64_t W);

/* mf_mask_label (scripts/data_utils.py:102-114, :135-147: the threshold `raw[..., 3] >= thres` and the regions findContours
 * traces): pixel g of the stack is read at alpha[g stride], stride 1 (an alpha plane) or 4 (channel 3 of RGBA in place: pass
 * rgba + 3); connectivity 8 or 4.  labels (F, H, W) int32.  Leaves area[f H W + label] of every region in scratch for
 * mf_mask_select.  Lock-free union-find: per tile in LDS, across the tile seams in global memory, then one flattening pass; the
 * scratch may hold anything on entry.  thres outside [0, 256], another connectivity or stride, a NULL: MF_E_INVALID. */
int32_t mf_mask_label(const uint8_t* alpha, int32_t stride, int64_t F, int64_t H, int64_t W, int32_t thres, int32_t below,
                      int32_t connectivity, int32_t* labels, void* scratch, void* stream);

/* mf_mask_select (scripts/data_utils.py:102-114 find_max_region, :135-147): out (F, H, W) bytes = 255 where the pixel's region
 * has area >= min_area and (largest == 0 or it is its frame's largest region: most pixels, ties to the smaller label), else 0; a
 * frame without members is all 0.  scratch as mf_mask_label of these labels left it.  One 64-bit atomicMax per wave and frame
 * finds the winner; no host read. */
int32_t mf_mask_select(const int32_t* labels, int64_t F, int64_t H, int64_t W, int32_t largest, int64_t min_area, uint8_t* out,
                       void* scratch, void* stream);

/* mf_mask_fill_holes (scripts/data_utils.py:102-114, :135-147 keep the outer contour's inside): in place on mask (F, H, W) bytes,
 * 0 = outside.  A hole is a 4-connected component of the zeros of a frame without a pixel on the frame's first or last row or
 * column (the complement of 8-connected foreground: a pocket that leaks only through a diagonal gap is a hole, a bay on the
 * border is not); its pixels become 255.  H <= 2 or W <= 2: nothing to fill, nothing launched. */
int32_t mf_mask_fill_holes(uint8_t* mask, int64_t F, int64_t H, int64_t W, void* scratch, void* stream);

/* mf_mask_table_count / mf_mask_table_emit (scripts/data_utils.py:102-114: the areas find_max_region ranks; :135-147).
 * count: counts[f] (int64) = the regions of frame f of these labels.  emit, after the caller has read the counts: C = their sum;
 * table (C, 7) int32, rows (frame0 + frame, label, area, x0, y0, x1, y1) with inclusive bounds (frame0 >= 0: the stack's place
 * in a longer one that the caller passes chunk by chunk), in (frame, label) order (ordered integer
 * ranks, csrc/mf_scan.hpp); needs only the labels, the scratch may hold anything.  A C below the true count leaves the later
 * regions out, one above it leaves the extra rows 0; C < 0 or C > F H W: MF_E_INVALID.  C = 0 launches nothing. */
int32_t mf_mask_table_count(const int32_t* labels, int64_t F, int64_t H, int64_t W, int64_t* counts, void* stream);
int32_t mf_mask_table_emit(const int32_t* labels, int64_t F, int64_t H, int64_t W, int64_t frame0, int64_t C, int32_t* table,
                           void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOCOFLOW_HIP_H */
