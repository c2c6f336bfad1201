// mf_layout.hpp -- packed-buffer layouts derived from the C-ABI descriptors (host + device).
#pragma once
#include "../../include/mocoflow_hip.h"
#include "mf_core.hpp"

namespace mf {

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// the single skip layer of a D-layer trunk (skip_mask bits 1 .. D-1): 0 = none, -1 = several
inline int single_skip_layer(uint32_t skip_mask, int D) {
  int s = 0;
  for (int l = 1; l < D; ++l)
    if ((skip_mask >> l) & 1u) { if (s) return -1; s = l; }
  return s;
}

// ------------------------------------------------------------------ the packed fragment streams (mf_pack.hip: pack_panels_kernel)
// Every stream -- the forward's W and each backward chain's W^T -- is a list of regions written by one kernel.  A region is
// `tiles` panels of `groups` 1 KiB groups; a panel's k range is up to two blocks in stream order.  Element (n, c) of a block's
// matrix is src[n * s_n + c * s_k]: a forward block reads W, (s_n, s_k) = (n_in, 1), a backward block the same layout of W^T,
// (1, ld).  fp32: panel = 32 rows, its groups alternate between its two 16-row tiles; group (tile half, k-quad q) holds, for
// lane (i = lane & 15, g = lane >> 4) and r = 0..3, row 32 P + 16 half + i at column c(step = 4 q + r, g).  bf16 (mf_bf16.hpp):
// panel = ONE 32-row tile, group = A fragment of v_mfma_f32_32x32x16_bf16: lane (i = lane & 31, h = lane >> 5) holds 8 bf16 =
// row 32 P + i at column c(k-step, slot 8 h + e), e = 0..7, each k-step as `split` groups (hi, lo[, ...] terms).
constexpr int kPackHidden = -1;   // PackBlock::kind of a plain k range: c = 16 q + 4 g + r (fp32) | 16 ks + hid_perm2(h, e) (bf16)
struct PackBlock {
  const float* src;
  int s_n, s_k;
  int kind;                  // kPackHidden, or the EmbKind of an embedded-input block (emb_feature / emb_feature2, mf_core.hpp)
  int steps;                 // fp32: k-quads (two groups each); bf16: 16-k steps (`split` groups each); 0 = no block
  int split;                 // bf16: groups per k-step: 1 = plain, 2 = (hi, lo), 3 = (hi, mid, lo)
  int cols;                  // columns present (c >= cols: zero)
};

struct PackRegion {          // one layer's panels
  PackBlock blk[2];
  int tiles;                 // panels
  int groups;                // groups per panel
  int n_rows;                // rows present (n >= n_rows: zero; 0 = all)
  int row_terms;             // bf16 head panels of the fast mode (NetLayout::head_tiles): tile row c < n_rows = bf16(W[c]), row row_terms + c =
                             // bf16(W[c] - hi); row_terms = 8 (NeRF sigma / rgb: <= 4 rows) or 16 (NoF head: 3 | 9 rows); 0 = off
  long long dst_group0;      // first group index (in 1 KiB units) within the panel area
};

struct ResCopy { const float* src; int dst_off; int n; float scale = 1.f; };

struct PackJob {
  PackRegion reg[MF_MAX_LAYERS + 3];
  int n_regions;
  int bf16;                  // groups hold 8 bf16 per lane (32x32x16 A fragments) instead of 4 fp32
  int xyz_cols;              // kEmbNofIn blocks: the index block starts there
  int half;                  // the split terms are IEEE halves of wscale * w (NetLayout::half) instead of bf16
  float wscale;
  long long total_groups;
  float* panels;
  float* poison;             // half-pair layouts: resident head-bias rows 27 (+ 4 = 31), set to NaN when a weight saturates; else null
  ResCopy res[2];            // the resident block, filled by the same launch (backward streams; the forward's has a launch of its own)
  int n_res, res_floats;
  float* resident;
  PackRegion& add(int tiles, int groups, const PackBlock& b0, const PackBlock& b1 = PackBlock{}) {   // host: the next region
    PackRegion& R = reg[n_regions++];
    R = PackRegion{{b0, b1}, tiles, groups, 0, 0, total_groups};
    total_groups += (long long)groups * tiles;
    return R;
  }
};
static_assert(sizeof(PackJob) <= 2048, "pack_panels_kernel's argument block");

// one launch of pack_panels_kernel: the job's resident block and its panels (mf_pack.hip)
int launch_pack(const PackJob& job, hipStream_t st, const char* what);

// returns false (layout zeroed) for configurations the kernels do not implement
// `bf16` = the MF_PREC_* value: 0 fp32, 1 bf16, 2 bf16x3 (bf16 layout with more (hi, lo) split ranges, mf_bf16.hpp)
inline bool nerf_layout(const mf_nerf_desc& d, NetLayout& L, int bf16 = 0) {
  L = NetLayout{};
  const bool x3 = bf16 == MF_PREC_BF16X3;
  L.bf16 = bf16 ? 1 : 0;
  if (d.W != 256 && d.W != 128) return false;
  if (d.D < 2 || d.D + 1 > MF_MAX_LAYERS) return false;
  // the embedded xyz block has slots for 3 channels x <= 10 frequencies = 63 features; a narrower in_channels_xyz (the
  // reference's default is 33, models/nerf.py:6-12) leaves the upper features without a weight column (packed as zeros), a
  // 64th column only ever sees the reference's zero padding (rendering.py:127-129)
  if (d.in_channels_xyz < 3 || d.in_channels_xyz > 64) return false;
  if (d.extra_feat_type != MF_EXTRA_NONE && (d.extra_feat_dim < 1 || d.extra_feat_dim > 32)) return false;
  if (d.skip_mask & 1u) return false;                 // layer 0 already takes the input
  if (d.skip_mask >> d.D) return false;
  L.W = d.W;
  L.NK = d.W / 16;
  L.NP = d.W / 32;
  L.n_trunk = d.D + 1;                                // + xyz_encoding_final (no ReLU)
  if (bf16 && d.W != 256) return false;
  L.emb_steps = bf16 ? kKsNerfXyz : kStepsNerfXyz;     // bf16: 16-slot k-steps (mf_bf16.hpp); fp32: 4-k MFMA steps
  L.emb_split = x3 ? 1 : 0;                            // bf16: the NeRF's encodings are plain bf16 operands (mf_bf16.hpp); x3: split
  L.hsplit_mask = x3 ? ((1u << (d.D + 2)) - 1u) & ~1u : 0u;   // x3: every hidden range (trunk, final, extra_encoding) as (hi, lo) pairs
  L.terms = 2;
  L.emb_mask = 1u | d.skip_mask;
  L.relu_mask = (1u << d.D) - 1u;
  switch (d.extra_feat_type) {
    case MF_EXTRA_NONE: L.extra_steps = 0; break;
    case MF_EXTRA_IND: L.extra_steps = bf16 ? kKsInd : kStepsInd; if (d.extra_feat_dim < 1) return false; break;
    case MF_EXTRA_DIR: L.extra_steps = bf16 ? kKsDir : kStepsDir; if (d.extra_feat_dim < 3) return false; break;
    default: return false;
  }
  int off = 0;
  L.off_bias_trunk = off; off += L.n_trunk * L.W;
  L.off_bias_extra = off; off += L.W / 2;
  L.off_head_w = off; off += L.W;
  L.off_head_b = off; off += 4;
  L.off_rgb_w = off; off += 3 * (L.W / 2);
  L.off_rgb_b = off; off += 4;
  L.n_head = 1;
  L.head_tiles = bf16 == MF_PREC_BF16 ? 1 : 0;        // fast bf16 mode: sigma / rgb heads on the matrix pipe (NetLayout::head_tiles)
  L.res_bytes = round_up((int64_t)off * 4, kGroupBytes);
  int64_t groups = 0;
  L.max_groups = 0;
  // stream order: trunk layers 0 .. D-1, [sigma head panel], xyz_encoding_final, extra_encoding, [rgb head panel]
  for (int l = 0; l < L.n_trunk; ++l) {
    if (l == L.n_trunk - 1) groups += nerf_sigma_groups(L);
    const int g = trunk_groups(L, l);
    groups += (int64_t)g * L.NP;
    if ((x3 ? panel_cap(g) : g) > L.max_groups) L.max_groups = x3 ? panel_cap(g) : g;
  }
  const int ge = extra_groups(L);
  groups += (int64_t)ge * (L.NP / 2);      // (W/2)-wide layer: NP/2 panels in either layout
  if ((x3 ? panel_cap(ge) : ge) > L.max_groups) L.max_groups = x3 ? panel_cap(ge) : ge;
  groups += nerf_rgb_groups(L);
  L.panel_bytes = groups * kGroupBytes;
  return true;
}

// The folded fp32 stream (mf_nerf_pack_fold, MF_F_FOLDED_FINAL): xyz_encoding_final has no activation and extra_encoding is its
// only consumer, so W' = W_e[:, :W] W_f and b' = b_e + W_e[:, :W] b_f replace the two layers' hidden part.  The stream is the
// fp32 one without the final layer's NP panels -- trunk 0 .. D-1, then extra_encoding over [h_{D-1} ; extra block] -- and the
// resident block keeps its size and offsets (the final layer's bias slot is unused, off_bias_extra holds b').  L stays the
// unfolded layout: the kernels read the same offsets and panel sizes from it.  W' ((W/2) x W, row-major) and b' (W/2) live in
// a scratch area behind the panels, padded to a whole group; it belongs to the packed buffer.  fp32 and W = 256 only.
// The extra block (rendering.py:133-142: the encoding of the ray's direction or image index) is the same for every sample of a
// ray, so the folded kernels add W_e[:, W:] PE(ext) to b' once per ray (mf_render_body.hpp, the per-ray bias table) and the
// stream's extra panels carry the hidden block alone: fold_extra_groups = 32 groups per panel, 2 048 in all instead of 2 064
// for a 27-column block.  W_e[:, W:] sits behind W' and b' for that phase: W/2 rows in natural order, fold_ext_cols floats
// each (the block's columns, zero-padded) -- exactly the bytes the extra k-quads occupied in the panels, so the packed buffer
// keeps its size.  (fold_extra_groups, fold_ext_cols: mf_core.hpp)
struct FoldLayout {
  int64_t panel_bytes;       // the folded stream's panels
  int64_t scratch_bytes;     // W' then b' (padded to a group), then W_e[:, W:]
  int64_t off_w, off_b;      // byte offsets of W' and b' in the packed buffer
  int64_t off_x;             // byte offset of W_e[:, W:] ((W/2) x fold_ext_cols, row-major)
};
inline bool nerf_fold_layout(const mf_nerf_desc& d, NetLayout& L, FoldLayout& F) {
  F = FoldLayout{};
  if (!nerf_layout(d, L, 0) || L.W != 256) return false;
  F.panel_bytes = L.panel_bytes - (int64_t)trunk_groups(L, L.n_trunk - 1) * L.NP * kGroupBytes -
                  (int64_t)(extra_groups(L) - fold_extra_groups(L)) * (L.NP / 2) * kGroupBytes;
  const int64_t wb_bytes = round_up(((int64_t)(L.W / 2) * L.W + L.W / 2) * 4, kGroupBytes);
  F.scratch_bytes = wb_bytes + (int64_t)(L.W / 2) * fold_ext_cols(L) * 4;
  F.off_w = L.res_bytes + F.panel_bytes;
  F.off_b = F.off_w + (int64_t)(L.W / 2) * L.W * 4;
  F.off_x = F.off_w + wb_bytes;
  return true;
}

// wide_ok: W = 256 too (fp32 only) -- the reference's bare `NoF()` (models/nof.py:7-15: D = 8, W = 256, skips = [4]); built for the
// module-level forward alone (mf_nof_forward and its packer): the fused passes keep three networks' resident blocks beside the ring
// and have no room for 256-wide NoFs, every other entry point keeps rejecting them
inline bool nof_layout(const mf_nof_desc& d, NetLayout& L, int bf16 = 0, bool wide_ok = false) {
  L = NetLayout{};
  const bool x3 = bf16 == MF_PREC_BF16X3;
  L.bf16 = bf16 ? 1 : 0;
  if (d.W != 128 && !(wide_ok && !bf16 && d.W == 256)) return false;
  if (d.D < 2 || d.D > MF_MAX_LAYERS) return false;
  // slots for 3 x <= 5 xyz frequencies (33 features) and 1 x <= 16 index frequencies (33); narrower blocks leave the upper
  // features without a column (models/nof.py:7-15: in_channels_xyz = 33, extra_feat_dim = 0 by default)
  if (d.in_channels_xyz < 3 || d.in_channels_xyz > 33 || d.extra_feat_dim < 0 || d.extra_feat_dim > 33) return false;
  if ((d.skip_mask & 1u) || (d.skip_mask >> d.D)) return false;
  L.W = d.W;
  L.NK = d.W / 16;
  L.NP = d.W / 32;
  L.n_trunk = d.D;
  L.emb_steps = bf16 ? kKsNofXyz : kStepsNofIn;         // bf16: xyz block only, the image-index block is a per-ray bias
  L.emb_split = bf16 ? 1 : 0;                          // bf16: the NoF's embedded input keeps 16 mantissa bits
  L.hsplit_mask = x3 ? ((1u << d.D) - 1u) & ~1u : 0u;  // x3: every hidden range split too
  L.terms = x3 ? kNofTermsX3 : 2;                      // x3: kNofTermsX3 terms per split operand (mf_core.hpp)
  L.half = (x3 && kNofHalfX3) ? 1 : 0;                 // x3: IEEE-half (hi, lo) pairs, scaled (mf_core.hpp)
  L.head_tiles = bf16 == MF_PREC_BF16 ? 1 : 0;         // fast mode: the head panel's terms as tile rows (NetLayout::head_tiles)
  L.emb_mask = 1u | d.skip_mask;
  L.relu_mask = (1u << d.D) - 1u;
  L.extra_steps = -1;
  L.n_head = d.use_quat ? 9 : 3;
  int off = 0;
  L.off_bias_trunk = off; off += L.n_trunk * L.W;
  L.off_head_w = off; off += L.n_head * L.W;
  L.off_head_b = off; off += bf16 ? 32 : 12;          // bf16: the head is an MFMA tile, its bias a 32-row vector
  L.res_bytes = round_up((int64_t)off * 4, kGroupBytes);
  int64_t groups = 0;
  L.max_groups = 0;
  for (int l = 0; l < L.n_trunk; ++l) {
    const int g = trunk_groups(L, l);
    groups += (int64_t)g * L.NP;
    if ((x3 ? panel_cap(g) : g) > L.max_groups) L.max_groups = x3 ? panel_cap(g) : g;
  }
  if (bf16) {                                          // head panel: one 32-row tile, hidden k-steps as (hi, lo[, ...]) groups
    groups += head_groups(L);
    if (head_groups(L) > L.max_groups) L.max_groups = head_groups(L);
  }
  L.panel_bytes = groups * kGroupBytes;
  L.n_emb_layers = __builtin_popcount(L.emb_mask);
  L.ind_bytes = bf16 ? round_up((int64_t)L.n_emb_layers * L.W * kNofIndCols * 4, kGroupBytes) : 0;
  return true;
}

}  // namespace mf
