// mf_render.hip -- one fused rendering pass of render_rays (models/rendering.py:195-375):
//
//   ray -> z (rendering.py:245-251) -> xyz (:262-263)
//       -> [bw NoF -> canonical xyz, fw NoF chains for the consensus terms (:270-286, :49-83)]
//       -> positional encoding (embedding.py:42-46) -> NeRF MLP (nerf.py:78-102)
//       -> sigma -> alpha -> exclusive transmittance scan -> rgb / depth / opacity (:157-192)
//
// in ONE kernel launch.  Nothing between the input rays and the output pixels is written to
// HBM except the optional (N,S) planes a caller asks for (weights/alphas feed sample_pdf and the
// consensus mask; disp_* are the per-sample consensus distances).
//
// Work decomposition: a workgroup (8 waves, two per SIMD, <= 256 registers each) takes a GROUP
// of G whole rays (G*S samples, a multiple of 128 whenever S allows), walks it in tiles of 128
// samples -- 16 per wave, one sample per lane&15, the four 16-lane groups holding the four
// k-quarters of every MFMA step -- and keeps each sample's (r,g,b,sigma,z) in LDS until the
// group's rays are composited by one wave per ray with a wavefront product-scan.  Workgroups
// are persistent (grid = #CUs) so the weight stream never drains between tiles.
#include <cstddef>

#include "mf_host.hpp"
#include "mf_layout.hpp"
#include "mf_nets.hpp"
#include "mf_plan.hpp"
#include "mf_raypass.hpp"

namespace mf {

struct RenderParams {
  const float* rays; long long ray_stride; long long n_rays;
  const float* bg;
  int S;
  const float* z_vals; const float* z_steps; int use_disp;
  const float* noise;
  int activation, flags;
  NetDev nerf;
  int extra_type;
  NetDev bw, fw;
  float emb_par[4][32];            // [nerf xyz, nerf extra, nof xyz, nof ind] x (freq[16], weight[16]) -> LDS at par_off
  uint32_t par_off;
  float *rgb, *depth, *opacity, *weights, *alphas, *disp_local, *disp_global;
  int G;
  long long n_groups;
  uint32_t ring_off, buf_bytes, sbuf_off, zbuf_off;
  int dbg;
  float* dump_acts; long long dump_stride; float* dump_rgbsigma; float* dump_xyz;   // training forward
  unsigned* dump_mask; long long dump_mask_stride;                                  // ReLU bit mask rows (optional)
  float* dump_nof_acts; long long dump_nof_stride; float* dump_nof_emb; float* dump_nof_out;   // per chain step
  uint32_t nof_plane_pack;     // plane of step k = (pack >> 3k) & 7   (a packed scalar: no runtime index into the kernarg)
};
// render_fold_kernel's parameters: RenderParams (the other kernels' kernarg stays what it was) and the group's per-ray bias table
// of extra_encoding, b' + W_e[:, W:] PE(ext): G rows of W/2 floats at rbias_off, behind them the rays' encodings (kRayPeFloats
// each); fold_wx = W_e[:, W:] in the packed buffer (FoldLayout::off_x), fold_xcols floats per row.  fold_wx null: no table
// (sigma-only pass, no extra block) -- every lane reads the layer's shared bias b'.
struct FoldRenderParams : RenderParams {
  const float* fold_wx; int fold_xcols;
  uint32_t rbias_off;
};
constexpr int kRayPeFloats = 32;          // an extra block's encoding, natural feature order, zero-padded (fold_ext_cols <= 32)
constexpr int kFoldHalf = 128;            // W / 2 of the folded kernels (W = 256 only)

// MF_BODY_FOLD: the body's text for the folded kernels (preprocessor, not `if constexpr`: it names FoldRenderParams' fields)
template <bool MOCO, bool DUMP>
__global__ __launch_bounds__(kThreads, 2) void render_kernel(RenderParams p) {
  constexpr bool FOLD = false;
#define MF_BODY_FOLD 0
#include "mf_render_body.hpp"
#undef MF_BODY_FOLD
}

// the two inference instantiations over the folded stream (MF_F_FOLDED_FINAL: nerf_eval<.., FOLD> skips xyz_encoding_final);
// kernels of their own name, so that render_kernel<MOCO, DUMP> keeps its names
template <bool MOCO>
__global__ __launch_bounds__(kThreads, 2) void render_fold_kernel(FoldRenderParams p) {
  constexpr bool DUMP = false, FOLD = true;
#define MF_BODY_FOLD 1
#include "mf_render_body.hpp"
#undef MF_BODY_FOLD
}

int render_pass_bf16(const mf_render_args* a, hipStream_t st, bool prepare_only);   // mf_render_bf16.hip
int64_t render_workspace_bytes_bf16(const mf_render_args* a);

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_render_workspace_bytes(const mf_render_args* a) {
  if (!a || (a->precision != MF_PREC_BF16 && a->precision != MF_PREC_BF16X3) || a->n_rays <= 0) return 0;
  return render_workspace_bytes_bf16(a);
}

extern "C" int32_t mf_nof_emb_slot_features(int32_t* features80) {
  if (!features80) return fail(MF_E_INVALID, "mf_nof_emb_slot_features: null argument");
  for (int g = 0; g < 4; ++g)
    for (int e = 0; e < kStepsNofIn; ++e) features80[kStepsNofIn * g + e] = emb_feature(kEmbNofIn, g, e, 33);
  return MF_OK;
}

// what every precision checks, in this order -- the fp32 layouts too: a descriptor the fp32 pass cannot take is refused as such
// before the bf16 pass looks at it; the fp32 layouts stay in L = {nerf, bw, fw} for render_pass_f32
static int32_t check_render_args(const mf_render_args* a, NetLayout (&L)[3]) {
  if (!a->rays || a->ray_stride < 9) return fail(MF_E_INVALID, "mf_render_pass: rays missing or ray_stride < 9");
  if (!a->z_vals && !a->z_steps) return fail(MF_E_INVALID, "mf_render_pass: need z_vals or z_steps");
  if (a->activation != MF_ACT_RELU && a->activation != MF_ACT_SOFTPLUS)
    return fail(MF_E_INVALID, "mf_render_pass: activation %d not supported", a->activation);
  if (a->precision < MF_PREC_F32 || a->precision > MF_PREC_BF16X3)
    return fail(MF_E_INVALID, "mf_render_pass: precision %d", a->precision);
  if (!nerf_layout(*a->nerf, L[0], 0)) return fail(MF_E_UNSUPPORTED, "mf_render_pass: unsupported NeRF configuration");
  if (L[0].NK != 16) return fail(MF_E_UNSUPPORTED, "mf_render_pass: only W=256 NeRF is built");
  const bool dump = a->dump_acts || a->dump_rgbsigma || a->dump_xyz || a->dump_nof_acts;
  if (dump && a->precision == MF_PREC_BF16)
    return fail(MF_E_UNSUPPORTED, "mf_render_pass: the activation dump (training forward) exists in fp32 and in bf16x3");
  if (a->flags & MF_F_FOLDED_FINAL) {         // the folded stream: fp32 inference only
    if (a->precision != MF_PREC_F32)
      return fail(MF_E_UNSUPPORTED, "mf_render_pass: MF_F_FOLDED_FINAL is built for MF_PREC_F32 (precision %d)", a->precision);
    if (dump || a->dump_mask || a->dump_nof_emb || a->dump_nof_out)
      return fail(MF_E_INVALID, "mf_render_pass: MF_F_FOLDED_FINAL with a dump_* pointer (the training forward reads mf_nerf_pack's stream)");
  }
  if (int e = check_xyz_embedding("mf_render_pass", a->emb_xyz, 10)) return e;
  // (the extra block's check stays here: MF_E_UNSUPPORTED and n_freqs < 0 read as no frequencies, unlike mf_points_radiance's -- mf_plan.hpp)
  const bool sigma_only = a->flags & MF_F_SIGMA_ONLY;
  if (!sigma_only && a->nerf->extra_feat_type == MF_EXTRA_DIR &&
      (a->emb_extra.in_channels != 3 || a->emb_extra.n_freqs > 4 ||
       3 * (2 * a->emb_extra.n_freqs + 1) > a->nerf->extra_feat_dim))
    return fail(MF_E_UNSUPPORTED, "mf_render_pass: dir embedding must have 3 channels, <= 4 frequencies and fit extra_feat_dim");
  if (!sigma_only && a->nerf->extra_feat_type == MF_EXTRA_IND &&
      (a->emb_extra.in_channels != 1 || a->emb_extra.n_freqs > 2 ||
       (2 * a->emb_extra.n_freqs + 1) > a->nerf->extra_feat_dim))
    return fail(MF_E_UNSUPPORTED, "mf_render_pass: ind embedding must have 1 channel, <= 2 frequencies and fit extra_feat_dim");
  const bool moco = a->nof_bw != nullptr;
  const bool chains = a->flags & (MF_F_CHAIN_LOCAL | MF_F_CHAIN_GLOBAL);
  if (!moco && chains) return fail(MF_E_INVALID, "mf_render_pass: chain flags need NoF models");
  if ((a->flags & MF_F_CHAIN_GLOBAL) && !(a->flags & MF_F_CHAIN_LOCAL))
    return fail(MF_E_INVALID, "mf_render_pass: chain_global without chain_local (the reference raises UnboundLocalError, rendering.py:276-280)");
  if ((a->flags & MF_F_CHAIN_GLOBAL) && a->ray_stride < 10)
    return fail(MF_E_INVALID, "mf_render_pass: chain_global needs the chained image index column (ray_stride >= 10)");
  if (moco) {
    if (!a->nof_bw_packed) return fail(MF_E_INVALID, "mf_render_pass: nof_bw_packed missing");
    if (!nof_layout(*a->nof_bw, L[1], 0)) return fail(MF_E_UNSUPPORTED, "mf_render_pass: unsupported backward NoF configuration");
    if (chains) {
      if (!a->nof_fw || !a->nof_fw_packed) return fail(MF_E_INVALID, "mf_render_pass: chain flags need the forward NoF");
      if (!nof_layout(*a->nof_fw, L[2], 0)) return fail(MF_E_UNSUPPORTED, "mf_render_pass: unsupported forward NoF configuration");
    }
    if (int e = check_nof_embeddings("mf_render_pass", a->nof_emb_xyz, a->nof_emb_ind)) return e;
  }
  return MF_OK;
}

// the fp32 pass of checked arguments: LDS placement, launch planning, the dumps' checks, launch
static int32_t render_pass_f32(const mf_render_args* a, const NetLayout (&L)[3], hipStream_t st) {
  const bool moco = a->nof_bw != nullptr;
  const bool chains = a->flags & (MF_F_CHAIN_LOCAL | MF_F_CHAIN_GLOBAL);
  FoldRenderParams p{};                    // (the unfolded kernels take its RenderParams)
  fill_render_io(p, a);
  p.dbg = debug_flags();
  LdsPlan plan;
  auto place = [&](NetDev& n, const NetLayout& l, const void* packed) { n.L = l; plan.place(n, packed); };
  place(p.nerf, L[0], a->nerf_packed);
  emb_table(a->emb_xyz, p.emb_par[0], p.emb_par[0] + 16);
  emb_table(a->emb_extra, p.emb_par[1], p.emb_par[1] + 16);
  if (moco) {
    place(p.bw, L[1], a->nof_bw_packed);
    if (chains) place(p.fw, L[2], a->nof_fw_packed);
    emb_table(a->nof_emb_xyz, p.emb_par[2], p.emb_par[2] + 16);
    emb_table(a->nof_emb_ind, p.emb_par[3], p.emb_par[3] + 16);
  }
  p.par_off = plan.place_tables();
  plan.ring(p.ring_off, p.buf_bytes);
  uint32_t lds = plan.lds;                 // the group's sample buffers go behind the ring

  // the folded kernels' per-ray bias table: one row of W/2 floats and one encoding per ray of the group, beside the 20 bytes per
  // staged sample -- where that leaves no room for the ray sets a group had, plan_ray_groups takes fewer
  FoldLayout F{};
  NetLayout Lf;
  const bool ray_table = (a->flags & MF_F_FOLDED_FINAL) && !(a->flags & MF_F_SIGMA_ONLY) &&
                         a->nerf->extra_feat_type != MF_EXTRA_NONE && nerf_fold_layout(*a->nerf, Lf, F);
  uint32_t ray_bytes = ray_table ? (kFoldHalf + kRayPeFloats) * 4 : 0;
  // A ray so long that its samples leave no room for one row (the envelope: S up to all the LDS behind the ring): the group is
  // that single ray, and its row and encoding live in the resident block's bias slot of xyz_encoding_final (W floats), which the
  // folded kernels never read.
  const bool home_row = ray_table && lds < kRenderLdsCap && (long long)a->n_samples * 20 + ray_bytes > (long long)(kRenderLdsCap - lds);
  if (home_row) ray_bytes = 0;
  if (int e = plan_ray_groups(a->n_rays, a->n_samples, kTile, lds, p.G, p.n_groups, ray_bytes)) return e;
  if (home_row) { p.G = 1; p.n_groups = a->n_rays; }
  place_sample_buffers(p, lds);
  if (ray_table) {
    static_assert((kFoldHalf + kRayPeFloats) <= 2 * kFoldHalf, "one row and one encoding fit a W-float bias slot");
    p.fold_wx = reinterpret_cast<const float*>(static_cast<const char*>(a->nerf_packed) + F.off_x);
    p.fold_xcols = fold_ext_cols(Lf);
    if (home_row) p.rbias_off = p.nerf.res_lds + (uint32_t)(p.nerf.L.off_bias_trunk + (p.nerf.L.n_trunk - 1) * p.nerf.L.W) * 4;
    else { p.rbias_off = lds; lds += (uint32_t)p.G * ray_bytes; }      // G rows, then G encodings
  }

  if (int e = check_dump_rows(a, p.nerf.L)) return e;
  if (int e = check_dump_mask(a, p.nerf.L)) return e;
  if (a->dump_nof_acts) {
    if (!moco || !a->dump_nof_emb || !a->dump_nof_out) return fail(MF_E_INVALID, "mf_render_pass: dump_nof_acts needs NoF models, dump_nof_emb and dump_nof_out");
    if (a->dump_nof_stride < (int64_t)p.bw.L.n_trunk * p.bw.L.W + 16 || (a->dump_nof_stride & 3))
      return fail(MF_E_INVALID, "mf_render_pass: dump_nof_stride %lld invalid", (long long)a->dump_nof_stride);
    if (a->nof_fw && (p.fw.L.n_trunk != p.bw.L.n_trunk || p.fw.L.W != p.bw.L.W))
      return fail(MF_E_UNSUPPORTED, "mf_render_pass: NoF dumps need bw and fw of the same depth and width");
    if (int e = nof_plane_pack(a, p.nof_plane_pack)) return e;
  }
  p.dump_nof_acts = a->dump_nof_acts; p.dump_nof_stride = a->dump_nof_stride; p.dump_nof_emb = a->dump_nof_emb; p.dump_nof_out = a->dump_nof_out;
  const bool dump = a->dump_acts || a->dump_rgbsigma || a->dump_xyz || a->dump_nof_acts;
  if (!dump && (a->flags & MF_F_FOLDED_FINAL))
    return launch_lds(moco ? render_fold_kernel<true> : render_fold_kernel<false>, persistent_grid(p.n_groups), kThreads, lds, st, p,
                      "mf_render_pass", "mf_render_pass");
  void (*kern)(RenderParams) = dump ? (moco ? render_kernel<true, true> : render_kernel<false, true>)
                                    : (moco ? render_kernel<true, false> : render_kernel<false, false>);
  return launch_lds(kern, persistent_grid(p.n_groups), kThreads, lds, st, static_cast<const RenderParams&>(p), "mf_render_pass",
                    "mf_render_pass");
}

static int32_t render_entry(const mf_render_args* a, void* stream, bool prepare_only) {
  if (!a || !a->nerf || !a->nerf_packed) return fail(MF_E_INVALID, "mf_render_pass: null argument");
  if (a->n_rays < 0 || a->n_samples < 1) return fail(MF_E_INVALID, "mf_render_pass: n_rays=%lld n_samples=%d", (long long)a->n_rays, a->n_samples);
  if (a->n_rays == 0) return MF_OK;
  NetLayout L[3];
  if (int e = check_render_args(a, L)) return e;
  if (a->precision != MF_PREC_F32) return render_pass_bf16(a, static_cast<hipStream_t>(stream), prepare_only);   // own layouts / launch
  return prepare_only ? MF_OK : render_pass_f32(a, L, static_cast<hipStream_t>(stream));
}
extern "C" int32_t mf_render_pass(const mf_render_args* a, void* stream) { return render_entry(a, stream, false); }
extern "C" int32_t mf_render_prepare(const mf_render_args* a, void* stream) { return render_entry(a, stream, true); }
