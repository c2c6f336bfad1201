// mf_forward.hip -- module-level entry points (the trainers call the networks directly,
// outside render_rays: trainer_moco_flow.py:146-187, 508-526; trainer_nerf.py:231,240):
//   mf_embedding_forward : Embedding.forward   models/embedding.py:30-47
//   mf_nerf_forward      : NeRF.forward        models/nerf.py:61-102
//   mf_nof_forward       : NoF.forward         models/nof.py:55-85
// The two network kernels run the same register-resident MFMA core as the fused render pass;
// only the prologue (embedded inputs are read from memory instead of being computed) and the
// epilogue (raw rgb/sigma rows are stored instead of being composited) differ.
#include "mf_host.hpp"
#include "mf_layout.hpp"
#include "mf_nets.hpp"
#include "mf_plan.hpp"
#include "mf_raypass.hpp"

namespace mf {

// ------------------------------------------------------------------ Embedding.forward
struct EmbFwdParams {
  mf_embedding e;
  const float* x;
  float* out;
  long long B;
  long long out_stride;   // floats per output row (>= the embedding's width; the columns past it are written 0)
  int repeat;             // output row b embeds input row b / repeat
};

// one thread per (output row, unit): unit u < C copies x_u; C <= u < C + C F evaluates ONE sincos for (frequency, channel)
// and writes both of its columns; the remaining units write the zero padding up to out_stride
__global__ void embedding_forward_kernel(EmbFwdParams p) {
  const int C = p.e.in_channels, F = p.e.n_freqs;
  const int OC = C * (2 * F + 1);
  const int units = C + C * F + (int)(p.out_stride - OC);
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.B * units) return;
  const long long b = idx / units;
  const int u = (int)(idx - b * units);
  const float* x = p.x + (b / p.repeat) * C;
  float* o = p.out + b * p.out_stride;
  if (u < C) {
    o[u] = x[u];
  } else if (u < C + C * F) {
    const int f = (u - C) / C, c = (u - C) % C;
    float sn, cs;
    sincosf(p.e.freq[f] * x[c], &sn, &cs);
    o[C + (2 * f) * C + c] = p.e.weight[f] * sn;
    o[C + (2 * f + 1) * C + c] = p.e.weight[f] * cs;
  } else {
    o[OC + (u - C - C * F)] = 0.f;
  }
}

// ------------------------------------------------------------------ NeRF.forward
struct NerfFwdParams {
  NetDev net;
  const float* in;
  long long in_stride, B;
  int sigma_only, extra_kind, extra_cols, xyz_cols;
  float* out;
  float* dump; long long dump_stride;          // DUMP: per-sample layer outputs [h_0 .. h_{D-1} | final | extra], as mf_render_pass dumps them
  uint32_t ring_off, buf_bytes;
};

template <bool DUMP>
__global__ __launch_bounds__(kThreads, 2) void nerf_forward_kernel(NerfFwdParams p) {
  const LaneId id;
  NetDev net = p.net;
  load_resident(net, id);
  Stream st;
  CarryT<kPD> carry;
  st.open(p.ring_off, p.buf_bytes);
  start_program(net, st, carry, id);                    // also drains the resident-block DMA
  const long long ntiles = (p.B + kTile - 1) / kTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long b = tile * kTile + id.wave * kWaveSamples + id.j;
    const bool valid = b < p.B;
    const float* row = p.in + (valid ? b : p.B - 1) * p.in_stride;
    float embx[kStepsNerfXyz], ext[kStepsExtraMax];
#pragma unroll
    for (int e = 0; e < kStepsNerfXyz; ++e) {
      const int f = sel4(id.g, emb_feature(kEmbNerfXyz, 0, e, 0), emb_feature(kEmbNerfXyz, 1, e, 0),
                         emb_feature(kEmbNerfXyz, 2, e, 0), emb_feature(kEmbNerfXyz, 3, e, 0));
      embx[e] = (f >= 0 && f < p.xyz_cols) ? row[f] : 0.f;      // (features beyond in_channels_xyz have no input column)
    }
#pragma unroll
    for (int e = 0; e < kStepsExtraMax; ++e) {
      int f = -1;
      if (p.extra_kind == kEmbDir)
        f = sel4(id.g, emb_feature(kEmbDir, 0, e, 0), emb_feature(kEmbDir, 1, e, 0), emb_feature(kEmbDir, 2, e, 0),
                 emb_feature(kEmbDir, 3, e, 0));
      else if (p.extra_kind == kEmbInd)
        f = sel4(id.g, emb_feature(kEmbInd, 0, e, 0), emb_feature(kEmbInd, 1, e, 0), emb_feature(kEmbInd, 2, e, 0),
                 emb_feature(kEmbInd, 3, e, 0));
      ext[e] = (!p.sigma_only && f >= 0 && f < p.extra_cols) ? row[p.xyz_cols + f] : 0.f;
    }
    float sigma, rgb[3] = {0.f, 0.f, 0.f};
    float* dump_row = nullptr;
    if constexpr (DUMP) {
      if (valid) dump_row = p.dump + b * p.dump_stride;
    }
    nerf_eval<16, DUMP>(net, embx, ext, p.sigma_only != 0, st, carry, id, follow_of(net), sigma, rgb, dump_row);
    // (the sample index is rebuilt from an opaque lane index: the 64-bit output address is then formed here instead of
    //  being carried -- with DUMP: spilled -- across the MFMA section)
    int jo = id.j;
    asm volatile("" : "+v"(jo));
    const long long bo = tile * kTile + id.wave * kWaveSamples + jo;
    if (bo < p.B && id.g == 0) {
      if (p.sigma_only) p.out[bo] = sigma;
      else *reinterpret_cast<float4*>(p.out + bo * 4) = make_float4(rgb[0], rgb[1], rgb[2], sigma);
    }
  }
  wait_vm0();   // the stream runs two panels ahead: drain the LDS-DMA before the workgroup retires
}

// ------------------------------------------------------------------ NoF.forward
struct NofFwdParams {
  NetDev net;
  const float* in;
  long long in_stride, B;
  const float* xyz;
  float* out;
  uint32_t ring_off, buf_bytes;
  int xyz_cols, in_cols;     // in_channels_xyz, in_channels_xyz + extra_feat_dim: the columns an input row has
};

template <int NK>
__global__ __launch_bounds__(kThreads, 2) void nof_forward_kernel(NofFwdParams p) {
  const LaneId id;
  NetDev net = p.net;
  load_resident(net, id);
  Stream st;
  CarryT<kPD> carry;
  st.open(p.ring_off, p.buf_bytes);
  start_program(net, st, carry, id);
  const long long ntiles = (p.B + kTile - 1) / kTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long b = tile * kTile + id.wave * kWaveSamples + id.j;
    const bool valid = b < p.B;
    const long long bb = valid ? b : p.B - 1;
    const float* row = p.in + bb * p.in_stride;
    float emb[kStepsNofIn];
#pragma unroll
    for (int e = 0; e < kStepsNofIn; ++e) {
      const int f = sel4(id.g, emb_feature(kEmbNofIn, 0, e, p.xyz_cols), emb_feature(kEmbNofIn, 1, e, p.xyz_cols),
                         emb_feature(kEmbNofIn, 2, e, p.xyz_cols), emb_feature(kEmbNofIn, 3, e, p.xyz_cols));
      emb[e] = (f >= 0 && f < p.in_cols) ? row[f] : 0.f;
    }
    const float xyz[3] = {p.xyz[bb * 3 + 0], p.xyz[bb * 3 + 1], p.xyz[bb * 3 + 2]};
    float o[3];
    nof_eval<false, NK>(net, emb, xyz, st, carry, id, follow_of(net), o);
    if (valid && id.g == 0) {
      p.out[b * 3 + 0] = o[0];
      p.out[b * 3 + 1] = o[1];
      p.out[b * 3 + 2] = o[2];
    }
  }
  wait_vm0();
}

// ------------------------------------------------------------------ fused point queries
// sigma (and the canonical position) of free points: the whole of forward_nof + embed + pad +
// NeRF(sigma_only) that trainer_moco_flow.py:146-187 / 500-526 (visualize_mesh lattice, SMPL-point
// losses) spell with five module calls and three padded temporaries per 10 000-point chunk, as one
// launch over all points: xyz -> [bw NoF(ind)] -> encode in registers -> NeRF trunk -> sigma.
struct PointsParams {
  NetDev nerf, nof;
  EmbParams exyz, nxyz, nind;
  const float* xyz;        // (B,3)
  const float* ind;        // (B,) per-point image index, or null -> ind_scalar
  float ind_scalar;
  long long B;
  float* sigma;            // (B,)  raw sigma (no activation)
  float* canon;            // (B,3) or null: the point after the backward flow
  uint32_t ring_off, buf_bytes;
};

template <bool NOF>
__global__ __launch_bounds__(kThreads, 2) void points_kernel(PointsParams p) {
  const LaneId id;
  load_resident(p.nerf, id);
  if (NOF) load_resident(p.nof, id);
  Stream st;
  CarryT<kPD> carry;
  st.open(p.ring_off, p.buf_bytes);
  const NextLayer prog_first = NOF ? follow_of(p.nof) : follow_of(p.nerf);
  if (NOF) start_program(p.nof, st, carry, id);
  else start_program(p.nerf, st, carry, id);
  const long long ntiles = (p.B + kTile - 1) / kTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long b = tile * kTile + id.wave * kWaveSamples + id.j;
    const bool valid = b < p.B;
    const long long bb = valid ? b : p.B - 1;
    float x[3] = {p.xyz[bb * 3 + 0], p.xyz[bb * 3 + 1], p.xyz[bb * 3 + 2]};
    if (NOF) {
      const float ind = p.ind ? p.ind[bb] : p.ind_scalar;
      float emb[kStepsNofIn], out[3];
      nof_embed(emb, x, ind, p.nxyz, p.nind, id.g);
      nof_eval<>(p.nof, emb, x, st, carry, id, follow_of(p.nerf), out);
      x[0] = out[0]; x[1] = out[1]; x[2] = out[2];
      if (valid && id.g == 0 && p.canon) {
        p.canon[b * 3 + 0] = x[0]; p.canon[b * 3 + 1] = x[1]; p.canon[b * 3 + 2] = x[2];
      }
    }
    float embx[kStepsNerfXyz], ext[kStepsExtraMax];
    emb_eval<3, 10>(embx, x, p.exyz, id.g);
#pragma unroll
    for (int e = BlkXyz10::SLOTS; e < kStepsNerfXyz; ++e) embx[e] = 0.f;
#pragma unroll
    for (int e = 0; e < kStepsExtraMax; ++e) ext[e] = 0.f;
    float sigma, rgb[3];
    nerf_eval<16>(p.nerf, embx, ext, true, st, carry, id, prog_first, sigma, rgb);
    if (valid && id.g == 0) p.sigma[b] = sigma;
  }
  wait_vm0();
}

// ------------------------------------------------------------------ fused point radiance query
// The whole of NeRF.forward on free points -- what colouring a mesh vertex or filling an RGBA lattice spells as NoF ->
// Embedding -> zero-pad -> Embedding of the extra block -> NeRF.forward with padded (B, 63 + extra) temporaries -- as one
// launch: xyz -> [bw NoF(ind)] -> encode in registers -> NeRF trunk -> sigma head, xyz_encoding_final, extra_encoding over
// the extra block embedded in registers (nerf_inference, rendering.py:133-142: the view direction as given, or the image
// index), rgb sigmoid.  A sibling of points_kernel (same persistent tile loop), so that kernel's code stays what it was.
struct RadianceParams {
  NetDev nerf, nof;
  float emb_par[4][32];    // [nerf xyz, nerf extra, nof xyz, nof ind] x (freq[16], weight[16]) -> LDS at par_off as in the render
  uint32_t par_off;        // pass (emb_eval_lds): read from the kernarg, four tables cost the NoF variant 16 bytes of scratch
  int extra_type;          // MF_EXTRA_*
  const float* xyz;        // (B,3)
  const float* dirs;       // (B,3) view directions (MF_EXTRA_DIR)
  const float* ind;        // (B,) per-point image index, or null -> ind_scalar
  float ind_scalar;
  long long B;
  float* out;              // (B,4) [rgb | raw sigma]: the columns of NeRF.forward (nerf.py:101)
  float* canon;            // (B,3) or null: the point after the backward flow
  uint32_t ring_off, buf_bytes;
};

template <bool NOF>
__global__ __launch_bounds__(kThreads, 2) void radiance_kernel(RadianceParams p) {
  const LaneId id;
  load_resident(p.nerf, id);
  if (NOF) load_resident(p.nof, id);
  emb_tables_to_lds(p);
  const uint32_t par_nerf_xyz = p.par_off, par_nerf_ext = p.par_off + 128, par_nof_xyz = p.par_off + 256,
                 par_nof_ind = p.par_off + 384;
  Stream st;
  CarryT<kPD> carry;
  st.open(p.ring_off, p.buf_bytes);
  const NextLayer prog_first = NOF ? follow_of(p.nof) : follow_of(p.nerf);
  if (NOF) start_program(p.nof, st, carry, id);
  else start_program(p.nerf, st, carry, id);
  const long long ntiles = (p.B + kTile - 1) / kTile;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // (the point index is rebuilt from an opaque lane index at each use, as in nerf_forward_kernel: neither it nor the
    //  64-bit addresses formed from it are carried across the MFMA sections)
    auto where = [&](bool& valid) {
      int jo = id.j;
      asm volatile("" : "+v"(jo));
      const long long b = tile * kTile + id.wave * kWaveSamples + jo;
      valid = b < p.B;
      return valid ? b : p.B - 1;
    };
    bool valid;
    long long bb = where(valid);
    float x[3] = {p.xyz[bb * 3 + 0], p.xyz[bb * 3 + 1], p.xyz[bb * 3 + 2]};
    if (NOF) {
      const float ind = p.ind ? p.ind[bb] : p.ind_scalar;
      float emb[kStepsNofIn], out[3];
      nof_embed_lds(emb, x, ind, par_nof_xyz, par_nof_ind, id.g);
      nof_eval<>(p.nof, emb, x, st, carry, id, follow_of(p.nerf), out);
      x[0] = out[0]; x[1] = out[1]; x[2] = out[2];
      bb = where(valid);
      if (valid && id.g == 0 && p.canon) {
        p.canon[bb * 3 + 0] = x[0]; p.canon[bb * 3 + 1] = x[1]; p.canon[bb * 3 + 2] = x[2];
      }
    }
    float embx[kStepsNerfXyz], ext[kStepsExtraMax];
    emb_eval_lds<3, 10>(embx, x, par_nerf_xyz, id.g);
#pragma unroll
    for (int e = BlkXyz10::SLOTS; e < kStepsNerfXyz; ++e) embx[e] = 0.f;
#pragma unroll
    for (int e = 0; e < kStepsExtraMax; ++e) ext[e] = 0.f;
    if (p.extra_type == MF_EXTRA_DIR) {
      const float dd[3] = {p.dirs[bb * 3 + 0], p.dirs[bb * 3 + 1], p.dirs[bb * 3 + 2]};
      emb_eval_lds<3, 4>(ext, dd, par_nerf_ext, id.g);                                        // rendering.py:138-142
    } else if (p.extra_type == MF_EXTRA_IND) {
      const float iv[1] = {p.ind ? p.ind[bb] : p.ind_scalar};
      emb_eval_lds<1, 2>(ext, iv, par_nerf_ext, id.g);                                        // rendering.py:133-137
    }
    float sigma, rgb[3] = {0.f, 0.f, 0.f};
    nerf_eval<16>(p.nerf, embx, ext, false, st, carry, id, prog_first, sigma, rgb);
    bb = where(valid);
    if (valid && id.g == 0) *reinterpret_cast<float4*>(p.out + bb * 4) = make_float4(rgb[0], rgb[1], rgb[2], sigma);
  }
  wait_vm0();
}

int device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return cus;
}

}  // namespace mf

using namespace mf;

static int32_t embedding_forward(const char* who, const mf_embedding* e, const float* x, int64_t B, int32_t repeat,
                                 float* out, int64_t out_stride, void* stream) {
  if (!e || (B > 0 && (!x || !out))) return fail(MF_E_INVALID, "%s: null argument", who);
  if (e->in_channels < 1 || e->n_freqs < 0 || e->n_freqs > MF_MAX_FREQS)
    return fail(MF_E_INVALID, "%s: in_channels=%d n_freqs=%d out of range", who, e->in_channels, e->n_freqs);
  const long long width = (long long)e->in_channels * (2 * e->n_freqs + 1);
  if (out_stride <= 0) out_stride = width;
  if (B < 0 || repeat < 1 || out_stride < width)
    return fail(MF_E_INVALID, "%s: B=%lld repeat=%d out_stride=%lld (embedding width %lld)", who, (long long)B, repeat,
                (long long)out_stride, width);
  if (B == 0) return MF_OK;
  EmbFwdParams p{*e, x, out, B, out_stride, repeat};
  const long long total = B * (e->in_channels * (1 + e->n_freqs) + (out_stride - width));
  hipLaunchKernelGGL(embedding_forward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), p);
  return check_launch(who);
}

extern "C" int32_t mf_embedding_forward(const mf_embedding* e, const float* x, int64_t B, float* out, void* stream) {
  return embedding_forward("mf_embedding_forward", e, x, B, 1, out, 0, stream);
}

extern "C" int32_t mf_embedding_forward_rows(const mf_embedding* e, const float* x, int64_t B, int32_t repeat, float* out,
                                             int64_t out_stride, void* stream) {
  return embedding_forward("mf_embedding_forward_rows", e, x, B, repeat, out, out_stride, stream);
}

static int32_t nerf_forward_launch(const char* who, const mf_nerf_desc* d, const void* packed, const float* inputs, int64_t in_stride,
                                   int64_t B, int32_t sigma_only, float* out, float* dump, int64_t dump_stride, void* stream) {
  if (!d || !packed || (B > 0 && (!inputs || !out))) return fail(MF_E_INVALID, "%s: null argument", who);
  NerfFwdParams p{};
  if (!nerf_layout(*d, p.net.L)) return fail(MF_E_UNSUPPORTED, "%s: unsupported NeRF configuration", who);
  if (p.net.L.NK != 16) return fail(MF_E_UNSUPPORTED, "%s: only W=256 is built", who);
  if (dump && dump_stride < (int64_t)p.net.L.n_trunk * p.net.L.W + p.net.L.W / 2)
    return fail(MF_E_INVALID, "%s: dump_stride %lld too small", who, (long long)dump_stride);
  if (B == 0) return MF_OK;
  LdsPlan plan;
  plan.place(p.net, packed);
  p.in = inputs; p.in_stride = in_stride; p.B = B; p.sigma_only = sigma_only; p.out = out;
  p.dump = dump; p.dump_stride = dump_stride;
  p.extra_kind = d->extra_feat_type == MF_EXTRA_DIR ? kEmbDir : (d->extra_feat_type == MF_EXTRA_IND ? kEmbInd : kEmbNone);
  p.extra_cols = d->extra_feat_type == MF_EXTRA_NONE ? 0 : d->extra_feat_dim;
  p.xyz_cols = d->in_channels_xyz;
  plan.ring(p.ring_off, p.buf_bytes);
  void (*kern)(NerfFwdParams) = dump ? nerf_forward_kernel<true> : nerf_forward_kernel<false>;
  return launch_lds(kern, persistent_grid((B + kTile - 1) / kTile), kThreads, plan.lds, static_cast<hipStream_t>(stream), p, who, who);
}

extern "C" int32_t mf_nerf_forward(const mf_nerf_desc* d, const void* packed, const float* inputs, int64_t in_stride,
                                   int64_t B, int32_t sigma_only, float* out, void* stream) {
  return nerf_forward_launch("mf_nerf_forward", d, packed, inputs, in_stride, B, sigma_only, out, nullptr, 0, stream);
}

extern "C" int32_t mf_nerf_forward_dump(const mf_nerf_desc* d, const void* packed, const float* inputs, int64_t in_stride,
                                        int64_t B, float* out, float* dump_acts, int64_t dump_stride, void* stream) {
  if (B > 0 && !dump_acts) return fail(MF_E_INVALID, "mf_nerf_forward_dump: null dump buffer");
  return nerf_forward_launch("mf_nerf_forward_dump", d, packed, inputs, in_stride, B, 0, out, dump_acts, dump_stride, stream);
}

extern "C" int32_t mf_nof_forward(const mf_nof_desc* d, const void* packed, const float* inputs, int64_t in_stride,
                                  const float* xyz, int64_t B, float* out, void* stream) {
  if (!d || !packed || (B > 0 && (!inputs || !xyz || !out))) return fail(MF_E_INVALID, "mf_nof_forward: null argument");
  NofFwdParams p{};
  if (!nof_layout(*d, p.net.L, 0, true)) return fail(MF_E_UNSUPPORTED, "mf_nof_forward: unsupported NoF configuration");
  if (B == 0) return MF_OK;
  LdsPlan plan;
  plan.place(p.net, packed);
  p.in = inputs; p.in_stride = in_stride; p.B = B; p.xyz = xyz; p.out = out;
  p.xyz_cols = d->in_channels_xyz; p.in_cols = d->in_channels_xyz + d->extra_feat_dim;
  plan.ring(p.ring_off, p.buf_bytes);
  void (*kern)(NofFwdParams) = p.net.L.NK == 16 ? nof_forward_kernel<16> : nof_forward_kernel<8>;     // W = 256: the bare NoF() default
  return launch_lds(kern, persistent_grid((B + kTile - 1) / kTile), kThreads, plan.lds, static_cast<hipStream_t>(stream), p, "mf_nof_forward", "mf_nof_forward");
}

namespace mf {
int points_sigma_bf16(int prec, const mf_nerf_desc* nerf, const void* nerf_packed, const mf_embedding* emb_xyz, const mf_nof_desc* nof,
                      const void* nof_packed, const mf_embedding* nof_emb_xyz, const mf_embedding* nof_emb_ind, const float* xyz,
                      const float* ind, float ind_scalar, int64_t B, float* sigma, float* canon, void* workspace,
                      int64_t workspace_bytes, hipStream_t st);   // mf_render_bf16.hip
int64_t points_workspace_bytes_bf16(const mf_nof_desc* nof, int per_point_ind, int64_t B);
}

extern "C" int64_t mf_points_sigma_workspace_bytes(int32_t precision, const mf_nof_desc* nof, int32_t per_point_ind, int64_t B) {
  return precision != MF_PREC_F32 ? points_workspace_bytes_bf16(nof, per_point_ind, B) : 0;
}

extern "C" int32_t mf_points_sigma(const mf_nerf_desc* nerf, const void* nerf_packed, const mf_embedding* emb_xyz,
                                   const mf_nof_desc* nof, const void* nof_packed, const mf_embedding* nof_emb_xyz,
                                   const mf_embedding* nof_emb_ind, const float* xyz, const float* ind,
                                   float ind_scalar, int64_t B, float* sigma, float* canon, void* stream) {
  return mf_points_sigma_p(MF_PREC_F32, nerf, nerf_packed, emb_xyz, nof, nof_packed, nof_emb_xyz, nof_emb_ind, xyz, ind, ind_scalar, B,
                           sigma, canon, nullptr, 0, stream);
}

extern "C" int32_t mf_points_sigma_p(int32_t precision, const mf_nerf_desc* nerf, const void* nerf_packed, const mf_embedding* emb_xyz,
                                     const mf_nof_desc* nof, const void* nof_packed, const mf_embedding* nof_emb_xyz,
                                     const mf_embedding* nof_emb_ind, const float* xyz, const float* ind,
                                     float ind_scalar, int64_t B, float* sigma, float* canon, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  if (!nerf || !nerf_packed || !emb_xyz || (B > 0 && (!xyz || !sigma)))
    return fail(MF_E_INVALID, "mf_points_sigma: null argument");
  if (precision < MF_PREC_F32 || precision > MF_PREC_BF16X3) return fail(MF_E_INVALID, "mf_points_sigma: precision %d", precision);
  if (int e = check_xyz_embedding("mf_points_sigma", *emb_xyz, 10)) return e;
  if (nof) {
    if (!nof_packed || !nof_emb_xyz || !nof_emb_ind) return fail(MF_E_INVALID, "mf_points_sigma: NoF arguments missing");
    if (int e = check_nof_embeddings("mf_points_sigma", *nof_emb_xyz, *nof_emb_ind)) return e;
  }
  if (precision != MF_PREC_F32) {
    if (B == 0) return MF_OK;
    return points_sigma_bf16(precision, nerf, nerf_packed, emb_xyz, nof, nof_packed, nof_emb_xyz, nof_emb_ind, xyz, ind, ind_scalar, B, sigma, canon,
                             workspace, workspace_bytes, static_cast<hipStream_t>(stream));
  }
  PointsParams p{};
  if (!nerf_layout(*nerf, p.nerf.L) || p.nerf.L.NK != 16)
    return fail(MF_E_UNSUPPORTED, "mf_points_sigma: unsupported NeRF configuration");
  if (B == 0) return MF_OK;
  LdsPlan plan;
  plan.place(p.nerf, nerf_packed);
  emb_table(*emb_xyz, p.exyz.freq, p.exyz.weight);
  if (nof) {
    if (!nof_layout(*nof, p.nof.L)) return fail(MF_E_UNSUPPORTED, "mf_points_sigma: unsupported NoF configuration");
    plan.place(p.nof, nof_packed);
    emb_table(*nof_emb_xyz, p.nxyz.freq, p.nxyz.weight);
    emb_table(*nof_emb_ind, p.nind.freq, p.nind.weight);
  }
  p.xyz = xyz; p.ind = ind; p.ind_scalar = ind_scalar; p.B = B; p.sigma = sigma; p.canon = canon;
  plan.ring(p.ring_off, p.buf_bytes);
  void (*kern)(PointsParams) = nof ? points_kernel<true> : points_kernel<false>;
  return launch_lds(kern, persistent_grid((B + kTile - 1) / kTile), kThreads, plan.lds, static_cast<hipStream_t>(stream), p, "mf_points_sigma", "mf_points_sigma");
}

extern "C" int32_t mf_points_radiance(const mf_nerf_desc* nerf, const void* nerf_packed, const mf_embedding* emb_xyz,
                                      const mf_embedding* emb_extra, const mf_nof_desc* nof, const void* nof_packed,
                                      const mf_embedding* nof_emb_xyz, const mf_embedding* nof_emb_ind, const float* xyz,
                                      const float* view_dirs, const float* ind, float ind_scalar, int64_t B, float* out,
                                      float* canon, void* stream) {
  if (!nerf || !nerf_packed || !emb_xyz || (B > 0 && (!xyz || !out)))
    return fail(MF_E_INVALID, "mf_points_radiance: null argument");
  if (B < 0) return fail(MF_E_INVALID, "mf_points_radiance: B=%lld", (long long)B);
  if (!is_aligned(out, 16)) return fail(MF_E_INVALID, "mf_points_radiance: out must be 16-byte aligned");
  RadianceParams p{};
  if (!nerf_layout(*nerf, p.nerf.L) || p.nerf.L.NK != 16)
    return fail(MF_E_UNSUPPORTED, "mf_points_radiance: unsupported NeRF configuration");
  if (int e = check_xyz_embedding("mf_points_radiance", *emb_xyz, 10)) return e;
  p.extra_type = nerf->extra_feat_type;
  // (the extra block's check stays here: MF_E_INVALID and n_freqs < 0 a fault, unlike the render pass's -- mf_plan.hpp)
  if (p.extra_type == MF_EXTRA_DIR) {
    if (!emb_extra || (B > 0 && !view_dirs)) return fail(MF_E_INVALID, "mf_points_radiance: a \"dir\" NeRF needs emb_extra and view_dirs");
    if (emb_extra->in_channels != 3 || emb_extra->n_freqs < 0 || emb_extra->n_freqs > 4 ||
        3 * (2 * emb_extra->n_freqs + 1) > nerf->extra_feat_dim)
      return fail(MF_E_INVALID, "mf_points_radiance: dir embedding must have 3 channels, <= 4 frequencies and fit extra_feat_dim");
  } else if (p.extra_type == MF_EXTRA_IND) {
    if (!emb_extra) return fail(MF_E_INVALID, "mf_points_radiance: an \"ind\" NeRF needs emb_extra");
    if (emb_extra->in_channels != 1 || emb_extra->n_freqs < 0 || emb_extra->n_freqs > 2 ||
        (2 * emb_extra->n_freqs + 1) > nerf->extra_feat_dim)
      return fail(MF_E_INVALID, "mf_points_radiance: ind embedding must have 1 channel, <= 2 frequencies and fit extra_feat_dim");
  }
  LdsPlan plan;
  plan.place(p.nerf, nerf_packed);
  emb_table(*emb_xyz, p.emb_par[0], p.emb_par[0] + 16);
  if (p.extra_type != MF_EXTRA_NONE) emb_table(*emb_extra, p.emb_par[1], p.emb_par[1] + 16);
  if (nof) {
    if (!nof_packed || !nof_emb_xyz || !nof_emb_ind) return fail(MF_E_INVALID, "mf_points_radiance: NoF arguments missing");
    if (!nof_layout(*nof, p.nof.L)) return fail(MF_E_UNSUPPORTED, "mf_points_radiance: unsupported NoF configuration");
    if (int e = check_nof_embeddings("mf_points_radiance", *nof_emb_xyz, *nof_emb_ind)) return e;
    plan.place(p.nof, nof_packed);
    emb_table(*nof_emb_xyz, p.emb_par[2], p.emb_par[2] + 16);
    emb_table(*nof_emb_ind, p.emb_par[3], p.emb_par[3] + 16);
  }
  if (B == 0) return MF_OK;
  p.par_off = plan.place_tables();
  p.xyz = xyz; p.dirs = view_dirs; p.ind = ind; p.ind_scalar = ind_scalar; p.B = B; p.out = out; p.canon = nof ? canon : nullptr;
  plan.ring(p.ring_off, p.buf_bytes);
  void (*kern)(RadianceParams) = nof ? radiance_kernel<true> : radiance_kernel<false>;
  return launch_lds(kern, persistent_grid((B + kTile - 1) / kTile), kThreads, plan.lds, static_cast<hipStream_t>(stream), p, "mf_points_radiance",
                    "mf_points_radiance");
}
