// mf_pack.hip -- re-order nn.Linear parameters into the MFMA fragment streams.
//
// Replaces nothing in the reference (it keeps (out,in) row-major tensors and calls addmm,
// models/nerf.py:84-99, models/nof.py:70-75); this is the layout transform the fused kernels
// need.  It is a pure permutation + zero padding: every packed float is either one source
// weight or 0 -- with ONE exception, the folded fp32 stream (mf_nerf_pack_fold): its extra_encoding
// panels hold W' = W_e[:, :W] W_f and its extra bias b' = b_e + W_e[:, :W] b_f, which fold_final_kernel
// computes in front of the pack (float64 sums in ascending k, rounded once); the extra block's columns W_e[:, W:] are not in
// that stream's panels but behind them in natural order, for the folded kernels' per-ray bias.  One kernel writes every stream from a region list (PackJob, mf_layout.hpp):
// the forward's here, each backward chain's -- the same layout of W^T -- next to the kernel
// that reads it (mf_backward.hip, mf_nofgrad.hip, mf_backward_bf16.hip, mf_nofgrad_bf16.hip).
#include <hip/hip_fp16.h>
#include "mf_host.hpp"
#include "mf_layout.hpp"

namespace mf {

__device__ inline unsigned short bf16_rne(float x) {        // round to nearest even (inf / nan pass through)
  const unsigned u = __float_as_uint(x);
  const unsigned rnd = u + 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(((u & 0x7f800000u) == 0x7f800000u ? u : rnd) >> 16);
}

__device__ inline float resident_value(const ResCopy* c, int n, int idx) {
  float v = 0.f;
  for (int k = 0; k < n; ++k) {
    const int o = idx - c[k].dst_off;
    if (o >= 0 && o < c[k].n) v = c[k].src[o] * c[k].scale;
  }
  return v;
}

__device__ inline float block_at(const PackBlock& B, int n, int c) {      // element (n, c) of the block's matrix, 0 past its columns
  return (c >= 0 && c < B.cols) ? B.src[(long long)n * B.s_n + (long long)c * B.s_k] : 0.f;
}

// one float4 slot per thread; the first res_floats threads also write the resident block
__global__ void pack_panels_kernel(PackJob job) {
  const long long gidx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gidx < job.res_floats) job.resident[gidx] = resident_value(job.res, job.n_res, (int)gidx);
  // a group is one wave's 64 slots (blockDim: a multiple of 64), so all that depends on the group alone is wave-uniform
  const long long grp = ((long long)blockIdx.x * blockDim.x + __builtin_amdgcn_readfirstlane(threadIdx.x)) >> 6;
  if (grp >= job.total_groups) return;
  const int lane = (int)(gidx & 63);
  int ri = 0;
  while (ri + 1 < job.n_regions && grp >= job.reg[ri + 1].dst_group0) ++ri;
  const PackRegion& R = job.reg[ri];
  const long long local = grp - R.dst_group0;
  const int P = (int)(local / R.groups), gi = (int)(local % R.groups);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float* pv = &v.x;
  if (job.bf16) {
    // embedded k-step ks: 1: bf16(w); 2: + lo = bf16(w - hi); 3: hi, mid, lo; hidden k-step ks covers features
    // 16 ks + hid_perm2(h, e)
    const int i = lane & 31, h = lane >> 5;
    int srow = 32 * P + i, rterm = 0;
    bool zero_row = R.n_rows && srow >= R.n_rows;
    if (R.row_terms) {                                       // (hi rows at 0 .., lo rows at 8 ..: both in lane half 0's accumulators)
      zero_row = !(srow < R.n_rows || (srow >= R.row_terms && srow < R.row_terms + R.n_rows));
      if (srow >= R.row_terms) { rterm = 1; srow -= R.row_terms; }
    }
    const int g0 = R.blk[0].split * R.blk[0].steps;
    const PackBlock B = gi < g0 ? R.blk[0] : R.blk[1];      // (both loaded, then selected: no dependent load)
    const int gb = gi < g0 ? gi : gi - g0;
    unsigned short h8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // term t of a weight: t = 0: bf16(w); 1: bf16(w - hi); 2: bf16(w - hi - mid)   (exact fp32 subtractions)
    const bool half = job.half != 0;
    const float ws = job.wscale;
    bool sat = false;
    auto term = [half, ws, &sat](float w, int t) {
      if (half) {                                           // hi = half(ws w) (saturated: no inf in the stream), lo = half(ws w - hi)
        // |ws w| beyond the half range (|w| >= 2047 at ws = 2^5: no trained NoF is near it) cannot be represented: the weight is
        // saturated AND the network's poison slots are set (job.poison, below) -- every point the network evaluates then comes out
        // NaN.  Round 5 saturated silently: finite WRONG results with no diagnostic; a host-side check would cost a
        // device sync at every re-pack, i.e. at every optimizer step.
        w = w * ws;
        if (!(fabsf(w) <= 65504.f)) sat = true;
        w = fminf(fmaxf(w, -65504.f), 65504.f);
        __half hb = __float2half_rn(w);
        if (t > 0) hb = __float2half_rn(w - __half2float(hb));
        return __half_as_ushort(hb);
      }
      unsigned short b = bf16_rne(w);
      for (int k = 0; k < t; ++k) {
        w -= __uint_as_float((unsigned)b << 16);
        b = bf16_rne(w);
      }
      return b;
    };
    if (!zero_row && gb < B.split * B.steps) {
      const int ks = gb / B.split, t = R.row_terms ? rterm : gb % B.split;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = B.kind == kPackHidden ? 16 * ks + hid_perm2(h, e) : emb_feature2(B.kind, h, 8 * ks + e, job.xyz_cols);
        h8[e] = term(block_at(B, srow, c), t);
      }
    }
    unsigned* pu = reinterpret_cast<unsigned*>(&v.x);
    for (int w = 0; w < 4; ++w) pu[w] = (unsigned)h8[2 * w] | ((unsigned)h8[2 * w + 1] << 16);
    reinterpret_cast<float4*>(job.panels)[gidx] = v;
    // poison: rows 27 / 31 of the head's 32-row bias vector (the two lane halves' last junk rows: zero weight rows, so their
    // accumulators ARE this value) -- nof_eval_x3 adds that accumulator to every output point: + 0 or + NaN
    if (sat && job.poison) { job.poison[0] = __int_as_float(0x7fc00000); job.poison[4] = __int_as_float(0x7fc00000); }
    return;
  }
  const int b = gi >> 1, half = gi & 1;                 // k-quad within the panel, tile half
  const int i = lane & 15, g = lane >> 4;
  const int n = 32 * P + 16 * half + i;
  const PackBlock B = b < R.blk[0].steps ? R.blk[0] : R.blk[1];
  const int q = b < R.blk[0].steps ? b : b - R.blk[0].steps;
  if (!(R.n_rows && n >= R.n_rows) && q < B.steps)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      pv[r] = block_at(B, n, B.kind == kPackHidden ? 16 * q + 4 * g + r : emb_feature(B.kind, g, 4 * q + r, job.xyz_cols));
  reinterpret_cast<float4*>(job.panels)[gidx] = v;
}

// the forward's resident block (biases, heads: up to 2 MF_MAX_LAYERS + 8 copies) -- a launch of its own in front of the panels,
// whose poison slots it zero-fills
struct ResJob { ResCopy c[2 * MF_MAX_LAYERS + 8]; int n; float* res; int total; };

__global__ void pack_resident_kernel(ResJob job) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= job.total) return;
  job.res[idx] = resident_value(job.c, job.n, idx);
}

// bf16 NoF: the fp32 image-index columns of the layers that consume the embedded input, TRANSPOSED:
// [embedded layer][column (kNofIndCols)][row] -- what nof_raybias_kernel contracts with emb(ind) once per ray, one thread
// per row reading its column entries coalesced
struct IndJob { const float* W[MF_MAX_LAYERS]; int n_in[MF_MAX_LAYERS]; int n_layers, rows, col0, cols; float* dst; float scale; };

__global__ void pack_ind_kernel(IndJob job) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int per_layer = job.rows * kNofIndCols;
  if (idx >= job.n_layers * per_layer) return;
  const int e = idx / per_layer, r = (idx % per_layer) / kNofIndCols, c = idx % kNofIndCols;
  job.dst[(e * kNofIndCols + c) * job.rows + r] = c < job.cols ? job.scale * job.W[e][(long long)r * job.n_in[e] + job.col0 + c] : 0.f;
}

// The fold of xyz_encoding_final into extra_encoding (mf_layout.hpp, FoldLayout): thread (n, k) writes
// Wp[n][k] = sum_j We[n][j] Wf[j][k], the first W / 2 threads also bp[n] = be[n] + sum_j We[n][j] bf[j].  Every product of two
// floats is exact in float64; the sums run over j ascending in float64 and are rounded to fp32 once.  No atomics: two packs of
// the same weights are bit-identical.
// The first (W / 2) * xcols threads also copy the extra block's columns: Wx[n][c] = We[n][W + c], 0 past the block's `ext` columns
// (FoldLayout::off_x: what the folded kernels' per-ray bias phase reads).
struct FoldJob { const float *We, *Wf, *be, *bf; int W, ld_e; float *Wp, *bp; float* Wx; int xcols, ext; };

__global__ void fold_final_kernel(FoldJob job) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = job.W / 2;
  if (idx >= half * job.W) return;
  if (idx < half * job.xcols) {
    const int n = idx / job.xcols, c = idx % job.xcols;
    job.Wx[idx] = c < job.ext ? job.We[(long long)n * job.ld_e + job.W + c] : 0.f;
  }
  const int n = idx / job.W, k = idx % job.W;
  const float* we = job.We + (long long)n * job.ld_e;
  double acc = 0.0;
  for (int j = 0; j < job.W; ++j) acc += (double)we[j] * (double)job.Wf[(long long)j * job.W + k];
  job.Wp[idx] = (float)acc;
  if (idx < half) {
    const float* wb = job.We + (long long)idx * job.ld_e;
    double b = 0.0;
#ifndef MF_FOLD_BREAK_BIAS   // (-DMF_FOLD_BREAK_BIAS: the deliberately broken build the float64 test of the fold must reject: W_e b_f dropped)
    for (int j = 0; j < job.W; ++j) b += (double)wb[j] * (double)job.bf[j];
#endif
    job.bp[idx] = (float)((double)job.be[idx] + b);
  }
}

int launch_pack(const PackJob& job, hipStream_t st, const char* what) {
  const long long slots = job.total_groups * 64 > job.res_floats ? job.total_groups * 64 : job.res_floats;
  hipLaunchKernelGGL(pack_panels_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, job);
  return check_launch(what);
}

static int launch_pack(const PackJob& job, const ResJob& rj, hipStream_t st) {
  hipLaunchKernelGGL(pack_resident_kernel, dim3((rj.total + 255) / 256), dim3(256), 0, st, rj);
  return launch_pack(job, st, "mf_pack");
}

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_nerf_packed_bytes_p(const mf_nerf_desc* d, int32_t precision) {
  NetLayout L;
  if (!d || (precision < MF_PREC_F32 || precision > MF_PREC_BF16X3) || !nerf_layout(*d, L, precision)) { fail(MF_E_UNSUPPORTED, "mf_nerf_packed_bytes: unsupported NeRF configuration"); return 0; }
  return L.res_bytes + L.panel_bytes;
}

extern "C" int64_t mf_nof_packed_bytes_p(const mf_nof_desc* d, int32_t precision) {
  NetLayout L;
  if (!d || (precision < MF_PREC_F32 || precision > MF_PREC_BF16X3) || !nof_layout(*d, L, precision, precision == MF_PREC_F32)) { fail(MF_E_UNSUPPORTED, "mf_nof_packed_bytes: unsupported NoF configuration"); return 0; }
  return L.res_bytes + L.panel_bytes + L.ind_bytes;
}

// fold (fp32): the folded stream of mf_nerf_pack_fold -- no panels and no bias for xyz_encoding_final, extra_encoding's hidden
// block and bias from the scratch area behind the panels, which fold_final_kernel fills first
static int32_t nerf_pack(const mf_nerf_desc* d, int32_t precision, void* packed, void* stream, bool fold) {
  NetLayout L;
  FoldLayout F{};
  if (!d || !packed) return fail(MF_E_INVALID, "mf_nerf_pack: null argument");
  if (precision < MF_PREC_F32 || precision > MF_PREC_BF16X3) return fail(MF_E_INVALID, "mf_nerf_pack: precision %d", precision);
  if (fold ? !nerf_fold_layout(*d, L, F) : !nerf_layout(*d, L, precision))
    return fail(MF_E_UNSUPPORTED, "mf_nerf_pack: unsupported NeRF configuration "
                                       "(W=%d D=%d in_channels_xyz=%d)", d->W, d->D, d->in_channels_xyz);
  const int64_t panel_bytes = fold ? F.panel_bytes : L.panel_bytes;
  float* const fold_w = fold ? reinterpret_cast<float*>(static_cast<char*>(packed) + F.off_w) : nullptr;
  float* const fold_b = fold ? reinterpret_cast<float*>(static_cast<char*>(packed) + F.off_b) : nullptr;
  PackJob job{};
  ResJob rj{};
  // fp32: embedded blocks in k-quads; bf16: 16-k steps, split into L.terms groups with emb_split
  const int esplit = L.emb_split ? L.terms : 1, equad = L.bf16 ? 1 : 4;
  auto head_region = [&](const float* W, int rows, int groups) {       // NetLayout::head_tiles: one 32-row tile, (hi, lo) ROW pairs
    PackRegion& R = job.add(1, groups, PackBlock{W, groups * 16, 1, kPackHidden, groups, 1, groups * 16});
    R.n_rows = rows;
    R.row_terms = 8;
  };
  for (int l = 0; l < L.n_trunk; ++l) {
    if (l == L.n_trunk - 1 && L.head_tiles) {
      if (!d->sigma_w) return fail(MF_E_INVALID, "mf_nerf_pack: missing sigma weight");
      head_region(d->sigma_w, 1, nerf_sigma_groups(L));
    }
    const bool has_emb = (L.emb_mask >> l) & 1;
    const float* W = l < d->D ? d->trunk_w[l] : d->final_w;
    if (!W) return fail(MF_E_INVALID, "mf_nerf_pack: missing weight pointer for layer %d", l);
    if (fold && l == d->D) continue;
    const int hid0 = has_emb ? d->in_channels_xyz : 0, n_in = hid0 + (l > 0 ? L.W : 0);
    job.add(L.NP, trunk_groups(L, l),
            PackBlock{W, n_in, 1, kEmbNerfXyz, has_emb ? L.emb_steps / equad : 0, esplit, d->in_channels_xyz},
            PackBlock{W + hid0, n_in, 1, kPackHidden, l > 0 ? hidden_batches(L) : 0, ((L.hsplit_mask >> l) & 1) ? L.terms : 1, L.W});
    const float* b = l < d->D ? d->trunk_b[l] : d->final_b;
    rj.c[rj.n++] = ResCopy{b, L.off_bias_trunk + l * L.W, L.W};
  }
  {
    const int ext = d->extra_feat_type == MF_EXTRA_NONE ? 0 : d->extra_feat_dim;
    const float* W = d->extra_w;
    if (!W) return fail(MF_E_INVALID, "mf_nerf_pack: missing extra_encoding weight");
    const int kind = d->extra_feat_type == MF_EXTRA_DIR ? kEmbDir : (d->extra_feat_type == MF_EXTRA_IND ? kEmbInd : kEmbNone);
    if (fold) job.add(L.NP / 2, fold_extra_groups(L), PackBlock{fold_w, L.W, 1, kPackHidden, hidden_batches(L), 1, L.W});   // hidden block only
    else job.add(L.NP / 2, extra_groups(L),
                 PackBlock{W, L.W + ext, 1, kPackHidden, hidden_batches(L), ((L.hsplit_mask >> L.n_trunk) & 1) ? L.terms : 1, L.W},
                 PackBlock{W + L.W, L.W + ext, 1, kind, L.extra_steps / equad, esplit, ext});
    if (fold && (!d->extra_b || !d->final_b)) return fail(MF_E_INVALID, "mf_nerf_pack: missing bias pointer of the folded layers");
    rj.c[rj.n++] = ResCopy{fold ? fold_b : d->extra_b, L.off_bias_extra, L.W / 2};
  }
  if (L.head_tiles) {
    if (!d->rgb_w) return fail(MF_E_INVALID, "mf_nerf_pack: missing rgb weight");
    head_region(d->rgb_w, 3, nerf_rgb_groups(L));
  }
  rj.c[rj.n++] = ResCopy{d->sigma_w, L.off_head_w, L.W};
  rj.c[rj.n++] = ResCopy{d->sigma_b, L.off_head_b, 1};
  rj.c[rj.n++] = ResCopy{d->rgb_w, L.off_rgb_w, 3 * (L.W / 2)};
  rj.c[rj.n++] = ResCopy{d->rgb_b, L.off_rgb_b, 3};
  for (int k = 0; k < rj.n; ++k)
    if (!rj.c[k].src) return fail(MF_E_INVALID, "mf_nerf_pack: missing bias/head pointer (%d)", k);
  job.bf16 = L.bf16;
  job.xyz_cols = d->in_channels_xyz;
  job.panels = reinterpret_cast<float*>(static_cast<char*>(packed) + L.res_bytes);
  rj.res = static_cast<float*>(packed);
  rj.total = (int)(L.res_bytes / 4);
  if (job.total_groups * kGroupBytes != panel_bytes) return fail(MF_E_INVALID, "mf_nerf_pack: layout mismatch");
  if (fold) {
    const int ext = d->extra_feat_type == MF_EXTRA_NONE ? 0 : d->extra_feat_dim;
    const FoldJob fj{d->extra_w, d->final_w, d->extra_b, d->final_b, L.W, L.W + ext, fold_w, fold_b,
                     reinterpret_cast<float*>(static_cast<char*>(packed) + F.off_x), fold_ext_cols(L), ext};
    hipLaunchKernelGGL(fold_final_kernel, dim3((L.W / 2) * L.W / 256), dim3(256), 0, static_cast<hipStream_t>(stream), fj);
    if (int e = check_launch("mf_nerf_pack_fold")) return e;
  }
  return launch_pack(job, rj, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mf_nerf_pack_p(const mf_nerf_desc* d, int32_t precision, void* packed, void* stream) {
  return nerf_pack(d, precision, packed, stream, false);
}

extern "C" int64_t mf_nerf_fold_packed_bytes(const mf_nerf_desc* d) {
  NetLayout L;
  FoldLayout F;
  if (!d || !nerf_fold_layout(*d, L, F)) { fail(MF_E_UNSUPPORTED, "mf_nerf_fold_packed_bytes: unsupported NeRF configuration (fp32, W = 256)"); return 0; }
  return L.res_bytes + F.panel_bytes + F.scratch_bytes;
}

extern "C" int32_t mf_nerf_pack_fold(const mf_nerf_desc* d, void* packed, void* stream) {
  return nerf_pack(d, MF_PREC_F32, packed, stream, true);
}

extern "C" int32_t mf_nof_pack_p(const mf_nof_desc* d, int32_t precision, void* packed, void* stream) {
  NetLayout L;
  if (!d || !packed) return fail(MF_E_INVALID, "mf_nof_pack: null argument");
  if (precision < MF_PREC_F32 || precision > MF_PREC_BF16X3) return fail(MF_E_INVALID, "mf_nof_pack: precision %d", precision);
  if (!nof_layout(*d, L, precision, precision == MF_PREC_F32)) return fail(MF_E_UNSUPPORTED, "mf_nof_pack: unsupported NoF configuration "
                                      "(W=%d D=%d in_channels_xyz=%d extra_feat_dim=%d)", d->W, d->D,
                                      d->in_channels_xyz, d->extra_feat_dim);
  PackJob job{};
  ResJob rj{};
  const int cin = d->in_channels_xyz + d->extra_feat_dim;
  // NetLayout::half (the NoF under MF_PREC_BF16X3): weights at 2^kNofHalfSW, biases at the accumulators' 2^(kNofHalfSA + kNofHalfSW)
  const float wscale = L.half ? (float)(1 << kNofHalfSW) : 1.f, bscale = L.half ? (float)(1 << (kNofHalfSA + kNofHalfSW)) : 1.f;
  const int esplit = L.emb_split ? L.terms : 1, equad = L.bf16 ? 1 : 4;
  for (int l = 0; l < L.n_trunk; ++l) {
    const bool has_emb = (L.emb_mask >> l) & 1;
    const float* W = d->trunk_w[l];
    if (!W || !d->trunk_b[l]) return fail(MF_E_INVALID, "mf_nof_pack: missing parameter pointer for layer %d", l);
    const int hid0 = has_emb ? cin : 0, n_in = hid0 + (l > 0 ? L.W : 0);
    job.add(L.NP, trunk_groups(L, l),
            PackBlock{W, n_in, 1, kEmbNofIn, has_emb ? L.emb_steps / equad : 0, esplit, cin},
            PackBlock{W + hid0, n_in, 1, kPackHidden, l > 0 ? hidden_batches(L) : 0, ((L.hsplit_mask >> l) & 1) ? L.terms : 1, L.W});
    rj.c[rj.n++] = ResCopy{d->trunk_b[l], L.off_bias_trunk + l * L.W, L.W, bscale};
  }
  if (!d->head_w || !d->head_b) return fail(MF_E_INVALID, "mf_nof_pack: missing head parameters");
  if (L.bf16) {
    PackRegion& R = job.add(1, head_groups(L), PackBlock{d->head_w, L.W, 1, kPackHidden, L.NK, L.head_tiles ? 1 : L.terms, L.W});
    R.n_rows = L.n_head;
    R.row_terms = L.head_tiles ? 16 : 0;
  }
  rj.c[rj.n++] = ResCopy{d->head_w, L.off_head_w, L.n_head * L.W};
  rj.c[rj.n++] = ResCopy{d->head_b, L.off_head_b, L.n_head, bscale};
  job.bf16 = L.bf16;
  job.xyz_cols = d->in_channels_xyz;
  job.half = L.half;
  job.wscale = wscale;
  job.panels = reinterpret_cast<float*>(static_cast<char*>(packed) + L.res_bytes);
  job.poison = L.half ? static_cast<float*>(packed) + L.off_head_b + 27 : nullptr;       // (the resident kernel zero-fills them first)
  rj.res = static_cast<float*>(packed);
  rj.total = (int)(L.res_bytes / 4);
  if (job.total_groups * kGroupBytes != L.panel_bytes) return fail(MF_E_INVALID, "mf_nof_pack: layout mismatch");
  if (L.bf16) {
    IndJob ij{};
    for (int l = 0; l < L.n_trunk; ++l)
      if ((L.emb_mask >> l) & 1) {
        ij.W[ij.n_layers] = d->trunk_w[l];
        ij.n_in[ij.n_layers] = cin + (l > 0 ? L.W : 0);
        ++ij.n_layers;
      }
    ij.rows = L.W; ij.col0 = d->in_channels_xyz; ij.cols = d->extra_feat_dim;
    ij.scale = bscale;                    // (the per-ray index bias b + W_ind emb(ind) comes out at the accumulators' scale)
    ij.dst = reinterpret_cast<float*>(static_cast<char*>(packed) + L.res_bytes + L.panel_bytes);
    const int total = ij.n_layers * ij.rows * kNofIndCols;
    hipLaunchKernelGGL(pack_ind_kernel, dim3((total + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), ij);
  }
  return launch_pack(job, rj, static_cast<hipStream_t>(stream));
}

extern "C" int64_t mf_nerf_packed_bytes(const mf_nerf_desc* d) { return mf_nerf_packed_bytes_p(d, MF_PREC_F32); }
extern "C" int64_t mf_nof_packed_bytes(const mf_nof_desc* d) { return mf_nof_packed_bytes_p(d, MF_PREC_F32); }
extern "C" int32_t mf_nerf_pack(const mf_nerf_desc* d, void* packed, void* stream) { return mf_nerf_pack_p(d, MF_PREC_F32, packed, stream); }
extern "C" int32_t mf_nof_pack(const mf_nof_desc* d, void* packed, void* stream) { return mf_nof_pack_p(d, MF_PREC_F32, packed, stream); }
