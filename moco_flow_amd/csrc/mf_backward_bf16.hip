// mf_backward_bf16.hip -- the input-gradient chain of the canonical NeRF (mf_backward.hip) in three bf16 products.
//
// Same mathematics as mf_nerf_backward -- per sample, given dL/d[rgb, sigma] and the forward's activation dump,
//     d_o = d_rgb rgb (1 - rgb);  d_e = (W_rgb^T d_o) [e > 0];  d_g = W_e[:, :W]^T d_e;
//     d_z_{D-1} = (W_f^T d_g + w_sigma d_sigma) [h_{D-1} > 0];  d_z_{l-1} = (W_l[:, hidden]^T d_z_l) [h_{l-1} > 0],  l = D-1 .. 1
// with every pre-activation gradient stored in the dump's layout for mf_weight_grads -- on the MF_PREC_BF16X3 core of
// mf_bf16.hpp: the D + 1 W-wide contractions as (hi, lo) bf16 pairs of the gradients AND the transposed weights, three
// products per k-step, fp32 accumulation; 4 waves (one per SIMD), 128 samples per pass over the transposed weight
// stream.  The ReLU masks come from the dump exactly as in the fp32 chain, so no unit changes side: the result differs from
// the fp32 chain's by the 2^-16 of the split operands (measured ~1e-5 max-rel on d z), not by mask flips.
// The layers are bwd_layer_x (mf_bwd3.hpp), shared with the NoF's chain (mf_nofgrad_bf16.hip).
// The gradient of the embedded input (g_emb, ABI v9: the joint stage's NoF training) = W_0[:, :63]^T d_z_0 (+ one skip
// layer: W_skip[:, :63]^T d_z_skip) follows as one or two 64-row layers behind the chain, d_z_skip re-read from the rows
// this lane stored several layers earlier.
#include "mf_bwd3.hpp"
#include "mf_host.hpp"
#include "mf_layout.hpp"
#include "mf_plan.hpp"

namespace mf {

namespace bf {

// packed buffer: [resident: zeros 32 | rgb.0.weight 3 x 128 (natural order) | sigma.weight 256, 1 KiB-aligned]
//                [panels: backward layer 0 = extra_encoding[:, :W]^T (K = 128: 8 tiles x 16 groups),
//                 layers 1 .. D = xyz_encoding_final^T, trunk layers D-1 .. 1 transposed (K = 256: 8 tiles x 32 groups)]
// group (hi | lo of k-step ks): lane (i = lane & 31, h = lane >> 5) holds Wt[32 P + i][16 ks + hid_perm2(h, e)], e = 0..7.
constexpr int kB3Zero = 0, kB3Rgb = 32, kB3Sig = 32 + 384, kB3ResFloats = 32 + 384 + 256;
constexpr int kB3ResBytes = ((kB3ResFloats * 4 + kGroupBytes - 1) / kGroupBytes) * kGroupBytes;
//                 [then, for g_emb: W_0[:, :63]^T and (one skip layer) W_skip[:, :63]^T: 2 tiles x 32 groups each, rows >= 63 zero]
inline long long bwd3_groups_total(int D, int n_emb) { return 8LL * 16 + (long long)D * 8 * 32 + (long long)n_emb * 2 * 32; }
struct Bwd3Params {
  Net net;                 // packed, res_lds, res_bytes, D
  long long P, stride;
  const float* g_out; const float* acts; const float* rgbsigma;
  float* gpre; float* ghead;
  float* g_emb;            // (P,64) dL/d embedded input (natural column order, column 63 = 0), or null
  int skip;                // the skip layer (0 = none)
  const unsigned* mask; long long mask_stride;   // the forward's ReLU bit-mask rows (BITS instantiation), else acts is read
  uint32_t ring_off, buf_bytes;
};

template <bool BITS>
__global__ __launch_bounds__(256, 1) void nerf_backward_kernel_x3(const Bwd3Params p) {
  constexpr int NW = 4, TILE = NW * kWaveSamples;
  const Lane id;
  load_resident<NW>(p.net, id);
  StreamT<NW> st;
  st.tl.start(nullptr, id);
  CarryX carry;
  const int D = p.net.D;
  const char* first = p.net.packed + p.net.res_bytes;
  st.start(first, 16, 16, p.ring_off, p.buf_bytes, id);
  carry.load(st.slot_off(0) + id.lane * 16);
  const uint32_t zero_off = p.net.res_lds + kB3Zero * 4, rgbw = p.net.res_lds + kB3Rgb * 4, sigw = p.net.res_lds + kB3Sig * 4;
  const Next n32{32, nullptr, 32, nullptr}, nfirst{16, first, 16, nullptr};
  const long long ntiles = (p.P + TILE - 1) / TILE;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long s = tile * TILE + id.wave * kWaveSamples + id.j;
    const bool valid = s < p.P;
    const long long ss = valid ? s : p.P - 1;
    const float4 go = *reinterpret_cast<const float4*>(p.g_out + ss * 4);
    const float4 rs = *reinterpret_cast<const float4*>(p.rgbsigma + ss * 4);
    const float d0 = go.x * rs.x * (1.f - rs.x), d1 = go.y * rs.y * (1.f - rs.y), d2 = go.z * rs.z * (1.f - rs.z);
    if (valid && id.h == 0) *reinterpret_cast<float4*>(p.ghead + s * 4) = make_float4(d0, d1, d2, go.w);
    // BITS: "activation rows" are the sample's mask words (8 per layer); else the dump rows + 4 h
    const float* arow = BITS ? reinterpret_cast<const float*>(p.mask + ss * p.mask_stride) : p.acts + ss * p.stride + 4 * id.h;
    constexpr int LW = BITS ? 8 : 256;                           // row elements per layer
    float* grow = p.gpre + s * p.stride + 4 * id.h;             // rows up to round_up(P, 128) exist
    // d_e = (W_rgb^T d_o) [e > 0] as the (hi, lo) operands of 8 k-steps: slot e of step ks = feature 16 ks + hid_perm2(h, e)
    u32x4 ah[16], al[16], bh[16], bl[16];
    {
      const float* erow = arow + (long long)(D + 1) * LW;
      float* gerow = grow + (long long)(D + 1) * 256;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 2; ++c) {                            // features 16 ks + 8 c + 4 h + (0..3)
          const int f = 16 * ks + 8 * c;
          const f32x4 w0 = lds_f4(rgbw + (0 * 128 + f + 4 * id.h) * 4), w1 = lds_f4(rgbw + (1 * 128 + f + 4 * id.h) * 4);
          const f32x4 w2 = lds_f4(rgbw + (2 * 128 + f + 4 * id.h) * 4);
          f32x4 e4;
          if constexpr (BITS) {                                  // outputs (f & 31) + 4 h + r of the forward's panel f / 32
            const int fp = (f & 31) + 4 * id.h;
            const unsigned wv = reinterpret_cast<const unsigned*>(erow)[relu_mask_word(f >> 5, fp)] >> relu_mask_shift(f >> 5, fp);
#pragma unroll
            for (int r = 0; r < 4; ++r) e4[r] = ((wv >> r) & 1u) ? 1.f : 0.f;
          } else {
            e4 = *reinterpret_cast<const f32x4*>(erow + f);
          }
          f32x4 g;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x = __builtin_fmaf(w2[r], d2, __builtin_fmaf(w1[r], d1, w0[r] * d0));
            g[r] = e4[r] > 0.f ? x : 0.f;
            v[4 * c + r] = g[r];
          }
          *reinterpret_cast<f32x4*>(gerow + f) = g;
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const unsigned hi = pack_bf16x2(v[2 * w], v[2 * w + 1]);
          ah[ks][w] = hi;
          al[ks][w] = pack_bf16x2(v[2 * w] - bflo(hi), v[2 * w + 1] - bfhi(hi));
        }
      }
#pragma unroll
      for (int ks = 8; ks < 16; ++ks) { ah[ks] = u32x4{0u, 0u, 0u, 0u}; al[ks] = u32x4{0u, 0u, 0u, 0u}; }
    }
    // layer 0: d_g = W_e[:, :W]^T d_e (a -> b; xyz_encoding_final has no activation)
    bwd_layer_x<8, 8, false, false, true, BITS>(st, id, carry, ah, al, bh, bl, zero_off, n32, nullptr, grow + (long long)D * 256, 0u, 0.f);
    // layer 1: d_z_{D-1} = (W_f^T d_g + w_sigma d_sigma) [h_{D-1} > 0] (b -> a)
    bwd_layer_x<8, 16, true, true, true, BITS>(st, id, carry, bh, bl, ah, al, zero_off, D >= 2 ? n32 : nfirst, arow + (long long)(D - 1) * LW,
                                      grow + (long long)(D - 1) * 256, sigw, go.w);
    // layers 2 .. D: d_z_{l-1} = (W_l^T d_z_l) [h_{l-1} > 0], l = D-1 .. 1 (a -> b, copied back); the last one only stores
    for (int i = 2; i < D; ++i) {
      const int l = D + 1 - i;
      bwd_layer_x<8, 16, true, false, true, BITS>(st, id, carry, ah, al, bh, bl, zero_off, n32, arow + (long long)(l - 1) * LW,
                                         grow + (long long)(l - 1) * 256, 0u, 0.f);
#pragma unroll
      for (int t = 0; t < 16; ++t) { ah[t] = bh[t]; al[t] = bl[t]; }
    }
    if (!p.g_emb) {
      bwd_layer_x<8, 16, true, false, false, BITS>(st, id, carry, ah, al, bh, bl, zero_off, nfirst, arow, grow, 0u, 0.f);
    } else {
      // d emb = W_0[:, :63]^T d_z_0 (+ W_skip[:, :63]^T d_z_skip): two 32-row tiles each, K = W
      bwd_layer_x<8, 16, true, false, true, BITS>(st, id, carry, ah, al, bh, bl, zero_off, n32, arow, grow, 0u, 0.f);     // d_z_0 as an operand too
      f32x16 ge[2];
      bwd_emb_x(st, id, carry, bh, bl, zero_off, p.skip > 0 ? n32 : nfirst, ge);
      if (p.skip > 0) {
        // d_z_skip was stored by this very lane several layers ago (the panel barriers' vmcnt waits retired the stores)
        const float* zrow = grow + (long long)p.skip * 256;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(zrow + 16 * ks), v1 = *reinterpret_cast<const f32x4*>(zrow + 16 * ks + 8);
          const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const unsigned hi = pack_bf16x2(v[2 * w], v[2 * w + 1]);
            ah[ks][w] = hi;
            al[ks][w] = pack_bf16x2(v[2 * w] - bflo(hi), v[2 * w + 1] - bfhi(hi));
          }
        }
        f32x16 g2[2];
        bwd_emb_x(st, id, carry, ah, al, zero_off, nfirst, g2);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) ge[t][r] += g2[t][r];
      }
      if (valid) {
        float* er = p.g_emb + s * 64 + 4 * id.h;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ge[t][4 * q + i];
            *reinterpret_cast<f32x4*>(er + 32 * t + 8 * q) = v;
          }
      }
    }
  }
  wait_vm0();
}

}  // namespace bf
}  // namespace mf

using namespace mf;

static bool bwd3_supported(const mf_nerf_desc* d) {
  NetLayout F;
  return d && nerf_layout(*d, F, MF_PREC_BF16X3) && F.W == 256 && d->D >= 2;
}
static int bwd3_n_emb(const mf_nerf_desc* d) {           // embedded-input layers behind the chain (0 = g_emb unsupported)
  const int sk = single_skip_layer(d->skip_mask, d->D);
  return sk < 0 ? 0 : (sk > 0 ? 2 : 1);
}

extern "C" int64_t mf_nerf_bwd3_packed_bytes(const mf_nerf_desc* d) {
  if (!bwd3_supported(d)) { fail(MF_E_UNSUPPORTED, "mf_nerf_bwd3_packed_bytes: unsupported NeRF configuration"); return 0; }
  return bf::kB3ResBytes + bf::bwd3_groups_total(d->D, bwd3_n_emb(d)) * kGroupBytes;
}

extern "C" int32_t mf_nerf_pack_bwd3(const mf_nerf_desc* d, void* packed, void* stream) {
  if (!d || !packed) return fail(MF_E_INVALID, "mf_nerf_pack_bwd3: null argument");
  if (!bwd3_supported(d)) return fail(MF_E_UNSUPPORTED, "mf_nerf_pack_bwd3: unsupported NeRF configuration (W=%d D=%d)", d->W, d->D);
  // the forward layout of W^T (mf_layout.hpp), every k-step as (hi, lo) bf16 groups
  PackJob job{};
  const int ext = d->extra_feat_type == MF_EXTRA_NONE ? 0 : d->extra_feat_dim;
  auto wt = [](const float* W, int ld, int ksteps) { return PackBlock{W, 1, ld, kPackHidden, ksteps, 2, 16 * ksteps}; };
  for (int i = 0; i <= d->D; ++i) {
    const int l = d->D + 1 - i, col0 = (i > 1 && ((d->skip_mask >> l) & 1u)) ? d->in_channels_xyz : 0;
    const float* W = i == 0 ? d->extra_w : (i == 1 ? d->final_w : d->trunk_w[l]);
    if (!W) return fail(MF_E_INVALID, "mf_nerf_pack_bwd3: missing weight pointer (backward layer %d)", i);
    if (i == 0) job.add(8, 16, wt(W, 256 + ext, 8));
    else job.add(8, 32, wt(W + col0, 256 + col0, 16));
  }
  const int n_emb = bwd3_n_emb(d), sk = single_skip_layer(d->skip_mask, d->D);
  for (int e = 0; e < n_emb; ++e) {
    const int l = e == 0 ? 0 : sk;
    if (!d->trunk_w[l]) return fail(MF_E_INVALID, "mf_nerf_pack_bwd3: missing weight pointer (backward layer %d)", d->D + 1 + e);
    job.add(2, 32, wt(d->trunk_w[l], (l == 0 ? 0 : 256) + d->in_channels_xyz, 16)).n_rows = d->in_channels_xyz;
  }
  if (!d->sigma_w || !d->rgb_w) return fail(MF_E_INVALID, "mf_nerf_pack_bwd3: missing sigma / rgb weight");
  job.bf16 = 1;
  job.res[job.n_res++] = ResCopy{d->rgb_w, bf::kB3Rgb, 384};
  job.res[job.n_res++] = ResCopy{d->sigma_w, bf::kB3Sig, 256};
  job.res_floats = bf::kB3ResBytes / 4;
  job.resident = static_cast<float*>(packed);
  job.panels = reinterpret_cast<float*>(static_cast<char*>(packed) + bf::kB3ResBytes);
  if (job.total_groups != bf::bwd3_groups_total(d->D, n_emb)) return fail(MF_E_INVALID, "mf_nerf_pack_bwd3: layout mismatch");
  return launch_pack(job, static_cast<hipStream_t>(stream), "mf_nerf_pack_bwd3");
}

extern "C" int32_t mf_nerf_backward3(const mf_nerf_desc* d, const void* packed_bwd3, int64_t P, const float* g_out,
                                     const float* acts, int64_t stride, const float* rgbsigma, float* gpre, float* ghead,
                                     float* g_emb, const uint32_t* mask, int64_t mask_stride, void* stream) {
  if (!d || !packed_bwd3 || (P > 0 && (!g_out || (!acts && !mask) || !rgbsigma || !gpre || !ghead)))
    return fail(MF_E_INVALID, "mf_nerf_backward3: null argument");
  if (!bwd3_supported(d)) return fail(MF_E_UNSUPPORTED, "mf_nerf_backward3: unsupported NeRF configuration (W=%d D=%d)", d->W, d->D);
  if (mask && mask_stride < (int64_t)(d->D + 2) * 8) return fail(MF_E_INVALID, "mf_nerf_backward3: mask_stride %lld < 8 (D + 2)", (long long)mask_stride);
  if (stride < (int64_t)(d->D + 1) * 256 + 128 || (stride & 3) || (reinterpret_cast<uintptr_t>(acts) & 15) || (reinterpret_cast<uintptr_t>(gpre) & 15))
    return fail(MF_E_INVALID, "mf_nerf_backward3: dump rows must be 16-byte aligned, stride >= (D + 1) W + W / 2 and a multiple of 4 floats");
  if (g_emb && bwd3_n_emb(d) == 0)
    return fail(MF_E_UNSUPPORTED, "mf_nerf_backward3: the embedded-input gradient is built for at most one skip layer");
  if (P == 0) return MF_OK;
  bf::Bwd3Params p{};
  p.g_emb = g_emb; p.skip = single_skip_layer(d->skip_mask, d->D) > 0 ? single_skip_layer(d->skip_mask, d->D) : 0;
  p.mask = mask; p.mask_stride = mask_stride;
  p.net.packed = static_cast<const char*>(packed_bwd3);
  p.net.res_lds = 0; p.net.res_bytes = bf::kB3ResBytes; p.net.D = d->D; p.net.emb_mask = 0; p.net.aux = 0;
  p.P = P; p.stride = stride; p.g_out = g_out; p.acts = acts; p.rgbsigma = rgbsigma; p.gpre = gpre; p.ghead = ghead;
  uint32_t lds = bf::kB3ResBytes;
  place_ring(lds, 32, p.ring_off, p.buf_bytes);
  const int grid = persistent_grid((P + 127) / 128);
  void (*kern)(const bf::Bwd3Params) = mask ? bf::nerf_backward_kernel_x3<true> : bf::nerf_backward_kernel_x3<false>;
  return launch_lds(kern, grid, 256, lds, static_cast<hipStream_t>(stream), p, "mf_nerf_backward3", "mf_nerf_backward3");
}
