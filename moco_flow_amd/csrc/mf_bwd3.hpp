// mf_bwd3.hpp -- one layer of an input-gradient chain on the MF_PREC_BF16X3 tile loop of mf_bf16.hpp (shared by the NeRF and NoF
// backward kernels, mf_backward_bf16.hip and mf_nofgrad_bf16.hip): the layer's input and the transposed weights as (hi, lo) bf16
// pairs, three products per k-step, fp32 accumulation.  A tile's epilogue (sigma term, mask, (hi, lo) split of the next layer's
// operand) runs in the MFMA gaps of the next tile; its four 16-byte row stores sit behind that tile's last LDS-DMA piece so that
// the panel barrier leaves exactly them (and the next tile's mask loads) in flight (StreamT::sync<KEEP>).
#pragma once
#include <utility>
#include "mf_bf16.hpp"

namespace mf {
namespace bf {

template <class F, int... T>
MF_D void each_tile(F&& f, std::integer_sequence<int, T...>) { (f(std::integral_constant<int, T>{}), ...); }

// value of accumulator register r of tile t: + the sigma term, masked by the forward activation
// (BITS: m[0][0] carries the two mask bytes of this lane half for the tile -- lane groups g = h (low byte) and g = 2 + h of the
//  forward's panel t, relu_mask_word / relu_mask_shift in mf_core.hpp: row 8 q + 4 h + i of the tile sits at bit
//  8 (q & 1) + 4 (q >> 1) + i)
template <bool MASK, bool SIG, bool BITS>
MF_D float b3_val(const f32x16& acc, const f32x4 (&m)[4], int r, uint32_t sigw_off, int t, int h, float dsig) {
  float v = acc[r];
  if (SIG) v = __builtin_fmaf(lds_f(sigw_off + (32 * t + 8 * (r >> 2) + 4 * h + (r & 3)) * 4), dsig, v);
  if (MASK) {
    if (BITS) v = ((__builtin_bit_cast(unsigned, m[0][0]) >> (((r >> 2) & 1) * 8 + ((r >> 2) >> 1) * 4 + (r & 3))) & 1u) ? v : 0.f;
    else v = m[r >> 2][r & 3] > 0.f ? v : 0.f;
  }
  return v;
}

// One backward layer of NT 32-row tiles: (out, outlo) <- split(mask * (Wt (in, inlo) [+ w_sigma d_sigma])), the fp32 values to
// grow[32 t + ...].  KHID = k-steps of the input (8 | 16).  mrow / grow: this lane's dump row / gradient row of the layer + 4 (lane >> 5).
// BITS: `mrow` points at the layer's mask words of this lane's sample instead (one 4-byte load per tile).  OUT: the result is an
// operand again.  SIG (the NeRF's xyz_encoding_final^T): + sigma.weight (LDS at sigw_off) x dsig; unused otherwise.
template <int NT, int KHID, bool MASK, bool SIG, bool OUT, bool BITS, class ST>
MF_D void bwd_layer_x(ST& st, const Lane& id, CarryX& carry, const u32x4 (&in)[2 * NT], const u32x4 (&inlo)[2 * NT],
                      u32x4 (&out)[2 * NT], u32x4 (&outlo)[2 * NT], uint32_t zero_off, const Next& nxt, const float* mrow, float* grow,
                      uint32_t sigw_off, float dsig) {
  constexpr int NG = 2 * KHID, NM = 3 * KHID, kSteps = 16;
  f32x16 pend = {};
  f32x4 pm[4] = {}, hm[4] = {};
  // The sigma term and the mask are applied ONCE per element -- in the hi step of its pair, written back into the pending
  // accumulators -- and the lo step and the row store read the finished value (round 5; before, each of the three re-did them).
  // Every hi step (sidx <= 14) lies in front of the first store gap.
  auto step = [&](f32x16& acc, const f32x4 (&m)[4], int sidx, int t) __attribute__((always_inline)) {
    const int u = sidx >> 1, w = u & 3, r = u < 4 ? 2 * u : 8 + 2 * (u - 4);
    if (!OUT) return;
    if (!(sidx & 1)) {
      acc[r] = b3_val<MASK, SIG, BITS>(acc, m, r, sigw_off, t, id.h, dsig);
      acc[r + 1] = b3_val<MASK, SIG, BITS>(acc, m, r + 1, sigw_off, t, id.h, dsig);
    }
    const float v0 = acc[r], v1 = acc[r + 1];
    u32x4& hv = u < 4 ? out[2 * t] : out[2 * t + 1];
    if (!(sidx & 1)) {
      unsigned hi = pack_bf16x2(v0, v1);
      asm volatile("" : "+v"(hi));
      hv[w] = hi;
    } else {
      const unsigned hi = hv[w];
      unsigned lo = pack_bf16x2(v0 - bflo(hi), v1 - bfhi(hi));
      asm volatile("" : "+v"(lo));
      (u < 4 ? outlo[2 * t] : outlo[2 * t + 1])[w] = lo;
    }
  };
  auto store = [&](const f32x16& acc, const f32x4 (&m)[4], int t, int q) __attribute__((always_inline)) {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = OUT ? acc[4 * q + i] : b3_val<MASK, SIG, BITS>(acc, m, 4 * q + i, sigw_off, t, id.h, dsig);   // (OUT: finished by the hi steps)
    *reinterpret_cast<f32x4*>(grow + 32 * t + 8 * q) = v;
  };
  auto run = [&](auto tc) __attribute__((always_inline)) {
    constexpr int t = decltype(tc)::value;
    const Ahead two{t + 2 < NT ? NG : (t == NT - 2 ? nxt.groups : nxt.groups2),
                    t == NT - 2 ? nxt.jump : (t == NT - 1 ? nxt.jump2 : nullptr), 0, nullptr, t + 2 < NT ? NG : -1, -1};
    if constexpr (MASK && BITS) {                             // this tile's two mask bytes: in flight across its MFMAs
      hm[0][0] = __builtin_bit_cast(float, relu_mask_pair(reinterpret_cast<const unsigned*>(mrow), t, id.h));
    } else if constexpr (MASK) {
#pragma unroll
      for (int q = 0; q < 4; ++q) hm[q] = *reinterpret_cast<const f32x4*>(mrow + 32 * t + 8 * q);
    }
    constexpr int tp = t > 0 ? t - 1 : 0;
    auto gap = [&](int m) __attribute__((always_inline)) {
      if (t == 0) return;
#pragma unroll
      for (int sidx = kSteps * m / NM; sidx < kSteps * (m + 1) / NM; ++sidx) step(pend, pm, sidx, tp);
      if (m >= NM - 4) store(pend, pm, tp, m - (NM - 4));
    };
    f32x16 acc;
    // VM operations younger than the previous panel's last piece at this tile's first barrier: the four row stores that
    // closed the previous tile (tile 0: the layer in front; none behind tile 0) + this tile's four mask loads
    constexpr int KEEP = (t == 1 ? 0 : 4) + (MASK ? (BITS ? 2 : 4) : 0);
    mma_tile_x<0, KHID, 2, true, KEEP, true>(st, id, carry, in, inlo, in, inlo, zero_off, two, acc, gap);
    st.advance();
    pend = acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) pm[q] = hm[q];
  };
  each_tile(run, std::make_integer_sequence<int, NT>{});
#pragma unroll
  for (int sidx = 0; sidx < kSteps; ++sidx) step(pend, pm, sidx, NT - 1);
#pragma unroll
  for (int q = 0; q < 4; ++q) store(pend, pm, NT - 1, q);
  __builtin_amdgcn_sched_barrier(0);
}

// A 64-row layer behind the chain (the embedded-input gradient): res[t] = Wt_tile (in, inlo), t = 0, 1; nothing stored.
template <int KHID, class ST>
MF_D void bwd_emb_x(ST& st, const Lane& id, CarryX& carry, const u32x4 (&in)[KHID], const u32x4 (&inlo)[KHID], uint32_t zero_off,
                    const Next& nxt, f32x16 (&res)[2]) {
  const Ahead t0{nxt.groups, nxt.jump, 0, nullptr}, t1{nxt.groups2, nxt.jump2, 0, nullptr};
  auto nogap = [](int) {};
  mma_tile_x<0, KHID, 2, true>(st, id, carry, in, inlo, in, inlo, zero_off, t0, res[0], nogap);
  st.advance();
  mma_tile_x<0, KHID, 2, true>(st, id, carry, in, inlo, in, inlo, zero_off, t1, res[1], nogap);
  st.advance();
}


}  // namespace bf
}  // namespace mf
