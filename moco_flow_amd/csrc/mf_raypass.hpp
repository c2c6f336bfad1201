// mf_raypass.hpp -- what the two fused render passes (mf_render.hip: fp32, mf_render_bf16.hip: bf16 / bf16x3) share around
// their MLP cores.  Device: the chain program's role table, the ray front end, the per-ray composite, the kernarg -> LDS copy of
// the embedding tables, the timeline's workgroup stamps -- templated on the parameter struct (each kernel keeps its own field
// order, kernarg offsets and scalar loads), lane / wave as plain ints (the families' lane structs differ).  Host: the fields the
// parameter structs have in common, the sample buffers' placement, the dumps' checks.
#pragma once
#include <cstddef>

#include "mf_core.hpp"
#include "mf_host.hpp"
#include "mf_layout.hpp"

namespace mf {

// ---- the chain program (rendering.py:270-282): step 0 bw(x,i) -> canon; local: fw(canon,i) -> recon;
// global: fw(canon,j) -> a; bw(a,j) -> b; fw(b,i) -> chained recon.
// role of a step: 0 = bw_i, 1 = local fw_i, 2 = fw_j, 3 = bw_j, 4 = final fw_i  (chain_global implies chain_local -- checked
// on the host -- so role == step).  Host and device.
constexpr int chain_steps(int flags) { return 1 + ((flags & MF_F_CHAIN_LOCAL) ? 1 : 0) + ((flags & MF_F_CHAIN_GLOBAL) ? 3 : 0); }
constexpr bool role_uses_fw(int role) { return role == 1 || role == 2 || role == 4; }   // else: the backward flow
constexpr int role_ind_column(int role) { return (role == 2 || role == 3) ? 9 : 8; }    // ray column of the image index it reads
// row of the bf16 passes' per-ray bias table a role reads: bw(i), fw(i), fw(j), bw(j); the final fw(i) is row 1 again
constexpr int role_bias_row(int role) { return role == 4 ? 1 : role; }
constexpr int chain_bias_rows(int flags) { return chain_steps(flags) < 4 ? chain_steps(flags) : 4; }   // rows the pass's roles read

// ---- ray front end: depth of sample `si` of ray `ray` (row `rp`), rendering.py:245-251, and the point o + d z (:262-263).
// Both round as torch does (-ffp-contract=off: sin(512 x) sees every ulp).
template <class P>
MF_D float ray_depth(const P& p, const float* rp, long long ray, int si) {
  if (p.z_vals) return p.z_vals[ray * p.S + si];
  const float nearv = rp[6], farv = rp[7], t = p.z_steps[si];
  if (!p.use_disp) return nearv * (1.f - t) + farv * t;                         // rendering.py:247
  return 1.f / (1.f / nearv * (1.f - t) + 1.f / farv * t);                       // rendering.py:249
}
MF_D void ray_point(const float (&o)[3], const float (&d)[3], float z, float (&x)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = o[c] + d[c] * z;                            // rendering.py:262-263
}

// ---- composite (rendering.py:157-192) of a group's rays out of the LDS sample buffers: one wave per ray, lanes over samples
template <int NW, class P>
MF_D void composite_group(const P& p, int lane, int wave, long long ray0, int nr, int S, bool sigma_only, const float4* sbuf,
                          const float* zbuf) {
  for (int rr = wave; rr < nr; rr += NW) {
    const long long ray = ray0 + rr;
    const float* rp = p.rays + ray * p.ray_stride;
    const float dnorm = sqrtf(rp[3] * rp[3] + rp[4] * rp[4] + rp[5] * rp[5]);  // rendering.py:164
    float carry_t = 1.f, acc_r = 0.f, acc_g = 0.f, acc_b = 0.f, acc_d = 0.f, acc_w = 0.f;
    for (int base = 0; base < S; base += 64) {
      // (opaque lane index: keeps hipcc from hoisting `plane + 4 lane` of every output plane out of the group loop
      //  as 64-bit per-lane addresses that then sit in -- or spill from -- registers across the MFMA section)
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int i = base + ln;
      const bool v = i < S;
      const int ii = v ? i : S - 1;
      const float4 s4 = sbuf[rr * S + ii];
      const float z = zbuf[rr * S + ii];
      const float znext = zbuf[rr * S + (ii + 1 < S ? ii + 1 : ii)];
      float delta = (ii == S - 1) ? 1e10f : znext - z;                       // :158-160
      delta = delta * dnorm;
      float sg = s4.w;
      if (p.noise) sg = sg + p.noise[ray * S + ii];                          // :166 (pre-scaled)
      float a;
      if (p.activation == MF_ACT_RELU) a = fmaxf(sg, 0.f);
      else a = softplus_torch(sg);                                             // nn.Softplus(beta=1, threshold=20)
      float alpha = 1.f - expf(-delta * a);                                  // :170/172
      if (!v) alpha = 0.f;
      const float pt = v ? (1.f - alpha) + 1e-10f : 1.f;                     // :176-177
      const float incl = wave_scan_mul_dpp(pt);
      const float excl = wave_shr1_dpp(1.f, incl);
      const float w = alpha * (carry_t * excl);                              // :178-179
      carry_t = carry_t * wave_last(incl);
      if (v) {
        if (p.weights) p.weights[ray * S + i] = w;
#ifndef MF_TIMELINE
        if (p.alphas) p.alphas[ray * S + i] = alpha;
#endif
        acc_w += w;
        acc_r += w * s4.x; acc_g += w * s4.y; acc_b += w * s4.z;
        acc_d += w * z;
      }
    }
    acc_w = wave_sum_dpp(acc_w);                                                 // :180
    if (!sigma_only) {
      acc_r = wave_sum_dpp(acc_r); acc_g = wave_sum_dpp(acc_g); acc_b = wave_sum_dpp(acc_b);   // :186
      acc_d = wave_sum_dpp(acc_d);                                               // :187
    }
    if (lane == 0) {
      if (p.opacity) p.opacity[ray] = acc_w;
      if (!sigma_only) {
        if (p.bg) {                                                          // :189-190
          const float k = 1.f - acc_w;
          acc_r = acc_r + p.bg[ray * 3 + 0] * k;
          acc_g = acc_g + p.bg[ray * 3 + 1] * k;
          acc_b = acc_b + p.bg[ray * 3 + 2] * k;
        }
        if (p.rgb) { p.rgb[ray * 3 + 0] = acc_r; p.rgb[ray * 3 + 1] = acc_g; p.rgb[ray * 3 + 2] = acc_b; }
        if (p.depth) p.depth[ray] = acc_d;
      }
    }
  }
}

// ---- the embedding tables (P::emb_par, 128 floats) kernarg -> LDS at p.par_off, through the kernarg segment pointer: a
// runtime index into the by-value struct would make hipcc keep a private (scratch) copy of all of `p`.  Published by the
// barrier of the kernel's start_program.
template <class P>
MF_D void emb_tables_to_lds(const P& p) {
  if (threadIdx.x < 128) {
    typedef const __attribute__((address_space(4))) char* kptr;
    const kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr() + offsetof(P, emb_par);
    *(float*)(smem + p.par_off + threadIdx.x * 4) = ((const __attribute__((address_space(4))) float*)ka)[threadIdx.x];
  }
}

// ---- (timing builds only, -DMF_TIMELINE) every workgroup's start / end on the chip-wide 100 MHz clock, in alphas[2..3] of
// its last group: `const WgClock wg;` first thing in the kernel, `wg.stamp(p);` last
struct WgClock {
#ifdef MF_TIMELINE
  unsigned long long rt0;
  MF_D WgClock() : rt0(__builtin_amdgcn_s_memrealtime()) {}
  template <class P> MF_D void stamp(const P& p) const {
    if (threadIdx.x == 0 && p.alphas && blockIdx.x < p.n_groups) {
      const long long lastg = blockIdx.x + ((p.n_groups - 1 - blockIdx.x) / gridDim.x) * gridDim.x;
      float* o = p.alphas + lastg * p.G * p.S;
      o[2] = (float)(rt0 & 0xFFFFFFull);
      o[3] = (float)(__builtin_amdgcn_s_memrealtime() & 0xFFFFFFull);
    }
  }
#else
  template <class P> MF_D void stamp(const P&) const {}
#endif
};

// ---- what mf_render_pass fills and checks for both families ----
// the fields the families' parameter structs share: rays, depths, noise, activation, flags, outputs, the NeRF dump's buffers
// (copied before the dumps' checks, also for a pass that dumps nothing: only the DUMP instantiations read p.dump_*)
template <class P>
inline void fill_render_io(P& p, const mf_render_args* a) {
  p.rays = a->rays; p.ray_stride = a->ray_stride; p.n_rays = a->n_rays; p.bg = a->background;
  p.S = a->n_samples; p.z_vals = a->z_vals; p.z_steps = a->z_steps; p.use_disp = a->use_disp;
  p.noise = a->noise; p.activation = a->activation; p.flags = a->flags;
  p.extra_type = a->nerf->extra_feat_type;
  p.rgb = a->rgb; p.depth = a->depth; p.opacity = a->opacity; p.weights = a->weights; p.alphas = a->alphas;
  p.disp_local = a->disp_local; p.disp_global = a->disp_global;
  p.dump_acts = a->dump_acts; p.dump_stride = a->dump_stride; p.dump_rgbsigma = a->dump_rgbsigma; p.dump_xyz = a->dump_xyz;
  p.dump_mask = a->dump_mask; p.dump_mask_stride = a->dump_mask_stride;
}

// the group's sample buffers behind everything else in LDS: float4 rgb-sigma + float depth per sample (plan_ray_groups' 20 bytes)
template <class P>
inline void place_sample_buffers(P& p, uint32_t& lds) {
  p.sbuf_off = lds; lds += (uint32_t)(p.G * p.S) * 16;
  p.zbuf_off = lds; lds += (uint32_t)(p.G * p.S) * 4;
  lds = (lds + 15u) & ~15u;
}

// the NeRF dump of a training forward, in the order the passes check it: rows of dump_acts wide enough for the layers of L, [the
// bf16x3 pass: their alignment,] the ReLU bit rows beside them (n_trunk = D + 1 layers: D + 2 rows of 8 words)
inline int check_dump_rows(const mf_render_args* a, const NetLayout& L) {
  if (a->dump_acts && a->dump_stride < (int64_t)L.n_trunk * L.W + L.W / 2)
    return fail(MF_E_INVALID, "mf_render_pass: dump_stride %lld too small", (long long)a->dump_stride);
  return MF_OK;
}
inline int check_dump_mask(const mf_render_args* a, const NetLayout& L) {
  if (a->dump_mask && (!a->dump_acts || a->dump_mask_stride < (int64_t)(L.n_trunk + 1) * 8))
    return fail(MF_E_INVALID, "mf_render_pass: dump_mask needs dump_acts and dump_mask_stride >= 8 (D + 2) words");
  return MF_OK;
}

// dump_nof_plane: the plane each NoF chain step of the pass writes, a permutation of 0 .. steps - 1 -> `pack`, 3 bits per step
inline int nof_plane_pack(const mf_render_args* a, uint32_t& pack) {
  const int nsteps = chain_steps(a->flags);
  uint32_t seen = 0;
  pack = 0;
  for (int k = 0; k < nsteps; ++k) {
    const int pl = a->dump_nof_plane[k];
    if (pl < 0 || pl >= nsteps || ((seen >> pl) & 1u)) return fail(MF_E_INVALID, "mf_render_pass: dump_nof_plane must be a permutation of 0..%d", nsteps - 1);
    seen |= 1u << pl;
    pack |= (uint32_t)pl << (3 * k);
  }
  return MF_OK;
}

}  // namespace mf
