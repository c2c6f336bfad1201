// mf_host.hpp -- host-side helpers shared by the C-ABI translation units (and softplus_torch, the one device helper all share).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#include "../../include/mocoflow_hip.h"
#include "mf_shares.hpp"   // kIndexLimit, align_up, share_of, Carver

namespace mf {

char* last_error_buf();   // thread-local, 512 bytes (mf_abi.hip)

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MF_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
  return MF_OK;
}

// A kernel that takes its parameter struct by value and `lds` bytes of dynamic LDS: raise its limit (`reserve` false: the size is
// inside every launch's default), launch, report the launch (what_launch null: the caller checks after its further launches).
template <class P>
inline int launch_lds(void (*kern)(P), unsigned grid, unsigned threads, size_t lds, hipStream_t stream, const P& params,
                      const char* what_reserve, const char* what_launch, bool reserve = true) {
  if (reserve && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(MF_E_LAUNCH, "%s: cannot reserve %zu bytes of LDS", what_reserve, lds);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, params);
  return what_launch ? check_launch(what_launch) : MF_OK;
}

int device_cus();   // mf_forward.hip

// grid of a persistent launch over `work` workgroup-sized items: at most one workgroup per CU
inline int persistent_grid(long long work) {
  const long long cus = device_cus();
  return (int)(work < cus ? work : cus);
}

// grid of a grid-stride launch: ceil(n / per_block) workgroups, at most `cap`, at least `floor`
inline long long capped_blocks(long long n, long long per_block, long long cap, long long floor = 0) {
  const long long b = (n + per_block - 1) / per_block; return b < floor ? floor : b < cap ? b : cap;
}

inline bool is_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }   // a: a power of 2
// the vertex and triangle counts of a unit that indexes a mesh with 32-bit integers
inline int mesh_index_shape(const char* what, int64_t V, int64_t T) {
  if (V < 0 || T < 0 || V >= kIndexLimit || T >= kIndexLimit)
    return fail(MF_E_INVALID, "%s: V=%lld T=%lld (32-bit indexing: both in [0, 2^31))", what, (long long)V, (long long)T);
  return MF_OK;
}
// torch.nn.Softplus(): beta 1, threshold 20 (the render pass, the composite, mf_point_loss_partials, the occupancy grid)
__device__ __forceinline__ float softplus_torch(float s) { return s > 20.f ? s : log1pf(expf(s)); }

// an embedding's frequencies and weights as 16-entry tables, 0 beyond n_freqs; returns: the frequencies are exactly 2^k
inline bool emb_table(const mf_embedding& e, float* freq, float* weight) {
  bool pow2 = true;
  for (int k = 0; k < 16; ++k) {
    freq[k] = k < e.n_freqs ? e.freq[k] : 0.f;
    weight[k] = k < e.n_freqs ? e.weight[k] : 0.f;
    if (k < e.n_freqs && e.freq[k] != (float)(1 << k)) pow2 = false;
  }
  return pow2;
}

// ---- launch planning of the render passes (mf_render.hip: fp32, mf_render_bf16.hip: bf16 / bf16x3) ----
constexpr uint32_t kRenderLdsCap = 160 * 1024;   // LDS of one render workgroup

// Rays per group of a render pass whose workgroup holds `lds` bytes before its 20 bytes per staged sample (float4 rgb-sigma,
// float depth): the smallest G with G*S a multiple of the tile (`tile` samples), capped by the LDS left; no exact fit: as many
// rays as reduce the padding waste.  Then several such ray sets per group (up to 8): the composite phase between two groups
// keeps at most one wave per ray busy and costs two workgroup barriers (~4 k cycles per 128-sample tile at G = 2 in the fp32
// pass: tools/timeline.py), so it should come once per several tiles -- as long as the CUs' shares stay what they were (same
// makespan in rays).
// `ray_bytes`: what the kernel stages per RAY of the group besides (the folded fp32 kernels' bias row and encoding, mf_render.hip).
inline int plan_ray_groups(long long n_rays, int S, int tile, uint32_t lds, int& G, long long& n_groups, uint32_t ray_bytes = 0) {
  const long long room = lds < kRenderLdsCap ? (long long)(kRenderLdsCap - lds) : 0;
  auto fits = [&](long long g) {       // (the per-ray rows sit behind place_sample_buffers' padding to 16 bytes)
    return (ray_bytes ? ((g * S * 20 + 15) & ~15ll) + g * (long long)ray_bytes : g * S * 20) <= room;
  };
  const int max_samples = (int)((room > ray_bytes ? room - ray_bytes : 0) / 20);      // of a single ray
  if (!fits(1)) return fail(MF_E_UNSUPPORTED, "mf_render_pass: n_samples=%d exceeds the %d samples a workgroup can stage", S, max_samples);
  G = 1;
  while ((G * S) % tile != 0 && fits(G + 1) && G < 64) ++G;
  if ((G * S) % tile != 0) {
    int best = 1; double best_eff = 0;
    for (int g = 1; fits(g) && g <= 64; ++g) {
      const int tiles = (g * S + tile - 1) / tile;
      const double eff = (double)(g * S) / (tiles * tile);
      if (eff > best_eff + 1e-9) { best_eff = eff; best = g; }
    }
    G = best;
  }
  const long long cus = device_cus();
  auto makespan = [&](long long g) { const long long groups = (n_rays + g - 1) / g; return (groups + cus - 1) / cus * g; };
  const long long base = makespan(G);
  int sets = 1;
  for (int c = 2; c <= 8; ++c)
    if (fits((long long)G * c) && (long long)G * c <= 64 && makespan((long long)G * c) <= base) sets = c;
  G *= sets;
  n_groups = (n_rays + G - 1) / G;
  return MF_OK;
}

}  // namespace mf
