// mf_plan.hpp -- the host side of a launch of the register-resident MFMA kernels, written once: where a workgroup's LDS
// holds what (LdsPlan), the embeddings those kernels are built for (check_*), the timing-ablation switches (debug_flags).
// Host-only; every fp32 entry point (mf_forward.hip, mf_nofgrad.hip, mf_backward.hip, mf_render.hip) plans with LdsPlan, the
// bf16 units share place_ring.
#pragma once
#include <cstdlib>

#include "mf_core.hpp"
#include "mf_host.hpp"

namespace mf {

// the 3-slot panel ring (Stream, mf_core.hpp) of `groups` 1 KiB groups per slot, at `lds`
inline void place_ring(uint32_t& lds, int groups, uint32_t& ring_off, uint32_t& buf_bytes) {
  ring_off = lds;
  buf_bytes = (uint32_t)groups * kGroupBytes;
  lds += 3 * buf_bytes;
}

// A workgroup's LDS from offset 0: [resident block of every network][the four 128-byte embedding tables, where the kernel reads
// them from LDS][ring of three slots of the largest panel]; `lds` = bytes placed so far (a render pass goes on behind the ring).
struct LdsPlan {
  uint32_t lds = 0;
  int max_groups = 0;
  void place(NetDev& n, const void* packed) {      // a network whose layout n.L is filled
    n.packed = static_cast<const char*>(packed);
    n.res_lds = lds; lds += (uint32_t)n.L.res_bytes;
    if (n.L.max_groups > max_groups) max_groups = n.L.max_groups;
  }
  uint32_t place_tables() { const uint32_t at = lds; lds += 512; return at; }
  void ring(uint32_t& ring_off, uint32_t& buf_bytes) { place_ring(lds, max_groups, ring_off, buf_bytes); }
};

// ---- the embeddings the kernels are built for; `who`: the entry point that words the refusal ----
inline int check_xyz_embedding(const char* who, const mf_embedding& e, int max_freqs) {
  if (e.in_channels != 3 || e.n_freqs > max_freqs)
    return fail(MF_E_UNSUPPORTED, "%s: xyz embedding must have 3 channels and <= %d frequencies", who, max_freqs);
  return MF_OK;
}

inline int check_nof_embeddings(const char* who, const mf_embedding& xyz, const mf_embedding& ind) {
  if (xyz.in_channels != 3 || xyz.n_freqs > 5 || ind.in_channels != 1 || ind.n_freqs > 16)
    return fail(MF_E_UNSUPPORTED, "%s: NoF embeddings must be xyz(3, <=5 freqs) and ind(1, <=16 freqs)", who);
  return MF_OK;
}

// The extra block of a "dir" / "ind" NeRF (rendering.py:133-142) has NO function here: its two checks differ in two ways --
// mf_render_pass refuses with MF_E_UNSUPPORTED and reads n_freqs < 0 as no frequencies, mf_points_radiance refuses with
// MF_E_INVALID and names n_freqs < 0 a fault -- so each entry point keeps its own.

// MF_DEBUG_FLAGS: timing ablations only (the kernels honour them in MF_TIMING_FLAGS builds)
inline int debug_flags() {
  const char* e = getenv("MF_DEBUG_FLAGS");
  return e ? atoi(e) : 0;
}

}  // namespace mf
