// mf_surface.hpp -- what the units on a MeshIndex share (mf_mesh_distance.hip, mf_mesh_rays.hip), written once: the tile
// constants, the checked corner load, the host checks of the mf_surface_* entry points.  No kernel here.  The tile walk stands in
// both search kernels: as one function template md_closest_kernel came out 25 % slower (profiles/ab_tile_walk_mi355x.txt).
#pragma once
#include <initializer_list>
#include "mf_f3.hpp"
#include "mf_host.hpp"
#include "mf_scan.hpp"

namespace mf {

constexpr int kSurfThreads = 256;                // per workgroup, of every kernel of the two units
constexpr int kSurfWaves = kSurfThreads / 64;
constexpr int kSurfTile = 64;                    // slots per tile: one per lane of a wave
constexpr int kSurfBox = 8;                      // floats per tile box, as md_build_kernel writes them: lo, hi, the kept slots, 0
constexpr int kSurfBoxKept = 6;                  // where a box holds the number of its kept slots

// The corners of triangle t of `tris` over V vertices; false if an index lies outside [0, V): before any address is formed.
__device__ __forceinline__ bool load_corners(const float* verts, const long long* tris, long long V, long long t, F3& a, F3& b, F3& c) {
  const long long i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
  if (!(in_range(i0, V) && in_range(i1, V) && in_range(i2, V))) return false;
  a = f3(verts + 3 * i0); b = f3(verts + 3 * i1); c = f3(verts + 3 * i2);
  return true;
}

inline bool surf_count_ok(int64_t n) { return n >= 0 && n < kIndexLimit - 1; }
inline long long surf_blocks(long long n) { return (n + kSurfThreads - 1) / kSurfThreads; }
inline int surf_tiles(int64_t T) { return (int)(align_up(T, kSurfTile) / kSurfTile); }
// true, with the error text in the entry's name, if an output is one of the inputs (a null output is none): MF_E_INVALID
inline bool surf_alias(const char* entry, std::initializer_list<const void*> out, std::initializer_list<const void*> in) {
  for (const void* o : out)
    for (const void* i : in)
      if (o && o == i) return fail(MF_E_INVALID, "%s: an output aliases an input", entry) != MF_OK;
  return false;
}

}  // namespace mf
