// mf_shares.hpp -- how a launch divides its input and its scratch buffer, written once.  Plain C++: no HIP include, a host
// compiler alone builds it (tests/test_host_cpu.py does, under the sanitizers).  Users: mf_batch.hip (mf_mask_compact),
// mf_regions.hip, mf_mesh_simplify.hip, mf_mesh_smooth.hip (share_of, Carver), mf_mesh_components.hip, mf_mesh.hip,
// mf_voxelize.hip, mf_distance.hip, mf_mesh_distance.hip (Carver); mf_host.hpp (kIndexLimit, align_up).  The device side of a share is mf_scan.hpp's share_range.
#pragma once
#include <cstdint>

namespace mf {

constexpr long long kIndexLimit = 1LL << 31;     // 32-bit internal indexing: what a unit indexes with int stays below it

inline long long align_up(long long x, long long a) { return (x + a - 1) & ~(a - 1); }   // a: a power of 2

// The contiguous-share plan of a kernel whose ranks follow the input order: workgroup b owns [b per, min(n, (b + 1) per)), per
// a multiple of the tile: ceil(n / (tile max_blocks)) tiles.  No workgroup owns an empty range; n == 0 launches nothing.
struct Share { long long per; int nblocks; };

inline Share share_of(long long n, int tile, int max_blocks) {
  const long long tiles = (n + tile - 1) / tile;
  const long long nb0 = tiles < max_blocks ? tiles : max_blocks;
  if (nb0 == 0) return {tile, 0};
  const long long per = (tiles + nb0 - 1) / nb0 * tile;
  return {per, (int)((n + per - 1) / per)};
}

// Carves one scratch buffer into its fields, in the order of the take calls.  The base is an integer: a size query passes null
// and reads bytes() alone.  A field is padded to `align` bytes (16, but for the two layouts that pack their tail).
struct Carver {
  uintptr_t base;
  long long at = 0;
  explicit Carver(const void* scratch) : base(reinterpret_cast<uintptr_t>(scratch)) {}
  template <class T>
  T* take(long long count, long long align = 16) {
    T* p = reinterpret_cast<T*>(base + (uintptr_t)at);
    at += align_up(count * (long long)sizeof(T), align);
    return p;
  }
  long long bytes() const { return at; }
};

}  // namespace mf
