// mf_unionfind.hpp -- the lock-free union-find of the library and its wave-aggregated integer counts, written once.  Users:
// mf_mesh_components.hip (vertices of an indexed mesh), mf_regions.hip (pixels of a thresholded image: in LDS per tile, then in
// global memory across the tile seams).
//
// Labelling: union-find on 32-bit parents.  parent[v] = v; unions over the edges; one pass reads root of v.  Three invariants
// hold at every instant, whatever the interleaving:
//   (1) parent[x] <= x, with equality exactly at roots: every chain strictly descends, so it ends and no cycle can form;
//   (2) a non-root never becomes a root again: the only write to a root is the compare-and-swap that hooks it, and path
//       splitting writes to x only after it has seen parent[x] != x;
//   (3) every write stores a vertex of the same tree: a union hooks the larger root under a vertex of the other tree of
//       the edge it was given, path splitting stores a former ancestor.
// A stale read therefore still yields a vertex of the right tree and only costs steps.  By (1) the root of a tree is its
// smallest index, and a union returns only when both ends have one root or its own compare-and-swap has hooked one under
// the other, so after the pass the trees are the components and the labels are their minima -- which thread won which
// compare-and-swap changes the shape of the trees in between, never the result.
// Nothing waits: a failed compare-and-swap means another thread has hooked that very root in the meantime (progress), the
// loser goes on from the value it got back, which is strictly smaller; there is no flag, no barrier across workgroups and no
// cooperative launch.
// A caller may start from any forest that satisfies (1) -- (3) instead of parent[v] = v (mf_regions.hip starts the global pass
// from the tiles' local results), and `parent` may live in LDS: the accesses are generic.
//
// Counts are integer atomic adds (sums do not depend on their order), first reduced across the lanes of a wave that hit
// the same label and, for the label most of the wave shares, across the wave's whole share of the input: an input that is one
// big component would otherwise send every add to one address.
#pragma once
#include <hip/hip_runtime.h>

namespace mf {
namespace uf {

// parents are read and written by many workgroups at once: relaxed agent-scope accesses (served by L2, never a stale L1 line
// for good), the hook itself is a compare-and-swap
__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; path splitting on the way: every visited vertex is re-pointed at its grandparent
__device__ __forceinline__ int find_root(int* parent, int x) {
  int p = ld(parent + x);
  while (p != x) {
    const int g = ld(parent + p);
    if (g == p) return p;
    st(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  int ra = find_root(parent, a), rb = find_root(parent, b);
  while (ra != rb) {
    if (ra < rb) { const int t = ra; ra = rb; rb = t; }          // hook the larger root under the smaller
    const int old = atomicCAS(parent + ra, ra, rb);
    if (old == ra) return;
    ra = find_root(parent, old);                                 // another thread hooked ra under old < ra: go on from there
    rb = find_root(parent, rb);
  }
}

// cnt[key] += 1 for every valid lane, summed on chip first: per distinct key of the wave one add of the lanes' number
// (ballot), and the key most of the wave shares is carried in a wave-uniform (key, count) pair across the trips of the
// grid-stride loop and added once at the end -- an input that is one big component sends one add per wave to the hot
// address, not one per 64 elements (returning or not, adds to one word are served one at a time).  Integer sums: the
// result does not depend on what was cached where.  Every lane of the wave calls both functions.
struct WaveCount { int key; int n; };

__device__ __forceinline__ void wave_count_flush(int* cnt, WaveCount& w) {
  if ((threadIdx.x & 63) == 0 && w.n) atomicAdd(cnt + w.key, w.n);
  w.n = 0;
}

__device__ __forceinline__ void wave_count(int* cnt, int key, bool valid, WaveCount& w) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, leader);
    const unsigned long long m = __ballot(valid && key == k);
    const int c = __popcll(m);
    if (w.n && k == w.key) {
      w.n += c;
    } else if (c > 32 || !w.n) {                                  // the wave's majority (or the first key seen) takes the pair
      wave_count_flush(cnt, w);
      w.key = k;
      w.n = c;
    } else if (lane == leader) {
      atomicAdd(cnt + k, c);
    }
    todo &= ~m;
  }
}

}  // namespace uf
}  // namespace mf
