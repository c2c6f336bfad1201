// mf_mesh_smooth.hip -- vertex adjacency and smoothing of an indexed triangle mesh on the device (include/mocoflow_hip.h:
// mf_rings_mesh_plan / mf_rings_mesh_emit, mf_smooth_mesh): the one-ring of every vertex as a CSR structure, and Laplacian /
// Taubin lambda|mu steps as a gather over it.  What a user of extract_mesh otherwise does on the host with a mesh library, after
// copying the whole mesh there.  tests/mesh_smooth_oracle.py restates both contracts in numpy.
//
// Rings.  A triangle with two equal indices is skipped, one with an index outside [0, V) is counted and never dereferenced.
// Every kept triangle (i, j, k) gives each corner its two partners: 2 raw entries per corner.
//   count   deg[v] += 2 per kept triangle of v (integer atomics)
//   scan    raw_off = the exclusive prefix of deg in vertex order (mf_scan.hpp: fixed workgroup shares, one workgroup over their
//           totals, the shares again); the vertices with more raw entries than 2 MF_MESH_MAX_TRIANGLES_PER_VERTEX are counted
//           here, the ones above kShort are listed (in any order: it is a work list, no output follows it)
//   fill    slot = raw_off[v] + (atomicSub(deg[v], 2) - 2): deg counts down to 0, no second array.  WHICH slot a partner lands in
//           depends on the order of the atomics; the multiset of a segment does not
//   sort    each segment ascending, then one pass over the runs of equal values: the distinct values move to the front of the
//           segment, their number goes to ucount[v], a run of length 1 is an edge in exactly one triangle: boundary[v].  After the
//           sort a segment is a function of its multiset alone, so the fill order shows in no output.  Segments of at most kShort
//           entries: one lane per vertex, insertion sort in a column of LDS (at most kShort^2 / 2 steps).  Longer ones: one workgroup per
//           listed vertex, a bitonic network in LDS of the next power of two (at most 4096 entries: the cap).  Neither runs when
//           the counting pass found a bad index or a vertex above the cap: no lane sorts a segment of unbounded length
//   scan    offsets = the exclusive prefix of ucount (int64, public), R = the total
//   emit    after the caller has read [bad, over_cap, R]: ring[offsets[v] + k] = segment[k], short segments one lane per vertex,
//           listed ones one workgroup each
//
// Smoothing.  A step is a gather: vertex i reads its own position and its ring's positions of the PREVIOUS step and writes the
// next buffer (Jacobi; two buffers).  Positions travel as 16-byte rows (x, y, z, flag): one dwordx4 per neighbour instead of
// three dword gathers of a 12-byte row; the flag (1.0f: the vertex does not move under boundary = fixed) rides in the fourth
// lane and costs no byte of its own.  offsets and ring are private int32 copies (R < 2^31).  One host entry packs, enqueues
// every step and unpacks; no kernel synchronises across workgroups.
#include <algorithm>
#include <climits>
#include <cmath>

#include "mf_host.hpp"
#include "mf_scan.hpp"

// s + p, s / n, m - p, f * d, p + (f d): each rounded once, as the oracle restates them (the Makefile builds every unit with
// -ffp-contract=off; the pragma keeps it true for a build that forgets it)
#pragma clang fp contract(off)

using namespace mf;

namespace mf {
namespace rg {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                 // as mf_mesh_components.hip: the grid stops growing at 8 waves per SIMD of 256 CUs
constexpr int kShort = 32;                       // raw entries a single lane sorts (kIndexLimit, mf_shares.hpp, bounds V and 6 T)
constexpr int kMaxRaw = 2 * MF_MESH_MAX_TRIANGLES_PER_VERTEX;   // raw entries of a vertex at the cap: the LDS of the long path
static_assert(kMaxRaw == 4096 && (kMaxRaw & (kMaxRaw - 1)) == 0, "the bitonic network sorts a power of two");

inline unsigned grid_for(long long n) { return (unsigned)capped_blocks(n, kThreads, kMaxBlocks, 1); }

struct Params {
  const long long* tris; long long T, V;
  long long* counts;            // [bad, over_cap, R]
  int* hdr;                     // [0]: listed vertices
  int* deg;                     // [V] raw entries; the fill counts it down to 0
  int* raw_off;                 // [V + 1]
  int* ucount;                  // [V] distinct neighbours
  long long* blk;               // [kMaxBlocks] totals of the shares, then their exclusive prefix
  int* list; long long list_cap;
  int* raw;                     // [6 T]
  long long* offsets;           // [V + 1] public
  Share sv;                     // contiguous shares of the vertices: the prefix follows the vertex order
  unsigned char* boundary;      // [V] public
  long long* ring; long long R; // emit
};

// the three corners of triangle t; false: skipped (two equal indices) or bad (an index outside [0, V): `bad` is set)
__device__ __forceinline__ bool corners(const Params& p, long long t, int (&c)[3], bool& bad) {
  const long long i = p.tris[3 * t], j = p.tris[3 * t + 1], k = p.tris[3 * t + 2];
  bad = !(in_range(i, p.V) && in_range(j, p.V) && in_range(k, p.V));
  if (bad || i == j || j == k || i == k) return false;
  c[0] = (int)i; c[1] = (int)j; c[2] = (int)k;
  return true;
}

__global__ __launch_bounds__(kThreads) void ring_count_kernel(const Params p) {
  long long nbad = 0;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < p.T; t += (long long)gridDim.x * kThreads) {
    int c[3]; bool bad;
    const bool ok = corners(p, t, c, bad);
    nbad += bad;
    if (!ok) continue;
    atomicAdd(p.deg + c[0], 2); atomicAdd(p.deg + c[1], 2); atomicAdd(p.deg + c[2], 2);
  }
  wave_add(p.counts, nbad);
}

// phase 0 scans deg into raw_off, phase 1 scans ucount into offsets
__global__ __launch_bounds__(kThreads) void ring_sum_kernel(const Params p, const int phase) {
  const int* vals = phase ? p.ucount : p.deg;
  long long lo, hi, n = 0, over = 0;
  share_range(p.sv.per, p.V, lo, hi);
  for (long long v = lo + threadIdx.x; v < hi; v += kThreads) {
    const int d = vals[v];
    n += d;
    over += !phase && d > kMaxRaw;
  }
  n = block_sum_i64<kThreads>(n);
  if (threadIdx.x == 0) p.blk[blockIdx.x] = n;
  if (!phase) wave_add(p.counts + 1, over);
}

// one workgroup: the exclusive prefix of the shares' totals in place, and the grand total behind the last vertex
__global__ __launch_bounds__(kThreads) void ring_top_kernel(const Params p, const int phase) {
  long long total[1];
  scan_totals<kThreads, 1>(p.blk, p.sv.nblocks, p.blk, total);
  if (threadIdx.x == 0) {
    if (phase) { p.offsets[p.V] = total[0]; p.counts[2] = total[0]; }
    else p.raw_off[p.V] = (int)total[0];                                   // <= 6 T < 2^31
  }
}

__global__ __launch_bounds__(kThreads) void ring_prefix_kernel(const Params p, const int phase) {
  const int* vals = phase ? p.ucount : p.deg;
  long long lo, hi, base = p.blk[blockIdx.x];
  share_range(p.sv.per, p.V, lo, hi);
  for (long long tile = lo; tile < hi; tile += kThreads) {                 // lo, hi: the same for every thread of the workgroup
    const long long v = tile + threadIdx.x;
    const int d = v < hi ? vals[v] : 0;
    long long wave_tot[1], front[1], tot[1];
    const long long before = wave_prefix_i64(d, wave_tot[0]);
    block_offsets<kThreads, 1>(wave_tot, front, tot);
    if (v < hi) {
      const long long at = base + front[0] + before;
      if (phase) p.offsets[v] = at;
      else {
        p.raw_off[v] = (int)at;
        if (d > kShort) {                                                  // the order of the list is free: nothing follows it
          const int slot = atomicAdd(p.hdr, 1);
          if (slot < p.list_cap) p.list[slot] = (int)v;
        }
      }
    }
    base += tot[0];
    __syncthreads();                                                       // block_offsets' LDS is rewritten by the next tile
  }
}

__global__ __launch_bounds__(kThreads) void ring_fill_kernel(const Params p) {
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < p.T; t += (long long)gridDim.x * kThreads) {
    int c[3]; bool bad;
    if (!corners(p, t, c, bad)) continue;                                  // the triangles the counting pass kept, no other
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int v = c[a];
      const int left = atomicSub(p.deg + v, 2) - 2;                        // 0 .. deg - 2: the counting pass made room for it
      const long long at = (long long)p.raw_off[v] + left;
      if (left >= 0 && at + 1 < 6 * p.T) { p.raw[at] = c[(a + 1) % 3]; p.raw[at + 1] = c[(a + 2) % 3]; }
    }
  }
}

__device__ __forceinline__ bool refused(const Params& p) { return p.counts[0] != 0 || p.counts[1] != 0; }

// segments of at most kShort raw entries, one lane per vertex.  The lane's segment is sorted in a column of LDS of its own
// (entry k of thread t at seg[k kThreads + t]: every lane of a wave is on its own bank whatever its k), not in global memory,
// where each step of the insertion sort would wait for the one before it at the latency of the L2
__global__ __launch_bounds__(kThreads) void ring_short_kernel(const Params p) {
  __shared__ int seg[kShort * kThreads];
  int* a = seg + threadIdx.x;
  const bool stop = refused(p);
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < p.V; v += (long long)gridDim.x * kThreads) {
    if (stop) { p.ucount[v] = 0; p.boundary[v] = 0; continue; }
    const int lo = p.raw_off[v], n = p.raw_off[v + 1] - lo;
    if (n > kShort) continue;                                              // the long kernel's
    int* g = p.raw + lo;
    for (int i = 0; i < n; ++i) a[i * kThreads] = g[i];
    for (int i = 1; i < n; ++i) {
      const int x = a[i * kThreads];
      int j = i - 1;
      while (j >= 0 && a[j * kThreads] > x) { a[(j + 1) * kThreads] = a[j * kThreads]; --j; }
      a[(j + 1) * kThreads] = x;
    }
    int u = 0;
    bool single = false;
    for (int k = 0; k < n;) {
      const int x = a[k * kThreads];
      int r = 1;
      while (k + r < n && a[(k + r) * kThreads] == x) ++r;
      g[u++] = x;                                                          // the distinct values, at the front of the segment
      single |= r == 1;
      k += r;
    }
    p.ucount[v] = u;
    p.boundary[v] = single;
  }
}

// listed segments, one workgroup per vertex: kShort < n <= kMaxRaw raw entries through LDS
__global__ __launch_bounds__(kThreads) void ring_long_kernel(const Params p) {
  __shared__ int buf[kMaxRaw];
  if (refused(p)) return;                                                  // the same for every thread
  const long long listed = min((long long)p.hdr[0], p.list_cap);
  for (long long e = blockIdx.x; e < listed; e += gridDim.x) {             // e, v, n, P: the same for the whole workgroup
    const int v = p.list[e];
    const int lo = p.raw_off[v], n = p.raw_off[v + 1] - lo;
    if (n > kMaxRaw || n <= kShort) continue;                              // never: the cap was checked, the list holds long ones
    int P = 64;
    while (P < n) P <<= 1;
    int* a = p.raw + lo;
    for (int i = threadIdx.x; i < P; i += kThreads) buf[i] = i < n ? a[i] : INT_MAX;     // an index is below 2^31 - 1
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int i = threadIdx.x; i < P; i += kThreads) {
          const int o = i ^ j;
          if (o > i) {
            const int x = buf[i], y = buf[o];
            if ((x > y) == ((i & k) == 0)) { buf[i] = y; buf[o] = x; }
          }
        }
      }
    }
    __syncthreads();
    int base = 0, single = 0;
    for (int tile = 0; tile < n; tile += kThreads) {
      const int i = tile + threadIdx.x;
      const bool head = i < n && (i == 0 || buf[i] != buf[i - 1]);
      single |= head && (i == n - 1 || buf[i + 1] != buf[i]);
      int wave_tot[1], front[1], tot[1];
      const int before = wave_rank(head, wave_tot[0]);
      block_offsets<kThreads, 1>(wave_tot, front, tot);
      if (head) a[base + front[0] + before] = buf[i];                      // the segment was read into LDS before the first write
      base += tot[0];
      __syncthreads();
    }
    single = __syncthreads_or(single);
    if (threadIdx.x == 0) { p.ucount[v] = base; p.boundary[v] = single != 0; }
    __syncthreads();                                                       // buf is rewritten by the next vertex
  }
}

__global__ __launch_bounds__(kThreads) void ring_emit_kernel(const Params p) {
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < p.V; v += (long long)gridDim.x * kThreads) {
    const int lo = p.raw_off[v], n = p.raw_off[v + 1] - lo;
    if (n > kShort) continue;
    const long long at = p.offsets[v];
    const int u = (int)min(p.offsets[v + 1] - at, (long long)n);         // offsets are the caller's: nothing beyond the segment is read
    for (int k = 0; k < u; ++k)
      if (in_range(at + k, p.R)) p.ring[at + k] = p.raw[lo + k];            // R is the caller's: nothing beyond it is written
  }
}

__global__ __launch_bounds__(kThreads) void ring_emit_long_kernel(const Params p) {
  const long long listed = min((long long)p.hdr[0], p.list_cap);
  for (long long e = blockIdx.x; e < listed; e += gridDim.x) {
    const int v = p.list[e];
    const int lo = p.raw_off[v], n = p.raw_off[v + 1] - lo;
    const long long at = p.offsets[v];
    const int u = (int)min(p.offsets[v + 1] - at, (long long)n);
    for (int k = threadIdx.x; k < u; k += kThreads)
      if (in_range(at + k, p.R)) p.ring[at + k] = p.raw[lo + k];
  }
}

// scratch: hdr int32 [4] | deg int32 [V] | raw_off int32 [V + 1] | ucount int32 [V] | blk int64 [kMaxBlocks] | list int32 [L] |
// raw int32 [6 T]; L = min(V, 6 T / (kShort + 1) + 1): a listed vertex owns more than kShort of the 6 T raw entries
struct Scratch { int* hdr; int* deg; int* raw_off; int* ucount; long long* blk; int* list; long long list_cap; int* raw; long long bytes; };

inline Scratch scratch_of(void* scratch, long long V, long long T) {
  Carver c(scratch);
  Scratch s;
  s.list_cap = std::min(V, 6 * T / (kShort + 1) + 1);
  s.hdr = c.take<int>(4);
  s.deg = c.take<int>(V);
  s.raw_off = c.take<int>(V + 1);
  s.ucount = c.take<int>(V);
  s.blk = c.take<long long>(kMaxBlocks);
  s.list = c.take<int>(s.list_cap);
  s.raw = c.take<int>(6 * T);
  s.bytes = c.bytes();
  return s;
}

int shape(const char* what, int64_t V, int64_t T) {
  if (const int rc = mesh_index_shape(what, V, T); rc != MF_OK) return rc;
  if (6 * T >= kIndexLimit)
    return fail(MF_E_INVALID, "%s: V=%lld T=%lld (32-bit indexing: V and 6 T in [0, 2^31))", what, (long long)V, (long long)T);
  return MF_OK;
}

Params params_of(const Scratch& sc, const int64_t* tris, int64_t T, int64_t V) {
  Params p{};
  p.tris = reinterpret_cast<const long long*>(tris); p.T = T; p.V = V;
  p.hdr = sc.hdr; p.deg = sc.deg; p.raw_off = sc.raw_off; p.ucount = sc.ucount; p.blk = sc.blk;
  p.list = sc.list; p.list_cap = sc.list_cap; p.raw = sc.raw;
  p.sv = share_of(V, kThreads, kMaxBlocks);
  return p;
}

// ---------------------------------------------------------------------------------------------------------------- smoothing
struct Smooth {
  const float* verts; long long V;
  const long long* offsets; const long long* ring; long long R;
  const unsigned char* boundary;              // null: every vertex with a ring moves
  float4* a; float4* b; int* off32; int* ring32;
  float* out;
};

// the private copies.  offsets are clamped into [0, R] and a ring entry outside [0, V) becomes 0: a `rings` argument that is no
// vertex_rings result gives positions that mean nothing, never an address outside the buffers
__global__ __launch_bounds__(kThreads) void smooth_pack_kernel(const Smooth s) {
  const long long start = (long long)blockIdx.x * kThreads + threadIdx.x, step = (long long)gridDim.x * kThreads;
  for (long long v = start; v < s.V; v += step) {
    const float fixed = s.boundary && s.boundary[v] ? 1.f : 0.f;
    s.a[v] = make_float4(s.verts[3 * v], s.verts[3 * v + 1], s.verts[3 * v + 2], fixed);
  }
  for (long long v = start; v <= s.V; v += step) {
    const long long o = s.offsets[v];
    s.off32[v] = (int)(o < 0 ? 0 : o > s.R ? s.R : o);
  }
  for (long long e = start; e < s.R; e += step) {
    const long long j = s.ring[e];
    s.ring32[e] = in_range(j, s.V) ? (int)j : 0;
  }
}

// One Jacobi step with factor f.  Per component: s = p[j0]; s = s + p[jk] in ring order; m = s / float(n); d = m - p_i;
// p_i' = p_i + f d.  A vertex that does not move (no ring, or flagged) is copied as it is.
__global__ __launch_bounds__(kThreads) void smooth_step_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                               const int* __restrict__ off, const int* __restrict__ ring,
                                                               const long long V, const float f) {
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < V; v += (long long)gridDim.x * kThreads) {
    float4 p = src[v];
    const int lo = off[v], hi = off[v + 1];
    if (hi > lo && p.w == 0.f) {
      const float4 q0 = src[ring[lo]];
      float sx = q0.x, sy = q0.y, sz = q0.z;
#pragma unroll 4
      for (int k = lo + 1; k < hi; ++k) {
        const float4 q = src[ring[k]];
        sx = sx + q.x; sy = sy + q.y; sz = sz + q.z;
      }
      const float n = (float)(hi - lo);
      const float dx = sx / n - p.x, dy = sy / n - p.y, dz = sz / n - p.z;
      const float ex = f * dx, ey = f * dy, ez = f * dz;
      p.x = p.x + ex; p.y = p.y + ey; p.z = p.z + ez;
    }
    dst[v] = p;
  }
}

__global__ __launch_bounds__(kThreads) void smooth_unpack_kernel(const float4* __restrict__ src, float* __restrict__ out, const long long V) {
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < V; v += (long long)gridDim.x * kThreads) {
    const float4 p = src[v];
    out[3 * v] = p.x; out[3 * v + 1] = p.y; out[3 * v + 2] = p.z;
  }
}

struct SmoothScratch { float4* a; float4* b; int* off32; int* ring32; long long bytes; };

inline SmoothScratch smooth_scratch_of(void* scratch, long long V, long long R) {
  Carver c(scratch);
  SmoothScratch s;
  s.a = c.take<float4>(V);
  s.b = c.take<float4>(V);
  s.off32 = c.take<int>(V + 1);
  s.ring32 = c.take<int>(R);
  s.bytes = c.bytes();
  return s;
}

int smooth_shape(const char* what, int64_t V, int64_t R) {
  if (V < 0 || R < 0 || V >= kIndexLimit || R >= kIndexLimit)
    return fail(MF_E_INVALID, "%s: V=%lld R=%lld (32-bit indexing: both in [0, 2^31))", what, (long long)V, (long long)R);
  return MF_OK;
}

}  // namespace rg
}  // namespace mf

using namespace mf::rg;

extern "C" int64_t mf_rings_mesh_scratch_bytes(int64_t V, int64_t T) {
  const int rc = shape("mf_rings_mesh_scratch_bytes", V, T);
  return rc != MF_OK ? rc : scratch_of(nullptr, V, T).bytes;
}

extern "C" int32_t mf_rings_mesh_plan(const int64_t* tris, int64_t T, int64_t V, int64_t* counts, int64_t* offsets, uint8_t* boundary,
                                      void* scratch, void* stream) {
  const char* what = "mf_rings_mesh_plan";
  const int rc = shape(what, V, T);
  if (rc != MF_OK) return rc;
  if (!counts || !offsets) return fail(MF_E_INVALID, "%s: counts or offsets is null", what);
  if (T > 0 && !tris) return fail(MF_E_INVALID, "%s: tris is null", what);
  if (V > 0 && !boundary) return fail(MF_E_INVALID, "%s: boundary is null", what);
  if (V > 0 && T > 0 && !scratch) return fail(MF_E_INVALID, "%s: scratch is null", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 24, s) != hipSuccess) return fail(MF_E_LAUNCH, "%s: hipMemsetAsync failed", what);
  if (V == 0 || T == 0) {                                                  // every ring is empty; with V = 0 every triangle is bad
    if (hipMemsetAsync(offsets, 0, (size_t)(8 * (V + 1)), s) != hipSuccess || (V > 0 && hipMemsetAsync(boundary, 0, (size_t)V, s) != hipSuccess))
      return fail(MF_E_LAUNCH, "%s: hipMemsetAsync failed", what);
    if (T == 0) return MF_OK;
    Params p{};
    p.tris = reinterpret_cast<const long long*>(tris); p.T = T; p.V = 0;
    p.counts = reinterpret_cast<long long*>(counts);
    hipLaunchKernelGGL(ring_count_kernel, dim3(grid_for(T)), dim3(kThreads), 0, s, p);   // V = 0: deg is never touched
    return check_launch(what);
  }
  const Scratch sc = scratch_of(scratch, V, T);
  Params p = params_of(sc, tris, T, V);
  p.counts = reinterpret_cast<long long*>(counts);
  p.offsets = reinterpret_cast<long long*>(offsets); p.boundary = boundary;
  if (hipMemsetAsync(sc.hdr, 0, (size_t)(16 + align_up(4 * V, 16)), s) != hipSuccess)   // hdr and deg lie together
    return fail(MF_E_LAUNCH, "%s: hipMemsetAsync failed", what);
  const dim3 threads(kThreads), shares((unsigned)p.sv.nblocks);
  hipLaunchKernelGGL(ring_count_kernel, dim3(grid_for(T)), threads, 0, s, p);
  hipLaunchKernelGGL(ring_sum_kernel, shares, threads, 0, s, p, 0);
  hipLaunchKernelGGL(ring_top_kernel, dim3(1), threads, 0, s, p, 0);
  hipLaunchKernelGGL(ring_prefix_kernel, shares, threads, 0, s, p, 0);
  hipLaunchKernelGGL(ring_fill_kernel, dim3(grid_for(T)), threads, 0, s, p);
  hipLaunchKernelGGL(ring_short_kernel, dim3(grid_for(V)), threads, 0, s, p);
  hipLaunchKernelGGL(ring_long_kernel, dim3(grid_for(sc.list_cap * kThreads)), threads, 0, s, p);
  hipLaunchKernelGGL(ring_sum_kernel, shares, threads, 0, s, p, 1);
  hipLaunchKernelGGL(ring_top_kernel, dim3(1), threads, 0, s, p, 1);
  hipLaunchKernelGGL(ring_prefix_kernel, shares, threads, 0, s, p, 1);
  return check_launch(what);
}

extern "C" int32_t mf_rings_mesh_emit(int64_t V, int64_t T, int64_t R, void* scratch, const int64_t* offsets, int64_t* ring, void* stream) {
  const char* what = "mf_rings_mesh_emit";
  const int rc = shape(what, V, T);
  if (rc != MF_OK) return rc;
  if (R < 0 || R > 6 * T) return fail(MF_E_INVALID, "%s: R=%lld of at most 6 T=%lld", what, (long long)R, (long long)(6 * T));
  if (R == 0) return MF_OK;
  if (!scratch || !offsets || !ring) return fail(MF_E_INVALID, "%s: null argument", what);
  const Scratch sc = scratch_of(scratch, V, T);
  Params p = params_of(sc, nullptr, T, V);
  p.offsets = const_cast<long long*>(reinterpret_cast<const long long*>(offsets));
  p.ring = reinterpret_cast<long long*>(ring); p.R = R;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ring_emit_kernel, dim3(grid_for(V)), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(ring_emit_long_kernel, dim3(grid_for(sc.list_cap * kThreads)), dim3(kThreads), 0, s, p);
  return check_launch(what);
}

extern "C" int64_t mf_smooth_mesh_scratch_bytes(int64_t V, int64_t R) {
  const int rc = smooth_shape("mf_smooth_mesh_scratch_bytes", V, R);
  return rc != MF_OK ? rc : smooth_scratch_of(nullptr, V, R).bytes;
}

extern "C" int32_t mf_smooth_mesh(const float* verts, int64_t V, const int64_t* offsets, const int64_t* ring, int64_t R,
                                  const uint8_t* boundary, int32_t iterations, float lam, float mu, int32_t taubin, float* out,
                                  void* scratch, void* stream) {
  const char* what = "mf_smooth_mesh";
  const int rc = smooth_shape(what, V, R);
  if (rc != MF_OK) return rc;
  if (iterations < 0 || iterations > (1 << 20)) return fail(MF_E_INVALID, "%s: iterations=%d (0 .. 2^20)", what, iterations);
  if (!std::isfinite(lam) || (taubin && !std::isfinite(mu))) return fail(MF_E_INVALID, "%s: lam=%g mu=%g (finite factors)", what, lam, mu);
  if (V == 0) return MF_OK;
  if (!verts || !out) return fail(MF_E_INVALID, "%s: verts or out is null", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (iterations == 0 || R == 0) {                                         // no step, or no vertex with a ring: a copy
    if (hipMemcpyAsync(out, verts, (size_t)(12 * V), hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(MF_E_LAUNCH, "%s: hipMemcpyAsync failed", what);
    return MF_OK;
  }
  if (!offsets || !ring || !scratch) return fail(MF_E_INVALID, "%s: offsets, ring or scratch is null", what);
  const SmoothScratch sc = smooth_scratch_of(scratch, V, R);
  Smooth m{};
  m.verts = verts; m.V = V;
  m.offsets = reinterpret_cast<const long long*>(offsets); m.ring = reinterpret_cast<const long long*>(ring); m.R = R;
  m.boundary = boundary;
  m.a = sc.a; m.b = sc.b; m.off32 = sc.off32; m.ring32 = sc.ring32; m.out = out;
  const dim3 threads(kThreads), grid(grid_for(V));
  hipLaunchKernelGGL(smooth_pack_kernel, dim3(grid_for(std::max<long long>(V + 1, R))), threads, 0, s, m);
  float4 *src = sc.a, *dst = sc.b;
  const int steps = taubin ? 2 * iterations : iterations;
  for (int k = 0; k < steps; ++k) {
    const float f = taubin && (k & 1) ? mu : lam;
    hipLaunchKernelGGL(smooth_step_kernel, grid, threads, 0, s, src, dst, sc.off32, sc.ring32, (long long)V, f);
    std::swap(src, dst);
  }
  hipLaunchKernelGGL(smooth_unpack_kernel, grid, threads, 0, s, src, out, (long long)V);
  return check_launch(what);
}
