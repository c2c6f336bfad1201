// mf_mesh_simplify.hip -- mesh simplification on the device by vertex clustering (include/mocoflow_hip.h:
// mf_simplify_mesh_plan / mf_simplify_mesh_emit): the vertices of an indexed triangle mesh are merged per cubic cell of a
// grid, triangles that collapse are dropped, triangles that become equal are kept once.  What a user of extract_mesh
// otherwise does on the host with a mesh library, after copying the whole mesh there.
//
// Contract (tests/mesh_simplify_oracle.py restates it in numpy): cell of a vertex per axis c = floor((double(v) - lo) / cell);
// a triangle is degenerate if two of its three cells are equal; two triangles are duplicates if their cell triples are equal
// up to cyclic rotation, the smallest triangle index of a class survives; survivors keep their order and their corner
// order; the new vertices are the cells a survivor names, ascending by cell id; first[k] = the smallest member of cell k;
// the mean position is summed in 2^-20 cell units as integers.  Every output is a pure function of the input.
//
// Duplicates: an open-addressing table of int32 slots that hold a TRIANGLE INDEX.  The key of a slot is recomputed from that
// triangle's three cells (a 93-bit key needs no wide compare-and-swap).  Insert probes linearly from the hash of the rotation-
// canonical triple: an empty slot is claimed by compare-and-swap; a slot whose triangle has the same key takes atomicMin of the
// index and ends the probe; any other slot is passed.  Invariant: a slot, once taken, is never empty again and the key class
// of its triangle never changes (atomicMin replaces a triangle only by one of the same class).  So what a probe has passed
// stays passed for every later probe of that class, every class settles in exactly one slot -- the first slot of its probe
// sequence that was empty or its own when one of its triangles came by -- and that slot ends as the minimum of the class,
// whoever won which compare-and-swap.  slots > T leaves an empty slot whatever happens, so every probe ends; the loop is
// bounded by `slots` as well.
//
// Ranks are mf_scan.hpp's: survivors by ballots within fixed workgroup shares; used cells by a bit mask of the cells, the
// exclusive prefix of the words' popcounts, and the popcount below the cell's bit.  Sums and minima over the members of a
// cell are integer atomics (order-free); the sums and the member count (uf::wave_count) are reduced across the wave first.
#include <climits>
#include <cmath>

#include "mf_host.hpp"
#include "mf_scan.hpp"
#include "mf_unionfind.hpp"

// t = (v - lo) / cell, (t - c) 2^20 and lo + cell (c + m / 2^20) are rounded after every operation, as the oracle restates them
// (the Makefile builds every unit with -ffp-contract=off; the pragma keeps it true for a build that forgets it)
#pragma clang fp contract(off)

using namespace mf;

namespace mf {
namespace sm {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                 // as mf_mesh_components.hip: the grid stops growing at 8 waves per SIMD of 256 CUs
constexpr int kEmpty = -1;                       // (kIndexLimit, mf_shares.hpp, bounds V, T, cells and slots)
constexpr double kFrac = 1048576.0;              // 2^20 fixed-point steps per cell

using namespace mf::uf;                          // ld, WaveCount / wave_count / wave_count_flush

inline unsigned grid_for(long long n) { return (unsigned)capped_blocks(n, kThreads, kMaxBlocks, 1); }

// sums[3 key + a] += q[a] for every valid lane, summed on chip first where lanes of the wave share the key (a mesh's vertices
// come sorted by lattice edge: neighbours share a cell): per distinct key one add per axis of the lanes' sum, as uf::wave_count
// does for counts.  A key with one lane adds directly.  Integer sums: the grouping never shows.  Every lane of the wave calls it.
__device__ __forceinline__ void wave_add3(long long* sums, int key, bool valid, const long long (&q)[3]) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {                                                         // todo, leader, k, m: the same for the whole wave
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, leader);
    const bool mine = valid && key == k;
    const unsigned long long m = __ballot(mine);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(sums + 3 * (long long)k);
    if (__popcll(m) == 1) {
      if (mine) { atomicAdd(dst, (unsigned long long)q[0]); atomicAdd(dst + 1, (unsigned long long)q[1]); atomicAdd(dst + 2, (unsigned long long)q[2]); }
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const long long s = wave_sum_i64(mine ? q[a] : 0);
        if (lane == leader) atomicAdd(dst + a, (unsigned long long)s);
      }
    }
    todo &= ~m;
  }
}

struct Grid {
  double lo[3], hi[3], cell;
  int n[3];
};

// cell and fixed-point offset of one vertex; false: not finite, or outside [lo, hi] on an axis (nothing is clamped)
__device__ __forceinline__ bool cell_of(const float* v, const Grid& g, int (&c)[3], long long (&q)[3]) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double x = (double)v[a];
    c[a] = 0; q[a] = 0;
    if (!(x >= g.lo[a] && x <= g.hi[a])) { ok = false; continue; }      // a NaN fails both
    const double t = (x - g.lo[a]) / g.cell;
    const double f = floor(t);
    if (!(f >= 0.0 && f < (double)g.n[a])) { ok = false; continue; }    // x <= hi gives f <= n - 1 (monotonic rounding): never taken
    c[a] = (int)f;
    q[a] = llrint((t - f) * kFrac);
  }
  return ok;
}

struct Params {
  const float* verts; long long V;
  const long long* tris; long long T;
  Grid g;
  long long ncells, nwords;
  unsigned slot_mask;
  int* cellid;                  // [V] cell id, -1 for a bad vertex
  int* table;                   // [slots]
  unsigned char* tflag;         // [T] survivor
  unsigned* mask;               // [nwords] bit per cell: a survivor names it
  int* wprefix;                 // [nwords] used cells in the words in front
  long long* blk_t;             // [kMaxBlocks] survivors of each workgroup's share, then their exclusive prefix
  long long* blk_w;             // [kMaxBlocks] used cells of each workgroup's share of the words, then the prefix
  Share st, sw;                 // contiguous shares of the triangles and of the words: the ranks follow the input order
  long long* counts;            // [Vk, Tk, bad]
  // emit
  long long Vk, Tk;
  long long* sums;              // [3 Vk] fixed-point sums, or null
  int* members;                 // [Vk]
  float* verts_k; long long* tris_k; long long* first; long long* cluster;
};

__global__ __launch_bounds__(kThreads) void cell_kernel(const Params p) {
  long long nbad = 0;
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < p.V; v += (long long)gridDim.x * kThreads) {
    int c[3]; long long q[3];
    const bool ok = cell_of(p.verts + 3 * v, p.g, c, q);
    p.cellid[v] = ok ? (c[0] * p.g.n[1] + c[1]) * p.g.n[2] + c[2] : -1;   // < n0 n1 n2 < 2^31
    nbad += !ok;
  }
  wave_add(p.counts + 2, nbad);
}

struct Key { int a, b, c; };
__device__ __forceinline__ bool same(const Key& x, const Key& y) { return x.a == y.a && x.b == y.b && x.c == y.c; }

// The rotation-canonical cell triple of triangle t (smallest cell first; the three are distinct, so it is unique).  false: an
// index out of range (bad_index), a bad vertex, or a degenerate triangle.
__device__ __forceinline__ bool tri_key(const Params& p, long long t, Key& k, bool& bad_index) {
  const long long i = p.tris[3 * t], j = p.tris[3 * t + 1], l = p.tris[3 * t + 2];
  bad_index = !(in_range(i, p.V) && in_range(j, p.V) && in_range(l, p.V));
  if (bad_index) return false;
  const int a = p.cellid[i], b = p.cellid[j], c = p.cellid[l];
  if (a < 0 || b < 0 || c < 0 || a == b || b == c || a == c) return false;
  if (a < b && a < c) k = Key{a, b, c};
  else if (b < c) k = Key{b, c, a};
  else k = Key{c, a, b};
  return true;
}

__device__ __forceinline__ unsigned hash_of(const Key& k) {
  unsigned h = (unsigned)k.a * 0x9E3779B1u;
  h = (h ^ (unsigned)k.b) * 0x85EBCA6Bu;
  h = (h ^ (h >> 15) ^ (unsigned)k.c) * 0xC2B2AE35u;
  h ^= h >> 13; h *= 0x27D4EB2Fu; h ^= h >> 16;
  return h;
}

__global__ __launch_bounds__(kThreads) void insert_kernel(const Params p) {
  long long nbad = 0;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < p.T; t += (long long)gridDim.x * kThreads) {
    Key k; bool bad;
    const bool ok = tri_key(p, t, k, bad);
    nbad += bad;
    if (!ok) continue;
    unsigned pos = hash_of(k) & p.slot_mask;
    for (unsigned trip = 0; trip <= p.slot_mask; ++trip, pos = (pos + 1) & p.slot_mask) {
      int s = ld(p.table + pos);                                         // an atomic load: a plain one may be hoisted out of the loop
      if (s == kEmpty) {
        s = atomicCAS(p.table + pos, kEmpty, (int)t);
        if (s == kEmpty) break;                                          // claimed
      }
      Key ks; bool b2;
      if (in_range(s, p.T) && tri_key(p, s, ks, b2) && same(ks, k)) { atomicMin(p.table + pos, (int)t); break; }
    }
  }
  wave_add(p.counts + 2, nbad);
}

// the triangle the table holds for key k: the smallest index of its class; -1 if the class is not there
__device__ __forceinline__ int lookup(const Params& p, const Key& k) {
  unsigned pos = hash_of(k) & p.slot_mask;
  for (unsigned trip = 0; trip <= p.slot_mask; ++trip, pos = (pos + 1) & p.slot_mask) {
    const int s = p.table[pos];
    if (s == kEmpty) return -1;
    Key ks; bool b2;
    if (in_range(s, p.T) && tri_key(p, s, ks, b2) && same(ks, k)) return s;
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void survive_kernel(const Params p) {
  long long lo, hi, n = 0;
  share_range(p.st.per, p.T, lo, hi);
  for (long long t = lo + threadIdx.x; t < hi; t += kThreads) {
    Key k; bool bad;
    const bool s = tri_key(p, t, k, bad) && lookup(p, k) == (int)t;
    p.tflag[t] = s;
    n += s;
    if (s) {
      atomicOr(p.mask + (k.a >> 5), 1u << (k.a & 31));
      atomicOr(p.mask + (k.b >> 5), 1u << (k.b & 31));
      atomicOr(p.mask + (k.c >> 5), 1u << (k.c & 31));
    }
  }
  n = block_sum_i64<kThreads>(n);
  if (threadIdx.x == 0) p.blk_t[blockIdx.x] = n;
}

__global__ __launch_bounds__(kThreads) void word_count_kernel(const Params p) {
  long long lo, hi, n = 0;
  share_range(p.sw.per, p.nwords, lo, hi);
  for (long long w = lo + threadIdx.x; w < hi; w += kThreads) n += __popc(p.mask[w]);
  n = block_sum_i64<kThreads>(n);
  if (threadIdx.x == 0) p.blk_w[blockIdx.x] = n;
}

// one workgroup: the exclusive prefixes of both columns of workgroup totals in place, and Vk, Tk
__global__ __launch_bounds__(kThreads) void scan_kernel(const Params p) {
  long long total[1];
  scan_totals<kThreads, 1>(p.blk_t, p.st.nblocks, p.blk_t, total);
  if (threadIdx.x == 0) p.counts[1] = total[0];
  __syncthreads();
  scan_totals<kThreads, 1>(p.blk_w, p.sw.nblocks, p.blk_w, total);
  if (threadIdx.x == 0) p.counts[0] = total[0];
}

__global__ __launch_bounds__(kThreads) void word_prefix_kernel(const Params p) {
  long long lo, hi, base = p.blk_w[blockIdx.x];
  share_range(p.sw.per, p.nwords, lo, hi);
  for (long long tile = lo; tile < hi; tile += kThreads) {               // lo, hi: the same for every thread of the workgroup
    const long long w = tile + threadIdx.x;
    const int c = w < hi ? __popc(p.mask[w]) : 0;                        // 0 .. 32: six bits
    int wave_tot[1], front[1], tot[1];
    const int before = wave_prefix_small<6>(c, wave_tot[0]);
    block_offsets<kThreads, 1>(wave_tot, front, tot);
    if (w < hi) p.wprefix[w] = (int)(base + front[0] + before);          // < Vk < 2^31
    base += tot[0];
    __syncthreads();                                                     // block_offsets' LDS is rewritten by the next tile
  }
}

// the new index of cell `cid`, -1 if no survivor names it (or cid is no cell)
__device__ __forceinline__ long long rank_of(const Params& p, int cid) {
  if (!in_range(cid, p.ncells)) return -1;
  const unsigned m = p.mask[cid >> 5], bit = 1u << (cid & 31);
  if (!(m & bit)) return -1;
  const long long r = (long long)p.wprefix[cid >> 5] + __popc(m & (bit - 1u));
  return in_range(r, p.Vk) ? r : -1;                                     // Vk is the caller's: nothing beyond it is written
}

__global__ __launch_bounds__(kThreads) void assign_kernel(const Params p) {
  WaveCount wc{0, 0};
  const long long step = (long long)gridDim.x * kThreads;
  for (long long base = (long long)blockIdx.x * kThreads; base < p.V; base += step) {   // base: the same for the whole wave
    const long long v = base + threadIdx.x;
    long long r = -1;
    long long q[3] = {0, 0, 0};
    if (v < p.V) {
      r = rank_of(p, p.cellid[v]);
      p.cluster[v] = r;
      if (r >= 0) {
        atomicMin(p.first + r, v);
        int c[3];
        if (p.sums) cell_of(p.verts + 3 * v, p.g, c, q);
      }
    }
    if (p.sums) {                                                        // wave-uniform: every lane of the wave is here
      wave_add3(p.sums, (int)r, r >= 0, q);
      wave_count(p.members, (int)r, r >= 0, wc);
    }
  }
  if (p.sums) wave_count_flush(p.members, wc);
}

__global__ __launch_bounds__(kThreads) void mean_kernel(const Params p) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < p.Vk; k += (long long)gridDim.x * kThreads) {
    const long long v = p.first[k];
    const int cid = in_range(v, p.V) ? p.cellid[v] : -1;
    const int n = p.members[k];
    if (cid < 0 || n <= 0) {                                             // a Vk that is not the plan's
      p.verts_k[3 * k] = p.verts_k[3 * k + 1] = p.verts_k[3 * k + 2] = 0.f;
      continue;
    }
    const int c2 = cid % p.g.n[2], t = cid / p.g.n[2];
    const int c[3] = {t / p.g.n[1], t % p.g.n[1], c2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double m = (double)p.sums[3 * k + a] / (double)n;
      p.verts_k[3 * k + a] = (float)(p.g.lo[a] + p.g.cell * ((double)c[a] + m / kFrac));
    }
  }
}

__global__ __launch_bounds__(kThreads) void tris_kernel(const Params p) {
  long long lo, hi, base = p.blk_t[blockIdx.x];
  share_range(p.st.per, p.T, lo, hi);
  for (long long tile = lo; tile < hi; tile += kThreads) {
    const long long t = tile + threadIdx.x;
    const bool s = t < hi && p.tflag[t] != 0;
    int wave_tot[1], front[1], tot[1];
    const int before = wave_rank(s, wave_tot[0]);
    block_offsets<kThreads, 1>(wave_tot, front, tot);
    const long long k = base + front[0] + before;
    if (s && k < p.Tk) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long i = p.tris[3 * t + c];
        p.tris_k[3 * k + c] = in_range(i, p.V) ? rank_of(p, p.cellid[i]) : -1;
      }
    }
    base += tot[0];
    __syncthreads();
  }
}

// scratch: cellid int32 [V] | tflag uint8 [T] | mask uint32 [W] | wprefix int32 [W] | blk_t, blk_w int64 [kMaxBlocks] each |
// table int32 [slots] (last: the emit step does not need it, nor its size)
struct Scratch { int* cellid; unsigned char* tflag; unsigned* mask; int* wprefix; long long* blk_t; long long* blk_w; int* table; long long bytes; };

inline Scratch scratch_of(void* scratch, long long V, long long T, long long nwords, long long slots) {
  Carver c(scratch);
  Scratch s;
  s.cellid = c.take<int>(V);
  s.tflag = c.take<unsigned char>(T);
  s.mask = c.take<unsigned>(nwords);
  s.wprefix = c.take<int>(nwords);
  s.blk_t = c.take<long long>(kMaxBlocks);
  s.blk_w = c.take<long long>(kMaxBlocks);
  s.table = c.take<int>(slots);
  s.bytes = c.bytes();
  return s;
}

int shape(const char* what, int64_t V, int64_t T, int64_t n0, int64_t n1, int64_t n2, long long& ncells) {
  if (const int rc = mesh_index_shape(what, V, T); rc != MF_OK) return rc;
  if (n0 < 1 || n1 < 1 || n2 < 1 || n0 >= kIndexLimit || n1 >= kIndexLimit || n2 >= kIndexLimit || n0 * n1 >= kIndexLimit ||
      n0 * n1 * n2 >= kIndexLimit)
    return fail(MF_E_INVALID, "%s: %lld x %lld x %lld cells (each axis at least 1, the product below 2^31)", what, (long long)n0,
                (long long)n1, (long long)n2);
  ncells = n0 * n1 * n2;
  return MF_OK;
}

int slots_ok(const char* what, int64_t slots, int64_t T) {
  if (slots < 1 || slots > kIndexLimit || (slots & (slots - 1)) != 0 || slots <= T)
    return fail(MF_E_INVALID, "%s: slots=%lld for T=%lld (a power of two above T, at most 2^31)", what, (long long)slots, (long long)T);
  return MF_OK;
}

int grid_of(const char* what, const double* lo, const double* hi, double cell, int64_t n0, int64_t n1, int64_t n2, Grid& g) {
  if (!lo || !hi) return fail(MF_E_INVALID, "%s: lo or hi is null", what);
  if (!(cell > 0.0) || !std::isfinite(cell)) return fail(MF_E_INVALID, "%s: cell=%g (a finite edge above 0)", what, cell);
  const int64_t n[3] = {n0, n1, n2};
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || hi[a] < lo[a])
      return fail(MF_E_INVALID, "%s: axis %d spans [%g, %g] (finite, hi >= lo)", what, a, lo[a], hi[a]);
    const double want = std::floor((hi[a] - lo[a]) / cell) + 1.0;
    if (want != (double)n[a])
      return fail(MF_E_INVALID, "%s: axis %d has %lld cells, floor((hi - lo) / cell) + 1 = %.0f", what, a, (long long)n[a], want);
    g.lo[a] = lo[a]; g.hi[a] = hi[a]; g.n[a] = (int)n[a];
  }
  g.cell = cell;
  return MF_OK;
}

}  // namespace sm
}  // namespace mf

using namespace mf::sm;

extern "C" int64_t mf_simplify_mesh_scratch_bytes(int64_t V, int64_t T, int64_t n0, int64_t n1, int64_t n2, int64_t slots) {
  long long ncells = 0;
  int rc = shape("mf_simplify_mesh_scratch_bytes", V, T, n0, n1, n2, ncells);
  if (rc == MF_OK) rc = slots_ok("mf_simplify_mesh_scratch_bytes", slots, T);
  return rc != MF_OK ? rc : scratch_of(nullptr, V, T, (ncells + 31) / 32, slots).bytes;
}

extern "C" int32_t mf_simplify_mesh_plan(const float* verts, int64_t V, const int64_t* tris, int64_t T, const double* lo,
                                         const double* hi, double cell, int64_t n0, int64_t n1, int64_t n2, int64_t slots,
                                         int64_t* counts, void* scratch, void* stream) {
  const char* what = "mf_simplify_mesh_plan";
  long long ncells = 0;
  int rc = shape(what, V, T, n0, n1, n2, ncells);
  if (rc == MF_OK) rc = slots_ok(what, slots, T);
  Params p{};
  if (rc == MF_OK) rc = grid_of(what, lo, hi, cell, n0, n1, n2, p.g);
  if (rc != MF_OK) return rc;
  if (!counts) return fail(MF_E_INVALID, "%s: counts is null", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 24, s) != hipSuccess) return fail(MF_E_LAUNCH, "%s: hipMemsetAsync failed", what);
  if (V == 0 && T == 0) return MF_OK;
  if (V > 0 && !verts) return fail(MF_E_INVALID, "%s: verts is null", what);
  if (T > 0 && !tris) return fail(MF_E_INVALID, "%s: tris is null", what);
  if (!scratch) return fail(MF_E_INVALID, "%s: scratch is null", what);
  const long long nwords = (ncells + 31) / 32;
  const Scratch sc = scratch_of(scratch, V, T, nwords, slots);
  p.verts = verts; p.V = V;
  p.tris = reinterpret_cast<const long long*>(tris); p.T = T;
  p.ncells = ncells; p.nwords = nwords;
  p.slot_mask = (unsigned)(slots - 1);
  p.cellid = sc.cellid; p.table = sc.table; p.tflag = sc.tflag; p.mask = sc.mask; p.wprefix = sc.wprefix;
  p.blk_t = sc.blk_t; p.blk_w = sc.blk_w;
  p.st = share_of(T, kThreads, kMaxBlocks); p.sw = share_of(nwords, kThreads, kMaxBlocks);
  p.counts = reinterpret_cast<long long*>(counts);
  if (V > 0) hipLaunchKernelGGL(cell_kernel, dim3(grid_for(V)), dim3(kThreads), 0, s, p);
  if (T == 0) return check_launch(what);                                  // no survivor: Vk = Tk = 0, the emit step launches nothing
  if (hipMemsetAsync(sc.table, 0xff, (size_t)(4 * slots), s) != hipSuccess || hipMemsetAsync(sc.mask, 0, (size_t)(4 * nwords), s) != hipSuccess)
    return fail(MF_E_LAUNCH, "%s: hipMemsetAsync failed", what);
  hipLaunchKernelGGL(insert_kernel, dim3(grid_for(T)), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(survive_kernel, dim3((unsigned)p.st.nblocks), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(word_count_kernel, dim3((unsigned)p.sw.nblocks), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(word_prefix_kernel, dim3((unsigned)p.sw.nblocks), dim3(kThreads), 0, s, p);
  return check_launch(what);
}

extern "C" int32_t mf_simplify_mesh_emit(const float* verts, int64_t V, const int64_t* tris, int64_t T, const double* lo,
                                         const double* hi, double cell, int64_t n0, int64_t n1, int64_t n2, int64_t Vk, int64_t Tk,
                                         void* scratch, void* sums, float* verts_k, int64_t* tris_k, int64_t* first,
                                         int64_t* cluster, void* stream) {
  const char* what = "mf_simplify_mesh_emit";
  long long ncells = 0;
  int rc = shape(what, V, T, n0, n1, n2, ncells);
  Params p{};
  if (rc == MF_OK) rc = grid_of(what, lo, hi, cell, n0, n1, n2, p.g);
  if (rc != MF_OK) return rc;
  if (Vk < 0 || Vk > V || Vk > ncells || Tk < 0 || Tk > T || (Vk == 0) != (Tk == 0))
    return fail(MF_E_INVALID, "%s: Vk=%lld of V=%lld in %lld cells, Tk=%lld of T=%lld", what, (long long)Vk, (long long)V, ncells,
                (long long)Tk, (long long)T);
  if (V == 0) return MF_OK;
  if (!cluster) return fail(MF_E_INVALID, "%s: cluster is null", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (Tk == 0) {                                                          // nothing kept: every vertex is dropped
    if (hipMemsetAsync(cluster, 0xff, (size_t)(8 * V), s) != hipSuccess) return fail(MF_E_LAUNCH, "%s: hipMemsetAsync failed", what);
    return MF_OK;
  }
  if (!verts || !tris || !scratch || !tris_k || !first) return fail(MF_E_INVALID, "%s: null argument", what);
  if ((verts_k != nullptr) != (sums != nullptr)) return fail(MF_E_INVALID, "%s: verts_k and sums go together (the mean placement)", what);
  const long long nwords = (ncells + 31) / 32;
  const Scratch sc = scratch_of(scratch, V, T, nwords, 0);
  p.verts = verts; p.V = V;
  p.tris = reinterpret_cast<const long long*>(tris); p.T = T;
  p.ncells = ncells; p.nwords = nwords;
  p.cellid = sc.cellid; p.tflag = sc.tflag; p.mask = sc.mask; p.wprefix = sc.wprefix; p.blk_t = sc.blk_t; p.blk_w = sc.blk_w;
  p.st = share_of(T, kThreads, kMaxBlocks); p.sw = share_of(nwords, kThreads, kMaxBlocks);
  p.Vk = Vk; p.Tk = Tk;
  p.sums = static_cast<long long*>(sums);
  p.members = sums ? reinterpret_cast<int*>(p.sums + 3 * Vk) : nullptr;
  p.verts_k = verts_k; p.tris_k = reinterpret_cast<long long*>(tris_k);
  p.first = reinterpret_cast<long long*>(first); p.cluster = reinterpret_cast<long long*>(cluster);
  if (hipMemsetAsync(first, 0x7f, (size_t)(8 * Vk), s) != hipSuccess ||                 // above every index
      (sums && hipMemsetAsync(sums, 0, (size_t)(28 * Vk), s) != hipSuccess))
    return fail(MF_E_LAUNCH, "%s: hipMemsetAsync failed", what);
  hipLaunchKernelGGL(assign_kernel, dim3(grid_for(V)), dim3(kThreads), 0, s, p);
  if (sums) hipLaunchKernelGGL(mean_kernel, dim3(grid_for(Vk)), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(tris_kernel, dim3((unsigned)p.st.nblocks), dim3(kThreads), 0, s, p);
  return check_launch(what);
}
