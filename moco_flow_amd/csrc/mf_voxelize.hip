// mf_voxelize.hip -- an occupancy bit grid from a triangle mesh (include/mocoflow_hip.h), in the layout mf_occ_build writes:
//   mf_voxel_mesh   : the cells a triangle's surface meets, decided exactly in integers on coordinates snapped to 1/64 cell
//   mf_voxel_fill   : + the empty cells that are not 6-connected, through empty cells, to the outside of the grid
//   mf_voxel_dilate : a box dilation by (rx, ry, rz) cells; optionally the occupied-cell count
// The reference labels a point "inside" iff it lies within `thickness` of a vertex of the posed SMPL mesh
// (datasets/moco_flow_dataset.py:87-142), builds the frame's AABB from that mesh (moco_flow_dataset.py:144-154) and renders every
// ray of that box's hull (trainer_moco_flow.py:226-268).  The grid of the posed mesh, filled and dilated by the thickness, is the
// region where its objective allows density at all; it needs no network and no density threshold.
// Every result is a function of integers: the surface bits are or-ed in (the order of ORs does not matter), the fill is the
// unique labelling of the components of the empty cells, the dilation writes each word from one lane; the count goes through
// mf_reduce.hpp.  Bit-identical from run to run.
#include "mf_host.hpp"
#include "mf_reduce.hpp"
#include "mf_unionfind.hpp"

// u = (p - lo) * inv_cell and u * 64 are rounded after every operation, as mf_ray_clip's cell rule and tests/voxelize_oracle.py
// restate them (the Makefile builds every unit with -ffp-contract=off; the pragma keeps it true for a build that forgets it)
#pragma clang fp contract(off)

namespace mf {

constexpr int kVoxThreads = 256;
constexpr int kVoxLanesPerTri = 8;                                   // lanes that share a triangle with a small box
constexpr int kVoxTrisPerBlock = kVoxThreads / kVoxLanesPerTri;      // triangles per workgroup and trip
constexpr int kVoxMaxBlocks = 512;                                   // workgroups of the small-box pass: the rest is grid-stride
constexpr int kVoxBigMaxBlocks = 64;                                 // ... of the large-box pass: the same triangles per trip
constexpr int kVoxSmallCells = 512;                                  // a larger box goes to the whole workgroup
constexpr int kVoxClearMaxBlocks = 2048;
constexpr int kVoxSub = 64;                                          // sub-cell units per cell
constexpr int kVoxMaxSide = 1024;                                    // cells per side of mf_voxel_mesh
constexpr float kVoxSnapLo = -65536.f, kVoxSnapHi = 131072.f;        // saturation: 1024 cells below the box, 2048 above its origin

struct VoxMeshParams {
  const float* verts; int V;                                         // V and T are below 2^31
  const long long* tris; int T;
  int gx, gy, gz, wz;
  float lo[3], inv_cell[3];
  unsigned* bits;
  long long n_words;
  unsigned long long* dropped;                                       // or null
};

__global__ __launch_bounds__(kVoxThreads) void voxel_clear_kernel(unsigned* bits, long long n_words, unsigned long long* dropped,
                                                                   unsigned long long dropped0) {
  for (long long i = (long long)blockIdx.x * kVoxThreads + threadIdx.x; i < n_words; i += (long long)gridDim.x * kVoxThreads) bits[i] = 0u;
  if (dropped && blockIdx.x == 0 && threadIdx.x == 0) *dropped = dropped0;
}

__device__ __forceinline__ bool vox_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN and inf

// q = rint(((p - lo) * inv_cell) * 64), saturated; p is finite, so nothing here is NaN (an overflow to inf saturates)
__device__ __forceinline__ int vox_snap(float p, float lo, float inv) {
  float s = ((p - lo) * inv) * (float)kVoxSub;
  s = s <= kVoxSnapHi ? s : kVoxSnapHi;
  s = s >= kVoxSnapLo ? s : kVoxSnapLo;
  return (int)rintf(s);
}

// What a triangle's cell tests need (Schwarz and Seidel's conservative test, in exact integers).  BOUND: snapped coordinates lie
// in [-2^16, 2^17], so edge differences are below 2^18 and the components of n = e0 x e1 below 2^37; box corners lie in
// [0, 2^16], so n . (corner - v0) is below 3 * 2^37 * 2^18 < 2^57 and every sum below fits int64 with room to spare.  The 2-D
// edge functions stay below 2^18 * 2^18 * 2 + 2^25 < 2^38.
struct VoxTri {
  long long n[3];                  // integer normal
  long long d_lo, d_hi;            // plane: with t = n . p (p the box's min corner) the box meets the plane iff t + d_lo <= 0 <= t + d_hi
  int mu[3][3], mv[3][3];          // per dropped axis a and edge i: the inward 2-D edge normal in the plane (a+1, a+2)
  long long c[3][3];               // ... and its constant: the box meets the edge's half-plane iff mu p_u + mv p_v + c >= 0
  int c0[3], nc[3];                // first cell and number of cells of the clipped bounding box
};

// false: the triangle sets nothing; `dropped` then tells whether it was skipped (bad index, non-finite vertex, zero normal) or
// merely lies outside the grid
__device__ __forceinline__ bool vox_setup(const VoxMeshParams& p, int t, VoxTri& s, bool& dropped) {
  dropped = true;
  long long idx[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    idx[c] = p.tris[3ll * t + c];
    if (idx[c] < 0 || idx[c] >= p.V) return false;                   // never used as an address
  }
  int q[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = p.verts[3 * idx[c] + a];
      if (!vox_finite(v)) return false;
      q[c][a] = vox_snap(v, p.lo[a], p.inv_cell[a]);
    }
  int e[3][3];                                                       // edge i: from corner i to corner i + 1
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int a = 0; a < 3; ++a) e[i][a] = q[(i + 1) % 3][a] - q[i][a];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
    s.n[a] = (long long)e[0][u] * e[1][v] - (long long)e[0][v] * e[1][u];
  }
  if (s.n[0] == 0 && s.n[1] == 0 && s.n[2] == 0) return false;
  dropped = false;
  const int g[3] = {p.gx, p.gy, p.gz};
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int mn = min(q[0][a], min(q[1][a], q[2][a])), mx = max(q[0][a], max(q[1][a], q[2][a]));
    int first = ((mn + kVoxSub - 1) >> 6) - 1, last = mx >> 6;       // closed boxes [64 i, 64 i + 64] that meet [mn, mx]
    first = first < 0 ? 0 : first;
    last = last > g[a] - 1 ? g[a] - 1 : last;
    s.c0[a] = first;
    s.nc[a] = last - first + 1;
    inside = inside && last >= first;
  }
  if (!inside) return false;
  long long nv0 = 0, up = 0, down = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    nv0 += s.n[a] * q[0][a];
    up += s.n[a] > 0 ? s.n[a] * kVoxSub : 0;
    down += s.n[a] < 0 ? s.n[a] * kVoxSub : 0;
  }
  s.d_lo = down - nv0;
  s.d_hi = up - nv0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
    const int sgn = s.n[a] >= 0 ? 1 : -1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int mu = -e[i][v] * sgn, mv = e[i][u] * sgn;
      s.mu[a][i] = mu;
      s.mv[a][i] = mv;
      s.c[a][i] = -((long long)mu * q[i][u] + (long long)mv * q[i][v]) + (long long)kVoxSub * ((mu > 0 ? mu : 0) + (mv > 0 ? mv : 0));
    }
  }
  return true;
}

// the closed triangle meets the closed box whose min corner is cell (ci, cj, ck); the box is inside the bounding box already
__device__ __forceinline__ bool vox_hit(const VoxTri& s, int ci, int cj, int ck) {
  const int pc[3] = {ci * kVoxSub, cj * kVoxSub, ck * kVoxSub};
  const long long t = s.n[0] * pc[0] + s.n[1] * pc[1] + s.n[2] * pc[2];
  bool hit = t + s.d_lo <= 0 && t + s.d_hi >= 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) hit = hit && (long long)s.mu[a][i] * pc[u] + (long long)s.mv[a][i] * pc[v] + s.c[a][i] >= 0;
  }
  return hit;
}

// lanes first, first + step, ... of the cells of the triangle's box, z fastest
__device__ __forceinline__ void vox_walk(const VoxMeshParams& p, const VoxTri& s, unsigned first, unsigned step) {
  const unsigned ny = (unsigned)s.nc[1], nz = (unsigned)s.nc[2], n = (unsigned)s.nc[0] * ny * nz;   // below 2^31: the grid is
  for (unsigned c = first; c < n; c += step) {
    const unsigned r = c / nz;
    const int ck = s.c0[2] + (int)(c - r * nz), cj = s.c0[1] + (int)(r % ny), ci = s.c0[0] + (int)(r / ny);
    if (vox_hit(s, ci, cj, ck)) atomicOr(p.bits + ((long long)ci * p.gy + cj) * p.wz + (ck >> 5), 1u << (ck & 31));
  }
}

__device__ __forceinline__ unsigned vox_cells(const VoxTri& s) { return (unsigned)s.nc[0] * (unsigned)s.nc[1] * (unsigned)s.nc[2]; }

// the triangle sets cells and its box is one of the large ones (the same decision as the small pass makes: the same set-up)
__device__ __forceinline__ bool vox_is_big(const VoxMeshParams& p, int t) {
  VoxTri s;
  bool dropped;
  return vox_setup(p, t, s, dropped) && vox_cells(s) > (unsigned)kVoxSmallCells;
}

// Small boxes: a workgroup takes kVoxTrisPerBlock triangles per trip, kVoxLanesPerTri lanes each (an SMPL triangle at 128^3 meets
// a handful of cells: one lane per triangle would leave the wave waiting for its largest box).  A triangle whose box holds more
// than kVoxSmallCells cells is left to voxel_surface_big_kernel.  This kernel counts the skipped triangles.
__global__ __launch_bounds__(kVoxThreads) void voxel_surface_kernel(const VoxMeshParams p) {
  const int sub = threadIdx.x % kVoxLanesPerTri, slot = threadIdx.x / kVoxLanesPerTri;
  const int chunks = (int)(((long long)p.T + kVoxTrisPerBlock - 1) / kVoxTrisPerBlock);
  for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    const long long t = (long long)chunk * kVoxTrisPerBlock + slot;
    if (t >= p.T) continue;
    VoxTri s;
    bool dropped;
    if (vox_setup(p, (int)t, s, dropped)) {
      if (vox_cells(s) <= (unsigned)kVoxSmallCells) vox_walk(p, s, sub, kVoxLanesPerTri);
    } else if (dropped && sub == 0 && p.dropped) {
      atomicAdd(p.dropped, 1ull);                                    // an integer sum: any order
    }
  }
}

// Large boxes: a workgroup looks at kVoxThreads triangles per trip, one lane each, lists those with a large box in LDS, and then
// walks every listed box with all its lanes: one triangle across the grid is walked by 256 lanes, not by one.
__global__ __launch_bounds__(kVoxThreads) void voxel_surface_big_kernel(const VoxMeshParams p) {
  __shared__ int big[kVoxThreads];
  __shared__ int n_big;
  const int chunks = (int)(((long long)p.T + kVoxThreads - 1) / kVoxThreads);
  for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
    if (threadIdx.x == 0) n_big = 0;
    __syncthreads();
    const long long t = (long long)chunk * kVoxThreads + threadIdx.x;
    if (t < p.T && vox_is_big(p, (int)t)) big[atomicAdd(&n_big, 1)] = (int)t;
    __syncthreads();
    const int nb = n_big;
    for (int b = 0; b < nb; ++b) {
      VoxTri s;
      bool dropped;
      if (vox_setup(p, big[b], s, dropped)) vox_walk(p, s, threadIdx.x, kVoxThreads);
    }
    __syncthreads();                                                 // the list is read: the next trip may reset it
  }
}

// ---- words of a grid, one lane each ----
struct VoxWord {
  long long row; int w, i, j, k0;
  unsigned vmask;                  // the word's bits that are cells
  long long cell0;                 // linear cell index (i gy + j) gz + k0 of bit 0
};

__device__ __forceinline__ VoxWord vox_word(long long wi, int gy, int gz, int wz) {
  VoxWord v;
  v.w = (int)(wi % wz);
  v.row = wi / wz;
  v.j = (int)(v.row % gy);
  v.i = (int)(v.row / gy);
  v.k0 = v.w * 32;
  const int left = gz - v.k0;
  v.vmask = left < 32 ? (1u << left) - 1u : 0xffffffffu;
  v.cell0 = v.row * gz + v.k0;
  return v;
}

// the lowest run of consecutive set bits of e (e != 0): its mask; s = its first bit
__device__ __forceinline__ unsigned vox_run(unsigned e, int& s) {
  s = __ffs((int)e) - 1;
  return e & ~(e + (1u << s));
}

struct VoxFillParams {
  const unsigned* in; unsigned* out;
  int gx, gy, gz, wz;
  long long n_words;
  int* parent;                     // node 0: the outside; node c + 1: cell c
};

// Union-find over the empty cells (mf_unionfind.hpp), node 0 standing for everything beyond the grid.  A run of empty bits inside
// one word is a tree from the start: all its cells point at its first cell, or at node 0 if the run touches the grid's border
// (a forest with parent[x] <= x whose trees are connected sets, which is what the union pass may start from).
__global__ __launch_bounds__(kVoxThreads) void voxel_fill_init_kernel(const VoxFillParams p) {
  const long long wi = (long long)blockIdx.x * kVoxThreads + threadIdx.x;
  if (wi == 0) p.parent[0] = 0;
  if (wi >= p.n_words) return;
  const VoxWord v = vox_word(wi, p.gy, p.gz, p.wz);
  const bool row_border = v.i == 0 || v.i == p.gx - 1 || v.j == 0 || v.j == p.gy - 1;
  unsigned e = ~p.in[wi] & v.vmask;
  while (e) {
    int s;
    const unsigned run = vox_run(e, s);
    const int last = s + __popc(run) - 1;
    const bool border = row_border || v.k0 + s == 0 || v.k0 + last == p.gz - 1;
    const int root = border ? 0 : (int)(v.cell0 + s + 1);
    for (int b = s; b <= last; ++b) p.parent[v.cell0 + b + 1] = root;
    e &= ~run;
  }
}

// Unions across words: the z seam between two words of a row, and towards rows (i, j + 1) and (i + 1, j) one union per run of
// bits that are empty in both words (the cells of such a run are connected inside either word already).
__global__ __launch_bounds__(kVoxThreads) void voxel_fill_union_kernel(const VoxFillParams p) {
  const long long wi = (long long)blockIdx.x * kVoxThreads + threadIdx.x;
  if (wi >= p.n_words) return;
  const VoxWord v = vox_word(wi, p.gy, p.gz, p.wz);
  const unsigned e = ~p.in[wi] & v.vmask;
  if (!e) return;
  const int node0 = (int)(v.cell0 + 1);
  if (v.w > 0 && (e & 1u) && !(p.in[wi - 1] >> 31)) uf::unite(p.parent, node0, node0 - 1);
#pragma unroll
  for (int axis = 0; axis < 2; ++axis) {
    const bool has = axis == 0 ? v.j + 1 < p.gy : v.i + 1 < p.gx;
    if (!has) continue;
    const long long dw = axis == 0 ? p.wz : (long long)p.gy * p.wz;
    const int dn = axis == 0 ? p.gz : p.gy * p.gz;                   // below 2^31: the grid has fewer cells
    const unsigned m = e & ~p.in[wi + dw];
    unsigned starts = m & ~(m << 1);
    while (starts) {
      const int s = __ffs((int)starts) - 1;
      uf::unite(p.parent, node0 + s, node0 + s + dn);
      starts &= starts - 1;
    }
  }
}

// A run of empty bits is filled iff its root is not the outside (roots are the smallest node of their tree, and the outside is 0)
__global__ __launch_bounds__(kVoxThreads) void voxel_fill_emit_kernel(const VoxFillParams p) {
  const long long wi = (long long)blockIdx.x * kVoxThreads + threadIdx.x;
  if (wi >= p.n_words) return;
  const VoxWord v = vox_word(wi, p.gy, p.gz, p.wz);
  unsigned word = p.in[wi] & v.vmask;
  unsigned e = ~word & v.vmask;
  while (e) {
    int s;
    const unsigned run = vox_run(e, s);
    if (uf::find_root(p.parent, (int)(v.cell0 + s + 1)) != 0) word |= run;
    e &= ~run;
  }
  p.out[wi] = word;
}

struct VoxDilateParams {
  const unsigned* in; unsigned* out;
  int gx, gy, gz, wz;
  long long n_words;
  int r;                           // clipped to side - 1
  int axis;                        // rows pass: 0 along x, 1 along y
  double* parts;                   // per-workgroup popcounts, or null
};

// z: bit b of word w is set iff a bit of [32 w + b - r, 32 w + b + r] is.  Inside the word: shifts by up to min(r, 31).  From a
// word d above, its LOWEST set bit a reaches furthest down: bits b >= 32 d + a - r; from a word d below, its HIGHEST set bit a
// reaches furthest up: bits b <= r - 32 d + a.  Words further than ceil(r / 32) away reach nothing.
__global__ __launch_bounds__(kVoxThreads) void voxel_dilate_z_kernel(const VoxDilateParams p) {
  const long long wi = (long long)blockIdx.x * kVoxThreads + threadIdx.x;
  if (wi >= p.n_words) return;
  const VoxWord v = vox_word(wi, p.gy, p.gz, p.wz);
  const unsigned* row = p.in + v.row * p.wz;
  const unsigned x = row[v.w];
  unsigned word = x;
  const int rr = p.r < 31 ? p.r : 31;
  for (int s = 1; s <= rr; ++s) word |= (x << s) | (x >> s);
  const int reach = (p.r + 31) / 32;
  for (int d = 1; d <= reach; ++d) {
    if (v.w + d < p.wz) {
      const unsigned y = row[v.w + d];
      if (y) {
        const int th = 32 * d + (__ffs((int)y) - 1) - p.r;
        if (th <= 31) word |= th <= 0 ? 0xffffffffu : 0xffffffffu << th;
      }
    }
    if (v.w - d >= 0) {
      const unsigned y = row[v.w - d];
      if (y) {
        const int top = p.r - 32 * d + (31 - __clz((int)y));
        if (top >= 0) word |= top >= 31 ? 0xffffffffu : (2u << top) - 1u;
      }
    }
  }
  p.out[wi] = word & v.vmask;
}

// x or y: the OR of the words of the rows within r along the axis; the last pass also counts
__global__ __launch_bounds__(kVoxThreads) void voxel_dilate_rows_kernel(const VoxDilateParams p) {
  const long long wi = (long long)blockIdx.x * kVoxThreads + threadIdx.x;
  double cnt = 0.0;
  if (wi < p.n_words) {
    const VoxWord v = vox_word(wi, p.gy, p.gz, p.wz);
    const int at = p.axis == 0 ? v.i : v.j, g = p.axis == 0 ? p.gx : p.gy;
    const long long stride = p.axis == 0 ? (long long)p.gy * p.wz : p.wz;
    const int q0 = at - p.r < 0 ? 0 : at - p.r, q1 = at + p.r > g - 1 ? g - 1 : at + p.r;
    unsigned word = 0;
    for (int q = q0; q <= q1; ++q) word |= p.in[wi + (q - at) * stride];
    word &= v.vmask;
    p.out[wi] = word;
    cnt = (double)__popc(word);
  }
  if (p.parts) {
    const double c[1] = {cnt};
    block_sum_d<kVoxThreads, 1>(c, p.parts + blockIdx.x);
  }
}

__global__ __launch_bounds__(kVoxThreads) void voxel_count_finish_kernel(const double* parts, long long n_parts, long long* count) {
  count_finish<kVoxThreads>(parts, n_parts, count);
}

inline bool vox_grid_ok(long long gx, long long gy, long long gz, long long max_side) {
  if (gx < 1 || gy < 1 || gz < 1 || gx > max_side || gy > max_side || gz > max_side) return false;
  const long long lim = 1LL << 31, a = gx * gy;                      // sides below 2^31: a below 2^62
  return a < lim && a * gz < lim;
}
inline long long vox_words(long long gx, long long gy, long long gz) { return gx * gy * ((gz + 31) / 32); }
inline long long vox_blocks(long long n_words) { return (n_words + kVoxThreads - 1) / kVoxThreads; }
constexpr long long kVoxAnySide = (1LL << 31) - 1;

// scratch of the dilation: the z and the y pass's words uint32 [n_words] each | the count's partials float64 [blocks], unpadded.
// Returns its size.
inline long long vox_dilate_scratch(void* scratch, long long n_words, unsigned* (&tmp)[2], double*& parts) {
  Carver c(scratch);
  tmp[0] = c.take<unsigned>(n_words);
  tmp[1] = c.take<unsigned>(n_words);
  parts = c.take<double>(vox_blocks(n_words), 8);
  return c.bytes();
}

}  // namespace mf

using namespace mf;

extern "C" int32_t mf_voxel_mesh(const float* verts, int64_t V, const int64_t* tris, int64_t T, int32_t gx, int32_t gy, int32_t gz,
                                 const float* lo, const float* hi, const float* inv_cell, uint32_t* bits_out, int64_t* dropped_out,
                                 void* stream) {
  if (!vox_grid_ok(gx, gy, gz, kVoxMaxSide))
    return fail(MF_E_INVALID, "mf_voxel_mesh: grid of %d x %d x %d cells (each side 1 .. %d, fewer than 2^31 cells)", gx, gy, gz, kVoxMaxSide);
  if (V < 0 || T < 0 || V >= (1LL << 31) || T >= (1LL << 31))
    return fail(MF_E_INVALID, "mf_voxel_mesh: V=%lld T=%lld (0 .. 2^31 - 1)", (long long)V, (long long)T);
  if (!lo || !hi || !inv_cell) return fail(MF_E_INVALID, "mf_voxel_mesh: null lo, hi or inv_cell");
  for (int a = 0; a < 3; ++a) {
    if (!(lo[a] < hi[a]) || !(fabsf(lo[a]) <= 3.402823466e+38f) || !(fabsf(hi[a]) <= 3.402823466e+38f))
      return fail(MF_E_INVALID, "mf_voxel_mesh: empty or inverted box on axis %d: lo=%g hi=%g", a, lo[a], hi[a]);
    if (!(inv_cell[a] > 0.f) || !(inv_cell[a] <= 3.402823466e+38f)) return fail(MF_E_INVALID, "mf_voxel_mesh: inv_cell[%d]=%g", a, inv_cell[a]);
  }
  if (!bits_out) return fail(MF_E_INVALID, "mf_voxel_mesh: null bits_out");
  const bool any = V > 0 && T > 0;
  if (any && (!verts || !tris)) return fail(MF_E_INVALID, "mf_voxel_mesh: null verts or tris");
  VoxMeshParams p{};
  p.verts = verts; p.V = (int)V;
  p.tris = reinterpret_cast<const long long*>(tris); p.T = (int)T;
  p.gx = gx; p.gy = gy; p.gz = gz; p.wz = (gz + 31) / 32;
  for (int a = 0; a < 3; ++a) { p.lo[a] = lo[a]; p.inv_cell[a] = inv_cell[a]; }
  p.bits = bits_out;
  p.n_words = vox_words(gx, gy, gz);
  p.dropped = reinterpret_cast<unsigned long long*>(dropped_out);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // without vertices every triangle has an index outside [0, V)
  hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)capped_blocks(p.n_words, kVoxThreads, kVoxClearMaxBlocks)), dim3(kVoxThreads), 0, s,
                     p.bits, p.n_words, p.dropped, (unsigned long long)(V == 0 ? T : 0));
  if (any) {
    hipLaunchKernelGGL(voxel_surface_kernel, dim3((unsigned)capped_blocks(T, kVoxTrisPerBlock, kVoxMaxBlocks)), dim3(kVoxThreads), 0, s, p);
    hipLaunchKernelGGL(voxel_surface_big_kernel, dim3((unsigned)capped_blocks(T, kVoxThreads, kVoxBigMaxBlocks)), dim3(kVoxThreads), 0, s, p);
  }
  return check_launch("mf_voxel_mesh");
}

extern "C" int64_t mf_voxel_fill_scratch_bytes(int64_t gx, int64_t gy, int64_t gz) {
  if (!vox_grid_ok(gx, gy, gz, kVoxAnySide))
    return fail(MF_E_INVALID, "mf_voxel_fill_scratch_bytes: grid of %lld x %lld x %lld cells (each side >= 1, fewer than 2^31 cells)",
                (long long)gx, (long long)gy, (long long)gz);
  return align_up((gx * gy * gz + 1) * (int64_t)sizeof(int), 16);
}

extern "C" int32_t mf_voxel_fill(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, uint32_t* bits_out, void* scratch, void* stream) {
  if (!vox_grid_ok(gx, gy, gz, kVoxAnySide))
    return fail(MF_E_INVALID, "mf_voxel_fill: grid of %d x %d x %d cells (each side >= 1, fewer than 2^31 cells)", gx, gy, gz);
  if (!bits || !bits_out || !scratch) return fail(MF_E_INVALID, "mf_voxel_fill: null bits, bits_out or scratch");
  VoxFillParams p{};
  p.in = bits; p.out = bits_out;
  p.gx = gx; p.gy = gy; p.gz = gz; p.wz = (gz + 31) / 32;
  p.n_words = vox_words(gx, gy, gz);
  p.parent = static_cast<int*>(scratch);
  const dim3 grid((unsigned)vox_blocks(p.n_words)), block(kVoxThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(voxel_fill_init_kernel, grid, block, 0, s, p);
  hipLaunchKernelGGL(voxel_fill_union_kernel, grid, block, 0, s, p);
  hipLaunchKernelGGL(voxel_fill_emit_kernel, grid, block, 0, s, p);
  return check_launch("mf_voxel_fill");
}

extern "C" int64_t mf_voxel_dilate_scratch_bytes(int64_t gx, int64_t gy, int64_t gz) {
  if (!vox_grid_ok(gx, gy, gz, kVoxAnySide))
    return fail(MF_E_INVALID, "mf_voxel_dilate_scratch_bytes: grid of %lld x %lld x %lld cells (each side >= 1, fewer than 2^31 cells)",
                (long long)gx, (long long)gy, (long long)gz);
  unsigned* tmp[2];
  double* parts;
  return vox_dilate_scratch(nullptr, vox_words(gx, gy, gz), tmp, parts);
}

extern "C" int32_t mf_voxel_dilate(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, int32_t rx, int32_t ry, int32_t rz,
                                   uint32_t* bits_out, int64_t* count_out, void* scratch, void* stream) {
  if (!vox_grid_ok(gx, gy, gz, kVoxAnySide))
    return fail(MF_E_INVALID, "mf_voxel_dilate: grid of %d x %d x %d cells (each side >= 1, fewer than 2^31 cells)", gx, gy, gz);
  if (rx < 0 || ry < 0 || rz < 0) return fail(MF_E_INVALID, "mf_voxel_dilate: radii (%d, %d, %d) must not be negative", rx, ry, rz);
  if (!bits || !bits_out || !scratch) return fail(MF_E_INVALID, "mf_voxel_dilate: null bits, bits_out or scratch");
  if (bits == bits_out) return fail(MF_E_INVALID, "mf_voxel_dilate: bits_out must not be bits");
  VoxDilateParams p{};
  p.gx = gx; p.gy = gy; p.gz = gz; p.wz = (gz + 31) / 32;
  p.n_words = vox_words(gx, gy, gz);
  unsigned* tmp[2];
  double* parts;
  vox_dilate_scratch(scratch, p.n_words, tmp, parts);
  const long long blocks = vox_blocks(p.n_words);
  const dim3 grid((unsigned)blocks), block(kVoxThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned* src = bits;
  if (rz > 0 && gz > 1) {
    p.in = src; p.out = tmp[0]; p.r = rz < gz - 1 ? rz : gz - 1;
    hipLaunchKernelGGL(voxel_dilate_z_kernel, grid, block, 0, s, p);
    src = tmp[0];
  }
  if (ry > 0 && gy > 1) {
    p.in = src; p.out = tmp[1]; p.r = ry < gy - 1 ? ry : gy - 1; p.axis = 1;
    hipLaunchKernelGGL(voxel_dilate_rows_kernel, grid, block, 0, s, p);
    src = tmp[1];
  }
  p.in = src; p.out = bits_out; p.r = rx < gx - 1 ? rx : gx - 1; p.axis = 0;       // always runs: it writes bits_out and counts
  p.parts = count_out ? parts : nullptr;
  hipLaunchKernelGGL(voxel_dilate_rows_kernel, grid, block, 0, s, p);
  if (count_out)
    hipLaunchKernelGGL(voxel_count_finish_kernel, dim3(1), block, 0, s, parts, blocks, reinterpret_cast<long long*>(count_out));
  return check_launch("mf_voxel_dilate");
}
