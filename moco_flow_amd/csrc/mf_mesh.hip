// mf_mesh.hip -- marching cubes on the device (mf_mc_scratch_bytes / mf_mc_count / mf_mc_emit): the isosurface step of
// visualize_mesh (trainer_moco_flow.py:528-545, trainer_nerf.py:247-259: mcubes.marching_cubes on the host) with the
// volume and the mesh kept on the device.
//
// Contract (tests/mc_oracle.py restates it in numpy, bit for bit):
//   - a corner is below iff v < iso (NaN is not); clamp_zero reads v < 0 ? 0 : v;
//   - one vertex per crossing lattice edge (p, axis), shared by the cells around it, at p + t e_axis with
//     t = (iso - f(p)) / (f(p + e_axis) - f(p)) in fp32 (index coordinates, one rounding per operation: -ffp-contract=off);
//   - vertices sorted by edge id 3 p + axis, triangles by the C-order index of their cell and within a cell in table order
//     (mf_mc_tables.hpp): the output does not depend on scheduling and is bit-identical from run to run.
//
// Three launches.  A block owns kPointsPerBlock consecutive lattice points (C order), 4 per thread, loaded as float4 along
// n2 where the rows allow it.  Per point: the crossing mask of the 3 edges it owns and the case of the cell it is the first
// corner of.  (1) count: block-local exclusive scans (wave ballots + LDS) of the vertex and triangle counts; per point that
// owns a crossing edge, map[p] = (block-local vertex base << 3) | mask; per block its two totals.  (2) scan: one block turns
// the per-block totals into int64 offsets and writes [V, T].  (3) emit: recomputes the masks and cases (the volume's second
// read), writes the vertices, and resolves each triangle corner (q, axis) to off[block of q] + (map[q] >> 3) + the number of
// q's crossing edges below `axis`.  map is read only where the count pass wrote it (the table uses crossing edges only).
#include "mf_host.hpp"
#include "mf_mc_tables.hpp"
#include "mf_scan.hpp"

#include <climits>

using namespace mf;
using namespace mf::mc;

namespace mf {
namespace mc {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kPointsPerBlock = kThreads * kPerThread;
constexpr int kScanThreads = 1024;

struct McParams {
  const float* vol;
  int n0, n1, n2;
  long long S, P;               // n1 n2, n0 n1 n2 (< 2^31)
  float iso;
  int clamp_zero;
  int nblocks;
  long long* off;               // [2 nblocks]: exclusive vertex / triangle offset of each block (scan)
  int* blk;                     // [2 nblocks]: vertex / triangle total of each block (count)
  int* map;                     // [P]: (block-local vertex base << 3) | crossing mask, at points that own a crossing edge
  long long* counts;            // [V, T]
  float* verts;                 // (V, 3)
  long long* tris;              // (T, 3)
};

// f(base + c), c = 0..4 (a thread's 4 points and the next one); entries at or past P are never used and read as 0
template <bool kVec>
__device__ __forceinline__ void load_row(const McParams& p, long long base, float f[5]) {
  if (kVec && base + 4 < p.P) {
    const float4 v = *reinterpret_cast<const float4*>(p.vol + base);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    f[4] = p.vol[base + 4];
  } else {
#pragma unroll
    for (int c = 0; c < 5; ++c) f[c] = base + c < p.P ? p.vol[base + c] : 0.f;
  }
  if (p.clamp_zero) {
#pragma unroll
    for (int c = 0; c < 5; ++c) f[c] = f[c] < 0.f ? 0.f : f[c];
  }
}

// One thread's 4 points: values of the rows p, p + n2, p + S, p + S + n2 (row r = 2 o0 + o1 holds corner offsets (o0, o1)),
// per point its lattice index, crossing mask (bit a: edge along axis a) and cell case (0 when p is not a cell's first corner).
struct Points {
  float f[4][5];
  int i[kPerThread], j[kPerThread], k[kPerThread];
  int mask[kPerThread], cases[kPerThread];
  int nv, nt;
};

template <bool kVec>
__device__ __forceinline__ void classify(const McParams& p, long long p0, Points& s) {
  load_row<kVec>(p, p0, s.f[0]);
  load_row<kVec>(p, p0 + p.n2, s.f[1]);
  load_row<kVec>(p, p0 + p.S, s.f[2]);
  load_row<kVec>(p, p0 + p.S + p.n2, s.f[3]);
  unsigned b[4];                                                // bit c of b[r]: f[r][c] below
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    b[r] = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) b[r] |= (s.f[r][c] < p.iso ? 1u : 0u) << c;
  }
  const unsigned pp = p0 < p.P ? (unsigned)p0 : 0u;
  int k = (int)(pp % (unsigned)p.n2), j = (int)((pp / (unsigned)p.n2) % (unsigned)p.n1), i = (int)(pp / (unsigned)p.S);
  s.nv = s.nt = 0;
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    s.i[q] = i; s.j[q] = j; s.k[q] = k;
    int mask = 0, cs = 0;
    if (p0 + q < p.P) {
      const unsigned b0 = (b[0] >> q) & 1u;
      if (i < p.n0 - 1 && b0 != ((b[2] >> q) & 1u)) mask |= 1;
      if (j < p.n1 - 1 && b0 != ((b[1] >> q) & 1u)) mask |= 2;
      if (k < p.n2 - 1 && b0 != ((b[0] >> (q + 1)) & 1u)) mask |= 4;
      if (i < p.n0 - 1 && j < p.n1 - 1 && k < p.n2 - 1) {
#pragma unroll
        for (int c = 0; c < 8; ++c) cs |= (int)((b[c >> 1] >> (q + (c & 1))) & 1u) << c;   // corner c = 4 o0 + 2 o1 + o2
      }
    }
    s.mask[q] = mask;
    s.cases[q] = cs;
    s.nv += __popc(mask);
    s.nt += kNumTri[cs];
    if (++k == p.n2) { k = 0; if (++j == p.n1) { j = 0; ++i; } }
  }
}

// exclusive prefix and total over the block of (a, b), a < 16, b < 32 per thread: bit-sliced wave ballots, then the wave totals
// via LDS.  The exchange is written out here: through block_offsets (mf_scan.hpp) mc_emit_kernel is allocated 58 VGPRs for 68
// and another schedule, which is faster on a sparse mesh and slower on a dense one.
__device__ __forceinline__ void block_scan(int a, int b, int (&ex)[2], int (&tot)[2]) {
  __shared__ int wave_tot[2][kThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = lanes_below(lane);
  int ea = 0, eb = 0, ta = 0, tb = 0;
#pragma unroll
  for (int bit = 0; bit < 4; ++bit) {
    const unsigned long long m = __ballot((a >> bit) & 1);
    ea += __popcll(m & below) << bit; ta += __popcll(m) << bit;
  }
#pragma unroll
  for (int bit = 0; bit < 5; ++bit) {
    const unsigned long long m = __ballot((b >> bit) & 1);
    eb += __popcll(m & below) << bit; tb += __popcll(m) << bit;
  }
  if (lane == 0) { wave_tot[0][w] = ta; wave_tot[1][w] = tb; }
  __syncthreads();
  tot[0] = tot[1] = 0;
#pragma unroll
  for (int v = 0; v < kThreads / 64; ++v) {
    if (v < w) { ea += wave_tot[0][v]; eb += wave_tot[1][v]; }
    tot[0] += wave_tot[0][v]; tot[1] += wave_tot[1][v];
  }
  ex[0] = ea; ex[1] = eb;
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void mc_count_kernel(const McParams p) {
  const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kPerThread;
  Points s;
  classify<kVec>(p, p0, s);
  int ex[2], tot[2];                                            // vertices, triangles
  block_scan(s.nv, s.nt, ex, tot);
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    if (s.mask[q]) {
      p.map[p0 + q] = (ex[0] << 3) | s.mask[q];
      ex[0] += __popc(s.mask[q]);
    }
  }
  if (threadIdx.x == 0) { p.blk[blockIdx.x] = tot[0]; p.blk[p.nblocks + blockIdx.x] = tot[1]; }
}

// one block: exclusive int64 prefix of the per-block totals (vertices, triangles), and the two grand totals
__global__ __launch_bounds__(kScanThreads) void mc_scan_kernel(const McParams p) {
  long long total[2];
  scan_totals<kScanThreads, 2>(p.blk, p.nblocks, p.off, total);
  if (threadIdx.x == 0) { p.counts[0] = total[0]; p.counts[1] = total[1]; }
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void mc_emit_kernel(const McParams p) {
  const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kPerThread;
  Points s;
  classify<kVec>(p, p0, s);
  int ex[2], tot[2];
  block_scan(s.nv, s.nt, ex, tot);
  long long vid = p.off[blockIdx.x] + ex[0];
  long long tid = p.off[p.nblocks + blockIdx.x] + ex[1];
#pragma unroll
  for (int q = 0; q < kPerThread; ++q) {
    const float f0 = s.f[0][q];
    const float f1[3] = {s.f[2][q], s.f[1][q], s.f[0][q + 1]};   // the far end of the edge along axis 0, 1, 2
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (s.mask[q] >> a & 1) {
        const float t = (p.iso - f0) / (f1[a] - f0);
        float x = (float)s.i[q], y = (float)s.j[q], z = (float)s.k[q];
        if (a == 0) x = x + t; else if (a == 1) y = y + t; else z = z + t;
        float* o = p.verts + vid * 3;
        o[0] = x; o[1] = y; o[2] = z;
        ++vid;
      }
    }
    const int cs = s.cases[q], nt = kNumTri[cs];
    for (int r = 0; r < nt; ++r) {
      long long* o = p.tris + tid * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int e = kTriEdges[cs][3 * r + c];
        const int a = e >> 2, u = (e >> 1) & 1, v = e & 1;
        const long long qp = p0 + q + (a == 0 ? u * (long long)p.n2 + v
                                     : a == 1 ? u * p.S + v
                                              : u * p.S + v * (long long)p.n2);
        const int m = p.map[qp];
        o[c] = p.off[qp / kPointsPerBlock] + (m >> 3) + __popc(m & ((1 << a) - 1));
      }
      ++tid;
    }
  }
}

// shape check shared by the three entry points; fills the geometry of p
int mc_shape(const char* what, int64_t n0, int64_t n1, int64_t n2, McParams& p) {
  if (n0 < 2 || n1 < 2 || n2 < 2)
    return fail(MF_E_INVALID, "%s: volume %lld x %lld x %lld (each side >= 2)", what, (long long)n0, (long long)n1, (long long)n2);
  if (n0 > INT_MAX || n1 > INT_MAX || n2 > INT_MAX || n1 * n2 > INT_MAX || n0 * (n1 * n2) > INT_MAX)
    return fail(MF_E_INVALID, "%s: volume %lld x %lld x %lld exceeds 2^31 - 1 points", what, (long long)n0, (long long)n1, (long long)n2);
  p.n0 = (int)n0; p.n1 = (int)n1; p.n2 = (int)n2;
  p.S = n1 * n2;
  p.P = n0 * p.S;
  p.nblocks = (int)((p.P + kPointsPerBlock - 1) / kPointsPerBlock);
  return MF_OK;
}

// scratch: off int64 [2 nb] | blk int32 [2 nb] | map int32 [P], unpadded.  Binds the three and returns the size
int64_t mc_bind(McParams& p, void* scratch) {
  Carver c(scratch);
  p.off = c.take<long long>(2LL * p.nblocks);
  p.blk = c.take<int>(2LL * p.nblocks, 8);
  p.map = c.take<int>(p.P, 4);
  return c.bytes();
}

// ---- vertex normals from the volume (mf_mc_normals): one thread per vertex, a gather of at most 12 values
struct NormalsParams {
  const float* vol;
  int n0, n1, n2;
  long long S;                  // n1 n2
  int clamp_zero;
  const float* verts;           // (V, 3) index coordinates
  long long V;
  float* normals;               // (V, 3)
};

__device__ __forceinline__ float vol_at(const NormalsParams& p, int i, int j, int k) {
  const float v = p.vol[i * p.S + (long long)j * p.n2 + k];
  return (p.clamp_zero && v < 0.f) ? 0.f : v;
}

// gradient at the lattice point (i, j, k): central differences, one-sided on a border face (every side >= 2)
__device__ __forceinline__ void lattice_gradient(const NormalsParams& p, int i, int j, int k, float g[3]) {
  const int i0 = i > 0 ? i - 1 : i, i1 = i < p.n0 - 1 ? i + 1 : i;
  const int j0 = j > 0 ? j - 1 : j, j1 = j < p.n1 - 1 ? j + 1 : j;
  const int k0 = k > 0 ? k - 1 : k, k1 = k < p.n2 - 1 ? k + 1 : k;
  const float d0 = vol_at(p, i1, j, k) - vol_at(p, i0, j, k);
  const float d1 = vol_at(p, i, j1, k) - vol_at(p, i, j0, k);
  const float d2 = vol_at(p, i, j, k1) - vol_at(p, i, j, k0);
  g[0] = i1 - i0 == 2 ? d0 * 0.5f : d0;
  g[1] = j1 - j0 == 2 ? d1 * 0.5f : d1;
  g[2] = k1 - k0 == 2 ? d2 * 0.5f : d2;
}

// lattice cell index of a coordinate: min(floor(x), n - 1), and 0 for anything below 0 or not a number (never out of bounds)
__device__ __forceinline__ int cell_of(float x, int n) {
  if (!(x >= 0.f)) return 0;
  const float f = floorf(x);
  return f >= (float)(n - 1) ? n - 1 : (int)f;
}

__global__ __launch_bounds__(kThreads) void mc_normals_kernel(const NormalsParams p) {
  const long long v = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (v >= p.V) return;
  const float x0 = p.verts[v * 3 + 0], x1 = p.verts[v * 3 + 1], x2 = p.verts[v * 3 + 2];
  const int i = cell_of(x0, p.n0), j = cell_of(x1, p.n1), k = cell_of(x2, p.n2);
  const float t0 = x0 - (float)i, t1 = x1 - (float)j, t2 = x2 - (float)k;
  int a = 0;                                                    // the axis of the vertex's edge: largest t, ties to the lowest
  float t = t0;
  if (t1 > t) { a = 1; t = t1; }
  if (t2 > t) { a = 2; t = t2; }
  float g[3];
  lattice_gradient(p, i, j, k, g);
  if (t > 0.f) {                                                // (t == 0: a lattice point; NaN: the gradient at the cell index)
    const int i2 = a == 0 && i < p.n0 - 1 ? i + 1 : i, j2 = a == 1 && j < p.n1 - 1 ? j + 1 : j, k2 = a == 2 && k < p.n2 - 1 ? k + 1 : k;
    float h[3];
    lattice_gradient(p, i2, j2, k2, h);
    const float s = 1.f - t;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = s * g[c] + t * h[c];
  }
  const float len2 = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
  float n[3] = {0.f, 0.f, 0.f};
  if (len2 > 0.f && len2 < __builtin_inff()) {                  // ||g|| == 0 or g not finite: the zero vector
    const float inv = 1.f / sqrtf(len2);
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = -(g[c] * inv);
  }
  float* o = p.normals + v * 3;
  o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

bool vec_rows(const McParams& p) { return p.n2 % 4 == 0 && is_aligned(p.vol, 16); }

}  // namespace mc
}  // namespace mf

extern "C" int64_t mf_mc_scratch_bytes(int64_t n0, int64_t n1, int64_t n2) {
  McParams p{};
  const int rc = mc_shape("mf_mc_scratch_bytes", n0, n1, n2, p);
  return rc != MF_OK ? rc : mc_bind(p, nullptr);
}

extern "C" int32_t mf_mc_count(const float* vol, int64_t n0, int64_t n1, int64_t n2, float iso, int32_t clamp_zero,
                               void* scratch, int64_t* counts, void* stream) {
  McParams p{};
  const int rc = mc_shape("mf_mc_count", n0, n1, n2, p);
  if (rc != MF_OK) return rc;
  if (!vol || !scratch || !counts) return fail(MF_E_INVALID, "mf_mc_count: null argument");
  p.vol = vol; p.iso = iso; p.clamp_zero = clamp_zero ? 1 : 0;
  p.counts = reinterpret_cast<long long*>(counts);
  mc_bind(p, scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec_rows(p)) hipLaunchKernelGGL(mc_count_kernel<true>, dim3(p.nblocks), dim3(kThreads), 0, s, p);
  else hipLaunchKernelGGL(mc_count_kernel<false>, dim3(p.nblocks), dim3(kThreads), 0, s, p);
  hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, p);
  return check_launch("mf_mc_count");
}

extern "C" int32_t mf_mc_emit(const float* vol, int64_t n0, int64_t n1, int64_t n2, float iso, int32_t clamp_zero,
                              const void* scratch, float* verts, int64_t* tris, void* stream) {
  McParams p{};
  const int rc = mc_shape("mf_mc_emit", n0, n1, n2, p);
  if (rc != MF_OK) return rc;
  if (!vol || !scratch) return fail(MF_E_INVALID, "mf_mc_emit: null argument");
  p.vol = vol; p.iso = iso; p.clamp_zero = clamp_zero ? 1 : 0;
  p.verts = verts;
  p.tris = reinterpret_cast<long long*>(tris);
  mc_bind(p, const_cast<void*>(scratch));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec_rows(p)) hipLaunchKernelGGL(mc_emit_kernel<true>, dim3(p.nblocks), dim3(kThreads), 0, s, p);
  else hipLaunchKernelGGL(mc_emit_kernel<false>, dim3(p.nblocks), dim3(kThreads), 0, s, p);
  return check_launch("mf_mc_emit");
}

extern "C" int32_t mf_mc_normals(const float* vol, int64_t n0, int64_t n1, int64_t n2, int32_t clamp_zero, const float* verts,
                                 int64_t V, float* normals, void* stream) {
  McParams shape{};
  const int rc = mc_shape("mf_mc_normals", n0, n1, n2, shape);
  if (rc != MF_OK) return rc;
  if (V < 0 || V > (int64_t)INT_MAX * kThreads) return fail(MF_E_INVALID, "mf_mc_normals: V=%lld", (long long)V);
  if (V == 0) return MF_OK;
  if (!vol || !verts || !normals) return fail(MF_E_INVALID, "mf_mc_normals: null argument");
  NormalsParams p{vol, shape.n0, shape.n1, shape.n2, shape.S, clamp_zero ? 1 : 0, verts, V, normals};
  hipLaunchKernelGGL(mc_normals_kernel, dim3((unsigned)((V + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  return check_launch("mf_mc_normals");
}
