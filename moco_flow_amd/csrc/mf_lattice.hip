// mf_lattice.hip -- sparse lattice queries: evaluate sigma only in the bricks of a lattice that an occupancy grid marks
// (include/mocoflow_hip.h):
//   mf_lattice_select  : bricks of 8 x 8 x 8 lattice points against the bit grid -> slot per brick, the active bricks in order, K
//   mf_lattice_points  : the active bricks' world points, 512 rows per brick -- the input of mf_points_sigma
//   mf_lattice_scatter : the compact sigma rows -> the dense (n0, n1, n2) volume, `fill` where a brick is inactive
// They serve the two jobs that evaluate a whole lattice: visualize_mesh's (trainer_moco_flow.py:490-538, trainer_nerf.py:200-259)
// and OccupancyGrid.from_field's.  The reference has no counterpart: it evaluates every point.
// Integer work and copies only; the host builds the cell-range tables (moco_flow_amd/points.py), so tests/lattice_oracle.py
// reproduces every decision exactly.  No atomics: ranks come from mf_scan.hpp, every output word has one writer.
#include "mf_host.hpp"
#include "mf_scan.hpp"

namespace mf {

constexpr int kLatThreads = 256;                                         // 4 waves
constexpr int kBrickPoints = 512;                                        // 8 x 8 x 8, local index (l0 << 6) | (l1 << 3) | l2
constexpr int kLatScatterMaxBlocks = 1 << 16;                            // the scatter's grid stops growing: more rows take more trips

__device__ __forceinline__ int pick3(int a, int v0, int v1, int v2) { return a == 0 ? v0 : a == 1 ? v1 : v2; }

struct LatSelectParams {
  const unsigned* bits;
  int g[3], wz;                    // grid cells per WORLD axis, words per (x, y) row
  const int* range[3];             // per WORLD axis w: the (nb_a, 2) table of the volume axis a that carries it
  int axis_of_world[3];            // that a
  int nb[3];                       // bricks per VOLUME axis
  long long n_bricks;
  int* slot; int* brick_ids; long long* count;
  long long* blk;                  // (nblocks) active bricks of each workgroup, then their exclusive prefix
  long long nblocks;
};

// launch 1: one lane per brick ORs the words of its cell box; slot[brick] = 0 | 1, blk[workgroup] = its active bricks
__global__ __launch_bounds__(kLatThreads) void lat_flag_kernel(const LatSelectParams p) {
  const long long bi = (long long)blockIdx.x * kLatThreads + threadIdx.x;
  bool on = false;
  if (bi < p.n_bricks) {
    const int b2 = (int)(bi % p.nb[2]);
    const long long t = bi / p.nb[2];
    const int b1 = (int)(t % p.nb[1]), b0 = (int)(t / p.nb[1]);
    int c0[3], c1[3];
    bool any = true;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const int b = pick3(p.axis_of_world[w], b0, b1, b2);
      const int lo = p.range[w][2 * b], hi = p.range[w][2 * b + 1];
      c0[w] = lo < 0 ? 0 : lo;                                           // a table is the caller's: nothing outside the grid is read
      c1[w] = hi > p.g[w] - 1 ? p.g[w] - 1 : hi;
      any = any && c0[w] <= c1[w];
    }
    if (any) {
      const int w0 = c0[2] >> 5, w1 = c1[2] >> 5;
      const unsigned first = ~0u << (c0[2] & 31), last = ~0u >> (31 - (c1[2] & 31));
      unsigned acc = 0;
      for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y) {
          const unsigned* row = p.bits + ((long long)x * p.g[1] + y) * p.wz;
          for (int w = w0; w <= w1; ++w) {
            unsigned m = row[w];
            if (w == w0) m &= first;
            if (w == w1) m &= last;
            acc |= m;
          }
        }
      on = acc != 0;
    }
    p.slot[bi] = on ? 1 : 0;
  }
  const long long c = block_sum_i64<kLatThreads>(on ? 1 : 0);
  if (threadIdx.x == 0) p.blk[blockIdx.x] = c;
}

// launch 2: one workgroup, the exclusive prefix of the workgroups' counts in place, and K
__global__ __launch_bounds__(kLatThreads) void lat_scan_kernel(const LatSelectParams p) {
  long long total[1];
  scan_totals<kLatThreads, 1>(p.blk, p.nblocks, p.blk, total);
  if (threadIdx.x == 0) *p.count = total[0];
}

// launch 3: the rank of an active brick = the workgroups in front + the waves in front + the lanes in front (mf_scan.hpp)
__global__ __launch_bounds__(kLatThreads) void lat_rank_kernel(const LatSelectParams p) {
  const long long bi = (long long)blockIdx.x * kLatThreads + threadIdx.x;
  const bool on = bi < p.n_bricks && p.slot[bi] != 0;
  int c[1], front[1], tot[1];
  const int before = wave_rank(on, c[0]);
  block_offsets<kLatThreads, 1>(c, front, tot);
  if (bi < p.n_bricks) {
    const long long r = p.blk[blockIdx.x] + front[0] + before;           // < K <= n_bricks < 2^31
    p.slot[bi] = on ? (int)r : -1;
    if (on) p.brick_ids[r] = (int)bi;
  }
}

struct LatPointsParams {
  const int* brick_ids;
  const float* axis[3];
  int n[3], nb[3], woa[3];
  long long n_bricks;
  float* pts;
};

// One workgroup per active brick, two points per lane.
__global__ __launch_bounds__(kLatThreads) void lat_points_kernel(const LatPointsParams p) {
  const long long r = blockIdx.x;
  long long id = p.brick_ids[r];
  id = id < 0 ? 0 : id >= p.n_bricks ? p.n_bricks - 1 : id;               // the list is the caller's: no axis is read out of range
  const int b2 = (int)(id % p.nb[2]);
  const long long t = id / p.nb[2];
  const int b1 = (int)(t % p.nb[1]), b0 = (int)(t / p.nb[1]);
#pragma unroll
  for (int h = 0; h < kBrickPoints / kLatThreads; ++h) {
    const int l = h * kLatThreads + threadIdx.x;
    const int i0 = 8 * b0 + (l >> 6), i1 = 8 * b1 + ((l >> 3) & 7), i2 = 8 * b2 + (l & 7);
    const float v0 = p.axis[0][i0 < p.n[0] - 1 ? i0 : p.n[0] - 1];       // a partial brick repeats its last point
    const float v1 = p.axis[1][i1 < p.n[1] - 1 ? i1 : p.n[1] - 1];
    const float v2 = p.axis[2][i2 < p.n[2] - 1 ? i2 : p.n[2] - 1];
    float* row = p.pts + (r * kBrickPoints + l) * 3;
    row[p.woa[0]] = v0; row[p.woa[1]] = v1; row[p.woa[2]] = v2;
  }
}

struct LatScatterParams {
  const float* sigma;
  const int* slot;
  long long K, rows;               // rows = n0 n1
  int n[3], nb[3];
  float fill;
  float* vol;
};

// One workgroup per (i0, i1) row of the volume and trip; every point is written once, by one lane.
__global__ __launch_bounds__(kLatThreads) void lat_scatter_kernel(const LatScatterParams p) {
  for (long long row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const int i1 = (int)(row % p.n[1]), i0 = (int)(row / p.n[1]);
    const long long brow = ((long long)(i0 >> 3) * p.nb[1] + (i1 >> 3)) * p.nb[2];
    const int local = ((i0 & 7) << 6) | ((i1 & 7) << 3);
    float* out = p.vol + row * p.n[2];
    for (int i2 = threadIdx.x; i2 < p.n[2]; i2 += kLatThreads) {
      const long long s = p.slot[brow + (i2 >> 3)];
      out[i2] = s >= 0 && s < p.K ? p.sigma[s * kBrickPoints + (local | (i2 & 7))] : p.fill;   // a slot beyond K reads nothing
    }
  }
}

// each side in [1, 2^31), fewer than 2^31 bricks; fills nb
inline bool lat_shape_ok(long long n0, long long n1, long long n2, long long (&nb)[3]) {
  const long long lim = 1LL << 31, n[3] = {n0, n1, n2};
  for (int a = 0; a < 3; ++a) {
    if (n[a] < 1 || n[a] >= lim) return false;
    nb[a] = (n[a] + 7) / 8;
  }
  const long long a = nb[0] * nb[1];                                       // below 2^56
  return a < lim && a * nb[2] < lim;
}

inline int lat_shape(const char* who, long long n0, long long n1, long long n2, long long (&nb)[3]) {
  if (lat_shape_ok(n0, n1, n2, nb)) return MF_OK;
  return fail(MF_E_INVALID, "%s: lattice %lld x %lld x %lld (each side >= 1, fewer than 2^31 bricks of 8 x 8 x 8)", who, n0, n1, n2);
}

inline int lat_perm(const char* who, const int32_t* woa) {
  if (!woa) return fail(MF_E_INVALID, "%s: null world_of_axis", who);
  int seen = 0;
  for (int a = 0; a < 3; ++a)
    if (woa[a] >= 0 && woa[a] <= 2) seen |= 1 << woa[a];
  if (seen != 7)
    return fail(MF_E_INVALID, "%s: world_of_axis = (%d, %d, %d) is not a permutation of (0, 1, 2)", who, woa[0], woa[1], woa[2]);
  return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_lattice_select_scratch_bytes(int64_t n0, int64_t n1, int64_t n2) {
  long long nb[3];
  if (lat_shape("mf_lattice_select_scratch_bytes", n0, n1, n2, nb) != MF_OK) return -1;
  return (nb[0] * nb[1] * nb[2] + kLatThreads - 1) / kLatThreads * (int64_t)sizeof(long long);
}

extern "C" int32_t mf_lattice_select(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, const int32_t* range0,
                                     const int32_t* range1, const int32_t* range2, int64_t n0, int64_t n1, int64_t n2,
                                     const int32_t* world_of_axis, int32_t* slot, int32_t* brick_ids, int64_t* count, void* scratch,
                                     void* stream) {
  long long nb[3];
  if (int e = lat_shape("mf_lattice_select", n0, n1, n2, nb)) return e;
  if (gx < 1 || gy < 1 || gz < 1 || (long long)gx * gy >= (1LL << 31) || (long long)gx * gy * gz >= (1LL << 31))
    return fail(MF_E_INVALID, "mf_lattice_select: grid of %d x %d x %d cells (each side >= 1, fewer than 2^31 cells)", gx, gy, gz);
  if (int e = lat_perm("mf_lattice_select", world_of_axis)) return e;
  if (!bits || !range0 || !range1 || !range2) return fail(MF_E_INVALID, "mf_lattice_select: null bits or range table");
  if (!slot || !brick_ids || !count || !scratch) return fail(MF_E_INVALID, "mf_lattice_select: null output (slot, brick_ids or count) or scratch");
  const int32_t* range[3] = {range0, range1, range2};
  LatSelectParams p{};
  p.bits = bits;
  p.g[0] = gx; p.g[1] = gy; p.g[2] = gz; p.wz = (gz + 31) / 32;
  for (int a = 0; a < 3; ++a) {
    p.nb[a] = (int)nb[a];
    p.range[world_of_axis[a]] = range[a];
    p.axis_of_world[world_of_axis[a]] = a;
  }
  p.n_bricks = nb[0] * nb[1] * nb[2];
  p.slot = slot; p.brick_ids = brick_ids; p.count = reinterpret_cast<long long*>(count);
  p.blk = static_cast<long long*>(scratch);
  p.nblocks = (p.n_bricks + kLatThreads - 1) / kLatThreads;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(lat_flag_kernel, dim3((unsigned)p.nblocks), dim3(kLatThreads), 0, s, p);
  hipLaunchKernelGGL(lat_scan_kernel, dim3(1), dim3(kLatThreads), 0, s, p);
  hipLaunchKernelGGL(lat_rank_kernel, dim3((unsigned)p.nblocks), dim3(kLatThreads), 0, s, p);
  return check_launch("mf_lattice_select");
}

extern "C" int32_t mf_lattice_points(const int32_t* brick_ids, int64_t K, const float* axis0, const float* axis1, const float* axis2,
                                     int64_t n0, int64_t n1, int64_t n2, const int32_t* world_of_axis, float* points, void* stream) {
  long long nb[3];
  if (int e = lat_shape("mf_lattice_points", n0, n1, n2, nb)) return e;
  if (int e = lat_perm("mf_lattice_points", world_of_axis)) return e;
  if (K < 0 || K > nb[0] * nb[1] * nb[2])
    return fail(MF_E_INVALID, "mf_lattice_points: K=%lld of %lld bricks", (long long)K, nb[0] * nb[1] * nb[2]);
  if (!axis0 || !axis1 || !axis2) return fail(MF_E_INVALID, "mf_lattice_points: null axis table");
  if (K == 0) return MF_OK;
  if (!brick_ids || !points) return fail(MF_E_INVALID, "mf_lattice_points: null brick_ids or points");
  LatPointsParams p{};
  p.brick_ids = brick_ids;
  p.axis[0] = axis0; p.axis[1] = axis1; p.axis[2] = axis2;
  const long long n[3] = {n0, n1, n2};
  for (int a = 0; a < 3; ++a) { p.n[a] = (int)n[a]; p.nb[a] = (int)nb[a]; p.woa[a] = world_of_axis[a]; }
  p.n_bricks = nb[0] * nb[1] * nb[2];
  p.pts = points;
  hipLaunchKernelGGL(lat_points_kernel, dim3((unsigned)K), dim3(kLatThreads), 0, static_cast<hipStream_t>(stream), p);
  return check_launch("mf_lattice_points");
}

extern "C" int32_t mf_lattice_scatter(const float* sigma, const int32_t* slot, int64_t K, int64_t n0, int64_t n1, int64_t n2,
                                      float fill, float* volume, void* stream) {
  long long nb[3];
  if (int e = lat_shape("mf_lattice_scatter", n0, n1, n2, nb)) return e;
  if (K < 0 || K > nb[0] * nb[1] * nb[2])
    return fail(MF_E_INVALID, "mf_lattice_scatter: K=%lld of %lld bricks", (long long)K, nb[0] * nb[1] * nb[2]);
  if (!slot || !volume) return fail(MF_E_INVALID, "mf_lattice_scatter: null slot or volume");
  if (K > 0 && !sigma) return fail(MF_E_INVALID, "mf_lattice_scatter: null sigma with K=%lld", (long long)K);
  LatScatterParams p{};
  p.sigma = sigma; p.slot = slot; p.K = K; p.rows = n0 * n1;
  const long long n[3] = {n0, n1, n2};
  for (int a = 0; a < 3; ++a) { p.n[a] = (int)n[a]; p.nb[a] = (int)nb[a]; }
  p.fill = fill; p.vol = volume;
  hipLaunchKernelGGL(lat_scatter_kernel, dim3((unsigned)capped_blocks(p.rows, 1, kLatScatterMaxBlocks)), dim3(kLatThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  return check_launch("mf_lattice_scatter");
}
