// mf_distance.hip -- the exact weighted squared distance field of an occupancy bit grid, and the Euclidean dilation it decides
// (include/mocoflow_hip.h, mf_grid_edt), in the layout mf_occ_build writes.  mf_voxel_dilate thickens a grid by a BOX of cells, a
// superset of the Euclidean shell that is sqrt(3) times too thick along a diagonal; this unit thickens it by the ellipsoid itself.
//   d2(i, j, k) = min(R + 1, min over set cells (a, b, c) of w_x (i - a)^2 + w_y (j - b)^2 + w_z (k - c)^2)         int32
// with integer weights w_a in [1, 65536] (65536 (cell_a / cmax)^2, floored on the host) and an integer radius 0 <= R < 2^30.
// Separable, and exact because a pass only drops terms that exceed R on their own (r_a = isqrt(R / w_a) is the reach along a):
//   edt_z_kernel  g = the distance in cells to the nearest set bit of the cell's row, capped at r_z + 1          uint16 per cell
//   edt_y_kernel  m = min over |dy| <= r_y of w_y dy^2 + w_z g^2, capped at R + 1                                 int32 per cell
//   edt_x_kernel  d2 = min over |dx| <= r_x of w_x dx^2 + m, capped at R + 1; stores d2 and / or the wave's ballot of d2 <= R
// BOUND: a term w_a d^2 with |d| <= r_a is <= R and a partial minimum is <= R + 1, so every sum is <= 2 R + 1 < 2^31.
// A wave owns 64 consecutive cells of one row, lanes along z: every load of a window is one coalesced line, and the ballot of a
// wave is two whole words of the row (lanes beyond the row vote 0: the padding bits).  None of the kernels has a grid-stride loop:
// one wave per 64 cells.  Integers only, no atomics, every output has one writer; the count goes through mf_reduce.hpp.
#include <cmath>

#include "mf_host.hpp"
#include "mf_reduce.hpp"

namespace mf {

constexpr int kEdtThreads = 256;
constexpr int kEdtWaves = kEdtThreads / 64;                          // waves, and so 64-cell pieces of a row, per workgroup
constexpr int kEdtMaxSide = 1024;                                    // cells per side
constexpr int kEdtMaxWeight = 65536;                                 // the weight of the longest cell edge
constexpr int kEdtRadiusLimit = 1 << 30;                             // R stays below it

struct EdtParams {
  const unsigned* bits;
  unsigned short* g;               // z pass
  int* m;                          // y pass
  int* d2;                         // or null
  unsigned* bits_out;              // or null
  double* parts;                   // per-workgroup popcounts, or null
  int gx, gy, gz, words, pieces;   // words and 64-cell pieces per row
  long long n_tasks;               // gx gy pieces
  int w[3], r[3], R;
};

struct EdtCell {
  long long row, cell;             // row = i gy + j; cell = row gz + k
  int i, j, k;
  bool live;                       // the lane has a cell
};

__device__ __forceinline__ EdtCell edt_cell(const EdtParams& p) {
  const long long task = (long long)blockIdx.x * kEdtWaves + (threadIdx.x >> 6);
  EdtCell c;
  const bool has = task < p.n_tasks;
  const long long t = has ? task : 0;
  c.row = t / p.pieces;
  c.k = (int)(t - c.row * p.pieces) * 64 + (int)(threadIdx.x & 63);
  c.live = has && c.k < p.gz;
  c.j = (int)(c.row % p.gy);
  c.i = (int)(c.row / p.gy);
  c.cell = c.row * p.gz + c.k;
  return c;
}

// Upwards the LOWEST set bit at or above the cell is the nearest, downwards the HIGHEST at or below it; a further word is looked
// at only while its nearest bit could still lie within r_z.
__global__ __launch_bounds__(kEdtThreads) void edt_z_kernel(const EdtParams p) {
  const EdtCell c = edt_cell(p);
  if (!c.live) return;
  const unsigned* row = p.bits + c.row * p.words;
  const int w = c.k >> 5, b = c.k & 31, rz = p.r[2];
  int best = rz + 1;
  const unsigned x = row[w];
  const unsigned up = x >> b;                                        // bit b lands on bit 0
  if (up) {
    best = min(best, __ffs((int)up) - 1);
  } else {
    for (int d = 1; w + d < p.words && 32 * d - b <= rz; ++d) {
      const unsigned y = row[w + d];
      if (y) { best = min(best, 32 * d - b + __ffs((int)y) - 1); break; }
    }
  }
  const unsigned down = x << (31 - b);                               // bit b lands on bit 31
  if (down) {
    best = min(best, __clz((int)down));
  } else {
    for (int d = 1; w - d >= 0 && 32 * d + b - 31 <= rz; ++d) {
      const unsigned y = row[w - d];
      if (y) { best = min(best, 32 * d + b - 31 + __clz((int)y)); break; }
    }
  }
  p.g[c.cell] = (unsigned short)best;                                // <= r_z + 1 <= 32768
}

__global__ __launch_bounds__(kEdtThreads) void edt_y_kernel(const EdtParams p) {
  const EdtCell c = edt_cell(p);
  if (!c.live) return;
  const int cap = p.R + 1, rz = p.r[2], wy = p.w[1];
  const unsigned wz = (unsigned)p.w[2];
  const int q0 = max(c.j - p.r[1], 0), q1 = min(c.j + p.r[1], p.gy - 1);     // r_y may exceed the side
  const unsigned short* col = p.g + (long long)c.i * p.gy * p.gz + c.k;
  int m = cap;
  for (int q = q0; q <= q1; ++q) {
    const unsigned g = col[(long long)q * p.gz];
    const int dy = q - c.j;
    const int tz = g > (unsigned)rz ? cap : (int)(wz * g * g);       // unsigned: the product of a g beyond r_z is never used
    m = min(m, wy * dy * dy + tz);
  }
  p.m[c.cell] = m;
}

// No lane leaves early: the ballot and the count need the whole workgroup.
__global__ __launch_bounds__(kEdtThreads) void edt_x_kernel(const EdtParams p) {
  const EdtCell c = edt_cell(p);
  bool set = false;
  if (c.live) {
    const int cap = p.R + 1, wx = p.w[0];
    const int q0 = max(c.i - p.r[0], 0), q1 = min(c.i + p.r[0], p.gx - 1);
    const long long stride = (long long)p.gy * p.gz;
    const int* col = p.m + c.cell - c.i * stride;
    int d = cap;
    for (int q = q0; q <= q1; ++q) {
      const int dx = q - c.i;
      d = min(d, wx * dx * dx + col[q * stride]);
    }
    if (p.d2) p.d2[c.cell] = d;
    set = d <= p.R;
  }
  if (!p.bits_out) return;                                           // uniform over the launch
  const unsigned long long mask = __ballot(set);
  const int lane = threadIdx.x & 63;
  if (c.live && (lane & 31) == 0) p.bits_out[c.row * p.words + (c.k >> 5)] = (unsigned)(mask >> lane);
  if (p.parts) {
    const double cnt[1] = {lane == 0 ? (double)__popcll(mask) : 0.0};
    block_sum_d<kEdtThreads, 1>(cnt, p.parts + blockIdx.x);
  }
}

__global__ __launch_bounds__(kEdtThreads) void edt_count_finish_kernel(const double* parts, long long n_parts, long long* count) {
  count_finish<kEdtThreads>(parts, n_parts, count);
}

inline bool edt_grid_ok(long long gx, long long gy, long long gz) {
  return gx >= 1 && gy >= 1 && gz >= 1 && gx <= kEdtMaxSide && gy <= kEdtMaxSide && gz <= kEdtMaxSide;
}
inline long long edt_tasks(long long gx, long long gy, long long gz) { return gx * gy * ((gz + 63) / 64); }
inline long long edt_blocks(long long n_tasks) { return (n_tasks + kEdtWaves - 1) / kEdtWaves; }

// scratch: g uint16 [cells] | m int32 [cells] | the count's partials float64 [workgroups].  Returns its size.
inline long long edt_scratch(void* scratch, long long cells, long long blocks, unsigned short*& g, int*& m, double*& parts) {
  Carver c(scratch);
  g = c.take<unsigned short>(cells);
  m = c.take<int>(cells);
  parts = c.take<double>(blocks);
  return c.bytes();
}

inline int edt_isqrt(int v) {                                        // floor(sqrt(v)), v >= 0
  long long s = (long long)std::sqrt((double)v);
  while (s * s > v) --s;
  while ((s + 1) * (s + 1) <= v) ++s;
  return (int)s;
}

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_grid_edt_scratch_bytes(int64_t gx, int64_t gy, int64_t gz) {
  if (!edt_grid_ok(gx, gy, gz))
    return fail(MF_E_INVALID, "mf_grid_edt_scratch_bytes: grid of %lld x %lld x %lld cells (each side 1 .. %d)", (long long)gx, (long long)gy,
                (long long)gz, kEdtMaxSide);
  unsigned short* g;
  int* m;
  double* parts;
  return edt_scratch(nullptr, gx * gy * gz, edt_blocks(edt_tasks(gx, gy, gz)), g, m, parts);
}

extern "C" int32_t mf_grid_edt(const uint32_t* bits, int32_t gx, int32_t gy, int32_t gz, const int32_t* w, int32_t R, int32_t* d2_out,
                               uint32_t* bits_out, int64_t* count_out, void* scratch, void* stream) {
  if (!edt_grid_ok(gx, gy, gz)) return fail(MF_E_INVALID, "mf_grid_edt: grid of %d x %d x %d cells (each side 1 .. %d)", gx, gy, gz, kEdtMaxSide);
  if (!w) return fail(MF_E_INVALID, "mf_grid_edt: null w");
  for (int a = 0; a < 3; ++a)
    if (w[a] < 1 || w[a] > kEdtMaxWeight) return fail(MF_E_INVALID, "mf_grid_edt: w[%d]=%d (1 .. %d)", a, w[a], kEdtMaxWeight);
  if (R < 0 || R >= kEdtRadiusLimit) return fail(MF_E_INVALID, "mf_grid_edt: R=%d (0 .. 2^30 - 1)", R);
  if (!bits || !scratch) return fail(MF_E_INVALID, "mf_grid_edt: null bits or scratch");
  if (!d2_out && !bits_out) return fail(MF_E_INVALID, "mf_grid_edt: null d2_out and bits_out: nothing to write");
  if (bits_out == bits) return fail(MF_E_INVALID, "mf_grid_edt: bits_out must not be bits");
  if (count_out && !bits_out) return fail(MF_E_INVALID, "mf_grid_edt: count_out needs bits_out");
  EdtParams p{};
  p.bits = bits; p.d2 = d2_out; p.bits_out = bits_out;
  p.gx = gx; p.gy = gy; p.gz = gz; p.words = (gz + 31) / 32; p.pieces = (gz + 63) / 64;
  p.n_tasks = edt_tasks(gx, gy, gz);
  p.R = R;
  for (int a = 0; a < 3; ++a) { p.w[a] = w[a]; p.r[a] = edt_isqrt(R / w[a]); }
  const long long blocks = edt_blocks(p.n_tasks);                    // at most 2^22
  double* parts;
  edt_scratch(scratch, (long long)gx * gy * gz, blocks, p.g, p.m, parts);
  p.parts = count_out ? parts : nullptr;
  const dim3 grid((unsigned)blocks), block(kEdtThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(edt_z_kernel, grid, block, 0, s, p);
  hipLaunchKernelGGL(edt_y_kernel, grid, block, 0, s, p);
  hipLaunchKernelGGL(edt_x_kernel, grid, block, 0, s, p);
  if (count_out)
    hipLaunchKernelGGL(edt_count_finish_kernel, dim3(1), block, 0, s, parts, blocks, reinterpret_cast<long long*>(count_out));
  return check_launch("mf_grid_edt");
}
