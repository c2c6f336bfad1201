// mf_mesh_distance.hip -- how far a point is from a triangle mesh, and what two surfaces are apart (include/mocoflow_hip.h:
// mf_surface_records, mf_surface_closest, mf_surface_weights, mf_surface_sample, mf_surface_stats).  THE CONTRACT IS FIXED
// ARITHMETIC: every fp32 operation below is rounded once, in the order written, with no FMA, so that tests/mesh_distance_oracle.py
// restates every output in np.float32 bit for bit; dot(x, y) = (x0 y0 + x1 y1) + x2 y2 everywhere.
//   md_fill / md_claim / md_build / md_unplaced   mf_surface_records: a slot per triangle in the caller's `order`, a 16-float record
//                                                 + a 12-float edge row (b, bc, the triangle's box) per slot, a box per 64-slot tile
//   md_closest_kernel                             mf_surface_closest: a query per lane, on the tile walk of include/mocoflow_hip.h
//   md_weights / md_sample                        integer area weights; a triangle by binary search of their running sum, a point
//   md_stats / md_stats_finish                    float64 sums through mf_reduce.hpp, a maximum, integer counts
// The distance to a triangle is the least of FOUR clamped candidates (edges ab, ac, bc, the face), branch-free: a wave never
// diverges over Voronoi regions, and a sliver degrades to its edges.  Its value is then raised to the query's squared distance
// to the triangle's box, lb: subtraction, max, squaring and sums of non-negatives are monotone under rounding, so for any box
// that CONTAINS the triangle's the computed lb is <= the triangle's own, which is <= the value -- exactly, in fp32.  A tile is
// therefore skipped on the strict test lb_tile > best with no slack, and the culled search equals the full sweep bit for bit,
// whatever the tile order, the visiting order or the launch shape: the result is the lexicographic minimum of (value, caller's
// triangle index).  None of the closest-point kernels has a grid-stride loop (a wave per 64 queries); md_stats has one
// (kMdStatBlocks).  No float atomics: the only atomics are integer (the slot claim's minimum, the dropped count).
// (the Makefile builds every unit with -ffp-contract=off; the pragma keeps it true for a build that forgets it)
#pragma clang fp contract(off)
#include <cmath>

#include "mf_reduce.hpp"
#include "mf_surface.hpp"

namespace mf {

constexpr int kMdThreads = 256;                  // (tests/ reads these two from this file: the literals stay here)
constexpr int kMdTile = 64;
static_assert(kMdThreads == kSurfThreads && kMdTile == kSurfTile, "one tile geometry: mf_surface.hpp");
constexpr int kMdRecord = 16;                    // floats per record
constexpr int kMdEdge = 12;                      // floats per edge row
constexpr int kMdStatBlocks = 1024;              // md_stats: workgroups of its grid-stride loop
constexpr int kMdMaxThresholds = 8;
constexpr int kMdStatSlots = 5 + kMdMaxThresholds;   // sum d, sum d^2, sum |n.n|, finite rows, rows left out, within[8]
constexpr int kMdWeightOne = 1 << 20;            // the weight of the largest triangle
constexpr int kMdNoSlot = 0x7fffffff;

__device__ __forceinline__ F3 along(F3 a, F3 d, float t) { return add3(a, mul3(d, t)); }                 // a + d t
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }                  // a NaN gives 0

struct Rec { F3 a, ab, ac; float r_ab, r_ac, r_bc, d00, d01, d11, rden; };
struct Edge { F3 b, bc, lo, hi; };

// the squared distance from q to the box [lo, hi]
__device__ __forceinline__ float box_lb(F3 q, F3 lo, F3 hi) {
  const F3 g = {fmaxf(fmaxf(lo.x - q.x, q.x - hi.x), 0.f), fmaxf(fmaxf(lo.y - q.y, q.y - hi.y), 0.f), fmaxf(fmaxf(lo.z - q.z, q.z - hi.z), 0.f)};
  return dot3(g, g);
}

// The value of a triangle at q.  The candidates in the fixed order ab, ac, bc, face; strict <, so the first minimum wins and a
// NaN never does.  `region` and `P` are dead code in the search loop (the winner's are recomputed once, behind it).
__device__ __forceinline__ float tri_value(const Rec& r, const Edge& e, F3 q, int& region, F3& P) {
  const F3 qa = sub3(q, r.a);
  const float d20 = dot3(qa, r.ab), d21 = dot3(qa, r.ac);
  const F3 p0 = along(r.a, r.ab, clamp01(d20 * r.r_ab));
  const F3 p1 = along(r.a, r.ac, clamp01(d21 * r.r_ac));
  const F3 p2 = along(e.b, e.bc, clamp01(dot3(sub3(q, e.b), e.bc) * r.r_bc));
  const float v = clamp01((r.d11 * d20 - r.d01 * d21) * r.rden);
  const float w = fminf(fmaxf((r.d00 * d21 - r.d01 * d20) * r.rden, 0.f), 1.f - v);
  const F3 p3 = add3(along(r.a, r.ab, v), mul3(r.ac, w));
  const F3 e0 = sub3(q, p0), e1 = sub3(q, p1), e2 = sub3(q, p2), e3 = sub3(q, p3);
  const float c0 = dot3(e0, e0), c1 = dot3(e1, e1), c2 = dot3(e2, e2), c3 = dot3(e3, e3);
  float m = INFINITY;
  region = 0; P = p0;
  if (c0 < m) { m = c0; }
  if (c1 < m) { m = c1; region = 1; P = p1; }
  if (c2 < m) { m = c2; region = 2; P = p2; }
  if (c3 < m) { m = c3; region = 3; P = p3; }
  const float lb = box_lb(q, e.lo, e.hi);
  return lb > m ? lb : m;
}

// (value, caller's index) below (best, best's index): a slot that holds no triangle has index -1 and never wins
__device__ __forceinline__ bool md_better(float d, int tri, float best, int btri) {
  return tri >= 0 && (d < best || (d == best && (unsigned)tri < (unsigned)btri));
}

// ---------------------------------------------------------------- records ----------------------------------------------------
struct RecordParams {
  const float* verts;
  const long long* tris;
  const int* order;                // or null: identity
  float* records; float* edges; int* slot_tri; float* tile_box;
  int* tri_slot; float* area2; float* normal; unsigned char* dropped;
  long long* dropped_count;
  long long V, T, Tpad;
};

__device__ __forceinline__ int md_order(const RecordParams& p, long long s) {       // the triangle slot s asks for, or -1
  if (s >= p.T) return -1;
  const long long o = p.order ? (long long)p.order[s] : s;
  return in_range(o, p.T) ? (int)o : -1;
}

__global__ __launch_bounds__(kMdThreads) void md_fill_kernel(const RecordParams p) {
  const long long t = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (t == 0) *p.dropped_count = 0;
  if (t < p.T) p.tri_slot[t] = kMdNoSlot;
}

// a triangle goes to the LOWEST slot that asks for it (an integer minimum: any order of arrival gives the same slot)
__global__ __launch_bounds__(kMdThreads) void md_claim_kernel(const RecordParams p) {
  const long long s = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  const int o = md_order(p, s);
  if (o >= 0) atomicMin(p.tri_slot + o, (int)s);
}

// A wave is a tile.  No lane leaves early: the tile's box and the count need the whole wave.
__global__ __launch_bounds__(kMdThreads) void md_build_kernel(const RecordParams p) {
  const long long s = (long long)blockIdx.x * kMdThreads + threadIdx.x;          // < Tpad: the grid is Tpad / kMdThreads, rounded up
  const bool slot = s < p.Tpad;
  int o = md_order(p, s);
  if (o >= 0 && p.tri_slot[o] != (int)s) o = -1;                                 // a repeated entry: a later slot
  Rec r{};
  Edge e{};
  e.lo = {INFINITY, INFINITY, INFINITY};
  e.hi = {-INFINITY, -INFINITY, -INFINITY};
  bool ok = false;
  if (o >= 0) {
    float area2 = 0.f;
    F3 nrm = {0.f, 0.f, 0.f}, a, b, c;
    if (load_corners(p.verts, p.tris, p.V, o, a, b, c)) {                        // else: a dropped triangle
      Rec k;
      k.a = a; k.ab = sub3(b, a); k.ac = sub3(c, a);
      const F3 bc = sub3(c, b);
      k.d00 = dot3(k.ab, k.ab); k.d01 = dot3(k.ab, k.ac); k.d11 = dot3(k.ac, k.ac);
      k.r_ab = 1.f / k.d00; k.r_ac = 1.f / k.d11; k.r_bc = 1.f / dot3(bc, bc);
      k.rden = 1.f / (k.d00 * k.d11 - k.d01 * k.d01);
      const F3 n = {k.ab.y * k.ac.z - k.ab.z * k.ac.y, k.ab.z * k.ac.x - k.ab.x * k.ac.z, k.ab.x * k.ac.y - k.ab.y * k.ac.x};
      const float nn = dot3(n, n);
      ok = nn > 0.f && isfinite(nn) && finite3(k.a) && finite3(k.ab) && finite3(k.ac) && isfinite(k.r_ab) && isfinite(k.r_ac) &&
           isfinite(k.r_bc) && isfinite(k.d00) && isfinite(k.d01) && isfinite(k.d11) && isfinite(k.rden);
      if (ok) {
        r = k;
        e.b = b; e.bc = bc;
        e.lo = {fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z)};
        e.hi = {fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z)};
        area2 = sqrtf(nn);
        nrm = mul3(n, 1.f / area2);
      }
    }
    p.area2[o] = area2;
    p.normal[3ll * o] = nrm.x; p.normal[3ll * o + 1] = nrm.y; p.normal[3ll * o + 2] = nrm.z;
    p.dropped[o] = ok ? 0 : 1;
  }
  if (slot) {
    float* rec = p.records + s * kMdRecord;
    reinterpret_cast<float4*>(rec)[0] = {r.a.x, r.a.y, r.a.z, r.ab.x};
    reinterpret_cast<float4*>(rec)[1] = {r.ab.y, r.ab.z, r.ac.x, r.ac.y};
    reinterpret_cast<float4*>(rec)[2] = {r.ac.z, r.r_ab, r.r_ac, r.r_bc};
    reinterpret_cast<float4*>(rec)[3] = {r.d00, r.d01, r.d11, r.rden};
    float* ed = p.edges + s * kMdEdge;
    reinterpret_cast<float4*>(ed)[0] = {e.b.x, e.b.y, e.b.z, e.bc.x};
    reinterpret_cast<float4*>(ed)[1] = {e.bc.y, e.bc.z, e.lo.x, e.lo.y};
    reinterpret_cast<float4*>(ed)[2] = {e.lo.z, e.hi.x, e.hi.y, e.hi.z};
    p.slot_tri[s] = ok ? o : -1;
  }
  F3 lo = e.lo, hi = e.hi;                                                       // of a slot without a triangle: the empty box
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    lo = {fminf(lo.x, __shfl_xor(lo.x, m)), fminf(lo.y, __shfl_xor(lo.y, m)), fminf(lo.z, __shfl_xor(lo.z, m))};
    hi = {fmaxf(hi.x, __shfl_xor(hi.x, m)), fmaxf(hi.y, __shfl_xor(hi.y, m)), fmaxf(hi.z, __shfl_xor(hi.z, m))};
  }
  const int kept = __popcll(__ballot(ok));
  if (slot && (threadIdx.x & 63) == 0) {
    float* box = p.tile_box + (s / kMdTile) * kSurfBox;
    reinterpret_cast<float4*>(box)[0] = {lo.x, lo.y, lo.z, hi.x};
    reinterpret_cast<float4*>(box)[1] = {hi.y, hi.z, (float)kept, 0.f};
  }
  wave_add(p.dropped_count, s < p.T && !ok ? 1 : 0);                             // as many failed slots as triangles without one
}

// the triangles no slot asked for (an `order` with repeats or entries out of range)
__global__ __launch_bounds__(kMdThreads) void md_unplaced_kernel(const RecordParams p) {
  const long long t = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (t >= p.T || p.tri_slot[t] != kMdNoSlot) return;
  p.tri_slot[t] = -1;
  p.area2[t] = 0.f;
  p.normal[3 * t] = 0.f; p.normal[3 * t + 1] = 0.f; p.normal[3 * t + 2] = 0.f;
  p.dropped[t] = 1;
}

// ---------------------------------------------------------------- closest point ----------------------------------------------
struct ClosestParams {
  const float* records; const float* edges; const int* slot_tri; const float* tile_box;
  const float* query;
  const int* qorder;               // or null: identity
  const int* start;                // or null: every wave starts at tile 0
  float* d2; int* tri; float* point; unsigned char* region;   // region: or null
  int* visited;                    // or null: per wave, the tiles it evaluated
  long long Q;
  int n_tiles, cull;
};

__device__ __forceinline__ Rec md_rec(const float* f) {
  return {{f[0], f[1], f[2]}, {f[3], f[4], f[5]}, {f[6], f[7], f[8]}, f[9], f[10], f[11], f[12], f[13], f[14], f[15]};
}
__device__ __forceinline__ Edge md_edge(const float* f) {
  return {{f[0], f[1], f[2]}, {f[3], f[4], f[5]}, {f[6], f[7], f[8]}, {f[9], f[10], f[11]}};
}

// The 28 floats of a slot are read at a wave-uniform address: scalar loads (the loop stores nothing, so they are unclobbered).
__global__ __launch_bounds__(kMdThreads) void md_closest_kernel(const ClosestParams p) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * kSurfWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave * 64 >= p.Q) return;                                                  // uniform over the wave
  const long long i = wave * 64 + lane;
  long long row = -1;
  if (i < p.Q) {
    row = p.qorder ? (long long)p.qorder[i] : i;
    if (!in_range(row, p.Q)) row = -1;                                           // before any address is formed
  }
  const bool live = row >= 0;
  const F3 q = live ? f3(p.query + 3 * row) : F3{0.f, 0.f, 0.f};
  float best = INFINITY;
  int btri = -1, bslot = -1;
  const int n = p.n_tiles;
  int s = p.start ? __builtin_amdgcn_readfirstlane(p.start[wave]) : 0;
  s = s < 0 ? 0 : s >= n ? n - 1 : s;
  const int reach = s > n - 1 - s ? s : n - 1 - s;
  int evaluated = 0;
  for (int k = 0; k <= 2 * reach; ++k) {                                         // s, s + 1, s - 1, s + 2, ...
    const int d = (k + 1) >> 1, t = (k & 1) ? s + d : s - d;
    if (t < 0 || t >= n) continue;
    if (p.cull) {
      const float* box = p.tile_box + (long long)t * kSurfBox;
      const float lb = box_lb(q, f3(box), f3(box + 3));
      const bool skip = !live || !(lb <= best);
      if (box[kSurfBoxKept] == 0.f || __all(skip)) continue;                     // the one decision of the wave
    }
    ++evaluated;
    const long long s0 = (long long)t * kMdTile;
#pragma unroll 2
    for (int j = 0; j < kMdTile; ++j) {
      const Rec r = md_rec(p.records + (s0 + j) * kMdRecord);
      const Edge e = md_edge(p.edges + (s0 + j) * kMdEdge);
      const int tri = p.slot_tri[s0 + j];
      int region; F3 P;
      const float v = tri_value(r, e, q, region, P);
      if (md_better(v, tri, best, btri)) { best = v; btri = tri; bslot = (int)s0 + j; }
    }
  }
  if (p.visited && lane == 0) p.visited[wave] = evaluated;
  if (!live) return;
  int region = 0;
  F3 P = {0.f, 0.f, 0.f};
  if (bslot >= 0) tri_value(md_rec(p.records + (long long)bslot * kMdRecord), md_edge(p.edges + (long long)bslot * kMdEdge), q, region, P);
  p.d2[row] = best;
  p.tri[row] = btri;
  p.point[3 * row] = P.x; p.point[3 * row + 1] = P.y; p.point[3 * row + 2] = P.z;
  if (p.region) p.region[row] = (unsigned char)region;
}

// ---------------------------------------------------------------- samples ----------------------------------------------------
__global__ __launch_bounds__(kMdThreads) void md_weights_kernel(const float* area2, const unsigned char* dropped, long long T, const float* amax,
                                                                long long* weights) {
  const long long t = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (t >= T) return;
  const float x = floorf(area2[t] * ((float)kMdWeightOne / *amax));
  const long long w = x >= 1.f ? (x < 4.f * kMdWeightOne ? (long long)x : 4ll * kMdWeightOne) : 1;      // a NaN gives 1
  weights[t] = dropped[t] ? 0 : w;
}

struct SampleParams {
  const float* verts; const long long* tris; const long long* cum; const long long* r; const float* u;
  float* points; int* tri;
  long long V, T, n;
};

__global__ __launch_bounds__(kMdThreads) void md_sample_kernel(const SampleParams p) {
  const long long i = (long long)blockIdx.x * kMdThreads + threadIdx.x;
  if (i >= p.n) return;
  const long long total = p.T > 0 ? p.cum[p.T - 1] : 0;
  int t = -1;
  F3 pt = {0.f, 0.f, 0.f};
  if (total > 0) {
    const unsigned long long r = (unsigned long long)p.r[i] & ((1ull << 53) - 1);
    const unsigned long long target = (__umul64hi(r, (unsigned long long)total) << 11) | ((r * (unsigned long long)total) >> 53);   // < total
    long long lo = 0, hi = p.T - 1;                                              // the first t with cum[t] > target
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((unsigned long long)p.cum[mid] > target) hi = mid; else lo = mid + 1;
    }
    F3 a, b, c;
    if (load_corners(p.verts, p.tris, p.V, lo, a, b, c)) {                       // (a foreign `cum` may point anywhere) else: tri = -1
      const float u0 = p.u[2 * i], u1 = p.u[2 * i + 1];
      const float s = sqrtf(u0), b0 = 1.f - s, b1 = s * (1.f - u1), b2 = s * u1;
      pt = add3(add3(mul3(a, b0), mul3(b, b1)), mul3(c, b2));
      t = (int)lo;
    }
  }
  p.tri[i] = t;
  p.points[3 * i] = pt.x; p.points[3 * i + 1] = pt.y; p.points[3 * i + 2] = pt.z;
}

// ---------------------------------------------------------------- statistics -------------------------------------------------
struct StatParams {
  const float* d2; const int* tri_src; const int* tri_dst; const float* n_src; const float* n_dst;
  double* parts; double* parts_max;
  long long n, T_src, T_dst;
  int n_thresholds;
  float tau[kMdMaxThresholds];
};

template <int THREADS>
__device__ inline void block_max_d(double v, double* dst) {
  __shared__ double red[THREADS / 64];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) s = fmax(s, red[w]);
    *dst = s;
  }
}

__global__ __launch_bounds__(kMdThreads) void md_stats_kernel(const StatParams p) {
  double acc[kMdStatSlots];
#pragma unroll
  for (int k = 0; k < kMdStatSlots; ++k) acc[k] = 0.0;
  double top = 0.0;
  for (long long i = (long long)blockIdx.x * kMdThreads + threadIdx.x; i < p.n; i += (long long)gridDim.x * kMdThreads) {
    const int ts = p.tri_src ? p.tri_src[i] : 0, td = p.tri_dst ? p.tri_dst[i] : 0;
    if (ts < 0 || td < 0) { acc[4] += 1.0; continue; }
    const float v = p.d2[i];
    if (!(v >= 0.f && v < INFINITY)) continue;
    const float d = sqrtf(v);
    acc[0] += (double)d;
    acc[1] += (double)d * (double)d;
    acc[3] += 1.0;
    top = fmax(top, (double)d);
#pragma unroll
    for (int k = 0; k < kMdMaxThresholds; ++k)
      if (k < p.n_thresholds && d <= p.tau[k]) acc[5 + k] += 1.0;
    if (p.n_src && p.n_dst && p.tri_src && p.tri_dst && ts < p.T_src && td < p.T_dst)
      acc[2] += (double)fabsf(dot3(f3(p.n_src + 3ll * ts), f3(p.n_dst + 3ll * td)));
  }
  block_sum_d<kMdThreads, kMdStatSlots>(acc, p.parts + (long long)blockIdx.x * kMdStatSlots);
  block_max_d<kMdThreads>(top, p.parts_max + blockIdx.x);
}

// out_f64 = [sum d, sum d^2, max d, sum |n.n|]; out_i64 = [within[0 .. 8), finite rows, rows left out]
__global__ __launch_bounds__(kMdThreads) void md_stats_finish_kernel(const double* parts, const double* parts_max, long long n_parts, double* out_f64,
                                                                     long long* out_i64) {
  __shared__ double total[kMdStatSlots + 1];
  gather_sum_d<kMdThreads, kMdStatSlots>(parts, n_parts, total);
  double top = 0.0;
  for (long long i = threadIdx.x; i < n_parts; i += kMdThreads) top = fmax(top, parts_max[i]);
  block_max_d<kMdThreads>(top, total + kMdStatSlots);
  __syncthreads();
  if (threadIdx.x == 0) {
    out_f64[0] = total[0]; out_f64[1] = total[1]; out_f64[2] = total[kMdStatSlots]; out_f64[3] = total[2];
    for (int k = 0; k < kMdMaxThresholds; ++k) out_i64[k] = (long long)total[5 + k];      // counts below 2^31: exact in float64
    out_i64[kMdMaxThresholds] = (long long)total[3];
    out_i64[kMdMaxThresholds + 1] = (long long)total[4];
  }
}

inline long long md_stat_blocks(long long n) { return capped_blocks(n, kMdThreads, kMdStatBlocks); }
// scratch of mf_surface_stats: the sums' partials float64 [workgroups][13] | the maxima float64 [workgroups].  Returns its size.
inline long long md_stat_scratch(void* scratch, long long blocks, double*& parts, double*& parts_max) {
  Carver c(scratch);
  parts = c.take<double>(blocks * kMdStatSlots);
  parts_max = c.take<double>(blocks);
  return c.bytes();
}

}  // namespace mf

using namespace mf;

extern "C" int32_t mf_surface_records(const float* verts, int64_t V, const int64_t* tris, int64_t T, const int32_t* order, float* records,
                                   float* edges, int32_t* slot_tri, float* tile_box, int32_t* tri_slot, float* area2, float* normal,
                                   uint8_t* dropped, int64_t* dropped_count, void* stream) {
  if (!surf_count_ok(V) || !surf_count_ok(T))
    return fail(MF_E_INVALID, "mf_surface_records: V=%lld T=%lld (both in [0, 2^31 - 1))", (long long)V, (long long)T);
  if (!dropped_count) return fail(MF_E_INVALID, "mf_surface_records: null dropped_count");
  if (T > 0 && (!tris || !records || !edges || !slot_tri || !tile_box || !tri_slot || !area2 || !normal || !dropped))
    return fail(MF_E_INVALID, "mf_surface_records: null tris or output with T=%lld", (long long)T);
  if (T > 0 && V > 0 && !verts) return fail(MF_E_INVALID, "mf_surface_records: null verts with V=%lld", (long long)V);
  if (T > 0 && surf_alias("mf_surface_records", {records, edges, slot_tri, tile_box, tri_slot, area2, normal, dropped, dropped_count}, {verts, tris, order})) return MF_E_INVALID;
  RecordParams p{};
  p.verts = verts; p.tris = reinterpret_cast<const long long*>(tris); p.order = order;
  p.records = records; p.edges = edges; p.slot_tri = slot_tri; p.tile_box = tile_box;
  p.tri_slot = tri_slot; p.area2 = area2; p.normal = normal; p.dropped = dropped;
  p.dropped_count = reinterpret_cast<long long*>(dropped_count);
  p.V = V; p.T = T; p.Tpad = align_up(T, kMdTile);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(kMdThreads), grid((unsigned)(T > 0 ? surf_blocks(p.Tpad) : 1));
  hipLaunchKernelGGL(md_fill_kernel, grid, block, 0, s, p);
  if (T > 0) {
    hipLaunchKernelGGL(md_claim_kernel, grid, block, 0, s, p);
    hipLaunchKernelGGL(md_build_kernel, grid, block, 0, s, p);
    hipLaunchKernelGGL(md_unplaced_kernel, grid, block, 0, s, p);
  }
  return check_launch("mf_surface_records");
}

extern "C" int32_t mf_surface_closest(const float* records, const float* edges, const int32_t* slot_tri, const float* tile_box, int64_t T,
                                   const float* query, int64_t Q, const int32_t* qorder, const int32_t* start, int32_t mode, float* d2,
                                   int32_t* tri, float* point, uint8_t* region, int32_t* visited, void* stream) {
  if (!surf_count_ok(T) || !surf_count_ok(Q))
    return fail(MF_E_INVALID, "mf_surface_closest: T=%lld Q=%lld (both in [0, 2^31 - 1))", (long long)T, (long long)Q);
  if (mode < 0 || mode > 1) return fail(MF_E_INVALID, "mf_surface_closest: mode=%d (0 sweep, 1 cull)", mode);
  if (Q == 0) return MF_OK;
  if (T > 0 && (!records || !edges || !slot_tri || !tile_box)) return fail(MF_E_INVALID, "mf_surface_closest: null records, edges, slot_tri or tile_box");
  if (!query || !d2 || !tri || !point) return fail(MF_E_INVALID, "mf_surface_closest: null query, d2, tri or point");
  if (surf_alias("mf_surface_closest", {d2, tri, point, region, visited}, {records, edges, slot_tri, tile_box, query, qorder, start})) return MF_E_INVALID;
  ClosestParams p{};
  p.records = records; p.edges = edges; p.slot_tri = slot_tri; p.tile_box = tile_box; p.query = query; p.qorder = qorder; p.start = start;
  p.d2 = d2; p.tri = tri; p.point = point; p.region = region; p.visited = visited;
  p.Q = Q; p.n_tiles = surf_tiles(T); p.cull = mode;
  const dim3 block(kMdThreads), grid((unsigned)surf_blocks(Q));
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(md_closest_kernel, grid, block, 0, s, p);
  return check_launch("mf_surface_closest");
}

extern "C" int32_t mf_surface_weights(const float* area2, const uint8_t* dropped, int64_t T, const float* amax, int64_t* weights, void* stream) {
  if (!surf_count_ok(T)) return fail(MF_E_INVALID, "mf_surface_weights: T=%lld (in [0, 2^31 - 1))", (long long)T);
  if (T == 0) return MF_OK;
  if (!area2 || !dropped || !amax || !weights) return fail(MF_E_INVALID, "mf_surface_weights: null area2, dropped, amax or weights");
  if ((const void*)weights == area2 || (const void*)weights == dropped || (const void*)weights == amax)
    return fail(MF_E_INVALID, "mf_surface_weights: weights aliases an input");
  hipLaunchKernelGGL(md_weights_kernel, dim3((unsigned)surf_blocks(T)), dim3(kMdThreads), 0, static_cast<hipStream_t>(stream), area2, dropped,
                     (long long)T, amax, reinterpret_cast<long long*>(weights));
  return check_launch("mf_surface_weights");
}

extern "C" int32_t mf_surface_sample(const float* verts, int64_t V, const int64_t* tris, int64_t T, const int64_t* cum, const int64_t* r,
                                  const float* u, int64_t n, float* points, int32_t* tri, void* stream) {
  if (!surf_count_ok(V) || !surf_count_ok(T) || !surf_count_ok(n))
    return fail(MF_E_INVALID, "mf_surface_sample: V=%lld T=%lld n=%lld (each in [0, 2^31 - 1))", (long long)V, (long long)T, (long long)n);
  if (n == 0) return MF_OK;
  if (!points || !tri) return fail(MF_E_INVALID, "mf_surface_sample: null points or tri");
  if (T > 0 && (!tris || !cum || !r || !u || (V > 0 && !verts))) return fail(MF_E_INVALID, "mf_surface_sample: null verts, tris, cum, r or u");
  if (surf_alias("mf_surface_sample", {points, tri}, {verts, tris, cum, r, u})) return MF_E_INVALID;
  SampleParams p{};
  p.verts = verts; p.tris = reinterpret_cast<const long long*>(tris); p.cum = reinterpret_cast<const long long*>(cum);
  p.r = reinterpret_cast<const long long*>(r); p.u = u; p.points = points; p.tri = tri;
  p.V = V; p.T = T; p.n = n;
  hipLaunchKernelGGL(md_sample_kernel, dim3((unsigned)surf_blocks(n)), dim3(kMdThreads), 0, static_cast<hipStream_t>(stream), p);
  return check_launch("mf_surface_sample");
}

extern "C" int64_t mf_surface_stats_scratch_bytes(int64_t n) {
  if (!surf_count_ok(n)) return fail(MF_E_INVALID, "mf_surface_stats_scratch_bytes: n=%lld (in [0, 2^31 - 1))", (long long)n);
  double *parts, *parts_max;
  return md_stat_scratch(nullptr, md_stat_blocks(n), parts, parts_max);
}

extern "C" int32_t mf_surface_stats(const float* d2, int64_t n, const int32_t* tri_src, const int32_t* tri_dst, const float* normal_src,
                                    int64_t T_src, const float* normal_dst, int64_t T_dst, const float* thresholds, int32_t n_thresholds,
                                    double* out_f64, int64_t* out_i64, void* scratch, void* stream) {
  if (!surf_count_ok(n) || !surf_count_ok(T_src) || !surf_count_ok(T_dst))
    return fail(MF_E_INVALID, "mf_surface_stats: n=%lld T_src=%lld T_dst=%lld (each in [0, 2^31 - 1))", (long long)n, (long long)T_src, (long long)T_dst);
  if (n_thresholds < 0 || n_thresholds > kMdMaxThresholds || (n_thresholds > 0 && !thresholds))
    return fail(MF_E_INVALID, "mf_surface_stats: n_thresholds=%d (0 .. %d, with a host array)", n_thresholds, kMdMaxThresholds);
  if (!out_f64 || !out_i64 || !scratch) return fail(MF_E_INVALID, "mf_surface_stats: null out_f64, out_i64 or scratch");
  if (n > 0 && !d2) return fail(MF_E_INVALID, "mf_surface_stats: null d2 with n=%lld", (long long)n);
  StatParams p{};
  p.d2 = d2; p.tri_src = tri_src; p.tri_dst = tri_dst; p.n_src = normal_src; p.n_dst = normal_dst;
  p.n = n; p.T_src = T_src; p.T_dst = T_dst; p.n_thresholds = n_thresholds;
  for (int k = 0; k < kMdMaxThresholds; ++k) p.tau[k] = k < n_thresholds ? thresholds[k] : 0.f;
  const long long blocks = md_stat_blocks(n);
  md_stat_scratch(scratch, blocks, p.parts, p.parts_max);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (blocks > 0) hipLaunchKernelGGL(md_stats_kernel, dim3((unsigned)blocks), dim3(kMdThreads), 0, s, p);
  hipLaunchKernelGGL(md_stats_finish_kernel, dim3(1), dim3(kMdThreads), 0, s, p.parts, p.parts_max, blocks, out_f64,
                     reinterpret_cast<long long*>(out_i64));
  return check_launch("mf_surface_stats");
}
