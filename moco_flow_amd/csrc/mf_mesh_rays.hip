// mf_mesh_rays.hip -- rays against a triangle mesh: the first hit, or whether there is one (include/mocoflow_hip.h:
// mf_surface_corners, mf_surface_cast).  THE CONTRACT IS FIXED ARITHMETIC, as in mf_mesh_distance.hip: every fp32
// operation below is rounded once, in the order written, with no FMA, so that tests/mesh_rays_oracle.py restates every output in
// np.float32 bit for bit.
//   mr_corners_kernel      mf_surface_corners: per slot of the index a 16-float row -- the three vertices as read, the triangle's box
//   mr_cast_kernel<MODE>   mf_surface_cast: a ray per lane, on the tile walk of include/mocoflow_hip.h (a lane tests the tile's sheared
//                          box).  MODE 0 first hit, 1 any hit.
// A ray picks its dominant axis kz and shears the mesh along itself: a vertex p becomes x = q[kx] - Sx q[kz], y = q[ky] - Sy q[kz],
// z = Sz q[kz] with q = p - o.  These three numbers depend on the vertex and the ray alone, so two triangles that share an edge
// see the same sheared end points, the edge function of one is exactly the negated edge function of the other, and a rounded
// difference of two rounded products never has the sign opposite to the exact one: a ray cannot slip between them (watertight).
// Subtracting a fixed o, multiplying by a fixed S and min / max are monotone under rounding, so the sheared intervals of a box
// that contains a vertex contain the vertex's x, y, z -- exactly, in fp32 -- and a tile is skipped with no slack: the culled
// search equals the full sweep bit for bit, whatever the tile order, the visiting order or the launch shape.  The result of MODE
// 0 is the lexicographic minimum of (t, caller's triangle index).  No grid-stride loop (a wave per 64 rays), no atomics.
// (the Makefile builds every unit with -ffp-contract=off; the pragma keeps it true for a build that forgets it)
#pragma clang fp contract(off)
#include <cmath>

#include "mf_surface.hpp"

namespace mf {

constexpr int kMrCorner = 16;                    // floats per corner row: a, b, c, lo, hi, 0

// ---------------------------------------------------------------- corner rows ------------------------------------------------
struct CornerParams {
  const float* verts;
  const long long* tris;
  const int* slot_tri;
  float* corners;
  long long V, T, Tpad;
};

__global__ __launch_bounds__(kSurfThreads) void mr_corners_kernel(const CornerParams p) {
  const long long s = (long long)blockIdx.x * kSurfThreads + threadIdx.x;
  if (s >= p.Tpad) return;
  F3 a = {0.f, 0.f, 0.f}, b = a, c = a, lo = a, hi = a;
  const long long t = p.slot_tri[s];
  if (in_range(t, p.T) && load_corners(p.verts, p.tris, p.V, t, a, b, c)) {      // else: a row of zeros
    lo = min3(min3(a, b), c);
    hi = max3(max3(a, b), c);
  }
  float* row = p.corners + s * kMrCorner;
  reinterpret_cast<float4*>(row)[0] = {a.x, a.y, a.z, b.x};
  reinterpret_cast<float4*>(row)[1] = {b.y, b.z, c.x, c.y};
  reinterpret_cast<float4*>(row)[2] = {c.z, lo.x, lo.y, lo.z};
  reinterpret_cast<float4*>(row)[3] = {hi.x, hi.y, hi.z, 0.f};
}

// ---------------------------------------------------------------- the cast ---------------------------------------------------
struct CastParams {
  const float* corners; const int* slot_tri; const float* tile_box;
  const float* origins; const float* dirs; const float* t_min; const float* t_max;
  const int* qorder;               // or null: identity
  const int* start;                // or null: every wave starts at tile 0
  float* t; int* tri; float* bary; unsigned char* hit;
  int* visited;                    // or null: per wave, the tiles it evaluated
  long long Q, ray_stride, bound_stride;
  int n_tiles, cull;
};

// A live ray: the origin's components in the order (kx, ky, kz), the shear, the range of t.  k0 / k1: the axis is 0 / 1 (else 2).
struct Ray {
  F3 o;
  float Sx, Sy, Sz, t_min, t_max;
  bool kx0, kx1, ky0, ky1, kz0, kz1;
};

__device__ __forceinline__ float pick(F3 p, bool k0, bool k1) { return k0 ? p.x : k1 ? p.y : p.z; }
__device__ __forceinline__ F3 permuted(F3 p, const Ray& r) { return {pick(p, r.kx0, r.kx1), pick(p, r.ky0, r.ky1), pick(p, r.kz0, r.kz1)}; }

// the sheared vertex: q = p - o; x = q[kx] - Sx q[kz], y = q[ky] - Sy q[kz], z = Sz q[kz]
__device__ __forceinline__ F3 sheared(F3 p, const Ray& r) {
  const F3 q = sub3(permuted(p, r), r.o);
  return {q.x - r.Sx * q.z, q.y - r.Sy * q.z, r.Sz * q.z};
}

struct Edges { float U, V, W, det; };
__device__ __forceinline__ Edges edge_functions(F3 A, F3 B, F3 C) {
  const float U = C.x * B.y - C.y * B.x, V = A.x * C.y - A.y * C.x, W = B.x * A.y - B.y * A.x;
  return {U, V, W, (U + V) + W};
}

// whether the ray accepts the triangle of a corner row, and at which t
__device__ __forceinline__ bool tri_hit(const float* row, const Ray& r, float& t) {
  const F3 A = sheared(f3(row), r), B = sheared(f3(row + 3), r), C = sheared(f3(row + 6), r);
  const Edges e = edge_functions(A, B, C);
  const bool sign = (e.U >= 0.f && e.V >= 0.f && e.W >= 0.f) || (e.U <= 0.f && e.V <= 0.f && e.W <= 0.f);
  const bool own = fminf(fminf(A.x, B.x), C.x) <= 0.f && 0.f <= fmaxf(fmaxf(A.x, B.x), C.x) &&
                   fminf(fminf(A.y, B.y), C.y) <= 0.f && 0.f <= fmaxf(fmaxf(A.y, B.y), C.y);
  t = INFINITY;
  if (!(sign && own && e.det != 0.f)) return false;
  const float t_raw = ((e.U * A.z + e.V * B.z) + e.W * C.z) * (1.f / e.det);
  t = fminf(fmaxf(t_raw, fminf(fminf(A.z, B.z), C.z)), fmaxf(fmaxf(A.z, B.z), C.z));
  return r.t_min <= t && t <= r.t_max;
}

// whether the ray wants a tile: 0 inside the sheared box's x and y intervals, its z interval meeting [t_min, min(t_max, best)]
__device__ __forceinline__ bool wants_tile(const float* box, const Ray& r, float best) {
  const F3 l = sub3(permuted(f3(box), r), r.o), h = sub3(permuted(f3(box + 3), r), r.o);
  const float xl = r.Sx * l.z, xh = r.Sx * h.z, yl = r.Sy * l.z, yh = r.Sy * h.z, zl = r.Sz * l.z, zh = r.Sz * h.z;
  const float x0 = l.x - fmaxf(xl, xh), x1 = h.x - fminf(xl, xh);
  const float y0 = l.y - fmaxf(yl, yh), y1 = h.y - fminf(yl, yh);
  const float z0 = fminf(zl, zh), z1 = fmaxf(zl, zh);
  return x0 <= 0.f && 0.f <= x1 && y0 <= 0.f && 0.f <= y1 && !(z1 < r.t_min) && !(z0 > r.t_max) && z0 <= best;
}

// The 16 floats of a slot are read at a wave-uniform address: scalar loads (the loop stores nothing, so they are unclobbered).
template <int MODE>
__global__ __launch_bounds__(kSurfThreads) void mr_cast_kernel(const CastParams p) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * kSurfWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave * 64 >= p.Q) return;                                                  // uniform over the wave
  const long long i = wave * 64 + lane;
  long long row = -1;
  if (i < p.Q) {
    row = p.qorder ? (long long)p.qorder[i] : i;
    if (!in_range(row, p.Q)) row = -1;                                           // before any address is formed
  }
  Ray r{};
  bool live = false;
  if (row >= 0) {
    const F3 o = f3(p.origins + row * p.ray_stride), d = f3(p.dirs + row * p.ray_stride);
    r.t_min = p.t_min[row * p.bound_stride];
    r.t_max = p.t_max[row * p.bound_stride];
    live = finite3(o) && finite3(d) && !(d.x == 0.f && d.y == 0.f && d.z == 0.f) && r.t_min <= r.t_max;
    int kz = 0;                                                                  // the first axis of the largest |d|
    float top = fabsf(d.x);
    if (fabsf(d.y) > top) { kz = 1; top = fabsf(d.y); }
    if (fabsf(d.z) > top) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = kz == 0 ? d.x : kz == 1 ? d.y : d.z;
    if (dz < 0.f) { const int k = kx; kx = ky; ky = k; }
    r.kx0 = kx == 0; r.kx1 = kx == 1; r.ky0 = ky == 0; r.ky1 = ky == 1; r.kz0 = kz == 0; r.kz1 = kz == 1;
    r.o = permuted(o, r);
    const F3 dp = permuted(d, r);
    r.Sx = dp.x / dp.z; r.Sy = dp.y / dp.z; r.Sz = 1.f / dp.z;
  }
  float best = INFINITY;
  int btri = -1, bslot = -1;
  bool found = false;
  const int n = p.n_tiles;
  int s = p.start ? __builtin_amdgcn_readfirstlane(p.start[wave]) : 0;
  s = s < 0 ? 0 : s >= n ? n - 1 : s;
  const int reach = s > n - 1 - s ? s : n - 1 - s;
  int evaluated = 0;
  for (int k = 0; k <= 2 * reach; ++k) {                                         // s, s + 1, s - 1, s + 2, ...
    const int d = (k + 1) >> 1, t = (k & 1) ? s + d : s - d;
    if (t < 0 || t >= n) continue;
    if (p.cull) {
      const bool done = !live || (MODE == 1 && found);
      if (__all(done)) break;                                                    // no lane wants anything any more
      const float* box = p.tile_box + (long long)t * kSurfBox;
      const bool want = !done && wants_tile(box, r, best);
      if (box[kSurfBoxKept] == 0.f || !__any(want)) continue;                              // the one decision of the wave
    }
    ++evaluated;
    const long long s0 = (long long)t * kSurfTile;
#pragma unroll 2
    for (int j = 0; j < kSurfTile; ++j) {
      const int tri = p.slot_tri[s0 + j];
      float th;
      const bool ok = tri_hit(p.corners + (s0 + j) * kMrCorner, r, th) && live && tri >= 0;
      if (MODE == 1) {
        found = found || ok;
      } else if (ok && (th < best || (th == best && (unsigned)tri < (unsigned)btri))) {
        best = th; btri = tri; bslot = (int)s0 + j;
      }
    }
  }
  if (p.visited && lane == 0) p.visited[wave] = evaluated;
  if (row < 0) return;
  if (MODE == 1) {
    p.hit[row] = found ? 1 : 0;
    return;
  }
  F3 bary = {0.f, 0.f, 0.f};
  if (bslot >= 0) {                                                              // the winner's, recomputed from its slot
    const float* c = p.corners + (long long)bslot * kMrCorner;
    const Edges e = edge_functions(sheared(f3(c), r), sheared(f3(c + 3), r), sheared(f3(c + 6), r));
    const float rdet = 1.f / e.det;
    bary = {e.U * rdet, e.V * rdet, e.W * rdet};
  }
  p.t[row] = best;
  p.tri[row] = btri;
  p.bary[3 * row] = bary.x; p.bary[3 * row + 1] = bary.y; p.bary[3 * row + 2] = bary.z;
}

}  // namespace mf

using namespace mf;

extern "C" int32_t mf_surface_corners(const float* verts, int64_t V, const int64_t* tris, int64_t T, const int32_t* slot_tri, float* corners,
                                      void* stream) {
  if (!surf_count_ok(V) || !surf_count_ok(T))
    return fail(MF_E_INVALID, "mf_surface_corners: V=%lld T=%lld (both in [0, 2^31 - 1))", (long long)V, (long long)T);
  if (T == 0) return MF_OK;
  if (!tris || !slot_tri || !corners) return fail(MF_E_INVALID, "mf_surface_corners: null tris, slot_tri or corners with T=%lld", (long long)T);
  if (V > 0 && !verts) return fail(MF_E_INVALID, "mf_surface_corners: null verts with V=%lld", (long long)V);
  if (!is_aligned(corners, 16)) return fail(MF_E_INVALID, "mf_surface_corners: corners must be 16-byte aligned");
  if ((const void*)corners == verts || (const void*)corners == tris || (const void*)corners == slot_tri)
    return fail(MF_E_INVALID, "mf_surface_corners: corners aliases an input");
  CornerParams p{};
  p.verts = verts; p.tris = reinterpret_cast<const long long*>(tris); p.slot_tri = slot_tri; p.corners = corners;
  p.V = V; p.T = T; p.Tpad = align_up(T, kSurfTile);
  hipLaunchKernelGGL(mr_corners_kernel, dim3((unsigned)surf_blocks(p.Tpad)), dim3(kSurfThreads), 0, static_cast<hipStream_t>(stream), p);
  return check_launch("mf_surface_corners");
}

extern "C" int32_t mf_surface_cast(const float* corners, const int32_t* slot_tri, const float* tile_box, int64_t T, const float* origins,
                                   const float* dirs, int64_t ray_stride, const float* t_min, const float* t_max, int64_t bound_stride,
                                   int64_t Q, const int32_t* qorder, const int32_t* start, int32_t mode, int32_t cull, float* t, int32_t* tri,
                                   float* bary, uint8_t* hit, int32_t* visited, void* stream) {
  if (!surf_count_ok(T) || !surf_count_ok(Q))
    return fail(MF_E_INVALID, "mf_surface_cast: T=%lld Q=%lld (both in [0, 2^31 - 1))", (long long)T, (long long)Q);
  if (mode < 0 || mode > 1) return fail(MF_E_INVALID, "mf_surface_cast: mode=%d (0 first, 1 any)", mode);
  if (cull < 0 || cull > 1) return fail(MF_E_INVALID, "mf_surface_cast: cull=%d (0 sweep, 1 cull)", cull);
  if (ray_stride < 3 || ray_stride >= kIndexLimit || bound_stride < 0 || bound_stride >= kIndexLimit)
    return fail(MF_E_INVALID, "mf_surface_cast: ray_stride=%lld (>= 3 floats) bound_stride=%lld (>= 0; 0: one bound for all)",
                (long long)ray_stride, (long long)bound_stride);
  if (Q == 0) return MF_OK;
  if (T > 0 && (!corners || !slot_tri || !tile_box)) return fail(MF_E_INVALID, "mf_surface_cast: null corners, slot_tri or tile_box");
  if (!origins || !dirs || !t_min || !t_max) return fail(MF_E_INVALID, "mf_surface_cast: null origins, dirs, t_min or t_max");
  if (mode == 0 && (!t || !tri || !bary)) return fail(MF_E_INVALID, "mf_surface_cast: mode 0 with null t, tri or bary");
  if (mode == 1 && !hit) return fail(MF_E_INVALID, "mf_surface_cast: mode 1 with null hit");
  if (surf_alias("mf_surface_cast", {t, tri, bary, hit, visited}, {corners, slot_tri, tile_box, origins, dirs, t_min, t_max, qorder, start})) return MF_E_INVALID;
  CastParams p{};
  p.corners = corners; p.slot_tri = slot_tri; p.tile_box = tile_box;
  p.origins = origins; p.dirs = dirs; p.t_min = t_min; p.t_max = t_max; p.qorder = qorder; p.start = start;
  p.t = t; p.tri = tri; p.bary = bary; p.hit = hit; p.visited = visited;
  p.Q = Q; p.ray_stride = ray_stride; p.bound_stride = bound_stride;
  p.n_tiles = surf_tiles(T); p.cull = cull;
  const dim3 block(kSurfThreads), grid((unsigned)surf_blocks(Q));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == 0) hipLaunchKernelGGL(mr_cast_kernel<0>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(mr_cast_kernel<1>, grid, block, 0, s, p);
  return check_launch("mf_surface_cast");
}
