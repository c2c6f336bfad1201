// mf_raster.hip -- a triangle rasterizer for the pictures the reference draws with pyrender (scripts/data_utils.py:23-86 Renderer,
// :273-336 create_init_nerf_data: the stage-1 views of the posed SMPL mesh; :255-263 the SMPL overlay), through the camera of
// mf_rays.hpp::pixel_ray (utils/camera.py:29-81), so that pixel (row j, column i) of a rasterized frame and the NeRF's ray for that
// pixel see the same surface point:
//   mf_project_vertices   world vertices -> snapped screen positions (1/256 pixel) and 1/z
//   mf_rasterize          clear the key plane, then one wave per 64 triangles: coverage in integers, one 64-bit atomicMin per
//                         covered sample
//   mf_raster_resolve     key plane -> face, depth, perspective-correct barycentrics
//   mf_raster_interpolate vertex attributes through (face, bary)
//   mf_raster_shade       key plane -> rgba bytes, mask, depth, ray_t, face in ONE launch (render_mesh)
// pyrender's metallic-roughness BRDF and its point lights are NOT restated (include/mocoflow_hip.h).
//
// PROJECTION (fp32, every operation rounded once: the unit is built with -ffp-contract=off), R = c2w[:, :3], t = c2w[:, 3]:
//   p = v - t                       c_a = (R[0][a] p.x + R[1][a] p.y) + R[2][a] p.z        (p_cam = R^T p)
//   z = -c_z                        x = cx + (f c_x) / z          y = cy - (f c_y) / z        inv_z = 1 / z
//   screen = (rintf(256 x), rintf(256 y)), saturated at +-2^30; z <= znear (or a NaN anywhere): screen = (INT32_MIN, INT32_MIN),
//   inv_z = 0 -- the flag a triangle is dropped by.
//
// COVERAGE (integers only).  The sample of pixel (j, i) is S = (256 i + o, 256 j + o), o = 0 (pixel_offset 0) or 128 (0.5).  For
// the edge opposite vertex k, from A = v_{k+1} to B = v_{k+2} (indices mod 3), with D = s (B - A):
//   e_k = D.x (S.y - A.y) - D.y (S.x - A.x)          int64: |D| <= 2^25 and |S - A| <= 2^25 inside the guard band
// s = +1 / -1 is the sign of the doubled area (B0 - A0) x ... = e_0 + e_1 + e_2 (a constant of the triangle), so that the interior
// is e_k > 0 for either winding; s = 0 (zero area) covers nothing.  FILL RULE (top-left, y pointing down the rows): a sample
// with e_k = 0 belongs to the triangle iff the edge is a top edge (D.y == 0 and D.x > 0: horizontal, interior below) or a left
// edge (D.y < 0: interior to its right).  A sample is covered iff this holds for k = 0, 1, 2.  The rule is "the sample moved by
// (eps, eps^2) is strictly inside", so triangles that tile a region -- whatever their windings -- cover each sample of it
// exactly once, on shared edges and at shared vertices alike.
//
// DEPTH AND BARYCENTRICS (fp32), w_k = inv_z of vertex k, E_k = (float) e_k (one rounding, to nearest even), A = e_0 + e_1 + e_2
// in int64 and then (float) A:
//   f_k = E_k w_k        den = (f_0 + f_1) + f_2        z = (float) A / den        bary_k = f_k / den
//
// VISIBILITY: the minimum over covering triangles of the key (bits(z) << 32) | triangle index (z > 0: its bit pattern orders as
// the number does).  A minimum does not depend on the order of arrival: the plane is bit-identical from run to run, and an exact
// depth tie goes to the lower index.  The all-ones key means "no triangle" (T < 2^31 keeps a real key below it).
//
// DROPPED TRIANGLES: a vertex index outside [0, V) (never dereferenced), a flagged vertex, or a vertex beyond +-2^15 pixels: the
// whole triangle is dropped and counted; there is no clipping.
//
// COST: a wave walks the bounding box of each of its 64 triangles in 8 x 8 pixel blocks, one after the other: SMPL and marching
// cubes triangles are one block each; a viewport-filling triangle is H W / 64 steps of ONE wave -- bounded, but many such
// triangles are slow.
#include <cmath>
#include <cstdint>

#include "mf_host.hpp"

namespace mf {

constexpr int kSub = 256;                  // sub-pixel units per pixel
constexpr int kGuard = 1 << 23;            // +-2^15 pixels
constexpr int kSnapMax = 1 << 30;
constexpr int32_t kBehind = INT32_MIN;
constexpr unsigned long long kNoKey = ~0ull;
constexpr int kRasterThreads = 256;

struct ProjCam {
  float R[9], t[3];
  float f, cx, cy, znear;
};

__device__ inline bool snap(float x, int32_t& s) {
  const float v = rintf(x * (float)kSub);
  if (!(v == v)) return false;
  s = v >= (float)kSnapMax ? kSnapMax : (v <= -(float)kSnapMax ? -kSnapMax : (int32_t)v);
  return true;
}

__global__ __launch_bounds__(kRasterThreads) void project_kernel(const float* verts, int V, ProjCam c, int32_t* screen, float* inv_z,
                                                                 float* xy) {
  const int v = blockIdx.x * kRasterThreads + threadIdx.x;
  if (v >= V) return;
  const float px = verts[3 * v] - c.t[0], py = verts[3 * v + 1] - c.t[1], pz = verts[3 * v + 2] - c.t[2];
  const float xc = (c.R[0] * px + c.R[3] * py) + c.R[6] * pz;
  const float yc = (c.R[1] * px + c.R[4] * py) + c.R[7] * pz;
  const float zc = (c.R[2] * px + c.R[5] * py) + c.R[8] * pz;
  const float z = -zc;
  float x = NAN, y = NAN, w = 0.f;
  int32_t sx = kBehind, sy = kBehind;
  if (z > c.znear) {
    x = c.cx + (c.f * xc) / z;
    y = c.cy - (c.f * yc) / z;
    int32_t ax, ay;
    if (snap(x, ax) && snap(y, ay)) {
      sx = ax;
      sy = ay;
      w = 1.f / z;
    }
  }
  screen[2 * v] = sx;
  screen[2 * v + 1] = sy;
  inv_z[v] = w;
  if (xy) {
    xy[2 * v] = x;
    xy[2 * v + 1] = y;
  }
}

// ---- one triangle, as every kernel below sees it ----
struct Tri {
  int32_t x[3], y[3];
  float w[3];
  int32_t sgn;           // sign of the doubled area; 0: covers nothing
};

enum { kTriOk = 0, kTriDropped = 1 };

struct MeshRef {
  const int32_t* screen;
  const float* inv_z;
  const int64_t* tris;
  long long V, T;
};

// vertex indices of triangle t into vi; false: one is outside [0, V)
__device__ inline bool tri_indices(const MeshRef& m, long long t, long long (&vi)[3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    vi[k] = m.tris[3 * t + k];
    ok = ok && vi[k] >= 0 && vi[k] < m.V;
  }
  return ok;
}

__device__ inline int load_tri(const MeshRef& m, long long t, Tri& q) {
  long long vi[3];
  q.sgn = 0;
  if (!tri_indices(m, t, vi)) return kTriDropped;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    q.x[k] = m.screen[2 * vi[k]];
    q.y[k] = m.screen[2 * vi[k] + 1];
    q.w[k] = m.inv_z[vi[k]];
    if (q.x[k] == kBehind || q.x[k] > kGuard || q.x[k] < -kGuard || q.y[k] > kGuard || q.y[k] < -kGuard) return kTriDropped;
  }
  const long long area = (long long)(q.x[1] - q.x[0]) * (q.y[2] - q.y[0]) - (long long)(q.y[1] - q.y[0]) * (q.x[2] - q.x[0]);
  q.sgn = area > 0 ? 1 : (area < 0 ? -1 : 0);
  return kTriOk;
}

// sample (sx, sy) in sub-pixel units against q: covered?  then its depth and barycentrics
__device__ inline bool sample_eval(const Tri& q, int sx, int sy, float& z, float (&b)[3]) {
  if (q.sgn == 0) return false;
  long long e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = (k + 1) % 3, c = (k + 2) % 3;
    const long long dx = (long long)q.sgn * (q.x[c] - q.x[a]), dy = (long long)q.sgn * (q.y[c] - q.y[a]);
    e[k] = dx * (sy - q.y[a]) - dy * (sx - q.x[a]);
    const bool top_left = dy < 0 || (dy == 0 && dx > 0);
    if (e[k] < (top_left ? 0 : 1)) return false;
  }
  const float f0 = (float)e[0] * q.w[0], f1 = (float)e[1] * q.w[1], f2 = (float)e[2] * q.w[2];
  const float den = (f0 + f1) + f2;
  z = (float)(e[0] + e[1] + e[2]) / den;
  b[0] = f0 / den;
  b[1] = f1 / den;
  b[2] = f2 / den;
  return true;
}

__device__ inline int floor_sub(int a) { return a >> 8; }            // floor(a / 256), arithmetic shift
__device__ inline int ceil_sub(int a) { return (a + (kSub - 1)) >> 8; }

struct RasterParams {
  MeshRef m;
  int H, W, off;                     // off: 0 or 128
  unsigned long long* keys;          // (H W)
  unsigned long long* dropped;       // 1
};

struct Box { int i0, i1, j0, j1; };

__global__ __launch_bounds__(64) void raster_walk_kernel(RasterParams p) {
  __shared__ Tri s_tri[64];
  __shared__ Box s_box[64];
  const int lane = threadIdx.x;
  const long long t = (long long)blockIdx.x * 64 + lane;
  Tri q;
  q.sgn = 0;
  Box box = {0, -1, 0, -1};
  bool drop = false;
  if (t < p.m.T) {
    drop = load_tri(p.m, t, q) == kTriDropped;
    if (q.sgn != 0) {
      const int x0 = min(q.x[0], min(q.x[1], q.x[2])), x1 = max(q.x[0], max(q.x[1], q.x[2]));
      const int y0 = min(q.y[0], min(q.y[1], q.y[2])), y1 = max(q.y[0], max(q.y[1], q.y[2]));
      box.i0 = max(0, ceil_sub(x0 - p.off));
      box.i1 = min(p.W - 1, floor_sub(x1 - p.off));
      box.j0 = max(0, ceil_sub(y0 - p.off));
      box.j1 = min(p.H - 1, floor_sub(y1 - p.off));
    }
  }
  const unsigned long long drops = __ballot(drop);
  if (lane == 0 && drops) atomicAdd(p.dropped, (unsigned long long)__popcll(drops));
  s_tri[lane] = q;
  s_box[lane] = box;
  __syncthreads();
  const int li = lane & 7, lj = lane >> 3;
  for (int k = 0; k < 64; ++k) {
    const Box bx = s_box[k];
    if (bx.i0 > bx.i1 || bx.j0 > bx.j1) continue;           // the same for every lane
    const Tri tq = s_tri[k];
    const unsigned long long index = (unsigned long long)blockIdx.x * 64 + k;
    const int bw = (bx.i1 - bx.i0 + 8) >> 3, bh = (bx.j1 - bx.j0 + 8) >> 3;
    for (int by = 0; by < bh; ++by) {
      const int j = bx.j0 + by * 8 + lj;
      for (int bxi = 0; bxi < bw; ++bxi) {
        const int i = bx.i0 + bxi * 8 + li;
        if (i > bx.i1 || j > bx.j1) continue;
        float z, b[3];
        if (sample_eval(tq, i * kSub + p.off, j * kSub + p.off, z, b))
          atomicMin(p.keys + ((long long)j * p.W + i), ((unsigned long long)__float_as_uint(z) << 32) | index);
      }
    }
  }
}

// the winner of pixel pix: false = none; else its triangle, depth and barycentrics (recomputed: the same function, the same bits)
__device__ inline bool resolve_pixel(const RasterParams& p, int pix, long long& t, float& z, float (&b)[3]) {
  const unsigned long long key = p.keys[pix];
  b[0] = b[1] = b[2] = 0.f;
  if (key == kNoKey) return false;
  t = (long long)(key & 0xffffffffull);
  if (t >= p.m.T) return false;                               // (cannot happen with a plane mf_rasterize filled for this mesh)
  Tri q;
  if (load_tri(p.m, t, q) != kTriOk) return false;
  const int j = pix / p.W, i = pix - j * p.W;
  float zz;
  if (!sample_eval(q, i * kSub + p.off, j * kSub + p.off, zz, b)) {
    b[0] = b[1] = b[2] = 0.f;
    return false;
  }
  z = __uint_as_float((unsigned)(key >> 32));
  return true;
}

__global__ __launch_bounds__(kRasterThreads) void raster_resolve_kernel(RasterParams p, int32_t* face, float* depth, float* bary) {
  const long long g = (long long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (g >= (long long)p.H * p.W) return;
  const int pix = (int)g;
  long long t = -1;
  float z = INFINITY, b[3];
  if (!resolve_pixel(p, pix, t, z, b)) { t = -1; z = INFINITY; }
  if (face) face[pix] = (int32_t)t;
  if (depth) depth[pix] = z;
  if (bary) {
    bary[3ll * pix] = b[0];
    bary[3ll * pix + 1] = b[1];
    bary[3ll * pix + 2] = b[2];
  }
}

constexpr int kInterpMaxC = 16;

__global__ __launch_bounds__(kRasterThreads) void raster_interpolate_kernel(const float* attrs, long long V, int C, const int64_t* tris,
                                                                            long long T, const int32_t* face, const float* bary,
                                                                            long long n_pix, float* out) {
  const long long pix = (long long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (pix >= n_pix) return;
  const long long f = face[pix];
  long long vi[3] = {0, 0, 0};
  bool ok = f >= 0 && f < T;
  if (ok) {
    MeshRef m{nullptr, nullptr, tris, V, T};
    ok = tri_indices(m, f, vi);
  }
  const float b0 = bary[3 * pix], b1 = bary[3 * pix + 1], b2 = bary[3 * pix + 2];
  for (int c = 0; c < C; ++c)
    out[pix * C + c] = ok ? (b0 * attrs[vi[0] * C + c] + b1 * attrs[vi[1] * C + c]) + b2 * attrs[vi[2] * C + c] : 0.f;
}

// ---- render_mesh's resolve ----
struct ShadeParams {
  RasterParams r;
  const float* verts;       // (V, 3) world; read with headlight shading only
  const float* colors;      // (V, 3) or null = white
  float f, cx, cy, offf;    // offf: 0 or 0.5
  float cam[3];             // c2w[:, 3]
  int background_kind;      // MF_RASTER_BG_*
  uint8_t bg[3];
  const uint8_t* bg_image;  // (H, W, 3)
  int shading;
  float ambient;
  uint8_t* rgba;
  uint8_t* mask;
  float* depth;
  float* ray_t;
  int32_t* face;
};

__device__ inline uint8_t quantise8(float v) {                      // vis.py / save_image: (uint8) clamp(v 255 + 0.5, 0, 255), truncated
  const float t = v * 255.0f + 0.5f;
  return (uint8_t)(t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0));   // (NaN: 0)
}

__global__ __launch_bounds__(kRasterThreads) void raster_shade_kernel(ShadeParams p) {
  const long long g = (long long)blockIdx.x * kRasterThreads + threadIdx.x;
  if (g >= (long long)p.r.H * p.r.W) return;
  const int pix = (int)g;
  long long t = -1;
  float z = INFINITY, b[3];
  const bool hit = resolve_pixel(p.r, pix, t, z, b);
  uint8_t px[4] = {0, 0, 0, 0};
  float rt = INFINITY;
  if (hit) {
    const int j = pix / p.r.W, i = pix - j * p.r.W;
    // the direction of pixel_ray (mf_rays.hpp) in camera coordinates, at the sample position
    const float dx = (((float)i + p.offf) - p.cx) / p.f;
    const float dy = -((((float)j + p.offf) - p.cy) / p.f);
    rt = z * sqrtf((dx * dx + dy * dy) + 1.f);
    long long vi[3];
    tri_indices(p.r.m, t, vi);                                  // in range: load_tri accepted them
    float shade = 1.f;
    if (p.shading == MF_RASTER_SHADE_HEADLIGHT) {
      float P[3][3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) P[k][a] = p.verts[3 * vi[k] + a];
      const float ux = P[1][0] - P[0][0], uy = P[1][1] - P[0][1], uz = P[1][2] - P[0][2];
      const float vx = P[2][0] - P[0][0], vy = P[2][1] - P[0][1], vz = P[2][2] - P[0][2];
      const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
      float e[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) e[a] = p.cam[a] - ((b[0] * P[0][a] + b[1] * P[1][a]) + b[2] * P[2][a]);
      const float nn = sqrtf((nx * nx + ny * ny) + nz * nz), ee = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
      const float d = nn * ee;
      const float cosv = d > 0.f ? fabsf((nx * e[0] + ny * e[1]) + nz * e[2]) / d : 0.f;
      shade = p.ambient + (1.f - p.ambient) * cosv;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = 1.f;
      if (p.colors) v = (b[0] * p.colors[3 * vi[0] + c] + b[1] * p.colors[3 * vi[1] + c]) + b[2] * p.colors[3 * vi[2] + c];
      if (p.shading == MF_RASTER_SHADE_HEADLIGHT) v = v * shade;
      px[c] = quantise8(v);
    }
    px[3] = 255;
  } else {
    t = -1;
    z = INFINITY;
    if (p.background_kind == MF_RASTER_BG_COLOUR) {
      px[0] = p.bg[0]; px[1] = p.bg[1]; px[2] = p.bg[2];
    } else if (p.background_kind == MF_RASTER_BG_IMAGE) {
      px[0] = p.bg_image[3ll * pix]; px[1] = p.bg_image[3ll * pix + 1]; px[2] = p.bg_image[3ll * pix + 2];
    }
  }
  if (p.rgba) reinterpret_cast<uint32_t*>(p.rgba)[pix] = (uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16 | (uint32_t)px[3] << 24;
  if (p.mask) p.mask[pix] = hit ? 1 : 0;
  if (p.depth) p.depth[pix] = z;
  if (p.ray_t) p.ray_t[pix] = rt;
  if (p.face) p.face[pix] = (int32_t)t;
}

// ---- host side ----
inline int check_view(const char* who, int64_t H, int64_t W) {
  if (H <= 0 || W <= 0) return fail(MF_E_INVALID, "%s: H=%lld W=%lld must both be positive", who, (long long)H, (long long)W);
  if (W > 0x7fffffffLL / H) return fail(MF_E_INVALID, "%s: H=%lld W=%lld: H W must be below 2^31", who, (long long)H, (long long)W);
  return MF_OK;
}

inline int check_mesh(const char* who, int64_t V, int64_t T) {
  if (V < 0 || T < 0 || V >= (1LL << 31) || T >= (1LL << 31))
    return fail(MF_E_INVALID, "%s: V=%lld T=%lld must be in [0, 2^31)", who, (long long)V, (long long)T);
  return MF_OK;
}

inline int check_offset(const char* who, float pixel_offset, int& off) {
  if (pixel_offset == 0.0f) off = 0;
  else if (pixel_offset == 0.5f) off = kSub / 2;
  else return fail(MF_E_INVALID, "%s: pixel_offset=%g must be 0 or 0.5", who, (double)pixel_offset);
  return MF_OK;
}

inline unsigned pixel_blocks(int64_t n) { return (unsigned)((n + kRasterThreads - 1) / kRasterThreads); }

inline int64_t key_bytes(int64_t H, int64_t W) { return H * W * 8; }

inline int fill_raster_params(const char* who, RasterParams& p, const int32_t* screen, const float* inv_z, int64_t V, const int64_t* tris,
                              int64_t T, int64_t H, int64_t W, float pixel_offset, void* scratch) {
  int rc;
  if ((rc = check_view(who, H, W)) != MF_OK || (rc = check_mesh(who, V, T)) != MF_OK || (rc = check_offset(who, pixel_offset, p.off)) != MF_OK)
    return rc;
  if (!scratch) return fail(MF_E_INVALID, "%s: scratch is null", who);
  if (T > 0 && !tris) return fail(MF_E_INVALID, "%s: tris is null", who);
  if (T > 0 && V > 0 && (!screen || !inv_z)) return fail(MF_E_INVALID, "%s: null argument (screen or inv_z)", who);
  p.m = MeshRef{screen, inv_z, tris, (long long)V, (long long)T};
  p.H = (int)H;
  p.W = (int)W;
  p.keys = static_cast<unsigned long long*>(scratch);
  p.dropped = p.keys + H * W;
  return MF_OK;
}

}  // namespace mf

using namespace mf;

extern "C" int32_t mf_project_vertices(const float* verts, int64_t V, const float* c2w_host, float focal, float cx, float cy, float znear,
                                       int32_t* screen, float* inv_z, float* xy, void* stream) {
  if (V < 0 || V >= (1LL << 31)) return fail(MF_E_INVALID, "mf_project_vertices: V=%lld must be in [0, 2^31)", (long long)V);
  if (!c2w_host) return fail(MF_E_INVALID, "mf_project_vertices: c2w_host is null");
  if (!(focal > 0.f)) return fail(MF_E_INVALID, "mf_project_vertices: focal=%g must be positive", (double)focal);
  if (!(znear > 0.f)) return fail(MF_E_INVALID, "mf_project_vertices: znear=%g must be positive", (double)znear);
  if (V == 0) return MF_OK;
  if (!verts || !screen || !inv_z) return fail(MF_E_INVALID, "mf_project_vertices: null argument (verts, screen or inv_z)");
  ProjCam c;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) c.R[a * 3 + b] = c2w_host[a * 4 + b];
    c.t[a] = c2w_host[a * 4 + 3];
  }
  c.f = focal; c.cx = cx; c.cy = cy; c.znear = znear;
  hipLaunchKernelGGL(project_kernel, dim3(pixel_blocks(V)), dim3(kRasterThreads), 0, static_cast<hipStream_t>(stream), verts, (int)V, c,
                     screen, inv_z, xy);
  return check_launch("mf_project_vertices");
}

extern "C" int64_t mf_raster_scratch_bytes(int64_t H, int64_t W) {
  if (check_view("mf_raster_scratch_bytes", H, W) != MF_OK) return MF_E_INVALID;
  return key_bytes(H, W) + 8;
}

extern "C" int32_t mf_rasterize(const int32_t* screen, const float* inv_z, int64_t V, const int64_t* tris, int64_t T, int64_t H, int64_t W,
                                float pixel_offset, void* scratch, void* stream) {
  RasterParams p;
  const int rc = fill_raster_params("mf_rasterize", p, screen, inv_z, V, tris, T, H, W, pixel_offset, scratch);
  if (rc != MF_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(p.keys, 0xff, key_bytes(H, W), st) != hipSuccess || hipMemsetAsync(p.dropped, 0, 8, st) != hipSuccess)
    return fail(MF_E_LAUNCH, "mf_rasterize: cannot clear the key plane");
  if (T == 0) return MF_OK;
  hipLaunchKernelGGL(raster_walk_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, st, p);
  return check_launch("mf_rasterize");
}

extern "C" int32_t mf_raster_resolve(const void* scratch, const int32_t* screen, const float* inv_z, int64_t V, const int64_t* tris, int64_t T,
                                     int64_t H, int64_t W, float pixel_offset, int32_t* face, float* depth, float* bary,
                                     int64_t* dropped_out, void* stream) {
  RasterParams p;
  const int rc = fill_raster_params("mf_raster_resolve", p, screen, inv_z, V, tris, T, H, W, pixel_offset, const_cast<void*>(scratch));
  if (rc != MF_OK) return rc;
  if (!face && !depth && !bary && !dropped_out) return fail(MF_E_INVALID, "mf_raster_resolve: every output is null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dropped_out && hipMemcpyAsync(dropped_out, p.dropped, 8, hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(MF_E_LAUNCH, "mf_raster_resolve: cannot copy the dropped count");
  if (!face && !depth && !bary) return MF_OK;
  hipLaunchKernelGGL(raster_resolve_kernel, dim3(pixel_blocks(H * W)), dim3(kRasterThreads), 0, st, p, face, depth, bary);
  return check_launch("mf_raster_resolve");
}

extern "C" int32_t mf_raster_interpolate(const float* attrs, int64_t V, int32_t C, const int64_t* tris, int64_t T, const int32_t* face,
                                         const float* bary, int64_t n_pix, float* out, void* stream) {
  if (C < 1 || C > kInterpMaxC) return fail(MF_E_INVALID, "mf_raster_interpolate: C=%d must be from 1 to %d", C, kInterpMaxC);
  int rc;
  if ((rc = check_mesh("mf_raster_interpolate", V, T)) != MF_OK) return rc;
  if (n_pix < 0 || n_pix >= (1LL << 31)) return fail(MF_E_INVALID, "mf_raster_interpolate: n_pix=%lld must be in [0, 2^31)", (long long)n_pix);
  if (n_pix == 0) return MF_OK;
  if (!face || !bary || !out) return fail(MF_E_INVALID, "mf_raster_interpolate: null argument (face, bary or out)");
  if (T > 0 && V > 0 && (!attrs || !tris)) return fail(MF_E_INVALID, "mf_raster_interpolate: null argument (attrs or tris)");
  if (V == 0) T = 0;                                            // no vertex: every face is out of range, nothing is read
  hipLaunchKernelGGL(raster_interpolate_kernel, dim3(pixel_blocks(n_pix)), dim3(kRasterThreads), 0, static_cast<hipStream_t>(stream), attrs,
                     (long long)V, (int)C, tris, (long long)T, face, bary, (long long)n_pix, out);
  return check_launch("mf_raster_interpolate");
}

extern "C" int32_t mf_raster_shade(const mf_raster_shade_args* a, void* stream) {
  if (!a) return fail(MF_E_INVALID, "mf_raster_shade: args is null");
  ShadeParams p{};
  const int rc = fill_raster_params("mf_raster_shade", p.r, a->screen, a->inv_z, a->V, a->tris, a->T, a->H, a->W, a->pixel_offset,
                                    const_cast<void*>(a->scratch));
  if (rc != MF_OK) return rc;
  if (!(a->focal > 0.f)) return fail(MF_E_INVALID, "mf_raster_shade: focal=%g must be positive", (double)a->focal);
  if (a->shading != MF_RASTER_SHADE_NONE && a->shading != MF_RASTER_SHADE_HEADLIGHT)
    return fail(MF_E_INVALID, "mf_raster_shade: shading=%d (0: none, 1: headlight)", a->shading);
  if (a->background_kind < MF_RASTER_BG_NONE || a->background_kind > MF_RASTER_BG_IMAGE)
    return fail(MF_E_INVALID, "mf_raster_shade: background_kind=%d (0: none, 1: colour, 2: image)", a->background_kind);
  if (a->background_kind == MF_RASTER_BG_IMAGE && !a->background_image) return fail(MF_E_INVALID, "mf_raster_shade: background_image is null");
  if (a->shading == MF_RASTER_SHADE_HEADLIGHT && a->T > 0 && a->V > 0 && !a->verts)
    return fail(MF_E_INVALID, "mf_raster_shade: headlight shading needs verts");
  if (!a->rgba && !a->mask && !a->depth && !a->ray_t && !a->face) return fail(MF_E_INVALID, "mf_raster_shade: every output is null");
  if (a->rgba && (reinterpret_cast<uintptr_t>(a->rgba) & 3)) return fail(MF_E_INVALID, "mf_raster_shade: rgba must be 4-byte aligned");
  p.verts = a->verts;
  p.colors = a->colors;
  p.f = a->focal; p.cx = a->cx; p.cy = a->cy;
  p.offf = a->pixel_offset;
  for (int k = 0; k < 3; ++k) {
    p.cam[k] = a->c2w[4 * k + 3];
    p.bg[k] = a->background_colour[k];
  }
  p.background_kind = a->background_kind;
  p.bg_image = a->background_image;
  p.shading = a->shading;
  p.ambient = a->ambient;
  p.rgba = a->rgba; p.mask = a->mask; p.depth = a->depth; p.ray_t = a->ray_t; p.face = a->face;
  hipLaunchKernelGGL(raster_shade_kernel, dim3(pixel_blocks(a->H * a->W)), dim3(kRasterThreads), 0, static_cast<hipStream_t>(stream), p);
  return check_launch("mf_raster_shade");
}
