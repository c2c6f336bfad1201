// mf_occupancy.hip -- an occupancy bit grid of a frame's density and the ray marcher through it (include/mocoflow_hip.h):
//   mf_occ_build : raw sigma lattice (query_sigma over the AABB) -> one bit per cell, dilated; optionally the occupied-cell count
//   mf_ray_clip  : per ray, the first and the last occupied cell it steps into -> [t_first, t_last] and a hit flag
// They cull and clip the rays of MoCoFlowTrainer.render (trainer_moco_flow.py:226-268) behind the hull of the projected AABB and
// the corner distances Camera.make_rays gives every ray as near / far (utils/camera.py:134-148), before render_rays samples
// them from near to far (models/rendering.py:239-249).  The reference has no counterpart: its only cull is the hull.
// No atomics: every grid word is written by one lane, the count goes through mf_reduce.hpp; bit-identical from run to run.
#include "mf_host.hpp"
#include "mf_reduce.hpp"

// t_k = tmin + k dt, p = o + d t_k and (p - lo) inv_cell are rounded after every operation, as tests/occupancy_oracle.py
// restates them (the Makefile builds every unit with -ffp-contract=off; the pragma keeps it true for a build that forgets it)
#pragma clang fp contract(off)

namespace mf {

constexpr int kOccThreads = 256;

__device__ __forceinline__ float occ_activate(float s, int act) {
  if (act == MF_ACT_RELU) return s < 0.f ? 0.f : s;                        // NaN stays NaN, as torch.relu leaves it
  return softplus_torch(s);
}

struct OccBuildParams {
  const float* vol;
  int nx, ny, nz;                  // lattice points
  int gx, gy, gz, wz;              // cells, words per (x, y) row
  long long n_words;
  int act, r;
  float tau;
  unsigned* bits;
  double* parts;                   // per-workgroup popcounts, or null
};

// One lane per word = 32 cells of one (i, j) row.  Cell k of the row is set iff a lattice point of [i-r, i+1+r] x [j-r, j+1+r] x
// [k-r, k+1+r] is active: first the row's z-points k0-r .. k0+32+r (at most 37) are or-ed over the x-y window into a 64-bit
// mask, bit m = z-point k0 - r + m; cell k0 + c then is the OR of the mask's bits c .. c + 1 + 2r.
__global__ __launch_bounds__(kOccThreads) void occ_build_kernel(const OccBuildParams p) {
  const long long wi = (long long)blockIdx.x * kOccThreads + threadIdx.x;
  double cnt = 0.0;
  if (wi < p.n_words) {
    const int w = (int)(wi % p.wz);
    const long long row = wi / p.wz;
    const int j = (int)(row % p.gy), i = (int)(row / p.gy);
    const int x0 = i - p.r < 0 ? 0 : i - p.r, x1 = i + 1 + p.r > p.nx - 1 ? p.nx - 1 : i + 1 + p.r;
    const int y0 = j - p.r < 0 ? 0 : j - p.r, y1 = j + 1 + p.r > p.ny - 1 ? p.ny - 1 : j + 1 + p.r;
    const long long k0 = (long long)w * 32;
    const long long zb = k0 - p.r;                                         // z-point of mask bit 0
    const int m0 = zb < 0 ? (int)-zb : 0;
    const int m1 = zb + 33 + 2 * p.r > p.nz - 1 ? (int)(p.nz - 1 - zb) : 33 + 2 * p.r;   // the last mask bit inside the lattice
    unsigned long long mask = 0;
    for (int x = x0; x <= x1; ++x)
      for (int y = y0; y <= y1; ++y) {
        const float* line = p.vol + ((long long)x * p.ny + y) * p.nz + zb;
        for (int m = m0; m <= m1; ++m) {
          const float a = occ_activate(line[m], p.act);
          mask |= (unsigned long long)(!(a <= p.tau)) << m;                // a > tau, or NaN
        }
      }
    unsigned long long cells = 0;
    for (int s = 0; s <= 1 + 2 * p.r; ++s) cells |= mask >> s;
    unsigned word = (unsigned)cells;
    const long long left = p.gz - k0;                                      // cells of the row from this word on: >= 1
    if (left < 32) word &= (1u << left) - 1u;
    p.bits[wi] = word;
    cnt = (double)__popc(word);
  }
  if (p.parts) {
    const double v[1] = {cnt};
    block_sum_d<kOccThreads, 1>(v, p.parts + blockIdx.x);
  }
}

__global__ __launch_bounds__(kOccThreads) void occ_count_finish_kernel(const double* parts, long long n_parts, long long* count) {
  count_finish<kOccThreads>(parts, n_parts, count);
}

struct RayClipParams {
  const float* rays; long long stride, n;
  const unsigned* bits;
  int gx, gy, gz, wz;
  float lo[3], hi[3], inv_cell[3];
  float dt;
  int max_steps;
  float* t_first; float* t_last; unsigned char* hit;
};

__device__ __forceinline__ bool occ_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN and inf

__device__ __forceinline__ int occ_cell(float p, float lo, float inv, int g) {
  float f = floorf((p - lo) * inv);
  f = f >= 0.f ? f : 0.f;                                                  // clamped as a float first: the conversion is defined
  const float top = (float)(g - 1);
  f = f <= top ? f : top;
  const int c = (int)f;
  return c > g - 1 ? g - 1 : c;
}

// One lane per ray.
__global__ __launch_bounds__(kOccThreads) void ray_clip_kernel(const RayClipParams p) {
  const long long i = (long long)blockIdx.x * kOccThreads + threadIdx.x;
  if (i >= p.n) return;
  const float* r = p.rays + i * p.stride;
  const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[3], r[4], r[5]};
  const float nearv = r[6], farv = r[7];
  float t_first = nearv, t_last = farv;
  unsigned char hit = 0;
  bool fin = occ_finite(nearv) && occ_finite(farv);
#pragma unroll
  for (int a = 0; a < 3; ++a) fin = fin && occ_finite(o[a]) && occ_finite(d[a]);
  if (!fin) {
    hit = 1;                                                               // never hidden: such a ray renders NaN, as without a grid
  } else {
    float tmin = nearv, tmax = farv;
    bool miss = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (d[a] != 0.f) {
        const float t1 = (p.lo[a] - o[a]) / d[a], t2 = (p.hi[a] - o[a]) / d[a];
        tmin = fmaxf(tmin, fminf(t1, t2));
        tmax = fminf(tmax, fmaxf(t1, t2));
      } else if (o[a] < p.lo[a] || o[a] > p.hi[a]) {
        miss = true;
      }
    }
    if (!miss && !(tmin > tmax)) {
      int kf = -1, kl = -1;
      bool cut = false;
      for (int k = 0;; ++k) {
        const float t = tmin + (float)k * p.dt;
        if (!(t <= tmax)) break;
        if (k >= p.max_steps) { cut = true; break; }                       // a direction shorter than 1: the rest counts as occupied
        const int cx = occ_cell(o[0] + d[0] * t, p.lo[0], p.inv_cell[0], p.gx);
        const int cy = occ_cell(o[1] + d[1] * t, p.lo[1], p.inv_cell[1], p.gy);
        const int cz = occ_cell(o[2] + d[2] * t, p.lo[2], p.inv_cell[2], p.gz);
        const unsigned word = p.bits[((long long)cx * p.gy + cy) * p.wz + (cz >> 5)];
        if ((word >> (cz & 31)) & 1u) {
          if (kf < 0) kf = k;
          kl = k;
        }
      }
      if (kf >= 0 || cut) {
        hit = 1;
        if (kf >= 0) t_first = fmaxf(nearv, (tmin + (float)kf * p.dt) - p.dt);
        if (!cut) t_last = fminf(farv, (tmin + (float)kl * p.dt) + p.dt);
      }
    }
  }
  p.t_first[i] = t_first;
  p.t_last[i] = t_last;
  p.hit[i] = hit;
}

inline bool occ_shape_ok(long long nx, long long ny, long long nz) {
  const long long lim = 1LL << 31;
  if (nx < 2 || ny < 2 || nz < 2 || nx >= lim || ny >= lim || nz >= lim) return false;
  const long long a = (nx - 1) * (ny - 1);                                 // below 2^62
  return a < lim && a * (nz - 1) < lim;
}

inline long long occ_words(long long nx, long long ny, long long nz) { return (nx - 1) * (ny - 1) * ((nz - 1 + 31) / 32); }

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_occ_build_scratch_bytes(int64_t nx, int64_t ny, int64_t nz) {
  if (!occ_shape_ok(nx, ny, nz))
    return fail(MF_E_INVALID, "mf_occ_build_scratch_bytes: lattice %lld x %lld x %lld (each side >= 2, fewer than 2^31 cells)",
                (long long)nx, (long long)ny, (long long)nz);
  return (occ_words(nx, ny, nz) + kOccThreads - 1) / kOccThreads * (int64_t)sizeof(double);
}

extern "C" int32_t mf_occ_build(const float* sigma, int64_t nx, int64_t ny, int64_t nz, int32_t activation, float tau,
                                int32_t dilate, uint32_t* bits_out, int64_t* count_out, void* scratch, void* stream) {
  if (!occ_shape_ok(nx, ny, nz))
    return fail(MF_E_INVALID, "mf_occ_build: lattice %lld x %lld x %lld (each side >= 2, fewer than 2^31 cells)", (long long)nx,
                (long long)ny, (long long)nz);
  if (activation != MF_ACT_RELU && activation != MF_ACT_SOFTPLUS) return fail(MF_E_INVALID, "mf_occ_build: activation=%d", activation);
  if (dilate < 0 || dilate > 2) return fail(MF_E_INVALID, "mf_occ_build: dilate=%d (0, 1 or 2)", dilate);
  if (tau != tau) return fail(MF_E_INVALID, "mf_occ_build: tau is NaN");
  if (!sigma || !bits_out) return fail(MF_E_INVALID, "mf_occ_build: null sigma or bits_out");
  if (count_out && !scratch) return fail(MF_E_INVALID, "mf_occ_build: count_out needs scratch (mf_occ_build_scratch_bytes)");
  OccBuildParams p{};
  p.vol = sigma;
  p.nx = (int)nx; p.ny = (int)ny; p.nz = (int)nz;
  p.gx = p.nx - 1; p.gy = p.ny - 1; p.gz = p.nz - 1; p.wz = (p.gz + 31) / 32;
  p.n_words = occ_words(nx, ny, nz);
  p.act = activation; p.r = dilate; p.tau = tau;
  p.bits = bits_out;
  p.parts = count_out ? static_cast<double*>(scratch) : nullptr;
  const long long blocks = (p.n_words + kOccThreads - 1) / kOccThreads;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(occ_build_kernel, dim3((unsigned)blocks), dim3(kOccThreads), 0, s, p);
  if (count_out)
    hipLaunchKernelGGL(occ_count_finish_kernel, dim3(1), dim3(kOccThreads), 0, s, p.parts, blocks, reinterpret_cast<long long*>(count_out));
  return check_launch("mf_occ_build");
}

extern "C" int32_t mf_ray_clip(const float* rays, int64_t ray_stride, int64_t n_rays, const uint32_t* bits, int32_t gx, int32_t gy,
                               int32_t gz, const float* lo, const float* hi, const float* inv_cell, float dt, float* t_first,
                               float* t_last, uint8_t* hit, void* stream) {
  if (n_rays < 0 || ray_stride < 8) return fail(MF_E_INVALID, "mf_ray_clip: n_rays=%lld ray_stride=%lld (>= 8)", (long long)n_rays, (long long)ray_stride);
  if (gx < 1 || gy < 1 || gz < 1 || (long long)gx * gy >= (1LL << 31) || (long long)gx * gy * gz >= (1LL << 31))
    return fail(MF_E_INVALID, "mf_ray_clip: grid of %d x %d x %d cells (each side >= 1, fewer than 2^31 cells)", gx, gy, gz);
  if (!lo || !hi || !inv_cell) return fail(MF_E_INVALID, "mf_ray_clip: null lo, hi or inv_cell");
  double diag2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    if (!(lo[a] < hi[a]) || !(fabsf(lo[a]) <= 3.402823466e+38f) || !(fabsf(hi[a]) <= 3.402823466e+38f))
      return fail(MF_E_INVALID, "mf_ray_clip: empty or inverted box on axis %d: lo=%g hi=%g", a, lo[a], hi[a]);
    if (!(inv_cell[a] > 0.f) || !(inv_cell[a] <= 3.402823466e+38f)) return fail(MF_E_INVALID, "mf_ray_clip: inv_cell[%d]=%g", a, inv_cell[a]);
    diag2 += ((double)hi[a] - (double)lo[a]) * ((double)hi[a] - (double)lo[a]);
  }
  if (!(dt > 0.f) || !(dt <= 3.402823466e+38f)) return fail(MF_E_INVALID, "mf_ray_clip: dt=%g must be positive", dt);
  const double steps = floor(sqrt(diag2) / (double)dt) + 2.0;
  if (!(steps <= 65536.0)) return fail(MF_E_INVALID, "mf_ray_clip: dt=%g takes %.0f steps through the box, more than 65536", dt, steps);
  if (n_rays == 0) return MF_OK;
  if (!rays || !bits) return fail(MF_E_INVALID, "mf_ray_clip: null rays or bits");
  if (!t_first || !t_last || !hit) return fail(MF_E_INVALID, "mf_ray_clip: null output (t_first, t_last or hit)");
  if ((n_rays + kOccThreads - 1) / kOccThreads >= (1LL << 31)) return fail(MF_E_INVALID, "mf_ray_clip: n_rays=%lld", (long long)n_rays);
  RayClipParams p{};
  p.rays = rays; p.stride = ray_stride; p.n = n_rays;
  p.bits = bits;
  p.gx = gx; p.gy = gy; p.gz = gz; p.wz = (gz + 31) / 32;
  for (int a = 0; a < 3; ++a) { p.lo[a] = lo[a]; p.hi[a] = hi[a]; p.inv_cell[a] = inv_cell[a]; }
  p.dt = dt;
  p.max_steps = (int)steps;
  p.t_first = t_first; p.t_last = t_last; p.hit = hit;
  hipLaunchKernelGGL(ray_clip_kernel, dim3((unsigned)((n_rays + kOccThreads - 1) / kOccThreads)), dim3(kOccThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  return check_launch("mf_ray_clip");
}
