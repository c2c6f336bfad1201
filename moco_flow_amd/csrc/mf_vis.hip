// mf_vis.hip -- the picture path behind decode_results (trainer_moco_flow.py:475-482) and visualize_frame / visualize_video
// (trainer_moco_flow.py:590-661):
//   mf_depth_range     min / max of nan_to_num(depth)                               utils/vis_utils.py:34-38
//   mf_depth_colormap  normalise, truncate to an 8-bit index, colour table, ToTensor utils/vis_utils.py:39-43
//   mf_frame_sheet     [gt | pred | depth | novel pred | novel depth] side by side, as save_image's bytes and / or the
//                      float planes, in ONE launch from the rendered rows          trainer_moco_flow.py:609-623, 644-659
// The index arithmetic is the reference's own, operation for operation in fp32 with one rounding each (the build has no
// fast-math and -ffp-contract=off; the subtraction, division and multiplication are spelled __f*_rn all the same):
//   v = nan_to_num(d)   den = (ma - mi) + 1e-8   x = (v - mi) / den   i = (uint8) trunc(255 x)
// ONE DEVIATION: where numpy's astype(np.uint8) is undefined -- 255 x outside [0, 256) or NaN, which needs a caller-given
// range narrower than the data or infinities in it -- the index is clamped to 0 .. 255 (NaN: 0).
// The colour table is the caller's 768 bytes; moco_flow_amd/vis.py builds Jet (OPENCV RESTATED, see the header).
#include <cfloat>

#include "mf_host.hpp"

namespace mf {

__device__ inline float nan_to_num(float d, float nan_value) {   // numpy's defaults for the infinities
  if (d != d) return nan_value;
  if (d > FLT_MAX) return FLT_MAX;
  if (d < -FLT_MAX) return -FLT_MAX;
  return d;
}

__device__ inline float depth_den(float mi, float ma) { return __fadd_rn(__fsub_rn(ma, mi), 1e-8f); }

__device__ inline int depth_index(float d, float mi, float den, float nan_value) {
  const float x = __fdiv_rn(__fsub_rn(nan_to_num(d, nan_value), mi), den);
  const float t = __fmul_rn(255.0f, x);
  return t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0);              // trunc inside [0, 256); the clamp (and NaN -> 0) outside
}

// ---- range: per-workgroup (min, max) partials in `scratch`, one finishing workgroup; min and max do not depend on the order ----
constexpr int kRangeThreads = 256, kRangePerThread = 4, kRangeMaxBlocks = 512;
constexpr int kRangeFinishThreads = 256;

__device__ inline void wave_minmax(float& lo, float& hi) {
  for (int m = 1; m < 64; m <<= 1) {
    lo = fminf(lo, __shfl_xor(lo, m, 64));
    hi = fmaxf(hi, __shfl_xor(hi, m, 64));
  }
}

// every thread of the workgroup calls it; thread 0 stores the workgroup's (min, max) at out2
template <int THREADS>
__device__ inline void block_minmax_store(float lo, float hi, float* out2) {
  __shared__ float red[THREADS / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_minmax(lo, hi);
  if (lane == 0) { red[wave][0] = lo; red[wave][1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < THREADS / 64; ++w) { lo = fminf(lo, red[w][0]); hi = fmaxf(hi, red[w][1]); }
    out2[0] = lo;
    out2[1] = hi;
  }
}

// VEC: depth is 16-byte aligned; the n / 4 float4s are strided over the grid, the n % 4 last elements go to workgroup 0
template <bool VEC>
__global__ __launch_bounds__(kRangeThreads) void depth_range_kernel(const float* depth, long long n, float nan_value, float* parts) {
  float lo = INFINITY, hi = -INFINITY;                             // identities: nan_to_num leaves nothing beyond +-FLT_MAX
  const long long nth = (long long)gridDim.x * kRangeThreads, t0 = (long long)blockIdx.x * kRangeThreads + threadIdx.x;
  if (VEC) {
    const float4* d4 = reinterpret_cast<const float4*>(depth);
    const long long n4 = n >> 2;
    for (long long i = t0; i < n4; i += nth) {
      const float4 d = d4[i];
      const float a = nan_to_num(d.x, nan_value), b = nan_to_num(d.y, nan_value), c = nan_to_num(d.z, nan_value), e = nan_to_num(d.w, nan_value);
      lo = fminf(fminf(lo, a), fminf(b, fminf(c, e)));
      hi = fmaxf(fmaxf(hi, a), fmaxf(b, fmaxf(c, e)));
    }
    if (t0 < (n & 3)) {
      const float a = nan_to_num(depth[(n4 << 2) + t0], nan_value);
      lo = fminf(lo, a);
      hi = fmaxf(hi, a);
    }
  } else {
    for (long long i = t0; i < n; i += nth) {
      const float a = nan_to_num(depth[i], nan_value);
      lo = fminf(lo, a);
      hi = fmaxf(hi, a);
    }
  }
  block_minmax_store<kRangeThreads>(lo, hi, parts + 2 * (long long)blockIdx.x);
}

__global__ __launch_bounds__(kRangeFinishThreads) void depth_range_finish_kernel(const float* parts, int n_parts, float* out2) {
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < n_parts; i += kRangeFinishThreads) {
    lo = fminf(lo, parts[2 * i]);
    hi = fmaxf(hi, parts[2 * i + 1]);
  }
  block_minmax_store<kRangeFinishThreads>(lo, hi, out2);
}

inline long long range_blocks(long long n) { return capped_blocks(n, (long long)kRangeThreads * kRangePerThread, kRangeMaxBlocks); }

// ---- the colour table in LDS: the bytes and their ToTensor values b / 255 (one fp32 division each) ----
struct LutLds {
  float f[768];
  uint8_t b[768];
};

__device__ inline void stage_lut(const uint8_t* lut, LutLds& s, int threads) {
  for (int j = threadIdx.x; j < 768; j += threads) {
    const uint8_t b = lut[j];
    s.b[j] = b;
    s.f[j] = __fdiv_rn((float)b, 255.0f);
  }
}

// ---- colour map: a thread owns four consecutive pixels; VEC: n % 4 == 0 and both pointers 16-byte aligned ----
constexpr int kVisThreads = 256, kVisPerThread = 4;

template <bool VEC>
__global__ __launch_bounds__(kVisThreads) void depth_colormap_kernel(const float* depth, long long n, const float* range2, float nan_value,
                                                                    const uint8_t* lut, float* out) {
  __shared__ LutLds s;
  stage_lut(lut, s, kVisThreads);
  __syncthreads();
  const float mi = range2[0], den = depth_den(mi, range2[1]);
  const long long p0 = ((long long)blockIdx.x * kVisThreads + threadIdx.x) * kVisPerThread;
  if (p0 >= n) return;
  if (VEC) {
    const float4 d = *reinterpret_cast<const float4*>(depth + p0);
    const int i0 = 3 * depth_index(d.x, mi, den, nan_value), i1 = 3 * depth_index(d.y, mi, den, nan_value),
              i2 = 3 * depth_index(d.z, mi, den, nan_value), i3 = 3 * depth_index(d.w, mi, den, nan_value);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float4*>(out + c * n + p0) = make_float4(s.f[i0 + c], s.f[i1 + c], s.f[i2 + c], s.f[i3 + c]);
  } else {
    const int cnt = n - p0 < kVisPerThread ? (int)(n - p0) : kVisPerThread;
    for (int j = 0; j < cnt; ++j) {
      const int i = 3 * depth_index(depth[p0 + j], mi, den, nan_value);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c * n + p0 + j] = s.f[i + c];
    }
  }
}

// ---- frame sheet: a thread owns four consecutive pixels of the (H, n_panels W) sheet, row-major ----
constexpr int kSheetMaxPanels = 8;

struct SheetParams {
  const float* rows[kSheetMaxPanels];
  int32_t kind[kSheetMaxPanels];
  float nan_value[kSheetMaxPanels];
  const float* range2s;
  const uint8_t* lut;
  uint8_t* out_u8;
  float* out_planar;
  int32_t W, n_panels, n_out;        // n_out = H n_panels W sheet pixels, 3 n_out < 2^31
  int32_t any_depth, vec_u8, vec_planar;
};

__device__ inline uint8_t quantise(float v) {                       // save_image: v.mul(255).add_(0.5).clamp_(0, 255).to(uint8)
  const float t = __fadd_rn(__fmul_rn(v, 255.0f), 0.5f);
  return (uint8_t)(t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0));   // (NaN: 0)
}

__global__ __launch_bounds__(kVisThreads) void frame_sheet_kernel(SheetParams p) {
  __shared__ LutLds s;
  __shared__ const float* s_rows[kSheetMaxPanels];
  __shared__ int s_kind[kSheetMaxPanels];
  __shared__ float s_nan[kSheetMaxPanels], s_mi[kSheetMaxPanels], s_den[kSheetMaxPanels];
  const int tid = threadIdx.x;
  if (p.any_depth) stage_lut(p.lut, s, kVisThreads);
  if (tid < p.n_panels) {
    s_rows[tid] = p.rows[tid];
    s_kind[tid] = p.kind[tid];
    s_nan[tid] = p.nan_value[tid];
    if (p.kind[tid] == 1) {
      const float mi = p.range2s[2 * tid];
      s_mi[tid] = mi;
      s_den[tid] = depth_den(mi, p.range2s[2 * tid + 1]);
    }
  }
  __syncthreads();
  const int q0 = (blockIdx.x * kVisThreads + tid) * kVisPerThread;
  if (q0 >= p.n_out) return;
  const int cnt = p.n_out - q0 < kVisPerThread ? p.n_out - q0 : kVisPerThread;
  const int KW = p.n_panels * p.W;
  float v[kVisPerThread][3];
  uint8_t u[kVisPerThread][3];
#pragma unroll
  for (int j = 0; j < kVisPerThread; ++j) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[j][c] = 0.f; u[j][c] = 0; }
    if (j >= cnt) continue;
    const int q = q0 + j, y = q / KW, xs = q - y * KW, k = xs / p.W, px = y * p.W + (xs - k * p.W);
    const float* rows = s_rows[k];
    if (s_kind[k] == 1) {
      const int i = 3 * depth_index(rows[px], s_mi[k], s_den[k], s_nan[k]);
#pragma unroll
      for (int c = 0; c < 3; ++c) { v[j][c] = s.f[i + c]; u[j][c] = s.b[i + c]; }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) { v[j][c] = rows[3 * px + c]; u[j][c] = quantise(v[j][c]); }
    }
  }
  if (p.out_u8) {
    if (cnt == kVisPerThread && p.vec_u8) {
      uint32_t w[3];
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) { const int e = 4 * m + b; x |= (uint32_t)u[e / 3][e % 3] << (8 * b); }
        w[m] = x;
      }
      uint32_t* o = reinterpret_cast<uint32_t*>(p.out_u8 + 3 * q0);
      o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
    } else {
      for (int j = 0; j < cnt; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) p.out_u8[3 * (q0 + j) + c] = u[j][c];
    }
  }
  if (p.out_planar) {
    if (cnt == kVisPerThread && p.vec_planar) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(p.out_planar + c * p.n_out + q0) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
    } else {
      for (int j = 0; j < cnt; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) p.out_planar[c * p.n_out + q0 + j] = v[j][c];
    }
  }
}

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_depth_range_scratch_bytes(int64_t n) {
  if (n < 0) return fail(MF_E_INVALID, "mf_depth_range_scratch_bytes: negative n=%lld", (long long)n);
  return range_blocks(n) * 2 * (int64_t)sizeof(float);
}

extern "C" int32_t mf_depth_range(const float* depth, int64_t n, float nan_value, float* out2, void* scratch, void* stream) {
  if (n < 0) return fail(MF_E_INVALID, "mf_depth_range: negative n=%lld", (long long)n);
  if (!out2) return fail(MF_E_INVALID, "mf_depth_range: out2 is null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (hipMemsetAsync(out2, 0, 2 * sizeof(float), st) != hipSuccess) return fail(MF_E_LAUNCH, "mf_depth_range: cannot clear out2");
    return MF_OK;
  }
  if (!depth || !scratch) return fail(MF_E_INVALID, "mf_depth_range: null argument (depth or scratch)");
  const long long blocks = range_blocks(n);
  float* parts = static_cast<float*>(scratch);
  if (is_aligned(depth, 16))
    hipLaunchKernelGGL(depth_range_kernel<true>, dim3((unsigned)blocks), dim3(kRangeThreads), 0, st, depth, (long long)n, nan_value, parts);
  else
    hipLaunchKernelGGL(depth_range_kernel<false>, dim3((unsigned)blocks), dim3(kRangeThreads), 0, st, depth, (long long)n, nan_value, parts);
  hipLaunchKernelGGL(depth_range_finish_kernel, dim3(1), dim3(kRangeFinishThreads), 0, st, parts, (int)blocks, out2);
  return check_launch("mf_depth_range");
}

extern "C" int32_t mf_depth_colormap(const float* depth, int64_t n, const float* range2, float nan_value, const uint8_t* lut,
                                     float* out_planar, void* stream) {
  if (n < 0) return fail(MF_E_INVALID, "mf_depth_colormap: negative n=%lld", (long long)n);
  if (n == 0) return MF_OK;
  if (!depth || !range2 || !lut || !out_planar) return fail(MF_E_INVALID, "mf_depth_colormap: null argument (depth, range2, lut or out_planar)");
  const long long per = (long long)kVisThreads * kVisPerThread;
  const long long blocks = (n + per - 1) / per;
  if (blocks > 0x7fffffffLL) return fail(MF_E_INVALID, "mf_depth_colormap: n=%lld needs more than 2^31 - 1 workgroups", (long long)n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n % 4 == 0 && is_aligned(depth, 16) && is_aligned(out_planar, 16))
    hipLaunchKernelGGL(depth_colormap_kernel<true>, dim3((unsigned)blocks), dim3(kVisThreads), 0, st, depth, (long long)n, range2, nan_value, lut, out_planar);
  else
    hipLaunchKernelGGL(depth_colormap_kernel<false>, dim3((unsigned)blocks), dim3(kVisThreads), 0, st, depth, (long long)n, range2, nan_value, lut, out_planar);
  return check_launch("mf_depth_colormap");
}

extern "C" int32_t mf_frame_sheet(const mf_sheet_panel* panels, int32_t n_panels, int64_t H, int64_t W, const float* range2s,
                                  const uint8_t* lut, uint8_t* out_u8, float* out_planar, void* stream) {
  if (n_panels < 1 || n_panels > kSheetMaxPanels)
    return fail(MF_E_INVALID, "mf_frame_sheet: n_panels=%d must be from 1 to %d", n_panels, kSheetMaxPanels);
  if (H < 0 || W < 0) return fail(MF_E_INVALID, "mf_frame_sheet: negative size (H=%lld W=%lld)", (long long)H, (long long)W);
  if (!panels) return fail(MF_E_INVALID, "mf_frame_sheet: panels is null");
  if (!out_u8 && !out_planar) return fail(MF_E_INVALID, "mf_frame_sheet: out_u8 and out_planar are both null");
  // 32-bit indexing: H W n_panels 3 < 2^31, checked without overflow
  const long long cap = 0x7fffffffLL / (3LL * n_panels);
  if (H != 0 && W > cap / H)
    return fail(MF_E_INVALID, "mf_frame_sheet: H=%lld W=%lld n_panels=%d: the sheet must hold fewer than 2^31 values (32-bit indexing)",
                (long long)H, (long long)W, n_panels);
  SheetParams p{};
  for (int k = 0; k < n_panels; ++k) {
    if (panels[k].kind != 0 && panels[k].kind != 1) return fail(MF_E_INVALID, "mf_frame_sheet: panel %d has kind=%d (0: rgb rows, 1: depth plane)", k, panels[k].kind);
    if (panels[k].kind == 1) p.any_depth = 1;
  }
  if (p.any_depth && (!range2s || !lut)) return fail(MF_E_INVALID, "mf_frame_sheet: a depth panel needs range2s and lut");
  if (H == 0 || W == 0) return MF_OK;
  for (int k = 0; k < n_panels; ++k) {
    if (!panels[k].rows) return fail(MF_E_INVALID, "mf_frame_sheet: panel %d has null rows", k);
    p.rows[k] = panels[k].rows;
    p.kind[k] = panels[k].kind;
    p.nan_value[k] = panels[k].nan_value;
  }
  p.range2s = range2s;
  p.lut = lut;
  p.out_u8 = out_u8;
  p.out_planar = out_planar;
  p.W = (int32_t)W;
  p.n_panels = n_panels;
  p.n_out = (int32_t)(H * W * n_panels);
  p.vec_u8 = out_u8 && is_aligned(out_u8, 4);
  p.vec_planar = out_planar && p.n_out % 4 == 0 && is_aligned(out_planar, 16);
  const int per = kVisThreads * kVisPerThread;
  const unsigned blocks = (unsigned)((p.n_out + (long long)per - 1) / per);
  hipLaunchKernelGGL(frame_sheet_kernel, dim3(blocks), dim3(kVisThreads), 0, static_cast<hipStream_t>(stream), p);
  return check_launch("mf_frame_sheet");
}
