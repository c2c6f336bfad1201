// mf_metrics.hip -- the validation metrics of val_step (trainer_moco_flow.py:453-473), models/metrics.py:4-22:
//   mf_ssim   kornia 0.6.5's kornia.metrics.ssim.ssim(img1, img2, window_size, max_val, eps) -- KORNIA RESTATED: kornia is
//             not available to this project, the published algorithm is restated here (as oracle/kornia_restated.py does
//             for the quaternion functions) and is unpinned against kornia itself -- plus the squared error of the same
//             frame pair, in ONE launch over strided images: no permute copy, no padded copy, no intermediate planes.
//   mf_sqerr  sum and count behind mse / psnr, with the optional per-element or per-row mask.
// Both reduce in the fixed order of mf_reduce.hpp (per-workgroup float64 partials in `scratch`, one finishing workgroup): two
// runs are bit-identical, no atomics.
#include <cmath>

#include "mf_host.hpp"
#include "mf_reduce.hpp"

namespace mf {

// ---- the finishing workgroup of both reductions: (n_parts, 2) float64 partials -> out[2] ----
constexpr int kFinishThreads = 256;

__global__ __launch_bounds__(kFinishThreads) void metrics_finish_kernel(const double* parts, long long n_parts, double* out) {
  gather_sum_d<kFinishThreads, 2>(parts, n_parts, out);
}

// ---- SSIM ----
// One workgroup of 256 threads owns a kSsimTileH x kSsimTileW output tile of one (b, c) plane.
//   stage   the tile plus its halo of R = ws / 2 pixels, both images, fp32, reflected indices resolved here
//   rows    the five horizontal windowed sums (a, b, a^2, b^2, a b) of every staged row at the tile's 32 columns
//   cols    the vertical windowed sums of those at the tile's 16 rows, the SSIM formula, the map, the two partials
// The moments are accumulated as the formula is written, in FLOAT64 (products of two fp32 values are exact there), and the
// map is rounded to fp32 once.  Where a frame is flat (background, saturated regions) sigma = f(a^2) - f(a)^2 cancels near 1,
// and a 1e-7 rounding of an fp32 sum stands against C2 = 9e-4 in the denominator: the fp32 arithmetic is 2e-4 .. 9e-4 off
// on the map there.  Centring the fp32 moments on the tile's centre pixel was tried first (emulated on the CPU): it removes
// that error only where the tile is flat AT the centre's value, and missed the mean's bar (2 x the fp32 reference's own
// error) on tiles that mix flat and textured regions.  The vector fp64 rate is half the fp32 one on this chip and the kernel
// is launch-bound at frame sizes (7 MB per 540 x 540 x 3 pair).
// LDS banks: a half-wave reads 32 consecutive floats of one row in the row pass (sA[y][x + j], ds_read_b32: 32 banks per
// 32-lane half) and 32 consecutive doubles of one row in the column pass (sh[k][y + j][x], ds_read_b64: one 256-byte bank
// row per half): conflict-free whatever the row stride.
constexpr int kSsimTileH = 16, kSsimTileW = 32, kSsimThreads = 256;
constexpr int kSsimMaxR = 5;
constexpr int kSsimStageH = kSsimTileH + 2 * kSsimMaxR, kSsimStageW = kSsimTileW + 2 * kSsimMaxR;

struct SsimParams {
  const float* a; const float* b;
  long long sa[4], sb[4];            // element strides (B, C, H, W)
  long long C, H, W;
  long long tiles_x, tiles_y;        // tiles per plane
  double w[2 * kSsimMaxR + 1];
  double c1, c2, eps;
  float* map;                        // (B, C, H, W) contiguous, or null
  double* parts;                     // (workgroups, 2)
};

__device__ inline long long reflect(long long i, long long n) {   // F.pad(mode='reflect'): -1 -> 1, n -> n - 2
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);     // (rows / columns beyond the halo of the last valid output: unused, kept in bounds)
}

template <int R>
__global__ __launch_bounds__(kSsimThreads) void ssim_kernel(SsimParams p) {
  constexpr int WS = 2 * R + 1, SH = kSsimTileH + 2 * R, SW = kSsimTileW + 2 * R;
  __shared__ float sA[kSsimStageH][kSsimStageW], sB[kSsimStageH][kSsimStageW];
  __shared__ double sh[5][kSsimStageH][kSsimTileW];
  const int tid = threadIdx.x;
  long long t = blockIdx.x;
  const long long tx = t % p.tiles_x; t /= p.tiles_x;
  const long long ty = t % p.tiles_y; t /= p.tiles_y;
  const long long c = t % p.C, b = t / p.C;
  const long long x0 = tx * kSsimTileW, y0 = ty * kSsimTileH;
  const float* pa = p.a + b * p.sa[0] + c * p.sa[1];
  const float* pb = p.b + b * p.sb[0] + c * p.sb[1];

  for (int i = tid; i < SH * SW; i += kSsimThreads) {
    const int ly = i / SW, lx = i % SW;
    const long long gy = reflect(y0 - R + ly, p.H), gx = reflect(x0 - R + lx, p.W);
    sA[ly][lx] = pa[gy * p.sa[2] + gx * p.sa[3]];
    sB[ly][lx] = pb[gy * p.sb[2] + gx * p.sb[3]];
  }
  __syncthreads();

  for (int i = tid; i < SH * kSsimTileW; i += kSsimThreads) {
    const int ly = i / kSsimTileW, ox = i % kSsimTileW;
    double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
#pragma unroll
    for (int j = 0; j < WS; ++j) {
      const double w = p.w[j], va = (double)sA[ly][ox + j], vb = (double)sB[ly][ox + j];
      ma += w * va; mb += w * vb;
      maa += w * (va * va); mbb += w * (vb * vb); mab += w * (va * vb);
    }
    sh[0][ly][ox] = ma; sh[1][ly][ox] = mb; sh[2][ly][ox] = maa; sh[3][ly][ox] = mbb; sh[4][ly][ox] = mab;
  }
  __syncthreads();

  double ssim_sum = 0.0, sq_sum = 0.0;
  const int ox = tid % kSsimTileW;
#pragma unroll
  for (int oy = tid / kSsimTileW; oy < kSsimTileH; oy += kSsimThreads / kSsimTileW) {
    const long long gy = y0 + oy, gx = x0 + ox;
    if (gy >= p.H || gx >= p.W) continue;
    double m[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < WS; ++j) s += p.w[j] * sh[k][oy + j][ox];
      m[k] = s;
    }
    const double mu1 = m[0], mu2 = m[1];
    const double s1 = m[2] - mu1 * mu1, s2 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
    const double num = (2.0 * (mu1 * mu2) + p.c1) * (2.0 * s12 + p.c2);
    const double den = (mu1 * mu1 + mu2 * mu2 + p.c1) * (s1 + s2 + p.c2);
    const float v = (float)(num / (den + p.eps));
    if (p.map) p.map[((b * p.C + c) * p.H + gy) * p.W + gx] = v;
    ssim_sum += (double)v;
    const double d = (double)sA[oy + R][ox + R] - (double)sB[oy + R][ox + R];
    sq_sum += d * d;
  }
  const double sums[2] = {ssim_sum, sq_sum};
  block_sum_d<kSsimThreads, 2>(sums, p.parts + 2 * (long long)blockIdx.x);
}

// ---- squared error ----
constexpr int kSqerrThreads = 256, kSqerrPerThread = 8, kSqerrMaxBlocks = 1024;

__global__ __launch_bounds__(kSqerrThreads) void sqerr_kernel(const float* a, const float* b, long long n, const uint8_t* mask,
                                                             long long row_len, double* parts) {
  double sq = 0.0, cnt = 0.0;
  const long long nth = (long long)gridDim.x * kSqerrThreads;
  for (long long i = (long long)blockIdx.x * kSqerrThreads + threadIdx.x; i < n; i += nth) {
    const bool m = !mask || mask[row_len == 1 ? i : i / row_len] != 0;
    const double d = (double)a[i] - (double)b[i];
    sq += m ? d * d : 0.0;
    cnt += m ? 1.0 : 0.0;
  }
  const double sums[2] = {sq, cnt};
  block_sum_d<kSqerrThreads, 2>(sums, parts + 2 * (long long)blockIdx.x);
}

inline long long ssim_workgroups(long long B, long long C, long long H, long long W) {
  if (B == 0 || C == 0 || H == 0 || W == 0) return 0;
  const long long tx = (W + kSsimTileW - 1) / kSsimTileW, ty = (H + kSsimTileH - 1) / kSsimTileH;
  // B C tiles <= 2^31 - 1, checked without overflow
  const long long cap = 0x7fffffffLL;
  if (tx > cap / ty) return -1;
  long long n = tx * ty;
  if (C > cap / n) return -1;
  n *= C;
  if (B > cap / n) return -1;
  return n * B;
}

inline long long sqerr_blocks(long long n) { return capped_blocks(n, (long long)kSqerrThreads * kSqerrPerThread, kSqerrMaxBlocks); }

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_ssim_scratch_bytes(int64_t B, int64_t C, int64_t H, int64_t W) {
  if (B < 0 || C < 0 || H < 0 || W < 0) return fail(MF_E_INVALID, "mf_ssim_scratch_bytes: negative size (B=%lld C=%lld H=%lld W=%lld)",
                                                   (long long)B, (long long)C, (long long)H, (long long)W);
  const long long wg = ssim_workgroups(B, C, H, W);
  if (wg < 0) return fail(MF_E_INVALID, "mf_ssim_scratch_bytes: B C H W needs more than 2^31 - 1 tiles");
  return wg * 2 * (int64_t)sizeof(double);
}

extern "C" int32_t mf_ssim(const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int64_t B, int64_t C,
                           int64_t H, int64_t W, int32_t window_size, float max_val, float eps, float* map_out, double* sums,
                           void* scratch, void* stream) {
  if (B < 0 || C < 0 || H < 0 || W < 0) return fail(MF_E_INVALID, "mf_ssim: negative size (B=%lld C=%lld H=%lld W=%lld)",
                                                   (long long)B, (long long)C, (long long)H, (long long)W);
  if (window_size < 3 || window_size > 2 * kSsimMaxR + 1 || window_size % 2 == 0)
    return fail(MF_E_INVALID, "mf_ssim: window_size=%d must be odd, from 3 to %d", window_size, 2 * kSsimMaxR + 1);
  if (!sums) return fail(MF_E_INVALID, "mf_ssim: sums is null");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long wg = ssim_workgroups(B, C, H, W);
  if (wg == 0) {
    if (hipMemsetAsync(sums, 0, 2 * sizeof(double), st) != hipSuccess) return fail(MF_E_LAUNCH, "mf_ssim: cannot clear sums");
    return MF_OK;
  }
  const int R = window_size / 2;
  if (R >= (H < W ? H : W))
    return fail(MF_E_INVALID, "mf_ssim: window_size=%d reflects by %d pixels, H=%lld W=%lld must both be larger", window_size, R,
                (long long)H, (long long)W);
  if (wg < 0) return fail(MF_E_INVALID, "mf_ssim: B C H W needs more than 2^31 - 1 tiles");
  if (!a || !b || !a_strides || !b_strides || !scratch) return fail(MF_E_INVALID, "mf_ssim: null argument (a, b, a_strides, b_strides or scratch)");

  SsimParams p{};
  p.a = a; p.b = b;
  for (int k = 0; k < 4; ++k) { p.sa[k] = a_strides[k]; p.sb[k] = b_strides[k]; }
  p.C = C; p.H = H; p.W = W;
  p.tiles_x = (W + kSsimTileW - 1) / kSsimTileW;
  p.tiles_y = (H + kSsimTileH - 1) / kSsimTileH;
  // kornia's get_gaussian_kernel1d(ws, 1.5), in float64
  double g[2 * kSsimMaxR + 1], gs = 0.0;
  for (int i = 0; i < window_size; ++i) { const double x = i - R; g[i] = std::exp(-(x * x) / (2.0 * 1.5 * 1.5)); gs += g[i]; }
  for (int i = 0; i < window_size; ++i) p.w[i] = g[i] / gs;
  p.c1 = (0.01 * (double)max_val) * (0.01 * (double)max_val);
  p.c2 = (0.03 * (double)max_val) * (0.03 * (double)max_val);
  p.eps = eps;
  p.map = map_out;
  p.parts = static_cast<double*>(scratch);
  void (*kern)(SsimParams) = R == 1 ? ssim_kernel<1> : R == 2 ? ssim_kernel<2> : R == 3 ? ssim_kernel<3> : R == 4 ? ssim_kernel<4> : ssim_kernel<5>;
  hipLaunchKernelGGL(kern, dim3((unsigned)wg), dim3(kSsimThreads), 0, st, p);
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, p.parts, wg, sums);
  return check_launch("mf_ssim");
}

extern "C" int64_t mf_sqerr_scratch_bytes(int64_t n) {
  if (n < 0) return fail(MF_E_INVALID, "mf_sqerr_scratch_bytes: negative n=%lld", (long long)n);
  return sqerr_blocks(n) * 2 * (int64_t)sizeof(double);
}

extern "C" int32_t mf_sqerr(const float* a, const float* b, int64_t n, const uint8_t* mask, int64_t row_len, double* out2,
                            void* scratch, void* stream) {
  if (n < 0) return fail(MF_E_INVALID, "mf_sqerr: negative n=%lld", (long long)n);
  if (!out2) return fail(MF_E_INVALID, "mf_sqerr: out2 is null");
  if (mask && (row_len < 1 || n % row_len != 0))
    return fail(MF_E_INVALID, "mf_sqerr: row_len=%lld must be >= 1 and divide n=%lld", (long long)row_len, (long long)n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (hipMemsetAsync(out2, 0, 2 * sizeof(double), st) != hipSuccess) return fail(MF_E_LAUNCH, "mf_sqerr: cannot clear out2");
    return MF_OK;
  }
  if (!a || !b || !scratch) return fail(MF_E_INVALID, "mf_sqerr: null argument (a, b or scratch)");
  const long long blocks = sqerr_blocks(n);
  double* parts = static_cast<double*>(scratch);
  hipLaunchKernelGGL(sqerr_kernel, dim3((unsigned)blocks), dim3(kSqerrThreads), 0, st, a, b, (long long)n, mask, mask ? (long long)row_len : 1LL, parts);
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, parts, blocks, out2);
  return check_launch("mf_sqerr");
}
