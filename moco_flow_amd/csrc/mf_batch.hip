// mf_batch.hip -- the ray batch of a training step, built on the device from the frame's constants (include/mocoflow_hip.h):
//   mf_mask_compact : val_inds = torch.nonzero(rays_msk).squeeze(1)          trainer/trainer_moco_flow.py:414
//   mf_ray_batch    : sel_inds = val_inds[perm[:N_rand]]; rays[sel], rgbs[sel], background[sel]             :415-416
//                     of rays = Camera.make_rays (datasets/moco_flow_dataset.py:196), rgbs = the image composited over
//                     the background from its alpha channel (:169-175), background (:176), and the chain_global column
//                     (_shared_step, trainer_moco_flow.py:308-312) -- none of those tables exists here.
// No atomics anywhere: the compaction keeps the pixel order and is bit-identical from run to run.
#include "mf_host.hpp"
#include "mf_pixels.hpp"   // the 8-bit pixel arithmetic (and the no-FMA pragma), shared with mf_frames.hip
#include "mf_rays.hpp"
#include "mf_scan.hpp"

namespace mf {

constexpr int kCompactThreads = 256;                                     // 4 waves
constexpr int kCompactPerLane = 16;                                      // bytes per lane and tile: one flag word of 16 bits
constexpr int kCompactTile = kCompactThreads * kCompactPerLane;          // 4096 bytes of the mask per workgroup trip
constexpr int kCompactMaxBlocks = 1024;                                  // the grid stops growing: longer masks take more trips
constexpr int kBatchThreads = 256;

struct MaskCompactParams {
  const unsigned char* mask;
  long long n, per;      // workgroup b owns the bytes [b per, min(n, (b + 1) per)), per a multiple of the tile (share_of)
  int nblocks;
  long long* blk;        // (nblocks) non-zero bytes of each workgroup's share
  long long* inds;
  long long* count;
};

// launch 1: the per-workgroup counts
__global__ __launch_bounds__(kCompactThreads) void mask_count_kernel(const MaskCompactParams p) {
  long long lo, hi, c = 0;
  share_range(p.per, p.n, lo, hi);
  for (long long i = lo + threadIdx.x; i < hi; i += kCompactThreads) c += p.mask[i] != 0;
  c = block_sum_i64<kCompactThreads>(c);
  if (threadIdx.x == 0) p.blk[blockIdx.x] = c;
}

// launch 2: every workgroup sums the counts in front of it (at most kCompactMaxBlocks integers), then scatters its share tile by
// tile: a wave owns 1024 consecutive bytes of a tile as 16 rows of 64, the position of a set byte is its rank within its row
// plus the rows, waves and tiles in front of it (mf_scan.hpp)
__global__ __launch_bounds__(kCompactThreads) void mask_scatter_kernel(const MaskCompactParams p) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long front = 0, all = 0;
  for (int b = threadIdx.x; b < p.nblocks; b += kCompactThreads) {
    const long long v = p.blk[b];
    all += v;
    if (b < (int)blockIdx.x) front += v;
  }
  long long base = block_sum_i64<kCompactThreads>(front);
  if (blockIdx.x == 0) {
    all = block_sum_i64<kCompactThreads>(all);
    if (threadIdx.x == 0) *p.count = all;
  }
  long long lo, hi;
  share_range(p.per, p.n, lo, hi);
  for (long long tile = lo; tile < hi; tile += kCompactTile) {           // lo, hi: the same for every thread of the workgroup
    const long long wbase = tile + (long long)w * (64 * kCompactPerLane);
    unsigned flags = 0;
    int c[1] = {0}, waves_front[1], tile_tot[1];
#pragma unroll
    for (int j = 0; j < kCompactPerLane; ++j) {
      const long long i = wbase + j * 64 + lane;
      const bool m = i < hi && p.mask[i] != 0;
      flags |= (unsigned)m << j;
      c[0] += wave_popcount(m);
    }
    block_offsets<kCompactThreads, 1>(c, waves_front, tile_tot);
    long long off = base + waves_front[0];
#pragma unroll
    for (int j = 0; j < kCompactPerLane; ++j) {
      const bool m = (flags >> j) & 1u;
      int row;
      const int before = wave_rank(m, row);
      if (m) p.inds[off + before] = wbase + j * 64 + lane;               // off + before < the total count <= n
      off += row;
    }
    base += tile_tot[0];
    __syncthreads();                                                     // block_offsets' LDS is rewritten by the next tile
  }
}

// no mask: every pixel is valid
__global__ __launch_bounds__(kCompactThreads) void mask_identity_kernel(long long n, long long* inds, long long* count) {
  const long long i = (long long)blockIdx.x * kCompactThreads + threadIdx.x;
  if (i < n) inds[i] = i;
  if (i == 0) *count = n;
}

enum { kImageNone = 0, kImageRows = 1, kImageU8Rgb = 2, kImageU8Rgba = 3 };
enum { kBackgroundNone = 0, kBackgroundRows = 1, kBackgroundColour = 2 };

struct RayBatchParams {
  RayCam cam;
  float chain_idx;
  const long long* val_inds; long long n_valid;
  const long long* perm; long long n;
  const void* image; int image_kind;
  const float* background; int background_kind;
  float* rays; float* rgbs; float* background_out; long long* sel;
  int rays_vec;                    // rays is 16-byte aligned: rows are stored in float4 pieces
};

// v[0..N) to o[0..N): kHead single floats up to the next 16-byte boundary, whole float4 pieces, the rest single
template <int N, int kHead>
__device__ __forceinline__ void store_ray_row_from(float* o, const float (&v)[N]) {
  constexpr int nvec = (N - kHead) / 4;
#pragma unroll
  for (int i = 0; i < kHead; ++i) o[i] = v[i];
#pragma unroll
  for (int q = 0; q < nvec; ++q)
    *reinterpret_cast<float4*>(o + kHead + 4 * q) = make_float4(v[kHead + 4 * q], v[kHead + 4 * q + 1], v[kHead + 4 * q + 2], v[kHead + 4 * q + 3]);
#pragma unroll
  for (int i = kHead + 4 * nvec; i < N; ++i) o[i] = v[i];
}

// row `row` of an (n, N) fp32 table whose base is 16-byte aligned when `vec` (else: plain stores)
template <int N>
__device__ __forceinline__ void store_ray_row(float* base, long long row, const float (&v)[N], int vec) {
  const long long start = row * N;
  float* o = base + start;
  if (!vec) {
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = v[i];
    return;
  }
  switch ((int)((4 - (start & 3)) & 3)) {
    case 0: store_ray_row_from<N, 0>(o, v); break;
    case 1: store_ray_row_from<N, 1>(o, v); break;
    case 2: store_ray_row_from<N, 2>(o, v); break;
    default: store_ray_row_from<N, 3>(o, v); break;
  }
}

// One thread per selected ray.  kCols = 9, or 10 with the chain_global column.
template <int kCols>
__global__ __launch_bounds__(kBatchThreads) void ray_batch_kernel(const RayBatchParams p) {
  const long long k = (long long)blockIdx.x * kBatchThreads + threadIdx.x;
  if (k >= p.n) return;
  const float nan = __builtin_nanf("");
  // an index out of range is not dereferenced: the row is NaN (the caller cannot validate the permutation without a sync)
  const long long pos = p.perm[k];
  long long pix64 = -1;
  if (pos >= 0 && pos < p.n_valid) {
    pix64 = p.val_inds[pos];
    if (pix64 < 0 || pix64 >= (long long)p.cam.H * p.cam.W) pix64 = -1;
  }
  const bool ok = pix64 >= 0;
  const int pix = ok ? (int)pix64 : 0;                                     // H W < 2^31 (checked by the entry point)
  if (p.sel) p.sel[k] = pix64;

  float r[kCols];
  {
    float q[9];
    const int j = pix / p.cam.W, i = pix - j * p.cam.W;
    pixel_ray(p.cam, j, i, q);
#pragma unroll
    for (int c = 0; c < 9; ++c) r[c] = ok ? q[c] : nan;
    if (kCols == 10) r[kCols - 1] = ok ? p.chain_idx : nan;                // trainer_moco_flow.py:309-312
  }
  store_ray_row<kCols>(p.rays, k, r, p.rays_vec);

  float bg[3] = {nan, nan, nan};
  if (ok && p.background_kind == kBackgroundRows) {
#pragma unroll
    for (int c = 0; c < 3; ++c) bg[c] = p.background[(size_t)pix * 3 + c];
  } else if (ok && p.background_kind == kBackgroundColour) {
#pragma unroll
    for (int c = 0; c < 3; ++c) bg[c] = p.background[c];
  }
  if (p.background_out) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p.background_out[k * 3 + c] = bg[c];
  }
  if (p.image_kind == kImageNone) return;
  float rgb[3] = {nan, nan, nan};
  if (ok && p.image_kind == kImageRows) {
    const float* im = static_cast<const float*>(p.image);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = im[(size_t)pix * 3 + c];
  } else if (ok && p.image_kind == kImageU8Rgb) {
    const unsigned char* im = static_cast<const unsigned char*>(p.image);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = u8_unit(im[(size_t)pix * 3 + c]);
  } else if (ok) {
    composite_u8_rgba(static_cast<const unsigned*>(p.image)[pix], bg, rgb);           // r | g << 8 | b << 16 | a << 24
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) p.rgbs[k * 3 + c] = rgb[c];
}

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_mask_compact_scratch_bytes(int64_t n) {
  if (n < 0) { fail(MF_E_INVALID, "mf_mask_compact_scratch_bytes: negative n=%lld", (long long)n); return -1; }
  return (int64_t)share_of(n, kCompactTile, kCompactMaxBlocks).nblocks * 8;
}

extern "C" int32_t mf_mask_compact(const uint8_t* mask, int64_t n, int64_t* inds_out, int64_t* count, void* scratch, void* stream) {
  if (n < 0) return fail(MF_E_INVALID, "mf_mask_compact: negative n=%lld", (long long)n);
  if (!count) return fail(MF_E_INVALID, "mf_mask_compact: count is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n == 0) {
    if (hipMemsetAsync(count, 0, 8, s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mask_compact: hipMemsetAsync failed");
    return MF_OK;
  }
  if (!inds_out) return fail(MF_E_INVALID, "mf_mask_compact: inds_out is null");
  long long* inds = reinterpret_cast<long long*>(inds_out);
  long long* cnt = reinterpret_cast<long long*>(count);
  if (!mask) {
    hipLaunchKernelGGL(mask_identity_kernel, dim3((unsigned)((n + kCompactThreads - 1) / kCompactThreads)), dim3(kCompactThreads), 0, s,
                       (long long)n, inds, cnt);
    return check_launch("mf_mask_compact (identity)");
  }
  if (!scratch) return fail(MF_E_INVALID, "mf_mask_compact: scratch is null");
  const Share plan = share_of(n, kCompactTile, kCompactMaxBlocks);
  MaskCompactParams p{mask, (long long)n, plan.per, plan.nblocks, static_cast<long long*>(scratch), inds, cnt};
  hipLaunchKernelGGL(mask_count_kernel, dim3((unsigned)plan.nblocks), dim3(kCompactThreads), 0, s, p);
  hipLaunchKernelGGL(mask_scatter_kernel, dim3((unsigned)plan.nblocks), dim3(kCompactThreads), 0, s, p);
  return check_launch("mf_mask_compact");
}

extern "C" int32_t mf_ray_batch(const mf_ray_batch_args* a, void* stream) {
  if (!a) return fail(MF_E_INVALID, "mf_ray_batch: args is null");
  if (a->H < 0 || a->W < 0 || a->focal == 0.f) return fail(MF_E_INVALID, "mf_ray_batch: H=%d W=%d focal=%g", a->H, a->W, a->focal);
  const long long HW = (long long)a->H * a->W;
  if (HW >= (1LL << 31)) return fail(MF_E_INVALID, "mf_ray_batch: H W = %lld, 32-bit pixel indexing needs H W < 2^31", HW);
  if (a->n_rows < 0 || a->n_rows >= (1LL << 31) || a->n_valid < 0 || a->n_valid > HW)
    return fail(MF_E_INVALID, "mf_ray_batch: n_rows=%lld n_valid=%lld H W=%lld", (long long)a->n_rows, (long long)a->n_valid, HW);
  if (a->image_kind < kImageNone || a->image_kind > kImageU8Rgba) return fail(MF_E_INVALID, "mf_ray_batch: image_kind=%d", a->image_kind);
  if (a->background_kind < kBackgroundNone || a->background_kind > kBackgroundColour)
    return fail(MF_E_INVALID, "mf_ray_batch: background_kind=%d", a->background_kind);
  if (a->image_kind == kImageU8Rgba && a->background_kind == kBackgroundNone)
    return fail(MF_E_INVALID, "mf_ray_batch: an RGBA image needs a background to composite over");
  if (a->n_rows == 0) return MF_OK;
  if (!a->val_inds || !a->perm || !a->rays_out) return fail(MF_E_INVALID, "mf_ray_batch: null val_inds, perm or rays_out");
  if (a->image_kind != kImageNone && (!a->image || !a->rgbs_out)) return fail(MF_E_INVALID, "mf_ray_batch: null image or rgbs_out");
  if (a->background_kind != kBackgroundNone && !a->background) return fail(MF_E_INVALID, "mf_ray_batch: null background");
  if (a->background_kind == kBackgroundNone && a->background_out) return fail(MF_E_INVALID, "mf_ray_batch: background_out without a background");
  if (a->image_kind == kImageU8Rgba && !is_aligned(a->image, 4))
    return fail(MF_E_INVALID, "mf_ray_batch: an RGBA image must be 4-byte aligned");
  RayBatchParams p{};
  p.cam.H = a->H; p.cam.W = a->W; p.cam.fx = a->focal; p.cam.cx = a->cx; p.cam.cy = a->cy;
  ray_cam_set_c2w(p.cam, a->has_c2w ? a->c2w : nullptr);
  p.cam.nearv = a->nearv; p.cam.farv = a->farv; p.cam.idx = a->idx;
  p.chain_idx = a->chain_idx;
  p.val_inds = reinterpret_cast<const long long*>(a->val_inds); p.n_valid = a->n_valid;
  p.perm = reinterpret_cast<const long long*>(a->perm); p.n = a->n_rows;
  p.image = a->image; p.image_kind = a->image_kind;
  p.background = a->background; p.background_kind = a->background_kind;
  p.rays = a->rays_out; p.rgbs = a->rgbs_out; p.background_out = a->background_out;
  p.sel = reinterpret_cast<long long*>(a->sel_out);
  p.rays_vec = is_aligned(a->rays_out, 16);
  const dim3 grid((unsigned)((a->n_rows + kBatchThreads - 1) / kBatchThreads)), block(kBatchThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (a->has_chain) hipLaunchKernelGGL(ray_batch_kernel<10>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(ray_batch_kernel<9>, grid, block, 0, s, p);
  return check_launch("mf_ray_batch");
}
