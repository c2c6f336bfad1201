// mf_reduce.hpp -- the fixed-order float64 reduction of the library, written once.  Users:
//   mf_loss.hip       loss_partials_kernel / loss_finish_kernel               12 slots
//   mf_supervise.hip  point_loss_partials_kernel / point_loss_finish_kernel    5 slots
//   mf_metrics.hip    ssim_kernel, sqerr_kernel / metrics_finish_kernel        2 slots
//   mf_occupancy.hip  occ_build_kernel / occ_count_finish_kernel               1 slot (count_finish)
//   mf_voxelize.hip   voxel_dilate_rows_kernel / voxel_count_finish_kernel     1 slot (count_finish)
//   mf_distance.hip   edt_x_kernel / edt_count_finish_kernel                   1 slot (count_finish)
//   mf_mesh_distance.hip  md_stats_kernel / md_stats_finish_kernel            13 slots
// THE CONTRACT IS THE ORDER OF THE ADDITIONS; "two runs are bit-identical, no atomics"  rests on it:
//   a thread      adds its own elements (or, in a finish, the partial rows t, t + THREADS, t + 2 THREADS, ...) in ascending order
//   wave_sum_d    adds the 64 lanes of a wave in the fixed tree below
//   block_sum_d   adds the waves' sums from 0.0 in wave order 0, 1, 2, ...
//   a launch      stores one row of SLOTS partials per workgroup (block_sum_d -> parts + blockIdx.x * SLOTS); ONE finishing
//                 workgroup gathers the rows (gather_sum_d) -- into the result, or into LDS in front of an epilogue of its own
// Every chain starts at +0.0, so no partial is ever -0.0 and `0.0 + x` is `x`.
#pragma once
#include <hip/hip_runtime.h>

namespace mf {

// Sum over the 64 lanes, returned wave-uniform, on the DPP path (row shifts + row broadcasts, both halves of the double moved
// together: ~20 instructions).  The six __shfl_xor steps it replaces are twelve ds_bpermute round trips per value, and the loss
// kernels reduce TWELVE values (round 4, under rocprofv3: partials kernel 9.9 -> 8.3 us, finish kernel 4.9 -> 4.5 at C5's shard).
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_f64(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xf, false);
  return __builtin_bit_cast(double, (unsigned long long)lo | ((unsigned long long)hi << 32));
}
// (row_bcast:15 / :31 exist on the GFX9 family only -- gfx90a / gfx942 / gfx950; this library is built for gfx950 alone, but the
//  Makefile's ARCH is overridable, so any other target takes the xor-shuffle tree: the sums are float64, the order is free)
__device__ inline double wave_sum_d(double v) {
#if !(defined(__gfx950__) || defined(__gfx942__) || defined(__gfx90a__)) && defined(__HIP_DEVICE_COMPILE__)
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
#endif
  v += dpp_f64<0x111, 0xf>(v);                   // row_shr:1, 2, 4, 8 -- lane 15 of every row holds the row's sum
  v += dpp_f64<0x112, 0xf>(v);
  v += dpp_f64<0x114, 0xf>(v);
  v += dpp_f64<0x118, 0xf>(v);
  v += dpp_f64<0x142, 0xa>(v);                   // row_bcast:15 -> rows 1, 3
  v += dpp_f64<0x143, 0xc>(v);                   // row_bcast:31 -> rows 2, 3: lane 63 holds the wave's sum
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, 63), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), 63);
  return __builtin_bit_cast(double, (unsigned long long)lo | ((unsigned long long)hi << 32));
}

// The workgroup's sums of SLOTS per-thread values -> dst[0 .. SLOTS), written by threads 0 .. SLOTS - 1.  Every one of the
// THREADS threads calls it, once per kernel.  dst: the workgroup's row of the partials, or LDS that the caller reads after a
// __syncthreads() of its own.
template <int THREADS, int SLOTS>
__device__ inline void block_sum_d(const double (&v)[SLOTS], double* dst) {
  static_assert(THREADS % 64 == 0 && SLOTS <= THREADS, "whole waves, one thread per slot");
  __shared__ double red[THREADS / 64][SLOTS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const double s = wave_sum_d(v[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < SLOTS) {
    double s = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) s += red[w][threadIdx.x];
    dst[threadIdx.x] = s;
  }
}

// The finishing workgroup: the sums of the (n_parts, SLOTS) partial rows -> dst[0 .. SLOTS).  Thread t adds rows t, t + THREADS,
// ... from 0.0 in that order (independent loads: one thread per slot walking the rows took longer than the partials kernel).
template <int THREADS, int SLOTS>
__device__ inline void gather_sum_d(const double* parts, long long n_parts, double* dst) {
  double v[SLOTS];
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) v[k] = 0.0;
  for (long long i = threadIdx.x; i < n_parts; i += THREADS) {
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) v[k] += parts[i * SLOTS + k];
  }
  block_sum_d<THREADS, SLOTS>(v, dst);
}

// The finishing workgroup of a cell count (occ_count_finish_kernel, voxel_count_finish_kernel): the partials are popcounts,
// integers whose sum stays below 2^31, so the float64 sum is exact in any order.
template <int THREADS>
__device__ inline void count_finish(const double* parts, long long n_parts, long long* count) {
  __shared__ double total[1];
  gather_sum_d<THREADS, 1>(parts, n_parts, total);
  __syncthreads();
  if (threadIdx.x == 0) *count = (long long)total[0];
}

}  // namespace mf
