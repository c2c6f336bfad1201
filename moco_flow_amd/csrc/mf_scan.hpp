// mf_scan.hpp -- the ordered integer prefix of the library, written once.  Users: mf_sample.hip (compact_*_kernel: mf_compact_mask),
// mf_batch.hip (mask_*_kernel: mf_mask_compact), mf_mesh.hip (mc_scan_kernel; mc::block_scan: lanes_below), mf_mesh_components.hip (in_range, wave_add), mf_mesh_distance.hip (the same two), mf_mesh_rays.hip (in_range),
// mf_regions.hip (reg_best_kernel, reg_table_*_kernel), mf_mesh_simplify.hip (the survivors' and the used cells' ranks), mf_mesh_smooth.hip
// (the raw and the compact ring offsets), mf_lattice.hip (lat_*_kernel).  The four units that walk contiguous shares (mf_shares.hpp:
// share_of) take their range from share_range.
// Integer arithmetic: the order of the additions is free.  THE CONTRACT IS WHO RANKS BEFORE WHOM AND WHO SYNCHRONISES; "bit-
// identical, no atomics, original order kept" (the ray batch) rests on it.  Workgroups are 1-D, whole waves (lane =
// threadIdx.x & 63, wave = threadIdx.x >> 6); lower lanes rank before higher ones, lower waves and lower threads' shares likewise.
//   wave_popcount, wave_rank, wave_prefix_small, wave_prefix_i64, wave_sum_i64   every lane of the wave calls them (converged); no
//                                 LDS, no barrier
//   block_sum_i64<THREADS>        every thread of the workgroup calls it and receives the sum.  Owns THREADS / 64 words of LDS and
//                                 opens with the barrier that lets it be called again: the caller places none
//   block_offsets<THREADS, COLS>  every thread calls it and receives, per column, the sum of the totals of the waves in front of
//                                 its own and the workgroup's total.  Owns THREADS / 64 x COLS words of LDS and holds ONE barrier,
//                                 between its store and its loads.  THE CALLER places a __syncthreads() between two calls (the end
//                                 of a tile loop's body): without it a fast wave rewrites a total that a slow one still reads
//   scan_totals<THREADS, COLS>    the single-workgroup pass, once per kernel: every thread calls it and receives the grand
//                                 totals; it stores the offsets, the caller stores what it needs of the totals
//   wave_add                      every lane of the wave calls it: the wave's sum goes to a device counter in one atomic add
//   share_range                   the workgroup's [lo, hi) of a share_of plan: the same for every thread of the workgroup
#pragma once
#include <hip/hip_runtime.h>

namespace mf {

__device__ __forceinline__ bool in_range(long long i, long long n) { return (unsigned long long)i < (unsigned long long)n; }   // 0 <= i < n

// workgroup b of a share_of plan (mf_shares.hpp) owns [b per, min(n, (b + 1) per))
__device__ __forceinline__ void share_range(long long per, long long n, long long& lo, long long& hi) {
  lo = blockIdx.x * per;
  hi = lo + per < n ? lo + per : n;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }   // lane 0 .. 63; 0 for lane 0
__device__ __forceinline__ int wave_popcount(bool m) { return __popcll(__ballot(m)); }                  // the wave's set lanes
__device__ __forceinline__ int wave_rank(bool m, int& total) {          // one ballot: the set lanes in front of this one; all of them
  const unsigned long long b = __ballot(m);
  total = __popcll(b);
  return __popcll(b & lanes_below(threadIdx.x & 63));
}

// the exclusive prefix over the lanes of a small count v in [0, 2^BITS), and the wave's sum: one ballot per bit of v
template <int BITS>
__device__ __forceinline__ int wave_prefix_small(int v, int& total) {
  const unsigned long long below = lanes_below(threadIdx.x & 63);
  int before = 0;
  total = 0;
#pragma unroll
  for (int bit = 0; bit < BITS; ++bit) {
    const unsigned long long m = __ballot((v >> bit) & 1);
    before += __popcll(m & below) << bit;
    total += __popcll(m) << bit;
  }
  return before;
}

// the exclusive prefix over the lanes of any integer v, and the wave's sum: six shuffles (wave_prefix_small is cheaper for a
// count of a few bits)
__device__ __forceinline__ long long wave_prefix_i64(long long v, long long& total) {
  long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const long long u = __shfl_up(incl, d); if ((threadIdx.x & 63) >= d) incl += u; }
  total = __shfl(incl, 63);
  return incl - v;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {         // every lane receives the sum
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// the wave's sum of v, added once to a device counter (an integer sum: any order); nothing is sent for a sum of 0
__device__ __forceinline__ void wave_add(long long* counter, long long v) {
  v = wave_sum_i64(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)v);
}

template <int THREADS>
__device__ __forceinline__ long long block_sum_i64(long long v) {
  __shared__ long long red[THREADS / 64];
  v = wave_sum_i64(v);
  __syncthreads();                                                       // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) s += red[w];
  return s;
}

// The cross-wave exchange.  wave_total: the wave's totals, taken from its LAST lane (a wave-uniform count, or lane 63 of an
// inclusive scan).  front: the sum over the waves in front; total: over the whole workgroup.
template <int THREADS, int COLS, class T>
__device__ __forceinline__ void block_offsets(const T (&wave_total)[COLS], T (&front)[COLS], T (&total)[COLS]) {
  __shared__ T wave_tot[COLS][THREADS / 64];
  const int w = threadIdx.x >> 6;
  for (int c = 0; c < COLS; ++c) {
    if ((threadIdx.x & 63) == 63) wave_tot[c][w] = wave_total[c];
    front[c] = total[c] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int v = 0; v < THREADS / 64; ++v) {
    for (int c = 0; c < COLS; ++c) { if (v < w) front[c] += wave_tot[c][v]; total[c] += wave_tot[c][v]; }
  }
}

// One workgroup turns COLS columns of n totals (column c at totals + c n) into their exclusive int64 prefixes (offsets + c n) and
// the grand totals.  Thread t owns the entries [t per, min(n, (t + 1) per)), per = ceil(n / THREADS): it sums them, the sums are
// scanned across the wave and the workgroup, then it walks its share again.  In place (offsets == totals) is fine.  Made for a
// few entries per thread: neighbouring lanes read `per` entries apart, which is not coalesced for large n.
template <int THREADS, int COLS, class T>
__device__ __forceinline__ void scan_totals(const T* totals, long long n, long long* offsets, long long (&grand)[COLS]) {
  const long long per = (n + THREADS - 1) / THREADS, lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
  long long sum[COLS] = {}, incl[COLS], front[COLS];
  for (long long b = lo; b < hi; ++b)
    for (int c = 0; c < COLS; ++c) sum[c] += totals[c * n + b];
  __builtin_memcpy(incl, sum, sizeof(sum));
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    for (int c = 0; c < COLS; ++c) { const long long u = __shfl_up(incl[c], d); if ((threadIdx.x & 63) >= d) incl[c] += u; }
  }
  block_offsets<THREADS, COLS>(incl, front, grand);
  for (int c = 0; c < COLS; ++c) front[c] += incl[c] - sum[c];          // the exclusive offset of the thread's first entry
  for (long long b = lo; b < hi; ++b)
    for (int c = 0; c < COLS; ++c) { const long long v = totals[c * n + b]; offsets[c * n + b] = front[c]; front[c] += v; }
}

}  // namespace mf
