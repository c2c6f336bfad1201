// mf_regions.hip -- matte clean-up on the device (include/mocoflow_hip.h: mf_mask_label, mf_mask_select, mf_mask_fill_holes,
// mf_mask_table_count / mf_mask_table_emit): the connected regions of a thresholded byte image, per frame of a stack; the mask of
// the largest region (or of every region of at least min_area pixels); its holes filled; the table of the regions with their
// areas and bounding boxes.  What scripts/data_utils.py:135-147 does per frame on the host with cv2 (threshold at 196, then
// find_max_region, :102-114).
//
// Contract (tests/regions_oracle.py restates it in numpy): members are alpha >= thres (below: alpha < thres); regions are the 8-
// or 4-connected components of the members of one frame (frames never interact, rows do not wrap); the label of a member is the
// smallest row-major index y W + x of its region, -1 for a non-member; the largest region has the most pixels, ties go to the
// smaller label; a hole of a mask is a 4-connected component of its zeros without a pixel on the frame's border.  Integers only;
// every output is a pure function of the input.
//
// Labelling is the union-find of mf_unionfind.hpp (invariants there) in three passes over parent[F H W], indexed by the global
// pixel index g = f H W + y W + x, -1 at non-members:
//   tile   one workgroup per tile of kRegTileH x 64 pixels.  A wave reads a row, one ballot gives the row's member bits; a member
//          starts under the first pixel of its run (bit operations on the row's mask), and the contacts with the row above come
//          from the two rows' masks: per pair of touching runs one union, in LDS, on tile-local indices.  The tile-local index
//          r 64 + c is monotone in g, so the local minimum is the global one and parent[x] <= x holds when the tile writes its
//          roots out as global indices: the global forest starts from the tiles' results, not from parent[x] = x.
//   seam   a member of a tile's top row unites with its N, NW and NE neighbours, one of its left column with W and NW, one of its
//          right column with NE (4-connectivity: N and W only): every neighbour pair that two tiles share, thinned as in the
//          tile pass to one union per pair of touching runs (reg_seam_kernel says why that loses nothing).
//   flat   labels[g] = root - f H W, and area[root] counted with uf::wave_count (a matte is one big region).
// Nothing waits on another workgroup; every loop is a strictly descending parent chain or a bounded grid-stride loop.
#include <climits>

#include "mf_host.hpp"
#include "mf_scan.hpp"
#include "mf_unionfind.hpp"

using namespace mf;

namespace mf {
namespace reg {

using namespace mf::uf;

constexpr int kRegTileH = 16;                   // rows of a tile: four per wave
constexpr int kRegTileW = 64;                   // one wave spans a tile row
constexpr int kRegThreads = 256;
constexpr int kRegMaxBlocks = 2048;             // grid-stride loops: the grid stops growing at 8 waves per SIMD of 256 CUs
constexpr int kRegWaves = kRegThreads / 64;
static_assert(kRegTileW == 64, "a wave's ballot is a tile row");

typedef unsigned long long u64;

struct Geom {
  int F, H, W, HW;
  int tiles_x, tiles_y;
  long long N;                                  // F H W < 2^31
};

inline Geom geom(int64_t F, int64_t H, int64_t W) {
  Geom g;
  g.F = (int)F; g.H = (int)H; g.W = (int)W; g.HW = (int)(H * W);
  g.tiles_x = (int)((W + kRegTileW - 1) / kRegTileW);
  g.tiles_y = (int)((H + kRegTileH - 1) / kRegTileH);
  g.N = F * H * W;
  return g;
}

inline unsigned grid_for(long long n) { return (unsigned)capped_blocks(n, kRegThreads, kRegMaxBlocks, 1); }

struct TileParams {
  Geom g;
  const unsigned char* alpha;                   // pixel g at alpha[g stride]
  int stride, thres, below, conn8;
  int* parent;
};

__global__ __launch_bounds__(kRegThreads) void reg_tile_kernel(const TileParams p) {
  __shared__ int lp[kRegTileH * kRegTileW];
  __shared__ u64 bits[kRegTileH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Geom& g = p.g;
  const long long ntiles = (long long)g.F * g.tiles_y * g.tiles_x;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {           // t: the same for the whole workgroup
    const int tx = (int)(t % g.tiles_x);
    const long long q = t / g.tiles_x;
    const int ty = (int)(q % g.tiles_y), f = (int)(q / g.tiles_y);
    const int x = tx * kRegTileW + lane, y0 = ty * kRegTileH, base = f * g.HW;
    // members of a row as one mask; a member starts under the first pixel of its run
    for (int r = wave; r < kRegTileH; r += kRegWaves) {
      const int y = y0 + r;
      bool m = false;
      if (y < g.H && x < g.W) {
        const int a = p.alpha[(long long)(base + y * g.W + x) * p.stride];
        m = p.below ? a < p.thres : a >= p.thres;
      }
      const u64 b = __ballot(m);
      if (lane == 0) bits[r] = b;
      const u64 gap = ~b & lanes_below(lane);                            // the non-members in front of this lane
      const int start = gap ? 64 - __clzll((long long)gap) : 0;
      lp[r * kRegTileW + lane] = r * kRegTileW + (m ? start : lane);
    }
    __syncthreads();
    // contacts with the row above: one union per pair of touching runs.  N at the first column the two runs share; NW / NE only
    // where no N contact of this pixel or its neighbour in the run already joins the same two runs
    for (int r = wave; r < kRegTileH; r += kRegWaves) {
      if (r == 0) continue;
      const u64 b = bits[r], a = bits[r - 1];
      const bool m = (b >> lane) & 1;
      const bool aN = (a >> lane) & 1, aW = lane > 0 && ((a >> (lane - 1)) & 1), aE = lane < 63 && ((a >> (lane + 1)) & 1);
      const bool bW = lane > 0 && ((b >> (lane - 1)) & 1), bE = lane < 63 && ((b >> (lane + 1)) & 1);
      const int me = r * kRegTileW + lane, up = me - kRegTileW;
      if (m) {
        if (aN && !(bW && aW)) unite(lp, me, up);
        if (p.conn8 && !aN) {
          if (aW && !bW) unite(lp, me, up - 1);
          if (aE && !bE) unite(lp, me, up + 1);
        }
      }
    }
    __syncthreads();
    for (int r = wave; r < kRegTileH; r += kRegWaves) {
      const int y = y0 + r;
      if (y < g.H && x < g.W) {
        int v = -1;
        if ((bits[r] >> lane) & 1) {
          const int l = find_root(lp, r * kRegTileW + lane);
          v = base + (y0 + (l >> 6)) * g.W + tx * kRegTileW + (l & 63);
        }
        p.parent[base + y * g.W + x] = v;
      }
    }
    __syncthreads();                                                     // lp and bits are rewritten by the next tile
  }
}

struct SeamParams {
  Geom g;
  int conn8;
  int* parent;
};

// items of a frame: the (tiles_y - 1) W pixels below a horizontal seam, then the (tiles_x - 1) H pixels right of a vertical one.
// Thinned like the tile pass, or the seams inside one big region would send three unions per pixel to one tree: W across a
// vertical seam always; N only at the first column that the run below and the run above share; a diagonal only where neither
// pixel beside it is a member -- through such a pixel the same two regions are joined by a W link, by an N link of this rule, or
// by the tile pass (members that touch inside a tile are joined by then).
__global__ __launch_bounds__(kRegThreads) void reg_seam_kernel(const SeamParams p) {
  const Geom& g = p.g;
  const long long hs = (long long)(g.tiles_y - 1) * g.W, vs = (long long)(g.tiles_x - 1) * g.H, per = hs + vs;
  const long long total = per * g.F;
  for (long long i = (long long)blockIdx.x * kRegThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kRegThreads) {
    const int f = (int)(i / per), base = f * g.HW;
    long long k = i - (long long)f * per;
    if (k < hs) {
      const int y = ((int)(k / g.W) + 1) * kRegTileH, x = (int)(k % g.W);      // y < H: a seam lies in front of the last tile row
      const int me = base + y * g.W + x, up = me - g.W;
      if (ld(p.parent + me) < 0) continue;
      const bool left = x > 0, right = x + 1 < g.W;
      const bool aN = ld(p.parent + up) >= 0, aW = left && ld(p.parent + up - 1) >= 0, aE = right && ld(p.parent + up + 1) >= 0;
      const bool bW = left && ld(p.parent + me - 1) >= 0, bE = right && ld(p.parent + me + 1) >= 0;
      if (aN && !(bW && aW)) unite(p.parent, me, up);
      if (p.conn8 && !aN) {
        if (aW && !bW) unite(p.parent, me, up - 1);
        if (aE && !bE) unite(p.parent, me, up + 1);
      }
    } else {
      k -= hs;
      const int x = ((int)(k / g.H) + 1) * kRegTileW, y = (int)(k % g.H);      // 0 < x < W
      const int me = base + y * g.W + x;
      const bool m = ld(p.parent + me) >= 0, mW = ld(p.parent + me - 1) >= 0;
      if (m && mW) unite(p.parent, me, me - 1);
      if (p.conn8 && y > 0 && m != mW) {                                      // one of the two, and its diagonal across the seam
        const int up = me - g.W;
        const bool aN = ld(p.parent + up) >= 0, aW = ld(p.parent + up - 1) >= 0;
        if (m && aW && !aN) unite(p.parent, me, up - 1);                      // NW
        if (mW && aN && !aW) unite(p.parent, me - 1, up);                     // NE from the last column of the tile on the left
      }
    }
  }
}

__global__ __launch_bounds__(kRegThreads) void reg_flatten_kernel(const Geom g, int* parent, int* labels, int* area) {
  WaveCount wc{0, 0};
  const long long step = (long long)gridDim.x * kRegThreads;
  for (long long b = (long long)blockIdx.x * kRegThreads; b < g.N; b += step) {      // b: the same for the whole wave
    const long long i = b + threadIdx.x;
    bool valid = false;
    int root = 0;
    if (i < g.N) {
      if (ld(parent + i) >= 0) {
        root = find_root(parent, (int)i);
        valid = true;
        labels[i] = root - (int)(i / g.HW) * g.HW;
      } else {
        labels[i] = -1;
      }
    }
    wave_count(area, root, valid, wc);
  }
  wave_count_flush(area, wc);
}

__device__ __forceinline__ bool is_root(const Geom& g, const int* labels, long long i, int& f, int& l) {
  l = labels[i];
  f = (int)(i / g.HW);
  return l >= 0 && l == (int)(i - (long long)f * g.HW);
}

// One value per frame from the roots of the stack.  Atomics to one word are served one at a time, so a wave walks a contiguous
// share and carries (frame, per-lane accumulator) until the frame changes: a few atomics per wave, not one per 64 pixels.
// value(i, label): what the root at pixel i gives; combine(acc, v): into the lane's accumulator, which starts at T(0);
// flush(frame, acc): every lane of the wave calls it, it reduces the lanes and sends the result to the frame's word.
template <class T, class Value, class Combine, class Flush>
__device__ __forceinline__ void carry_frames(const Geom& g, const int* labels, long long per, Value value, Combine combine, Flush flush) {
  long long lo, hi;
  share_range(per, g.N, lo, hi);
  T acc = 0;
  int fa = -1;                                                           // wave-uniform
  for (long long b = lo; b < hi; b += kRegThreads) {                     // b: the same for the whole wave
    const long long i = b + threadIdx.x;
    int f = -1, l;
    const bool root = i < hi && is_root(g, labels, i, f, l);
    const T v = root ? value(i, l) : T(0);
    u64 have = __ballot(root);
    while (have) {                                                       // the frames of the wave's roots, in order
      const int f0 = __shfl(f, __ffsll((long long)have) - 1);
      const bool mine = root && f == f0;
      if (f0 != fa) {
        if (fa >= 0) flush(fa, acc);
        acc = 0;
        fa = f0;
      }
      if (mine) combine(acc, v);
      have &= ~__ballot(mine);
    }
  }
  if (fa >= 0) flush(fa, acc);
}

// best[f] = max over the roots of (area << 32) | ~label: the largest area, ties to the smaller label; 0 without a member.
__global__ __launch_bounds__(kRegThreads) void reg_best_kernel(const Geom g, const int* labels, const int* area, u64* best, long long per) {
  carry_frames<u64>(g, labels, per,
                    [&](long long i, int l) { return ((u64)(unsigned)area[i] << 32) | (unsigned)~l; },
                    [](u64& acc, u64 v) { if (v > acc) acc = v; },
                    [&](int f, u64 v) {
#pragma unroll
                      for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(v, d); v = o > v ? o : v; }
                      if ((threadIdx.x & 63) == 0 && v) atomicMax(best + f, v);
                    });
}

__global__ __launch_bounds__(kRegThreads) void reg_select_kernel(const Geom g, const int* labels, const int* area, const u64* best,
                                                                 int largest, long long min_area, unsigned char* out) {
  for (long long i = (long long)blockIdx.x * kRegThreads + threadIdx.x; i < g.N; i += (long long)gridDim.x * kRegThreads) {
    const int l = labels[i];
    bool keep = false;
    if (l >= 0 && l < g.HW) {                                            // labels are an argument: never index beyond the frame
      const int f = (int)(i / g.HW);
      keep = area[f * g.HW + l] >= min_area && (!largest || l == (int)~(unsigned)best[f]);
    }
    out[i] = keep ? 255 : 0;
  }
}

// ---- holes: the zeros of the mask, 4-connected (reg_tile_kernel / reg_seam_kernel); a region with a pixel on the frame's border
// is marked at its root (every writer stores the same 1), the members of the unmarked ones are filled
__global__ __launch_bounds__(kRegThreads) void reg_hole_mark_kernel(const Geom g, int* parent, int* mark) {
  const long long per = 2LL * g.W + 2LL * g.H, total = per * g.F;
  for (long long i = (long long)blockIdx.x * kRegThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kRegThreads) {
    const int f = (int)(i / per);
    const int k = (int)(i - (long long)f * per);
    int x, y;
    if (k < g.W) { y = 0; x = k; }
    else if (k < 2 * g.W) { y = g.H - 1; x = k - g.W; }
    else if (k < 2 * g.W + g.H) { y = k - 2 * g.W; x = 0; }
    else { y = k - 2 * g.W - g.H; x = g.W - 1; }
    const int me = f * g.HW + y * g.W + x;
    if (ld(parent + me) >= 0) mark[find_root(parent, me)] = 1;
  }
}

__global__ __launch_bounds__(kRegThreads) void reg_hole_fill_kernel(const Geom g, int* parent, const int* mark, unsigned char* mask) {
  for (long long i = (long long)blockIdx.x * kRegThreads + threadIdx.x; i < g.N; i += (long long)gridDim.x * kRegThreads) {
    if (ld(parent + i) >= 0 && mark[find_root(parent, (int)i)] == 0) mask[i] = 255;
  }
}

// ---- table
// counts[f] += roots of frame f; a wave carries (frame, per-lane count) along its contiguous share, as reg_best_kernel does
__global__ __launch_bounds__(kRegThreads) void reg_table_count_kernel(const Geom g, const int* labels, long long* counts, long long per) {
  carry_frames<long long>(g, labels, per, [](long long, int) { return 1LL; }, [](long long& acc, long long v) { acc += v; },
                          [&](int f, long long v) { wave_add(counts + f, v); });
}

// workgroup b owns the pixels [b per, min(N, (b + 1) per)), per a multiple of the workgroup: rank of a root = the roots of the
// workgroups in front + of the rounds, waves and lanes in front (mf_scan.hpp): the rows come out in (frame, label) order
struct TableParams {
  Geom g;
  const int* labels;
  long long per;
  int nblocks;
  int frame0;                   // added to the table's frame column: the stack is a chunk of a longer one
  long long C;
  long long* blk;               // [nblocks] roots of each workgroup's share
  int* area;                    // [N] at the roots
  int* rank;                    // [N] at the roots: the row of the region, -1 beyond C
  int* table;                   // [C, 7]
};

__global__ __launch_bounds__(kRegThreads) void reg_table_area_kernel(const TableParams p) {
  const Geom& g = p.g;
  long long lo, hi, c = 0;
  share_range(p.per, g.N, lo, hi);
  WaveCount wc{0, 0};
  for (long long b = lo; b < hi; b += kRegThreads) {
    const long long i = b + threadIdx.x;
    int f = 0, l = -1;
    if (i < hi) c += is_root(g, p.labels, i, f, l);
    wave_count(p.area, f * g.HW + l, l >= 0 && l < g.HW, wc);
  }
  wave_count_flush(p.area, wc);
  c = block_sum_i64<kRegThreads>(c);
  if (threadIdx.x == 0) p.blk[blockIdx.x] = c;
}

__global__ __launch_bounds__(kRegThreads) void reg_table_rows_kernel(const TableParams p) {
  const Geom& g = p.g;
  long long front = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += kRegThreads) front += p.blk[b];
  long long lo, hi, base = block_sum_i64<kRegThreads>(front);
  share_range(p.per, g.N, lo, hi);
  for (long long b = lo; b < hi; b += kRegThreads) {                     // lo, hi: the same for every thread of the workgroup
    const long long i = b + threadIdx.x;
    int f = 0, l = -1;
    const bool root = i < hi && is_root(g, p.labels, i, f, l);
    int c[1], waves_front[1], round_tot[1];
    const int before = wave_rank(root, c[0]);
    block_offsets<kRegThreads, 1>(c, waves_front, round_tot);
    if (root) {
      const long long k = base + waves_front[0] + before;
      if (k < p.C) {
        int* row = p.table + 7 * k;
        row[0] = p.frame0 + f; row[1] = l; row[2] = p.area[i];
        row[3] = INT_MAX; row[4] = INT_MAX; row[5] = -1; row[6] = -1;
        p.rank[i] = (int)k;
      } else {
        p.rank[i] = -1;
      }
    }
    base += round_tot[0];
    __syncthreads();                                                     // block_offsets' LDS is rewritten by the next round
  }
}

// the bounds: integer atomicMin / atomicMax into the region's row.  A wave walks a contiguous share and carries the region most
// of it lies in (wave-uniform key, per-lane bounds) until another region takes the majority: one big region costs four atomics
// per wave, not per 64 pixels; a region with one pixel in the wave goes straight to its row, a few pixels are reduced first
__global__ __launch_bounds__(kRegThreads) void reg_table_bbox_kernel(const TableParams p) {
  const Geom& g = p.g;
  const int lane = threadIdx.x & 63;
  long long lo, hi;
  share_range(p.per, g.N, lo, hi);
  int ck = -1, cx0 = INT_MAX, cy0 = INT_MAX, cx1 = -1, cy1 = -1;        // ck: the same for the whole wave
  auto emit = [&](int kk, int x0, int y0, int x1, int y1) {             // every lane calls it; lane 0 holds the result
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
      x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
    }
    if (lane == 0) {
      int* row = p.table + 7 * (long long)kk;
      atomicMin(row + 3, x0); atomicMin(row + 4, y0); atomicMax(row + 5, x1); atomicMax(row + 6, y1);
    }
  };
  for (long long b = lo; b < hi; b += kRegThreads) {                     // b: the same for the whole wave
    const long long i = b + threadIdx.x;
    int k = -1, x = 0, y = 0;
    if (i < hi) {
      const int l = p.labels[i];
      if (l >= 0 && l < g.HW) {
        const int f = (int)(i / g.HW), pix = (int)(i - (long long)f * g.HW);
        k = p.rank[f * g.HW + l];
        y = pix / g.W;
        x = pix - y * g.W;
      }
    }
    u64 todo = __ballot(k >= 0);
    if (ck >= 0) {
      const bool mine = k == ck;
      if (mine) { cx0 = min(cx0, x); cy0 = min(cy0, y); cx1 = max(cx1, x); cy1 = max(cy1, y); }
      todo &= ~__ballot(mine);
    }
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int kk = __shfl(k, leader);
      const bool mine = k == kk;
      const u64 m = __ballot(mine);
      const int c = __popcll(m);
      if (c == 1) {
        if (lane == leader) {
          int* row = p.table + 7 * (long long)kk;
          atomicMin(row + 3, x); atomicMin(row + 4, y); atomicMax(row + 5, x); atomicMax(row + 6, y);
        }
      } else if (c > 32 || ck < 0) {                                     // the wave's majority (or the first region seen) is carried
        if (ck >= 0) emit(ck, cx0, cy0, cx1, cy1);
        ck = kk;
        cx0 = cy0 = INT_MAX; cx1 = cy1 = -1;
        if (mine) { cx0 = cx1 = x; cy0 = cy1 = y; }
      } else {
        emit(kk, mine ? x : INT_MAX, mine ? y : INT_MAX, mine ? x : -1, mine ? y : -1);
      }
      todo &= ~m;
    }
  }
  if (ck >= 0) emit(ck, cx0, cy0, cx1, cy1);
}

// scratch of every entry: parent int32 [N] | area int32 [N] | best uint64 [F] | blk int64 [kRegMaxBlocks]
struct Scratch { int* parent; int* area; u64* best; long long* blk; long long bytes; };

inline Scratch scratch_of(void* scratch, const Geom& g) {             // scratch null: the size alone
  Carver c(scratch);
  Scratch s;
  s.parent = c.take<int>(g.N);
  s.area = c.take<int>(g.N);
  s.best = c.take<u64>(g.F);
  s.blk = c.take<long long>(kRegMaxBlocks);
  s.bytes = c.bytes();
  return s;
}

int stack_shape(const char* what, int64_t F, int64_t H, int64_t W) {
  bool ok = F >= 0 && H >= 0 && W >= 0;
  if (ok && F > 0 && H > 0 && W > 0) {
    const unsigned __int128 hw = (unsigned __int128)H * (unsigned __int128)W;
    ok = hw < (unsigned __int128)kIndexLimit && hw * (unsigned __int128)F < (unsigned __int128)kIndexLimit;
  } else if (ok) {
    ok = F < kIndexLimit && H < kIndexLimit && W < kIndexLimit;
  }
  if (!ok) return fail(MF_E_INVALID, "%s: F=%lld H=%lld W=%lld (32-bit indexing: all >= 0 and F H W < 2^31)", what, (long long)F, (long long)H, (long long)W);
  return MF_OK;
}

// the three labelling passes; parent[] holds the forest afterwards (not yet flat)
void label_passes(const Geom& g, const unsigned char* alpha, int stride, int thres, int below, int conn8, int* parent, hipStream_t s) {
  const long long ntiles = (long long)g.F * g.tiles_y * g.tiles_x;
  TileParams tp{g, alpha, stride, thres, below, conn8, parent};
  hipLaunchKernelGGL(reg_tile_kernel, dim3((unsigned)capped_blocks(ntiles, 1, kRegMaxBlocks, 1)), dim3(kRegThreads), 0, s, tp);
  const long long seams = ((long long)(g.tiles_y - 1) * g.W + (long long)(g.tiles_x - 1) * g.H) * g.F;
  if (seams > 0) {
    SeamParams sp{g, conn8, parent};
    hipLaunchKernelGGL(reg_seam_kernel, dim3(grid_for(seams)), dim3(kRegThreads), 0, s, sp);
  }
}

}  // namespace reg
}  // namespace mf

using namespace mf::reg;

extern "C" int64_t mf_mask_label_scratch_bytes(int64_t F, int64_t H, int64_t W) {
  const int rc = stack_shape("mf_mask_label_scratch_bytes", F, H, W);
  return rc != MF_OK ? rc : scratch_of(nullptr, geom(F, H, W)).bytes;
}

extern "C" int32_t mf_mask_label(const uint8_t* alpha, int32_t stride, int64_t F, int64_t H, int64_t W, int32_t thres, int32_t below,
                                 int32_t connectivity, int32_t* labels, void* scratch, void* stream) {
  const int rc = stack_shape("mf_mask_label", F, H, W);
  if (rc != MF_OK) return rc;
  if (thres < 0 || thres > 256) return fail(MF_E_INVALID, "mf_mask_label: thres=%d; needs 0 <= thres <= 256", thres);
  if (connectivity != 4 && connectivity != 8) return fail(MF_E_INVALID, "mf_mask_label: connectivity=%d; 4 or 8", connectivity);
  if (stride != 1 && stride != 4) return fail(MF_E_INVALID, "mf_mask_label: stride=%d; 1 (alpha plane) or 4 (a channel of RGBA)", stride);
  const Geom g = geom(F, H, W);
  if (g.N == 0) return MF_OK;
  if (!alpha || !labels || !scratch) return fail(MF_E_INVALID, "mf_mask_label: alpha, labels or scratch is null");
  if (!is_aligned(labels, 4) || !is_aligned(scratch, 16)) return fail(MF_E_INVALID, "mf_mask_label: labels must be 4-byte, scratch 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Scratch sc = scratch_of(scratch, g);
  if (hipMemsetAsync(sc.area, 0, (size_t)(4 * g.N), s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mask_label: hipMemsetAsync failed");
  label_passes(g, alpha, stride, thres, below != 0, connectivity == 8, sc.parent, s);
  hipLaunchKernelGGL(reg_flatten_kernel, dim3(grid_for(g.N)), dim3(kRegThreads), 0, s, g, sc.parent, labels, sc.area);
  return check_launch("mf_mask_label");
}

extern "C" int32_t mf_mask_select(const int32_t* labels, int64_t F, int64_t H, int64_t W, int32_t largest, int64_t min_area, uint8_t* out,
                                  void* scratch, void* stream) {
  const int rc = stack_shape("mf_mask_select", F, H, W);
  if (rc != MF_OK) return rc;
  const Geom g = geom(F, H, W);
  if (g.N == 0) return MF_OK;
  if (!labels || !out || !scratch) return fail(MF_E_INVALID, "mf_mask_select: labels, out or scratch is null");
  if (!is_aligned(labels, 4) || !is_aligned(scratch, 16)) return fail(MF_E_INVALID, "mf_mask_select: labels must be 4-byte, scratch 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Scratch sc = scratch_of(scratch, g);
  if (hipMemsetAsync(sc.best, 0, (size_t)(8LL * g.F), s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mask_select: hipMemsetAsync failed");
  const Share plan = share_of(g.N, kRegThreads, kRegMaxBlocks);
  if (largest) hipLaunchKernelGGL(reg_best_kernel, dim3((unsigned)plan.nblocks), dim3(kRegThreads), 0, s, g, labels, sc.area, sc.best, plan.per);
  hipLaunchKernelGGL(reg_select_kernel, dim3(grid_for(g.N)), dim3(kRegThreads), 0, s, g, labels, sc.area, sc.best, (int)(largest != 0),
                     (long long)min_area, out);
  return check_launch("mf_mask_select");
}

extern "C" int32_t mf_mask_fill_holes(uint8_t* mask, int64_t F, int64_t H, int64_t W, void* scratch, void* stream) {
  const int rc = stack_shape("mf_mask_fill_holes", F, H, W);
  if (rc != MF_OK) return rc;
  const Geom g = geom(F, H, W);
  if (g.N == 0) return MF_OK;
  if (!mask || !scratch) return fail(MF_E_INVALID, "mf_mask_fill_holes: mask or scratch is null");
  if (!is_aligned(scratch, 16)) return fail(MF_E_INVALID, "mf_mask_fill_holes: scratch must be 16-byte aligned");
  if (H <= 2 || W <= 2) return MF_OK;                                   // every pixel lies on the border
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Scratch sc = scratch_of(scratch, g);
  if (hipMemsetAsync(sc.area, 0, (size_t)(4 * g.N), s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mask_fill_holes: hipMemsetAsync failed");
  label_passes(g, mask, 1, 1, 1, 0, sc.parent, s);                      // members: mask < 1, 4-connected
  hipLaunchKernelGGL(reg_hole_mark_kernel, dim3(grid_for((2 * H + 2 * W) * F)), dim3(kRegThreads), 0, s, g, sc.parent, sc.area);
  hipLaunchKernelGGL(reg_hole_fill_kernel, dim3(grid_for(g.N)), dim3(kRegThreads), 0, s, g, sc.parent, sc.area, mask);
  return check_launch("mf_mask_fill_holes");
}

extern "C" int32_t mf_mask_table_count(const int32_t* labels, int64_t F, int64_t H, int64_t W, int64_t* counts, void* stream) {
  const int rc = stack_shape("mf_mask_table_count", F, H, W);
  if (rc != MF_OK) return rc;
  if (F == 0) return MF_OK;
  if (!counts) return fail(MF_E_INVALID, "mf_mask_table_count: counts is null");
  const Geom g = geom(F, H, W);
  if (g.N > 0 && !labels) return fail(MF_E_INVALID, "mf_mask_table_count: labels is null");
  if (!is_aligned(labels, 4) || !is_aligned(counts, 8)) return fail(MF_E_INVALID, "mf_mask_table_count: labels must be 4-byte, counts 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, (size_t)(8 * F), s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mask_table_count: hipMemsetAsync failed");
  if (g.N == 0) return MF_OK;
  const Share plan = share_of(g.N, kRegThreads, kRegMaxBlocks);
  hipLaunchKernelGGL(reg_table_count_kernel, dim3((unsigned)plan.nblocks), dim3(kRegThreads), 0, s, g, labels, reinterpret_cast<long long*>(counts),
                     plan.per);
  return check_launch("mf_mask_table_count");
}

extern "C" int32_t mf_mask_table_emit(const int32_t* labels, int64_t F, int64_t H, int64_t W, int64_t frame0, int64_t C, int32_t* table,
                                      void* scratch, void* stream) {
  const int rc = stack_shape("mf_mask_table_emit", F, H, W);
  if (rc != MF_OK) return rc;
  const Geom g = geom(F, H, W);
  if (frame0 < 0 || frame0 >= kIndexLimit - F) return fail(MF_E_INVALID, "mf_mask_table_emit: frame0=%lld; needs 0 <= frame0 and frame0 + F < 2^31", (long long)frame0);
  if (C < 0 || C > g.N) return fail(MF_E_INVALID, "mf_mask_table_emit: C=%lld of F H W=%lld", (long long)C, g.N);
  if (C == 0) return MF_OK;
  if (!labels || !table || !scratch) return fail(MF_E_INVALID, "mf_mask_table_emit: labels, table or scratch is null");
  if (!is_aligned(labels, 4) || !is_aligned(table, 4) || !is_aligned(scratch, 16))
    return fail(MF_E_INVALID, "mf_mask_table_emit: labels and table must be 4-byte, scratch 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const Scratch sc = scratch_of(scratch, g);
  const Share plan = share_of(g.N, kRegThreads, kRegMaxBlocks);
  TableParams p{g, labels, plan.per, plan.nblocks, (int)frame0, (long long)C, sc.blk, sc.area, sc.parent, table};
  if (hipMemsetAsync(sc.area, 0, (size_t)(4 * g.N), s) != hipSuccess || hipMemsetAsync(table, 0, (size_t)(28 * C), s) != hipSuccess)
    return fail(MF_E_LAUNCH, "mf_mask_table_emit: hipMemsetAsync failed");
  hipLaunchKernelGGL(reg_table_area_kernel, dim3((unsigned)plan.nblocks), dim3(kRegThreads), 0, s, p);
  hipLaunchKernelGGL(reg_table_rows_kernel, dim3((unsigned)plan.nblocks), dim3(kRegThreads), 0, s, p);
  hipLaunchKernelGGL(reg_table_bbox_kernel, dim3((unsigned)plan.nblocks), dim3(kRegThreads), 0, s, p);
  return check_launch("mf_mask_table_emit");
}
