// mf_mesh_components.hip -- mesh clean-up on the device (include/mocoflow_hip.h: mf_mesh_label, mf_mesh_table_count /
// mf_mesh_table_emit, mf_mesh_filter_plan / mf_mesh_filter_emit, mf_gather_rows): connected components of an indexed
// triangle mesh through shared vertex indices, the per-component table, and the stable compaction of the mesh to the
// components a caller keeps.  What a user of extract_mesh otherwise does on the host with a graph library, after copying
// the whole mesh there.
//
// Contract (tests/mesh_components_oracle.py restates it in numpy): two vertices are adjacent if a triangle names both; the
// label of a vertex is the smallest vertex index of its component; a triangle belongs to the component of its column-0
// vertex; every output is a pure function of the input.
//
// Labelling: the lock-free union-find of mf_unionfind.hpp (its invariants are proved there) on 32-bit parents.  parent[v] = v;
// one pass over the triangles unites (t0, t1) and (t1, t2); one pass writes labels[v] = root of v, the smallest index of the
// component -- which thread won which compare-and-swap never shows in the result.
//
// Counts are uf::wave_count's integer atomic adds, reduced across a wave first: a mesh that is one big component would
// otherwise send every add to one address.  Compaction is
// mf_mask_compact (mf_batch.hip): ballots and fixed-order sums, original order kept.
#include "mf_host.hpp"
#include "mf_scan.hpp"
#include "mf_unionfind.hpp"

using namespace mf;

namespace mf {
namespace cc {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                 // grid-stride loops: the grid stops growing at 8 waves per SIMD of 256 CUs
// The two passes over the parents run 2 waves per SIMD: fewer unions in flight collide less often and find the paths already
// split by the ones before them.  Measured at 512^3 with 512 / 1024 / 2048 workgroups: a smooth field (1.8 M triangles, 4
// components) 1.32 / 1.68 / 1.88 ms, the random test NeRF's sigma (100 M triangles in 1.5 M components) 12.0 / 8.6 / 8.0 ms;
// a trained field's surface is the first kind.
constexpr int kUnionBlocks = 512;

inline unsigned grid_for(long long n, int cap = kMaxBlocks) { return (unsigned)capped_blocks(n, kThreads, cap, 1); }

using namespace mf::uf;                          // ld / st, find_root, unite, WaveCount / wave_count / wave_count_flush

__global__ __launch_bounds__(kThreads) void init_kernel(int* parent, long long V) {
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < V; v += (long long)gridDim.x * kThreads) parent[v] = (int)v;
}

__global__ __launch_bounds__(kThreads) void union_kernel(const long long* tris, long long T, long long V, int* parent, long long* bad) {
  long long nbad = 0;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < T; t += (long long)gridDim.x * kThreads) {
    const long long a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (in_range(a, V) && in_range(b, V) && in_range(c, V)) {
      unite(parent, (int)a, (int)b);
      unite(parent, (int)b, (int)c);
    } else {
      ++nbad;
    }
  }
  wave_add(bad, nbad);
}

__global__ __launch_bounds__(kThreads) void flatten_kernel(int* parent, long long V, long long* labels) {
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < V; v += (long long)gridDim.x * kThreads)
    labels[v] = find_root(parent, (int)v);
}

// ---- component table
struct TableParams {
  const long long* tris;
  long long T, V;
  const long long* labels;
  int* tcount;                  // [V] triangles of the component rooted here
  int* vcount;                  // [V] vertices
  unsigned char* is_root;       // [V]
  long long* counts;            // [C, bad]
};

__global__ __launch_bounds__(kThreads) void table_tris_kernel(const TableParams p) {
  long long nbad = 0;
  WaveCount wc{0, 0};
  const long long step = (long long)gridDim.x * kThreads;
  for (long long base = (long long)blockIdx.x * kThreads; base < p.T; base += step) {   // base: the same for the whole wave
    const long long t = base + threadIdx.x;
    bool ok = false;
    long long l = 0;
    if (t < p.T) {
      const long long a = p.tris[3 * t];
      if (in_range(a, p.V)) l = p.labels[a];
      ok = in_range(a, p.V) && in_range(l, p.V);
      if (!ok) ++nbad;
    }
    wave_count(p.tcount, (int)l, ok, wc);
  }
  wave_count_flush(p.tcount, wc);
  wave_add(p.counts + 1, nbad);
}

__global__ __launch_bounds__(kThreads) void table_verts_kernel(const TableParams p) {
  long long nbad = 0, nroot = 0;
  WaveCount wc{0, 0};
  const long long step = (long long)gridDim.x * kThreads;
  for (long long base = (long long)blockIdx.x * kThreads; base < p.V; base += step) {
    const long long v = base + threadIdx.x;
    bool ok = false;
    long long l = 0;
    if (v < p.V) {
      l = p.labels[v];
      ok = in_range(l, p.V);
      if (!ok) ++nbad;
      p.is_root[v] = l == v;
      nroot += l == v;
    }
    wave_count(p.vcount, (int)l, ok, wc);
  }
  wave_count_flush(p.vcount, wc);
  wave_add(p.counts, nroot);
  wave_add(p.counts + 1, nbad);
}

__global__ __launch_bounds__(kThreads) void table_gather_kernel(const long long* ids, long long C, const int* tcount, const int* vcount,
                                                                long long* tri_counts, long long* vert_counts) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < C; k += (long long)gridDim.x * kThreads) {
    const long long r = ids[k];
    tri_counts[k] = tcount[r];
    vert_counts[k] = vcount[r];
  }
}

// scratch of the table: tcount int32 [V] | vcount int32 [V] | is_root uint8 [V] | count int64 | mf_mask_compact's
struct TableScratch { int* tcount; int* vcount; unsigned char* is_root; long long* slot; void* compact; long long bytes; };

inline TableScratch table_scratch(void* scratch, long long V) {
  Carver c(scratch);
  TableScratch s;
  s.tcount = c.take<int>(V);
  s.vcount = c.take<int>(V);
  s.is_root = c.take<unsigned char>(V);
  s.slot = c.take<long long>(1);
  s.compact = c.take<char>(mf_mask_compact_scratch_bytes(V));
  s.bytes = c.bytes();
  return s;
}

// ---- filter
struct FilterParams {
  const long long* tris;
  long long T, V;
  const long long* labels;
  const long long* ids;
  const unsigned char* keep;
  long long C;
  unsigned char* keep_root;     // [V] 1 at the root of a kept component
  unsigned char* vflag;         // [V]
  unsigned char* tflag;         // [T]
  long long* counts;            // [kept vertices, kept triangles, bad]
};

__global__ __launch_bounds__(kThreads) void keep_roots_kernel(const FilterParams p) {
  long long nbad = 0;
  for (long long c = (long long)blockIdx.x * kThreads + threadIdx.x; c < p.C; c += (long long)gridDim.x * kThreads) {
    const long long r = p.ids[c];
    if (!in_range(r, p.V)) ++nbad;
    else if (p.keep[c]) p.keep_root[r] = 1;
  }
  wave_add(p.counts + 2, nbad);
}

__global__ __launch_bounds__(kThreads) void keep_verts_kernel(const FilterParams p) {
  long long nbad = 0, nkeep = 0;
  for (long long v = (long long)blockIdx.x * kThreads + threadIdx.x; v < p.V; v += (long long)gridDim.x * kThreads) {
    const long long l = p.labels[v];
    const bool ok = in_range(l, p.V);
    const bool k = ok && p.keep_root[l] != 0;
    if (!ok) ++nbad;
    p.vflag[v] = k;
    nkeep += k;
  }
  wave_add(p.counts, nkeep);
  wave_add(p.counts + 2, nbad);
}

__global__ __launch_bounds__(kThreads) void keep_tris_kernel(const FilterParams p) {
  long long nbad = 0, nkeep = 0;
  for (long long t = (long long)blockIdx.x * kThreads + threadIdx.x; t < p.T; t += (long long)gridDim.x * kThreads) {
    const long long a = p.tris[3 * t], b = p.tris[3 * t + 1], c = p.tris[3 * t + 2];
    const bool ok = in_range(a, p.V) && in_range(b, p.V) && in_range(c, p.V);
    const bool k = ok && p.vflag[a] != 0;
    if (!ok) ++nbad;
    p.tflag[t] = k;
    nkeep += k;
  }
  wave_add(p.counts + 1, nkeep);
  wave_add(p.counts + 2, nbad);
}

__global__ __launch_bounds__(kThreads) void remap_kernel(const long long* vert_inds, long long Vk, int* remap) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < Vk; k += (long long)gridDim.x * kThreads)
    remap[vert_inds[k]] = (int)k;
}

__global__ __launch_bounds__(kThreads) void reindex_kernel(const long long* tris, long long V, const long long* tri_inds, long long Tk,
                                                           const int* remap, long long* tris_out) {
  for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < Tk; k += (long long)gridDim.x * kThreads) {
    const long long t = tri_inds[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long i = tris[3 * t + c];
      tris_out[3 * k + c] = in_range(i, V) ? remap[i] : -1;
    }
  }
}

// scratch of the filter: keep_root uint8 [V] | vflag uint8 [V] | tflag uint8 [T] | remap int32 [V] | count int64 |
// mf_mask_compact's, the larger of the two masks' needs
struct FilterScratch { unsigned char* keep_root; unsigned char* vflag; unsigned char* tflag; int* remap; long long* slot; void* compact; long long bytes; };

inline FilterScratch filter_scratch(void* scratch, long long V, long long T) {
  Carver c(scratch);
  FilterScratch s;
  s.keep_root = c.take<unsigned char>(V);
  s.vflag = c.take<unsigned char>(V);
  s.tflag = c.take<unsigned char>(T);
  s.remap = c.take<int>(V);
  s.slot = c.take<long long>(1);
  const long long cv = mf_mask_compact_scratch_bytes(V), ct = mf_mask_compact_scratch_bytes(T);   // not monotonic in n
  s.compact = c.take<char>(cv > ct ? cv : ct);
  s.bytes = c.bytes();
  return s;
}

// ---- row gather: dst row k = src row inds[k], rows of `words` 4-byte words (kWord) or of `words` bytes
template <class W>
__global__ __launch_bounds__(kThreads) void gather_rows_kernel(const W* src, long long n_src, long long words, const long long* inds,
                                                               long long n, W* dst) {
  const long long total = n * words;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const long long k = i / words, w = i - k * words;
    const long long r = inds[k];
    dst[i] = in_range(r, n_src) ? src[r * words + w] : W(0);
  }
}

}  // namespace cc
}  // namespace mf

using namespace mf::cc;

extern "C" int64_t mf_mesh_label_scratch_bytes(int64_t V, int64_t T) {
  const int rc = mesh_index_shape("mf_mesh_label_scratch_bytes", V, T);
  return rc != MF_OK ? rc : align_up(4 * V, 16);
}

extern "C" int32_t mf_mesh_label(const int64_t* tris, int64_t T, int64_t V, int64_t* labels, int64_t* bad, void* scratch,
                                 void* stream) {
  const int rc = mesh_index_shape("mf_mesh_label", V, T);
  if (rc != MF_OK) return rc;
  if (!bad) return fail(MF_E_INVALID, "mf_mesh_label: bad is null");
  if (T > 0 && !tris) return fail(MF_E_INVALID, "mf_mesh_label: tris is null");
  if (V > 0 && (!labels || !scratch)) return fail(MF_E_INVALID, "mf_mesh_label: labels or scratch is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(bad, 0, 8, s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mesh_label: hipMemsetAsync failed");
  int* parent = static_cast<int*>(scratch);
  const long long* tr = reinterpret_cast<const long long*>(tris);
  if (V > 0) hipLaunchKernelGGL(init_kernel, dim3(grid_for(V)), dim3(kThreads), 0, s, parent, (long long)V);
  if (T > 0) hipLaunchKernelGGL(union_kernel, dim3(grid_for(T, kUnionBlocks)), dim3(kThreads), 0, s, tr, (long long)T, (long long)V, parent,
                                reinterpret_cast<long long*>(bad));
  if (V > 0) hipLaunchKernelGGL(flatten_kernel, dim3(grid_for(V, kUnionBlocks)), dim3(kThreads), 0, s, parent, (long long)V,
                                reinterpret_cast<long long*>(labels));
  return check_launch("mf_mesh_label");
}

extern "C" int64_t mf_mesh_table_scratch_bytes(int64_t V, int64_t T) {
  const int rc = mesh_index_shape("mf_mesh_table_scratch_bytes", V, T);
  return rc != MF_OK ? rc : table_scratch(nullptr, V).bytes;
}

extern "C" int32_t mf_mesh_table_count(const int64_t* tris, int64_t T, int64_t V, const int64_t* labels, int64_t* counts,
                                       void* scratch, void* stream) {
  const int rc = mesh_index_shape("mf_mesh_table_count", V, T);
  if (rc != MF_OK) return rc;
  if (!counts) return fail(MF_E_INVALID, "mf_mesh_table_count: counts is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 16, s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mesh_table_count: hipMemsetAsync failed");
  if (V == 0 && T == 0) return MF_OK;
  if (T > 0 && !tris) return fail(MF_E_INVALID, "mf_mesh_table_count: tris is null");
  if (V > 0 && (!labels || !scratch)) return fail(MF_E_INVALID, "mf_mesh_table_count: labels or scratch is null");
  const TableScratch ts = table_scratch(scratch, V);
  TableParams p{reinterpret_cast<const long long*>(tris), (long long)T, (long long)V, reinterpret_cast<const long long*>(labels),
                ts.tcount, ts.vcount, ts.is_root, reinterpret_cast<long long*>(counts)};
  if (V > 0 && hipMemsetAsync(ts.tcount, 0, (size_t)(reinterpret_cast<char*>(ts.is_root) - reinterpret_cast<char*>(ts.tcount)), s) != hipSuccess)
    return fail(MF_E_LAUNCH, "mf_mesh_table_count: hipMemsetAsync failed");
  if (T > 0) hipLaunchKernelGGL(table_tris_kernel, dim3(grid_for(T)), dim3(kThreads), 0, s, p);
  if (V > 0) hipLaunchKernelGGL(table_verts_kernel, dim3(grid_for(V)), dim3(kThreads), 0, s, p);
  return check_launch("mf_mesh_table_count");
}

extern "C" int32_t mf_mesh_table_emit(int64_t V, int64_t C, void* scratch, int64_t* ids, int64_t* tri_counts, int64_t* vert_counts,
                                      void* stream) {
  const int rc = mesh_index_shape("mf_mesh_table_emit", V, 0);
  if (rc != MF_OK) return rc;
  if (C < 0 || C > V) return fail(MF_E_INVALID, "mf_mesh_table_emit: C=%lld of V=%lld", (long long)C, (long long)V);
  if (C == 0) return MF_OK;
  if (!scratch || !ids || !tri_counts || !vert_counts) return fail(MF_E_INVALID, "mf_mesh_table_emit: null argument");
  const TableScratch ts = table_scratch(scratch, V);
  const int rc2 = mf_mask_compact(ts.is_root, V, ids, reinterpret_cast<int64_t*>(ts.slot), ts.compact, stream);
  if (rc2 != MF_OK) return rc2;
  hipLaunchKernelGGL(table_gather_kernel, dim3(grid_for(C)), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(ids), (long long)C, ts.tcount, ts.vcount,
                     reinterpret_cast<long long*>(tri_counts), reinterpret_cast<long long*>(vert_counts));
  return check_launch("mf_mesh_table_emit");
}

extern "C" int64_t mf_mesh_filter_scratch_bytes(int64_t V, int64_t T) {
  const int rc = mesh_index_shape("mf_mesh_filter_scratch_bytes", V, T);
  return rc != MF_OK ? rc : filter_scratch(nullptr, V, T).bytes;
}

extern "C" int32_t mf_mesh_filter_plan(const int64_t* tris, int64_t T, int64_t V, const int64_t* labels, const int64_t* ids,
                                       const uint8_t* keep, int64_t C, int64_t* counts, void* scratch, void* stream) {
  const int rc = mesh_index_shape("mf_mesh_filter_plan", V, T);
  if (rc != MF_OK) return rc;
  if (C < 0 || C > V) return fail(MF_E_INVALID, "mf_mesh_filter_plan: C=%lld of V=%lld", (long long)C, (long long)V);
  if (!counts) return fail(MF_E_INVALID, "mf_mesh_filter_plan: counts is null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(counts, 0, 24, s) != hipSuccess) return fail(MF_E_LAUNCH, "mf_mesh_filter_plan: hipMemsetAsync failed");
  if (V == 0 && T == 0) return MF_OK;
  if (T > 0 && !tris) return fail(MF_E_INVALID, "mf_mesh_filter_plan: tris is null");
  if (V > 0 && (!labels || !scratch)) return fail(MF_E_INVALID, "mf_mesh_filter_plan: labels or scratch is null");
  if (C > 0 && (!ids || !keep)) return fail(MF_E_INVALID, "mf_mesh_filter_plan: ids or keep is null");
  if (V == 0 && !scratch) return fail(MF_E_INVALID, "mf_mesh_filter_plan: scratch is null");
  const FilterScratch fs = filter_scratch(scratch, V, T);
  FilterParams p{reinterpret_cast<const long long*>(tris), (long long)T, (long long)V, reinterpret_cast<const long long*>(labels),
                 reinterpret_cast<const long long*>(ids), keep, (long long)C, fs.keep_root, fs.vflag, fs.tflag,
                 reinterpret_cast<long long*>(counts)};
  if (V > 0 && (hipMemsetAsync(fs.keep_root, 0, (size_t)V, s) != hipSuccess || hipMemsetAsync(fs.remap, 0xff, (size_t)(4 * V), s) != hipSuccess))
    return fail(MF_E_LAUNCH, "mf_mesh_filter_plan: hipMemsetAsync failed");
  if (C > 0) hipLaunchKernelGGL(keep_roots_kernel, dim3(grid_for(C)), dim3(kThreads), 0, s, p);
  if (V > 0) hipLaunchKernelGGL(keep_verts_kernel, dim3(grid_for(V)), dim3(kThreads), 0, s, p);
  if (T > 0) hipLaunchKernelGGL(keep_tris_kernel, dim3(grid_for(T)), dim3(kThreads), 0, s, p);
  return check_launch("mf_mesh_filter_plan");
}

extern "C" int32_t mf_mesh_filter_emit(const int64_t* tris, int64_t T, int64_t V, int64_t Vk, int64_t Tk, void* scratch,
                                       int64_t* vert_inds, int64_t* tri_inds, int64_t* tris_out, void* stream) {
  const int rc = mesh_index_shape("mf_mesh_filter_emit", V, T);
  if (rc != MF_OK) return rc;
  if (Vk < 0 || Vk > V || Tk < 0 || Tk > T)
    return fail(MF_E_INVALID, "mf_mesh_filter_emit: Vk=%lld of V=%lld, Tk=%lld of T=%lld", (long long)Vk, (long long)V, (long long)Tk, (long long)T);
  if (Vk == 0 && Tk == 0) return MF_OK;
  if (!scratch) return fail(MF_E_INVALID, "mf_mesh_filter_emit: scratch is null");
  if (Vk > 0 && !vert_inds) return fail(MF_E_INVALID, "mf_mesh_filter_emit: vert_inds is null");
  if (Tk > 0 && (!tris || !tri_inds || !tris_out)) return fail(MF_E_INVALID, "mf_mesh_filter_emit: tris, tri_inds or tris_out is null");
  const FilterScratch fs = filter_scratch(scratch, V, T);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (Vk > 0) {
    const int rc2 = mf_mask_compact(fs.vflag, V, vert_inds, reinterpret_cast<int64_t*>(fs.slot), fs.compact, stream);
    if (rc2 != MF_OK) return rc2;
    hipLaunchKernelGGL(remap_kernel, dim3(grid_for(Vk)), dim3(kThreads), 0, s, reinterpret_cast<const long long*>(vert_inds),
                       (long long)Vk, fs.remap);
  }
  if (Tk > 0) {
    const int rc2 = mf_mask_compact(fs.tflag, T, tri_inds, reinterpret_cast<int64_t*>(fs.slot), fs.compact, stream);
    if (rc2 != MF_OK) return rc2;
    hipLaunchKernelGGL(reindex_kernel, dim3(grid_for(Tk)), dim3(kThreads), 0, s, reinterpret_cast<const long long*>(tris), (long long)V,
                       reinterpret_cast<const long long*>(tri_inds), (long long)Tk, fs.remap, reinterpret_cast<long long*>(tris_out));
  }
  return check_launch("mf_mesh_filter_emit");
}

extern "C" int32_t mf_gather_rows(const void* src, int64_t n_src, int64_t row_bytes, const int64_t* inds, int64_t n, void* dst,
                                  void* stream) {
  if (n_src < 0 || n < 0 || row_bytes < 0)
    return fail(MF_E_INVALID, "mf_gather_rows: n_src=%lld n=%lld row_bytes=%lld", (long long)n_src, (long long)n, (long long)row_bytes);
  if (n == 0 || row_bytes == 0) return MF_OK;
  if (n > INT64_MAX / row_bytes) return fail(MF_E_INVALID, "mf_gather_rows: n row_bytes overflows");
  if (!inds || !dst || (n_src > 0 && !src)) return fail(MF_E_INVALID, "mf_gather_rows: null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long* ix = reinterpret_cast<const long long*>(inds);
  const bool words = row_bytes % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
  if (words)
    hipLaunchKernelGGL(gather_rows_kernel<unsigned>, dim3(grid_for(n * (row_bytes / 4))), dim3(kThreads), 0, s,
                       static_cast<const unsigned*>(src), (long long)n_src, (long long)(row_bytes / 4), ix, (long long)n, static_cast<unsigned*>(dst));
  else
    hipLaunchKernelGGL(gather_rows_kernel<unsigned char>, dim3(grid_for(n * row_bytes)), dim3(kThreads), 0, s,
                       static_cast<const unsigned char*>(src), (long long)n_src, (long long)row_bytes, ix, (long long)n, static_cast<unsigned char*>(dst));
  return check_launch("mf_gather_rows");
}
