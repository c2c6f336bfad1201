// mf_supervise.hip -- the SMPL point supervision of a training step on the device, without a compaction or a host read
// (include/mocoflow_hip.h):
//   mf_point_correspond             : query points -> nearest source-pose vertex -> that vertex's transform -> [query | cano],
//                                     inside = dist < thickness                    datasets/moco_flow_dataset.py:107-132
//   mf_point_loss_partials          : the three point losses as (sum, count) pairs  trainer/trainer_moco_flow.py:146-157, 330-363
//   mf_point_loss_partials_backward : their seeds, written whole (zeros where the mask is off)
// Outputs are full length and keep the queries' order; the inside / outside split is a mask.  The reductions are the fixed-order
// sums of mf_reduce.hpp through `scratch`: no atomics, bit-identical from run to run.
#include "mf_host.hpp"
#include "mf_reduce.hpp"

// near-surface queries are verts[pick] + noise * thickness as torch evaluates them: the product and the sum rounded once each
// (the Makefile builds every unit with -ffp-contract=off; the pragma keeps it true for a build that forgets the flag)
#pragma clang fp contract(off)

namespace mf {

constexpr int kCorrThreads = 256;
constexpr int kCorrTile = 1024;                     // vertices per LDS tile, as mf_knn1
constexpr int kNoVertex = 0x7fffffff;               // the index of a lane that saw no candidate: loses every comparison

struct CorrespondParams {
  const float* verts; const float* trans; int V;
  const float* query; long long q_given;
  const long long* pick; const float* noise; long long q_near;
  float thickness;
  float* pairs; unsigned char* inside; float* dist; long long* ind;
};

// kLanes lanes of one wave share a query (kLanes = 1: mf_knn1's one thread per query); a workgroup holds 256 / kLanes queries.
// Lane s of a query's group takes the vertices v = s (mod kLanes) of every tile, in ascending order with a strict `<`, so it
// holds the FIRST minimum of its own share; the shares are then merged with the lexicographic minimum of (d, index), which is
// the first minimum of the whole scan: among equal d the lowest index wins, whichever lane held it.
//
// LDS: the tile keeps mf_knn1's layout, word 3 v + c for component c of vertex v.  The three reads of a candidate are 4-byte
// reads (12-byte rows give no wider alignment), banked (address / 4) mod 32 within each half-wave of 32 lanes.  In one
// half-wave the lanes of a group read words 3 (v0 + s) + c, s = 0 .. min(kLanes, 32) - 1: since 3 is a unit mod 32, at most 32
// consecutive s fall into 32 different banks -- no conflict; the other groups of the half-wave read the SAME words, which the
// LDS broadcasts.  The fill writes word k from lane k (mod 256): consecutive words, consecutive banks.
template <int kLanes>
__global__ __launch_bounds__(kCorrThreads) void point_correspond_kernel(const CorrespondParams p) {
  __shared__ float tile[kCorrTile * 3];
  const int sub = threadIdx.x % kLanes;
  const long long Q = p.q_given + p.q_near;
  const long long q = (long long)blockIdx.x * (kCorrThreads / kLanes) + threadIdx.x / kLanes;
  const bool valid = q < Q;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (valid) {
    if (q < p.q_given) {
      qx = p.query[q * 3]; qy = p.query[q * 3 + 1]; qz = p.query[q * 3 + 2];
    } else {                                                       // moco_flow_dataset.py:110-111
      const long long j = q - p.q_given;
      long long v = p.pick[j];
      v = v < 0 ? 0 : (v >= p.V ? p.V - 1 : v);
      const float t = p.thickness;
      const float mx = p.noise[j * 3] * t, my = p.noise[j * 3 + 1] * t, mz = p.noise[j * 3 + 2] * t;
      qx = p.verts[v * 3] + mx; qy = p.verts[v * 3 + 1] + my; qz = p.verts[v * 3 + 2] + mz;
    }
  }
  float best = __builtin_inff();
  int besti = kNoVertex;
  for (int base = 0; base < p.V; base += kCorrTile) {              // the same trips for every thread of the workgroup
    const int n = p.V - base < kCorrTile ? p.V - base : kCorrTile;
    __syncthreads();
    for (int k = threadIdx.x; k < n * 3; k += kCorrThreads) tile[k] = p.verts[(long long)base * 3 + k];
    __syncthreads();
    for (int v = sub; v < n; v += kLanes) {
      const float ax = tile[v * 3] - qx, ay = tile[v * 3 + 1] - qy, az = tile[v * 3 + 2] - qz;
      const float d = __builtin_fmaf(az, az, __builtin_fmaf(ay, ay, ax * ax));      // mf_knn1's expression
      if (d < best) { best = d; besti = base + v; }
    }
  }
#pragma unroll
  for (int m = 1; m < kLanes; m <<= 1) {                           // butterfly inside the group: every lane ends with the minimum
    const float od = __shfl_xor(best, m, 64);
    const int oi = __shfl_xor(besti, m, 64);
    if (od < best || (od == best && oi < besti)) { best = od; besti = oi; }
  }
  if (!valid || sub != 0) return;
  const int vi = besti == kNoVertex ? 0 : besti;                   // no candidate below +inf: index 0, as mf_knn1
  if (p.dist) p.dist[q] = sqrtf(best);
  if (p.ind) p.ind[q] = vi;
  p.inside[q] = sqrtf(best) < p.thickness ? 1 : 0;                 // strict, moco_flow_dataset.py:123
  const float* T = p.trans + (long long)vi * 16;
  float* o = p.pairs + q * 6;
  o[0] = qx; o[1] = qy; o[2] = qz;
#pragma unroll
  for (int r = 0; r < 3; ++r) {                                    // mf_apply_vertex_transforms' expression
    float acc = T[r * 4] * qx;
    acc = __builtin_fmaf(T[r * 4 + 1], qy, acc);
    acc = __builtin_fmaf(T[r * 4 + 2], qz, acc);
    o[3 + r] = acc + T[r * 4 + 3];
  }
}

// ---- the three point losses ----
constexpr int kPtLossThreads = 256;
constexpr int kPtLossMaxBlocks = 256;
constexpr int kPtLossSlots = 5;                     // sum |bw - cano|, sum |fw - query|, sum bce, rows taken by L1, outside rows

inline int point_loss_blocks(long long Q) { return (int)capped_blocks(Q, kPtLossThreads, kPtLossMaxBlocks); }

struct PointLossParams {
  long long Q;
  const float* pairs; const unsigned char* inside; int use_all;
  const float* pred_bw; const float* pred_fw;
  int n_nerfs; const float* sigma[2]; float delta[2];
  double* scratch; double* out6; float* means3;
  // backward
  const float* seeds3; float* g_bw; float* g_fw; float* g_sigma[2];
};

__global__ __launch_bounds__(kPtLossThreads) void point_loss_partials_kernel(const PointLossParams p) {
  double acc[kPtLossSlots];
#pragma unroll
  for (int k = 0; k < kPtLossSlots; ++k) acc[k] = 0.0;
  const long long nth = (long long)gridDim.x * kPtLossThreads;
  for (long long i = (long long)blockIdx.x * kPtLossThreads + threadIdx.x; i < p.Q; i += nth) {
    const bool in = p.inside ? p.inside[i] != 0 : true;
    const bool l1 = in || p.use_all;
    if (l1) {
      acc[3] += 1.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (p.pred_bw) acc[0] += (double)fabsf(p.pred_bw[i * 3 + c] - p.pairs[i * 6 + 3 + c]);
        if (p.pred_fw) acc[1] += (double)fabsf(p.pred_fw[i * 3 + c] - p.pairs[i * 6 + c]);
      }
    }
    if (!in) {
      acc[4] += 1.0;
      for (int k = 0; k < p.n_nerfs; ++k) {
        const float sp = softplus_torch(p.sigma[k][i]);
        const float alpha = 1.f - expf(-p.delta[k] * sp);                 // trainer_moco_flow.py:154
        const float lg = logf(1.f - alpha);                              // nn.BCELoss against a zero target
        acc[2] += (double)(-(lg > -100.f ? lg : -100.f));
      }
    }
  }
  block_sum_d<kPtLossThreads, kPtLossSlots>(acc, p.scratch + (long long)blockIdx.x * kPtLossSlots);
}

// one workgroup gathers the blocks' partials (thread b: block b's; none when Q = 0), then the pairs and the means
__global__ __launch_bounds__(kPtLossMaxBlocks) void point_loss_finish_kernel(const PointLossParams p, int n_blocks) {
  __shared__ double tot[kPtLossSlots];
  gather_sum_d<kPtLossMaxBlocks, kPtLossSlots>(p.scratch, n_blocks, tot);
  __syncthreads();
  if (threadIdx.x == 0) {
    p.out6[0] = p.pred_bw ? tot[0] : 0.0; p.out6[1] = p.pred_bw ? 3.0 * tot[3] : 0.0;
    p.out6[2] = p.pred_fw ? tot[1] : 0.0; p.out6[3] = p.pred_fw ? 3.0 * tot[3] : 0.0;
    p.out6[4] = tot[2];                   p.out6[5] = tot[4] * (double)p.n_nerfs;        // the length of torch.cat at :359
    if (p.means3)
      for (int k = 0; k < 3; ++k) p.means3[k] = p.out6[2 * k + 1] > 0.0 ? (float)(p.out6[2 * k] / p.out6[2 * k + 1]) : 0.f;
  }
}

__global__ __launch_bounds__(kPtLossThreads) void point_loss_backward_kernel(const PointLossParams p) {
  const long long i = (long long)blockIdx.x * kPtLossThreads + threadIdx.x;
  if (i >= p.Q) return;
  const bool in = p.inside ? p.inside[i] != 0 : true;
  const bool l1 = in || p.use_all;
  // Every step below is rounded where torch's own backward kernels round it, so a seed is bit-identical to the one the
  // compacted path gets.  A mean's backward divides by a count as torch divides a tensor by a host scalar: it multiplies by
  // the rounded reciprocal.
  // nn.L1Loss: seed / count, times sign(pred - target) (sign(0) = 0); an empty term has zero gradients
  const float cb = (float)p.out6[1], cf = (float)p.out6[3], cm = (float)p.out6[5];
  if (p.g_bw) {
    const float g = cb > 0.f ? p.seeds3[0] * (1.f / cb) : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = p.pred_bw[i * 3 + c] - p.pairs[i * 6 + 3 + c];
      p.g_bw[i * 3 + c] = l1 ? (d > 0.f ? g : (d < 0.f ? -g : 0.f)) : 0.f;
    }
  }
  if (p.g_fw) {
    const float g = cf > 0.f ? p.seeds3[1] * (1.f / cf) : 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = p.pred_fw[i * 3 + c] - p.pairs[i * 6 + c];
      p.g_fw[i * 3 + c] = l1 ? (d > 0.f ? g : (d < 0.f ? -g : 0.f)) : 0.f;
    }
  }
  for (int k = 0; k < p.n_nerfs; ++k) {
    if (!p.g_sigma[k]) continue;
    float g = 0.f;
    if (!in && cm > 0.f) {
      const float s = p.sigma[k][i];
      const float sp = softplus_torch(s);
      const float e = expf(-p.delta[k] * sp);
      const float alpha = 1.f - e;
      const float den = (1.f - alpha) * alpha;
      const float g_elem = p.seeds3[2] * alpha / (den > 1e-12f ? den : 1e-12f);           // binary_cross_entropy_backward ...
      const float g_alpha = g_elem * (1.f / cm);                                          // ... then div_(numel) for the mean
      const float g_sp = g_alpha * e * p.delta[k];                                        // 1 - exp(-delta sp)
      const float z = expf(s);
      g = s > 20.f ? g_sp : g_sp * z / (z + 1.f);                                         // softplus_backward: (a z) / (z + 1)
    }
    p.g_sigma[k][i] = g;
  }
}

}  // namespace mf

using namespace mf;

extern "C" int32_t mf_point_correspond(const float* verts, const float* trans, int64_t V, const float* query, int64_t q_given,
                                       const int64_t* pick, const float* noise, int64_t q_near, float thickness,
                                       int32_t lanes_per_query, float* pairs, uint8_t* inside, float* dist, int64_t* ind, void* stream) {
  if (V < 1 || V >= kNoVertex || q_given < 0 || q_near < 0)
    return fail(MF_E_INVALID, "mf_point_correspond: V=%lld q_given=%lld q_near=%lld", (long long)V, (long long)q_given, (long long)q_near);
  int T = lanes_per_query;
  if (T != 0 && T != 1 && T != 4 && T != 16 && T != 64)
    return fail(MF_E_INVALID, "mf_point_correspond: lanes_per_query=%d (0 = automatic, 1, 4, 16 or 64)", T);
  const long long Q = (long long)q_given + q_near;
  if (Q > (1LL << 31) - 1) return fail(MF_E_INVALID, "mf_point_correspond: %lld queries, at most 2^31 - 1", Q);
  if (Q == 0) return MF_OK;
  if (!verts || !trans || !pairs || !inside) return fail(MF_E_INVALID, "mf_point_correspond: null verts, trans, pairs or inside");
  if (q_given > 0 && !query) return fail(MF_E_INVALID, "mf_point_correspond: null query");
  if (q_near > 0 && (!pick || !noise)) return fail(MF_E_INVALID, "mf_point_correspond: null pick or noise");
  if (T == 0) {
    // the fewest lanes per query that still give every SIMD two waves (4 SIMDs per CU); 64 when even that does not
    const long long want = 8LL * device_cus();
    T = 64;
    for (int t = 16; t >= 1; t /= 4)
      if (Q * t >= want * 64) T = t;
  }
  CorrespondParams p{verts, trans, (int)V, query, q_given, reinterpret_cast<const long long*>(pick), noise, q_near, thickness,
                     pairs, inside, dist, reinterpret_cast<long long*>(ind)};
  const long long per = kCorrThreads / T;
  const dim3 grid((unsigned)((Q + per - 1) / per)), block(kCorrThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (T) {
    case 1: hipLaunchKernelGGL(point_correspond_kernel<1>, grid, block, 0, s, p); break;
    case 4: hipLaunchKernelGGL(point_correspond_kernel<4>, grid, block, 0, s, p); break;
    case 16: hipLaunchKernelGGL(point_correspond_kernel<16>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(point_correspond_kernel<64>, grid, block, 0, s, p); break;
  }
  return check_launch("mf_point_correspond");
}

extern "C" int64_t mf_point_loss_partials_scratch_bytes(int64_t Q) {
  if (Q < 0) { fail(MF_E_INVALID, "mf_point_loss_partials_scratch_bytes: negative Q=%lld", (long long)Q); return -1; }
  return (int64_t)point_loss_blocks(Q) * kPtLossSlots * sizeof(double);
}

static int point_loss_params(const char* what, const mf_point_loss_args* a, PointLossParams& p) {
  if (!a) return fail(MF_E_INVALID, "%s: args is null", what);
  if (a->Q < 0) return fail(MF_E_INVALID, "%s: negative Q=%lld", what, (long long)a->Q);
  if (a->n_nerfs < 0 || a->n_nerfs > 2) return fail(MF_E_INVALID, "%s: n_nerfs=%d (at most 2)", what, a->n_nerfs);
  p.Q = a->Q; p.pairs = a->pairs; p.inside = a->inside; p.use_all = a->use_all != 0;
  p.pred_bw = a->pred_bw; p.pred_fw = a->pred_fw; p.n_nerfs = a->n_nerfs;
  for (int k = 0; k < a->n_nerfs; ++k) { p.sigma[k] = a->sigma[k]; p.delta[k] = a->delta[k]; }
  if (a->Q == 0) return MF_OK;
  if (!a->pairs) return fail(MF_E_INVALID, "%s: null pairs", what);
  for (int k = 0; k < a->n_nerfs; ++k)
    if (!a->sigma[k]) return fail(MF_E_INVALID, "%s: null sigma[%d]", what, k);
  return MF_OK;
}

extern "C" int32_t mf_point_loss_partials(const mf_point_loss_args* a, double* out6, float* means3, void* scratch, void* stream) {
  PointLossParams p{};
  if (int rc = point_loss_params("mf_point_loss_partials", a, p)) return rc;
  if (!out6) return fail(MF_E_INVALID, "mf_point_loss_partials: null out6");
  if (a->Q > 0 && !scratch) return fail(MF_E_INVALID, "mf_point_loss_partials: null scratch");
  p.scratch = static_cast<double*>(scratch); p.out6 = out6; p.means3 = means3;
  const int blocks = point_loss_blocks(a->Q);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (blocks > 0) hipLaunchKernelGGL(point_loss_partials_kernel, dim3(blocks), dim3(kPtLossThreads), 0, s, p);
  hipLaunchKernelGGL(point_loss_finish_kernel, dim3(1), dim3(kPtLossMaxBlocks), 0, s, p, blocks);
  return check_launch("mf_point_loss_partials");
}

extern "C" int32_t mf_point_loss_partials_backward(const mf_point_loss_args* a, const double* out6, const float* seeds3, float* g_pred_bw,
                                                   float* g_pred_fw, float* g_sigma0, float* g_sigma1, void* stream) {
  PointLossParams p{};
  if (int rc = point_loss_params("mf_point_loss_partials_backward", a, p)) return rc;
  if (!out6 || !seeds3) return fail(MF_E_INVALID, "mf_point_loss_partials_backward: null out6 or seeds3");
  if ((g_pred_bw && !a->pred_bw) || (g_pred_fw && !a->pred_fw))
    return fail(MF_E_INVALID, "mf_point_loss_partials_backward: a gradient without its prediction");
  if ((g_sigma0 && a->n_nerfs < 1) || (g_sigma1 && a->n_nerfs < 2))
    return fail(MF_E_INVALID, "mf_point_loss_partials_backward: a sigma gradient beyond n_nerfs=%d", a->n_nerfs);
  if (a->Q == 0) return MF_OK;
  if (a->Q > (1LL << 31) - 1) return fail(MF_E_INVALID, "mf_point_loss_partials_backward: Q=%lld, at most 2^31 - 1", (long long)a->Q);
  p.out6 = const_cast<double*>(out6); p.seeds3 = seeds3; p.g_bw = g_pred_bw; p.g_fw = g_pred_fw;
  p.g_sigma[0] = g_sigma0; p.g_sigma[1] = g_sigma1;
  hipLaunchKernelGGL(point_loss_backward_kernel, dim3((unsigned)((a->Q + kPtLossThreads - 1) / kPtLossThreads)), dim3(kPtLossThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  return check_launch("mf_point_loss_partials_backward");
}
