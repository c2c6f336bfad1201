// mf_frames.hip -- frame ingest on the device: from decoded 8-bit frames to the tensors the training step, the metrics and the
// sheets take (include/mocoflow_hip.h):
//   mf_resize_u8         T.Resize on the PIL image: PIL's antialiased bilinear resample     datasets/moco_flow_dataset.py:51-55, 169
//   mf_composite_rows    img[:3] * a + bkgd * (1 - a) over the whole frame                  datasets/moco_flow_dataset.py:174-176
//   mf_background_plate  np.sort(img / 255. * (1 - msk / 255.), axis=0)[k]                  scripts/data_utils.py:150-163
// The resize and the plate are integer arithmetic on bytes, the composite is fp32 with one rounding per operation (mf_pixels.hpp):
// every result is pinned bit for bit.  No atomics anywhere; every output byte is written by one lane with a plain store.
#include "mf_host.hpp"
#include "mf_pixels.hpp"

namespace mf {

// ---- resize: PIL's ImagingResampleHorizontal_8bpc / Vertical_8bpc, one lane per output unit ----
constexpr int kResizeThreads = 256;                                       // one workgroup's share: 256 output units
constexpr int kResizePrecisionBits = 22;                                  // PIL's PRECISION_BITS = 32 - 8 - 2

// PIL's RGBA -> RGBa (MULDIV255) and RGBa -> RGBA
__device__ __forceinline__ int premultiply(int c, int a) {
  const int t = c * a + 128;
  return (t + (t >> 8)) >> 8;
}
__device__ __forceinline__ int unpremultiply(int c, int a) {
  if (a == 0 || a == 255) return c;
  const int v = 255 * c / a;
  return v > 255 ? 255 : v;
}
__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> kResizePrecisionBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// a unit of kN bytes: with kPre / kUnpre a pixel whose last byte is its alpha (kN = 4), otherwise kN independent bytes
template <int kN, bool kPre>
__device__ __forceinline__ void tap_add(int (&acc)[kN], const uint8_t* src, int w) {
  int v[kN];
  if constexpr (kN == 4) {
    const unsigned px = *reinterpret_cast<const unsigned*>(src);          // 4-byte aligned (checked by the entry point)
#pragma unroll
    for (int c = 0; c < kN; ++c) v[c] = (int)((px >> (8 * c)) & 0xffu);
  } else {
#pragma unroll
    for (int c = 0; c < kN; ++c) v[c] = src[c];
  }
  if (kPre) {
#pragma unroll
    for (int c = 0; c < kN - 1; ++c) v[c] = premultiply(v[c], v[kN - 1]);
  }
  // a byte times a coefficient of at most 2^22 + 1: the 24-bit multiply-add, one full-rate instruction per channel.  (Written as
  // v[c] * w, hipcc (ROCm 7.2) took v_mad_u64_u32 for it, and the vertical pass over four independent bytes returned a wrong
  // fourth byte on the MI355X -- the one channel whose 64-bit destination pair also held the coefficient.  The cause is not
  // established; tests/test_gpu_frames.py::test_resize_equals_pil[dot_up_l] is the case that showed it.)
#pragma unroll
  for (int c = 0; c < kN; ++c) acc[c] += (int)__umul24((unsigned)v[c], (unsigned)w);
}

template <int kN, bool kUnpre>
__device__ __forceinline__ void unit_store(uint8_t* dst, const int (&acc)[kN]) {
  int v[kN];
#pragma unroll
  for (int c = 0; c < kN; ++c) v[c] = clip8(acc[c]);
  if (kUnpre) {
#pragma unroll
    for (int c = 0; c < kN - 1; ++c) v[c] = unpremultiply(v[c], v[kN - 1]);
  }
  if constexpr (kN == 4) {
    *reinterpret_cast<unsigned*>(dst) = (unsigned)v[0] | (unsigned)v[1] << 8 | (unsigned)v[2] << 16 | (unsigned)v[3] << 24;
  } else {
#pragma unroll
    for (int c = 0; c < kN; ++c) dst[c] = (uint8_t)v[c];
  }
}

struct ResizePassParams {
  const uint8_t* in;
  uint8_t* out;
  const int32_t* bounds;         // (n_out, 2): first tap, tap count
  const int32_t* kk;             // (n_out, ksize)
  int32_t ksize;
  int32_t n_in, n_out;           // the axis being resampled
  int32_t units;                 // vertical pass: units per row; horizontal pass: unused
  int32_t total;                 // output units of the pass, < 2^31
};

// the taps of output index o, clamped to the axis: a table entry never forms an address outside the image
__device__ __forceinline__ void taps_of(const ResizePassParams& p, int o, int& first, int& n) {
  first = p.bounds[2 * o];
  n = p.bounds[2 * o + 1];
  first = first < 0 ? 0 : (first > p.n_in ? p.n_in : first);
  n = n > p.ksize ? p.ksize : n;
  n = n > p.n_in - first ? p.n_in - first : n;
}

// horizontal: rows of n_in pixels of kC bytes -> rows of n_out pixels; unit i = pixel (row i / n_out, column i % n_out)
template <int kC, bool kPre, bool kUnpre>
__global__ __launch_bounds__(kResizeThreads) void resize_horizontal_kernel(const ResizePassParams p) {
  const int i = blockIdx.x * kResizeThreads + threadIdx.x;
  if (i >= p.total) return;
  const int row = i / p.n_out, x = i - row * p.n_out;
  int first, n;
  taps_of(p, x, first, n);
  const uint8_t* src = p.in + ((size_t)row * p.n_in + first) * kC;
  const int32_t* k = p.kk + (size_t)x * p.ksize;
  int acc[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) acc[c] = 1 << (kResizePrecisionBits - 1);
  for (int t = 0; t < n; ++t) tap_add<kC, kPre>(acc, src + (size_t)t * kC, k[t]);
  unit_store<kC, kUnpre>(p.out + (size_t)i * kC, acc);
}

// vertical: frames of n_in rows of `units` units of kN bytes -> frames of n_out rows; consecutive lanes read consecutive units
template <int kN, bool kPre, bool kUnpre>
__global__ __launch_bounds__(kResizeThreads) void resize_vertical_kernel(const ResizePassParams p) {
  const int i = blockIdx.x * kResizeThreads + threadIdx.x;
  if (i >= p.total) return;
  const int r = i / p.units, u = i - r * p.units;                         // r: output row over all frames
  const int f = r / p.n_out, y = r - f * p.n_out;
  int first, n;
  taps_of(p, y, first, n);
  const size_t pitch = (size_t)p.units * kN;
  const uint8_t* src = p.in + ((size_t)f * p.n_in + first) * pitch + (size_t)u * kN;
  const int32_t* k = p.kk + (size_t)y * p.ksize;
  int acc[kN];
#pragma unroll
  for (int c = 0; c < kN; ++c) acc[c] = 1 << (kResizePrecisionBits - 1);
  for (int t = 0; t < n; ++t) tap_add<kN, kPre>(acc, src + (size_t)t * pitch, k[t]);
  unit_store<kN, kUnpre>(p.out + (size_t)i * kN, acc);
}

template <class K>
inline void launch_resize(K kern, const ResizePassParams& p, hipStream_t s) {
  hipLaunchKernelGGL(kern, dim3((unsigned)((p.total + kResizeThreads - 1) / kResizeThreads)), dim3(kResizeThreads), 0, s, p);
}

// ---- composite: a lane owns four consecutive pixels ----
constexpr int kCompositeThreads = 256;
constexpr int kCompositePerThread = 4;                                    // one workgroup's share: 1024 pixels

struct CompositeParams {
  const void* image;
  const void* background;
  float* rows;
  int32_t n;                     // H W, 4 n < 2^31
  int32_t background_kind;
  int32_t vec;                   // every pointer in use is 16-byte aligned: whole lanes move in 12- and 16-byte pieces
};

template <bool kRgba>
__global__ __launch_bounds__(kCompositeThreads) void composite_rows_kernel(const CompositeParams p) {
  const int p0 = (blockIdx.x * kCompositeThreads + threadIdx.x) * kCompositePerThread;
  if (p0 >= p.n) return;
  const int cnt = p.n - p0 < kCompositePerThread ? p.n - p0 : kCompositePerThread;
  const bool whole = cnt == kCompositePerThread && p.vec;
  float o[kCompositePerThread * 3];
  if (!kRgba) {
    const uint8_t* im = static_cast<const uint8_t*>(p.image) + (size_t)p0 * 3;
    if (whole) {                                                           // 12 bytes, 4-byte aligned (p0 is a multiple of 4)
      const unsigned* w = reinterpret_cast<const unsigned*>(im);
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        const unsigned x = w[m];
#pragma unroll
        for (int b = 0; b < 4; ++b) o[4 * m + b] = u8_unit((x >> (8 * b)) & 0xffu);
      }
    } else {
#pragma unroll
      for (int e = 0; e < kCompositePerThread * 3; ++e) o[e] = e < cnt * 3 ? u8_unit(im[e]) : 0.f;
    }
  } else {
    unsigned px[kCompositePerThread];
    float bg[kCompositePerThread * 3];
    const unsigned* im = static_cast<const unsigned*>(p.image) + p0;
    if (whole) {
      const uint4 q = *reinterpret_cast<const uint4*>(im);
      px[0] = q.x; px[1] = q.y; px[2] = q.z; px[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < kCompositePerThread; ++j) px[j] = j < cnt ? im[j] : 0u;
    }
    if (p.background_kind == MF_BACKGROUND_COLOUR) {
      const float* b = static_cast<const float*>(p.background);
#pragma unroll
      for (int e = 0; e < kCompositePerThread * 3; ++e) bg[e] = b[e % 3];
    } else if (p.background_kind == MF_BACKGROUND_ROWS) {
      const float* b = static_cast<const float*>(p.background) + (size_t)p0 * 3;
      if (whole) {
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const float4 v = reinterpret_cast<const float4*>(b)[m];
          bg[4 * m] = v.x; bg[4 * m + 1] = v.y; bg[4 * m + 2] = v.z; bg[4 * m + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < kCompositePerThread * 3; ++e) bg[e] = e < cnt * 3 ? b[e] : 0.f;
      }
    } else {                                                               // MF_BACKGROUND_U8
      const uint8_t* b = static_cast<const uint8_t*>(p.background) + (size_t)p0 * 3;
      if (whole) {
        const unsigned* w = reinterpret_cast<const unsigned*>(b);
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const unsigned x = w[m];
#pragma unroll
          for (int k = 0; k < 4; ++k) bg[4 * m + k] = u8_unit((x >> (8 * k)) & 0xffu);
        }
      } else {
#pragma unroll
        for (int e = 0; e < kCompositePerThread * 3; ++e) bg[e] = e < cnt * 3 ? u8_unit(b[e]) : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < kCompositePerThread; ++j) {
      const float b3[3] = {bg[3 * j], bg[3 * j + 1], bg[3 * j + 2]};
      float rgb[3];
      composite_u8_rgba(px[j], b3, rgb);
      o[3 * j] = rgb[0]; o[3 * j + 1] = rgb[1]; o[3 * j + 2] = rgb[2];
    }
  }
  float* out = p.rows + (size_t)p0 * 3;
  if (whole) {
#pragma unroll
    for (int m = 0; m < 3; ++m) reinterpret_cast<float4*>(out)[m] = make_float4(o[4 * m], o[4 * m + 1], o[4 * m + 2], o[4 * m + 3]);
  } else {
#pragma unroll
    for (int e = 0; e < kCompositePerThread * 3; ++e)
      if (e < cnt * 3) out[e] = o[e];
  }
}

// ---- background plate: the k-th smallest 16-bit key u (255 - m) over the frames, per pixel and channel ----
// An element e = 3 pixel + channel is one output byte.  The k-th smallest key is the largest v with #(key < v) <= k, built
// from its top bit down: 16 counting steps.
constexpr int kPlateThreads = 256;                                        // streamed: one lane per element
constexpr int kPlateStagedThreads = 1024;                                 // staged: 16 waves load the tile, 3 of them select
constexpr int kPlateTilePixels = 64;                                      // one staged workgroup's share: 64 pixels = 192 elements
constexpr int kPlateTileElems = kPlateTilePixels * 3;
constexpr int kPlateGroup = 4;                                            // keys of 4 frames side by side: one 8-byte LDS read
// F up to here is staged: 192 elements x 424 frames x 2 bytes = 159 KiB of the CU's 160 KiB of LDS.  Beyond it: streamed.
constexpr int kPlateLdsMaxFrames = 424;
constexpr int kPlateKeyBits = 16;                                         // 255 * 255 = 65025 < 2^16
constexpr unsigned kPlatePadKey = 0xffffu;                                // above every key: never counted

struct PlateParams {
  const uint8_t* frames;
  const uint8_t* masks;
  uint8_t* out;
  int32_t F, k;
  int32_t n;                     // H W, 4 n < 2^31
};

__device__ __forceinline__ unsigned plate_key(const uint8_t* frame_byte, const uint8_t* mask_byte) {
  return (unsigned)*frame_byte * (255u - (unsigned)*mask_byte);
}
__device__ __forceinline__ uint8_t plate_byte(unsigned key) { return (uint8_t)((key + 127u) / 255u); }

// two 16-bit keys side by side, counted side by side in three packed instructions: with t >= 1, sat(min(key, t) - (t - 1)) is 1
// where key >= t and 0 where key < t (as a comparison per half hipcc takes six instructions)
typedef unsigned short plate_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ plate_u16x2 plate_not_below(unsigned two_keys, plate_u16x2 t, plate_u16x2 t_less_1) {
  return __builtin_elementwise_sub_sat(__builtin_elementwise_min(__builtin_bit_cast(plate_u16x2, two_keys), t), t_less_1);
}

// staged: the tile's keys go to LDS as [frame group][element][4 frames]; wave w loads the groups w, w + 16, ..: lane l takes the
// elements l, l + 64, l + 128 -- consecutive lanes, consecutive bytes of the frame -- with the 24 loads of a group in flight
// together and 16 waves side by side (a workgroup with F = 300 fills most of the CU's LDS: what hides the memory latency is
// inside it).  Then each of the first 192 lanes selects its element from LDS alone, one 8-byte read per four frames.
template <int kC>
__global__ __launch_bounds__(kPlateStagedThreads) void plate_staged_kernel(const PlateParams p) {
  extern __shared__ __align__(16) unsigned char plate_lds[];
  uint2* keys = reinterpret_cast<uint2*>(plate_lds);                       // [(F + 3) / 4][kPlateTileElems]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e_lo = blockIdx.x * kPlateTileElems, e_hi = 3 * p.n;           // this tile's first element, the frame's last + 1
  const int groups = (p.F + kPlateGroup - 1) / kPlateGroup;
  const size_t frame_bytes = (size_t)p.n * kC;
  for (int g = wave; g < groups; g += kPlateStagedThreads / 64) {
    unsigned key[3][kPlateGroup];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = e_lo + lane + 64 * i;
      const int pix = e / 3, off = pix * kC + (e - pix * 3);
#pragma unroll
      for (int j = 0; j < kPlateGroup; ++j) {
        const int f = g * kPlateGroup + j;
        key[i][j] = kPlatePadKey;
        if (f < p.F && e < e_hi) key[i][j] = plate_key(p.frames + (size_t)f * frame_bytes + off, p.masks + (size_t)f * p.n + pix);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
      keys[g * kPlateTileElems + lane + 64 * i] = make_uint2(key[i][0] | key[i][1] << 16, key[i][2] | key[i][3] << 16);
  }
  __syncthreads();
  const int el = threadIdx.x, e = e_lo + el;
  if (el >= kPlateTileElems || e >= e_hi) return;
  unsigned v = 0;
#pragma unroll 1
  for (int bit = kPlateKeyBits - 1; bit >= 0; --bit) {
    const unsigned t = v | (1u << bit);
    const plate_u16x2 tt = {(unsigned short)t, (unsigned short)t}, tl = {(unsigned short)(t - 1), (unsigned short)(t - 1)};
    plate_u16x2 rest = {0, 0};                                             // keys >= t, the padding among them: <= 2 groups per half
    for (int g = 0; g < groups; ++g) {
      const uint2 q = keys[g * kPlateTileElems + el];
      rest += plate_not_below(q.x, tt, tl) + plate_not_below(q.y, tt, tl);
    }
    if (kPlateGroup * groups - ((int)rest.x + (int)rest.y) <= p.k) v = t;
  }
  p.out[e] = plate_byte(v);
}

// streamed: a lane owns an element and reads its byte of every frame once per counting step
template <int kC>
__global__ __launch_bounds__(kPlateThreads) void plate_streamed_kernel(const PlateParams p) {
  const int e = blockIdx.x * kPlateThreads + threadIdx.x;
  if (e >= 3 * p.n) return;
  const int pix = e / 3, off = pix * kC + (e - pix * 3);
  const size_t frame_bytes = (size_t)p.n * kC;
  unsigned v = 0;
#pragma unroll 1
  for (int bit = kPlateKeyBits - 1; bit >= 0; --bit) {
    const unsigned t = v | (1u << bit);
    int below = 0;
    const uint8_t* fb = p.frames + off;
    const uint8_t* mb = p.masks + pix;
#pragma unroll 4
    for (int f = 0; f < p.F; ++f, fb += frame_bytes, mb += p.n) below += plate_key(fb, mb) < t;
    if (below <= p.k) v = t;
  }
  p.out[e] = plate_byte(v);
}

inline size_t plate_lds_bytes(int F) { return (size_t)((F + kPlateGroup - 1) / kPlateGroup) * kPlateTileElems * sizeof(uint2); }

inline bool resize_sizes_ok(int64_t F, int64_t H0, int64_t W0, int32_t C, int64_t H, int64_t W) {
  return F >= 0 && H0 >= 0 && W0 >= 0 && H >= 0 && W >= 0 && (C == 1 || C == 3 || C == 4);
}
// a b c d without overflow: false once the product reaches 2^31
inline bool below_2_31(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t cap = (int64_t)1 << 31;
  int64_t v = 1;
  for (int64_t x : {a, b, c, d}) {
    if (x == 0) return true;
    if (v > (cap - 1) / x) return false;
    v *= x;
  }
  return v < cap;
}

}  // namespace mf

using namespace mf;

extern "C" int64_t mf_resize_u8_scratch_bytes(int64_t F, int64_t H0, int64_t W0, int32_t C, int64_t H, int64_t W) {
  if (!resize_sizes_ok(F, H0, W0, C, H, W))
    return fail(MF_E_INVALID, "mf_resize_u8_scratch_bytes: F=%lld (%lld, %lld) -> (%lld, %lld), C=%d; sizes >= 0 and C in {1, 3, 4}",
                (long long)F, (long long)H0, (long long)W0, (long long)H, (long long)W, C);
  if (H0 == H || W0 == W) return 0;
  if (!below_2_31(F, H0, W, C)) return fail(MF_E_INVALID, "mf_resize_u8_scratch_bytes: the intermediate needs 32-bit indexing, F H0 W C < 2^31");
  return F * H0 * W * C;
}

extern "C" int32_t mf_resize_u8(const uint8_t* in, int64_t F, int64_t H0, int64_t W0, int32_t C, int64_t H, int64_t W,
                                const int32_t* xbounds, const int32_t* xkk, int32_t xksize,
                                const int32_t* ybounds, const int32_t* ykk, int32_t yksize, uint8_t* out, void* scratch, void* stream) {
  if (!resize_sizes_ok(F, H0, W0, C, H, W))
    return fail(MF_E_INVALID, "mf_resize_u8: F=%lld (%lld, %lld) -> (%lld, %lld), C=%d; sizes >= 0 and C in {1, 3, 4}",
                (long long)F, (long long)H0, (long long)W0, (long long)H, (long long)W, C);
  if (!below_2_31(F, H0, W0, C) || !below_2_31(F, H0, W, C) || !below_2_31(F, H, W, C))
    return fail(MF_E_INVALID, "mf_resize_u8: F=%lld (%lld, %lld) -> (%lld, %lld), C=%d: 32-bit indexing needs F H0 W0 C, F H0 W C and "
                "F H W C < 2^31", (long long)F, (long long)H0, (long long)W0, (long long)H, (long long)W, C);
  if (F * H * W == 0) return MF_OK;
  if (H0 == 0 || W0 == 0) return fail(MF_E_INVALID, "mf_resize_u8: an empty (%lld, %lld) input cannot fill a (%lld, %lld) output",
                                      (long long)H0, (long long)W0, (long long)H, (long long)W);
  if (!in || !out) return fail(MF_E_INVALID, "mf_resize_u8: null in or out");
  const bool horizontal = W != W0, vertical = H != H0;
  if (horizontal && (!xbounds || !xkk || xksize < 1)) return fail(MF_E_INVALID, "mf_resize_u8: the width changes: xbounds, xkk and xksize >= 1 are needed");
  if (vertical && (!ybounds || !ykk || yksize < 1)) return fail(MF_E_INVALID, "mf_resize_u8: the height changes: ybounds, ykk and yksize >= 1 are needed");
  if (horizontal && vertical && !scratch) return fail(MF_E_INVALID, "mf_resize_u8: both axes change: scratch is needed");
  if (C == 4 && (!is_aligned(in, 4) || !is_aligned(out, 4) || (horizontal && vertical && !is_aligned(scratch, 4))))
    return fail(MF_E_INVALID, "mf_resize_u8: RGBA in, out and scratch must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!horizontal && !vertical) {
    if (hipMemcpyAsync(out, in, (size_t)(F * H * W * C), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(MF_E_LAUNCH, "mf_resize_u8: hipMemcpyAsync failed");
    return MF_OK;
  }
  uint8_t* mid = horizontal && vertical ? static_cast<uint8_t*>(scratch) : out;
  if (horizontal) {
    ResizePassParams p{in, mid, xbounds, xkk, xksize, (int32_t)W0, (int32_t)W, 0, (int32_t)(F * H0 * W)};
    if (C == 1) launch_resize(resize_horizontal_kernel<1, false, false>, p, s);
    else if (C == 3) launch_resize(resize_horizontal_kernel<3, false, false>, p, s);
    else if (vertical) launch_resize(resize_horizontal_kernel<4, true, false>, p, s);
    else launch_resize(resize_horizontal_kernel<4, true, true>, p, s);
  }
  if (vertical) {
    const uint8_t* src = horizontal ? mid : in;
    const int64_t row_bytes = W * C;
    ResizePassParams p{src, out, ybounds, ykk, yksize, (int32_t)H0, (int32_t)H, 0, 0};
    if (C == 4) {
      p.units = (int32_t)W;
      p.total = (int32_t)(F * H * W);
      if (horizontal) launch_resize(resize_vertical_kernel<4, false, true>, p, s);
      else launch_resize(resize_vertical_kernel<4, true, true>, p, s);
    } else if (row_bytes % 4 == 0 && is_aligned(src, 4) && is_aligned(out, 4)) {   // channels are independent: four bytes a lane
      p.units = (int32_t)(row_bytes / 4);
      p.total = (int32_t)(F * H * (row_bytes / 4));
      launch_resize(resize_vertical_kernel<4, false, false>, p, s);
    } else {
      p.units = (int32_t)row_bytes;
      p.total = (int32_t)(F * H * row_bytes);
      launch_resize(resize_vertical_kernel<1, false, false>, p, s);
    }
  }
  return check_launch("mf_resize_u8");
}

extern "C" int32_t mf_composite_rows(const void* image, int32_t image_kind, int64_t H, int64_t W, const void* background,
                                     int32_t background_kind, float* rows_out, void* stream) {
  if (H < 0 || W < 0) return fail(MF_E_INVALID, "mf_composite_rows: negative size (H=%lld W=%lld)", (long long)H, (long long)W);
  if (!below_2_31(H, W, 4, 1)) return fail(MF_E_INVALID, "mf_composite_rows: H=%lld W=%lld, 32-bit indexing needs 4 H W < 2^31", (long long)H, (long long)W);
  if (image_kind != MF_IMAGE_U8_RGB && image_kind != MF_IMAGE_U8_RGBA)
    return fail(MF_E_INVALID, "mf_composite_rows: image_kind=%d; MF_IMAGE_U8_RGB or MF_IMAGE_U8_RGBA", image_kind);
  const bool rgba = image_kind == MF_IMAGE_U8_RGBA;
  if (rgba && background_kind != MF_BACKGROUND_ROWS && background_kind != MF_BACKGROUND_COLOUR && background_kind != MF_BACKGROUND_U8)
    return fail(MF_E_INVALID, "mf_composite_rows: background_kind=%d; an RGBA image needs a background to composite over", background_kind);
  if (!rgba && background_kind != MF_BACKGROUND_NONE)
    return fail(MF_E_INVALID, "mf_composite_rows: background_kind=%d; an RGB image takes no background", background_kind);
  const int64_t n = H * W;
  if (n == 0) return MF_OK;
  if (!image || !rows_out) return fail(MF_E_INVALID, "mf_composite_rows: null image or rows_out");
  if (rgba && !background) return fail(MF_E_INVALID, "mf_composite_rows: null background");
  if (rgba && !is_aligned(image, 4)) return fail(MF_E_INVALID, "mf_composite_rows: an RGBA image must be 4-byte aligned");
  CompositeParams p{image, background, rows_out, (int32_t)n, background_kind, 0};
  p.vec = is_aligned(image, 16) && is_aligned(rows_out, 16) && (!rgba || background_kind == MF_BACKGROUND_COLOUR || is_aligned(background, 16));
  const int per = kCompositeThreads * kCompositePerThread;
  const dim3 grid((unsigned)((n + per - 1) / per)), block(kCompositeThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rgba) hipLaunchKernelGGL(composite_rows_kernel<true>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(composite_rows_kernel<false>, grid, block, 0, s, p);
  return check_launch("mf_composite_rows");
}

extern "C" int32_t mf_background_plate(const uint8_t* frames, const uint8_t* masks, int64_t F, int64_t H, int64_t W, int32_t C, int64_t k,
                                       int32_t path, uint8_t* out, void* stream) {
  if (H < 0 || W < 0 || (C != 3 && C != 4))
    return fail(MF_E_INVALID, "mf_background_plate: H=%lld W=%lld C=%d; sizes >= 0 and C in {3, 4}", (long long)H, (long long)W, C);
  if (F < 1 || F >= 65536) return fail(MF_E_INVALID, "mf_background_plate: F=%lld; 1 <= F < 65536", (long long)F);
  if (k < 0 || k >= F) return fail(MF_E_INVALID, "mf_background_plate: k=%lld; 0 <= k < F=%lld", (long long)k, (long long)F);
  if (!below_2_31(H, W, 4, 1)) return fail(MF_E_INVALID, "mf_background_plate: H=%lld W=%lld, 32-bit indexing needs 4 H W < 2^31", (long long)H, (long long)W);
  if (path != MF_PLATE_AUTO && path != MF_PLATE_STAGED && path != MF_PLATE_STREAMED) return fail(MF_E_INVALID, "mf_background_plate: path=%d", path);
  if (path == MF_PLATE_STAGED && F > kPlateLdsMaxFrames)
    return fail(MF_E_INVALID, "mf_background_plate: F=%lld frames cannot be staged, the LDS holds %d", (long long)F, kPlateLdsMaxFrames);
  const int64_t n = H * W;
  if (n == 0) return MF_OK;
  if (!frames || !masks || !out) return fail(MF_E_INVALID, "mf_background_plate: null frames, masks or out");
  const PlateParams p{frames, masks, out, (int32_t)F, (int32_t)k, (int32_t)n};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool staged = path == MF_PLATE_STAGED || (path == MF_PLATE_AUTO && F <= kPlateLdsMaxFrames);
  if (staged) {
    const unsigned grid = (unsigned)((n + kPlateTilePixels - 1) / kPlateTilePixels);
    const size_t lds = plate_lds_bytes((int)F);
    return launch_lds(C == 4 ? plate_staged_kernel<4> : plate_staged_kernel<3>, grid, kPlateStagedThreads, lds, s, p, "mf_background_plate",
                      "mf_background_plate (staged)", lds > 48 * 1024);
  }
  const dim3 grid((unsigned)((3 * n + kPlateThreads - 1) / kPlateThreads)), block(kPlateThreads);
  if (C == 4) hipLaunchKernelGGL(plate_streamed_kernel<4>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(plate_streamed_kernel<3>, grid, block, 0, s, p);
  return check_launch("mf_background_plate (streamed)");
}
