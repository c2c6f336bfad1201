// mf_pixels.hpp -- ONE 8-bit pixel to fp32, shared by mf_ray_batch (mf_batch.hip: the selected pixels of a training batch) and
// mf_composite_rows (mf_frames.hip: every pixel of a frame), so that a batch row is bit for bit the row of the full table.
//   ToTensor and img[:3] * a + bkgd * (1 - a)            datasets/moco_flow_dataset.py:169-176
// 8-bit compositing is the torch expression operation for operation: no fused multiply-add (the Makefile builds every unit
// with -ffp-contract=off; the pragma keeps it true for a build that forgets the flag)
#pragma once
#pragma clang fp contract(off)

// u8.float() / 255 as torch evaluates it ON THE DEVICE: a tensor divided by a host scalar is multiplied by the scalar's fp32
// reciprocal, one rounding for the reciprocal and one for the product.  For 126 of the 256 byte values that is one ulp from the
// fp32 quotient ToTensor computes on the host; the rows equal the eager device expression they replace, bit for bit.

namespace mf {

constexpr float kInv255 = 1.0f / 255.0f;                                  // rounded once, to fp32

__device__ __forceinline__ float u8_unit(unsigned u) { return (float)u * kInv255; }     // .float().div(255) on the device

// px = r | g << 8 | b << 16 | a << 24 over the background bg -> rgb
__device__ __forceinline__ void composite_u8_rgba(unsigned px, const float (&bg)[3], float (&rgb)[3]) {
  const float a = u8_unit(px >> 24);
  const float na = 1.f - a;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = u8_unit((px >> (8 * c)) & 0xffu);
    const float fg = v * a, back = bg[c] * na;                             // moco_flow_dataset.py:174, one rounding each
    rgb[c] = fg + back;
  }
}

}  // namespace mf
