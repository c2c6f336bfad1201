// mf_f3.hpp -- three floats and the few operations on them that the fixed-arithmetic mesh units share (mf_mesh_distance.hip,
// mf_mesh_rays.hip).  Every operation is rounded once, in the order written: dot3(x, y) = (x0 y0 + x1 y1) + x2 y2.  The units that
// include this are built with -ffp-contract=off and say so themselves (#pragma clang fp contract(off)) before they include it.
#pragma once
#include <hip/hip_runtime.h>

namespace mf {

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 f3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ F3 sub3(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 add3(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 mul3(F3 a, float t) { return {a.x * t, a.y * t, a.z * t}; }
__device__ __forceinline__ bool finite3(F3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ F3 min3(F3 a, F3 b) { return {fminf(a.x, b.x), fminf(a.y, b.y), fminf(a.z, b.z)}; }
__device__ __forceinline__ F3 max3(F3 a, F3 b) { return {fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z)}; }

}  // namespace mf
