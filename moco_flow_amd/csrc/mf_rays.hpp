// mf_rays.hpp -- the ray of ONE pixel, shared by mf_make_rays (mf_aux.hip: every pixel of a frame) and mf_ray_batch
// (mf_batch.hip: the selected pixels of a training batch), so that a batch row is bit for bit the row of the full table.
//   Camera.make_rays / gen_ray_directions / gen_rays   utils/camera.py:29-81, 134-148
// Units that include this are built with -ffp-contract=off: every product, sum and quotient below is rounded once.
#pragma once

namespace mf {

struct RayCam {
  int H, W;
  float fx, cx, cy;
  float R[9], t[3];
  int has_c2w;
  float nearv, farv, idx;
};

// c2w_host: the 3x4 row-major camera-to-world matrix, or null for camera coordinates
inline void ray_cam_set_c2w(RayCam& c, const float* c2w_host) {
  c.has_c2w = c2w_host != nullptr;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) c.R[a * 3 + b] = c2w_host ? c2w_host[a * 4 + b] : 0.f;
    c.t[a] = c2w_host ? c2w_host[a * 4 + 3] : 0.f;
  }
}

// pixel (row j, column i) -> o[0..8] = [origin, unit direction, near, far, idx]
__device__ __forceinline__ void pixel_ray(const RayCam& p, int j, int i, float (&o)[9]) {
  // camera.py:47-48: ((i - cx)/f0, -(j - cy)/f0, -1); both axes use focal[0]
  const float dx = ((float)i - p.cx) / p.fx;
  const float dy = -(((float)j - p.cy) / p.fx);
  const float dz = -1.f;
  float wx, wy, wz, ox = 0.f, oy = 0.f, oz = 0.f;
  if (p.has_c2w) {
    // camera.py:73: directions @ c2w[:, :3].T  (dot over the camera axes, in order)
    wx = dx * p.R[0] + dy * p.R[1] + dz * p.R[2];
    wy = dx * p.R[3] + dy * p.R[4] + dz * p.R[5];
    wz = dx * p.R[6] + dy * p.R[7] + dz * p.R[8];
    ox = p.t[0]; oy = p.t[1]; oz = p.t[2];
  } else {
    wx = dx; wy = dy; wz = dz;
  }
  const float nrm = sqrtf(wx * wx + wy * wy + wz * wz);      // camera.py:68/74
  o[0] = ox; o[1] = oy; o[2] = oz;
  o[3] = wx / nrm; o[4] = wy / nrm; o[5] = wz / nrm;
  o[6] = p.nearv; o[7] = p.farv; o[8] = p.idx;
}

}  // namespace mf
