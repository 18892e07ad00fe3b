// IoU of two 3D corner boxes (x0, y0, z0, x1, y1, z1), the reference's operation order (utils.py:105-149) in f32.  Shared by
// the per-image NMS (detect.hip) and the cross-view merge (views.hip): both are compiled with FMA contraction off, so equal
// inputs give equal bits in either, and the function commutes in every operation (iou6(a, b) == iou6(b, a) bitwise).
// Include inside the including file's own namespace.
#pragma once

__device__ __forceinline__ float iou6(const float* a, const float* b) {
  float e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float lo = fmaxf(a[i], b[i]);
    const float hi = fminf(a[3 + i], b[3 + i]);
    e[i] = fmaxf(hi - lo, 0.0f);
  }
  const float inter = e[0] * e[1] * e[2];
  const float va = (a[3] - a[0]) * (a[4] - a[1]) * (a[5] - a[2]);
  const float vb = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
  const float uni = va + vb - inter;
  return inter / uni;
}
