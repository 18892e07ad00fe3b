// Corner / centre-size boxes and their IoU in the reference's operation order (utils.py:42-51, :105-149), f32.  Shared by the
// matcher (multibox.hip) and the prior fit report (priorfit.hip): both are compiled with FMA contraction off, so equal inputs
// give equal bits in either and in the CPU oracle (oracle/boxes.py).
// Include inside the including file's own namespace.
#pragma once

struct Box {
  float v[6];
};

__device__ __forceinline__ Box load_box(const float* p) {
  Box b;
#pragma unroll
  for (int i = 0; i < 6; ++i) b.v[i] = p[i];
  return b;
}

// utils.py:42-51
__device__ __forceinline__ Box c_to_xyz(const Box& c) {
  Box o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float h = c.v[3 + i] / 2.0f;
    o.v[i] = c.v[i] - h;
    o.v[3 + i] = c.v[i] + h;
  }
  return o;
}
__device__ __forceinline__ float box_vol(const Box& b) {
  return (b.v[3] - b.v[0]) * (b.v[4] - b.v[1]) * (b.v[5] - b.v[2]);
}
// utils.py:105-149
__device__ __forceinline__ float box_inter(const Box& a, const Box& b) {
  float e[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float lo = fmaxf(a.v[i], b.v[i]);
    const float hi = fminf(a.v[3 + i], b.v[3 + i]);
    e[i] = fmaxf(hi - lo, 0.0f);
  }
  return e[0] * e[1] * e[2];
}
__device__ __forceinline__ float box_iou(const Box& a, float vol_a, const Box& b, float vol_b) {
  const float inter = box_inter(a, b);
  const float uni = vol_a + vol_b - inter;
  return inter / uni;
}
