// The ray set-up arithmetic that render.hip (the crop's rays) and scene.hip (the scene's rays, include/oi_scene.h) share: one
// definition, so "the ray of scene pixel (X, Y)" is oi_gen_rays' ray bit for bit.  Internal linkage.
#ifndef OI_RAY_COMMON_H_
#define OI_RAY_COMMON_H_

#include "oi_common.h"

namespace {

// torch.linspace(start, end, n)[i] in fp32: start + i*step below the midpoint, end - (n-1-i)*step above.
__device__ __forceinline__ float linspace_at(float start, float end, int n, int i) {
  if (n == 1) return start;
  const float step = (end - start) / (float)(n - 1);
  return i < n / 2 ? start + step * (float)i : end - step * (float)(n - 1 - i);
}

// Ray set-up arithmetic shared by the stand-alone kernels and the fused prep_render_kernel.  Floating-point contraction is OFF
// inside these helpers: left to the compiler, a*b + c becomes an fma in one kernel and a multiply + add in another (it
// depends on what surrounds the expression after inlining), and "the same expressions" would differ in the last bit.
struct RayOD {
  float o[3], d[3], near_, far_;
};
// build_rays: pixels = linspace(0,1,R) * recp_size + offset   (generator.py:325-329): the coordinate of pixel i of R
__device__ __forceinline__ float pixel_coord(int R, int i, float off) {
#pragma clang fp contract(off)
  return linspace_at(0.f, 1.f, R, i) * (float)R + off;
}

// the ray through the pixel coordinates (px, py): a pixel centre (make_ray) or a point inside a pixel (aa.hip's sub-pixel rays)
__device__ __forceinline__ RayOD make_ray_at(const float* __restrict__ M /* c2b 4x4 */, const float* __restrict__ kinv, float px,
                                             float py) {
#pragma clang fp contract(off)
  RayOD r;
  float p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = kinv[i * 3 + 0] * px + kinv[i * 3 + 1] * py + kinv[i * 3 + 2];
  const float nrm = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  p[0] /= nrm;
  p[1] /= nrm;
  p[2] /= nrm;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.d[i] = M[i * 4 + 0] * p[0] + M[i * 4 + 1] * p[1] + M[i * 4 + 2] * p[2];
    r.o[i] = M[i * 4 + 3];
  }
  // near_far_from_sphere (generator.py:336-342)
  const float a = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
  const float bb = 2.0f * (r.o[0] * r.d[0] + r.o[1] * r.d[1] + r.o[2] * r.d[2]);
  const float mid = 0.5f * (-bb) / a;
  r.near_ = mid - 1.0f;
  r.far_ = mid + 1.0f;
  return r;
}

__device__ __forceinline__ RayOD make_ray(const float* __restrict__ M /* c2b 4x4 */, const float* __restrict__ kinv, float offx,
                                          float offy, int R, int x, int y) {
  return make_ray_at(M, kinv, pixel_coord(R, x, offx), pixel_coord(R, y, offy));
}

}  // namespace

#endif  // OI_RAY_COMMON_H_
