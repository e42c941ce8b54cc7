// What aa.hip and scene_aa.hip share (include/oi_aa.h, include/oi_scene_aa.h; DESIGN sections 4.29 and 4.30): the arithmetic of the
// plane and normal criteria on a pair of neighbouring hit pixels -- ONE __device__ function, so the single view's classifier
// and the scene's flag the same pairs bit for bit -- the clearing of the compaction's counter, and the check of a sample
// count.  fp32 multiplies and adds only, contraction off, associated as oi_aa.h states them: tests/helpers/aa_ref.py restates
// them in numpy fp32.  Internal linkage, as trace_common.h.
#ifndef OI_AA_COMMON_H_
#define OI_AA_COMMON_H_

#include "trace_common.h"
#include "../../include/oi_aa.h"

namespace {

// (a . b) summed x, y, z in that order, every product and sum rounded on its own
__device__ __forceinline__ float dot3(const float* a, const float* b) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// oi_aa.h's off(a): (g . u)^2 > ((s s) (g . g)) (u . u)
__device__ __forceinline__ bool off_plane(const float* g, float gg, const float* u, float uu, float s2) {
#pragma clang fp contract(off)
  const float du = dot3(g, u);
  return du * du > (s2 * gg) * uu;
}

// oi_aa.h's (plane) || (normal) for two hit pixels p and q: their points xp, xq and raw gradients gp, gq in ONE frame, gpp =
// gp . gp (the caller holds it across its neighbours), s2 and c2 the squared thresholds
__device__ __forceinline__ bool aa_pair_edge(const float* xp, const float* gp, float gpp, const float* xq, const float* gq, float s2,
                                             float c2) {
#pragma clang fp contract(off)
  float u[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) u[a] = xq[a] - xp[a];
  const float uu = dot3(u, u), gqq = dot3(gq, gq);
  if (off_plane(gp, gpp, u, uu, s2) || off_plane(gq, gqq, u, uu, s2)) return true;  // ((g . -u)^2 == (g . u)^2 exactly)
  const float d = dot3(gp, gq);
  return d <= 0.f || d * d < (c2 * gpp) * gqq;
}

__global__ void __launch_bounds__(64) aa_clear_kernel(int* __restrict__ count) {
  if (threadIdx.x == 0) *count = 0;
}

inline int check_aa_samples(const char* what, int S) {
  OI_REQUIRE(S >= 2 && S <= OI_AA_MAX_SAMPLES, "%s: S=%d (2 .. %d samples)", what, S, OI_AA_MAX_SAMPLES);
  return OI_OK;
}

inline int check_aa_thresholds(const char* what, float plane_threshold, float cos_threshold) {
  OI_REQUIRE(plane_threshold >= 0.f && plane_threshold < 1.f && cos_threshold >= 0.f && cos_threshold < 1.f,
             "%s: plane_threshold %g, cos_threshold %g (both in [0, 1))", what, (double)plane_threshold, (double)cos_threshold);
  return OI_OK;
}

}  // namespace

#endif  // OI_AA_COMMON_H_
