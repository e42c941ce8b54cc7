// One sample of the bounce transfer: what bounce_resolve_kernel (envbounce.hip, include/oi_envbounce.h)
// and scene_bounce_resolve_kernel (scene_bounce.hip, include/oi_scene_bounce.h, 4.26) add for a transfer ray that ended on a
// surface.  Written once, so a one-instance scene and the single view give the same bytes.  Internal linkage, as trace_common.h.
#ifndef OI_BOUNCE_COMMON_H_
#define OI_BOUNCE_COMMON_H_

#include "trace_common.h"
#include "../../include/oi_envbounce.h"

namespace {

static_assert(OI_BOUNCE_FLOATS == 3 * OI_ENV_COEFFS, "[3][9] per pixel");

// one pixel's running sums of the bounce transfer, [channel][coefficient].  A struct that bounce_sample takes and returns BY
// VALUE: through a reference the compiler pairs the 27 sums differently and bounce_resolve_kernel needs 86 VGPRs instead of 60
// (DESIGN section 4.26).
struct BounceSums {
  float v[3][OI_ENV_COEFFS];
};

// The secondary hit k (gradient grad2[k], albedo rgb2[k]) of a ray whose direction in the hit's frame is rays_d[r], w2b that
// frame's pose: n = g / max(|g|, 1e-6); a back face (not n . d < 0) adds nothing; otherwise a.v[ch][c] = fmaf(rho_ch, A_band(c)
// y_c(w2b[:3,:3]^T n), a.v[ch][c]) -- transfer_normal_kernel's closed form at the secondary hit.  -> the sums with the sample.
__device__ __forceinline__ BounceSums bounce_sample(const float* __restrict__ grad2, const float* __restrict__ rgb2, long long k,
                                                    const float* __restrict__ rays_d, long long r,
                                                    const float* __restrict__ w2b, BounceSums a) {
  float nx, ny, nz, t[OI_ENV_COEFFS];
  unit_normal(grad2, k, nx, ny, nz);
  if (nx * rays_d[r * 3 + 0] + ny * rays_d[r * 3 + 1] + nz * rays_d[r * 3 + 2] < 0.f) {  // else a back face
    normal_transfer(w2b, nx, ny, nz, t);
    const float r0 = rgb2[k * 3 + 0], r1 = rgb2[k * 3 + 1], r2 = rgb2[k * 3 + 2];
#pragma unroll
    for (int c = 0; c < OI_ENV_COEFFS; ++c) {
      a.v[0][c] = __fmaf_rn(r0, t[c], a.v[0][c]);
      a.v[1][c] = __fmaf_rn(r1, t[c], a.v[1][c]);
      a.v[2][c] = __fmaf_rn(r2, t[c], a.v[2][c]);
    }
  }
  return a;
}

}  // namespace

#endif  // OI_BOUNCE_COMMON_H_
