// The per-sample shading arithmetic that the compositing kernels (render.hip, render_bwd.hip), relighting (relight.hip), the
// scalar glue (loss.hip) and the traced surface (trace_common.h, env_shade_common.h and the files that include them) share:
// each formula stands here once, so the backward differentiates the forward it calls, and the light-transport kernels that
// must agree with the compositing kernel bit for bit call its expressions instead of restating them.  What differs per caller
// stays with the caller: the composite kernels' scalar light, relight_kernel's per-channel colours and light groups,
// surface_shade_at's visibility and occlusion factors, the environment shade's pixel.
// Not here: mesh_attr.hip forms its normal as g * (1 / max(|g|, 1e-6)), which rounds differently from the quotient below,
// and render.hip's upsample_alpha is the resampling's alpha (renderer.py:143-173), another formula.
// Everything here has internal linkage.
#ifndef OI_SHADE_COMMON_H_
#define OI_SHADE_COMMON_H_

#include "oi_common.h"

namespace {

// F.normalize(v, eps): v / max(|v|, eps)
__device__ __forceinline__ void normalize3(float& x, float& y, float& z, float eps) {
  const float n = fmaxf(sqrtf(x * x + y * y + z * z), eps);
  x /= n;
  y /= n;
  z /= n;
}

// n = g / max(|g|, 1e-6) of a raw sdf gradient g; gn: |g| where the caller holds it (the eikonal term's)
__device__ __forceinline__ void unit_normal(float gx, float gy, float gz, float gn, float& nx, float& ny, float& nz) {
  const float gnc = fmaxf(gn, 1e-6f);
  nx = gx / gnc, ny = gy / gnc, nz = gz / gnc;
}
__device__ __forceinline__ void unit_normal(float gx, float gy, float gz, float& nx, float& ny, float& nz) {
  const float gnc = fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-6f);
  nx = gx / gnc, ny = gy / gnc, nz = gz / gnc;
}

// v = (eye - point) / max(|eye - point|, 1e-6)
__device__ __forceinline__ void unit_view(float ex, float ey, float ez, float px, float py, float pz, float& vx, float& vy,
                                          float& vz) {
  vx = ex - px, vy = ey - py, vz = ez - pz;
  normalize3(vx, vy, vz, 1e-6f);
}

// The unit direction of the light lt = (l, ...) in the box frame Wb (w2b, 4 x 4 row-major): w2b[:3,:3] (l / |l|), the
// direction the generator's light gets at ray set-up (lighting.py:62-64, 115-119), then the F.normalize the compositing
// kernels put in front of the Phong terms: a light equal to the module's gives the forward's direction bit for bit.
__device__ __forceinline__ void light_dir(const float* __restrict__ lt, const float* __restrict__ Wb, float& lx, float& ly,
                                          float& lz) {
  const float l0 = lt[0], l1 = lt[1], l2 = lt[2];
  const float ln = sqrtf(l0 * l0 + l1 * l1 + l2 * l2);
  lx = Wb[0] * (l0 / ln) + Wb[1] * (l1 / ln) + Wb[2] * (l2 / ln);
  ly = Wb[4] * (l0 / ln) + Wb[5] * (l1 / ln) + Wb[6] * (l2 / ln);
  lz = Wb[8] * (l0 / ln) + Wb[9] * (l1 / ln) + Wb[10] * (l2 / ln);
  normalize3(lx, ly, lz, 1e-6f);
}

// Phong geometry of the unit normal n, the unit light direction l and the unit view vector v (lighting.py:167-170, 212-225;
// generator.py:128-152): n . l, v . r with r = -l + 2 (n . l) n, and al = max(v . r, 0) [n . l > 0], the base of the
// specular power.  (The forward kernels drop v . r; the backward needs its sign.)
struct PhongGeometry {
  float ndl, vr, al;
};
__device__ __forceinline__ PhongGeometry phong_geometry(float nx, float ny, float nz, float lx, float ly, float lz, float vx,
                                                        float vy, float vz) {
  PhongGeometry g;
  g.ndl = nx * lx + ny * ly + nz * lz;
  const float rx = -lx + 2.0f * (g.ndl * nx), ry = -ly + 2.0f * (g.ndl * ny), rz = -lz + 2.0f * (g.ndl * nz);
  g.vr = vx * rx + vy * ry + vz * rz;
  g.al = fmaxf(g.vr, 0.f) * (g.ndl > 0.f ? 1.f : 0.f);
  return g;
}

// The light block of the compositing kernels: ambient = sigmoid(a), diffuse = 1 - ambient, specular = max(s, 0), shininess
// (lighting.py:50-60)
struct LightTerms {
  float amb, dif, spec, shin;
};
__device__ __forceinline__ LightTerms light_terms(float ambient, float specular, float shininess) {
  LightTerms l;
  l.amb = oi::sigmoidf_(ambient);
  l.dif = 1.0f - l.amb;
  l.spec = fmaxf(specular, 0.f);
  l.shin = shininess;
  return l;
}

// SingleVarianceNetwork + clip (neus/models/fields.py:267-268; renderer.py:266, 404): inv_s = clamp(exp(10 variance), 1e-6, 1e6).
// raw: before the clamp; unclamped(): the clamp is inactive, so d inv_s / d variance = 10 raw.
struct InvS {
  float v, raw;
  __device__ __forceinline__ bool unclamped() const { return raw > 1e-6f && raw < 1e6f; }
};
__device__ __forceinline__ InvS inv_s_of(float variance) {
  InvS s;
  s.raw = expf(variance * 10.0f);
  s.v = fminf(fmaxf(s.raw, 1e-6f), 1e6f);
  return s;
}

// The annealed cosine of a section whose ray meets the gradient at true_cos = d . g (renderer.py:269-276)
__device__ __forceinline__ float anneal_cos(float true_cos, float car) {
  return -(fmaxf(-true_cos * 0.5f + 0.5f, 0.f) * (1.0f - car) + fmaxf(-true_cos, 0.f) * car);
}

// NeuS alpha of a section (renderer.py:269-286): the sdf's logistic CDF at the section's two ends, alpha = the share of
// prev_cdf lost across it, clipped to [0, 1].  prev_cdf is an output of the forward too.
struct NeusAlpha {
  float alpha, prev_cdf;
};
__device__ __forceinline__ NeusAlpha neus_alpha(float true_cos, float sdf, float dist, float car, float inv_s) {
  NeusAlpha a;
  const float iter_cos = anneal_cos(true_cos, car);
  a.prev_cdf = oi::sigmoidf_((sdf - iter_cos * dist * 0.5f) * inv_s);
  const float next_cdf = oi::sigmoidf_((sdf + iter_cos * dist * 0.5f) * inv_s);
  a.alpha = (a.prev_cdf - next_cdf + 1e-5f) / (a.prev_cdf + 1e-5f);
  a.alpha = fminf(fmaxf(a.alpha, 0.f), 1.f);
  return a;
}

// One 64-sample chunk of the transmittance T_i = prod_{j < i} om_j, om = 1 - alpha + 1e-7 (1 on the lanes past the ray's end):
// weights = alpha * cumprod([1, 1 - alpha + 1e-7])[:-1]   (renderer.py:300) as a wavefront product scan, shifted by
// one lane, times the product of the chunks before it.  -> T_i; carry (1 before the first chunk) takes this chunk's product.
// Every lane of the wavefront calls it.
__device__ __forceinline__ float transmittance_step(float om, int lane, float& carry) {
  const float incl = oi::wave_scan_mul(om, lane);
  float excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 1.0f;
  const float Ti = excl * carry;
  carry *= __shfl(incl, 63, 64);
  return Ti;
}

}  // namespace

#endif  // OI_SHADE_COMMON_H_
