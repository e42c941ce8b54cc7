/*
 * oi_relight.h -- relighting of a captured render (liboi_hip.so, gfx950).
 *
 * Not a reference replacement: the reference has no relighting (its scripts/test.py:256-258 only carries a commented-out
 * call to a light walk that was never shipped), so this entry lives outside include/oi_hip.h, whose entries each cite
 * the reference interface they replace.  Conventions are oi_hip.h's: raw device pointers, caller-owned buffers, one
 * asynchronous launch ordered on `stream`, 0 or a negative oi_status, oi_last_error() for the text.
 *
 * The shading of Generator.render_maps (generator.py:107-172; lighting.py:126-225) is a per-sample function of the
 * compositing weight, the raw SDF gradient, the albedo and the view direction -- none of which depends on the light.
 * Given those per-sample tensors of one render (Generator.forward(..., return_raw=True): raw_render_out["weights"],
 * ["gradients"], ["raw_color"], ["mid_z_vals"]), oi_relight_fwd shades and composites them under L directional lights
 * in one launch.  For light l and element e:
 *
 *   d_l      = dir_l / |dir_l|                              (world frame, as DirectionalLight.direction)
 *   l_le     = normalize(w2b[e][:3,:3] d_l, eps 1e-6)
 *   n_i      = g_i / max(|g_i|, 1e-6)                       (g = raw SDF gradient)
 *   v_i      = normalize(o - (o + d mz_i), eps 1e-6)
 *   diff_i   = c_d * relu(n_i . l)                          (c_d, c_a, c_s: RGB)
 *   spec_i   = c_s * (relu(v_i . (2 (n_i . l) n_i - l)) [n_i . l > 0]) ^ shininess
 *   shade_i  = c_a + diff_i
 *   image_no_bg = sum_i w_i (shade_i * albedo_i + spec_i),   image = image_no_bg + bg_e (1 - sum_i w_i)
 *   shading = sum_i w_i shade_i,   diffuse = sum_i w_i diff_i,   specular = sum_i w_i spec_i
 *
 * The per-sample expressions and the summation order (per lane over 64-sample chunks, then a wavefront sum) are those of
 * oi_composite_fwd, so a light equal to the generator's reproduces its maps, and result l of an L-light launch is
 * bitwise equal to a 1-light launch of light l.  No atomics; two launches give identical bytes.
 */
#ifndef OI_RELIGHT_H_
#define OI_RELIGHT_H_

#include "oi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one light: dir[3], pad, ambient[3], pad, diffuse[3], pad, specular[3], shininess (world-frame direction, not
 * necessarily unit; the colours are RGB) */
#define OI_RELIGHT_LIGHT_FLOATS 16
/* lights per launch: the launch loops over its lights inside each ray's wavefront, so its time grows with L; larger
 * sets are split by the caller */
#define OI_RELIGHT_MAX_LIGHTS 256

typedef struct oi_relight_params {
  /* the capture: per sample [N][T] / [N][T][3], per ray [N][3], per element [B][4][4] */
  const float* weights;
  const float* grad;    /* raw SDF gradient (not normalised) */
  const float* rgb;     /* albedo */
  const float* mid_z;
  const float* rays_o;
  const float* rays_d;
  const float* w2b;
  const float* lights;  /* [L][OI_RELIGHT_LIGHT_FLOATS], device memory */
  const float* bg;      /* [B][3] background colour, or NULL (then image == image_no_bg) */
  long long N;          /* rays; N % B == 0, rows element-major */
  int T;                /* samples per ray, >= 1 */
  int B;                /* elements, >= 1 */
  int L;                /* lights, 1 .. OI_RELIGHT_MAX_LIGHTS */
  /* outputs, planar [L][B][3][N / B] (the (L, B, 3, H, W) maps); any may be NULL, every element of one given is written */
  float* image;
  float* image_no_bg;
  float* shading;
  float* diffuse;
  float* specular;
} oi_relight_params;

/* The capture is read from memory once per launch whatever L is while a ray's T samples fit the launch's staging area
 * (T <= 1600: 40 bytes of LDS per sample); beyond that the launch re-reads them once per group of lights, with the same
 * results.  OI_ERR_INVALID_ARG (nothing launched) for a NULL params / capture / lights pointer, N < 1, T < 1, B < 1,
 * N % B != 0, or L outside 1 .. OI_RELIGHT_MAX_LIGHTS. */
int oi_relight_fwd(const oi_relight_params* p, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_RELIGHT_H_ */
