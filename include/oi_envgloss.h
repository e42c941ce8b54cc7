/*
 * oi_envgloss.h -- glossy environment lighting on the sphere-traced surface (liboi_hip.so, gfx950): the Phong lobe of the
 * learned material under an environment map, as a prefiltered map per shininess, a reflection-lobe visibility from the
 * secondary rays of ONE occlusion trace, and a shading entry that adds the term to oi_env_shade's diffuse response.
 *
 * An addition to include/oi_envlight.h, whose conventions hold: raw device pointers (where an argument is HOST memory it
 * says so), caller-owned buffers, nothing allocated, asynchronous launches ordered on `stream`, arguments checked on the
 * host before any launch, 0 or a negative oi_status, 64-bit indices.  No float atomics; every sum has one fixed order, so
 * two runs give identical bytes.
 *
 *   oi_env_prefilter          radiance maps -> G_s on an equirectangular grid              (once per environment map)
 *   oi_occlusion_lobe_begin, the any-hit loop (oi_occlusion_step), oi_trace_finish, oi_occlusion_resolve with L = 1
 *                             S lobe-distributed rays per visible point -> V_spec [N]     (once per captured view)
 *   oi_env_shade_glossy       oi_env_shade's image plus k_s V_spec G_s(R_f^T r_world)      (once per 256 frames)
 *
 * Model.  For a visible point with unit normal n, unit view vector v (towards the eye) and r = 2 (n . v) n - v, the Phong
 * specular term of oi_surface_shade under a light from l is c_s relu(v . (2 (n . l) n - l))^s [n . l > 0], and
 * v . (2 (n . l) n - l) = l . r.  Its response to an environment L(w) is
 *
 *   spec = k_s (1 / pi) integral of L(w) V(w) [n . w > 0] relu(w . r)^s dw
 *
 * (1 / pi as in oi_amd.envlight.EnvLight.from_lights: a light of colour c is the radiance pi c delta, and gives
 * k_s c relu(l . r)^s).  It is evaluated as the usual split-sum APPROXIMATION
 *
 *   spec ~= k_s V_spec G_s(r_world),   G_s(d) = (1 / pi) integral of L(w) relu(w . d)^s dw
 *
 * with V_spec the share of S rays distributed as relu(w . r)^s about r that are above the horizon of n and leave the scene.
 * The split is exact for a constant environment and in the limit s -> infinity; in between it replaces the visibility under
 * the integral by its lobe-weighted mean.  A rotated environment L'(w) = L(R^T w) has G'(d) = G(R^T d): a rotation walk
 * prefilters once and rotates the lookup direction.
 */
#ifndef OI_ENVGLOSS_H_
#define OI_ENVGLOSS_H_

#include "oi_envlight.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_ENVGLOSS_MIN_SHININESS 1
#define OI_ENVGLOSS_MAX_SHININESS 4096
#define OI_ENVGLOSS_CHUNK 2048   /* input pixels per partial of oi_env_prefilter */

/* Floats of oi_env_prefilter's `partial` (0 for arguments oi_env_prefilter refuses): E * ceil(He * We / 2048) * 3 * Hp * Wp,
 * every one of which the launch writes. */
size_t oi_env_prefilter_partial_floats(int E, int He, int We, int Hp, int Wp);

/* radiance [E][3][He][We] -> glossy [E][3][Hp][Wp], both equirectangular with oi_env_project's pixel directions and weights
 * (theta = pi (r + 1/2) / H, phi = 2 pi (c + 1/2) / W, both through sincospif; w_r the exact band area over We, evaluated as
 * there):
 *   glossy[e][ch][a][b] = sum over (r, c) of (w_r / pi) radiance[e][ch][r][c] K(d_ab . d_rc),
 *   K(x) = exp2(shininess * log2(x)) on the hardware's v_exp_f32 / v_log_f32 for x > 0, an exact 0 for x <= 0;
 *   d_ab . d_rc = fmaf(z, z', fmaf(y, y', x x')).
 * Two stages, each with a fixed order.  Stage 1: a workgroup owns 256 output texels (one per thread) and the input pixels
 * [2048 k, 2048 (k + 1)) of one environment; it forms their records (d, (w / pi) L) once, 256 at a time, in LDS, and every
 * thread sums them in chains of 32, the chains' sums in chains of 8, those in a chain of 8, into partial[e][k][ch][texel].
 * Stage 2: one thread per output value sums its partials in chains of at most 32 nested four times.  No term passes through
 * more than 176 additions; element e does not depend on E, and nothing depends on how a launch was sized.
 * 1 <= shininess <= 4096 and finite; 1 <= E <= OI_ENV_MAX_ENVS; He, We, Hp, Wp >= 1; E * He * We < 2^31,
 * E * 3 * Hp * Wp < 2^31 and E * ceil(He * We / 2048) * ceil(Hp * Wp / 256) <= 2^23 (the workgroups of stage 1: the largest
 * grid the library launches anywhere, 2^31 threads; 256 maps of 256 x 512 filtered to 64 x 128 are 2^19). */
int oi_env_prefilter(const float* radiance, int E, int He, int We, float shininess, int Hp, int Wp, float* partial,
                     float* glossy, oi_stream_t stream);

/* Reflection-lobe rays: L = 1, s->N == S * n_hit, ray q = j * n_hit + i; oi_occlusion_ambient_begin's arguments with the
 * eyes rays_o [N_primary][3] of the primary trace and the shininess in place of the distance.
 * n = g / max(|g|, 1e-6); v = e / max(|e|, 1e-6) with e = rays_o[hit_index[i]] - hit_points[i] (oi_surface_shade's view
 * vector); axis a = r = 2 (n . v) n - v, evaluated as 2 ((n . v) n) - v.  Sample numbers, tangent frame and direction formula
 * are oi_occlusion.h's.  The polar law has density proportional to cos^s(alpha): cos(alpha) = u1^(1 / (s + 1)), evaluated as
 * expf(logf(u1) / (s + 1)), and sin(alpha) = sqrt(max(0, 1 - cos^2(alpha))), evaluated as sqrt(-expm1f(2 logf(u1) / (s + 1)))
 * (the same number without the cancellation).
 * n . d > 0: origin = point + bias n, near = 0, far = the exit of the unit sphere, status MARCH, entered in the active list.
 * n . d <= 0: OI_TRACE_BACKFACING, not traced -- the horizon is part of the visibility.  counts[0] = the traced rays.
 * Writes every array oi_occlusion_ambient_begin writes.  1 <= shininess <= 4096 and finite; the other limits are
 * oi_occlusion_ambient_begin's.  V_spec is oi_occlusion_resolve of the finished states with L = 1. */
int oi_occlusion_lobe_begin(const oi_trace_state* s, const float* rays_o, const float* hit_points, const float* grad,
                            const int* hit_index, long long n_hit, int S, float shininess, float bias, unsigned seed,
                            oi_stream_t stream);

/* oi_env_shade (p: its parameters, p->envs the SH halves of the F environments) plus the glossy term.  rays_o [N][3] the
 * eyes of the primary trace, hit_points / grad [n_hit][3], w2b [16]; spec_vis [N] or NULL (= 1); glossy [M][3][Hp][Wp] the
 * prefiltered maps, 1 <= M <= OI_ENV_MAX_ENVS; map_index [F] in HOST memory: environment f looks up map map_index[f], every
 * value is checked here and travels in the kernel's arguments; rot [F][9] row-major world rotations R_f (device); k_s [3]
 * (device); specular [F][3][N] or NULL.  At least one of p->shading, p->image, specular.  Per pixel on the mask:
 *   n, v, r as oi_occlusion_lobe_begin forms them (the eye is rays_o[pixel]);  r_w = w2b[:3,:3]^T r;  d = R_f^T r_w
 *   theta = acosf(clamp(d.z, -1, 1)),  phi = atan2f(d.y, d.x), + 2 pi when negative
 *   u = theta / pi * Hp - 1/2,  v = phi / (2 pi) * Wp - 1/2;  i0 = floor(u), j0 = floor(v), fu = u - i0, fv = v - j0
 *   rows i0, i0 + 1 clamped to [0, Hp - 1]; columns j0, j0 + 1 taken modulo Wp
 *   lookup = lerp(lerp(g[i0][j0], g[i0][j1], fv), lerp(g[i1][j0], g[i1][j1], fv), fu),  lerp(a, b, f) = fmaf(f, b - a, a)
 *   specular = (k_s spec_vis) lookup, the products rounded in this order
 *   image = max(shading, 0) albedo + specular (the sum skipped where specular == 0); bg off the mask
 * shading is oi_env_shade's expression, unchanged; specular is 0 off the mask.  One thread per pixel loops over the F
 * environments: result f of an F-environment launch is bitwise that of the 1-environment launch of environment f.  With
 * k_s == 0, image and shading are byte-equal to oi_env_shade's. */
int oi_env_shade_glossy(const oi_env_shade_params* p, const float* rays_o, const float* hit_points, const float* grad,
                        const float* w2b, const float* spec_vis, const float* glossy, int M, int Hp, int Wp,
                        const int* map_index, const float* rot, const float* k_s, float* specular, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_ENVGLOSS_H_ */
