/*
 * oi_envbounce.h -- one diffuse interreflection bounce under environment lighting (liboi_hip.so, gfx950): the transfer rays
 * of a captured view that END ON THE OBJECT carry the radiance the surface reflects there, folded into a per-channel transfer
 * vector, so the shading stays a dot product per pixel and channel (precomputed radiance transfer with interreflection,
 * Sloan et al. 2002, on the visible points of one view).
 *
 * An addition to include/oi_envlight.h, whose conventions hold: raw device pointers, caller-owned buffers, nothing allocated,
 * asynchronous launches ordered on `stream`, arguments checked on the host before any launch, 0 or a negative oi_status,
 * 64-bit indices.  There is NO atomic here, float or integer: every sum has one fixed order, so two runs give identical bytes.
 *
 *   oi_occlusion_ambient_begin          S cosine-weighted rays per visible point             (oi_occlusion.h)
 *   the CLOSEST-HIT loop: oi_trace_step on that state, not oi_occlusion_step                  (oi_trace.h)
 *   oi_trace_finish                     -> hit_index2, hit_points2 [n_hit2][3], hit_slot2 [S * n_hit]
 *   the full MLP pass at hit_points2    -> grad2, rgb2 [n_hit2][3]
 *   oi_transfer_resolve                 the direct transfer T0 [9][N]: the rays that ended MISS (oi_envlight.h; the set of rays
 *                                       that end MISS is the same under both steps, oi_occlusion.h)
 *   oi_bounce_resolve                   the bounce transfer T1 [3][9][N]: the rays that ended HIT on a front face
 *   oi_env_shade_bounce                 (T0 + T1[ch]) . coefficients for F environments
 *
 * Estimator.  x a visible point, d_j its S rays (density (n . w) / pi), y_j the nearest intersection of ray j with the surface,
 * n_j = g_j / max(|g_j|, 1e-6) the normal and rho(y_j) the albedo there.  The outgoing diffuse radiance of y_j is taken as
 * rho(y_j) sum_c A_band(c) y_c(n_j) L_c, A = (1, 2/3, 1/4): oi_transfer_normal's unshadowed closed form.  So
 *
 *   T1[ch][c] = (1 / S) sum_j [status_j == OI_TRACE_HIT and n_j . d_j < 0] rho_ch(y_j) A_band(c) y_c(n_j in the world frame)
 *   shading[ch] = sum_c T0_c L_c[ch] + sum_c T1[ch][c] L_c[ch]
 *
 * Approximations.  ONE bounce.  The bounce is DIFFUSE (the Phong lobe of the secondary point is ignored).  The secondary
 * point's own occlusion is ignored (its radiance is the unshadowed closed form): that OVER-estimates.  Rays that end
 * OI_TRACE_LIMIT, START_INSIDE, NONFINITE or BACKFACING, and rays that reach a back face (n_j . d_j >= 0), bounce nothing:
 * that UNDER-estimates.  Under a constant environment and a white albedo the sum is exactly 1 for every pixel whose rays all
 * end MISS or on a front face (A_0 y_0 2 sqrt(pi) = 1): the furnace.
 */
#ifndef OI_ENVBOUNCE_H_
#define OI_ENVBOUNCE_H_

#include "oi_envlight.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_BOUNCE_FLOATS 27   /* one pixel's bounce transfer: [3][9], channel then coefficient */

/* The bounce transfer of a finished closest-hit trace of oi_occlusion_ambient_begin's rays (ray q = j * n_hit + i: sample j of
 * hit slot i).  status / rays_d: the state's, [S * n_hit] and [S * n_hit][3]; hit_slot2 [S * n_hit]: oi_trace_finish's on that
 * state (the position of ray q in the list of secondary hits, or -1); grad2 / rgb2 [n_hit2][3]: the gradient and the albedo at
 * the secondary hits; hit_slot [N] of the primary trace; w2b [16].  bounce [3][9][N], planar.  For a pixel with hit slot i:
 *   B[ch][c] = (sum over j = 0 .. S - 1, in this order, of [status == OI_TRACE_HIT and 0 <= k < n_hit2 and n . d < 0]
 *               rho_ch * (A_band(c) y_c(n_w))) / S,       k = hit_slot2[q], g = grad2[k], rho = rgb2[k], d = rays_d[q],
 *   n = g / max(|g|, 1e-6),  n_w = w2b[:3,:3]^T n  (oi_transfer_normal's normal and rotation, its products A_band(c) y_c),
 * each term added with one fmaf(rho_ch, A y_c, sum), one division at the end.  A pixel without a hit gets 27 zeros.  One
 * thread per pixel, slot-major: the reads of status, rays_d and hit_slot2 are coalesced across the pixels of a wave; grad2 and
 * rgb2 are gathered.
 * 1 <= N < 2^31, 0 <= n_hit <= N, 1 <= S <= OI_OCCLUSION_MAX_SAMPLES, S * n_hit < 2^31 (oi_transfer_resolve's limits),
 * 0 <= n_hit2 <= S * n_hit; status, rays_d and hit_slot2 may be NULL when n_hit == 0; grad2 and rgb2 may be NULL when
 * n_hit2 == 0, and then every output is 0 (written). */
int oi_bounce_resolve(const uint8_t* status, const float* rays_d, const int* hit_slot2, const float* grad2, const float* rgb2,
                      const int* hit_slot, long long N, long long n_hit, long long n_hit2, int S, const float* w2b, float* bounce,
                      oi_stream_t stream);

/* oi_env_shade_params' fields in its order, then the bounce transfer and its own output. */
typedef struct oi_env_shade_bounce_params {
  long long N;             /* pixels, 1 <= N < 2^31 */
  long long n_hit;         /* 0 <= n_hit <= N */
  int F;                   /* environments, 1 .. OI_ENV_MAX_ENVS */
  const uint8_t* status;   /* [N] of the primary trace: the mask is status == OI_TRACE_HIT */
  const int* hit_slot;     /* [N] */
  const float* rgb;        /* [n_hit][3] albedo (NULL when n_hit == 0 or image == NULL) */
  const float* transfer;   /* [9][N] */
  const float* envs;       /* [F][9][3], device memory */
  const float* bg;         /* [3] or NULL (black) */
  float* shading;          /* [F][3][N] or NULL: D + I, not clamped; 0 off the mask */
  float* image;            /* [F][3][N] or NULL: max(shading, 0) albedo on the mask, bg off it */
  const float* bounce;     /* [3][9][N], required */
  float* indirect;         /* [F][3][N] or NULL: I; 0 off the mask */
} oi_env_shade_bounce_params;

/* One captured view with its bounce transfer under F environments; at least one output.  Per pixel, environment and channel:
 *   D = fmaf(T_8, env[8][ch], ... fmaf(T_0, env[0][ch], 0))              exactly oi_env_shade's chain
 *   I = fmaf(B[ch][8], env[8][ch], ... fmaf(B[ch][0], env[0][ch], 0))
 *   shading = D + I,  indirect = I,  image = max(shading, 0) albedo on the mask, bg off it.
 * One thread per pixel reads its 9 + 27 transfer values once for all F; the loop over F runs inside the thread, so result f of
 * an F-environment launch is bitwise that of a 1-environment launch of environment f.  With bounce == 0 shading and image are
 * oi_env_shade's. */
int oi_env_shade_bounce(const oi_env_shade_bounce_params* p, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_ENVBOUNCE_H_ */
