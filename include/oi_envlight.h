/*
 * oi_envlight.h -- environment lighting on the sphere-traced surface (liboi_hip.so, gfx950): environments as 9 spherical-
 * harmonic coefficients per colour, a per-pixel transfer vector from the secondary rays of ONE occlusion trace, and the
 * diffuse response of the captured view to F environments per launch.
 *
 * An addition to include/oi_trace.h and include/oi_occlusion.h, whose conventions hold: raw device pointers, caller-owned
 * buffers, nothing allocated, asynchronous launches ordered on `stream`, arguments checked on the host before any launch,
 * 0 or a negative oi_status, 64-bit indices.  There is NO atomic here, float or integer: every sum has one fixed order, so
 * two runs give identical bytes.
 *
 *   oi_occlusion_ambient_begin, the any-hit loop, oi_trace_finish     S cosine-weighted rays per visible point (oi_occlusion.h)
 *   oi_transfer_resolve      their final states and directions -> the transfer map [9][N]
 *     (or oi_transfer_normal: the unshadowed closed form, nothing traced)
 *   oi_env_project           equirectangular radiance maps -> coefficients          (once per environment)
 *   oi_env_shade             transfer . coefficients for F environments              (once per 256 frames)
 *
 * SH basis.  Real, bands 0 .. 2, of a unit vector (x, y, z); the index order is fixed:
 *
 *   y0 = 0.28209479                  (1 / (2 sqrt(pi)))
 *   y1 = 0.48860251 y                (sqrt(3 / (4 pi)))
 *   y2 = 0.48860251 z
 *   y3 = 0.48860251 x
 *   y4 = 1.09254843 x y              (sqrt(15 / (4 pi)))
 *   y5 = 1.09254843 y z
 *   y6 = 0.31539157 (3 z^2 - 1)      (sqrt(5 / (16 pi)))
 *   y7 = 1.09254843 x z
 *   y8 = 0.54627422 (x^2 - y^2)      (sqrt(15 / (16 pi)))
 *
 * band(c) = 0, 1, 1, 1, 2, 2, 2, 2, 2.  An environment is float[9][3] -- coefficient-major, RGB -- in the WORLD frame:
 * radiance L(w) = sum_c env[c][.] y_c(w).
 *
 * Transfer.  T_c = integral of V(w) y_c(w) (n . w) / pi dw over the hemisphere of a visible point, V = 1 where the ray
 * towards w leaves the scene (precomputed radiance transfer, Sloan et al. 2002, on the visible points of one view).  The rays
 * of oi_occlusion_ambient_begin are distributed as (n . w) / pi, so the Monte-Carlo estimate is a plain mean over the S
 * samples of [escaped] y_c.  With V = 1 the integral is A_band(c) y_c(n), A = (1, 2/3, 1/4) (Ramamoorthi & Hanrahan 2001,
 * divided by pi).  The diffuse response to an environment is sum_c T_c env[c][ch]; under the constant environment
 * env[0] = 2 sqrt(pi) it is the share of escaped rays, i.e. oi_occlusion_resolve's ambient occlusion.
 */
#ifndef OI_ENVLIGHT_H_
#define OI_ENVLIGHT_H_

#include "oi_occlusion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_ENV_COEFFS 9
#define OI_ENV_FLOATS 27      /* one environment: [9][3] */
#define OI_ENV_MAX_ENVS 256   /* environments per oi_env_project / oi_env_shade launch */

/* Floats of oi_env_project's `partial` (0 for arguments oi_env_project refuses): E * ceil(He * We / 8192) * 27, every one of
 * which the launch writes. */
size_t oi_env_project_partial_floats(int E, int He, int We);

/* radiance [E][3][He][We] equirectangular maps -> coeffs [E][9][3].  Pixel (r, c): polar angle theta = pi (r + 1/2) / He from
 * +z, azimuth phi = 2 pi (c + 1/2) / We, d = (sin theta cos phi, sin theta sin phi, cos theta); weight
 * w_r = (cos(pi r / He) - cos(pi (r + 1) / He)) 2 pi / We, the exact area of the band over We, so the weights sum to 4 pi
 * (evaluated as 2 sin(theta) sin(pi / (2 He)) 2 pi / We: the same number without the cancellation).
 * coeffs[e][c][ch] = sum over the pixels of w_r radiance[e][ch][r][c] y_c(d).
 * Two stages, each with a fixed order: workgroup b of environment e sums pixels [8192 b, 8192 (b + 1)) -- per thread 32 pixels
 * in sequence, then a tree over the 256 threads -- into partial[e][b][27]; one workgroup per environment sums the partials,
 * per thread chains of at most 32 terms nested twice, then the same tree.  No term passes through more than 128 additions,
 * and element e does not depend on E.  1 <= E <= OI_ENV_MAX_ENVS, He >= 1, We >= 1, E * He * We < 2^31. */
int oi_env_project(const float* radiance, int E, int He, int We, float* partial, float* coeffs, oi_stream_t stream);

/* The transfer map of a finished oi_occlusion_ambient_begin trace (ray q = j * n_hit + i: sample j of hit slot i).
 * status / rays_d: the state's, [S * n_hit] and [S * n_hit][3]; hit_slot [N] of the primary trace; w2b [16].
 * transfer [9][N], planar.  For a pixel with hit slot i:
 *   T_c = (sum over j = 0 .. S - 1, in this order, of [status == OI_TRACE_MISS] y_c(d_w)) / S
 *   d_w = v / max(|v|, 1e-6),  v = w2b[:3,:3]^T d  (the rotation oi_surface_shade applies for normal_world)
 * Every other final state -- OI_TRACE_BACKFACING, HIT, LIMIT, START_INSIDE, NONFINITE -- counts as occluded: exactly
 * oi_occlusion_resolve's notion.  A pixel without a hit gets nine zeros.  One thread per pixel, slot-major: the reads of
 * status and rays_d are coalesced across the pixels of a wave.
 * 1 <= N < 2^31, 0 <= n_hit <= N, 1 <= S <= OI_OCCLUSION_MAX_SAMPLES, S * n_hit < 2^31 (oi_occlusion_resolve's limits);
 * status and rays_d may be NULL when n_hit == 0. */
int oi_transfer_resolve(const uint8_t* status, const float* rays_d, const int* hit_slot, long long N, long long n_hit, int S,
                        const float* w2b, float* transfer, oi_stream_t stream);

/* The unshadowed closed form, for S = 0: T_c = A_band(c) y_c(n_w), A = (1, 2/3, 1/4); n_w = w2b[:3,:3]^T (g / max(|g|, 1e-6)),
 * oi_surface_shade's normal_world.  grad [n_hit][3] (NULL when n_hit == 0), hit_slot [N], transfer [9][N]; nine zeros for a
 * pixel without a hit.  1 <= N < 2^31, 0 <= n_hit <= N. */
int oi_transfer_normal(const float* grad, const int* hit_slot, long long N, long long n_hit, const float* w2b, float* transfer,
                       oi_stream_t stream);

typedef struct oi_env_shade_params {
  long long N;             /* pixels, 1 <= N < 2^31 */
  long long n_hit;         /* 0 <= n_hit <= N */
  int F;                   /* environments, 1 .. OI_ENV_MAX_ENVS */
  const uint8_t* status;   /* [N] of the primary trace: the mask is status == OI_TRACE_HIT */
  const int* hit_slot;     /* [N] */
  const float* rgb;        /* [n_hit][3] albedo (NULL when n_hit == 0 or image == NULL) */
  const float* transfer;   /* [9][N] */
  const float* envs;       /* [F][9][3], device memory */
  const float* bg;         /* [3] or NULL (black) */
  float* shading;          /* [F][3][N] or NULL: sum_c T_c env[c][ch], not clamped; 0 off the mask */
  float* image;            /* [F][3][N] or NULL: max(shading, 0) albedo on the mask, bg off it */
} oi_env_shade_params;

/* One captured view under F environments; at least one output.  shading = fmaf(T_8, env[8][ch], ... fmaf(T_0, env[0][ch], 0)),
 * c = 0 .. 8 in this order.  One thread per pixel reads its nine transfer values once for all F.  Result f of an F-environment
 * launch is bitwise that of a 1-environment launch of environment f (the property oi_relight_fwd documents for its lights). */
int oi_env_shade(const oi_env_shade_params* p, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_ENVLIGHT_H_ */
