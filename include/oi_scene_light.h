/*
 * oi_scene_light.h -- soft shadows, ambient occlusion and environment lighting BETWEEN the instances of a scene
 * (liboi_hip.so, gfx950).
 *
 * An addition to include/oi_scene.h, whose shadows are one hard ray per directional light, and to include/oi_occlusion.h /
 * include/oi_envlight.h, whose sampled secondary rays know one instance alone in its unit sphere.
 * Here S sampled rays per visible point of a scene are tested against EVERY instance: each direction is drawn once, in the
 * frame of the instance that owns the point, by include/oi_occlusion.h's sampler (one __device__ function with
 * oi_occlusion_light_begin / oi_occlusion_ambient_begin), and moved into every other instance's box frame; a sample counts as
 * free only when its ray ended OI_TRACE_MISS in every element (oi_scene_visibility's rule).  Conventions are oi_scene.h's:
 * raw device pointers, caller-owned memory, nothing allocated, no scratch, asynchronous launches ordered on `stream`, 0 or a
 * negative oi_status, oi_last_error() for the text, 64-bit indices, every argument checked before any launch, no float
 * atomics; the only device atomics are the compaction's integer counters (one add and one max per workgroup); the element
 * index is blockIdx.y where a launch is per element; one thread per ray or scene pixel.
 *
 * CHUNKS.  A trace holds E * L * Sc * n_vis rays: the samples [j0, j0 + Sc) of the S strata.  The two resolves accumulate
 * across chunks -- integer counts, and fp32 sums added in sample order -- so that a capture split into chunks equals the
 * unsplit one byte for byte.  The chunks are resolved in increasing j0, the one that ends at S with last != 0.
 *
 * THE SEQUENCE (oi_amd.scene.SceneSurface.visibility / ambient / capture_transfer run it), after oi_scene_points:
 *
 *   oi_scene_point_pixels       once: the scene pixel of every visible point, the key of its sample sequence
 *   per chunk:
 *     oi_scene_occlusion_begin  E occluder elements of L * Sc * n_vis sampled rays
 *     oi_sdf_mlp_fwd_segments / oi_trace_batch_step_anyhit ...   the batched march in its any-hit form, from bound = live[0]
 *     oi_trace_batch_finish     rays in flight -> OI_TRACE_LIMIT
 *     oi_scene_occlusion_resolve  or  oi_scene_transfer_resolve
 *   oi_scene_shade_ao           oi_scene_shade with an occlusion factor on the ambient term
 *   oi_env_shade                (include/oi_envlight.h, unchanged) on the scene's planes: N = n_hit = S * S, status = HIT on the
 *                               mask, hit_slot = the pixel's own index, rgb = the scene's albedo map
 */
#ifndef OI_SCENE_LIGHT_H_
#define OI_SCENE_LIGHT_H_

#include "oi_envlight.h"
#include "oi_occlusion.h"
#include "oi_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pixel [n_vis] int32: the scene pixel index Y * S + X of visible point g = offset[e] + slot (slot < counts[e][last]), X =
 * window[e][0] + i, Y = window[e][1] + j of its ray vis_index[e][slot] = j * W + i.  b: the primary batch, s.N == W * W;
 * vis_index [E][N]; window [E][2]; offset [E].  1 <= n_vis <= E * N.  The role hit_index has in oi_occlusion_*_begin. */
int oi_scene_point_pixels(const oi_trace_batch* b, const int* vis_index, const int* window, int W, int S, const int* offset,
                          long long n_vis, int* pixel, oi_stream_t stream);

typedef struct oi_scene_occlusion_params {
  int L;                   /* lights, 1 .. OI_RELIGHT_MAX_LIGHTS; 1 when ambient */
  int S;                   /* strata per (light, point), 1 .. OI_OCCLUSION_MAX_SAMPLES */
  int j0, Sc;              /* this chunk's samples: [j0, j0 + Sc) within [0, S), Sc >= 1 */
  int ambient;             /* != 0: the cosine hemisphere about the normal (L == 1); 0: a cap about each light's direction */
  unsigned seed;
  float bias;              /* >= 0, finite */
  float distance;          /* ambient: > 0, INFINITY allowed; not read otherwise */
  long long n_pad;         /* rows of hit_points / grad, >= 1 */
  long long n_vis;         /* 1 .. E * n_pad */
  const float* hit_points; /* [E][n_pad][3] */
  const float* grad;       /* [E][n_pad][3] */
  const int* offset;       /* [E] */
  const int* elem;         /* [n_vis]  (oi_scene_points) */
  const int* pixel;        /* [n_vis]  (oi_scene_point_pixels) */
  const float* position;   /* [n_vis][3] world frame */
  const float* normal;     /* [n_vis][3] world frame */
  const float* lights;     /* [L][OI_RELIGHT_LIGHT_FLOATS] world frame; not read when ambient (may be NULL) */
  const float* radius;     /* [L] angular radii in radians, clamped to [0, pi / 2]; not read when ambient (may be NULL) */
  const float* w2b;        /* [E][16] */
} oi_scene_occlusion_params;

/* sb: a batch of E occluder elements with sb->s.N == L * Sc * n_vis.  Ray (l * Sc + jj) * n_vis + g of element e' asks
 * whether instance e' blocks sample j = j0 + jj of light l (of the hemisphere when ambient) from point g.  With e = elem[g], n
 * the object-frame normal of g and d the direction drawn in e's frame exactly as oi_occlusion_light_begin /
 * oi_occlusion_ambient_begin draw it for hit_index = pixel[g] and sample j of S:
 *   n . d <= 0:  OI_TRACE_BACKFACING in every element, not entered.
 *   e' == e:     the owner's own ray: origin = point + bias n, direction d, near 0, far = the exit of the unit sphere, min'd
 *                with `distance` when ambient; entered.
 *   e' != e:     origin = w2b_e' applied to (position[g] + bias normal[g]), direction = w2b_e'[:3,:3] (w2b_e[:3,:3]^T d);
 *                culled against the unit sphere as by oi_scene_begin (OI_TRACE_MISS, not entered), otherwise near and far at
 *                the sphere; when ambient far = min(far, distance) and a ray with near >= distance is OI_TRACE_MISS, not
 *                entered.
 * Every array of the state, counts[e'][0] and live[0] are written as by oi_scene_shadow_begin. */
int oi_scene_occlusion_begin(const oi_trace_batch* sb, const oi_scene_occlusion_params* p, oi_stream_t stream);

/* oi_trace_batch_step in oi_occlusion_step's any-hit form: a ray ends at its first negative sample, per element.  Arguments
 * and checks are oi_trace_batch_step's. */
int oi_trace_batch_step_anyhit(const oi_trace_batch* b, const float* sdf, long long bound, int k, float tol, float omega,
                               oi_stream_t stream);

/* count [L][S * S] int32 (the caller's accumulator; overwritten when j0 == 0, added to otherwise), out [L][S * S].
 * status [E][L * Sc * n_vis]: the finished states of the chunk [j0, j0 + Sc).  For an owned pixel the count grows by the
 * number of the chunk's samples whose ray ended OI_TRACE_MISS in EVERY element (a fixed-order loop over the elements); with
 * last != 0 out = count / S there and 1 off the mask; out is not touched with last == 0.  E, N, n_vis as for
 * oi_scene_visibility, n_vis >= 1. */
int oi_scene_occlusion_resolve(const uint8_t* status, const int* owner, const int* owner_ray, const int* vis_slot,
                               const int* offset, int E, long long N, int L, int S, int j0, int Sc, long long n_vis,
                               int scene_S, int last, int* count, float* out, oi_stream_t stream);

/* transfer [9][S * S], planar, WORLD frame: between chunks the running fp32 sums (loaded when j0 > 0, stored at the end of
 * the chunk).  Per owned pixel and per sample in sample order: when the ray escaped every element, sh9 of the world direction
 * (w2b_owner[:3,:3]^T d of the owner's element, normalised with eps 1e-6: oi_transfer_resolve's expressions) is added.  With
 * last != 0 the sums are divided by S once.  Nine zeros off the mask.  status, rays_d [E][Sc * n_vis] (L == 1, ambient). */
int oi_scene_transfer_resolve(const uint8_t* status, const float* rays_d, const int* owner, const int* owner_ray,
                              const int* vis_slot, const int* offset, const float* w2b, int E, long long N, int S, int j0,
                              int Sc, long long n_vis, int scene_S, int last, float* transfer, oi_stream_t stream);

/* The unshadowed closed form, oi_transfer_normal's arithmetic on the owner's slices: transfer [9][S * S] = A_band y_c(world
 * normal) on the mask, zeros off it.  grad [E][n_pad][3]; nothing is traced. */
int oi_scene_transfer_normal(const float* grad, long long n_pad, const int* owner, const int* owner_ray, const int* vis_slot,
                             const float* w2b, int E, long long N, int scene_S, float* transfer, oi_stream_t stream);

typedef struct oi_scene_shade_ao_params {
  oi_scene_shade_params s;
  const float* ambient_occlusion; /* [S * S] in [0, 1] or NULL: multiplies the ambient term; NULL: oi_scene_shade's bytes */
} oi_scene_shade_ao_params;

int oi_scene_shade_ao(const oi_scene_shade_ao_params* p, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_SCENE_LIGHT_H_ */
