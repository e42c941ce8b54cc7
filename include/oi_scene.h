/*
 * oi_scene.h -- a scene of many instances: one trace, occlusion between instances, mutual shadows (liboi_hip.so, gfx950).
 *
 * An addition to include/oi_trace_batch.h, whose E elements are E unrelated pictures.  Here the E elements are E instances
 * of ONE picture: K latents at K rigid poses in the scene image of the generator's own camera, the picture the model was
 * trained from.  The union of E surfaces is traced exactly by tracing each instance in its own box
 * frame and keeping the nearest hit per pixel, so the march is the batched trace's, unchanged; this header is the scene
 * layer around it.  Conventions are oi_trace_batch.h's: raw device pointers, caller-owned memory, nothing allocated, no
 * scratch, asynchronous launches ordered on `stream`, 0 or a negative oi_status, oi_last_error() for the text, 64-bit
 * indices, every argument checked before any launch, no float atomics; the only device atomics are integer counters (one add
 * and one max per workgroup); the element index is blockIdx.y where a launch is per element.
 *
 * GEOMETRY.  The scene image is S x S.  Scene pixel (X, Y) has, in instance e's box frame, exactly the ray that
 * oi_gen_rays(c2b_e, kinv, offs = 0, R = S) writes at (X, Y) (one __device__ function; the pixel coordinate is
 * linspace(0, 1, S)[X] * S, not X).  The camera is shared and the poses are rigid, so the ray parameter t of one scene pixel
 * is comparable between instances.  Instance e owns a window of W x W scene pixels with the integer origin window[e] =
 * (x0, y0), which may lie partly or wholly outside the image; W is one value for the scene.  Element e of the batch has
 * N = W * W rays, local ray j * W + i is scene pixel (x0 + i, y0 + j).
 *
 * THE SEQUENCE (oi_amd.scene.trace_scene / SceneSurface.shade run it):
 *
 *   oi_scene_begin            windowed rays, the bounding-sphere cull, the state of the batched trace
 *   oi_sdf_mlp_fwd_segments / oi_trace_batch_step ...   the batched march, unchanged, from bound = live[0]
 *   oi_trace_batch_finish     per element the dense list of its hits
 *   oi_scene_resolve          per scene pixel the nearest hit: owner, owner_ray
 *   oi_scene_visible          per element the dense list of the rays that own their pixel; counts[e][last], live[last]
 *   oi_trace_batch_gather     (hit_index = vis_index) the visible points, padded to n_pad = live[last]
 *   oi_sdf_mlp_fwd            the full pass, B = E, n_per_elem = n_pad: hidden hits never reach it
 *   oi_scene_shade            G-buffer and Phong image of the scene
 * and with shadows, in front of the shading:
 *   oi_scene_points           the visible points of all elements as one list in the world frame
 *   oi_scene_shadow_begin     E occluder elements of L * n_vis shadow rays
 *   the batched march again, oi_trace_batch_finish
 *   oi_scene_visibility       a pixel is lit when its ray ended OI_TRACE_MISS in every element
 */
#ifndef OI_SCENE_H_
#define OI_SCENE_H_

#include "oi_trace_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_SCENE_MAX_RESOLUTION 32768 /* S * S < 2^31 */

/* b: s.N == W * W; every array of the state is written (rays_o, rays_d, near_, far_ included), points [E][N][3] wholly: the
 * slots behind an element's entered rays hold the coordinate origin, valid input of the MLP pass.  c2b [E][16], kinv [9],
 * window [E][2] int32.  1 <= W, 1 <= S <= OI_SCENE_MAX_RESOLUTION.
 * Cull: mid = -o.d / d.d, c2 = |o + mid d|^2, h = sqrt((1 - c2) / d.d).  A ray whose pixel is outside the image, or with
 * c2 >= 1, or with mid + h <= 0 (the unit sphere wholly behind the origin) gets OI_TRACE_MISS, steps = 0, t = near_ = far_ =
 * 0, and does not enter the active list.  Every other ray gets near_ = max(mid - h, 0), far_ = mid + h, t = near_,
 * OI_TRACE_MARCH, its sample point and what oi_trace_batch_begin writes, and is entered compacted within its element.
 * counts[e][0] = the entered rays, live[0] their maximum, every other word of counts and live 0. */
int oi_scene_begin(const oi_trace_batch* b, const float* c2b, const float* kinv, const int* window, int W, int S,
                   oi_stream_t stream);

/* owner, owner_ray [S * S] int32: among the elements whose window covers the pixel and whose ray there is OI_TRACE_HIT,
 * the one with the smallest t (equal t: the lowest element index) and the local index of that ray; -1 in both arrays for a
 * pixel without a hit.  One thread per pixel, a fixed-order loop over the elements, no atomics. */
int oi_scene_resolve(const oi_trace_batch* b, const int* window, int W, int S, int* owner, int* owner_ray,
                     oi_stream_t stream);

/* vis_index [E][N] (the first n_vis_e entries of row e are written, in no fixed order: the rays that own their pixel),
 * vis_slot [E][N] (every element: the ray's position in its row of vis_index, or -1).  OVERWRITES counts[e][last] with
 * n_vis_e and live[last] with their maximum: the state then describes the visible hits, and oi_trace_batch_gather with
 * hit_index = vis_index gathers them.  (The host reads the hit counts before this call.) */
int oi_scene_visible(const oi_trace_batch* b, const int* owner, const int* window, int W, int S, int* vis_index,
                     int* vis_slot, oi_stream_t stream);

typedef struct oi_scene_shade_params {
  int E, W, S, L;          /* elements, window, scene resolution, lights (1 .. OI_RELIGHT_MAX_LIGHTS; 0 with image == NULL) */
  long long n_pad;         /* rows of the padded hit arrays, 0 <= n_pad <= W * W; 0: no pixel is owned */
  const int* owner;        /* [S * S] */
  const int* owner_ray;    /* [S * S] */
  const float* rays_o;     /* [E][N][3], N = W * W */
  const float* rays_d;     /* [E][N][3] */
  const float* t;          /* [E][N] */
  const int* vis_slot;     /* [E][N] */
  const float* hit_points; /* [E][n_pad][3] the visible points (oi_trace_batch_gather) */
  const float* grad;       /* [E][n_pad][3] raw SDF gradient there */
  const float* rgb;        /* [E][n_pad][3] albedo there */
  const float* w2b;        /* [E][16] */
  const float* b2w;        /* [E][16] */
  const float* lights;     /* [L][OI_RELIGHT_LIGHT_FLOATS], world frame */
  const float* bg;         /* [3] or NULL (black) */
  const float* visibility; /* [L][S * S] in [0, 1] or NULL: multiplies the diffuse and the specular term, not the ambient */
  /* outputs; any may be NULL, every element of one given is written.  Off the mask: depth NaN, instance -1, the others 0,
   * image = bg.  For an owned pixel depth, normal, normal_world, albedo, mask and image are oi_surface_shade's on element
   * e's slices with e's w2b, bit for bit (one __device__ function). */
  float* depth;            /* [S * S] the ray parameter t */
  float* position;         /* [S * S][3] WORLD frame: b2w_e applied to the hit point */
  float* normal;           /* [S * S][3] object frame of the owner */
  float* normal_world;     /* [S * S][3] w2b_e[:3,:3]^T normal */
  float* albedo;           /* [S * S][3] */
  float* mask;             /* [S * S] */
  int* instance;           /* [S * S] the owner */
  float* image;            /* [L][3][S * S] */
} oi_scene_shade_params;

int oi_scene_shade(const oi_scene_shade_params* p, oi_stream_t stream);

/* The visible points of all elements as one list: point g = offset[e] + slot (slot < n_vis_e = counts[e][last]; offset [E]
 * int32, the exclusive prefix sum of the visible counts, n_vis their sum).  hit_points, grad [E][n_pad][3]; b2w, w2b
 * [E][16].  position [n_vis][3]: b2w_e applied to the point; normal [n_vis][3]: w2b_e[:3,:3]^T (g / max(|g|, 1e-6));
 * elem [n_vis] int32: e.  1 <= n_pad <= N, 1 <= n_vis <= E * n_pad. */
int oi_scene_points(const oi_trace_batch* b, const float* hit_points, const float* grad, long long n_pad, const int* offset,
                    long long n_vis, const float* b2w, const float* w2b, float* position, float* normal, int* elem,
                    oi_stream_t stream);

/* Shadow rays of the n_vis visible points under L lights against every instance.  sb: a batch of E occluder elements with
 * sb->s.N == L * n_vis; ray l * n_vis + g of element e' asks whether instance e' blocks light l from point g.  Every array
 * of the state is written as by oi_scene_begin.  With e = elem[g], n the object-frame normal and l_e the light's direction
 * in e's frame (oi_trace_shadow_begin's expressions, one __device__ function; the compiler is free to contract them
 * differently in the two kernels, so the rays agree with oi_trace_shadow_begin's to the last bits, their states as tested):
 *   n . l_e <= 0: OI_TRACE_BACKFACING in every element, not entered.
 *   e' == e:      oi_trace_shadow_begin's own ray: origin = point + bias n, direction l_e, near 0, far the exit of the unit
 *                 sphere, entered.
 *   e' != e:      origin = w2b_e' applied to (position[g] + bias normal[g]), direction = the light's direction in e''s frame,
 *                 culled against the unit sphere as by oi_scene_begin (OI_TRACE_MISS, not entered) or entered with near and
 *                 far at the sphere.
 * counts[e'][0], live[0] as by oi_scene_begin. */
int oi_scene_shadow_begin(const oi_trace_batch* sb, const float* hit_points, const float* grad, long long n_pad,
                          const int* offset, const int* elem, const float* position, const float* normal, long long n_vis,
                          const float* lights, int L, const float* w2b, float bias, oi_stream_t stream);

/* visibility [L][S * S]: 1 off the mask; on the mask 1 only if the pixel's shadow ray ended OI_TRACE_MISS in EVERY element,
 * 0 for any other status in any element.  shadow_status [E][L * n_vis]; vis_slot [E][N]; a fixed-order loop over the
 * elements, no atomics. */
int oi_scene_visibility(const uint8_t* shadow_status, const int* owner, const int* owner_ray, const int* vis_slot,
                        const int* offset, int E, long long N, int L, long long n_vis, int S, float* visibility,
                        oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_SCENE_H_ */
