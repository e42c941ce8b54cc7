/*
 * oi_occlusion_batch.h -- the secondary rays and the shade of E views in ONE chain (liboi_hip.so, gfx950): hard shadows, soft
 * shadows, local lights, ambient occlusion and the Phong image for the elements of a batched primary trace.
 *
 * An addition to include/oi_trace_batch.h, include/oi_occlusion.h and include/oi_local_light.h.  The
 * batched trace puts the primary march and the full MLP pass of E views into one chain of launches; here the stages that
 * depend on the light follow: element e's rays are tested against element e's OWN field only, with its own w2b, its own hit
 * list of n_hit_e <= n_pad points and its own sample keys.  Conventions are oi_trace_batch.h's: raw device pointers,
 * caller-owned memory, nothing allocated, asynchronous launches ordered on `stream`, 0 or a negative oi_status,
 * oi_last_error() for the text, 64-bit indices, every argument checked on the host before any launch, blockIdx.y = element,
 * one thread per ray or pixel, no float atomics; the only device atomics are the compaction's integer add and max per
 * workgroup.  No struct of its own: the batch of oi_trace_batch.h, oi_occlusion.h's shade parameters, plain arguments.
 *
 * LAYOUT.  A secondary batch sb has E elements of sb->s.N == L * Sc * n_pad rays: ray (l * Sc + jj) * n_pad + i of element e
 * is sample j = j0 + jj (of S strata) of light l at hit slot i of view e.  The inputs come from the primary batch:
 *
 *   hit_points [E][n_pad][3]   oi_trace_batch_gather's array        grad [E][n_pad][3]   the full pass's gradient rows
 *   hit_index  [E][N]          oi_trace_batch_finish's              hit_slot [E][N]      oi_trace_batch_finish's
 *   counts     [E][OI_TRACE_COUNT_WORDS]  the primary batch's counters: n_hit_e is the last word of row e, read ON THE
 *                              DEVICE -- the host reads nothing       w2b [E][16]          one pose per view
 *
 * THE CHAIN (oi_amd.trace.render_surfaces(batch_secondary=True) sequences it, per chunk [j0, j0 + Sc) of the S samples):
 *
 *   oi_occlusion_batch_begin    the rays of every view; counts[e][0] = the entered rays of element e, live[0] their maximum
 *   for k = 0 .. max_steps - 1, from bound = live[0], while bound > 0:
 *     oi_sdf_mlp_fwd_segments   B = E, n_per_elem = bound, stride = sb->s.N           (oi_trace_batch.h, unchanged)
 *     oi_trace_batch_step       mode SHADOW: the closest-hit step, as the single view's shadow trace runs it
 *     oi_trace_batch_step_anyhit  the sampled modes: a ray ends at its first occluder   (oi_scene_light.h, unchanged)
 *   oi_trace_batch_finish       rays in flight -> OI_TRACE_LIMIT
 *   oi_occlusion_batch_resolve  the chunk's rays that ended OI_TRACE_MISS, added per (view, light, hit slot); the last chunk
 *                               writes the (E, L, N) map
 *   oi_surface_shade_batch      ONE launch for the G-buffers and Phong images of all E views
 *
 * INVARIANTS.
 *   - For i < n_hit_e, ray (l * Sc + jj) * n_pad + i of element e has the origin, direction, near, far and begin status that
 *     the single-view entry of its mode writes for ray (l * S + j) * n_hit_e + i of view e alone, bit for bit: the kernels
 *     call the same device functions (csrc/trace_common.h) on the element's slices.  After the march every such ray's t,
 *     status and steps equal the single-view state's: they depend neither on the slot nor on the bound.
 *   - A slot i >= n_hit_e is OI_TRACE_MISS with origin, direction, near and far 0; it is not entered, the march never sees
 *     it and the resolve never reads it.
 *   - counts[e][0], live[0] and the sample points behind an element's entered rays (the coordinate origin) are written as
 *     oi_scene_shadow_begin writes them.
 *   - A trace split into chunks of increasing j0 equals the unsplit one byte for byte: the resolve adds integers and divides
 *     once.
 */
#ifndef OI_OCCLUSION_BATCH_H_
#define OI_OCCLUSION_BATCH_H_

#include "oi_local_light.h"
#include "oi_occlusion.h"
#include "oi_trace_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the ray of a secondary batch, and the single-view entry whose rays it reproduces per view */
#define OI_OCCLUSION_BATCH_SHADOW 0     /* the hard shadow ray: oi_trace_shadow_begin; S == Sc == 1 */
#define OI_OCCLUSION_BATCH_CAP 1        /* a sample of the light's cap: oi_occlusion_light_begin */
#define OI_OCCLUSION_BATCH_HEMISPHERE 2 /* a cosine hemisphere sample: oi_occlusion_ambient_begin; L == 1, distance > 0 */
#define OI_OCCLUSION_BATCH_LOCAL 3      /* aimed at a local light and ending there: oi_local_light_begin */

/* sb: E elements of L * Sc * n_pad rays, every array written.  N: the rays per element of the PRIMARY batch (the stride of
 * hit_index), 1 <= n_pad <= N, E * N < 2^31.  1 <= L <= OI_RELIGHT_MAX_LIGHTS, 1 <= S <= OI_OCCLUSION_MAX_SAMPLES, the chunk
 * [j0, j0 + Sc) within [0, S).  lights [L][OI_RELIGHT_LIGHT_FLOATS] (mode LOCAL: [L][OI_LOCAL_LIGHT_FLOATS]; HEMISPHERE: not
 * read, may be NULL), radius [L] device memory (CAP only; NULL otherwise), w2b [E][16] (HEMISPHERE: not read, may be NULL),
 * bias >= 0 and finite, distance: HEMISPHERE only.  The sample numbers are keyed on hit_index[e][i], sample j of S and seed. */
int oi_occlusion_batch_begin(const oi_trace_batch* sb, int mode, const float* hit_points, const float* grad,
                             const int* hit_index, const int* counts, long long N, long long n_pad, int L, int S, int j0, int Sc,
                             const float* lights, const float* radius, const float* w2b, float bias, float distance,
                             unsigned seed, oi_stream_t stream);

/* status [E][L * Sc * n_pad]: a finished chunk's.  count [E][L][n_pad] int32: entry (e, l, i) for i < n_hit_e is overwritten
 * at j0 == 0 and added to otherwise (the entries behind a view's hits are set to 0 at j0 == 0); chunks come in increasing j0.  last != 0: out
 * [E][L][N] = count / S at a pixel with a hit slot (oi_occlusion_resolve's single division), 1 off the mask; last == 0: out is
 * not touched (and may be NULL).  E * N < 2^31, 1 <= n_pad <= N, E * L * Sc * n_pad < 2^31. */
int oi_occlusion_batch_resolve(const uint8_t* status, const int* hit_slot, const int* counts, int E, long long N,
                               long long n_pad, int L, int S, int j0, int Sc, int last, int* count, float* out,
                               oi_stream_t stream);

/* oi_surface_shade_ao (local != 0: oi_surface_shade_local, p->lights at local records) for E views in one launch.  Every
 * pointer of p except lights and bg carries a leading element dimension: rays_o, rays_d, t, status, hit_slot and the outputs
 * with stride p->N pixels, hit_points / grad / rgb with stride n_pad points, w2b [E][16], visibility [E][L][N], image
 * [E][L][3][N], ambient_occlusion [E][N] or NULL.  p->n_hit is not read; 0 <= n_pad <= N, E * N < 2^31; the hit arrays may be
 * NULL with n_pad == 0.  Per view the bytes are those of the single-view entry on the view's slices. */
int oi_surface_shade_batch(const oi_surface_ao_params* p, int E, long long n_pad, int local, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_OCCLUSION_BATCH_H_ */
