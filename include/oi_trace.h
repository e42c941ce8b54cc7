/*
 * oi_trace.h -- sphere-traced surface rendering: ray / surface intersection, G-buffer, cast shadows (liboi_hip.so, gfx950).
 *
 * Not a reference replacement: the reference renders by volume integration only, so these entries live outside
 * include/oi_hip.h, whose entries each cite the reference interface they replace (as include/oi_relight.h and
 * include/oi_mesh_attr.h do).  Conventions are oi_hip.h's: raw device pointers, caller-owned buffers, asynchronous launches
 * ordered on `stream`, 0 or a negative oi_status, oi_last_error() for the text.  Nothing is allocated; 64-bit indices; the
 * only device atomics are integer counters (one add per workgroup); arguments are checked before any launch.
 *
 * One trace marches N rays of ONE latent (one gamma / beta row, B = 1 for the MLP passes) against the SDF.  The host
 * sequences the loop (oi_amd.trace.sphere_trace); the MLP passes are the library's own, unchanged:
 *
 *   oi_trace_begin     per ray: t = near, status = MARCH, point = o + t d; active list = identity, counts[0] = N
 *   for k = 0 .. max_steps - 1:
 *     oi_sdf_mlp_fwd   (grad == NULL: the sdf-only kernel) on the first `bound` compacted points
 *     oi_trace_step    per active slot: read its sdf, advance the ray, write its new t / status, and COMPACT the
 *                      surviving rays: the next active list and their points, densely, and counts[k + 1]
 *   oi_trace_finish    rays still in flight get OI_TRACE_LIMIT; the hits are gathered into a dense list (+ points)
 *
 * `bound` may be any upper bound of counts[k] that the host knows: the count never grows, so a count read some steps ago
 * is valid.  Slots at or above counts[k] hold earlier, valid points; oi_trace_step ignores them.
 *
 * The ray state machine (one thread per active ray; s = sdf at o + t d; restated in fp64 by tests/helpers/trace_ref.py):
 *
 *   any phase   s not finite                     -> OI_TRACE_NONFINITE
 *               |s| <= tol                       -> OI_TRACE_HIT at t
 *   MARCH       s < 0 on the ray's first sample  -> OI_TRACE_START_INSIDE (t = near)
 *               s < 0 later                      -> REFINE with the bracket [t_lo, t] (t_lo: the last positive sample)
 *               otherwise                        -> t_lo = t, s_lo = s, t += max(omega s, tol); t > far -> OI_TRACE_MISS
 *   REFINE      Illinois regula falsi: s replaces the bracket end of its sign; when the same end is replaced twice in a
 *               row the retained end's value is halved; t = t_lo + (t_hi - t_lo) s_lo / (s_lo - s_hi), so t is monotone
 *               within [t_lo, t_hi].  Runs until |s| <= tol.  A bracket that cannot be split any more (neither the secant
 *               point nor the mid-point lies strictly inside: the ends are adjacent numbers) ends as a HIT at t_hi.
 *
 * The field is not 1-Lipschitz (|d sdf/dx| reaches 2.8 inside the unit ball), so marching alone overshoots; the bracket
 * recovers those rays.  Slot order after a compaction is not deterministic across workgroups; per-ray results are, because
 * the MLP pass's arithmetic per point does not depend on the slot.
 */
#ifndef OI_TRACE_H_
#define OI_TRACE_H_

#include "oi_hip.h"
#include "oi_relight.h"

#ifdef __cplusplus
extern "C" {
#endif

/* terminal ray states */
#define OI_TRACE_MISS 0
#define OI_TRACE_HIT 1
#define OI_TRACE_LIMIT 2        /* still in flight after max_steps */
#define OI_TRACE_START_INSIDE 3 /* negative sdf on the first sample */
#define OI_TRACE_NONFINITE 4    /* inf / NaN sdf */
#define OI_TRACE_BACKFACING 5   /* shadow rays only: n . l <= 0, not traced */
/* states in flight (never left behind by oi_trace_finish) */
#define OI_TRACE_MARCH 16
#define OI_TRACE_REFINE 17

/* defaults: the values of the rehearsal on the fp64 oracle */
#define OI_TRACE_DEFAULT_TOL 1e-5f
#define OI_TRACE_DEFAULT_OMEGA 1.0f
#define OI_TRACE_DEFAULT_MAX_STEPS 64
#define OI_TRACE_DEFAULT_BIAS 1e-2f /* shadow-ray offset along the normal (scene radius 1) */
/* steps a caller may ask for */
#define OI_TRACE_MAX_STEPS 1024
/* int32 words of `counts`: counts[k] = rays active before step k (0 <= k <= OI_TRACE_MAX_STEPS), the last word = hits */
#define OI_TRACE_COUNT_WORDS 1026

/* One trace's arrays, all caller-owned device memory.  oi_trace_begin writes every element of t, status, steps, bracket,
 * side, active[0 .. N), points and counts; oi_trace_shadow_begin also writes rays_o, rays_d, near_ and far_. */
typedef struct oi_trace_state {
  long long N;      /* rays, 1 <= N < 2^31 */
  float* rays_o;    /* [N][3] */
  float* rays_d;    /* [N][3] */
  float* near_;     /* [N] */
  float* far_;      /* [N] */
  float* t;         /* [N] ray parameter of the last sample / of the result */
  uint8_t* status;  /* [N] OI_TRACE_* */
  uint16_t* steps;  /* [N] sdf evaluations the ray used */
  float* bracket;   /* [N][4] t_lo, s_lo, t_hi, s_hi */
  uint8_t* side;    /* [N] the bracket end replaced last (0 none, 1 low, 2 high) */
  int* active;      /* [2][N] compacted ray indices, double buffered by step parity */
  float* points;    /* [N][3] compacted sample points: the input of the next MLP pass */
  int* counts;      /* [OI_TRACE_COUNT_WORDS] */
} oi_trace_state;

int oi_trace_begin(const oi_trace_state* s, oi_stream_t stream);

/* Step k (0 <= k < OI_TRACE_MAX_STEPS): sdf [bound] are the values at points [0 .. bound).  counts[k] <= bound <= N.
 * tol > 0, omega > 0. */
int oi_trace_step(const oi_trace_state* s, const float* sdf, long long bound, int k, float tol, float omega,
                  oi_stream_t stream);

/* hit_index [N] (the first counts[last] entries are written: the rays with OI_TRACE_HIT, in no fixed order), hit_points
 * [N][3] (o + t d of those rays, bit-equal to the points the MLP saw), hit_slot [N] (every element: the ray's position in
 * hit_index, or -1).  The hit count is counts[OI_TRACE_COUNT_WORDS - 1]. */
int oi_trace_finish(const oi_trace_state* s, int* hit_index, float* hit_points, int* hit_slot, oi_stream_t stream);

/* Shadow rays of n_hit surface points under L lights, s->N == L * n_hit, ray q = l * n_hit + i.  hit_points / grad
 * [n_hit][3]: the points and the raw SDF gradient there (the full MLP pass); lights [L][OI_RELIGHT_LIGHT_FLOATS]; w2b [16].
 * n = g / max(|g|, 1e-6), l = the light's direction in the object frame (oi_relight.h).  n . l > 0: origin = point + bias n,
 * direction = l, near = 0, far = the exit of the unit sphere (0 when the origin is outside and the ray leaves it), status
 * MARCH, entered in the active list.  n . l <= 0: OI_TRACE_BACKFACING, not traced.  counts[0] = the traced rays. */
int oi_trace_shadow_begin(const oi_trace_state* s, const float* hit_points, const float* grad, long long n_hit,
                          const float* lights, int L, const float* w2b, float bias, oi_stream_t stream);

/* visibility [L][N] of the N pixels of the primary trace: 1 for a pixel without a hit (unused) and for a shadow ray that
 * ended OI_TRACE_MISS; 0 for every other state (HIT, START_INSIDE, LIMIT, NONFINITE, BACKFACING). */
int oi_trace_visibility(const uint8_t* shadow_status, const int* hit_slot, long long N, long long n_hit, int L,
                        float* visibility, oi_stream_t stream);

typedef struct oi_surface_params {
  long long N;             /* pixels (rays of the primary trace) */
  long long n_hit;
  int L;                   /* lights, 1 .. OI_RELIGHT_MAX_LIGHTS (0 with image == NULL) */
  const float* rays_o;     /* [N][3] */
  const float* rays_d;     /* [N][3] */
  const float* t;          /* [N] */
  const uint8_t* status;   /* [N] */
  const int* hit_slot;     /* [N] */
  const float* hit_points; /* [n_hit][3] */
  const float* grad;       /* [n_hit][3] raw SDF gradient at the hit points */
  const float* rgb;        /* [n_hit][3] albedo there */
  const float* w2b;        /* [16] */
  const float* lights;     /* [L][OI_RELIGHT_LIGHT_FLOATS] */
  const float* bg;         /* [3] or NULL (black) */
  const float* visibility; /* [L][N] in [0, 1] or NULL: multiplies the diffuse and the specular term, not the ambient */
  /* outputs; any may be NULL, every element of one given is written.  Off the mask: depth NaN, the others 0, image = bg. */
  float* depth;            /* [N] the ray parameter t */
  float* position;         /* [N][3] */
  float* normal;           /* [N][3] g / max(|g|, 1e-6): oi_relight_fwd's normal, object frame */
  float* normal_world;     /* [N][3] w2b[:3,:3]^T normal */
  float* albedo;           /* [N][3] */
  float* mask;             /* [N] 1 where status == OI_TRACE_HIT */
  float* image;            /* [L][3][N] Phong with oi_relight_fwd's expressions at weight 1 */
} oi_surface_params;

int oi_surface_shade(const oi_surface_params* p, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_TRACE_H_ */
