/*
 * oi_trace_batch.h -- batched sphere tracing: E latents / views in ONE chain of steps (liboi_hip.so, gfx950).
 *
 * An addition to include/oi_trace.h, whose trace marches N rays of one latent: a frame is then a chain of max_steps
 * dependent (MLP pass, step) pairs whatever its resolution, and a walk of many frames is as many chains on a GPU that each
 * leaves almost empty (DESIGN sections 4.13 and 4.17).  Here E elements (a latent with its own rays: one frame each) share the
 * chain: every launch has blockIdx.y = element.  Conventions are oi_trace.h's: raw device pointers, caller-owned memory,
 * nothing allocated, no scratch, asynchronous launches ordered on `stream`, 0 or a negative oi_status, oi_last_error() for
 * the text, 64-bit indices, every argument checked before any launch, no float atomics; the only device atomics are integer
 * counters (one add and one max per workgroup).
 *
 * LAYOUT.  An oi_trace_batch holds an oi_trace_state whose N is the rays PER ELEMENT and whose arrays carry a leading
 * element dimension, each element with stride N rays:
 *
 *   rays_o, rays_d, points [E][N][3]    near_, far_, t, status, steps, side [E][N]    bracket [E][N][4]
 *   active [E][2][N]    ray indices are local to the element (0 .. N - 1)
 *   counts [E][OI_TRACE_COUNT_WORDS]    counts[e][k] = rays of element e active before step k, the last word = its hits
 *   live   [OI_TRACE_COUNT_WORDS]       live[k] = max_e counts[e][k], the last word = max_e n_hit_e
 *
 * 1 <= E <= OI_TRACE_BATCH_MAX_ELEMS, N >= 1, E * N < 2^31.  Element e's slice of every array is a valid oi_trace_state of N
 * rays: the kernels run oi_trace.h's ray state machine (one __device__ function, csrc/trace_common.h) on that view, and
 * oi_surface_shade, oi_trace_shadow_begin and the entries of oi_occlusion.h take the slices as they are.
 *
 * THE LOOP (oi_amd.trace.sphere_trace_batch sequences it; gamma / beta hold one FiLM row set per element):
 *
 *   oi_trace_batch_begin      per element oi_trace_begin's work; live[0] = N, live[1 ..] = 0
 *   for k = 0 .. max_steps - 1, while bound > 0:
 *     oi_sdf_mlp_fwd_segments B = E, n_per_elem = bound, stride = N: the sdf-only pass on the first `bound` compacted points of
 *                             EVERY element, sdf[e * N + i] for point i of element e
 *     oi_trace_batch_step     per element oi_trace_step's work on min(counts[e][k], bound) slots; live[k + 1]
 *   oi_trace_batch_finish     rays in flight -> OI_TRACE_LIMIT; per element the dense list of its hits; live[last]
 *   n_pad = live[last]        (one word read by the host)
 *   oi_trace_batch_gather     hit_points_padded [E][n_pad][3]
 *   oi_sdf_mlp_fwd            the library's own full pass, unchanged, with B = E, n_per_elem = n_pad
 *
 * INVARIANTS.
 *   - `bound` may be any value with live[k] <= bound <= N that the host knows.  No count ever grows, so a live word read some
 *     steps ago is valid; the host reads ONE word per read-back, as for a single trace.
 *   - Element e is compacted within its own segment: step k writes its surviving rays to active[e][(k + 1) & 1][0 ..
 *     counts[e][k + 1]) and their sample points to points[e][0 .. counts[e][k + 1]).  Slots at or above counts[e][k] hold
 *     earlier, valid points: the MLP pass evaluates them (an element that has ended rides along until the last one ends) and
 *     the step ignores them.
 *   - live[k + 1] is exact when the step's launch has ended: every workgroup puts the value of its element's counter after its
 *     own add into the word with one integer atomicMax, and the workgroup that adds last holds the final count.
 *   - Per-ray results (t, status, steps) are those of oi_trace.h's single trace on that element alone, bit for bit: they depend
 *     neither on the slot nor on the bound, and the MLP pass's arithmetic per point does not depend on blockIdx.y.  Slot order
 *     after a compaction is not deterministic across workgroups.
 *   - hit_points_padded[e][i] is o + t d of ray hit_index[e][i] for i < n_hit_e, by the expression every kernel of the trace
 *     uses: bit-equal to the point the MLP saw.  The slots n_hit_e .. n_pad - 1 hold the coordinate origin, so the list is
 *     valid input of the full pass for every element, one without a hit included; what the pass writes for them is never read.
 *   - n_pad == 0 (no element has a hit): nothing more is launched.
 *
 * What is batched here: the primary trace and the full pass at its hits.  Secondary rays (shadows, soft shadows, ambient
 * occlusion) are traced per element by oi_trace.h / oi_occlusion.h on the element's slices, or for all elements in one chain
 * by include/oi_occlusion_batch.h.
 */
#ifndef OI_TRACE_BATCH_H_
#define OI_TRACE_BATCH_H_

#include "oi_trace.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_TRACE_BATCH_MAX_ELEMS 1024

typedef struct oi_trace_batch {
  oi_trace_state s; /* N = rays per element; every array with the leading element dimension described above */
  int E;            /* elements, 1 .. OI_TRACE_BATCH_MAX_ELEMS, E * s.N < 2^31 */
  int* live;        /* [OI_TRACE_COUNT_WORDS] */
} oi_trace_batch;

/* The sdf-only MLP pass on a segmented point list: point loc (0 <= loc < n_per_elem) of element e (0 <= e < B) is read from
 * pts[(e * stride + loc) * 3 ..] and its sdf written to sdf[e * stride + loc]; nothing else of sdf is written.  gamma / beta
 * [B][9][128] as for oi_sdf_mlp_fwd, whose kernel this is with another point source.  B > 0, 0 < n_per_elem <= stride,
 * B * stride < 2^31. */
int oi_sdf_mlp_fwd_segments(const float* pts, const void* packed, const float* gamma, const float* beta, float* sdf, int B,
                            long long n_per_elem, long long stride, int prec, int fast_trig, oi_stream_t stream);

int oi_trace_batch_begin(const oi_trace_batch* b, oi_stream_t stream);

/* Step k (0 <= k < OI_TRACE_MAX_STEPS): sdf [E][N], of which [e][0 .. bound) are the values at points[e][0 .. bound).
 * live[k] <= bound <= N.  tol > 0, omega > 0. */
int oi_trace_batch_step(const oi_trace_batch* b, const float* sdf, long long bound, int k, float tol, float omega,
                        oi_stream_t stream);

/* hit_index [E][N] (the first n_hit_e entries of row e are written, in no fixed order), hit_slot [E][N] (every element: the
 * ray's position in its row of hit_index, or -1).  n_hit_e = counts[e][OI_TRACE_COUNT_WORDS - 1]; live's last word their
 * maximum. */
int oi_trace_batch_finish(const oi_trace_batch* b, int* hit_index, int* hit_slot, oi_stream_t stream);

/* hit_points_padded [E][n_pad][3], every element written.  max_e n_hit_e <= n_pad <= N; n_pad == 0 launches nothing. */
int oi_trace_batch_gather(const oi_trace_batch* b, const int* hit_index, long long n_pad, float* hit_points_padded,
                          oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_TRACE_BATCH_H_ */
