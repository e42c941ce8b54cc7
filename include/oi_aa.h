/*
 * oi_aa.h -- adaptive anti-aliasing of the sphere-traced surface renderer (liboi_hip.so, gfx950).
 *
 * An addition to oi_trace.h, and its conventions hold: raw device pointers, caller-owned buffers, nothing allocated,
 * asynchronous launches ordered on `stream`, 0 or a negative oi_status, 64-bit indices, arguments checked on the host before
 * any launch; the only device atomic is the integer add per workgroup of the compaction.  The header defines no type of its own:
 * every entry takes plain pointers and oi_trace.h's oi_trace_state.
 *
 * The primary trace shoots one ray through each pixel centre (sample 0).  The pixels whose neighbourhood shows a geometric
 * edge get S - 1 more rays through points inside the pixel; those rays are one more oi_trace_state, marched and shaded by the
 * entries that march and shade any ray set, and the pixel's value is the mean of its S samples (a box filter of one pixel):
 *
 *   oi_aa_classify   which pixels need more samples: the compacted list of flagged pixels
 *   oi_aa_begin      the sub-pixel camera rays of the flagged pixels, started as oi_trace_begin starts rays
 *   (oi_sdf_mlp_fwd / oi_trace_step / oi_trace_finish, the full MLP pass, the shade entries: unchanged)
 *   oi_aa_resolve    per plane and pixel: the centre value, or the mean of the centre and the S - 1 sub-samples
 */
#ifndef OI_AA_H_
#define OI_AA_H_

#include "oi_trace.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_AA_MAX_SAMPLES 64      /* samples per flagged pixel, the centre included */
#define OI_AA_DEFAULT_PLANE 0.5f  /* plane_threshold: the sine of the angle between a neighbour's offset and the tangent plane */
#define OI_AA_DEFAULT_COS 0.5f    /* cos_threshold: the cosine of the angle between neighbouring normals */

/* The primary trace's status [N], hit_slot [N], hit_points [n_hit][3] and the raw SDF gradient grad [n_hit][3] of an H x W
 * image, N = H * W, pixel (x, y) = ray y * W + x.  hit(p): status[p] == OI_TRACE_HIT (a hit whose hit_slot lies outside
 * 0 .. n_hit - 1 breaks the caller's contract and is read as no hit).  Pixel p is FLAGGED when one of its up to 8 neighbours q
 * inside the image satisfies one of
 *   (mask)    hit(p) != hit(q)
 *   (plane)   both hit, u = x_q - x_p (the hit points), g the gradients:  off(p) || off(q),
 *             off(a):  (g_a . u)^2 > ((s s) (g_a . g_a)) (u . u),  s = plane_threshold
 *             -- the neighbour's point leaves a's tangent plane by more than the angle asin(s).  Both directions are tested:
 *             at an occluding contour the near pixel's normal is perpendicular to the jump, only the far side sees it
 *   (normal)  both hit, d = g_p . g_q:  d <= 0 || d d < ((c c) (g_p . g_p)) (g_q . g_q),  c = cos_threshold
 * in fp32 with multiplies and adds only, no contraction, every dot product summed (x + y) + z and every product associated
 * as written above: a restatement in fp32 is bit-exact.  0 <= s < 1, 0 <= c < 1, finite.
 * edge_index [N]: the first *count entries are written, the flagged pixels in no fixed order; edge_slot [N]: every element,
 * the pixel's position in edge_index or -1; count: one int32 word, cleared by a launch ahead of the kernel. */
int oi_aa_classify(const uint8_t* status, const int* hit_slot, const float* hit_points, const float* grad, long long n_hit,
                   int H, int W, float plane_threshold, float cos_threshold, int* edge_index, int* edge_slot, int* count,
                   oi_stream_t stream);

/* The sub-pixel rays of n_edge flagged pixels of an R x R view: s->N == (S - 1) * n_edge, ray q = (j - 1) * n_edge + e is
 * sample j (1 .. S - 1) of pixel edge_index[e] = y * R + x.  Sample 0 is the pixel centre, which the primary trace holds.
 * c2b [16], kinv [9], offs [2]: oi_gen_rays' at B = 1.  offsets [S][2] (device memory): the samples' positions in units of the
 * pixel pitch, row 0 is not read.  With pitch = (float)R / (float)(R - 1) and (px, py) the pixel coordinates of oi_gen_rays,
 *   px_j = px + offsets[j][0] * pitch,  py_j = py + offsets[j][1] * pitch   (the product and the sum each rounded)
 * and the ray of (px_j, py_j) is oi_gen_rays' arithmetic from there on: with an offset of 0 it is that pixel's ray bit for bit.
 * Writes rays_o, rays_d, near_, far_, and everything oi_trace_begin writes when handed those rays, byte for byte: t, status,
 * steps, bracket, side, active[0 .. N) (the identity), points and counts.  2 <= S <= OI_AA_MAX_SAMPLES, n_edge >= 1, R >= 2. */
int oi_aa_begin(const oi_trace_state* s, const float* c2b, const float* kinv, const float* offs, int R, const int* edge_index,
                long long n_edge, const float* offsets, int S, oi_stream_t stream);

/* centre [P][N], sub [P][(S - 1) * n_edge], out [P][N]; edge_slot [N] is oi_aa_classify's.  edge_slot[p] < 0 (or >= n_edge):
 * out = centre, bit for bit; elsewhere out = (centre + sub_1 + ... + sub_{S-1}) / (float)S with sub_j = sub[(j - 1) * n_edge +
 * edge_slot[p]] of the plane, summed in fp32 in ascending j, one division: the same bits in any launch geometry.
 * P >= 1, 2 <= S <= OI_AA_MAX_SAMPLES, 0 <= n_edge <= N; n_edge == 0: a copy, sub may be NULL. */
int oi_aa_resolve(const float* centre, const float* sub, const int* edge_slot, long long N, long long n_edge, int S, int P,
                  float* out, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_AA_H_ */
