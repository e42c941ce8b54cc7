/*
 * oi_raster.h -- a mesh rasteriser: the G-buffer of a triangle mesh (an oi_amd.mesh.IntrinsicMesh or the textured asset of
 * include/oi_mesh_tex.h) under the generator's camera, in the arrays oi_surface_shade / oi_surface_shade_local read
 * (liboi_hip.so, gfx950).
 *
 * An addition to include/oi_trace.h and include/oi_mesh_tex.h, whose conventions hold: raw device pointers, caller-owned
 * memory, nothing allocated, no scratch, asynchronous launches ordered on `stream`, 0 or a negative oi_status,
 * oi_last_error() for the text, 64-bit indices, every argument checked on the host before any launch, no float atomics; the
 * view is blockIdx.y.  This header declares no struct: the entries take plain arguments.  The device atomics are the
 * compaction's integer counters (one add per workgroup) and the depth buffer's 64-bit integer minimum.
 *
 * WHAT THE ENTRIES SHARE.  E views, 1 <= E <= OI_RASTER_MAX_VIEWS, of R x R pixels, 1 <= R <= OI_RASTER_MAX_RESOLUTION,
 * N = R * R, E * N < 2^31.  pos [V][3] the vertex positions in the box frame; triangles [F][3] int32 indices into pos,
 * 0 <= F < 2^31, 1 <= V < 2^31 when F > 0 (a triangle with an index outside 0 .. V - 1 is dropped by the setup and never
 * read by the later stages; oi_amd.raster refuses such a mesh by name).  F == 0 launches nothing in setup and fill.
 *   c2b  [E][16]  the camera-to-box matrices, row-major (what oi_gen_rays is given)
 *   kinv [9]      the inverse intrinsics (what oi_gen_rays is given)
 *   b2c  [E][16]  the inverses of c2b;  K [9] the intrinsics, last row (0, 0, 1)
 *   offs [E][2]   the crop offsets of the views' pixel coordinates (oi_gen_rays' x_offset, y_offset), or NULL for zeros
 *
 * GEOMETRY (csrc/ray_common.h, not restated).  Pixel (X, Y) of view e has the ray make_ray(c2b_e, kinv, offs_e, R, X, Y):
 * the ray through the pixel coordinate px = X R / (R - 1) + offs_e.x (R == 1: px = offs_e.x).  A point p with camera
 * coordinates pc = b2c_e (p, 1) projects to px = (K pc)_x / pc_z, py = (K pc)_y / pc_z, and its raster coordinate is
 * x = (px - offs_e.x) (R - 1) / R (R == 1: the factor is 1): pixel centres are the integers.  Contraction is off in the
 * projection as in the ray helpers.  Coordinates are snapped to 24.8 fixed point, rint(x * 256) as int32.
 *
 * THE THREE STAGES (oi_amd.raster.render_mesh runs them; the caller fills zbuf with all-ones before the fill):
 *
 *   oi_raster_setup    one thread per (view, triangle): corners, bounding box, class; the small and the large triangles
 *                      compacted into two lists per view, IN NO FIXED ORDER (nothing downstream depends on it)
 *   oi_raster_fill     the visible triangle of every pixel: the small list one thread per triangle, the large list one
 *                      wave64 per triangle with its lanes over 8 x 8 blocks of the box
 *   oi_raster_resolve  one thread per (view, pixel): the ray state and the G-buffer of include/oi_trace.h's oi_surface_params
 *
 * COVERAGE is exact: with the corners a, b, c oriented to positive area, the centre P = (256 X, 256 Y) is covered when each
 * edge function (b - a) x (P - a) (int64) is positive, or zero on an edge the triangle owns: the top-left rule -- the edge
 * a -> b with (dx, dy) = b - a is owned when dy < 0, or dy == 0 and dx > 0 (image row 0 on top).  Two triangles that share an
 * edge cover every centre on it exactly once, in either orientation, and a closed fan covers its apex once.
 * DEPTH is the ray parameter t of the pixel's own ray against the triangle's plane: n = (v1 - v0) x (v2 - v0),
 * t = n . (v0 - o) / n . d with contraction off, ONE device function that fill and resolve both call with the vertices in
 * the order of `triangles`: the bits agree, and t is comparable with the traced surface's depth.  A candidate whose t is
 * not finite or <= 0 is skipped.  The visible triangle is the minimum of the key (float_as_uint(t) << 32) | f under a 64-bit
 * integer atomic minimum: equal t goes to the lower index, and the result is a function of the arguments alone.
 *
 * LIMITS.  No clipping: a triangle with a vertex at camera depth <= near is dropped whole, so is one with a snapped
 * coordinate beyond +-OI_RASTER_MAX_COORD pixels.  No mip levels: one bilinear lookup of level 0.  No shadows or occlusion
 * rays (the shade entries take visibility == NULL).  A triangle that fills a large screen is walked by one wave.
 */
#ifndef OI_RASTER_H_
#define OI_RASTER_H_

#include "oi_mesh_tex.h"
#include "oi_trace.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_RASTER_MAX_VIEWS 1024
#define OI_RASTER_MAX_RESOLUTION 16384
#define OI_RASTER_MAX_COORD 4194304 /* 2^22 pixels: the edge functions of snapped corners stay inside int64 */

/* the classes of a triangle in one view */
#define OI_RASTER_DROPPED 0 /* a vertex at camera depth <= near or not finite, a coordinate beyond the limit, a bad index */
#define OI_RASTER_EMPTY 1   /* zero signed area, or the bounding box holds no pixel centre of the screen */
#define OI_RASTER_SMALL 2   /* the box holds at most small_max pixel centres */
#define OI_RASTER_LARGE 3

/* the attribute sources of oi_raster_resolve */
#define OI_RASTER_VERTEX 0
#define OI_RASTER_TEXTURE 1

/* corners [E][F][3][2] int32: the snapped (x, y) of every corner (zeros for a dropped triangle); bbox [E][F][4] int32: x0, y0,
 * x1, y1, the pixel centres x0 <= X <= x1, y0 <= Y <= y1 inside the corners' box and the screen (0, 0, -1, -1 for a dropped
 * or empty triangle); cls [E][F] uint8: OI_RASTER_*; small_list, large_list [E][F] int32: the first counts[e][0] /
 * counts[e][1] entries of row e are written; counts [E][2] int32, cleared here.  near > 0 (the camera depth a vertex must
 * exceed); small_max >= 0: 0 sends every triangle to the large list, a huge value every triangle to the small list. */
int oi_raster_setup(const float* b2c, const float* K, const float* offs, int R, int E, const float* pos, const int* triangles,
                    long long V, long long F, float near_, long long small_max, int* corners, int* bbox, uint8_t* cls,
                    int* small_list, int* large_list, int* counts, oi_stream_t stream);

/* zbuf [E][R * R] uint64, all-ones before the call: afterwards the key of the visible triangle, all-ones where no triangle
 * covers the centre.  corners, bbox, small_list, large_list, counts: oi_raster_setup's, same E, R, F and mesh. */
int oi_raster_fill(const float* c2b, const float* kinv, const float* offs, int R, int E, const float* pos, const int* triangles,
                   long long V, long long F, const int* corners, const int* bbox, const int* small_list, const int* large_list,
                   const int* counts, unsigned long long* zbuf, oi_stream_t stream);

/* Per pixel q = Y * R + X of view e with the visible triangle f (the low word of its key; the high word is not trusted: t is
 * recomputed by the shared function) and p = o + t d (one fused multiply-add per component):
 *   barycentrics  b0 = n . ((v1 - p) x (v2 - p)), b1 = n . ((v2 - p) x (v0 - p)), b2 = n . ((v0 - p) x (v1 - p)), each clamped
 *                 at 0, then divided by their sum ((1, 0, 0) when the sum is 0 or not finite): a bilinear tap never
 *                 leaves the triangle's own texels
 *   mode OI_RASTER_VERTEX   vnormal, valbedo [V][3] interpolated; the normal divided by max(|n|, 1e-6)
 *   mode OI_RASTER_TEXTURE  uv [F][3][2] interpolated; x = u W - 0.5, y = (1 - v) H - 0.5 (image row 0 on top, texel centres
 *                 at + 0.5), the four taps floor / floor + 1 clamped to the atlas, weights from the fractions.  Exactly one
 *                 albedo atlas and one normal atlas [H][W][3] is given: albedo_u8 (byte / 255) or albedo_f32; normal_u8
 *                 (byte / 255 * 2 - 1) or normal_f32; the looked-up normal divided by max(|n|, 1e-6).  1 <= W, H <=
 *                 OI_TEX_MAX_SIZE.
 * Outputs, each optional, every element of one given is written ([E] leading):
 *   rays_o, rays_d [N][3], t [N], status [N] uint8 (OI_TRACE_HIT / OI_TRACE_MISS), hit_slot [N] int32 = q (every pixel: the
 *   view's n_hit is N), hit_points [N][3] = p, grad [N][3] = the unit normal, rgb [N][3], triangle [N] int32, barycentric [N][3].
 * Off the mesh (all-ones key, or a key that names no valid triangle of this mesh, or t not finite or <= 0): status MISS,
 * t = 0, hit_points, grad, rgb, barycentric = 0, triangle = -1; rays_o, rays_d and hit_slot as everywhere. */
int oi_raster_resolve(const float* c2b, const float* kinv, const float* offs, int R, int E, const float* pos,
                      const int* triangles, long long V, long long F, const unsigned long long* zbuf, int mode,
                      const float* vnormal, const float* valbedo, const float* uv, int W, int H,
                      const unsigned char* albedo_u8, const float* albedo_f32, const unsigned char* normal_u8,
                      const float* normal_f32, float* rays_o, float* rays_d, float* t, uint8_t* status, int* hit_slot,
                      float* hit_points, float* grad, float* rgb, int* triangle, float* barycentric, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_RASTER_H_ */
