/*
 * oi_mesh_tex.h -- textured mesh export: a per-triangle UV atlas with baked albedo and normal maps (liboi_hip.so, gfx950).
 *
 * Not a reference replacement (the reference's extract_geometry stops at positions and triangles): an addition to
 * oi_mesh_attr.h, whose conventions hold here -- raw device pointers, caller-owned buffers, asynchronous launches ordered on
 * `stream`, 0 or a negative oi_status, oi_last_error() for the text.  Plain arguments, no struct.  Nothing is allocated, no
 * atomics, fixed order: two identical calls give identical bytes.  Every kernel is one thread per texel or per corner.
 *
 * THE ATLAS (closed form, no packer).  T: the texel size of a triangle, OI_TEX_MIN_TEXEL <= T <= OI_TEX_MAX_TEXEL;
 * F triangles; a triangle owns n_T = T (T + 1) / 2 texels.
 *   cells    triangle f lives in cell c = f >> 1; a cell is T + 1 texels wide and T high; ncells = (F + 1) >> 1;
 *            cols = the smallest integer with cols * cols >= ncells (at least 1); rows = ceil(ncells / cols) (at least 1);
 *            W = cols (T + 1), H = rows T; cell origin x0 = (c % cols)(T + 1), y0 = (c / cols) T; image row 0 is the top row.
 *            W, H <= OI_TEX_MAX_SIZE.
 *   texels   local (i, j), j = 0 .. T - 1, i = 0 .. T - 1 - j, numbered k = j T - j (j - 1) / 2 + i (rows of falling length).
 *            even f (lower half): pixel (x0 + i, y0 + j); odd f (upper half, the point reflection): (x0 + T - i,
 *            y0 + T - 1 - j).  The two halves tile the cell exactly; for odd F the last cell's upper half has no owner.
 *   corners  corner m of triangles[f] has the centre coordinates c_0 = (0, 0), c_1 = (T - 2, 0), c_2 = (0, T - 2): the
 *            interior is i + j <= T - 2, the row i + j = T - 1 is the gutter past the hypotenuse.  Pixel position of (cu, cv):
 *            lower half (x0 + 0.5 + cu, y0 + 0.5 + cv), upper half (x0 + T + 0.5 - cu, y0 + T - 0.5 - cv);
 *            u = x / W, v = 1 - y / H (the OBJ convention).  Every tap of a bilinear lookup (texel centres at + 0.5) that
 *            carries non-zero weight, anywhere in the closed UV triangle, is a texel the triangle owns.  Mip levels above 0
 *            bleed into the neighbours, as in every per-triangle atlas.
 *   points   b1 = float(i) / float(T - 2), b2 = float(j) / float(T - 2) (fp32 divisions), b0 = (1 - b1) - b2; per axis
 *            p = fma(b2, v2, fma(b1, v1, b0 * v0)) from the vertex positions.  Gutter texels have b0 < 0: they are
 *            EXTRAPOLATED in the triangle's plane, not clamped.  The T - 1 texels along an edge sit at the parameters
 *            k / (T - 2) on both triangles that share it.
 *
 * The bake of a chunk of whole triangles f0 .. f0 + nf - 1 (oi_amd.mesh.bake_textures sequences it):
 *   oi_tex_points -> (oi_sdf_mlp_fwd + oi_mesh_newton) x refine -> oi_sdf_mlp_fwd -> oi_mesh_attr_finalize -> oi_tex_store
 */
#ifndef OI_MESH_TEX_H_
#define OI_MESH_TEX_H_

#include "oi_mesh_attr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OI_TEX_MIN_TEXEL 3
#define OI_TEX_MAX_TEXEL 64
#define OI_TEX_MAX_SIZE 16384

/* Host only: the atlas of F triangles at texel size T.  W, H, cols (each optional) are written whenever F and T are legal,
 * also when the atlas is over OI_TEX_MAX_SIZE -- which, like a T outside its range or F outside 0 .. 2^31 - 1, gives a
 * negative status.  The one place where the rule above stands in C. */
int oi_tex_layout(long long F, int T, int* W, int* H, int* cols);

/* uv [F][3][2]: the texture coordinates of every corner.  F == 0 launches nothing. */
int oi_tex_uv(long long F, int T, float* uv, oi_stream_t stream);

/* The planar points of one chunk.  pos [V][3]: vertex positions; triangles [F][3] int32 indices into pos (the caller has
 * checked them against V); out [nf * n_T][3]: the points in the order (f, k); flags [nf * n_T] (optional) is cleared: the
 * start of a pass, as oi_mesh_vertex_world does.  0 <= f0, 0 <= nf, nf * n_T < 2^31; nf == 0 launches nothing. */
int oi_tex_points(const float* pos, const int* triangles, long long f0, long long nf, int T, float* out, uint8_t* flags,
                  oi_stream_t stream);

/* Scatter the finalized values of one chunk to their pixels.  normals, rgb [nf * n_T][3] in the order (f, k); F: the mesh's
 * triangle count (it fixes the atlas); f0 + nf <= F.  Each atlas is optional: albedo_f32, normal_f32 [H][W][3] float32 =
 * rgb, normals as they are; albedo_u8 [H][W][3] = round-to-nearest-even of clamp(rgb, 0, 1) * 255 (NaN -> 0: the rule of the
 * vertex record); normal_u8 [H][W][3] = the same rule on n * 0.5 + 0.5 (an object-space normal map).  Pixels no triangle
 * owns are never written: the caller fills the atlases beforehand. */
int oi_tex_store(const float* normals, const float* rgb, long long f0, long long nf, int T, long long F, float* albedo_f32,
                 float* normal_f32, unsigned char* albedo_u8, unsigned char* normal_u8, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_MESH_TEX_H_ */
