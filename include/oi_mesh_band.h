/*
 * oi_mesh_band.h -- narrow-band mesh extraction: the SDF is evaluated only near the surface (liboi_hip.so, gfx950).
 *
 * Not a reference replacement: it accelerates the reference's extract_fields (src/third_party/neus/models/renderer.py:15-41),
 * which evaluates the network at every lattice point, and whose drop-in is oi_sdf_lattice.  So these entries live outside
 * include/oi_hip.h (as include/oi_relight.h, include/oi_mesh_attr.h and include/oi_trace.h do).  Conventions are oi_hip.h's:
 * raw device pointers, caller-owned buffers, launches ordered on `stream`, 0 or a negative oi_status, oi_last_error().
 *
 * THE RULE.  Lattice of nx x ny x nz points on the axes xs, ys, zs that oi_sdf_lattice takes; u = scale * sdf; level iso; a
 * point is inside iff u > iso (marching cubes' rule).  hx, hy, hz: the axis spacings, d = sqrt(hx^2 + hy^2 + hz^2) the length
 * of a cell diagonal (h = d / sqrt(3); on a cubic lattice h is the spacing).  Blocks of b points per axis, b in {4, 8}:
 * block (i, j, k) holds the points [b i, b i + b) per axis, the last block of an axis may be ragged; nb = ceil(n / b) blocks
 * per axis, block id (i nby + j) nbz + k.  G: the caller's bound on |grad sdf| (`lipschitz`).
 *
 *   1. coarse pass      one value uc per block at the centre of its full, un-ragged extent: index b i + (b - 1) / 2 per axis,
 *                       on the line through the axis' end points (the centre of a ragged block may lie outside the box).
 *                       The caller makes it with oi_sdf_lattice on three centre axes, with `scale`.
 *   2. classification   a block is INACTIVE iff uc is finite and |uc - iso| > |scale| G m, compared in double, with
 *                           m = d (1 + (b - 1) / 2).
 *                       Every other block is ACTIVE; a block whose uc is inf / NaN is active, so that marching cubes' own
 *                       non-finite check still sees the point.
 *   3. why              (a) a cell crossed by the level holds a point s with u(s) = iso, and each of its eight corners p lies
 *                       within one cell diagonal of s: |u(p) - iso| <= |scale| G d.  (b) a point p of a block differs from the
 *                       block's centre c by at most (b - 1) / 2 lattice steps on every axis -- ragged or not, c is the centre
 *                       of the FULL extent -- so |p - c| <= sqrt(((b-1)/2 hx)^2 + ((b-1)/2 hy)^2 + ((b-1)/2 hz)^2) =
 *                       (b - 1) / 2 d, the norm carried through the three axes: |u(p) - uc| <= |scale| G (b - 1) / 2 d.
 *                       (a) + (b): a block that holds a corner of a crossed cell has |uc - iso| <= |scale| G m and is active.
 *                       (b) alone: every point of an inactive block has |u(p) - uc| < |uc - iso|, i.e. the sign of uc - iso.
 *                       G has to hold on the box grown by (b - 1) / 2 cells, where the centres of ragged blocks may lie.
 *   4. field            points of active blocks: scale * sdf from the MLP, bit-identical to oi_sdf_lattice at that point;
 *                       points of inactive blocks: their block's uc.  A level-crossing cell has all its corners in active
 *                       blocks, every other cell keeps the signs of its corners: marching cubes gives the dense mesh, byte for
 *                       byte.
 *   5. guard            the largest slope between the centres of face-adjacent blocks, |uc_a - uc_b| / (|scale| b h_axis) over
 *                       pairs of finite values, is returned: a lower bound of the true constant.  Above G the caller's bound
 *                       is proven wrong and the field must not be used (oi_amd.mesh.sdf_lattice_band raises ValueError).
 *
 * One element (B == 1) per call.  Call order: oi_sdf_lattice (centre axes) -> oi_band_classify -> oi_sdf_lattice_band.
 */
#ifndef OI_MESH_BAND_H_
#define OI_MESH_BAND_H_

#include "oi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* axis limits (oi_mc_workspace_bytes has the same) */
#define OI_BAND_MIN_RES 2
#define OI_BAND_MAX_RES 1024

/* Bytes of the workspace of oi_band_classify for the lattice and block size: the active list (one uint32 block id per
 * block, at offset 0) and the counters behind it.  0 and oi_last_error() on a bad argument. */
size_t oi_band_workspace_bytes(int nx, int ny, int nz, int block);

/* Classification and fill (steps 2, 4 for inactive blocks, and 5).
 *   coarse [nbx][nby][nbz]   the coarse pass, scale * sdf at the block centres (device; read only)
 *   B                        batch elements of the coarse field: 1 (a batch is refused)
 *   hx, hy, hz               axis spacings (> 0, finite); iso, scale finite, scale != 0; lipschitz > 0 and finite
 *   field [nx][ny][nz]       device; every point of an inactive block is written with its block's uc, no other point is touched
 *   workspace                device, oi_band_workspace_bytes; on return its first counts[1] uint32 are the ids of the active
 *                            blocks, in no particular order (the field does not depend on it)
 *   counts [4]  (host)       blocks, active blocks, inactive blocks with uc > iso, inactive blocks with uc < iso
 *   max_slope   (host)       the guard's slope (0 when no pair of finite face neighbours exists)
 * The two host outputs arrive in one device -> host copy, the call's only synchronisation. */
int oi_band_classify(const float* coarse, int B, int nx, int ny, int nz, int block, double hx, double hy, double hz,
                     float iso, float scale, double lipschitz, float* field, void* workspace, size_t workspace_bytes,
                     long long* counts, float* max_slope, oi_stream_t stream);

/* The band launch (step 4 for active blocks): point pt of the launch belongs to block list[pt / b^3] and has the local index
 * pt % b^3 = (lx b + ly) b + lz inside it; it is evaluated at (xs[b i + lx], ys[b j + ly], zs[b k + lz]) and stored to
 * field[(ix ny + iy) nz + iz].  A local point beyond the lattice (ragged last block) stores nothing.  packed, gamma, beta,
 * prec, fast_trig, scale: as oi_sdf_lattice; B == 1.  list [n_active] device uint32 block ids (< nbx nby nbz; an id outside
 * stores nothing); n_active == 0 launches nothing. */
int oi_sdf_lattice_band(const void* packed, const float* gamma, const float* beta, int B, const float* xs, const float* ys,
                        const float* zs, int nx, int ny, int nz, int block, const unsigned* list, long long n_active,
                        float scale, float* field, int prec, int fast_trig, oi_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* OI_MESH_BAND_H_ */
