"""Mesh extraction -- drop-in for the reference's extract_fields / extract_geometry
(src/third_party/neus/models/renderer.py:15-41) and for mcubes.marching_cubes (PyMCubes), which is not part of this stack.

    sdf_lattice      dense SDF field of a latent on a lattice   oi_sdf_lattice   (the points are never materialised)
    marching_cubes   triangle mesh of a field                   oi_mc_count + oi_mc_emit
    extract_fields / extract_geometry   the reference's functions with a caller-supplied query_func (64^3 chunks)
    save_ply         binary little-endian PLY with numpy only (optionally with normals and colours)
    sdf_lattice_band the same field with the MLP run only near the level set   oi_sdf_lattice (one value per block) +
                     oi_band_classify + oi_sdf_lattice_band   (include/oi_mesh_band.h; marching cubes gives the same mesh)
    vertex_attributes / extract_intrinsic_mesh   the intrinsic mesh: vertices moved onto the level set, analytic normals
                     and albedo per vertex   oi_mesh_vertex_world + (oi_sdf_mlp_fwd + oi_mesh_newton) x refine +
                     oi_sdf_mlp_fwd + oi_mesh_attr_finalize   (include/oi_mesh_attr.h)
    bake_textures / extract_textured_mesh   the textured mesh: a per-triangle UV atlas, every texel projected onto the level
                     set, baked albedo and object-space normal maps   oi_tex_uv + per chunk (oi_tex_points + the vertex
                     pass's chain + oi_tex_store)   (include/oi_mesh_tex.h)
    save_png / save_obj   8-bit RGB PNG with zlib and struct only; Wavefront OBJ + MTL + the two maps of a TexturedMesh

DESIGN section 4.10 has the table rule, the output order and the measured numbers; section 4.12 the vertex pass; section 4.14
the narrow band; section 4.28 the texture atlas."""
import ctypes
import dataclasses
from typing import Optional

import numpy as np
import torch

from . import lib as _l
from . import ops
from .fields import LatentField, field_pack as _field_pack   # (inference.export_mesh resolves its pack through it)
from .ops import _p, _stream

MAX_RESOLUTION = 1024  # per axis (oi_mc_workspace_bytes)


def _axes(bound_min, bound_max, resolution, device):
    """torch.linspace per axis, exactly as renderer.py:17-19 builds them (resolution: int or (nx, ny, nz))."""
    res = (resolution,) * 3 if np.isscalar(resolution) else tuple(resolution)
    bmin = [float(v) for v in (bound_min.tolist() if torch.is_tensor(bound_min) else bound_min)]
    bmax = [float(v) for v in (bound_max.tolist() if torch.is_tensor(bound_max) else bound_max)]
    return [torch.linspace(bmin[a], bmax[a], int(res[a]), device=device) for a in range(3)]


def sdf_lattice(pack, bound_min, bound_max, resolution, z=None, w=None, scale=1.0):
    """(B, nx, ny, nz) CUDA field scale * sdf on the lattice of torch.linspace(bound_min[a], bound_max[a], resolution[a])
    for latents z (B, 64) or style vectors w (B, 64).  `pack`: a ShapeNetwork or a fields.FieldPack (its precision and
    fast_trig).  One launch of oi_sdf_lattice; no graph (the field is not differentiable)."""
    f = LatentField(pack, z, w, "sdf_lattice", need_color=False, batch_ok=True)
    L = _l.load()
    with torch.no_grad():
        f.prepare(z, w)
        xs, ys, zs = _axes(bound_min, bound_max, resolution, f.gamma.device)
        nx, ny, nz = len(xs), len(ys), len(zs)
        out = torch.empty(f.B, nx, ny, nz, dtype=torch.float32, device=f.gamma.device)
        _l.check(L.oi_sdf_lattice(_p(f.packed), _p(f.gamma), _p(f.beta), f.B, _p(xs), _p(ys), _p(zs), nx, ny, nz, float(scale),
                                  _p(out), f.prec, f.fast, _stream()), "oi_sdf_lattice")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the narrow band (include/oi_mesh_band.h)
# ---------------------------------------------------------------------------------------------------------------------
# Bound on |d sdf/dx|: twice the largest gradient norm of the golden field over the box [-1, 1]^3, corners included, rounded up
# to one significant digit (DESIGN 4.14 has the measurement).  The slope guard is the runtime net below it.
DEFAULT_LIPSCHITZ = 20.0
DEFAULT_BLOCK = 4   # 30 % of the points at 512^3 against 71 % for block 8


@dataclasses.dataclass
class BandInfo:
    """What sdf_lattice_band did: blocks of `block` points per axis; active ones went through the MLP, inactive ones hold their
    centre's value, above (u > iso) or below the level; points_evaluated: the coarse pass plus the band launch (ragged ends
    included); max_slope: the largest slope seen between the centres of face-adjacent blocks, a lower bound of the true
    bound on |d sdf/dx|; lipschitz: the bound the call used.  coarse (nbx, nby, nbz): the coarse pass (scale applied);
    active_list (active_blocks,) int32: the ids of the active blocks, in no particular order."""
    block: int
    blocks: int
    active_blocks: int
    inactive_above: int
    inactive_below: int
    points_evaluated: int
    max_slope: float
    lipschitz: float
    coarse: Optional[torch.Tensor] = None
    active_list: Optional[torch.Tensor] = None

    @property
    def inactive_blocks(self):
        return self.inactive_above + self.inactive_below

    @property
    def active_fraction(self):
        return self.active_blocks / max(self.blocks, 1)


def _check_band_args(what, lipschitz, block):
    lipschitz = DEFAULT_LIPSCHITZ if lipschitz is None else lipschitz
    block = DEFAULT_BLOCK if block is None else block
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or int(block) not in (4, 8):
        raise ValueError(f"{what}: block={block!r} (4 or 8)")
    if isinstance(lipschitz, bool) or not isinstance(lipschitz, (int, float, np.integer, np.floating)) or \
            not (float(lipschitz) > 0.0 and np.isfinite(float(lipschitz))):
        raise ValueError(f"{what}: lipschitz={lipschitz!r} (a finite bound > 0 on |d sdf/dx| inside the box)")
    return float(lipschitz), int(block)


def sdf_lattice_band(pack, bound_min, bound_max, resolution, iso, z=None, w=None, scale=1.0, lipschitz=None, block=None):
    """sdf_lattice for marching cubes at level `iso`, with the network evaluated only near that level (the rule is stated in
    include/oi_mesh_band.h): -> (field (1, nx, ny, nz), BandInfo).  The field equals sdf_lattice's bit for bit at every point
    of an active block and holds the block's centre value -- of the same side of iso -- everywhere else, so
    marching_cubes(field[0], iso) is the dense field's mesh, byte for byte, as long as `lipschitz` bounds |d sdf/dx| in the
    box (grown by (block - 1) / 2 cells).  A slope between two block centres above `lipschitz` proves the bound wrong:
    ValueError, no field.  One latent; lipschitz / block default to DEFAULT_LIPSCHITZ / DEFAULT_BLOCK."""
    lipschitz, block = _check_band_args("sdf_lattice_band", lipschitz, block)
    f = LatentField(pack, z, w, "sdf_lattice_band", need_color=False)
    res = (resolution,) * 3 if np.isscalar(resolution) else tuple(resolution)
    nx, ny, nz = (int(r) for r in res)
    if not all(_l.BAND_MIN_RES <= n <= _l.BAND_MAX_RES for n in (nx, ny, nz)):
        raise ValueError(f"sdf_lattice_band: lattice {nx} x {ny} x {nz} (every axis {_l.BAND_MIN_RES}..{_l.BAND_MAX_RES})")
    iso, scale = float(iso), float(scale)
    if not (np.isfinite(iso) and np.isfinite(scale) and scale != 0.0):
        raise ValueError(f"sdf_lattice_band: iso={iso} scale={scale} (finite, scale != 0)")
    bmin = [float(v) for v in _host(bound_min).reshape(-1)]
    bmax = [float(v) for v in _host(bound_max).reshape(-1)]
    h = [abs(bmax[a] - bmin[a]) / (n - 1) for a, n in enumerate((nx, ny, nz))]
    if not all(v > 0.0 and np.isfinite(v) for v in h):
        raise ValueError(f"sdf_lattice_band: empty box {bmin} .. {bmax}")
    L = _l.load()
    with torch.no_grad():
        f.prepare(z, w)
        gamma, beta, packed, dev = f.gamma, f.beta, f.packed, f.gamma.device
        xs, ys, zs = _axes(bmin, bmax, (nx, ny, nz), dev)
        # the coarse pass: index block * i + (block - 1) / 2 per axis, on the line through the axis' end points (float64 on
        # the host, as tests/helpers/band_ref.py builds them)
        nb = [(n + block - 1) // block for n in (nx, ny, nz)]
        cax = [torch.from_numpy((bmin[a] + (block * np.arange(nb[a], dtype=np.float64) + (block - 1) / 2.0) *
                                 ((bmax[a] - bmin[a]) / (n - 1))).astype(np.float32)).to(dev)
               for a, n in enumerate((nx, ny, nz))]
        coarse = torch.empty(nb[0], nb[1], nb[2], dtype=torch.float32, device=dev)
        _l.check(L.oi_sdf_lattice(_p(packed), _p(gamma), _p(beta), 1, _p(cax[0]), _p(cax[1]), _p(cax[2]), nb[0], nb[1], nb[2],
                                  scale, _p(coarse), f.prec, f.fast, _stream()), "oi_sdf_lattice")
        nbytes = L.oi_band_workspace_bytes(nx, ny, nz, block)
        if nbytes == 0:
            msg = L.oi_last_error()
            raise _l.OiHipError(f"sdf_lattice_band: {msg.decode() if msg else 'bad lattice'}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        field = torch.empty(1, nx, ny, nz, dtype=torch.float32, device=dev)
        counts = (ctypes.c_longlong * 4)()
        slope = ctypes.c_float(0.0)
        _l.check(L.oi_band_classify(_p(coarse), 1, nx, ny, nz, block, h[0], h[1], h[2], iso, scale, lipschitz, _p(field),
                                    _p(ws), nbytes, counts, ctypes.byref(slope), _stream()), "oi_band_classify")
        n_active = int(counts[1])
        if not slope.value <= lipschitz:
            raise ValueError(f"sdf_lattice_band: slope {slope.value:.6g} seen between two block centres, above lipschitz="
                             f"{lipschitz:.6g}: the bound on |d sdf/dx| is wrong for this field, no band field is returned "
                             "(pass a larger lipschitz, or band=False)")
        _l.check(L.oi_sdf_lattice_band(_p(packed), _p(gamma), _p(beta), 1, _p(xs), _p(ys), _p(zs), nx, ny, nz, block, _p(ws),
                                       n_active, scale, _p(field), f.prec, f.fast, _stream()), "oi_sdf_lattice_band")
        active_list = ws[:4 * n_active].view(torch.int32)
    info = BandInfo(block, int(counts[0]), n_active, int(counts[2]), int(counts[3]),
                    int(counts[0]) + n_active * block ** 3, float(slope.value), lipschitz, coarse, active_list)
    return field, info


def _level_field(pack, bound_min, bound_max, resolution, threshold, z, w, band, lipschitz, block, what):
    """The field u = -sdf the mesh entries run marching cubes on: dense (band=False, the path they always took) or narrow
    band at the call's threshold.  -> (u (nx, ny, nz), BandInfo or None)."""
    if not band:
        if lipschitz is not None or block is not None:
            raise ValueError(f"{what}: lipschitz= and block= belong to band=True")
        return sdf_lattice(pack, bound_min, bound_max, resolution, z=z, w=w, scale=-1.0)[0], None
    u, info = sdf_lattice_band(pack, bound_min, bound_max, resolution, threshold, z=z, w=w, scale=-1.0, lipschitz=lipschitz,
                               block=block)
    return u[0], info


def marching_cubes(volume, isovalue):
    """Drop-in for mcubes.marching_cubes(volume, isovalue): a point is inside iff volume > isovalue.
    numpy in -> numpy (V, 3) float64 index-space vertices, (F, 3) int64 triangles;
    CUDA tensor in -> CUDA (V, 3) float32, (F, 3) int32 (no host copy of the mesh).  No surface: (0, 3) arrays."""
    as_numpy = not torch.is_tensor(volume)
    if as_numpy:
        u = torch.from_numpy(np.ascontiguousarray(volume, dtype=np.float32)).cuda()
    else:
        if not volume.is_cuda:
            raise _l.OiHipError("marching_cubes: a tensor input must be on the GPU (numpy arrays are copied there)")
        u = volume.detach().float().contiguous()
    if u.dim() != 3:
        raise ValueError(f"marching_cubes: expected a 3-D volume, got shape {tuple(u.shape)}")
    nx, ny, nz = (int(s) for s in u.shape)
    L = _l.load()
    nbytes = L.oi_mc_workspace_bytes(nx, ny, nz)
    if nbytes == 0:  # before any allocation
        msg = L.oi_last_error()
        raise _l.OiHipError(f"marching_cubes: {msg.decode() if msg else 'bad lattice'}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=u.device)
    tot = (ctypes.c_longlong * 3)()
    iso = float(isovalue)
    _l.check(L.oi_mc_count(_p(u), nx, ny, nz, iso, _p(ws), nbytes, tot, _stream()), "oi_mc_count")
    nv, nt = int(tot[0]), int(tot[1])
    verts = torch.empty(nv, 3, dtype=torch.float32, device=u.device)
    tris = torch.empty(nt, 3, dtype=torch.int32, device=u.device)
    if nv > 0 or nt > 0:
        _l.check(L.oi_mc_emit(_p(u), nx, ny, nz, iso, _p(ws), nbytes, ctypes.c_void_p(verts.data_ptr()), nv,
                              ctypes.c_void_p(tris.data_ptr()), nt, _stream()), "oi_mc_emit")
    if as_numpy:
        return verts.cpu().numpy().astype(np.float64), tris.cpu().numpy().astype(np.int64)
    return verts, tris


def extract_fields(bound_min, bound_max, resolution, query_func):
    """The reference's extract_fields (renderer.py:15-31): 64^3 chunks of torch.meshgrid points through query_func
    -> numpy (R, R, R) float32."""
    N = 64
    X, Y, Z = (a.split(N) for a in _axes(bound_min, bound_max, resolution, "cuda"))
    u = np.zeros([resolution, resolution, resolution], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    val = query_func(pts).reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
                    u[xi * N: xi * N + len(xs), yi * N: yi * N + len(ys), zi * N: zi * N + len(zs)] = val
    return u


def to_world(vertices, bound_min, bound_max, resolution):
    """Index space -> world, in float64 on the host (renderer.py:37-40)."""
    b_max = np.asarray(bound_max.detach().cpu().numpy() if torch.is_tensor(bound_max) else bound_max, dtype=np.float64)
    b_min = np.asarray(bound_min.detach().cpu().numpy() if torch.is_tensor(bound_min) else bound_min, dtype=np.float64)
    return vertices / (resolution - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func):
    """The reference's extract_geometry (renderer.py:33-41) with the GPU marching cubes: numpy (V, 3) float64 world-space
    vertices, (F, 3) int64 triangles."""
    u = extract_fields(bound_min, bound_max, resolution, query_func)
    vertices, triangles = marching_cubes(u, threshold)
    return to_world(vertices, bound_min, bound_max, resolution), triangles


RECORD_DTYPE = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])   # OI_MESH_RECORD_BYTES = 27, packed


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def quantise_colours(c):
    """float RGB -> uint8 as the record holds it: round-to-nearest-even of clamp(c, 0, 1) * 255 in float32 (NaN -> 0);
    uint8 input is returned as it is."""
    c = _host(c)
    if c.dtype == np.uint8:
        return c.reshape(-1, 3)
    c = np.nan_to_num(c.astype(np.float32).reshape(-1, 3), nan=0.0)
    return np.rint(np.clip(c, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def save_ply(path, vertices, triangles, normals=None, colors=None):
    """Binary little-endian PLY: float32 x y z per vertex, uchar count + int32 indices per face (numpy only).
    normals (V, 3): adds float nx ny nz; colors (V, 3), float in [0, 1] or uint8: adds uchar red green blue (the property
    names MeshLab and Blender read).  `vertices` may instead be the interleaved record of vertex_attributes(...,
    want_record=True) -- a (V, 27) uint8 tensor or array, x y z nx ny nz r g b -- which is written as it is (one
    device -> host copy, no pass over the vertices on the host); normals and colors must then be None.
    With neither normals nor colors nor a record, the file is what this function always wrote."""
    t = np.asarray(_host(triangles), dtype=np.int64).reshape(-1, 3)
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    v = _host(vertices)
    props = "property float x\nproperty float y\nproperty float z\n"
    p_nrm = "property float nx\nproperty float ny\nproperty float nz\n"
    p_col = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    if v.dtype == np.uint8 and v.ndim == 2 and v.shape[1] == RECORD_DTYPE.itemsize:
        if normals is not None or colors is not None:
            raise ValueError("save_ply: an interleaved vertex record already holds normals and colours")
        nv, body, props = len(v), np.ascontiguousarray(v).tobytes(), props + p_nrm + p_col
    else:
        v = np.ascontiguousarray(np.asarray(v, dtype="<f4").reshape(-1, 3))
        nv = len(v)
        if normals is None and colors is None:
            body = v.tobytes()
        else:
            fields = [("p", "<f4", (3,))]
            cols = {"p": v}
            if normals is not None:
                cols["n"] = np.asarray(_host(normals), dtype="<f4").reshape(-1, 3)
                fields.append(("n", "<f4", (3,)))
                props += p_nrm
            if colors is not None:
                cols["c"] = quantise_colours(colors)
                fields.append(("c", "u1", (3,)))
                props += p_col
            for k, a in cols.items():
                if len(a) != nv:
                    raise ValueError(f"save_ply: {nv} vertices but {len(a)} rows of {'normals' if k == 'n' else 'colors'}")
            rec = np.empty(nv, dtype=np.dtype(fields))   # packed: no padding between the fields
            for k, a in cols.items():
                rec[k] = a
            body = rec.tobytes()
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {nv}\n" + props +
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(body)
        fh.write(faces.tobytes())


# ---------------------------------------------------------------------------------------------------------------------
# the intrinsic mesh (include/oi_mesh_attr.h)
# ---------------------------------------------------------------------------------------------------------------------
MAX_REFINE = _l.MESH_MAX_REFINE


@dataclasses.dataclass
class IntrinsicMesh:
    """The vertex pass's result, CUDA tensors: positions (V, 3) world space, on sdf = -threshold; normals (V, 3) unit
    d sdf/dx (outward); albedo (V, 3) float32 RGB; residual (refine + 1, V): |sdf + threshold| / |d sdf/dx| before each
    Newton step and after the last; flags (V,) uint8 (oi_amd.lib.MESH_FLAG_*: a flagged vertex stopped where it was);
    record (V, 27) uint8 or None: x y z nx ny nz float32 + r g b uint8 per vertex, as save_ply writes it;
    triangles (F, 3) int32 or None (extract_intrinsic_mesh sets it); shaded (V, 3) or None: the vertex colours under a
    light (inference.export_mesh(..., light=...) sets it)."""
    positions: torch.Tensor
    normals: torch.Tensor
    albedo: torch.Tensor
    residual: torch.Tensor
    flags: torch.Tensor
    record: Optional[torch.Tensor] = None
    triangles: Optional[torch.Tensor] = None
    shaded: Optional[torch.Tensor] = None
    band: Optional[BandInfo] = None   # extract_intrinsic_mesh(..., band=True) sets it


def _check_refine(refine, what):
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or not 0 <= int(refine) <= MAX_REFINE:
        raise ValueError(f"{what}: refine={refine!r} (an integer, 0 <= refine <= {MAX_REFINE})")
    return int(refine)


def vertex_attributes(pack_or_generator, vertices_index, bound_min, bound_max, resolution, z=None, w=None, refine=2,
                      threshold=0.0, want_record=False):
    """Index-space marching-cubes vertices (V, 3) (CUDA, as marching_cubes returns them for a field of sdf_lattice on the same
    bounds and resolution) -> IntrinsicMesh: world positions moved onto the level set by `refine` Newton steps
    p <- p - s g / |g|^2 (s = sdf + threshold, g = d sdf/dx), unit normals g / |g| and albedo there.  The mesh is the
    surface u = -sdf = threshold, so the steps go towards sdf = -threshold.  A vertex never moves further than half a lattice
    cell per axis from its marching-cubes position; one that would, or whose sdf / gradient is not finite or whose gradient
    vanishes, stays where it was and is flagged.  refine = 0: the marching-cubes vertices with their attributes.
    Every pass is the full MLP forward (sdf, gradient, albedo) in the pack's precision -- the only pass with a gradient the
    library has; the albedo of the refinement passes is discarded.  One latent: z (1, 64) or w (1, 64)."""
    refine = _check_refine(refine, "vertex_attributes")
    f = LatentField(pack_or_generator, z, w, "vertex_attributes")
    if not torch.is_tensor(vertices_index) or vertices_index.dim() != 2 or vertices_index.shape[1] != 3:
        raise ValueError("vertex_attributes: vertices_index must be a (V, 3) tensor of index-space vertices")
    if not vertices_index.is_cuda:
        raise _l.OiHipError("vertex_attributes: vertices_index must be on the GPU (there is no CPU path)")
    vi = vertices_index.detach().float().contiguous()
    V = vi.shape[0]
    if V >= 1 << 31:
        raise ValueError(f"vertex_attributes: {V} vertices (at most 2^31 - 1)")
    dev = vi.device
    if V == 0:   # a field without a crossing: nothing is launched
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
        return IntrinsicMesh(e(0, 3), e(0, 3), e(0, 3), e(refine + 1, 0), e(0, dt=torch.uint8),
                             e(0, RECORD_DTYPE.itemsize, dt=torch.uint8) if want_record else None)
    with torch.no_grad():
        f.prepare(z, w)
        xs, ys, zs = _axes(bound_min, bound_max, resolution, dev)
        bmin, bmax = ([float(v) for v in _host(b).reshape(-1)] for b in (bound_min, bound_max))
        limits = [0.5 * (bmax[a] - bmin[a]) / (len(x) - 1) for a, x in enumerate((xs, ys, zs))]
        pos, flags = ops.mesh_vertex_world(vi, xs, ys, zs)
        pos0 = pos.clone() if refine else pos
        residual = ops._new(pos, refine + 1, V)
        scratch = torch.empty(ops.mlp_scratch_bytes(1, V, f.prec), dtype=torch.uint8, device=dev)
        for k in range(refine):
            sdf, grad, _ = f.full(pos, scratch)
            ops.mesh_newton(pos, pos0, sdf, grad, threshold, limits, residual[k], flags)
        sdf, grad, rgb = f.full(pos, scratch)
        normals, albedo, record = ops.mesh_attr_finalize(pos, sdf, grad, rgb, threshold, residual[refine], want_record)
    return IntrinsicMesh(pos, normals, albedo, residual, flags, record)


def extract_intrinsic_mesh(renderer_or_generator, z=None, w=None, resolution=256, threshold=0.0,
                           bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), refine=2, want_record=False, band=False,
                           lipschitz=None, block=None):
    """sdf_lattice -> marching_cubes -> vertex_attributes, nothing on the host in between except the mesh's sizes.
    band=True: the field comes from sdf_lattice_band at `threshold` (lipschitz, block: its arguments) -- the same mesh from
    fewer MLP evaluations; the BandInfo is returned in .band.
    -> IntrinsicMesh with triangles (F, 3) int32, the array marching_cubes returns for the same field.  The mesh is the level
    set u = -sdf = threshold (extract_geometry's convention): with threshold != 0 the vertices are refined towards
    sdf = -threshold."""
    refine = _check_refine(refine, "extract_intrinsic_mesh")
    pack = LatentField(renderer_or_generator, z, w, "extract_intrinsic_mesh").pack
    u, info = _level_field(pack, bound_min, bound_max, resolution, threshold, z, w, band, lipschitz, block,
                           "extract_intrinsic_mesh")
    vi, tris = marching_cubes(u, threshold)
    del u
    out = vertex_attributes(pack, vi, bound_min, bound_max, resolution, z=z, w=w, refine=refine, threshold=threshold,
                            want_record=want_record)
    out.triangles = tris
    out.band = info
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the textured mesh (include/oi_mesh_tex.h)
# ---------------------------------------------------------------------------------------------------------------------
DEFAULT_TEXEL = 8
DEFAULT_MAX_TEXELS = 1 << 20


@dataclasses.dataclass
class TexturedMesh:
    """An intrinsic mesh with a per-triangle texture atlas (include/oi_mesh_tex.h has the layout): mesh: the IntrinsicMesh it
    was built on (positions, normals, triangles); uv (F, 3, 2): texture coordinates per corner, OBJ convention (v up);
    albedo_map, normal_map (H, W, 3) uint8: the baked colour and the object-space normal n * 0.5 + 0.5, row 0 on top;
    albedo_f32, normal_f32 (H, W, 3) float32 or None (want_float=True): the values before quantisation (unowned pixels: 0
    and 0.5); texel: the texel size T of a triangle; size = (W, H); texel_flags (F, n_T) uint8 and texel_residual (F, n_T):
    the flags (oi_amd.lib.MESH_FLAG_*) and the last residual |sdf + threshold| / |d sdf/dx| of every texel's projection;
    texel_positions (F, n_T, 3) or None (keep_points=True): the final points.  A bilinear lookup inside a triangle's UV
    triangle reads that triangle's texels only; mip levels above 0 bleed into the neighbours, as in every per-triangle atlas."""
    mesh: IntrinsicMesh
    uv: torch.Tensor
    albedo_map: torch.Tensor
    normal_map: torch.Tensor
    texel: int
    size: tuple
    texel_flags: torch.Tensor
    texel_residual: torch.Tensor
    albedo_f32: Optional[torch.Tensor] = None
    normal_f32: Optional[torch.Tensor] = None
    texel_positions: Optional[torch.Tensor] = None


def _check_max_texels(max_texels, what):
    if isinstance(max_texels, bool) or not isinstance(max_texels, (int, np.integer)) or not 1 <= int(max_texels) < 1 << 31:
        raise ValueError(f"{what}: max_texels={max_texels!r} (an integer, 1 <= max_texels < 2^31)")
    return int(max_texels)


def bake_textures(pack_or_generator, mesh, bound_min, bound_max, resolution, z=None, w=None, texel=DEFAULT_TEXEL, refine=2,
                  threshold=0.0, max_texels=DEFAULT_MAX_TEXELS, want_float=False, keep_points=False, shade=None):
    """The atlas of an IntrinsicMesh with triangles (extract_intrinsic_mesh's result; bounds, resolution, latent and
    threshold as it was extracted with) -> TexturedMesh.  Every texel of every triangle is a point in the triangle's plane
    (gutter texels past the hypotenuse are extrapolated, not clamped), projected onto the level set by `refine` Newton steps
    limited to half a lattice cell per axis around the planar point -- the vertex pass's own rule and kernels -- and the unit
    normal and the albedo there go to the texel's pixel.  Chunks of whole triangles, max(1, max_texels // n_T) at a time:
    oi_tex_points, (full MLP pass + oi_mesh_newton) x refine, the full pass, oi_mesh_attr_finalize, oi_tex_store.  Texels are
    independent, so any max_texels gives the same bytes.  shade(points, normals, albedo) -> (n, 3) colours, optional: what the
    albedo maps hold instead of the albedo (inference.export_mesh(..., light=...) passes shade_vertices).
    F == 0: nothing is launched, the atlases are the filled (texel, texel + 1, 3) images.  One latent."""
    what = "bake_textures"
    tris = mesh.triangles
    if tris is None or not torch.is_tensor(tris) or tris.dim() != 2 or tris.shape[1] != 3:
        raise ValueError(f"{what}: the mesh needs its (F, 3) triangles (extract_intrinsic_mesh sets them)")
    F, V = int(tris.shape[0]), int(mesh.positions.shape[0])
    try:
        W, H, _ = ops.tex_layout(F, texel)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None
    T = int(texel)
    nT = T * (T + 1) // 2
    refine = _check_refine(refine, what)
    max_texels = _check_max_texels(max_texels, what)
    f = LatentField(pack_or_generator, z, w, what)
    if F and (int(tris.min()) < 0 or int(tris.max()) >= V):
        raise ValueError(f"{what}: triangles index {int(tris.min())} .. {int(tris.max())}, the mesh has {V} vertices")
    pos_v = mesh.positions
    if not pos_v.is_cuda:
        raise _l.OiHipError(f"{what}: the mesh must be on the GPU (there is no CPU path)")
    dev = pos_v.device
    fill = lambda t, v: t.fill_(v)
    albedo_u8 = fill(ops._bytes(pos_v, H * W * 3).view(H, W, 3), 0)
    normal_u8 = fill(ops._bytes(pos_v, H * W * 3).view(H, W, 3), 128)
    albedo_f32 = fill(ops._new(pos_v, H, W, 3), 0.0) if want_float else None
    normal_f32 = fill(ops._new(pos_v, H, W, 3), 0.5) if want_float else None
    flags = ops._bytes(pos_v, F * nT)
    residual = ops._new(pos_v, F * nT)
    points = ops._new(pos_v, F * nT, 3) if keep_points else None
    out = TexturedMesh(mesh, None, albedo_u8, normal_u8, T, (W, H), flags.view(F, nT), residual.view(F, nT), albedo_f32,
                       normal_f32, points.view(F, nT, 3) if keep_points else None)
    if F == 0:
        out.uv = torch.empty(0, 3, 2, dtype=torch.float32, device=dev)
        return out
    with torch.no_grad():
        f.prepare(z, w)
        pos_v = pos_v.detach().float().contiguous()
        tris = tris.detach().to(torch.int32).contiguous()
        out.uv = ops.tex_uv(F, T, pos_v)
        bmin, bmax = ([float(v) for v in _host(b).reshape(-1)] for b in (bound_min, bound_max))
        res = (resolution,) * 3 if np.isscalar(resolution) else tuple(resolution)
        limits = [0.5 * (bmax[a] - bmin[a]) / (int(res[a]) - 1) for a in range(3)]
        nf_max = min(F, max(1, max_texels // nT))
        buf = None if keep_points else ops._new(pos_v, nf_max * nT, 3)
        buf0 = ops._new(pos_v, nf_max * nT, 3) if refine else None
        scratch = torch.empty(ops.mlp_scratch_bytes(1, nf_max * nT, f.prec), dtype=torch.uint8, device=dev)
        for f0 in range(0, F, nf_max):
            nf = min(nf_max, F - f0)
            a, b = f0 * nT, (f0 + nf) * nT
            pts, fl = ops.tex_points(pos_v, tris, f0, nf, T, out=points[a:b] if keep_points else buf, flags=flags[a:b])
            if refine:
                pts0 = buf0[:b - a].copy_(pts)
                for _ in range(refine):
                    sdf, grad, _ = f.full(pts, scratch)
                    ops.mesh_newton(pts, pts0, sdf, grad, threshold, limits, None, fl)
            sdf, grad, rgb = f.full(pts, scratch)
            normals, albedo, _ = ops.mesh_attr_finalize(pts, sdf, grad, rgb, threshold, residual[a:b])
            if shade is not None:
                albedo = shade(pts, normals, albedo).contiguous()
            ops.tex_store(normals, albedo, f0, nf, T, F, albedo_f32, normal_f32, albedo_u8, normal_u8)
    return out


def extract_textured_mesh(renderer_or_generator, z=None, w=None, resolution=64, texel=DEFAULT_TEXEL, threshold=0.0,
                          bound_min=(-1.0, -1.0, -1.0), bound_max=(1.0, 1.0, 1.0), refine=2, band=False, lipschitz=None,
                          block=None, max_texels=DEFAULT_MAX_TEXELS, want_float=False, keep_points=False, shade=None):
    """extract_intrinsic_mesh (band, lipschitz, block: its arguments) followed by bake_textures: a coarse mesh whose texture
    carries the detail of the albedo and of the analytic normal field -> TexturedMesh (save_obj writes it)."""
    what = "extract_textured_mesh"
    try:
        ops.tex_layout(0, texel)      # the texel size, before anything is launched
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None
    _check_max_texels(max_texels, what)
    m = extract_intrinsic_mesh(renderer_or_generator, z=z, w=w, resolution=resolution, threshold=threshold,
                               bound_min=bound_min, bound_max=bound_max, refine=refine, band=band, lipschitz=lipschitz,
                               block=block)
    pack = LatentField(renderer_or_generator, z, w, what).pack
    return bake_textures(pack, m, bound_min, bound_max, resolution, z=z, w=w, texel=texel, refine=refine,
                         threshold=threshold, max_texels=max_texels, want_float=want_float, keep_points=keep_points,
                         shade=shade)


PNG_COMPRESSION = 6   # fixed: the same image gives the same bytes


def save_png(path, image_u8):
    """8-bit RGB PNG of an (H, W, 3) uint8 image (tensor or array), row 0 on top, with zlib and struct alone: one IDAT chunk,
    filter type 0 on every row, compression level PNG_COMPRESSION.  The same input gives the same bytes."""
    import struct
    import zlib
    img = _host(image_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"save_png: expected an (H, W, 3) uint8 image, got {img.dtype} {tuple(img.shape)}")
    H, W = img.shape[:2]
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)   # filter byte 0, then the row
    rows[:, 1:] = img.reshape(H, 3 * W)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
                 chunk(b"IDAT", zlib.compress(rows.tobytes(), PNG_COMPRESSION)) + chunk(b"IEND", b""))


def obj_file_names(path):
    """The four files of save_obj(path, ...), and the stem they share without its folder: (obj, mtl, albedo png, normal png,
    stem).  ValueError unless path ends in .obj."""
    import os
    if not str(path).lower().endswith(".obj"):
        raise ValueError(f"save_obj: {path!r} must end in .obj")
    stem = str(path)[:-4]
    return str(path), stem + ".mtl", stem + "_albedo.png", stem + "_normal.png", os.path.basename(stem)


def save_obj(path, textured_mesh, light_map=None):
    """Wavefront OBJ of a TexturedMesh, four files: `path` (<stem>.obj) with v and vn per vertex, vt per corner (3 F of them)
    and f a/ta/a b/tb/b c/tc/c, 1-based, floats as %.9g (float32 values round-trip exactly); <stem>.mtl with newmtl intrinsic,
    Kd 1 1 1, map_Kd <stem>_albedo.png and norm <stem>_normal.png; and the two PNGs (save_png).  light_map (H, W, 3) uint8,
    optional: the image written as <stem>_albedo.png instead of the albedo map (e.g. a shaded one)."""
    obj, mtl, png_a, png_n, stem = obj_file_names(path)
    tm = textured_mesh
    v = np.asarray(_host(tm.mesh.positions), dtype=np.float32).reshape(-1, 3)
    n = np.asarray(_host(tm.mesh.normals), dtype=np.float32).reshape(-1, 3)
    t = np.asarray(_host(tm.mesh.triangles), dtype=np.int64).reshape(-1, 3)
    uv = np.asarray(_host(tm.uv), dtype=np.float32).reshape(-1, 2)
    if len(uv) != 3 * len(t) or len(n) != len(v):
        raise ValueError(f"save_obj: {len(t)} triangles but {len(uv)} texture coordinates, {len(v)} vertices but {len(n)} normals")
    g = lambda x: "%.9g" % x
    lines = [f"mtllib {stem}.mtl", "usemtl intrinsic"]
    lines += ["v " + " ".join(map(g, r)) for r in v.tolist()]
    lines += ["vn " + " ".join(map(g, r)) for r in n.tolist()]
    lines += ["vt " + " ".join(map(g, r)) for r in uv.tolist()]
    lines += ["f " + " ".join(f"{a + 1}/{3 * k + m + 1}/{a + 1}" for m, a in enumerate(r)) for k, r in enumerate(t.tolist())]
    with open(obj, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(mtl, "w") as fh:
        fh.write(f"newmtl intrinsic\nKd 1 1 1\nmap_Kd {stem}_albedo.png\nnorm {stem}_normal.png\n")
    save_png(png_a, tm.albedo_map if light_map is None else light_map)
    save_png(png_n, tm.normal_map)


def load_png(path):
    """The (H, W, 3) uint8 numpy image of a PNG as save_png writes it: 8-bit RGB, non-interlaced, filter type 0 on every row,
    with zlib and struct alone.  Anything else -- another bit depth or colour type, an interlaced image, a filtered row, a
    damaged chunk -- is refused by name."""
    import struct
    import zlib
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"load_png: {path!r} is not a PNG file")
    at, head, idat, ended = 8, None, b"", False
    while at + 12 <= len(data) and not ended:
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if len(body) != n or at + 12 + n > len(data) or struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(tag + body) & 0xffffffff:
            raise ValueError(f"load_png: {path!r}: chunk {tag!r} is truncated or fails its CRC")
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            ended = True
        elif not tag[:1].islower():   # (an ancillary chunk may be skipped, a critical one may not)
            raise ValueError(f"load_png: {path!r}: critical chunk {tag!r} is not supported")
        at += 12 + n
    if head is None or not ended:
        raise ValueError(f"load_png: {path!r} has no IHDR or no IEND chunk")
    W, H, depth, colour, comp, filt, interlace = head
    if depth != 8:
        raise ValueError(f"load_png: {path!r} has bit depth {depth} (8-bit only)")
    if colour != 2:
        raise ValueError(f"load_png: {path!r} has colour type {colour} (2, RGB, only)")
    if interlace != 0:
        raise ValueError(f"load_png: {path!r} is interlaced (non-interlaced only)")
    if comp != 0 or filt != 0 or W < 1 or H < 1:
        raise ValueError(f"load_png: {path!r}: compression {comp}, filter method {filt}, size {W} x {H}")
    raw = zlib.decompress(idat)
    if len(raw) != H * (1 + 3 * W):
        raise ValueError(f"load_png: {path!r} holds {len(raw)} bytes, {H * (1 + 3 * W)} expected for {W} x {H} RGB")
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    if rows[:, 0].any():
        raise ValueError(f"load_png: {path!r}: row filter type {int(rows[:, 0].max())} (save_png writes type 0 on every row)")
    return rows[:, 1:].reshape(H, W, 3).copy()


def load_obj(path, device=None):
    """The TexturedMesh of the four files save_obj writes, and only those: <stem>.obj with mtllib, usemtl, v, vn, vt and
    f a/ta/a b/tb/b c/tc/c (1-based; the normal's index is the vertex's), <stem>.mtl with newmtl, Kd, map_Kd and norm, and the
    two PNGs (load_png), next to the OBJ.  Any other statement or face form is refused by name.  -> TexturedMesh on `device`
    (default cuda when there is one): mesh.positions, mesh.normals (V, 3), mesh.triangles (F, 3) int32, uv (F, 3, 2),
    albedo_map, normal_map (H, W, 3) uint8, size (W, H); what a file does not hold is None (mesh.albedo, residual, flags, the
    texel size, texel_flags, texel_residual)."""
    import os
    obj = obj_file_names(path)[0]
    dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    v, vn, vt, faces, mtllib = [], [], [], [], None
    with open(obj) as fh:
        for no, line in enumerate(fh, 1):
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] == "mtllib" and len(w) == 2:
                mtllib = w[1]
            elif w[0] == "usemtl" and len(w) == 2:
                pass
            elif w[0] in ("v", "vn") and len(w) == 4:
                (v if w[0] == "v" else vn).append([float(x) for x in w[1:]])
            elif w[0] == "vt" and len(w) == 3:
                vt.append([float(x) for x in w[1:]])
            elif w[0] == "f" and len(w) == 4:
                c = [x.split("/") for x in w[1:]]
                if any(len(x) != 3 or x[0] != x[2] or not (x[0].isdigit() and x[1].isdigit()) for x in c):
                    raise ValueError(f"load_obj: {obj}:{no}: face {line.strip()!r} (only v/vt/vn corners with vn == v)")
                faces.append([[int(x[0]) - 1, int(x[1]) - 1] for x in c])
            else:
                raise ValueError(f"load_obj: {obj}:{no}: unsupported statement {line.strip()!r}")
    if mtllib is None:
        raise ValueError(f"load_obj: {obj} names no material library (mtllib)")
    maps = {}
    folder = os.path.dirname(obj)
    with open(os.path.join(folder, mtllib)) as fh:
        for no, line in enumerate(fh, 1):
            w = line.split()
            if not w or w[0].startswith("#") or w[0] in ("newmtl", "Kd"):
                continue
            if w[0] in ("map_Kd", "norm") and len(w) == 2:
                maps[w[0]] = w[1]
            else:
                raise ValueError(f"load_obj: {mtllib}:{no}: unsupported statement {line.strip()!r}")
    if set(maps) != {"map_Kd", "norm"}:
        raise ValueError(f"load_obj: {mtllib} must name map_Kd and norm, has {sorted(maps)}")
    albedo, normal = (load_png(os.path.join(folder, maps[k])) for k in ("map_Kd", "norm"))
    if albedo.shape != normal.shape:
        raise ValueError(f"load_obj: the maps differ in size: {albedo.shape[:2]} and {normal.shape[:2]}")
    if len(vn) != len(v):
        raise ValueError(f"load_obj: {len(v)} vertices but {len(vn)} normals")
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3, 2)
    if len(f) and (f.min() < 0 or f[..., 0].max() >= len(v) or f[..., 1].max() >= len(vt)):
        raise ValueError(f"load_obj: {obj}: a face index lies outside the {len(v)} vertices or {len(vt)} texture coordinates")
    t32 = lambda a, *sh: torch.from_numpy(np.asarray(a, dtype=np.float32).reshape(*sh)).to(dev)
    uv = np.asarray(vt, dtype=np.float32).reshape(-1, 2)[f[..., 1]] if len(f) else np.zeros((0, 3, 2), dtype=np.float32)
    m = IntrinsicMesh(t32(v, -1, 3), t32(vn, -1, 3), None, None, None,
                      triangles=torch.from_numpy(f[..., 0].astype(np.int32).reshape(-1, 3)).to(dev))
    return TexturedMesh(m, t32(uv, -1, 3, 2), torch.from_numpy(albedo).to(dev), torch.from_numpy(normal).to(dev), None,
                        (albedo.shape[1], albedo.shape[0]), None, None)
