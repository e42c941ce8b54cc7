"""Mesh extraction -- drop-in for the reference's extract_fields / extract_geometry
(src/third_party/neus/models/renderer.py:15-41) and for mcubes.marching_cubes (PyMCubes), which is not part of this stack.

    sdf_lattice      dense SDF field of a latent on a lattice   oi_sdf_lattice   (the points are never materialised)
    marching_cubes   triangle mesh of a field                   oi_mc_count + oi_mc_emit
    extract_fields / extract_geometry   the reference's functions with a caller-supplied query_func (64^3 chunks)
    save_ply         binary little-endian PLY with numpy only

DESIGN section 4.10 has the table rule, the output order and the measured numbers."""
import ctypes

import numpy as np
import torch

from . import lib as _l
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
    from .fields import FieldPack
    if not isinstance(pack, FieldPack):
        pack = pack._own_pack()
    if z is None and w is None:
        raise ValueError("sdf_lattice: a latent z or a style vector w is needed")
    L = _l.load()
    with torch.no_grad():
        w_, gamma, beta = pack.film(z=z if w is None else None, w=w)
        B = w_.shape[0]
        xs, ys, zs = _axes(bound_min, bound_max, resolution, gamma.device)
        nx, ny, nz = len(xs), len(ys), len(zs)
        out = torch.empty(B, nx, ny, nz, dtype=torch.float32, device=gamma.device)
        _l.check(L.oi_sdf_lattice(_p(pack.packed()), _p(gamma.contiguous()), _p(beta.contiguous()), B, _p(xs), _p(ys),
                                  _p(zs), nx, ny, nz, float(scale), _p(out), pack.prec, int(bool(pack.fast_trig)), _stream()),
                 "oi_sdf_lattice")
    return out


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


def save_ply(path, vertices, triangles):
    """Binary little-endian PLY: float32 x y z per vertex, uchar count + int32 indices per face (numpy only)."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype="<f4").reshape(-1, 3))
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    faces = np.empty(len(t), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = t
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {len(t)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        fh.write(v.tobytes())
        fh.write(faces.tobytes())
