"""fp64 CPU restatement of the intrinsic-mesh vertex pass (include/oi_mesh_attr.h) on the oracle's
field (oracle/oi_oracle.py: FiLM-SIREN sdf, analytic gradient, colour head), and the REHEARSAL of its safeguards:

    field on the lattice (oracle, float64)  ->  tests/helpers/mc_numpy.py  ->  index-space vertices to world through the
    axis arrays  ->  `refine` Newton steps p <- p - s g / max(|g|^2, eps), s = sdf + threshold, with the half-cell limit and
    the flags of the kernel  ->  unit normals g / |g| and albedo.

`rehearsal` reports, for the reference alone: how many vertices were flagged, how the residual |s| / |g| falls per step,
and on how many faces (above the area floor) the winding and the summed vertex normals disagree.  Nothing here touches the
code under test."""
import os

import numpy as np
import torch

import oi_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")

FLAG_NONFINITE, FLAG_SMALL_GRADIENT, FLAG_LIMIT = 1, 2, 4   # OI_MESH_FLAG_* of include/oi_mesh_attr.h
GRAD_EPS = 1e-12                                            # OI_MESH_GRAD_EPS: on |g|^2
AREA_FLOOR = 0.01                                           # faces below 1 % of the median area are not judged
RECORD_DTYPE = np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))])   # 27 bytes, packed


def golden_state(dtype=torch.float64):
    """(sdf state dict, colour state dict) of tests/golden in `dtype`."""
    out = []
    for name in ("weights_sdf", "weights_color"):
        with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
            out.append({k: torch.from_numpy(np.asarray(f[k])).to(dtype) for k in f.files})
    return tuple(out)


def latent(seed, B=1):
    return torch.randn(B, 64, generator=torch.Generator().manual_seed(seed))


def field(sd, csd, w, pts, chunk=1 << 16):
    """Oracle sdf (n,), gradient (n, 3), albedo (n, 3) at pts (n, 3), float64 numpy; csd None: no albedo."""
    pts = torch.as_tensor(np.asarray(pts), dtype=torch.float64).reshape(-1, 3)
    s, g, c = [], [], []
    with torch.no_grad():
        for i in range(0, len(pts), chunk):
            sdf, feat, grad = O.sdf_forward(sd, pts[i:i + chunk], w, want_grad=True)
            s.append(sdf.squeeze(-1))
            g.append(grad)
            if csd is not None:
                c.append(O.color_head(csd, feat, grad, w))
    cat = lambda v: torch.cat(v).numpy() if v else np.zeros((0,))
    return cat(s).reshape(-1), cat(g).reshape(-1, 3), (cat(c).reshape(-1, 3) if csd is not None else None)


def axes(bmin, bmax, res):
    """The float32 axis arrays the library is given (torch.linspace, renderer.py:17-19), as float64 numpy."""
    res = (res,) * 3 if np.isscalar(res) else tuple(res)
    return [torch.linspace(float(bmin[a]), float(bmax[a]), int(res[a])).double().numpy() for a in range(3)]


def vertex_world(verts_index, ax):
    """oi_mesh_vertex_world: per axis i = floor(c), t = c - i; x[i] when t == 0, else x[i] + t (x[i + 1] - x[i])."""
    v = np.asarray(verts_index, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(v)
    for a in range(3):
        x = ax[a]
        i = np.clip(np.floor(v[:, a]).astype(np.int64), 0, len(x) - 1)
        t = v[:, a] - i
        j = np.minimum(i + 1, len(x) - 1)
        out[:, a] = np.where(t == 0, x[i], x[i] + t * (x[j] - x[i]))
    return out


def half_cell(ax):
    return np.array([0.5 * (x[-1] - x[0]) / (len(x) - 1) for x in ax])


def newton_step(p, p0, s, g, limit):
    """One step of oi_mesh_newton: -> (new positions, residual before the step, flag bits of this step)."""
    g2 = (g * g).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        res = np.abs(s) / np.sqrt(g2)
    flags = np.zeros(len(p), dtype=np.uint8)
    flags[~(np.isfinite(s) & np.isfinite(g).all(-1))] |= FLAG_NONFINITE
    flags[(flags == 0) & (g2 < GRAD_EPS)] |= FLAG_SMALL_GRADIENT
    with np.errstate(invalid="ignore", over="ignore"):
        cand = p - (s / np.maximum(g2, GRAD_EPS))[:, None] * g
        over = (flags == 0) & ~(np.abs(cand - p0) <= limit[None, :]).all(-1)
    flags[over] |= FLAG_LIMIT
    return np.where((flags == 0)[:, None], cand, p), res, flags


def refine_vertices(fn, p0, limit, threshold, refine):
    """fn(p) -> (sdf, grad, albedo).  -> positions, (sdf, grad, albedo) there, residual (refine + 1, V), flags (V,)."""
    p, flags, rows = p0.copy(), np.zeros(len(p0), dtype=np.uint8), []
    for _ in range(refine):
        s, g, _ = fn(p)
        p, res, f = newton_step(p, p0, s + threshold, g, limit)
        rows.append(res)
        flags |= f
    s, g, c = fn(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        rows.append(np.abs(s + threshold) / np.sqrt((g * g).sum(-1)))
    return p, (s, g, c), np.stack(rows), flags


def unit(g, eps=1e-6):
    return g / np.maximum(np.linalg.norm(g, axis=-1, keepdims=True), eps)


def winding_disagreements(pos, tris, normals, floor=AREA_FLOOR):
    """-> (faces judged, faces with ((v1 - v0) x (v2 - v0)) . (n0 + n1 + n2) <= 0) among the faces whose area is at least
    `floor` x the median face area."""
    t = np.asarray(tris, dtype=np.int64)
    if len(t) == 0:
        return 0, 0
    v = np.asarray(pos, dtype=np.float64)[t]
    cr = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    area = 0.5 * np.linalg.norm(cr, axis=-1)
    keep = area >= floor * np.median(area)
    dots = (cr * np.asarray(normals, dtype=np.float64)[t].sum(1)).sum(-1)
    return int(keep.sum()), int((dots[keep] <= 0).sum())


def rehearsal(seed, R, threshold=0.0, refine=2, bmin=(-1.0,) * 3, bmax=(1.0,) * 3):
    """The whole pass on the reference in float64.  -> dict of counts and medians (see the module docstring)."""
    import helpers.mc_numpy as M
    sd, csd = golden_state()
    w = O.style_mlp(sd, latent(seed).double())
    ax = axes(bmin, bmax, R)
    xx, yy, zz = np.meshgrid(*ax, indexing="ij")
    u = -field(sd, None, w, np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1))[0].reshape(xx.shape)
    vi, tris = M.marching_cubes(u, threshold)
    p0 = vertex_world(vi, ax)
    fn = lambda p: field(sd, csd, w, p)
    p, (s, g, c), res, flags = refine_vertices(fn, p0, half_cell(ax), threshold, refine)
    judged, bad = winding_disagreements(p, tris, unit(g))
    j0, bad0 = winding_disagreements(p0, tris, unit(fn(p0)[1]))
    return {"seed": seed, "R": R, "threshold": threshold, "refine": refine, "V": len(p0), "F": len(tris),
            "flagged": int((flags != 0).sum()), "flag_bits": int(np.bitwise_or.reduce(flags)) if len(flags) else 0,
            "residual_median": [float(np.median(r)) for r in res], "residual_max": [float(r.max()) for r in res],
            "min_grad_norm": float(np.linalg.norm(g, axis=-1).min()),
            "max_shift_cells": float((np.abs(p - p0) / half_cell(ax)[None]).max() * 0.5),
            "faces_judged": judged, "faces_disagree": bad, "faces_disagree_refine0": bad0}


def read_ply(path):
    """A reader of the binary little-endian PLY files save_ply writes, from the header alone.  -> (vertex structured array
    with one field per property, (F, 3) int32 triangles, [(name, type)] of the vertex properties)."""
    types = {"float": "<f4", "uchar": "u1", "int": "<i4", "double": "<f8"}
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    elements, cur = [], None
    for ln in lines[2:]:
        tok = ln.split()
        if tok[:1] == ["element"]:
            cur = {"name": tok[1], "count": int(tok[2]), "props": []}
            elements.append(cur)
        elif tok[:1] == ["property"]:
            cur["props"].append(tuple(tok[1:]))
    assert [e["name"] for e in elements] == ["vertex", "face"], elements
    ve, fe = elements
    props = [(p[1], p[0]) for p in ve["props"]]
    vdt = np.dtype([(n, types[t]) for n, t in props])
    assert fe["props"] == [("list", "uchar", "int", "vertex_indices")], fe["props"]
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    nvb, nfb = ve["count"] * vdt.itemsize, fe["count"] * fdt.itemsize
    assert len(data) == end + nvb + nfb, (len(data), end, nvb, nfb)
    verts = np.frombuffer(data, dtype=vdt, count=ve["count"], offset=end)
    faces = np.frombuffer(data, dtype=fdt, count=fe["count"], offset=end + nvb)
    assert (faces["n"] == 3).all()
    return verts, faces["i"].copy(), props
