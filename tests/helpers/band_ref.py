"""fp64 numpy restatement of the narrow-band rule of include/oi_mesh_band.h, on any callable field.

    u = scale * f;  inside iff u > iso;  blocks of b points per axis (the last may be ragged);  one coarse value uc per block at
    index b i + (b - 1) / 2 per axis, on the line through the axis' end points;  a block is INACTIVE iff uc is finite and
    |uc - iso| > |scale| G m,  m = sqrt(hx^2 + hy^2 + hz^2) (1 + (b - 1) / 2);  the band field holds u in active blocks and uc
    in inactive ones;  the guard is the largest |uc_a - uc_b| / (|scale| b h_axis) over face-adjacent blocks with finite values.

Nothing here touches the code under test.  `f` is called as f(P) with P (n, 3) float64 world points -> (n,) values."""
import numpy as np


def _res(res):
    return (int(res),) * 3 if np.isscalar(res) else tuple(int(r) for r in res)


def spacings(bmin, bmax, res):
    """Axis spacings (hx, hy, hz) of the lattice of torch.linspace(bmin[a], bmax[a], res[a]), float64."""
    res = _res(res)
    return np.array([abs(float(bmax[a]) - float(bmin[a])) / (res[a] - 1) for a in range(3)], dtype=np.float64)


def axes(bmin, bmax, res):
    res = _res(res)
    return [np.linspace(float(bmin[a]), float(bmax[a]), res[a]) for a in range(3)]


def n_blocks(res, b):
    return tuple((r + b - 1) // b for r in _res(res))


def centre_axes(bmin, bmax, res, b):
    """World coordinate of index b i + (b - 1) / 2 per axis (beyond the last lattice point for a ragged last block)."""
    res = _res(res)
    out = []
    for a in range(3):
        idx = b * np.arange((res[a] + b - 1) // b, dtype=np.float64) + (b - 1) / 2.0
        out.append(float(bmin[a]) + idx * ((float(bmax[a]) - float(bmin[a])) / (res[a] - 1)))
    return out


def distance_bound(h, b):
    """m: one cell diagonal (a corner of a crossed cell to the surface) plus (b - 1) / 2 cell diagonals (a point of a block to
    the block's centre)."""
    h = np.asarray(h, dtype=np.float64)
    return float(np.sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]) * (1.0 + (b - 1) / 2.0))


def grid_points(ax):
    xx, yy, zz = np.meshgrid(*ax, indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1)


def classify(uc, iso, scale, G, h, b):
    """uc (nbx, nby, nbz): the coarse values (scale applied).  -> dict: inactive (bool array), blocks, active,
    inactive_above (uc > iso), inactive_below, max_slope."""
    uc = np.asarray(uc, dtype=np.float64)
    thr = abs(float(scale)) * float(G) * distance_bound(h, b)
    fin = np.isfinite(uc)
    with np.errstate(invalid="ignore"):
        inactive = fin & (np.abs(uc - float(iso)) > thr)
        above = inactive & (uc > float(iso))
    slope = 0.0
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        ua, ub = uc[tuple(lo)], uc[tuple(hi)]
        ok = np.isfinite(ua) & np.isfinite(ub)
        if ok.any():
            slope = max(slope, float((np.abs(ua[ok] - ub[ok]) / (abs(float(scale)) * b * float(h[a]))).max()))
    return {"inactive": inactive, "blocks": int(uc.size), "active": int(uc.size - inactive.sum()),
            "inactive_above": int(above.sum()), "inactive_below": int(inactive.sum() - above.sum()), "max_slope": slope,
            "threshold": thr}


def expand(per_block, res, b):
    """A per-block array -> per lattice point (ragged last blocks cut)."""
    res = _res(res)
    out = np.asarray(per_block)
    for a in range(3):
        out = np.repeat(out, b, axis=a)
    return out[:res[0], :res[1], :res[2]]


def crossed_corners(u, iso):
    """bool (nx, ny, nz): the point is a corner of a cell whose corners do not all lie on one side of iso (u > iso)."""
    inside = np.asarray(u) > iso
    nx, ny, nz = inside.shape
    cnt = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cnt += inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    crossed = (cnt > 0) & (cnt < 8)
    out = np.zeros(inside.shape, dtype=bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        out[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz] |= crossed
    return out


def band(f, bmin, bmax, res, iso, scale, G, b):
    """The whole rule on a callable field, dense evaluation included (small lattices).  -> dict: dense (nx, ny, nz) u,
    field (the band field), uc, and classify()'s entries."""
    res = _res(res)
    ax = axes(bmin, bmax, res)
    dense = float(scale) * np.asarray(f(grid_points(ax)), dtype=np.float64).reshape(res)
    cax = centre_axes(bmin, bmax, res, b)
    uc = float(scale) * np.asarray(f(grid_points(cax)), dtype=np.float64).reshape([len(c) for c in cax])
    out = classify(uc, iso, scale, G, spacings(bmin, bmax, res), b)
    inact = expand(out["inactive"], res, b)
    out.update(dense=dense, uc=uc, field=np.where(inact, expand(uc, res, b), dense), inactive_points=inact)
    return out
