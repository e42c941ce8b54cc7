"""The mesh rasteriser (include/oi_raster.h): an IntrinsicMesh or a TexturedMesh under the generator's
camera, as the G-buffer the traced surface's shade kernels read.  render_mesh launches no MLP entry and needs no latent: the
three raster stages, then oi_surface_shade / oi_surface_shade_local per view, unchanged."""
import numpy as np
import torch

from . import lib as _l
from . import ops
from .mesh import IntrinsicMesh, TexturedMesh

SMALL_MAX = 16                   # pixel centres in a triangle's box up to which one thread walks it
MAX_BYTES = 1 << 30              # working memory of one launch of E views: larger sets of views go in chunks
SOURCES = ("vertex", "texture")


def _check_mesh(mesh, source, what):
    """-> (the IntrinsicMesh, source, the attribute arrays of ops.raster_resolve as a dict)."""
    if isinstance(mesh, TexturedMesh):
        base, source = mesh.mesh, "texture" if source is None else source
    elif isinstance(mesh, IntrinsicMesh):
        base, source = mesh, "vertex" if source is None else source
    else:
        raise TypeError(f"{what}: mesh must be an oi_amd.mesh.IntrinsicMesh or TexturedMesh, not {type(mesh).__name__}")
    if source not in SOURCES:
        raise ValueError(f"{what}: source={source!r} (one of {SOURCES})")
    if source == "texture" and not isinstance(mesh, TexturedMesh):
        raise ValueError(f"{what}: source='texture' needs a TexturedMesh (an IntrinsicMesh carries no atlas)")
    if base.triangles is None:
        raise ValueError(f"{what}: the mesh has no triangles (vertex_attributes alone gives none: extract_intrinsic_mesh sets them)")
    tris, pos = base.triangles, base.positions
    if tris.dtype != torch.int32 or tris.dim() != 2 or tris.shape[1] != 3 or pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"{what}: triangles {tuple(tris.shape)} {tris.dtype}, positions {tuple(pos.shape)}, expected (F, 3) int32 "
                         "and (V, 3)")
    if not (pos.is_cuda and tris.is_cuda):
        raise _l.OiHipError(f"{what}: the mesh must be on the GPU (there is no CPU path)")
    F, V = tris.shape[0], pos.shape[0]
    if F >= 1 << 31 or V >= 1 << 31:
        raise ValueError(f"{what}: F={F} triangles, V={V} vertices (each below 2^31)")
    if source == "vertex":
        if base.normals is None or base.albedo is None:
            raise ValueError(f"{what}: source='vertex' needs per-vertex normals and albedo (a mesh read by load_obj carries no "
                             "vertex colours: source='texture')")
        attr = {"vertex": (base.normals.float().contiguous(), base.albedo.float().contiguous())}
    else:
        attr = {"texture": (mesh.uv.float().contiguous(), mesh.albedo_map.contiguous(), mesh.normal_map.contiguous())}
    if F:   # one pass over the indices on the device, one read-back
        lo, hi = (int(v) for v in torch.stack([tris.min(), tris.max()]).tolist())
        if lo < 0 or hi >= V:
            raise ValueError(f"{what}: triangle indices {lo} .. {hi} outside the mesh's {V} vertices")
    return base, source, attr


def _check_views(gen, b2ws, resolution, near, what):
    b2w = torch.as_tensor(b2ws).detach()
    if b2w.dim() == 2:
        b2w = b2w[None]
    if b2w.dim() != 3 or tuple(b2w.shape[1:]) != (4, 4) or not 1 <= b2w.shape[0]:
        raise ValueError(f"{what}: b2ws {tuple(b2w.shape)}, expected one (4, 4) pose or (E, 4, 4)")
    if not bool(torch.isfinite(b2w.float().cpu()).all()):
        raise ValueError(f"{what}: the poses are not finite")
    R = gen.resolution if resolution is None else resolution
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= int(R) <= _l.RASTER_MAX_RESOLUTION:
        raise ValueError(f"{what}: resolution={resolution!r} (an integer, 1 <= resolution <= {_l.RASTER_MAX_RESOLUTION})")
    R = int(R)
    if b2w.shape[0] * R * R >= 1 << 31:
        raise ValueError(f"{what}: {b2w.shape[0]} views of {R} x {R} pixels (E * R * R < 2^31)")
    if isinstance(near, bool) or not isinstance(near, (int, float, np.integer, np.floating)) or not (0 < float(near) < float("inf")):
        raise ValueError(f"{what}: near={near!r} (positive and finite)")
    return b2w, R, float(near)


def _cameras(gen, b2w, R):
    """The cameras of the poses b2w (E, 4, 4), exactly as render_surface's rays have them: -> c2b, b2c (E, 4, 4), kinv, K
    (3, 3), offs (E, 2), w2b (E, 4, 4), float32 on the device.  A resolution other than the generator's keeps the frustum:
    the pixel pitch, and with it K, kinv and the crop offsets, scale by R / gen.resolution."""
    dev = gen.it.device
    prior = gen.sample_prior(b2w.shape[0], {"b2w": b2w.to(dev, torch.float32)})
    c2b = prior["c2b"].float().contiguous()
    offs = gen.crop_offsets(prior["b2w"]).float()
    kinv = gen._kinv(dev).float()
    K = gen.camera.intrinsics[:3, :3].to(dev).float()
    if R != gen.resolution:
        s = R / gen.resolution
        scale = torch.tensor([s, s, 1.0], device=dev)
        K, kinv, offs = scale[:, None] * K, kinv / scale[None, :], offs * s
    b2c = torch.linalg.inv(c2b.double().cpu()).float().to(dev)
    return c2b, b2c.contiguous(), kinv.contiguous(), K.contiguous(), offs.contiguous(), prior["w2b"].float().contiguous()


def _views_per_launch(E, F, N):
    """Views of one launch: the setup's and the fill's working memory and the resolve's arrays, within MAX_BYTES."""
    per_view = F * (24 + 16 + 1 + 8) + N * (8 + 4 * 26 + 1) + 8
    return max(1, min(E, _l.RASTER_MAX_VIEWS, MAX_BYTES // max(per_view, 1)))


def rasterise(gen, mesh, b2ws, source=None, resolution=None, near=1e-3, small_max=SMALL_MAX, what="rasterise"):
    """The raster stages alone: the arguments are checked here, the stages run as the chunks are asked for.  -> (an iterator
    of chunks (first view, w2b of the chunk's views, setup dict, zbuf, resolve dict), the checked mesh, R).  A chunk's working
    memory (setup, zbuf) lives only as long as the caller holds it: render_mesh shades a chunk and lets it go before the next
    one is made, so the peak is one chunk within MAX_BYTES and the results."""
    b2w, R, near = _check_views(gen, b2ws, resolution, near, what)
    base, source, attr = _check_mesh(mesh, source, what)
    c2b, b2c, kinv, K, offs, w2b = _cameras(gen, b2w, R)
    E, F, pos = b2w.shape[0], base.triangles.shape[0], base.positions.float().contiguous()
    step = _views_per_launch(E, F, R * R)

    def chunks():
        for a in range(0, E, step):
            b = min(E, a + step)
            setup = ops.raster_setup(b2c[a:b], K, offs[a:b], R, pos, base.triangles, near, small_max)
            zbuf = ops.raster_fill(c2b[a:b], kinv, offs[a:b], R, pos, base.triangles, setup)
            g = ops.raster_resolve(c2b[a:b], kinv, offs[a:b], R, pos, base.triangles, zbuf, **attr)
            yield a, w2b[a:b], setup, zbuf, g
            del setup, zbuf, g   # (before the next chunk is allocated)
    return chunks(), base, R


def _stats(setup, g, F):
    """The class counts and the covered pixels of every view of a chunk: one read-back."""
    E = g["triangle"].shape[0]
    cls = torch.stack([(setup["cls"] == k).sum(1) for k in range(4)], 1) if F else torch.zeros(E, 4, dtype=torch.long, device=g["triangle"].device)
    rows = torch.cat([cls, (g["triangle"] >= 0).sum(1, keepdim=True)], 1).tolist()
    return [{"triangles": F, "dropped": r[_l.RASTER_DROPPED], "empty": r[_l.RASTER_EMPTY], "small": r[_l.RASTER_SMALL],
             "large": r[_l.RASTER_LARGE], "covered": r[4]} for r in rows]


@torch.no_grad()
def render_mesh(gen, mesh, b2ws, lights=None, bg=None, source=None, resolution=None, near=1e-3):
    """A mesh under the generator's camera (include/oi_raster.h).  mesh: an oi_amd.mesh.IntrinsicMesh
    with triangles (source "vertex": its per-vertex normals and albedo, interpolated) or a TexturedMesh (default source
    "texture": a bilinear lookup of its byte atlases through its uv; "vertex" reads the mesh it was built on).  b2ws: one
    (4, 4) pose or (E, 4, 4), any number of views, rasterised E <= 1024 per launch and in chunks within raster.MAX_BYTES;
    the camera is the generator's, exactly as render_surface's rays have it (resolution: another image side R for the
    same frustum).  lights: oi_amd.relight.Light or LocalLight objects (default the generator's trained light), shaded by
    oi_surface_shade / oi_surface_shade_local as the traced surface is, WITHOUT shadows or occlusion.  near: the camera
    depth a vertex must exceed; a triangle with a vertex nearer is dropped whole (no clipping).
    -> per view a dict with render_surface's keys depth (1, 1, H, W) (the ray parameter, NaN off the mesh), position,
    normal_map (world frame), normal_object, albedo (1, 3, H, W), mask (1, 1, H, W), image (L, 3, H, W), and triangle
    (1, 1, H, W) int32 (-1 off the mesh), barycentric (1, 3, H, W), stats (triangles, dropped, empty, small, large, covered);
    a list of E such dicts when b2ws is (E, 4, 4).  No MLP entry is launched and no latent is needed.
    Refused by name: a mesh without triangles, source="texture" on an IntrinsicMesh, indices outside the vertices (one
    check on the device, one read-back), F >= 2^31, E * R * R >= 2^31, more than 256 lights, poses that are not finite."""
    from .trace import _MAP_NAMES, _bg, _is_local, _maps, _stack_lights
    what = "render_mesh"
    gen.eval()
    dev = gen.it.device
    lt = _stack_lights(gen, lights, dev, what)
    single = torch.as_tensor(b2ws).dim() == 2
    chunks, base, R = rasterise(gen, mesh, b2ws, source, resolution, near, what=what)
    F, N, bgv, out = base.triangles.shape[0], R * R, _bg(bg, dev), []
    shade = ops.surface_shade_local if _is_local(lt) else ops.surface_shade
    for chunk in chunks:
        _, w2b, setup, _, g = chunk
        stats = _stats(setup, g, F)
        del chunk, setup, _
        for e in range(w2b.shape[0]):
            maps = shade(g["rays_o"][e], g["rays_d"][e], g["t"][e], g["status"][e], g["hit_slot"][e], g["hit_points"][e],
                         g["grad"][e], g["rgb"][e], N, w2b[e], lt, bgv, None)
            res = {_MAP_NAMES[k]: v for k, v in _maps({k: v for k, v in maps.items() if k != "image"}, R, R).items()}
            res["image"] = maps["image"].view(-1, 3, R, R)
            res["triangle"] = g["triangle"][e].view(1, 1, R, R)
            res["barycentric"] = g["barycentric"][e].view(1, R, R, 3).permute(0, 3, 1, 2)
            res["stats"] = stats[e]
            out.append(res)
    return out[0] if single else out
