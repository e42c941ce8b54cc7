"""NeuS renderer -- drop-in for src.third_party.neus.models.renderer.NeuSRenderer
(renderer.py:77-96 ctor, 351-473 render) with the same constructor kwargs and the same keys /
shapes in the dict `render()` returns.  Every stage is a HIP kernel:

    coarse z + points          oi_coarse_samples     (renderer.py:359-373, 391)
    coarse SDF                 oi_sdf_mlp_fwd        (renderer.py:396; sdf-only variant)
    K x importance resampling  oi_upsample [+ oi_sdf_mlp_fwd + oi_merge_sorted]  (:400-413)
    mid-points                 oi_midpoints          (:219-235)
    SDF + d sdf/dx + albedo    oi_sdf_mlp_fwd        (:241-261; ONE pass instead of the reference's three)
    compositing (+ Phong maps) oi_composite_fwd      (:266-311, 338; generator.py:80-174)
"""
import numpy as np
import torch

from . import ops
from .autograd import sdf_mlp
from .fields import FieldPack


class NeuSRenderer:
    def __init__(self, nerf, sdf_network, deviation_network, color_network, n_samples, n_importance, n_outside,
                 up_sample_steps, perturb, precision="f16x3", fast_trig=None):
        if n_outside != 0:
            raise NotImplementedError("n_outside > 0 (NeRF++ background) is dead on the path (train.yaml:73)")
        self.nerf = nerf
        self.sdf_network = sdf_network
        self.deviation_network = deviation_network
        self.color_network = color_network
        self.n_samples = n_samples
        self.n_importance = n_importance
        self.n_outside = n_outside
        self.up_sample_steps = up_sample_steps
        self.perturb = perturb
        self.pack = FieldPack(sdf_network, color_network, precision, fast_trig)

    # -- stages -----------------------------------------------------------------------------
    def sample_z(self, rays_o, rays_d, near, far, gamma, beta, B, perturb, with_mid=False, coarse=None):
        """Hierarchical sampling (no grad, as in the reference: renderer.py:390, 180).  -> z (N, S+I) [, (dists, mid_z, pts):
        the section mid-points, which the last up-sampling launch produces as well (None when there is no such launch)]."""
        S, I, K = self.n_samples, self.n_importance, self.up_sample_steps
        N = rays_o.shape[0]
        mid = None
        with torch.no_grad():
            if coarse is not None:   # (z, pts) of the coarse samples from the caller's fused launch (jitter already drawn)
                z, pts = coarse
            else:
                jitter = torch.rand([N, 1], device=rays_o.device) if perturb > 0 else None  # renderer.py:372
                z, pts = ops.coarse_samples(rays_o, rays_d, near, far, S, jitter)
            if I > 0:
                sdf = sdf_mlp(self.pack, pts.view(-1, 3), gamma, beta, B, False, False, False)[0].view(N, S)
                for i in range(K):
                    last = i + 1 == K
                    if last and with_mid:
                        _, _, z, mid = ops.upsample(rays_o, rays_d, z, sdf, I // K, 64.0 * 2 ** i, mid_last_dist=2.0 / S)
                        break
                    z_new, pts_new, z_merged = ops.upsample(rays_o, rays_d, z, sdf, I // K, 64.0 * 2 ** i, merge=last)
                    if last:
                        z = z_merged
                    else:
                        sdf_new = sdf_mlp(self.pack, pts_new.view(-1, 3), gamma, beta, B, False, False, False)[0]
                        z, sdf = ops.merge_sorted(z, sdf, z_new, sdf_new.view(N, -1))
        return (z, mid) if with_mid else z

    def render_full(self, rays_o, rays_d, near, far, perturb_overwrite=-1, cos_anneal_ratio=0.0, z=None, w=None,
                    light=None, light_dir=None, bg=None, outputs=None, film=None, image_planar=False, coarse=None,
                    f3_scratch=None):
        """Shared implementation: returns (per-sample/per-ray dict, composite dict).  f3_scratch: the fine pass's working memory
        with the f16x3 kernel's per-element blobs already in it (ops.f3_scratch_for; written by the caller's prep launch)."""
        from .autograd import composite
        rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
        N = rays_o.shape[0]
        if N == 0:
            raise ValueError("NeuSRenderer.render: empty ray batch (the reference reshapes rays to (B, N/B, 3), fields.py:55)")
        # `film` = (w, gamma, beta) precomputed by the caller (one launch per forward instead of one per chunk + style)
        w_, gamma, beta = film if film is not None else self.pack.film(z=z if w is None else None, w=w)
        B = w_.shape[0]
        if N % B != 0:
            raise ValueError(f"NeuSRenderer.render: {N} rays cannot be split over {B} latent codes (rows of one batch "
                             "element are contiguous, fields.py:55)")
        perturb = self.perturb if perturb_overwrite < 0 else perturb_overwrite
        zv, mid = self.sample_z(rays_o, rays_d, near, far, gamma.detach(), beta.detach(), B, perturb, with_mid=True,
                                 coarse=coarse)
        T = zv.shape[1]
        if mid is not None:
            dists, mid_z, pts = mid
        else:  # no importance samples: the coarse list itself
            with torch.no_grad():
                dists, mid_z, pts = ops.midpoints(rays_o, rays_d, zv, 2.0 / self.n_samples)
        sdf, grad, rgb, _ = sdf_mlp(self.pack, pts.view(-1, 3), gamma, beta, B, True, True, False, scratch=f3_scratch,
                                    blob_ready=f3_scratch is not None)
        dev = rays_o.device
        if light is None:
            light = torch.tensor([0.0, 0.0, 1.0], device=dev)
            light_dir = torch.tensor([[0.0, 0.0, -1.0]], device=dev).expand(B, 3)
        comp = composite(sdf.view(N, T), grad.view(N, T, 3), rgb.view(N, T, 3), dists, mid_z, rays_o, rays_d,
                         light_dir, bg, self.deviation_network.variance, light, cos_anneal_ratio, B, outputs,
                         image_planar=image_planar)
        samples = {"sdf": sdf.view(N, T), "gradients": grad.view(N, T, 3), "raw_color": rgb.view(N, T, 3),
                   "mid_z_vals": mid_z, "pts": pts, "dists": dists, "z_vals": zv}
        return samples, comp

    # -- reference API ----------------------------------------------------------------------
    def render(self, rays_o, rays_d, near, far, perturb_overwrite=-1, background_rgb=None, cos_anneal_ratio=0.0,
               siren_network=None, z=None, w=None, second_order=None, compute_color=True, compute_sample_dist=False,
               blend_background=False):
        if siren_network is not None or second_order or compute_sample_dist or blend_background:
            raise NotImplementedError("only the code path exercised by generator.py:245-252 is implemented")
        s, c = self.render_full(rays_o, rays_d, near, far, perturb_overwrite, cos_anneal_ratio, z, w,
                                outputs=("weights", "cdf", "inside_sphere", "pts_norm", "weight_sum", "weight_max",
                                         "color_fine", "reduce4"))
        return assemble_render_dict(s, c, self.deviation_network.variance, background_rgb)

    def extract_geometry(self, bound_min, bound_max, resolution, threshold=0.0, siren_network=None, z=None, w=None, band=False,
                         lipschitz=None, block=None):
        """renderer.py:475-492: the mesh of u = -sdf at `threshold` -> numpy (V, 3) float64 world-space vertices, (F, 3) int64
        triangles.  The field comes from one lattice launch (oi_sdf_lattice: no points materialised, no query_func) and the
        marching cubes run on the GPU (oi_mc_count / oi_mc_emit).  band=True: the field comes from mesh.sdf_lattice_band at
        `threshold` (lipschitz, block: its arguments): the network runs only near the surface, the mesh is the same."""
        from . import mesh
        if siren_network is not None:
            raise NotImplementedError("siren_network is not on the path (as in render())")
        if z is None and w is None:
            raise ValueError("extract_geometry: ShapeNetwork.sdf needs a latent -- pass z or w")
        B = (w if w is not None else z).shape[0]
        if B != 1:
            raise ValueError(f"extract_geometry: one latent expected, got a batch of {B} (the reference's sdf(pts, z) would "
                             "split the lattice across them)")
        u, _ = mesh._level_field(self.pack, bound_min, bound_max, resolution, threshold, z, w, band, lipschitz, block,
                                 "extract_geometry")
        vertices, triangles = mesh.marching_cubes(u, threshold)
        vertices = vertices.cpu().numpy().astype(np.float64)
        return mesh.to_world(vertices, bound_min, bound_max, resolution), triangles.cpu().numpy().astype(np.int64)

    def extract_intrinsic_geometry(self, bound_min, bound_max, resolution, threshold=0.0, siren_network=None, z=None, w=None,
                                   refine=2, band=False, lipschitz=None, block=None):
        """extract_geometry's arguments (plus `refine`; band, lipschitz, block as there), the intrinsic mesh out: numpy (V, 3) float64 world-space vertices moved
        onto the level set sdf = -threshold by `refine` Newton steps, (F, 3) int64 triangles (those of extract_geometry),
        (V, 3) float32 unit normals d sdf/dx / |d sdf/dx| and (V, 3) float32 albedo.  oi_amd.mesh.extract_intrinsic_mesh has
        the device tensors, the residuals and the per-vertex flags."""
        from . import mesh
        if siren_network is not None:
            raise NotImplementedError("siren_network is not on the path (as in render())")
        m = mesh.extract_intrinsic_mesh(self, z=z, w=w, resolution=resolution, threshold=threshold, bound_min=bound_min,
                                        bound_max=bound_max, refine=refine, band=band, lipschitz=lipschitz, block=block)
        return (m.positions.cpu().numpy().astype(np.float64), m.triangles.cpu().numpy().astype(np.int64),
                m.normals.cpu().numpy(), m.albedo.cpu().numpy())

    def extract_textured_geometry(self, z=None, w=None, resolution=64, texel=8, **kw):
        """oi_amd.mesh.extract_textured_mesh on this renderer: a coarse intrinsic mesh with a per-triangle UV atlas and baked
        albedo and normal maps -> oi_amd.mesh.TexturedMesh (mesh.save_obj writes it)."""
        from . import mesh
        return mesh.extract_textured_mesh(self, z=z, w=w, resolution=resolution, texel=texel, **kw)


class _RenderScalars(torch.autograd.Function):
    """(gradient_error, surface_loss) from the compositing reductions in one launch each way (oi_render_scalars_fwd / _bwd);
    as tensor ops: add, div, div forward and six launches backward per training render."""

    @staticmethod
    def forward(ctx, r4, inv_nt):
        r4 = r4.detach().contiguous()
        out = ops.render_scalars_fwd(r4, inv_nt)
        ctx.r4, ctx.inv_nt = r4, inv_nt
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_err, g_surf):
        if g_err is None and g_surf is None:
            return None, None
        c = lambda g: None if g is None else g.contiguous()
        return ops.render_scalars_bwd(ctx.r4, c(g_err), c(g_surf), ctx.inv_nt), None


def render_scalars(r4, n_samples_total):
    """-> (gradient_error, surface_loss) (renderer.py:430-446)."""
    return _RenderScalars.apply(r4, 1.0 / float(n_samples_total))


_INV_S_CACHE = {}


def _inv_s(variance):
    """-> (inv_s, 1 / inv_s), inv_s = exp(10 variance).clamp(1e-6, 1e6) (renderer.py:404): four launches, cached per parameter
    version.  Reported values only: the compositing kernel computes its own copy from `variance` and owns the gradient (the
    reference's `s_val` entry carries a graph that no loss of the path uses; ours does not -- four launches forward and four
    backward per training render otherwise)."""
    key = (variance.data_ptr(), variance._version)
    hit = _INV_S_CACHE.get(variance.device)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            inv = torch.exp(variance * 10.0).clamp(1e-6, 1e6)
            hit = _INV_S_CACHE[variance.device] = (key, inv, 1.0 / inv)
    return hit[1], hit[2]


def assemble_render_dict(s, c, variance, background_rgb=None, finals=None, s_val=None):
    """Same keys/shapes as NeuSRenderer.render's return value (renderer.py:448-473).  `finals`: the derived scalars
    of ops.composite_fwd (gradient_error and surface_loss already divided, no extra launches; no-grad callers only).
    `s_val`: 1 / inv_s when the caller already has it (Generator._glue: one launch per parameter version for all scalar glue)."""
    N, T = s["sdf"].shape
    r4 = c["reduce4"]
    if s_val is None:
        _, s_val = _inv_s(variance)
    color = c["color_fine"]
    if background_rgb is not None:
        color = color + background_rgb * (1.0 - c["weight_sum"])
    gradient_error, surface_loss = (finals[0], finals[1]) if finals is not None else render_scalars(r4, N * T)
    # (entries the caller did not ask the compositing launch for -- Generator.forward without return_raw, which hands this dict
    # to nobody -- are None)
    return {
        "s_val": s_val.detach().reshape(1, 1).expand(N, 1),   # a report without a graph (stated deviation: see _inv_s)
        "cdf_fine": c.get("cdf"),
        "weight_sum": c["weight_sum"],
        "weight_max": c.get("weight_max"),
        "gradients": s["gradients"],
        "weights": c.get("weights"),
        "gradient_error": gradient_error,
        "inside_sphere": c.get("inside_sphere"),
        "mid_z_vals": s["mid_z_vals"],
        "surface_loss": surface_loss,
        "sdf": s["sdf"],
        "pts_norm": c.get("pts_norm"),
        "pts": s["pts"],
        "color_fine": color,
        "raw_color": s["raw_color"],
    }
