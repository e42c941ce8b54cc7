"""A scene of many instances: K latents at K rigid poses in ONE scene image of the generator's own camera -- the picture
the model was trained from -- with occlusion between the instances and the shadows they cast on each other
(include/oi_scene.h), and with sampled secondary rays between them: soft shadows, ambient occlusion
and environment lighting (include/oi_scene_light.h).

    sample_scene   K latents and K poses from the generator's latent distribution and pose prior
    trace_scene    the light-independent half: windowed scene rays with a bounding-sphere cull, ONE batched march for all
                   instances (oi_amd.trace's, unchanged), the depth resolve across instances, the full MLP pass at the
                   VISIBLE hits only -> SceneSurface
    SceneSurface.shade  the scene under L lights, optionally with one shadow ray per light and visible point tested against
                   EVERY instance -- or `shadow_samples` rays towards a light of angular radius `light_radius` (penumbrae) --
                   and ambient occlusion (`ao_samples` rays over the hemisphere of each visible point), all of them tested
                   against every instance: contact shadows between objects
    render_scene   both
                   aa_samples > 1 (trace_scene, render_scene): adaptive anti-aliasing -- the scene pixels at an outline, at a
                   contour between two instances or at a geometric edge get sub-pixel rays in every instance, which pass the
                   same march, resolve and shade, and the image is the mean of a pixel's samples (include/oi_scene_aa.h;
                   DESIGN section 4.30)
    SceneSurface.capture_transfer  the secondary rays traced ONCE into a per-pixel SH transfer map of the whole scene ->
                   SceneTransfer, shaded under any number of environment lights (oi_amd.envlight.EnvLight); with bounces=1 the
                   rays that end on ANY instance carry one diffuse interreflection bounce (include/oi_scene_bounce.h; DESIGN
                   section 4.26): the instances colour each other
    render_scene_env  trace_scene + capture_transfer + shade
    Ground         a plane in the scene's world frame that catches the instances' shadows and contact darkening and blocks their
                   own ambient and directional rays (include/oi_ground.h): ground= on SceneSurface.shade,
                   render_scene and the light walks; SceneSurface.ground -> GroundSurface, the plane's pixels and their
                   secondary rays; composite_over puts the result over a photograph by its shadow matte

The union of K surfaces is traced exactly by tracing each instance in its own box frame and keeping the nearest hit per
pixel: the camera is shared and the poses are rigid, so the ray parameter of one scene pixel is comparable between
instances.  Per ray the trace is oi_amd.trace.sphere_trace's on that instance alone, bit for bit."""
import math

import numpy as np
import torch

from . import lib as _l
from . import ops
from . import trace as _t
from .fields import LatentField
from .relight import local_lights_given

DEFAULT_BIAS = _t.DEFAULT_BIAS
MAX_SHADOW_RAYS = 1 << 24     # rays of one shadow batch, counted as E * L * n_vis (about 80 bytes of state each)


def sample_scene(gen, K, seed):
    """K instances for one scene: latents zs (K, z_dim) from the generator's latent distribution (standard normal) and poses
    b2ws (K, 4, 4) from gen.pose_prior, both a function of `seed` alone.  The pose prior draws from numpy's global generator;
    its state is put back."""
    if not _t._is_count(K, 1, _l.TRACE_BATCH_MAX_ELEMS):
        raise ValueError(f"sample_scene: K={K!r} instances (an integer, 1 .. {_l.TRACE_BATCH_MAX_ELEMS})")
    _t._check_seed(seed, "sample_scene")
    zs = torch.randn(int(K), gen.z_dim, generator=torch.Generator().manual_seed(int(seed)))
    state = np.random.get_state()
    try:
        np.random.seed(int(seed))
        b2ws = np.asarray(gen.pose_prior(int(K)), dtype=np.float32)
    finally:
        np.random.set_state(state)
    return zs, torch.from_numpy(b2ws)


def scene_windows(gen, b2ws, window=None, what="trace_scene"):
    """The windows of the instances in the scene image, on the host in float64.  b2ws (K, 4, 4).  -> (W, origins (K, 2)
    int64): instance e covers scene pixels (x0 + i, y0 + j), 0 <= i, j < W.  W: `window`, or the smallest value for which
    every instance's unit sphere projects inside its window: seen from the camera the sphere's extent along x is the pair of
    tangents tan(atan2(c_x, c_z) -+ asin(1 / hypot(c_x, c_z))) at the centre c, likewise along y; pixel X looks along
    (X S / (S - 1) - K_02) / K_00.  The origins centre the projection in the window.
    Refused, naming the instance: a camera inside or within 1 of an instance's unit sphere, an instance behind the camera."""
    b2w = np.asarray(b2ws.detach().cpu() if torch.is_tensor(b2ws) else b2ws, dtype=np.float64).reshape(-1, 4, 4)
    S = int(gen.scene_resolution)
    Kc = gen.camera.intrinsics.detach().cpu().double().numpy()
    w2c = gen.camera.w2c.detach().cpu().double().numpy()
    lo, hi = np.zeros((len(b2w), 2), dtype=np.int64), np.zeros((len(b2w), 2), dtype=np.int64)
    for e, m in enumerate(b2w):
        c = (w2c @ m)[:3, 3]
        if not np.isfinite(c).all():
            raise ValueError(f"{what}: instance {e}: the pose is not finite")
        if c[2] <= 0:
            raise ValueError(f"{what}: instance {e} is behind the camera (depth {c[2]:.4g})")
        if np.linalg.norm(c) < 2.0:
            raise ValueError(f"{what}: instance {e}: the camera is inside or within 1 of its unit sphere (distance "
                             f"{np.linalg.norm(c):.4g} from its centre, at least 2 needed)")
        if c[2] <= 1.0:
            raise ValueError(f"{what}: instance {e} is behind the camera (its unit sphere reaches the camera plane: depth {c[2]:.4g})")
        for a in range(2):
            mid, half = math.atan2(c[a], c[2]), math.asin(1.0 / math.hypot(c[a], c[2]))
            px = [Kc[a, a] * math.tan(mid + s * half) + Kc[a, 2] for s in (-1, 1)]
            scale = (S - 1) / S if S > 1 else 1.0
            lo[e, a], hi[e, a] = math.floor(px[0] * scale), math.ceil(px[1] * scale)
    if window is None:
        W = int((hi - lo).max()) + 1
    else:
        if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or int(window) < 1:
            raise ValueError(f"{what}: window={window!r} (a positive number of scene pixels)")
        W = int(window)
    origin = lo - (W - (hi - lo + 1)) // 2
    return W, origin


def virtual_image_size(n_sub, E, what="trace_scene"):
    """The side Q of the virtual scene image that holds n_sub sub-sample rays per instance (include/oi_scene_aa.h): the
    smallest Q with Q * Q >= n_sub, so fewer than 2 Q + 1 of its pixels are padding.  Refused: E * Q * Q >= 2^31, or Q above the
    scene entries' largest resolution."""
    Q = math.isqrt(int(n_sub) - 1) + 1 if n_sub > 0 else 0
    if E * Q * Q >= 1 << 31 or Q > _l.SCENE_MAX_RESOLUTION:
        raise ValueError(f"{what}: {n_sub} sub-sample rays per instance need a virtual image of {Q} x {Q} pixels, {E} instances x "
                         f"{Q} x {Q} = {E * Q * Q} rays (E * Q^2 < 2^31, Q <= {_l.SCENE_MAX_RESOLUTION}): fewer aa_samples, or "
                         "aa_adaptive=True")
    return Q


class Ground:
    """A ground plane in the world frame of a scene (include/oi_ground.h): the points x with normal . x =
    offset within `extent` of `centre`, a Lambertian surface of colour `albedo` seen from the side the normal points to.
    Refused with ValueError: a normal that is not unit to 1e-4, a non-finite offset or centre, an albedo outside [0, 1], an
    extent that is not positive (inf is allowed)."""

    def __init__(self, normal, offset, albedo=(0.8, 0.8, 0.8), extent=math.inf, centre=(0.0, 0.0, 0.0)):
        as3 = lambda v, name: np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)
        n, a, c = as3(normal, "normal"), np.broadcast_to(as3(albedo, "albedo"), (3,)).copy(), as3(centre, "centre")
        if n.shape != (3,) or not np.isfinite(n).all() or abs(np.linalg.norm(n) - 1.0) > 1e-4:
            raise ValueError(f"Ground: normal={normal!r} (three finite numbers of unit length, to 1e-4)")
        if c.shape != (3,) or not np.isfinite(c).all():
            raise ValueError(f"Ground: centre={centre!r} (three finite numbers)")
        if not math.isfinite(float(offset)):
            raise ValueError(f"Ground: offset={offset!r} (a finite number)")
        if not ((a >= 0).all() and (a <= 1).all()):
            raise ValueError(f"Ground: albedo={albedo!r} (within [0, 1])")
        if not float(extent) > 0:
            raise ValueError(f"Ground: extent={extent!r} (> 0; inf is allowed)")
        self.normal, self.offset, self.albedo = tuple(n.tolist()), float(offset), tuple(a.tolist())
        self.extent, self.centre = float(extent), tuple(c.tolist())

    @classmethod
    def through(cls, point, normal, **kw):
        """The plane through the world point `point`."""
        p = np.asarray(point.detach().cpu() if torch.is_tensor(point) else point, dtype=np.float64).reshape(3)
        n = np.asarray(normal.detach().cpu() if torch.is_tensor(normal) else normal, dtype=np.float64).reshape(3)
        return cls(normal, float(n @ p), **kw)

    @classmethod
    def below(cls, points, normal, gap=0.0, **kw):
        """The plane at min(normal . p) - gap over the world points `points` (n, 3), for example
        SceneSurface.world_points()[0]: what the instances stand on."""
        p = np.asarray(points.detach().cpu() if torch.is_tensor(points) else points, dtype=np.float64).reshape(-1, 3)
        n = np.asarray(normal.detach().cpu() if torch.is_tensor(normal) else normal, dtype=np.float64).reshape(3)
        if len(p) == 0 or not np.isfinite(p).all():
            raise ValueError("Ground.below: points must be a non-empty (n, 3) array of finite numbers")
        return cls(normal, float((p @ n).min()) - float(gap), **kw)

    def packed(self):
        """The record [OI_GROUND_FLOATS] as float32 numpy."""
        return np.array([*self.normal, self.offset, *self.albedo, self.extent, *self.centre, 0.0], dtype=np.float32)


def check_ground_keyword(ground, aa, what):
    """The `ground` keyword of `what` before anything is traced: a Ground or None, and not together with anti-aliasing."""
    if ground is None:
        return
    if not isinstance(ground, Ground):
        raise ValueError(f"{what}: ground={ground!r} (an oi_amd.scene.Ground)")
    if aa is not None:
        raise ValueError(f"{what}: ground with aa_samples={aa.S}; the ground plane has no anti-aliasing stage yet (aa_samples=1)")


def refuse_env_ground(ground, what):
    """The `ground` keyword of an environment path: refused unless None (capture_transfer's maps know no ground plane yet)."""
    if ground is not None:
        raise ValueError(f"{what}: ground= is not supported by capture_transfer and the environment paths (the ground plane is "
                         "shaded by SceneSurface.shade under directional and local lights)")


class GroundSurface(_t._Stages):
    """A Ground in one traced scene (SceneSurface.ground): record (12,) on the device; t (S * S,), the ground's ray parameter
    per scene pixel, NaN off the ground; n_g ground pixels, index (n_g,) int32 ascending, slot (S * S,) int32 (a pixel's
    position in index, -1 off the ground); evals: the sdf evaluations of its secondary rays so far."""

    def __init__(self, scene, ground):
        s, dev = scene, scene.b2w.device
        c2w = s.c2w.detach().cpu().double().numpy()
        rec = ground.packed()
        height = float(np.asarray(ground.normal) @ c2w[:3, 3]) - ground.offset
        if not height > 0:
            raise ValueError(f"SceneSurface.ground: the camera is on or below the plane (normal . eye - offset = {height:.4g}, > 0 "
                             "needed)")
        self.scene, self.ground, self.evals = s, ground, 0
        self.record = torch.from_numpy(rec).to(dev)
        M = s.S * s.S
        owned = s.owner is not None
        self.t, index, count = ops.ground_begin(s.c2w, s.kinv, s.S, self.record, s.owner, s.owner_ray if owned else None,
                                                s.state.t if owned else None, s.window if owned else None, s.W, s.E)
        self.n_g = int(count.item())
        self.slot = torch.full((M,), -1, dtype=torch.int32, device=dev)
        self.index = _t._ascending(index, self.n_g, self.slot).contiguous()

    def _args(self):
        s = self.scene
        return s.c2w, s.kinv, s.S, self.record, self.t, self.index, self.n_g

    def _sampled(self, what, samples, seed, max_shadow_rays, lights=None, radius=None, distance=None):
        """The sampled any-hit trace of the ground points against every instance, in chunks of the samples under
        max_shadow_rays as SceneSurface._sampled's: a chunk holds E * L * Sc * n_g rays.  -> out (L, n_g)."""
        s = self.scene
        L = 1 if lights is None else lights.shape[0]
        per = s.E * L * self.n_g
        chunks = _t.sample_chunks(samples, per, max_shadow_rays, what,
                                  f"{s.E} instances x {L} lights x {self.n_g} ground points = E * L * n_g = {per} rays per sample")
        count, out = ops._new(self.record, L, self.n_g).view(torch.int32), ops._new(self.record, L, self.n_g)
        evals, self.last = _t.sampled_trace(
            s.field, s.kw, self.record, s.E, L * self.n_g, samples, chunks,
            lambda sb, j0, c: ops.ground_rays_begin(sb, *self._args(), s.w2b, s.bias, samples, j0, c, seed, lights, radius, distance),
            lambda sb, j0, c, last: ops.ground_resolve(sb.status, s.E, self.n_g, L, samples, j0, c, count, out, last))
        self.evals += evals
        return out

    def visibility(self, lights, radius=None, samples=1, seed=0, max_shadow_rays=MAX_SHADOW_RAYS):
        """(L, n_g): the share of `samples` rays per directional light (L, 16) and ground point, over the light's cap of angular
        radius radius[l] (None: 0, the hard shadow ray), that miss EVERY instance."""
        L = lights.shape[0]
        if self.n_g == 0:
            return torch.ones(L, 0, device=lights.device)
        radius = torch.zeros(L, device=lights.device) if radius is None else \
            torch.as_tensor(radius, dtype=torch.float32).reshape(-1).to(lights.device)
        return self._sampled("GroundSurface.visibility", samples, seed, max_shadow_rays, lights, radius)

    def local_visibility(self, lights, samples=1, seed=0, max_shadow_rays=MAX_SHADOW_RAYS):
        """(L, n_g): the share of `samples` rays per local light (L, 20) and ground point, aimed at the light's sphere and ending
        there, that miss every instance.  An instance beyond the light throws no shadow on the ground."""
        if self.n_g == 0:
            return torch.ones(lights.shape[0], 0, device=lights.device)
        return self._sampled("GroundSurface.local_visibility", samples, seed, max_shadow_rays, lights)

    def ambient(self, samples, distance, seed=0, max_shadow_rays=MAX_SHADOW_RAYS):
        """(n_g,): the share of `samples` cosine-weighted rays over the plane's hemisphere per ground point that meet no instance
        within `distance`: the contact shadow."""
        if self.n_g == 0:
            return torch.ones(0, device=self.record.device)
        return self._sampled("GroundSurface.ambient", samples, seed, max_shadow_rays, distance=float(distance)).view(self.n_g)

    def shade(self, maps, lt, vis=None, ao=None):
        """oi_ground_shade: the ground into `maps` (ops.GROUND_OUT's names), in place.  -> ground_mask (S * S,), shadow_matte (L,
        3, S * S)."""
        return ops.ground_shade(*self._args(), lt, {k: v for k, v in maps.items() if k in ops.GROUND_OUT}, vis, ao)


def composite_over(result, photo):
    """A rendered scene with a ground plane (SceneSurface.shade's dict with ground=) over a photograph: `image` on the
    instances' mask, photo * shadow_matte elsewhere -- the photograph darkened by the instances' shadows and contact
    occlusion where the ground catches them, untouched off the ground.  photo: (3, S, S) or (L, 3, S, S).  -> (L, 3, S, S)."""
    if "shadow_matte" not in result:
        raise ValueError("composite_over: the result has no shadow_matte (render the scene with ground=)")
    image, matte, mask = result["image"], result["shadow_matte"], result["mask"]
    photo = torch.as_tensor(photo, dtype=image.dtype).to(image.device)
    if photo.dim() == 3:
        photo = photo[None]
    if photo.shape[-3:] != image.shape[-3:] or photo.shape[0] not in (1, image.shape[0]):
        raise ValueError(f"composite_over: photo {tuple(photo.shape)} for an image {tuple(image.shape)}")
    return torch.where(mask > 0, image, photo * matte)


class SceneSurface(_t._Stages):
    """One traced scene and what the light-dependent stages reuse: the batched state (rays, t, status per instance), the
    owner map, the visible hits of every instance and the gradient and albedo there.
    E instances, window W, scene resolution S; window (E, 2) int32; n_entered / n_hit / n_vis: per instance the rays
    entered, the hits and the hits that own their pixel; n_pad = max(n_vis); state: ops.TraceBatchState."""
    OUTPUTS, AA_RESOLVE = ("depth", "position", "normal_world", "albedo", "mask", "instance", "image"), "aa_resolve_strided"
    n_pixels, side, n_points = property(lambda self: self.S * self.S), property(lambda self: self.S), property(lambda self: sum(self.n_vis))
    device = property(lambda self: self.b2w.device)

    def __init__(self, gen, zs, b2ws, window, bias, trace_kw, aa=None):
        kw, bias = _t._Surface.params(bias, trace_kw, "trace_scene")
        dev = gen.it.device
        zs = _t._latents(zs, dev)
        b2ws = (b2ws if torch.is_tensor(b2ws) else torch.stack([torch.as_tensor(b) for b in b2ws])).float().reshape(-1, 4, 4)
        E = zs.shape[0]
        if b2ws.shape[0] != E or not 1 <= E <= _l.TRACE_BATCH_MAX_ELEMS:
            raise ValueError(f"trace_scene: {E} latents and {b2ws.shape[0]} poses (one pose per latent, 1 .. "
                             f"{_l.TRACE_BATCH_MAX_ELEMS} instances)")
        W, origin = scene_windows(gen, b2ws, window)
        if E * W * W >= 1 << 31:
            raise ValueError(f"trace_scene: {E} instances x {W} x {W} window rays = {E * W * W} (E * W^2 < 2^31)")
        S = int(gen.scene_resolution)
        if not 1 <= S <= _l.SCENE_MAX_RESOLUTION:
            raise ValueError(f"trace_scene: scene_resolution={S} (1 .. {_l.SCENE_MAX_RESOLUTION})")
        field = LatentField(gen, zs, None, "trace_scene", batch_ok=True)
        gen.eval()
        field.prepare(zs, None)
        prior = gen.sample_prior(E, {"b2w": b2ws.to(dev)})
        b2w = prior["b2w"].contiguous()
        win = torch.from_numpy(origin.astype(np.int32)).to(dev)
        st = ops.trace_batch_state_empty(E, W * W, b2w)
        c2b, kinv = prior["c2b"].contiguous(), gen._kinv(dev)
        ops.scene_begin(st, c2b, kinv, win, W, S)
        self._set(gen, field, kw, bias, b2w, prior["w2b"].contiguous(), win, W, S, st)
        self.c2w, self.kinv = gen.camera.c2w.detach().to(dev).float().contiguous(), kinv   # the scene's world rays (ground())
        if aa is not None:
            self._antialias(aa, c2b, kinv)

    def _set(self, gen, field, kw, bias, b2w, w2b, window, W, S, st):
        """Everything behind the begin entry, on a batch st of E elements x W * W rays that oi_scene_begin or
        oi_scene_aa_begin has filled: the march, the finish, the depth resolve, the visible lists, the gather, the full MLP
        pass at the visible hits and their prefix offsets.  What the primary surface and the sub-sample surface share."""
        E, dev = st.E, b2w.device
        self.gen, self.field, self.kw, self.bias = gen, field, kw, bias
        self.E, self.W, self.S, self.N = E, W, S, W * W
        self.b2w, self.w2b, self.window, self.state = b2w, w2b, window, st
        self.n_evals = self.n_steps = self.shadow_evals = self.occlusion_evals = self.transfer_evals = self.n_pad = 0
        self.n_hit = self.n_vis = [0] * E
        self.owner = self.owner_ray = self.vis_slot = self.offset = self.points = self.grad = self.rgb = None
        self._world = self._pixel = self.vis_index = self.shadow = self.ao = self.transfer_state = None
        self.glossy_evals, self.glossy_state, self._reflect = 0, None, None
        self.bounce_points, self.bounce_hits = 0, None
        self.aa = self.sub = self.edge_slot = None   # the anti-aliasing stage (_antialias), when there is one
        self._grounds = {}                           # GroundSurface per ground record (ground())
        self.n_edge = 0
        bound = int(st.live[0].item())
        self.n_entered = st.counts[:, 0].tolist()
        if bound == 0:      # nothing enters a window: every ray is a MISS already
            return
        total, self.n_steps = _t._march_batch(self.field, st, *self.kw, bound=bound)
        self.n_evals = total
        hit_index, _ = ops.trace_batch_finish(st)
        if int(st.live[-1].item()) == 0:   # nothing is hit
            return
        self.n_hit = st.counts[:, -1].tolist()
        self.owner, self.owner_ray = ops.scene_resolve(st, self.window, W, S)
        vis_index, self.vis_slot = ops.scene_visible(st, self.owner, self.window, W, S)
        self.vis_index = vis_index
        self.n_pad = int(st.live[-1].item())
        self.n_vis = st.counts[:, -1].tolist()
        self.points = ops.trace_batch_gather(st, vis_index, self.n_pad)
        _, grad, rgb = self.field.full(self.points.view(E * self.n_pad, 3))
        self.grad, self.rgb = grad.view(E, self.n_pad, 3), rgb.view(E, self.n_pad, 3)
        self.offset = torch.tensor(np.concatenate([[0], np.cumsum(self.n_vis)[:-1]]), dtype=torch.int32, device=dev)

    @classmethod
    def from_batch(cls, parent, st, Q):
        """The SceneSurface of a begun batch st of parent.E elements x Q * Q rays whose layout is a VIRTUAL scene image of Q x
        Q pixels (include/oi_scene_aa.h): every window is the whole image, local ray q of every element is virtual pixel q.
        Field, trace parameters, bias and poses are the parent's."""
        self = cls.__new__(cls)
        window = torch.zeros(parent.E, 2, dtype=torch.int32, device=parent.b2w.device)
        self._set(parent.gen, parent.field, parent.kw, parent.bias, parent.b2w, parent.w2b, window, Q, Q, st)
        return self

    def _antialias(self, aa, c2b, kinv):
        """The anti-aliasing stage (include/oi_scene_aa.h): the flagged scene pixels (adaptive:
        oi_scene_aa_classify and ONE read-back of their number; otherwise every scene pixel), per instance their aa.S - 1
        sub-pixel rays each (oi_scene_aa_begin), and everything _set does, on those rays.  self.sub: the sub-samples as one more
        SceneSurface over a virtual image of Q x Q pixels -- virtual pixel (j - 1) * n_edge + e is sample j of the e-th
        flagged pixel in ascending order -- which the light-dependent stages treat as they treat this one; None without a
        flagged pixel or without a primary hit."""
        M, dev = self.S * self.S, self.b2w.device
        self.aa = aa
        self.edge_slot = torch.full((M,), -1, dtype=torch.int32, device=dev)
        if self.n_pad == 0:
            return
        edge_index, self.edge_slot, n_edge = _t._flagged(aa, M, dev, lambda: ops.scene_aa_classify(
            self.owner, self.owner_ray, self.vis_slot, self.points, self.grad, self.n_pad, self.S, aa.plane, aa.cos))
        self.n_edge = n_edge
        if n_edge == 0:
            return
        Q = virtual_image_size((aa.S - 1) * n_edge, self.E, "trace_scene")
        st = ops.trace_batch_state_empty(self.E, Q * Q, self.b2w)
        ops.scene_aa_begin(st, c2b, kinv, self.window, self.W, self.S, edge_index, n_edge, torch.from_numpy(aa.offsets).to(dev))
        self.sub = SceneSurface.from_batch(self, st, Q)

    def world_points(self):
        """position, normal (n_vis, 3) in the world frame and elem (n_vis,) int32 of the visible points of all instances, point
        offset[e] + slot; computed once."""
        if self._world is None:
            self._world = ops.scene_points(self.state, self.points, self.grad, self.n_pad, self.offset, sum(self.n_vis), self.b2w,
                                           self.w2b)
        return self._world

    def point_pixels(self):
        """(n_vis,) int32: the scene pixel of every visible point, the key of its sample sequence; computed once."""
        if self._pixel is None:
            self._pixel = ops.scene_point_pixels(self.state, self.vis_index, self.window, self.W, self.S, self.offset,
                                                 sum(self.n_vis))
        return self._pixel

    def ground(self, ground):
        """The ground plane `ground` (a Ground) in this scene: -> GroundSurface, its ground pixels classified against the owner
        map (oi_ground_begin) and listed in ascending order; cached per record.  Refused: a scene traced with aa_samples > 1, a
        camera on or below the plane."""
        if isinstance(ground, GroundSurface):
            return ground
        if not isinstance(ground, Ground):
            raise ValueError(f"SceneSurface.ground: ground={ground!r} (an oi_amd.scene.Ground)")
        if getattr(self, "aa", None) is not None:
            raise ValueError(f"SceneSurface.ground: the scene was traced with aa_samples={self.aa.S}; the ground plane has no "
                             "anti-aliasing stage yet (trace the scene with aa_samples=1)")
        key = ground.packed().tobytes()
        if key not in self._grounds:
            self._grounds[key] = GroundSurface(self, ground)
        return self._grounds[key]

    def _sampled(self, what, samples, seed, max_shadow_rays, resolve, lights=None, radius=None, distance=None, *, lobe=None,
                 anyhit=True, local=False, ground=None):
        """The sampled any-hit trace against every instance, in chunks of the samples: a chunk holds E * L * Sc * n_vis rays, Sc
        the largest number for which that stays within max_shadow_rays and below 2^31.  resolve(sb, j0, Sc, last) accumulates
        each finished chunk.  lights and radius: caps about the lights; distance: the hemisphere about the normal; lobe (a
        shininess): the reflection lobe about the reflected view vector (include/oi_scene_gloss.h).  anyhit False: the same rays
        marched to their CLOSEST hit (oi_trace_batch_step), what the bounce follows (include/oi_scene_bounce.h).  local: `lights`
        are local records (L, 20) and the rays are aimed at them and end there (include/oi_local_light.h).  ground (a
        GroundSurface; caps and the hemisphere only): the plane blocks the owner's ray of every finished chunk
        (oi_ground_occlude) before its resolve.  -> (sdf evaluations per element, the last chunk's state)."""
        L, n_vis = 1 if lights is None else lights.shape[0], self.n_points
        per = self.E * L * n_vis
        chunks = _t.sample_chunks(samples, per, max_shadow_rays, what,
                                  f"{self.E} instances x {L} lights x {n_vis} visible points = {per} rays per sample")
        pos, nrm, elem = self.world_points()
        pixel = self.point_pixels()
        points = (self.points, self.grad, self.n_pad, self.offset, elem, pixel, pos, nrm, n_vis, self.w2b, self.bias, samples)
        if local:
            begin = lambda sb, j0, c: ops.scene_local_light_begin(sb, *points, j0, c, lights, seed)
        elif lobe is None:
            begin = lambda sb, j0, c: ops.scene_occlusion_begin(sb, *points, j0, c, seed, lights, radius, distance)
        else:
            begin = lambda sb, j0, c: ops.scene_lobe_begin(sb, self.state.rays_o, self.vis_index, self.N, *points, j0, c, lobe, seed)
        done = resolve
        if ground is not None:
            def done(sb, j0, c, last):
                ops.ground_occlude(sb, ground.record, elem, self.b2w, n_vis, math.inf if distance is None else distance)
                resolve(sb, j0, c, last)
        return _t.sampled_trace(self.field, self.kw, pos, self.E, L * n_vis, samples, chunks, begin, done, anyhit)

    def visibility(self, lights, radius=None, samples=1, seed=0, max_shadow_rays=MAX_SHADOW_RAYS, ground=None):
        """(L, S * S) visibility of `lights` (L, 16).  radius None (or all zero) and one sample: one shadow ray per light and
        visible point, marched against EVERY instance in one batch of E occluder elements; a pixel is lit (1) when its ray
        missed them all, else 0.  Otherwise radius (L,) holds the lights' angular radii and `samples` rays per light and
        visible point sample each light's cap, every ray tested against every instance in its any-hit form: the share in
        [0, 1] of a pixel's samples that reach the light.  Split into chunks of samples above max_shadow_rays.
        ground (a Ground): the plane blocks the instances' shadow rays too (oi_ground_occlude on each chunk)."""
        L, n_vis = lights.shape[0], sum(self.n_vis)
        ground = None if ground is None else self.ground(ground)
        if n_vis == 0:
            return torch.ones(L, self.S * self.S, device=lights.device)
        if radius is not None:
            radius = torch.as_tensor(radius, dtype=torch.float32).reshape(-1).to(lights.device)
        if int(samples) != 1 or (radius is not None and bool((radius != 0).any())):
            if radius is None:
                radius = torch.zeros(L, device=lights.device)
            M = self.S * self.S
            count, out = ops._new(lights, L, M).view(torch.int32), ops._new(lights, L, M)
            resolve = lambda sb, j0, c, last: ops.scene_occlusion_resolve(
                sb.status, self.owner, self.owner_ray, self.vis_slot, self.offset, self.E, self.N, L, samples, j0, c, n_vis, self.S,
                count, out, last)
            evals, self.shadow = self._sampled("SceneSurface.shade", samples, seed, max_shadow_rays, resolve, lights, radius,
                                               ground=ground)
            self.shadow_evals += evals
            return out
        rays = self.E * L * n_vis
        if rays > max_shadow_rays or rays >= 1 << 31:
            raise ValueError(f"SceneSurface.shade: {self.E} instances x {L} lights x {n_vis} visible points = {rays} shadow rays "
                             f"(at most max_shadow_rays={max_shadow_rays} and below 2^31; inference.scene_light_walk splits the lights)")
        pos, nrm, elem = self.world_points()
        sb = ops.trace_batch_state_empty(self.E, L * n_vis, pos)
        ops.scene_shadow_begin(sb, self.points, self.grad, self.n_pad, self.offset, elem, pos, nrm, n_vis, lights, self.w2b, self.bias)
        bound = int(sb.live[0].item())
        if bound:
            total, _ = _t._march_batch(self.field, sb, *self.kw, bound=bound)
            self.shadow_evals += total
            ops.trace_batch_finish(sb)   # in-flight rays -> LIMIT
        if ground is not None:
            ops.ground_occlude(sb, ground.record, elem, self.b2w, n_vis, math.inf)
        self.shadow = sb
        return ops.scene_visibility(sb.status, self.owner, self.owner_ray, self.vis_slot, self.offset, self.E, self.N, L, n_vis, self.S)

    def local_visibility(self, lights, samples=1, seed=0, max_shadow_rays=MAX_SHADOW_RAYS):
        """(L, S * S) visibility of the local lights `lights` (L, 20), world frame (include/oi_local_light.h): `samples` rays per
        light and visible point, aimed at the light's sphere and ending there, every ray tested against EVERY instance in its
        any-hit form: the share of a pixel's samples that reach the light.  An instance beyond the light throws no shadow.
        Split into chunks of samples above max_shadow_rays, which changes no byte."""
        L, n_vis, M = lights.shape[0], sum(self.n_vis), self.S * self.S
        if n_vis == 0:
            return torch.ones(L, M, device=lights.device)
        acc = []   # count, out: taken with the first chunk, so a trace that is refused leaves no output behind

        def resolve(sb, j0, c, last):
            if not acc:
                acc.extend((ops._new(lights, L, M).view(torch.int32), ops._new(lights, L, M)))
            ops.scene_occlusion_resolve(sb.status, self.owner, self.owner_ray, self.vis_slot, self.offset, self.E, self.N, L, samples,
                                        j0, c, n_vis, self.S, acc[0], acc[1], last)
        evals, self.shadow = self._sampled("SceneSurface.shade", samples, seed, max_shadow_rays, resolve, lights, local=True)
        self.shadow_evals += evals
        return acc[1]

    def ambient(self, samples, distance, seed=0, max_shadow_rays=MAX_SHADOW_RAYS, ground=None):
        """(S * S,) ambient occlusion: the share of `samples` cosine-weighted hemisphere rays per visible point that meet no
        instance -- the point's own or any other -- within `distance` (world units; inf allowed); 1 off the mask.  ground (a
        Ground): nor the plane (oi_ground_occlude on each chunk): an instance darkens where it nears the ground."""
        M, n_vis, dev = self.S * self.S, sum(self.n_vis), self.b2w.device
        ground = None if ground is None else self.ground(ground)
        if n_vis == 0:
            return torch.ones(M, device=dev)
        count, out = ops._new(self.b2w, 1, M).view(torch.int32), ops._new(self.b2w, 1, M)
        resolve = lambda sb, j0, c, last: ops.scene_occlusion_resolve(
            sb.status, self.owner, self.owner_ray, self.vis_slot, self.offset, self.E, self.N, 1, samples, j0, c, n_vis, self.S, count,
            out, last)
        evals, self.ao = self._sampled("SceneSurface.ambient", samples, seed, max_shadow_rays, resolve, distance=float(distance),
                                       ground=ground)
        self.occlusion_evals += evals
        return out.view(M)

    def transfer(self, samples, seed=0, max_shadow_rays=MAX_SHADOW_RAYS):
        """(9, S * S) SH transfer map of the scene in the WORLD frame (include/oi_scene_light.h): ambient()'s rays without a
        distance limit, resolved into the mean of [escaped every instance] y_c(world direction) per pixel; samples == 0: the
        unshadowed closed form, nothing traced.  Zeros off the mask."""
        M, n_vis = self.S * self.S, sum(self.n_vis)
        if n_vis == 0:
            return torch.zeros(_l.ENV_COEFFS, M, device=self.b2w.device)
        if samples == 0:
            return ops.scene_transfer_normal(self.grad, self.n_pad, self.owner, self.owner_ray, self.vis_slot, self.w2b, self.E, self.N,
                                             self.S)
        out = ops._new(self.b2w, _l.ENV_COEFFS, M)
        resolve = lambda sb, j0, c, last: ops.scene_transfer_resolve(
            sb.status, sb.rays_d, self.owner, self.owner_ray, self.vis_slot, self.offset, self.w2b, self.E, self.N, samples, j0, c,
            n_vis, self.S, out, last)
        evals, self.transfer_state = self._sampled("SceneSurface.capture_transfer", samples, seed, max_shadow_rays, resolve,
                                                   distance=math.inf)
        self.transfer_evals += evals
        return out

    def transfer_bounce(self, samples, seed=0, max_shadow_rays=MAX_SHADOW_RAYS):
        """transfer()'s (9, S * S) map and the bounce transfer (3, 9, S * S) of the same rays (include/oi_scene_bounce.h): the rays
        are marched to their closest hit in every instance; per chunk the direct transfer is resolved as by transfer(), then
        the nearest instance of every ray is found, the full MLP pass runs at the hits that win (E * n_pad2 points; skipped
        when nothing wins) and oi_scene_bounce_resolve folds their albedo and normals into the running sums.  samples >= 1.
        Without a visible point: zeros, nothing launched."""
        M, n_vis, E = self.S * self.S, sum(self.n_vis), self.E
        if n_vis == 0:
            return (torch.zeros(_l.ENV_COEFFS, M, device=self.b2w.device), torch.zeros(3, _l.ENV_COEFFS, M, device=self.b2w.device))
        out, bounce = ops._new(self.b2w, _l.ENV_COEFFS, M), ops._new(self.b2w, 3, _l.ENV_COEFFS, M)

        def resolve(sb, j0, c, last):
            ops.scene_transfer_resolve(sb.status, sb.rays_d, self.owner, self.owner_ray, self.vis_slot, self.offset, self.w2b, E, self.N,
                                       samples, j0, c, n_vis, self.S, out, last)
            winner = ops.scene_bounce_nearest(sb.status, sb.t, E, sb.N)
            sel_index, sel_slot = ops.scene_bounce_visible(sb, winner)
            n_pad2 = int(sb.live[-1].item())
            points2 = grad2 = rgb2 = None
            if n_pad2:
                self.bounce_points += sum(sb.counts[:, -1].tolist())
                points2 = ops.trace_batch_gather(sb, sel_index, n_pad2)
                _, grad2, rgb2 = self.field.full(points2.view(E * n_pad2, 3))
                grad2, rgb2 = grad2.view(E, n_pad2, 3), rgb2.view(E, n_pad2, 3)
            ops.scene_bounce_resolve(winner, sel_slot, sb.rays_d, grad2, rgb2, n_pad2, self.owner, self.owner_ray, self.vis_slot,
                                     self.offset, self.w2b, E, self.N, samples, j0, c, n_vis, self.S, bounce, last)
            # what oi_scene_bounce_resolve read for the last chunk (samples j0 .. j0 + c - 1; ray jj * n_vis + g)
            self.bounce_hits = dict(j0=j0, chunk=c, winner=winner, sel_index=sel_index, sel_slot=sel_slot, n_pad2=n_pad2,
                                    points=points2, grad=grad2, rgb=rgb2)

        evals, self.transfer_state = self._sampled("SceneSurface.capture_transfer", samples, seed, max_shadow_rays, resolve,
                                                   distance=math.inf, anyhit=False)
        self.transfer_evals += evals
        return out, bounce

    def lobe_visibility(self, samples, shininess, seed=0, max_shadow_rays=MAX_SHADOW_RAYS):
        """(S * S,) reflection-lobe visibility V_spec (include/oi_scene_gloss.h): the share of `samples` rays per visible point,
        distributed as cos^shininess about the reflected view vector, that are above the point's horizon and meet no instance
        -- the point's own or any other; 1 off the mask.  Chunked as ambient()."""
        M, n_vis = self.S * self.S, sum(self.n_vis)
        if n_vis == 0:
            return torch.ones(M, device=self.b2w.device)
        count, out = ops._new(self.b2w, 1, M).view(torch.int32), ops._new(self.b2w, 1, M)
        resolve = lambda sb, j0, c, last: ops.scene_occlusion_resolve(
            sb.status, self.owner, self.owner_ray, self.vis_slot, self.offset, self.E, self.N, 1, samples, j0, c, n_vis, self.S, count,
            out, last)
        evals, self.glossy_state = self._sampled("SceneSurface.lobe_visibility", samples, seed, max_shadow_rays, resolve,
                                                 lobe=float(shininess))
        self.glossy_evals += evals
        return out.view(M)

    def reflection(self):
        """(S * S, 3): the reflected view vector of every scene pixel in the world frame (the lookup direction of the glossy
        shade), zeros off the mask; computed once."""
        if self._reflect is None:
            if self.n_pad == 0:
                self._reflect = torch.zeros(self.S * self.S, 3, device=self.b2w.device)
            else:
                self._reflect = ops.scene_reflect(self.state.rays_o, self.points, self.grad, self.n_pad, self.owner, self.owner_ray,
                                                  self.vis_slot, self.w2b, self.E, self.N, self.S)
        return self._reflect

    def capture_transfer(self, transfer_samples=64, seed=0, max_shadow_rays=MAX_SHADOW_RAYS, glossy_samples=None, shininess=None,
                         bounces=0):
        """The scene prepared for environment lighting: `transfer_samples` (0 .. 256) cosine-weighted rays per visible point,
        each tested against EVERY instance, resolved into a 9-coefficient world-frame transfer vector per scene pixel (0: the
        unshadowed closed form, nothing traced).
        Glossy environments (oi_amd.envlight.EnvMap): glossy_samples in 1 .. 256 also traces that many rays per visible point
        about the reflected view vector, distributed as cos^shininess and tested against every instance, into spec_visibility;
        shininess None takes the generator's learned value; glossy_samples = 0 prepares a glossy capture without that trace
        (V_spec = 1), and a shininess without glossy_samples is refused (oi_amd.trace.capture_transfer's rules).  With both left
        at None the launches and outputs are those of a call without them.
        bounces = 1 (the integer; with transfer_samples >= 1, not with the glossy keywords) follows the transfer rays to their
        nearest intersection with ANY instance and folds one diffuse interreflection bounce between the instances -- and of an
        instance on itself -- into a per-channel transfer, SceneTransfer.bounce (include/oi_scene_bounce.h has the estimator and
        its approximations); the direct transfer is bit for bit that of bounces = 0, which launches what it always did.
        (The transfer map knows no ground plane: render_scene_env and inference.scene_env_walk refuse ground=; DESIGN section
        4.31.)
        -> SceneTransfer."""
        aa = getattr(self, "aa", None)
        if aa is not None:
            raise ValueError(f"SceneSurface.capture_transfer: the scene was traced with aa_samples={aa.S}; the environment "
                             "paths have no anti-aliasing stage (trace the scene with aa_samples=1)")
        samples, seed = _t._check_transfer(transfer_samples, seed, "SceneSurface.capture_transfer")
        bounces = _t._check_bounces(bounces, samples, glossy_samples, shininess, "SceneSurface.capture_transfer")
        g_samples, shin, spec = _t._check_glossy(getattr(self, "gen", None), glossy_samples, shininess, "SceneSurface.capture_transfer")
        if bounces:
            transfer, bounce = self.transfer_bounce(samples, seed, max_shadow_rays)
        else:
            transfer, bounce = self.transfer(samples, seed, max_shadow_rays), None
        out = self._shade(None, None, outputs=self.OUTPUTS[:-1])
        if g_samples is None:
            return SceneTransfer(self, transfer, out, samples, bounce=bounce)
        vis = self.lobe_visibility(g_samples, shin, seed, max_shadow_rays) if g_samples else None
        return SceneTransfer(self, transfer, out, samples, g_samples, shin, spec, vis, self.reflection())

    def _shade(self, lt, bg, visibility=None, outputs=OUTPUTS, image_out=None, ao=None):
        """ops.scene_shade on this scene (ao: ops.scene_shade_ao, the occlusion factor (S * S,) on the ambient
        term); without a visible hit nothing is launched and every map is its off-mask value."""
        M, dev = self.S * self.S, lt.device if lt is not None else self.b2w.device
        if self.n_pad:
            args = (self.state, self.W, self.S, self.owner, self.owner_ray, self.vis_slot, self.points, self.grad, self.rgb, self.n_pad,
                    self.w2b, self.b2w, lt, bg, visibility)
            if lt is not None and _t._is_local(lt):   # local lights: their own kernel
                return ops.scene_shade_local(*args, ao, outputs, image_out)
            return ops.scene_shade(*args, outputs, image_out) if ao is None else ops.scene_shade_ao(*args, ao, outputs, image_out)
        res = {}
        for k in outputs:
            if k == "image":
                fill = (torch.zeros(3, device=dev) if bg is None else bg).view(1, 3, 1).expand(lt.shape[0], 3, M)
                res[k] = fill.contiguous() if image_out is None else image_out.copy_(fill)
            elif k == "instance":
                res[k] = torch.full((M,), -1, dtype=torch.int32, device=dev)
            elif k == "depth":
                res[k] = torch.full((M,), float("nan"), device=dev)
            else:
                res[k] = torch.zeros((M,) if ops.SCENE_OUT[k] == (1,) else (M, 3), device=dev)
        return res

    def shade(self, lights=None, shadows=False, bg=None, max_shadow_rays=MAX_SHADOW_RAYS, shadow_samples=1, light_radius=0.0,
              ao_samples=0, ao_distance=0.5, seed=0, ground=None):
        """The scene under `lights` (oi_amd.relight.Light objects in the WORLD frame; default the generator's trained light; at
        most RELIGHT_MAX_LIGHTS; or oi_amd.relight.LocalLight objects, lights that stand between the instances: their shadow
        rays end at the light, shadow_samples sample the light's own sphere and light_radius must stay 0).  -> dict of image (L, 3, S, S); depth (the ray parameter; NaN off the mask), mask, instance
        (int32, -1 off the mask) (1, 1, S, S); position (world frame), normal_map (world frame), albedo (1, 3, S, S);
        visibility (L, 1, S, S) when `shadows` (refused above max_shadow_rays = E * L * n_vis rays); stats.  bg: (3,)
        background colour (black when None).
        Soft shadows: light_radius (radians; a scalar or one value per light) and shadow_samples (1 .. 256), as
        oi_amd.trace.render_surface takes them: `visibility` is the share in [0, 1] of the samples that reach the light past
        EVERY instance.  Ambient occlusion: ao_samples > 0 rays over each visible point's hemisphere as far as ao_distance (world
        units), tested against every instance; the share that escapes multiplies the ambient term and is returned as
        ambient_occlusion (1, 1, S, S).  The samples are a function of scene pixel, sample number and `seed` alone; traces
        above max_shadow_rays are split into chunks of samples, which changes no byte.  At the defaults the launches and the
        bytes are those of a call without these arguments.
        On a scene traced with aa_samples > 1 (trace_scene) the sub-sample surface passes the same stages
        with the same arguments and `image` is the mean over each flagged pixel's samples, off-surface samples carrying bg; new
        keys coverage (1, 1, S, S), the mean of the mask over a pixel's samples, and aa_mask (1, 1, S, S), the flagged pixels;
        every other map stays the centre sample's.
        ground (a Ground): a plane in the world that is visible where no instance is nearer, shaded as a
        Lambertian surface under the lights, and that catches the instances' shadows (with `shadows`) and ambient occlusion
        (with ao_samples) and blocks their own ambient and directional shadow rays (not their local-light rays).  It is
        written into every map at its pixels -- there mask = 0 and instance = -1 -- and adds ground_mask (1, 1, S, S) and
        shadow_matte (L, 3, S, S), the shaded ground over the unoccluded one (1 off the ground; composite_over); stats gains
        ground_pixels and ground_evals.  Refused on a scene traced with aa_samples > 1.  None: the launches and bytes of a
        call without the keyword."""
        dev = self.b2w.device
        gs = None if ground is None else self.ground(ground)
        lt = _t._stack_lights(self.gen, lights, dev, "SceneSurface.shade", "; inference.scene_light_walk splits larger sets")
        occlusion = _t._checked_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, lt, "SceneSurface.shade")
        S = self.S

        def grounded(planes):   # the ground's own secondary rays, and the plane into the shaded planes
            ground_mask, matte = gs.shade(planes, lt, *_t._occlusion(gs, lt, *occlusion, max_shadow_rays))
            return {"ground_mask": ground_mask.view(1, 1, S, S), "shadow_matte": matte.view(-1, 3, S, S)}
        res = _t._lit_stages(self, lt, _t._bg(bg, dev), occlusion, max_shadow_rays, gs, None if gs is None else grounded)
        res["stats"] = self.stats()
        if gs is not None:
            for st in res["stats"]:
                st.update(ground_pixels=gs.n_g, ground_evals=gs.evals)
        return res

    def stats(self):
        """Per instance: rays entered and culled, rays per status (culled rays are misses), hits, visible hits; sdf
        evaluations of the primary march and of the shadow, ambient-occlusion, transfer and reflection-lobe marches so far (every
        instance carries the batch's bound); bounce_points: the secondary hits the bounce evaluated, over all chunks and instances."""
        st = self.state
        per = torch.stack([torch.bincount(st.status[e].long(), minlength=6)[:6] for e in range(self.E)]).tolist()
        out = []
        for e in range(self.E):
            s = {name: int(per[e][code]) for code, name in _l.TRACE_STATUS_NAMES.items()}
            s.update(n_rays=self.N, entered=int(self.n_entered[e]), culled=self.N - int(self.n_entered[e]), hits=int(self.n_hit[e]),
                     visible=int(self.n_vis[e]), n_evals=self.n_evals, n_steps=self.n_steps, shadow_evals=self.shadow_evals,
                     occlusion_evals=self.occlusion_evals, transfer_evals=self.transfer_evals, glossy_evals=self.glossy_evals,
                     bounce_points=self.bounce_points)
            if self.aa is not None:   # aa_evals: every sdf evaluation the sub-samples cost (their march, shadow and occlusion rays)
                sub = self.sub
                s.update(aa_pixels=self.n_edge, aa_rays=(self.aa.S - 1) * self.n_edge,
                         aa_evals=0 if sub is None else sub.n_evals + sub.shadow_evals + sub.occlusion_evals)
            out.append(s)
        return out


class SceneTransfer:
    """One traced scene and its SH transfer map: everything shade() needs, none of which depends on the light.
    scene: the SceneSurface; transfer (1, 9, S, S), world frame; maps: SceneSurface.shade's G-buffer maps (depth, position,
    normal_map, albedo, mask, instance); samples: the rays per visible point (0: the closed form).  A capture made with
    glossy_samples also holds the shininess its lobe was traced for, specular (the learned specular colour), spec_visibility
    (1, 1, S, S) (None with glossy_samples = 0: V_spec = 1) and reflection (1, 3, S, S), the world-frame reflected view vector.
    A capture made with bounces=1 also holds bounce (1, 3, 9, S, S), the per-channel transfer of one diffuse interreflection
    bounce between the instances (None otherwise; include/oi_scene_bounce.h)."""

    def __init__(self, scene, transfer, planes, samples, glossy_samples=None, shininess=None, specular=None, spec_vis=None,
                 reflection=None, bounce=None):
        S = scene.S
        self.scene, self.samples, self.S = scene, samples, S
        self._transfer = transfer                       # (9, S * S), planar: what oi_env_shade reads
        self.transfer = transfer.view(1, _l.ENV_COEFFS, S, S)
        self._bounce = bounce                           # (3, 9, S * S), planar, or None: what oi_env_shade_bounce reads
        self.bounce = None if bounce is None else bounce.view(1, 3, _l.ENV_COEFFS, S, S)
        self.maps = {_t._MAP_NAMES[k]: v for k, v in _t._maps(planes, S, S).items()}
        # oi_env_shade's view of the scene's planes: every scene pixel is a ray, the owned ones are hits at their own index
        M, dev = S * S, transfer.device
        on = planes["instance"] >= 0
        self._status = on.to(torch.uint8) * _l.TRACE_HIT
        self._hit_slot = torch.where(on, torch.arange(M, dtype=torch.int32, device=dev), torch.full((M,), -1, dtype=torch.int32, device=dev))
        self._rgb = planes["albedo"]
        # glossy_samples: None = never mentioned (a glossy shade is refused), 0 = no lobe trace on purpose (V_spec = 1)
        self.glossy_samples, self.shininess, self.specular = glossy_samples, shininess, specular
        self._spec_vis, self._reflect = spec_vis, reflection     # (S * S,) or None; (S * S, 3) or None
        self.spec_visibility = None if spec_vis is None else spec_vis.view(1, 1, S, S)
        self.reflection = None if reflection is None else reflection.view(S, S, 3).permute(2, 0, 1)[None]

    def shade(self, envs, bg=None, specular=None):
        """The scene under each of `envs` (any number: launches of ENV_MAX_ENVS).
        EnvLight objects: -> {"image": (F, 3, S, S) = max(shading, 0) albedo on the mask, bg off it; "shading": (F, 3, S, S), not
        clamped; the G-buffer maps; "stats"}.  On a capture made with bounces=1 (oi_env_shade_bounce) shading = direct + indirect, and
        "indirect": (F, 3, S, S) is the bounce's part.
        EnvMap objects (every element; a mixed list is refused), on a capture made with glossy_samples: the glossy path
        (include/oi_scene_gloss.h), image = max(shading, 0) albedo + specular and "specular": (F, 3, S, S) = k_s V_spec
        G_s(reflected view vector), V_spec knowing every instance.  k_s = `specular`: None takes the generator's learned specular
        colour, a scalar or an RGB triple overrides it.  The maps' shininess must be the capture's."""
        from .envlight import EnvLight, EnvMap, stack_envs, stack_maps
        seq = [envs] if isinstance(envs, (EnvLight, EnvMap)) else list(envs)
        if not seq or not all(isinstance(e, (EnvLight, EnvMap)) for e in seq):
            raise ValueError("SceneTransfer.shade: EnvLight objects only, or EnvMap objects only")
        glossy = any(isinstance(e, EnvMap) for e in seq)
        if glossy and not all(isinstance(e, EnvMap) for e in seq):
            raise ValueError("SceneTransfer.shade: EnvMap and EnvLight objects in one list (shade them in two calls)")
        if not glossy and specular is not None:
            raise ValueError("SceneTransfer.shade: specular= needs EnvMap environments (an EnvLight has no glossy half)")
        bounce = getattr(self, "_bounce", None)
        if glossy and bounce is not None:
            raise ValueError("SceneTransfer.shade: EnvMap environments on a capture made with bounces=1 (the glossy shade has no "
                             "bounce input yet; shade EnvLight objects, or capture without the bounce)")
        if glossy and self.glossy_samples is None:
            raise ValueError("SceneTransfer.shade: this capture has no reflection-lobe trace; capture_transfer(glossy_samples=S) "
                             "traces one, glossy_samples=0 with a shininess states that V_spec = 1 is meant")
        if glossy and any(e.shininess != self.shininess for e in seq):
            raise ValueError(f"SceneTransfer.shade: maps prefiltered for shininess {sorted({e.shininess for e in seq})}, the "
                             f"capture's lobe is {self.shininess:g}")
        s, S = self.scene, self.S
        dev, M = self._transfer.device, S * S
        F = len(seq)
        bgv = _t._bg(bg, dev)
        names = ops.ENV_GLOSSY_OUT if glossy else ops.ENV_SHADE_OUT if bounce is None else ops.ENV_BOUNCE_OUT
        view = (self._status, self._hit_slot, self._rgb, M, self._transfer)
        if s.n_pad == 0:   # no hit at all: nothing is launched
            out = {k: ops._new(self._transfer, F, 3, M) for k in names}
            for k in names:
                if k != "image":
                    out[k].zero_()
            out["image"].copy_((torch.zeros(3, device=dev) if bgv is None else bgv).view(1, 3, 1).expand(F, 3, M))
        elif not glossy:
            ev = stack_envs(seq, dev)
            if bounce is None:
                launch = lambda a, b, out: ops.env_shade(*view, ev[a:b], bgv, out=out)
            else:
                launch = lambda a, b, out: ops.env_shade_bounce(*view, bounce, ev[a:b], bgv, out=out)
            out = _t._shade_chunks(self._transfer, names, F, M, launch)
        else:
            ks = self.specular if specular is None else specular
            ks = torch.as_tensor(np.broadcast_to(np.asarray(ks, dtype=np.float32), (3,)).copy()).to(dev)

            def launch(a, b, out):
                ev, maps, index, rot, _ = stack_maps(seq[a:b], dev)
                ops.env_shade_glossy_dirs(*view, ev, self._reflect, self._spec_vis, maps, index, rot, ks, bgv, out=out)
            out = _t._shade_chunks(self._transfer, names, F, M, launch)
        res = {k: v.view(F, 3, S, S) for k, v in out.items()}
        res.update(self.maps)
        res["stats"] = s.stats()
        return res


@torch.no_grad()
def trace_scene(gen, zs, b2ws, window=None, bias=DEFAULT_BIAS, aa_samples=1, aa_adaptive=True, aa_plane=_l.AA_DEFAULT_PLANE,
                aa_cos=_l.AA_DEFAULT_COS, aa_pattern=None, **trace_kw):
    """The scene of K instances of `gen` (latents zs: K of (z_dim,) or (K, z_dim); rigid poses b2ws: K of (4, 4), as
    sample_prior takes them), 1 <= K <= 1024, in the S x S scene image of the generator's camera (S = gen.scene_resolution),
    traced once: -> SceneSurface.  window: the side W of every instance's window in scene pixels (default: the smallest that
    holds every unit sphere's projection; scene_windows); K * W^2 < 2^31.  trace_kw: tol, omega, max_steps, readback of
    sphere_trace.  Refused with ValueError, naming the instance: a camera inside or within 1 of an instance's unit sphere, an
    instance behind the camera.
    Anti-aliasing (include/oi_scene_aa.h): aa_samples = Sa in 2 .. 64 takes Sa samples inside each FLAGGED
    scene pixel -- the centre and Sa - 1 sub-pixel rays per instance at aa_pattern (Sa, 2), oi_amd.trace.render_surface's
    keywords with its default pattern.  A pixel is flagged when a neighbour differs in the mask or belongs to another
    instance, or -- same instance -- lies off its tangent plane by more than asin(aa_plane) or has a normal more than
    acos(aa_cos) away; aa_adaptive=False flags every scene pixel.  The sub-samples are SceneSurface.sub, one more SceneSurface
    over a virtual image of Q x Q pixels, Q = ceil(sqrt((Sa - 1) * flagged pixels)); K * Q^2 >= 2^31 is refused.  With
    aa_samples == 1 nothing of this runs."""
    aa = _t._check_aa(aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, "trace_scene")
    return SceneSurface(gen, zs, b2ws, window, bias, trace_kw, aa=aa)


@torch.no_grad()
def render_scene(gen, zs, b2ws, lights=None, shadows=False, bg=None, window=None, bias=DEFAULT_BIAS,
                 max_shadow_rays=MAX_SHADOW_RAYS, shadow_samples=1, light_radius=0.0, ao_samples=0, ao_distance=0.5, seed=0,
                 aa_samples=1, aa_adaptive=True, aa_plane=_l.AA_DEFAULT_PLANE, aa_cos=_l.AA_DEFAULT_COS, aa_pattern=None,
                 ground=None, **trace_kw):
    """trace_scene + SceneSurface.shade: K instances in one scene image, nearer instances hiding farther ones and, with
    `shadows`, every instance throwing its shadow on itself and on the others; shadow_samples, light_radius, ao_samples,
    ao_distance, seed: shade's soft shadows and ambient occlusion between the instances; aa_samples, aa_adaptive, aa_plane,
    aa_cos, aa_pattern: trace_scene's anti-aliasing; ground: shade's ground plane (a Ground; not with aa_samples > 1).
    -> SceneSurface.shade's dict, with "scene" (the SceneSurface)."""
    rad = light_radius.detach().cpu() if torch.is_tensor(light_radius) else light_radius
    # (before the trace; shade checks a radius per light against the lights it stacks)
    _t._check_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, np.size(rad) if np.ndim(rad) == 1 else 1,
                        "render_scene", local_lights_given(lights))
    aa = _t._check_aa(aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, "render_scene")
    check_ground_keyword(ground, aa, "render_scene")
    s = trace_scene(gen, zs, b2ws, window, bias, aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, **trace_kw)
    res = s.shade(lights, shadows, bg, max_shadow_rays, shadow_samples, light_radius, ao_samples, ao_distance, seed, ground)
    res["scene"] = s
    return res


@torch.no_grad()
def render_scene_env(gen, zs, b2ws, envs, transfer_samples=64, seed=0, bg=None, window=None, bias=DEFAULT_BIAS,
                     max_shadow_rays=MAX_SHADOW_RAYS, glossy_samples=None, shininess=None, specular=None, bounces=0, ground=None,
                     **trace_kw):
    """trace_scene + capture_transfer + shade: K instances in one scene image under the environment lights `envs`
    (oi_amd.envlight.EnvLight objects, or EnvMap objects with glossy_samples given: capture_transfer's and shade's keywords pass
    through), every instance occluding the sky for itself and for the others -- and, on the glossy path, standing in the
    others' reflections.  -> SceneTransfer.shade's dict, with "transfer" (1, 9, S, S), "scene" (the SceneSurface) and "capture"
    (the SceneTransfer); on the glossy path also "specular" (F, 3, S, S), "spec_visibility" (1, 1, S, S) or None and
    "reflection" (1, 3, S, S); with bounces=1 (EnvLight objects only) also "indirect" (F, 3, S, S) and "bounce" (1, 3, 9, S, S):
    the instances colour each other."""
    refuse_env_ground(ground, "render_scene_env")
    samples, _ = _t._check_transfer(transfer_samples, seed, "render_scene_env")
    _t._check_bounces(bounces, samples, glossy_samples, shininess, "render_scene_env")
    _t._check_glossy(gen, glossy_samples, shininess, "render_scene_env")
    s = SceneSurface(gen, zs, b2ws, window, bias, trace_kw)   # (not trace_scene: the environment paths take no aa_* keyword)
    cap = s.capture_transfer(transfer_samples, seed, max_shadow_rays, glossy_samples, shininess, bounces)
    res = cap.shade(envs, bg, specular)
    res.update(transfer=cap.transfer, scene=s, capture=cap)
    if cap.bounce is not None:
        res["bounce"] = cap.bounce
    if cap.glossy_samples is not None:
        res.update(spec_visibility=cap.spec_visibility, reflection=cap.reflection)
    return res
