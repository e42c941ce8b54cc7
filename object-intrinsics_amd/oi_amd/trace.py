"""Sphere-traced surface rendering: ray / surface intersection, a G-buffer at the visible surface point, cast shadows
(include/oi_trace.h).

    sphere_trace     rays against the learned SDF -> per-ray t, status, evaluations, the dense list of hits
    sphere_trace_batch  the same for E latents with N rays each in ONE chain of steps (include/oi_trace_batch.h; DESIGN
                     section 4.17)
    render_surfaces  E views of a Generator (a latent and a pose each): one batched primary trace and one full MLP pass for
                     all of them, then render_surface's light-dependent stages per view
    render_surface   one view of a Generator: depth, position, normals, albedo, mask, the Phong image under L lights,
                     optionally with cast shadows (one shadow ray per light and visible point, or `shadow_samples` rays
                     towards a light of angular radius `light_radius`: penumbrae) and ambient occlusion (`ao_samples` rays
                     over the hemisphere of each visible point; include/oi_occlusion.h)
                     `lights` may also be oi_amd.relight.LocalLight objects: point, spot and sphere lights that stand in the
                     world, whose shadow rays end at the light (include/oi_local_light.h)
                     aa_samples > 1: adaptive anti-aliasing -- the pixels at a geometric edge get sub-pixel rays, which go
                     through the same march and shade, and the image is the mean of a pixel's samples (include/oi_aa.h,
                     DESIGN section 4.29)
    capture_transfer one view's secondary rays traced ONCE into a per-pixel SH transfer map; the TransferCapture is then shaded
                     under any number of environment lights (oi_amd.envlight.EnvLight), 256 per launch
                     (include/oi_envlight.h); with glossy_samples it also traces a reflection-lobe
                     visibility, and the capture is shaded under oi_amd.envlight.EnvMap objects with the learned Phong lobe
                     (include/oi_envgloss.h); with bounces=1 the transfer rays are followed to their
                     nearest intersection and one diffuse interreflection bounce is folded into a per-channel transfer
                     (include/oi_envbounce.h)
    render_surface_env  capture_transfer + shade in one call

The loop runs on the host: oi_trace_begin, then per step the library's sdf-only MLP pass (unchanged) on the rays still in
flight and oi_trace_step, which advances them and compacts the survivors.  The number of rays in flight lives on the device;
the host launches each pass on the last count it read (a valid upper bound: the count never grows) and reads the count back
every step while more than READBACK_DENSE rays were in flight, every READBACK_SPARSE steps after that."""
import ctypes
import dataclasses
from typing import Optional

import numpy as np
import torch

from . import lib as _l
from . import ops
from .fields import LatentField

# read-back cadence of the number of rays in flight (DESIGN section 4.13 has the measurements)
READBACK_DENSE = 1024    # above this many rays a stale bound costs MLP time: read every step
READBACK_SPARSE = 4      # below it a pass is launch-bound whatever its size: read every 4th step

# how far the transfer rays of capture_transfer go: beyond the unit sphere's diameter, so `far` is the sphere's exit
TRANSFER_DISTANCE = 4.0
ENV_MAX_ENVS = _l.ENV_MAX_ENVS   # environments per oi_env_shade launch; larger sets are split

DEFAULT_TOL, DEFAULT_OMEGA, DEFAULT_MAX_STEPS, DEFAULT_BIAS = (_l.TRACE_DEFAULT_TOL, _l.TRACE_DEFAULT_OMEGA,
                                                               _l.TRACE_DEFAULT_MAX_STEPS, _l.TRACE_DEFAULT_BIAS)


@dataclasses.dataclass
class TraceResult:
    """CUDA tensors per ray: t (N,) float32 (the hit's ray parameter; the last sample's otherwise), status (N,) uint8
    (oi_amd.lib.TRACE_*), steps (N,) int16 (sdf evaluations the ray used); hit_index (n_hit,) int32: the rays with
    TRACE_HIT, in no fixed order; n_evals: points sent through the sdf-only MLP pass (the cost, stale bounds included);
    n_steps: loop iterations run.  hit_points (n_hit, 3) and hit_slot (N,) (position in hit_index, or -1) go with hit_index."""
    t: torch.Tensor
    status: torch.Tensor
    steps: torch.Tensor
    hit_index: torch.Tensor
    n_evals: int
    n_steps: int = 0
    hit_points: Optional[torch.Tensor] = None
    hit_slot: Optional[torch.Tensor] = None

    def counts(self):
        """{status name: rays} (one device -> host copy)."""
        c = torch.bincount(self.status.long(), minlength=6).tolist()
        return {name: int(c[code]) for code, name in _l.TRACE_STATUS_NAMES.items()}


def _check_params(tol, omega, max_steps, readback, what):
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or not 1 <= int(max_steps) <= _l.TRACE_MAX_STEPS:
        raise ValueError(f"{what}: max_steps={max_steps!r} (an integer, 1 <= max_steps <= {_l.TRACE_MAX_STEPS})")
    if not (float(tol) > 0 and np.isfinite(float(tol)) and float(omega) > 0 and np.isfinite(float(omega))):
        raise ValueError(f"{what}: tol={tol!r}, omega={omega!r} (both positive and finite)")
    if readback != "auto" and (isinstance(readback, bool) or not isinstance(readback, (int, np.integer)) or int(readback) < 1):
        raise ValueError(f"{what}: readback={readback!r} ('auto' or a positive number of steps)")


def _march(field, st, bound, tol, omega, max_steps, readback, anyhit=False):
    """The one march loop, on a state that a begin entry has filled.  -> (sum of the bounds = points evaluated, per element
    of a batch; steps run).  An ops.TraceState steps with oi_trace_step -- anyhit: oi_occlusion_step, a ray ends at its first
    occluder -- after oi_sdf_mlp_fwd with B = 1 on the first `bound` points, and reads counts[k]; an ops.TraceBatchState steps
    with oi_trace_batch_step (anyhit: oi_trace_batch_step_anyhit) after oi_sdf_mlp_fwd_segments on the first `bound` points of each of its E segments of N, and
    reads live[k], the largest count of any element.  Two launches per step through the C ABI directly, the pointers converted
    and these differences bound once, before the loop: its tail is a handful of rays per step, where the host's time per
    launch is the frame's time."""
    L = _l.load()
    sdf = torch.empty(st.t.shape, dtype=torch.float32, device=st.t.device)   # working memory: step k's pass writes the first `bound`
    pts_p, sdf_p, state_p, stream = ops._p(st.points), ops._p(sdf), ctypes.byref(st.c), ops._stream()
    mlp_args = [pts_p, ops._p(field.packed), ops._p(field.gamma), ops._p(field.beta), sdf_p]
    if isinstance(st, ops.TraceBatchState):
        mlp_name, step_name, counter = "oi_sdf_mlp_fwd_segments", "oi_trace_batch_step_anyhit" if anyhit else "oi_trace_batch_step", st.live
        mlp_args, at = mlp_args + [st.E, bound, st.N, field.prec, field.fast, stream], 6       # at: where the bound goes
    else:
        mlp_name, step_name, counter = "oi_sdf_mlp_fwd", "oi_occlusion_step" if anyhit else "oi_trace_step", st.counts
        mlp_args, at = mlp_args + [None, None, None, None, 1, bound, field.prec, field.fast, stream], 10
    mlp, step = getattr(L, mlp_name), getattr(L, step_name)
    total = k = since = 0
    while k < max_steps and bound > 0:
        mlp_args[at] = bound
        rc = mlp(*mlp_args)
        if rc:
            _l.check(rc, mlp_name)
        rc = step(state_p, sdf_p, bound, k, tol, omega, stream)
        if rc:
            _l.check(rc, step_name)
        total += bound
        k += 1
        since += 1
        every = (1 if bound > READBACK_DENSE else READBACK_SPARSE) if readback == "auto" else int(readback)
        if since >= every and k < max_steps:
            bound, since = int(counter[k].item()), 0
    return total, k


def _finish(st, n_evals, n_steps):
    hit_index, hit_points, hit_slot = ops.trace_finish(st)
    n_hit = int(st.counts[-1].item())
    return TraceResult(st.t, st.status, st.steps, hit_index[:n_hit], n_evals, n_steps, hit_points[:n_hit], hit_slot)


@torch.no_grad()
def sphere_trace(pack_or_generator, rays_o, rays_d, near=None, far=None, z=None, w=None, tol=DEFAULT_TOL, omega=DEFAULT_OMEGA,
                 max_steps=DEFAULT_MAX_STEPS, siren_network=None, readback="auto"):
    """Rays (N, 3) + (N, 3) (CUDA, any leading shape) against the SDF of one latent z (1, 64) or style vector w (1, 64) of a
    FieldPack, a NeuSRenderer or a Generator, in the pack's precision.  near / far (N,): default near_far_from_sphere (the
    unit sphere's mid-point -1 / +1).  Per ray: march t += max(omega sdf, tol) from near; |sdf| <= tol is a hit; the first
    negative sample closes a bracket that Illinois regula falsi refines until |sdf| <= tol (include/oi_trace.h has the state
    machine).  readback: 'auto' or the number of steps between reads of the number of rays in flight.  -> TraceResult."""
    if siren_network is not None:
        raise NotImplementedError("siren_network is not on the path (as in render())")
    _check_params(tol, omega, max_steps, readback, "sphere_trace")
    field = LatentField(pack_or_generator, z, w, "sphere_trace")
    if not torch.is_tensor(rays_o) or not torch.is_tensor(rays_d) or rays_o.shape != rays_d.shape or rays_o.shape[-1] != 3:
        raise ValueError("sphere_trace: rays_o and rays_d must be tensors of the same (..., 3) shape")
    if not rays_o.is_cuda:
        raise _l.OiHipError("sphere_trace: the rays must be on the GPU (there is no CPU path)")
    ro, rd = rays_o.detach().float().reshape(-1, 3).contiguous(), rays_d.detach().float().reshape(-1, 3).contiguous()
    N, dev = ro.shape[0], ro.device
    if N >= 1 << 31:
        raise ValueError(f"sphere_trace: {N} rays (at most 2^31 - 1)")
    if N == 0:   # nothing is launched
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
        return TraceResult(e(0), e(0, dt=torch.uint8), e(0, dt=torch.int16), e(0, dt=torch.int32), 0, 0, e(0, 3), e(0, dt=torch.int32))
    if near is None or far is None:
        mid = -(ro * rd).sum(-1) / (rd * rd).sum(-1)   # generator.py:336-342
        near = mid - 1.0 if near is None else near
        far = mid + 1.0 if far is None else far
    near, far = (torch.as_tensor(v, dtype=torch.float32, device=dev).reshape(-1).expand(N) for v in (near, far))
    field.prepare(z, w)
    st = ops.TraceState(N, ro, rd, near, far)
    ops.trace_begin(st)
    n_evals, k = _march(field, st, N, float(tol), float(omega), int(max_steps), readback)
    return _finish(st, n_evals, k)


class TraceResults(list):
    """E TraceResults, views of the batched arrays of one sphere_trace_batch.  n_evals: points sent through the sdf-only MLP
    pass by the whole batch, E * sum_k bound_k (each element carries its share, sum_k bound_k); n_steps: loop iterations run;
    n_pad: the largest hit count; hit_points_padded (E, n_pad, 3): row e holds hit_points of element e, then the coordinate
    origin; n_hit: the hit counts; counts (E, TRACE_COUNT_WORDS) / live (TRACE_COUNT_WORDS,) int32: the device's counters
    (counts[e][k]: rays of element e in flight before step k; live[k] their maximum)."""
    n_evals = n_steps = n_pad = 0
    hit_points_padded = counts = live = None
    hit_index = hit_slot = None   # (E, N) int32, oi_trace_batch_finish's arrays: what the batched secondary rays read
    n_hit = ()


def _march_batch(field, st, tol, omega, max_steps, readback, bound=None, anyhit=False):
    """_march on an ops.TraceBatchState.  bound: live[0] where a begin kernel enters only some of the rays (oi_amd.scene),
    else N.  anyhit: the sampled secondary rays of a scene, which end at their first occluder (oi_trace_batch_step_anyhit)."""
    return _march(field, st, st.N if bound is None else int(bound), tol, omega, max_steps, readback, anyhit=anyhit)


@torch.no_grad()
def sphere_trace_batch(pack_or_generator, rays_o, rays_d, near=None, far=None, z=None, w=None, tol=DEFAULT_TOL,
                       omega=DEFAULT_OMEGA, max_steps=DEFAULT_MAX_STEPS, readback="auto"):
    """sphere_trace for E latents at once: rays (E, N, 3) + (E, N, 3) (CUDA), z or w (E, 64), near / far (E, N) (default: as
    sphere_trace).  ONE chain of steps marches all E * N rays: per step one sdf-only MLP pass over the first live[k] compacted
    points of every element and one oi_trace_batch_step, where live[k] is the largest number of rays any element still has
    in flight; the host reads that one word by sphere_trace's rule (every step while live[k] > READBACK_DENSE).  Per ray
    the result is sphere_trace's on that element alone, bit for bit.  -> TraceResults: E TraceResult objects that are views of
    the batched arrays, and the batch's n_evals = E * sum_k bound_k.  E * N == 0 launches nothing."""
    _check_params(tol, omega, max_steps, readback, "sphere_trace_batch")
    field = LatentField(pack_or_generator, z, w, "sphere_trace_batch", batch_ok=True)
    if (not torch.is_tensor(rays_o) or not torch.is_tensor(rays_d) or rays_o.shape != rays_d.shape or rays_o.dim() != 3
            or rays_o.shape[-1] != 3):
        raise ValueError("sphere_trace_batch: rays_o and rays_d must be tensors of the same (E, N, 3) shape")
    lat = w if w is not None else z
    E, N, dev = rays_o.shape[0], rays_o.shape[1], rays_o.device
    if lat.dim() != 2 or lat.shape[0] != E:
        raise ValueError(f"sphere_trace_batch: latents {tuple(lat.shape)} for {E} elements (one row per element)")
    if E > _l.TRACE_BATCH_MAX_ELEMS or E * N >= 1 << 31:
        raise ValueError(f"sphere_trace_batch: {E} elements x {N} rays (at most {_l.TRACE_BATCH_MAX_ELEMS} elements, E * N < 2^31)")
    if not rays_o.is_cuda:
        raise _l.OiHipError("sphere_trace_batch: the rays must be on the GPU (there is no CPU path)")
    out = TraceResults()
    if E * N == 0:   # nothing is launched
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
        out.extend(TraceResult(e(N), e(N, dt=torch.uint8), e(N, dt=torch.int16), e(0, dt=torch.int32), 0, 0, e(0, 3),
                               e(N, dt=torch.int32)) for _ in range(E))
        out.hit_points_padded, out.n_hit = e(E, 0, 3), (0,) * E
        return out
    ro, rd = rays_o.detach().float().contiguous(), rays_d.detach().float().contiguous()
    if near is None or far is None:
        mid = -(ro * rd).sum(-1) / (rd * rd).sum(-1)   # generator.py:336-342
        near = mid - 1.0 if near is None else near
        far = mid + 1.0 if far is None else far
    near, far = (torch.as_tensor(v, dtype=torch.float32, device=dev).expand(E, N) for v in (near, far))
    field.prepare(z, w)
    return _trace_batch(field, ops.TraceBatchState(E, N, ro, rd, near, far), float(tol), float(omega), int(max_steps), readback)


def _trace_batch(field, st, tol, omega, max_steps, readback):
    ops.trace_batch_begin(st)
    total, k = _march_batch(field, st, tol, omega, max_steps, readback)
    hit_index, hit_slot = ops.trace_batch_finish(st)
    n_pad = int(st.live[-1].item())                        # the one word the host waits for
    padded = ops.trace_batch_gather(st, hit_index, n_pad)
    n_hit = st.counts[:, -1].tolist()                      # slicing the views below needs every element's count
    out = TraceResults(TraceResult(st.t[e], st.status[e], st.steps[e], hit_index[e, :n_hit[e]], total, k, padded[e, :n_hit[e]],
                                   hit_slot[e]) for e in range(st.E))
    out.n_evals, out.n_steps, out.n_pad, out.hit_points_padded, out.n_hit = st.E * total, k, n_pad, padded, tuple(n_hit)
    out.counts, out.live, out.hit_index, out.hit_slot = st.counts, st.live, hit_index, hit_slot
    return out


def _view_rays_camera(gen, b2w):
    """_view_rays and the view's camera, what oi_gen_rays was given: -> rays_o, rays_d (N, 3), near, far (N,), w2b (4, 4), c2b
    (4, 4), kinv (3, 3), offs (2,).  The sub-pixel rays of the anti-aliasing stage are generated from the last three."""
    dev = gen.it.device
    prior = gen.sample_prior(1, {"b2w": b2w.to(dev, torch.float32).reshape(1, 4, 4)})
    rays = gen.gen_rays_at({}, prior)
    offs = torch.stack([rays["x_offset"][0], rays["y_offset"][0]]).float().contiguous()
    return (rays["rays_o"].reshape(-1, 3), rays["rays_d"].reshape(-1, 3), rays["near"].reshape(-1), rays["far"].reshape(-1),
            prior["w2b"][0].contiguous(), prior["c2b"][0].float().contiguous(), gen._kinv(dev), offs)


def _view_rays(gen, b2w):
    """The rays of Generator.forward for one pose (4, 4): its own oi_gen_rays path.  -> rays_o, rays_d (N, 3), near, far (N,),
    w2b (4, 4)."""
    return _view_rays_camera(gen, b2w)[:5]


# ---------------------------------------------------------------------------------------------------------------------
# anti-aliasing (include/oi_aa.h)
# ---------------------------------------------------------------------------------------------------------------------
AA_R2 = (0.7548776662466927, 0.5698402909980532)   # 1 / g and 1 / g^2 of the plastic number g: the R2 low-discrepancy sequence


def aa_pattern_r2(S):
    """The default sub-pixel pattern: offsets[j] = frac(0.5 + j AA_R2) - 0.5 in float64, rounded to float32.  -> (S, 2) numpy
    float32 in units of the pixel pitch; row 0 (the pixel centre) is (0, 0), every row lies in [-0.5, 0.5)."""
    v = 0.5 + np.arange(int(S), dtype=np.float64)[:, None] * np.asarray(AA_R2, dtype=np.float64)[None]
    return (v - np.floor(v) - 0.5).astype(np.float32)


@dataclasses.dataclass
class _AA:
    """Checked anti-aliasing parameters: S samples per flagged pixel (the centre included), offsets (S, 2) numpy float32."""
    S: int
    adaptive: bool
    plane: float
    cos: float
    offsets: np.ndarray


def _check_aa(aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, what):
    """-> None for aa_samples == 1 (no anti-aliasing stage), else the _AA.  Everything is checked either way."""
    if not _is_count(aa_samples, 1, _l.AA_MAX_SAMPLES):
        raise ValueError(f"{what}: aa_samples={aa_samples!r} (an integer, 1 <= aa_samples <= {_l.AA_MAX_SAMPLES})")
    if not isinstance(aa_adaptive, (bool, np.bool_)):
        raise ValueError(f"{what}: aa_adaptive={aa_adaptive!r} (True or False)")
    for name, v in (("aa_plane", aa_plane), ("aa_cos", aa_cos)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= float(v) < 1:   # (NaN fails the comparison)
            raise ValueError(f"{what}: {name}={v!r} (a number, 0 <= {name} < 1)")
    S = int(aa_samples)
    if aa_pattern is None:
        offsets = aa_pattern_r2(S)
    else:
        try:
            pat = np.asarray(aa_pattern.detach().cpu() if torch.is_tensor(aa_pattern) else aa_pattern, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: aa_pattern must be an array of shape ({S}, 2)") from None
        if pat.shape != (S, 2):
            raise ValueError(f"{what}: aa_pattern of shape {pat.shape} (one row per sample: ({S}, 2))")
        if not (np.isfinite(pat).all() and (np.abs(pat) <= 0.5).all() and (pat[0] == 0).all()):
            raise ValueError(f"{what}: aa_pattern (row 0, the pixel centre, must be (0, 0); every row within [-0.5, 0.5] pixel pitches)")
        offsets = pat.astype(np.float32)
    return None if S == 1 else _AA(S, bool(aa_adaptive), float(aa_plane), float(aa_cos), offsets)


def _ascending(index, n, slot):
    """The compaction's order differs from run to run, and a compacted pixel's position keys its shadow and occlusion samples:
    ascending order makes the frame a function of its arguments alone.  -> index[:n] sorted; slot[index[k]] = k is written."""
    order = torch.sort(index[:n]).values
    slot[order.long()] = torch.arange(n, dtype=torch.int32, device=slot.device)
    return order


def _flagged(aa, n_pixels, dev, classify):
    """The pixels that get sub-samples: -> (edge_index, edge_slot, n_edge).  Adaptive: classify() -> (edge_index, edge_slot,
    count) and ONE read-back of the count, the flagged pixels in ascending order; otherwise every pixel."""
    if not aa.adaptive:
        every = torch.arange(n_pixels, dtype=torch.int32, device=dev)
        return every, every, n_pixels
    edge_index, edge_slot, count = classify()
    n_edge = int(count.item())
    if n_edge:
        edge_index[:n_edge] = _ascending(edge_index, n_edge, edge_slot)
    return edge_index, edge_slot, n_edge


class _Stages:
    """What the light-dependent stages (_lit_stages, oi_amd.inference's light walks) read of a traced surface, the same for a
    view (_Surface) and a scene (oi_amd.scene.SceneSurface): n_pixels, the pixels its maps cover, side x side; n_points, its
    visible points; device; OUTPUTS, _shade's default; visibility / local_visibility / ambient, whose `limit` caps the rays
    of one trace; _shade(lights, bg, visibility, outputs, image_out, ao); with an anti-aliasing stage aa,
    sub (the sub-samples, one more surface of the same kind, or None), edge_slot, n_edge and AA_RESOLVE, the resolve entry
    that reads sub's planes.  A scene's ground (oi_amd.scene.GroundSurface) has the visibility half."""

    def light_visibility(self, lt, radii, samples, seed, limit=None, **ground):
        """The visibility of the stacked lights lt, (L, pixels): local lights (their own size; a ground plane does not block
        their rays), else caps of the angular radii `radii` (L,), None for the hard shadow ray."""
        if _is_local(lt):
            return self.local_visibility(lt, samples, seed, limit)
        return self.visibility(lt, radii, samples, seed, limit, **ground)

    def resolve(self, lt, bgv, centre, vis_sub, ao_sub, image_out=None, want_mask=False):
        """The anti-aliased image of a surface with an anti-aliasing stage: the sub-sample surface shaded as the centres were
        (under lt, with its own visibility and occlusion; off-surface samples carry bg) and the mean over each flagged pixel's
        samples, centre["image"] (L, 3, pixels) elsewhere (AA_RESOLVE; without a sub-sample surface a copy).  -> image (L, 3,
        pixels) (written into image_out when given), coverage (pixels,) or None (want_mask: the same mean over centre["mask"])."""
        L, M, sub = lt.shape[0], self.n_pixels, None
        if self.sub is not None:
            sub = self.sub._shade(lt, bgv, vis_sub, ("mask", "image") if want_mask else ("image",), ao=ao_sub)
        mean = lambda k, P, out=None: getattr(ops, self.AA_RESOLVE)(centre[k].view(P, M), None if sub is None else sub[k].view(P, -1),
                                                                   self.edge_slot, self.n_edge, self.aa.S, out=out)
        image = mean("image", 3 * L, None if image_out is None else image_out.view(3 * L, M)).view(L, 3, M)
        return image, mean("mask", 1).view(M) if want_mask else None


class _Surface(_Stages):
    """One traced view and everything the light-dependent stages reuse: the primary trace, the full MLP pass at its hits."""
    OUTPUTS, AA_RESOLVE = tuple(ops.SURFACE_OUT) + ("image",), "aa_resolve"
    n_pixels, side, n_points = property(lambda self: self.N), property(lambda self: self.H), property(lambda self: self.n_hit)
    device = property(lambda self: self.ro.device)

    @staticmethod
    def params(bias, trace_kw, what="render_surface"):
        """The checked trace parameters (tol, omega, max_steps, readback) and the bias."""
        tol, omega = trace_kw.get("tol", DEFAULT_TOL), trace_kw.get("omega", DEFAULT_OMEGA)
        max_steps, readback = trace_kw.get("max_steps", DEFAULT_MAX_STEPS), trace_kw.get("readback", "auto")
        unknown = set(trace_kw) - {"tol", "omega", "max_steps", "readback"}
        if unknown:
            raise TypeError(f"{what}: unknown arguments {sorted(unknown)}")
        _check_params(tol, omega, max_steps, readback, what)
        if not (float(bias) >= 0 and np.isfinite(float(bias))):
            raise ValueError(f"{what}: bias={bias!r} (>= 0 and finite)")
        return (float(tol), float(omega), int(max_steps), readback), float(bias)

    def __init__(self, gen, z, b2w, bias, trace_kw, w=None, aa=None):
        kw, bias = self.params(bias, trace_kw)
        field = LatentField(gen, z, w, "render_surface")
        gen.eval()
        dev = gen.it.device
        field.prepare(None if z is None else z.to(dev), None if w is None else w.to(dev))
        ro, rd, near, far, w2b, *camera = _view_rays_camera(gen, b2w)
        st = ops.TraceState(ro.shape[0], ro, rd, near, far)
        ops.trace_begin(st)
        res = _finish(st, *_march(field, st, st.N, *kw))
        grad = rgb = None
        if res.hit_index.shape[0]:
            _, grad, rgb = field.full(res.hit_points)
        self._set(field, kw, bias, ro, rd, w2b, gen.resolution, res, grad, rgb)
        if aa is not None:
            self._antialias(aa, *camera)

    def _set(self, field, kw, bias, ro, rd, w2b, H, res, grad, rgb):
        self.kw, self.bias, self.field = kw, bias, field
        self.ro, self.rd, self.w2b, self.N, self.H = ro, rd, w2b, ro.shape[0], H
        self.res, self.n_hit, self.grad, self.rgb = res, res.hit_index.shape[0], grad, rgb
        self.shadow_evals = self.ao_evals = self.transfer_evals = self.glossy_evals = self.bounce_points = 0
        self.shadow = self.ao = self.transfer_state = self.glossy_state = self.bounce_hits = None
        self.aa = self.sub = self.edge_slot = None   # the anti-aliasing stage (_antialias), when there is one
        self.n_edge = 0

    @classmethod
    def from_batch(cls, field, kw, bias, ro, rd, w2b, H, res, grad, rgb):
        """One element of render_surfaces: slices of the batched arrays, its own w2b and FiLM rows (field: B = 1)."""
        self = cls.__new__(cls)
        self._set(field, kw, bias, ro, rd, w2b, H, res, grad, rgb)
        return self

    def _antialias(self, aa, c2b, kinv, offs):
        """The anti-aliasing stage (include/oi_aa.h): the flagged pixels (adaptive: oi_aa_classify and one read-back of their
        number; otherwise every pixel), their aa.S - 1 sub-pixel rays each, the march on those rays (closest hit) and one full
        MLP pass at their hits.  self.sub: the sub-sample rays as one more _Surface (ray (j - 1) * n_edge + e: sample j of
        flagged pixel e), which the light-dependent stages treat as they treat this one; None without a flagged pixel."""
        r, H = self.res, self.H
        edge_index, edge_slot, n_edge = _flagged(aa, self.N, self.ro.device, lambda: ops.aa_classify(
            r.status, r.hit_slot, r.hit_points, self.grad, self.n_hit, H, H, aa.plane, aa.cos))
        self.aa, self.edge_slot, self.n_edge = aa, edge_slot, n_edge
        if n_edge == 0:
            return
        st = ops.TraceState((aa.S - 1) * n_edge, ref=self.ro)
        ops.aa_begin(st, c2b, kinv, offs, H, edge_index, n_edge, torch.from_numpy(aa.offsets).to(self.ro.device))
        res = _finish(st, *_march(self.field, st, st.N, *self.kw))
        grad = rgb = None
        if res.hit_index.shape[0]:
            _, grad, rgb = self.field.full(res.hit_points)
        self.sub = _Surface.from_batch(self.field, self.kw, self.bias, st.rays_o, st.rays_d, self.w2b, H, res, grad, rgb)

    def _secondary(self, st, anyhit=True):
        """The loop on a state of secondary rays that a begin entry has filled (any-hit after an oi_occlusion_*_begin); rays in
        flight at the end -> LIMIT."""
        n_evals, _ = _march(self.field, st, int(st.counts[0].item()), *self.kw, anyhit=anyhit)
        ops.trace_finish(st)
        return n_evals

    def visibility(self, lights, radius=None, samples=1, seed=0, limit=None):
        """(L, N) visibility of `lights` (L, 16) (limit: not read; a view's walks size their chunks of lights instead).  radius None and one sample: one shadow trace over all L x n_hit rays (0 or
        1 per pixel).  Otherwise radius (L,) holds the lights' angular radii and one any-hit trace runs over all
        L x samples x n_hit rays: the share of a pixel's samples that reach the light."""
        L = lights.shape[0]
        if self.n_hit == 0:
            return torch.ones(L, self.N, device=self.ro.device)
        if radius is None and samples == 1:
            st = ops.TraceState(L * self.n_hit, ref=self.ro)
            ops.trace_shadow_begin(st, self.res.hit_points, self.grad, self.n_hit, lights, self.w2b, self.bias)
            self.shadow_evals += self._secondary(st, anyhit=False)
            self.shadow = st
            return ops.trace_visibility(st.status, self.res.hit_slot, self.N, self.n_hit, L)
        if radius is None:
            radius = torch.zeros(L, device=self.ro.device)
        st = ops.TraceState(L * samples * self.n_hit, ref=self.ro)
        ops.occlusion_light_begin(st, self.res.hit_points, self.grad, self.res.hit_index, self.n_hit, lights, radius, samples,
                                  self.w2b, self.bias, seed)
        self.shadow_evals += self._secondary(st)
        self.shadow = st
        return ops.occlusion_resolve(st.status, self.res.hit_slot, self.N, self.n_hit, L, samples)

    def local_visibility(self, lights, samples=1, seed=0, limit=None):
        """(L, N) visibility of the local lights `lights` (L, 20) (include/oi_local_light.h): one any-hit trace over all
        L x samples x n_hit rays, each aimed at its light's sphere and ending there; the share of a pixel's samples that
        reach the light (0 or 1 for a point light with one sample)."""
        L = lights.shape[0]
        if self.n_hit == 0:
            return torch.ones(L, self.N, device=self.ro.device)
        st = ops.TraceState(L * samples * self.n_hit, ref=self.ro)
        ops.local_light_begin(st, self.res.hit_points, self.grad, self.res.hit_index, self.n_hit, lights, samples, self.w2b,
                              self.bias, seed)
        self.shadow_evals += self._secondary(st)
        self.shadow = st
        return ops.occlusion_resolve(st.status, self.res.hit_slot, self.N, self.n_hit, L, samples)

    def ambient(self, samples, distance, seed=0, limit=None):
        """(N,) ambient occlusion: the share of `samples` cosine-weighted hemisphere rays per visible point that leave the
        point's neighbourhood (`distance`) without meeting the surface; 1 off the mask."""
        if self.n_hit == 0:
            return torch.ones(self.N, device=self.ro.device)
        st = ops.TraceState(samples * self.n_hit, ref=self.ro)
        ops.occlusion_ambient_begin(st, self.res.hit_points, self.grad, self.res.hit_index, self.n_hit, samples, self.bias,
                                    distance, seed)
        self.ao_evals += self._secondary(st)
        self.ao = st
        return ops.occlusion_resolve(st.status, self.res.hit_slot, self.N, self.n_hit, 1, samples).view(self.N)

    def transfer(self, samples, seed=0):
        """(9, N) SH transfer map (include/oi_envlight.h): ambient()'s rays as far as the exit of the unit sphere, resolved
        into the mean of [escaped] y_c(world direction) per pixel; samples == 0: the unshadowed closed form, nothing traced."""
        if self.n_hit == 0:
            return torch.zeros(_l.ENV_COEFFS, self.N, device=self.ro.device)
        if samples == 0:
            return ops.transfer_normal(self.grad, self.res.hit_slot, self.N, self.n_hit, self.w2b)
        st = ops.TraceState(samples * self.n_hit, ref=self.ro)
        ops.occlusion_ambient_begin(st, self.res.hit_points, self.grad, self.res.hit_index, self.n_hit, samples, self.bias,
                                    TRANSFER_DISTANCE, seed)
        self.transfer_evals += self._secondary(st)
        self.transfer_state = st
        return ops.transfer_resolve(st.status, st.rays_d, self.res.hit_slot, self.N, self.n_hit, samples, self.w2b)

    def transfer_bounce(self, samples, seed=0):
        """transfer()'s (9, N) map and the bounce transfer (3, 9, N) of the same rays (include/oi_envbounce.h).  The rays are
        transfer()'s, marched with the closest-hit step (oi_trace_step): the ones that end MISS are the same, the others are
        refined to their nearest intersection; one full MLP pass there gives the normals and the albedo that
        oi_bounce_resolve folds into a per-channel transfer.  samples >= 1."""
        dev = self.ro.device
        if self.n_hit == 0:
            return torch.zeros(_l.ENV_COEFFS, self.N, device=dev), torch.zeros(3, _l.ENV_COEFFS, self.N, device=dev)
        st = ops.TraceState(samples * self.n_hit, ref=self.ro)
        ops.occlusion_ambient_begin(st, self.res.hit_points, self.grad, self.res.hit_index, self.n_hit, samples, self.bias,
                                    TRANSFER_DISTANCE, seed)
        n_evals, _ = _march(self.field, st, int(st.counts[0].item()), *self.kw, anyhit=False)
        hit_index2, hit_points2, hit_slot2 = ops.trace_finish(st)     # rays in flight at the end -> LIMIT
        n_hit2 = int(st.counts[-1].item())
        grad2 = rgb2 = None
        if n_hit2:
            _, grad2, rgb2 = self.field.full(hit_points2[:n_hit2])
        self.transfer_evals += n_evals
        self.bounce_points += n_hit2
        self.transfer_state = st
        # what oi_bounce_resolve read: the secondary hits of the state (ray q = j * n_hit + i)
        self.bounce_hits = dict(hit_index=hit_index2[:n_hit2], hit_points=hit_points2[:n_hit2], hit_slot=hit_slot2, grad=grad2,
                                rgb=rgb2, n_hit=n_hit2)
        direct = ops.transfer_resolve(st.status, st.rays_d, self.res.hit_slot, self.N, self.n_hit, samples, self.w2b)
        bounce = ops.bounce_resolve(st.status, st.rays_d, hit_slot2, grad2, rgb2, n_hit2, self.res.hit_slot, self.N, self.n_hit,
                                    samples, self.w2b)
        return direct, bounce

    def lobe_visibility(self, samples, shininess, seed=0):
        """(N,) reflection-lobe visibility V_spec (include/oi_envgloss.h): the share of `samples` rays per visible point,
        distributed as cos^shininess about the reflected view vector, that are above the point's horizon and leave the scene;
        1 off the mask."""
        if self.n_hit == 0:
            return torch.ones(self.N, device=self.ro.device)
        st = ops.TraceState(samples * self.n_hit, ref=self.ro)
        ops.occlusion_lobe_begin(st, self.ro, self.res.hit_points, self.grad, self.res.hit_index, self.n_hit, samples, shininess,
                                 self.bias, seed)
        self.glossy_evals += self._secondary(st)
        self.glossy_state = st
        return ops.occlusion_resolve(st.status, self.res.hit_slot, self.N, self.n_hit, 1, samples).view(self.N)

    def _shade(self, lights, bg, visibility=None, outputs=OUTPUTS, image_out=None, ao=None):
        r = self.res
        dummy = self.ro   # never read when n_hit == 0
        args = (self.ro, self.rd, r.t, r.status, r.hit_slot, r.hit_points if self.n_hit else dummy,
                self.grad if self.n_hit else dummy, self.rgb if self.n_hit else dummy, self.n_hit, self.w2b, lights, bg, visibility)
        if lights is not None and _is_local(lights):   # local lights: their own kernel
            return ops.surface_shade_local(*args, ao, outputs, image_out)
        if ao is None:
            return ops.surface_shade(*args, outputs, image_out)
        return ops.surface_shade_ao(*args, ao, outputs, image_out)

    def shade(self, lights, bg, visibility=None, outputs=OUTPUTS, image_out=None, ambient_occlusion=None):
        """_shade under the name and keywords a view's callers know (a scene's `shade` is its public entry)."""
        return self._shade(lights, bg, visibility, outputs, image_out, ambient_occlusion)

    def stats(self):
        s = self.res.counts()
        s.update(n_rays=self.N, n_evals=self.res.n_evals, n_steps=self.res.n_steps, shadow_evals=self.shadow_evals,
                 ao_evals=self.ao_evals)
        if self.aa is not None:   # aa_evals: every sdf evaluation the sub-samples cost (their march, shadow and occlusion rays)
            sub = self.sub
            s.update(aa_pixels=self.n_edge, aa_rays=(self.aa.S - 1) * self.n_edge,
                     aa_evals=0 if sub is None else sub.res.n_evals + sub.shadow_evals + sub.ao_evals)
        return s


def _is_count(v, lo, hi=_l.OCCLUSION_MAX_SAMPLES):
    """An integer (no bool) with lo <= v <= hi: a number of samples, instances or lights."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and lo <= int(v) <= hi


def _check_seed(seed, what):
    if not _is_count(seed, 0, (1 << 32) - 1):
        raise ValueError(f"{what}: seed={seed!r} (an integer, 0 <= seed < 2^32)")


def _check_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, n_lights, what, local=False):
    """-> the lights' angular radii as a list of n_lights floats, or None for hard shadows (one ray, no radius).  local: the
    lights are LocalLights, whose size is their own radius: a light_radius other than 0 is refused, and None is returned."""
    if not _is_count(shadow_samples, 1):
        raise ValueError(f"{what}: shadow_samples={shadow_samples!r} (an integer, 1 <= shadow_samples <= {_l.OCCLUSION_MAX_SAMPLES})")
    if not _is_count(ao_samples, 0):
        raise ValueError(f"{what}: ao_samples={ao_samples!r} (an integer, 0 <= ao_samples <= {_l.OCCLUSION_MAX_SAMPLES})")
    if not (float(ao_distance) > 0 and np.isfinite(float(ao_distance))):
        raise ValueError(f"{what}: ao_distance={ao_distance!r} (positive and finite)")
    _check_seed(seed, what)
    rad = np.asarray(light_radius.detach().cpu() if torch.is_tensor(light_radius) else light_radius, dtype=np.float64)
    if rad.ndim > 1 or (rad.ndim == 1 and rad.shape[0] != n_lights):
        raise ValueError(f"{what}: light_radius of shape {rad.shape} (a scalar or one value per light: {n_lights})")
    if not (np.isfinite(rad).all() and (rad >= 0).all() and (rad <= np.pi / 2).all()):
        raise ValueError(f"{what}: light_radius={light_radius!r} (radians, 0 <= light_radius <= pi / 2)")
    soft = int(shadow_samples) != 1 or bool((rad != 0).any())
    if local and bool((rad != 0).any()):
        raise ValueError(f"{what}: light_radius={light_radius!r} with local lights (the size is the light's own: LocalLight.radius)")
    if soft and not shadows:
        raise ValueError(f"{what}: shadow_samples / light_radius need shadows=True")
    if local:
        return None
    return np.broadcast_to(rad, (n_lights,)).tolist() if soft else None


def _checked_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, lt, what):
    """_check_occlusion for the stacked lights lt, and the checked values coerced ONCE for everything below: -> the occlusion
    tuple (radii (L,) float32 on the lights' device or None, shadows, shadow_samples, ao_samples, ao_distance, seed)."""
    radii = _check_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, lt.shape[0], what, _is_local(lt))
    if radii is not None:
        radii = torch.tensor(radii, dtype=torch.float32, device=lt.device)
    return radii, bool(shadows), int(shadow_samples), int(ao_samples), float(ao_distance), int(seed)


def _bg(bg, dev):
    return None if bg is None else torch.as_tensor(bg, dtype=torch.float32).to(dev).reshape(3).contiguous()


def _is_local(lt):
    """Does the stacked light array hold local records (include/oi_local_light.h)?"""
    return lt.shape[-1] == _l.LOCAL_LIGHT_FLOATS


def _stack_lights(gen, lights, dev, what, hint=""):
    """`lights` (oi_amd.relight.Light objects; default the generator's trained light) as (L, 16) on dev, or LocalLight
    objects as (L, 20); a list that mixes the two is refused.  More than RELIGHT_MAX_LIGHTS are refused in the name of `what`;
    hint: where larger sets are split."""
    from .relight import Light, local_lights_given, stack_lights, stack_local_lights
    if local_lights_given(lights):
        lt = stack_local_lights(lights, dev)
    else:
        lt = stack_lights(Light.from_module(gen.light) if lights is None else lights, dev)
    if lt.shape[0] > _l.RELIGHT_MAX_LIGHTS:
        raise ValueError(f"{what}: {lt.shape[0]} lights (at most {_l.RELIGHT_MAX_LIGHTS}{hint})")
    return lt


def _latents(zs, dev):
    """E latents, a tensor (E, z_dim) or a sequence of (z_dim,) or (1, z_dim) -> (E, z_dim) float32 on dev."""
    zs = (zs if torch.is_tensor(zs) else torch.stack([z.reshape(-1) for z in zs])).to(dev).float()
    return zs.reshape(-1, zs.shape[-1])


def _maps(out, H, W):
    """(N,) / (N, 3) G-buffer arrays -> (1, C, H, W) maps."""
    return {k: (v.view(1, H, W, -1).permute(0, 3, 1, 2) if v.dim() == 2 else v.view(1, 1, H, W)) for k, v in out.items()}


_MAP_NAMES = {"depth": "depth", "position": "position", "normal_world": "normal_map", "normal": "normal_object",
              "albedo": "albedo", "mask": "mask", "instance": "instance"}   # (instance: a scene's)


@torch.no_grad()
def render_surface(gen, z, b2w, lights=None, shadows=False, bg=None, bias=DEFAULT_BIAS, shadow_samples=1, light_radius=0.0,
                   ao_samples=0, ao_distance=0.5, seed=0, aa_samples=1, aa_adaptive=True, aa_plane=_l.AA_DEFAULT_PLANE,
                   aa_cos=_l.AA_DEFAULT_COS, aa_pattern=None, **trace_kw):
    """One view of `gen` (latent z (z_dim,) or (1, z_dim), pose b2w (4, 4)) by intersecting each pixel's ray with the surface:
    -> dict of depth (1, 1, H, W) (the ray parameter; NaN off the mask), position, normal_map (world frame), normal_object,
    albedo (1, 3, H, W), mask (1, 1, H, W), image (L, 3, H, W) under `lights` (oi_amd.relight.Light objects; default the
    generator's trained light; or oi_amd.relight.LocalLight objects, lights that stand in the world: include/oi_local_light.h,
    DESIGN section 4.27 -- their shadow rays end at the light, shadow_samples sample the light's own sphere and light_radius
    must stay 0), visibility (L, 1, H, W) when `shadows` (one shadow ray per light and visible point, offset by
    `bias` along the normal), stats (rays per status, sdf evaluations), trace (the primary TraceResult).  The rays are Generator.forward's.  bg: (3,)
    background colour (black when None).  trace_kw: tol, omega, max_steps, readback of sphere_trace.
    Soft shadows: light_radius (radians; a scalar or one value per light) gives the lights an angular size and shadow_samples
    (1 .. 256) rays per light and visible point sample its cap, so `visibility` is the share in [0, 1] that reaches the light.
    Ambient occlusion: ao_samples > 0 sends that many cosine-weighted rays over each visible point's hemisphere, as far as
    ao_distance; the share that escapes multiplies the ambient term and is returned as ambient_occlusion (1, 1, H, W).  The
    samples are a function of pixel, sample number and `seed` alone.  With shadow_samples == 1, light_radius == 0 and
    ao_samples == 0 the launches are those of a call without these arguments.
    Anti-aliasing (include/oi_aa.h): aa_samples = S in 2 .. 64 takes S samples inside each FLAGGED pixel --
    the centre and S - 1 sub-pixel rays at aa_pattern (S, 2), offsets in pixel pitches within [-0.5, 0.5] whose row 0 is
    (0, 0); default aa_pattern_r2(S) -- and `image` is the mean of their shaded values, off-surface samples carrying bg.  A
    pixel is flagged when a neighbour differs in the mask, lies off its tangent plane by more than asin(aa_plane), or has a
    normal more than acos(aa_cos) away; aa_adaptive=False flags every pixel.  The sub-samples pass the same stages as the
    centres (shadows, occlusion, local lights; their sample numbers keyed by the sub-sample ray).  New keys: coverage
    (1, 1, H, W), the mean of the mask over a pixel's samples; aa_mask (1, 1, H, W), the flagged pixels; aa_trace, the
    sub-samples' TraceResult (ray (j - 1) * aa_pixels + e: sample j of the e-th flagged pixel in ascending order; None without one); stats
    gains aa_pixels, aa_rays, aa_evals.  Every other map stays the centre sample's.  With aa_samples == 1 nothing of this runs."""
    aa = _check_aa(aa_samples, aa_adaptive, aa_plane, aa_cos, aa_pattern, "render_surface")
    dev = gen.it.device
    z = z.to(dev).reshape(1, -1)
    s = _Surface(gen, z, b2w, bias, trace_kw, aa=aa)
    lt = _stack_lights(gen, lights, dev, "render_surface", "; inference.surface_light_walk splits larger sets")
    return _lit(s, lt, *_checked_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, lt, "render_surface"),
                bg, dev)


def _occlusion(s, lt, radii, shadows, shadow_samples, ao_samples, ao_distance, seed, limit=None, **ground):
    """The secondary rays of the light-dependent stages on s (a view, a scene, its sub-samples or its ground; _Stages):
    -> (visibility (L, pixels) or None without shadows, ambient occlusion (pixels,) or None without ao_samples).  ground (a
    scene's): the plane blocks the ambient and the directional rays."""
    return (s.light_visibility(lt, radii, shadow_samples, seed, limit, **ground) if shadows else None,
            s.ambient(ao_samples, ao_distance, seed, limit, **ground) if ao_samples else None)


def _lit_stages(s, lt, bgv, occlusion, limit=None, ground=None, after_shade=None):
    """The light-dependent stages of one traced surface s (a view or a scene; _Stages) under the stacked lights lt: occlusion
    (_occlusion's radii .. seed), shade, the maps under their public names, and with an anti-aliasing stage the same on the
    sub-samples and the mean over each flagged pixel's samples.  after_shade(planes): the caller's hook on the shaded planes
    before they are named (a scene's ground writes itself into them), -> its own keys of the result.  -> the dict of maps, image, coverage / aa_mask,
    visibility, ambient_occlusion that render_surface and SceneSurface.shade share."""
    shadows, ao_samples = occlusion[1], occlusion[3]
    vis, ao = _occlusion(s, lt, *occlusion, limit, **({} if ground is None else {"ground": ground}))
    out = s._shade(lt, bgv, vis, ao=ao)
    extra = {} if after_shade is None else after_shade(out)
    H = s.side
    res = {_MAP_NAMES[k]: v for k, v in _maps({k: v for k, v in out.items() if k != "image"}, H, H).items()}
    res["image"] = out["image"].view(-1, 3, H, H)
    if s.aa is not None:   # the sub-samples through the same stages, then the mean over each flagged pixel's samples
        vis_sub, ao_sub = (None, None) if s.sub is None else _occlusion(s.sub, lt, *occlusion, limit)
        image, coverage = s.resolve(lt, bgv, out, vis_sub, ao_sub, want_mask=True)
        res["image"], res["coverage"] = image.view(-1, 3, H, H), coverage.view(1, 1, H, H)
        res["aa_mask"] = (s.edge_slot >= 0).float().view(1, 1, H, H)
    if shadows:
        res["visibility"] = vis.view(-1, 1, H, H)
    if ao_samples:
        res["ambient_occlusion"] = ao.view(1, 1, H, H)
    res.update(extra)
    return res


def _lit(s, lt, radii, shadows, shadow_samples, ao_samples, ao_distance, seed, bg, dev):
    """The light-dependent stages of one traced view (a _Surface) and render_surface's dict: _lit_stages' and the view's own
    ray states and statistics."""
    if radii is not None:
        radii = torch.as_tensor(radii, dtype=torch.float32, device=dev)
    # each stage's ray state goes behind the map it made (the order of the keys is _lit_batch's):
    # shadow_trace: ops.TraceState of the L x n_hit shadow rays (ray l * n_hit + i), or None without a hit (soft shadows: L x
    # shadow_samples x n_hit, ray (l * S + j) * n_hit + i); ao_trace: of the ao_samples x n_hit rays (ray j * n_hit + i), or None
    staged = _lit_stages(s, lt, _bg(bg, dev), (radii, shadows, shadow_samples, ao_samples, ao_distance, seed))
    states = {"aa_mask": ("aa_trace", None if s.sub is None else s.sub.res), "visibility": ("shadow_trace", s.shadow),
              "ambient_occlusion": ("ao_trace", s.ao)}
    res = {}
    for k, v in staged.items():
        res[k] = v
        if k in states:
            res.update([states[k]])
    res["stats"] = s.stats()
    res["trace"] = s.res
    return res


MAX_SECONDARY_RAYS = 1 << 24   # rays of one batch of secondary rays (oi_amd.scene.MAX_SHADOW_RAYS' value), counted as E_g * L * Sc * n_pad


def _check_batch_secondary(batch_secondary, max_secondary_rays, what):
    """-> the cap on the rays of one secondary batch (default MAX_SECONDARY_RAYS).  Both keywords are checked either way."""
    if not isinstance(batch_secondary, (bool, np.bool_)):
        raise ValueError(f"{what}: batch_secondary={batch_secondary!r} (True or False)")
    if max_secondary_rays is None:
        return MAX_SECONDARY_RAYS
    if not _is_count(max_secondary_rays, 1, 1 << 62):
        raise ValueError(f"{what}: max_secondary_rays={max_secondary_rays!r} (a positive integer, or None for {MAX_SECONDARY_RAYS})")
    return int(max_secondary_rays)


def plan_secondary(E, L, S, n_pad, max_secondary_rays, what="render_surfaces"):
    """How E views' S samples per (light, hit slot) are cut into batches of at most max_secondary_rays rays (and below 2^31),
    a batch of E_g views and Sc samples counted as E_g * L * Sc * n_pad.  A pure function.  Samples are split first: while one
    sample of all views fits, every view is in one group and Sc is the largest number that fits; otherwise Sc = 1 and the
    views are split into consecutive groups of the largest size that fits, which keep the batch's n_pad.  One sample of a
    single view that does not fit is refused.  -> (groups [(e0, e1)], chunks [(j0, Sc)]); n_pad == 0: ([], [])."""
    E, L, S, n_pad = int(E), int(L), int(S), int(n_pad)
    if n_pad == 0:
        return [], []
    cap, per = min(int(max_secondary_rays), (1 << 31) - 1), L * n_pad
    words = (what, f"1 view x {L} lights x {n_pad} hit slots = L * n_pad = {per} rays per sample of one view", "max_secondary_rays", "")
    sample_chunks(1, per, max_secondary_rays, *words)   # one sample of a single view has to fit
    if E * per <= cap:
        group, chunks = E, sample_chunks(S, E * per, max_secondary_rays, *words)
    else:
        group, chunks = cap // per, [(j0, 1) for j0 in range(S)]
    return [(a, min(E, a + group)) for a in range(0, E, group)], chunks


def sample_chunks(samples, per, cap, what, rays, cap_name="max_shadow_rays", hint="; inference.scene_light_walk splits the lights"):
    """The chunk rule of every sampled secondary trace: `samples` samples of `per` rays each, cut into chunks of Sc samples, Sc
    the largest number for which Sc * per stays within `cap` and below 2^31.  A pure function.  -> [(j0, Sc)]: the chunk of
    samples j0 .. j0 + Sc - 1 (the last one may be smaller).  One sample that does not fit is refused in the name of `what`;
    rays: the sentence that says what `per` counts, cap_name and hint: how the cap is called and what else the caller may do."""
    samples = int(samples)
    chunk = min(samples, min(int(cap), (1 << 31) - 1) // per)
    if chunk < 1:
        raise ValueError(f"{what}: {rays} (at most {cap_name}={cap} and below 2^31{hint})")
    return [(j0, min(chunk, samples - j0)) for j0 in range(0, samples, chunk)]


def sampled_trace(field, kw, like, E, per, samples, chunks, begin, resolve, anyhit=True):
    """The one chunked loop of sampled secondary rays on a batch of E elements: per chunk (j0, Sc) of sample_chunks a fresh state
    of per * Sc rays per element (on like's device), begin(sb, j0, Sc), one read of the rays entered, the batched march
    (anyhit: a ray ends at its first occluder), finish (in-flight rays -> LIMIT) and resolve(sb, j0, Sc, last), which
    accumulates the chunk.  -> (sdf evaluations per element, the last chunk's state)."""
    evals, sb = 0, None
    for j0, c in chunks:
        sb = ops.trace_batch_state_empty(E, per * c, like)
        begin(sb, j0, c)
        bound = int(sb.live[0].item())
        if bound:
            evals += _march_batch(field, sb, *kw, bound=bound, anyhit=anyhit)[0]
            ops.trace_batch_finish(sb)
        resolve(sb, j0, c, j0 + c == samples)
    return evals, sb


def _secondary_batch(field, kw, bias, st, res, grad, w2b, mode, L, S, cap, seed=0, lights=None, radius=None, distance=None):
    """One kind of secondary rays for all E views of a batched primary trace (include/oi_occlusion_batch.h): per group of
    views (plan_secondary) one sampled_trace on the views' own fields.  st, res: the primary ops.TraceBatchState and its
    TraceResults; grad (E, n_pad, 3); w2b (E, 4, 4).  -> the map (E, L, N), and per view the sdf evaluations of the chains in
    its segment, sum_k bound_k."""
    import copy
    E, N, n_pad = st.E, st.N, res.n_pad
    groups, chunks = plan_secondary(E, L, S, n_pad, cap)
    count, out = ops.occlusion_batch_maps(st.t, E, L, N, n_pad)
    evals = [0] * E
    for a, b in groups:
        sub = field
        if (a, b) != (0, E):   # the group's own FiLM rows
            sub = copy.copy(field)
            sub.B, sub.gamma, sub.beta = b - a, field.gamma[a:b], field.beta[a:b]
        begin = lambda sb, j0, c: ops.occlusion_batch_begin(
            sb, mode, res.hit_points_padded[a:b], grad[a:b], res.hit_index[a:b], st.counts[a:b], n_pad, S, j0, c, bias, seed, lights,
            radius, None if distance is not None else w2b[a:b], distance)
        resolve = lambda sb, j0, c, last: ops.occlusion_batch_resolve(sb.status, res.hit_slot[a:b], st.counts[a:b], n_pad, L, S, j0, c,
                                                                      count[a:b], out[a:b], last)
        evals[a:b] = [sampled_trace(sub, kw, st.t, b - a, L * n_pad, S, chunks, begin, resolve, mode != _l.OCCLUSION_BATCH_SHADOW)[0]] * (b - a)
    return out, evals


def _lit_batch(field, kw, bias, st, res, grad, rgb, w2b, H, lt, radii, shadows, shadow_samples, ao_samples, ao_distance, seed, bg,
               cap, dev):
    """_lit for all E views of a batched primary trace with ONE chain per stage: the visibility light_visibility would choose per
    view (hard shadows, soft shadows or local lights), the ambient occlusion, and one shade launch.  -> E dicts as _lit
    returns them, shadow_trace / ao_trace None (the states are shared and chunked)."""
    E, N, n_pad, L = st.E, st.N, res.n_pad, lt.shape[0]
    S, A = shadow_samples, ao_samples
    if n_pad:   # both plans before anything is launched: a refusal leaves nothing half done
        if shadows:
            plan_secondary(E, L, S, n_pad, cap)
        if A:
            plan_secondary(E, 1, A, n_pad, cap)
    vis = ao = None
    shadow_evals, ao_evals = [0] * E, [0] * E
    if shadows and n_pad == 0:
        vis = torch.ones(E, L, N, device=dev)
    elif shadows:
        if _is_local(lt):
            mode, extra = _l.OCCLUSION_BATCH_LOCAL, {}
        elif radii is None:
            mode, extra = _l.OCCLUSION_BATCH_SHADOW, {}
        else:
            mode, extra = _l.OCCLUSION_BATCH_CAP, dict(radius=radii)
        vis, shadow_evals = _secondary_batch(field, kw, bias, st, res, grad, w2b, mode, L, S, cap, seed, lt, **extra)
    if A and n_pad == 0:
        ao = torch.ones(E, N, device=dev)
    elif A:
        ao, ao_evals = _secondary_batch(field, kw, bias, st, res, grad, w2b, _l.OCCLUSION_BATCH_HEMISPHERE, 1, A, cap, seed,
                                        distance=ao_distance)
        ao = ao.view(E, N)
    out = ops.surface_shade_batch(st.rays_o, st.rays_d, st.t, st.status, res.hit_slot, res.hit_points_padded if n_pad else None,
                                  grad, rgb, n_pad, w2b, lt, _bg(bg, dev), vis, ao)
    K = 8   # the final status codes are below it
    per_status = torch.bincount((st.status.long() + K * torch.arange(E, device=dev)[:, None]).view(-1), minlength=K * E).view(E, K).tolist()
    results = []
    for e in range(E):
        r = {_MAP_NAMES[k]: v for k, v in _maps({k: v[e] for k, v in out.items() if k != "image"}, H, H).items()}
        r["image"] = out["image"][e].view(-1, 3, H, H)
        if shadows:
            r["visibility"], r["shadow_trace"] = vis[e].view(-1, 1, H, H), None
        if A:
            r["ambient_occlusion"], r["ao_trace"] = ao[e].view(1, 1, H, H), None
        stats = {name: int(per_status[e][code]) for code, name in _l.TRACE_STATUS_NAMES.items()}
        stats.update(n_rays=N, n_evals=res[e].n_evals, n_steps=res[e].n_steps, shadow_evals=shadow_evals[e], ao_evals=ao_evals[e],
                     secondary_batched=True)
        r["stats"], r["trace"] = stats, res[e]
        results.append(r)
    return results


@torch.no_grad()
def render_surfaces(gen, zs, b2ws, lights=None, shadows=False, bg=None, bias=DEFAULT_BIAS, shadow_samples=1, light_radius=0.0,
                    ao_samples=0, ao_distance=0.5, seed=0, batch_secondary=False, max_secondary_rays=None, **trace_kw):
    """render_surface for E views at once (latents zs: E of (z_dim,) or (E, z_dim); poses b2ws: E of (4, 4)), 1 <= E <= 1024:
    ONE batched primary trace (sphere_trace_batch's chain of steps for all E * H * W rays) and ONE full MLP pass at the hits
    of all views, padded per view to the largest hit count.  Each view then is what render_surface holds -- slices of the
    batched arrays, its own w2b and FiLM rows -- and the light-dependent stages run per view, unchanged: the shading, and with
    `shadows` / `ao_samples` the single-latent shadow and occlusion traces.
    batch_secondary=True (include/oi_occlusion_batch.h) puts those stages into ONE chain each for all E
    views: the visibility (hard shadows, soft shadows or local lights, as for a single view), the ambient occlusion, and one
    shade launch; every view's rays are tested against its own field only.  The list of dicts and their keys are unchanged and
    the maps are the same, bit for bit; shadow_trace and ao_trace are None (the ray state is shared and chunked), stats gains
    secondary_batched=True, and shadow_evals / ao_evals are the sdf evaluations of the shared chains in the view's segment,
    sum_k bound_k.  A batch of secondary rays holds at most max_secondary_rays rays (default MAX_SECONDARY_RAYS), counted as
    E_g * L * Sc * n_pad: samples are split first; if one sample of all views does not fit, the views are split into consecutive
    groups that keep the batch's n_pad; a single view that does not fit is refused before anything of these stages is launched.
    No split changes a byte.  Without a hit in any view nothing of these stages is launched.
    The other arguments are render_surface's, the same for every view.  -> a list of E dicts as render_surface returns
    them; per view the maps are render_surface's own, bit for bit."""
    import copy
    dev = gen.it.device
    cap = _check_batch_secondary(batch_secondary, max_secondary_rays, "render_surfaces")
    kw, bias = _Surface.params(bias, trace_kw, "render_surfaces")
    zs = _latents(zs, dev)
    E = zs.shape[0]
    if len(b2ws) != E or not 1 <= E <= _l.TRACE_BATCH_MAX_ELEMS:
        raise ValueError(f"render_surfaces: {E} latents and {len(b2ws)} poses (one pose per latent, 1 .. {_l.TRACE_BATCH_MAX_ELEMS} views)")
    lt = _stack_lights(gen, lights, dev, "render_surfaces")
    occlusion = _checked_occlusion(shadows, shadow_samples, light_radius, ao_samples, ao_distance, seed, lt, "render_surfaces")
    field = LatentField(gen, zs, None, "render_surfaces", batch_ok=True)
    gen.eval()
    field.prepare(zs, None)
    views = [_view_rays(gen, b2w) for b2w in b2ws]
    ro, rd, near, far = (torch.stack([v[i] for v in views]) for i in range(4))
    N = ro.shape[1]
    st = ops.TraceBatchState(E, N, ro, rd, near, far)
    res = _trace_batch(field, st, *kw)
    grad = rgb = None
    if res.n_pad:   # the full pass: the library's own, B = E elements of n_pad points
        _, grad, rgb = field.full(res.hit_points_padded.view(E * res.n_pad, 3))
        grad, rgb = grad.view(E, res.n_pad, 3), rgb.view(E, res.n_pad, 3)
    if batch_secondary:
        return _lit_batch(field, kw, bias, st, res, grad, rgb, torch.stack([v[4] for v in views]).contiguous(), gen.resolution, lt,
                          *occlusion, bg, cap, dev)
    out = []
    for e in range(E):
        one = copy.copy(field)   # the element's own FiLM rows: the field of one latent
        one.B, one.gamma, one.beta = 1, field.gamma[e:e + 1], field.beta[e:e + 1]
        n = res.n_hit[e]
        s = _Surface.from_batch(one, kw, bias, st.rays_o[e], st.rays_d[e], views[e][4], gen.resolution, res[e],
                                grad[e, :n] if n else None, rgb[e, :n] if n else None)
        out.append(_lit(s, lt, *occlusion, bg, dev))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# environment lighting (include/oi_envlight.h)
# ---------------------------------------------------------------------------------------------------------------------
def _check_transfer(transfer_samples, seed, what):
    """_check_occlusion's rule for ao_samples and seed."""
    v = transfer_samples
    if not _is_count(v, 0):
        raise ValueError(f"{what}: transfer_samples={v!r} (an integer, 0 <= transfer_samples <= {_l.OCCLUSION_MAX_SAMPLES})")
    _check_seed(seed, what)
    return int(v), int(seed)


def _check_bounces(bounces, samples, glossy_samples, shininess, what):
    """bounces: the integer 0 or 1 (no bool); a bounce follows the transfer rays, and the glossy shade does not read one."""
    if not _is_count(bounces, 0, 1):
        raise ValueError(f"{what}: bounces={bounces!r} (the integer 0 or 1: one diffuse interreflection bounce at the most)")
    if bounces and samples == 0:
        raise ValueError(f"{what}: bounces=1 with transfer_samples=0 (the bounce follows the transfer rays, and there are none)")
    if bounces and (glossy_samples is not None or shininess is not None):
        raise ValueError(f"{what}: bounces=1 with glossy_samples / shininess (the glossy shade has no bounce input yet)")
    return int(bounces)


def _shade_chunks(like, names, F, N, launch):
    """-> {name: (F, 3, N) plane} for `names`, filled by launch(a, b, out) for the environments [a, b) in steps of ENV_MAX_ENVS;
    out: the planes' rows [a, b)."""
    planes = {k: ops._new(like, F, 3, N) for k in names}
    for a in range(0, F, ENV_MAX_ENVS):
        b = min(F, a + ENV_MAX_ENVS)
        launch(a, b, {k: v[a:b] for k, v in planes.items()})
    return planes


class TransferCapture:
    """One traced view and its SH transfer map: everything shade() needs, none of which depends on the light.
    surface: the _Surface (primary trace, gradients and albedo at the hits); transfer (1, 9, H, W); maps: render_surface's
    G-buffer maps (depth, position, normal_map, normal_object, albedo, mask).  A capture made with bounces=1 also holds bounce
    (1, 3, 9, H, W), the per-channel transfer of one diffuse interreflection bounce (None otherwise; include/oi_envbounce.h).
    A capture made with glossy_samples > 0 also
    holds spec_visibility (1, 1, H, W), the reflection-lobe visibility, and the shininess it was traced for."""

    def __init__(self, surface, transfer, maps, samples, glossy_samples=None, shininess=None, spec_vis=None, specular=None,
                 bounce=None):
        self.surface, self.samples, self.maps = surface, samples, maps
        self._transfer = transfer                       # (9, N), planar: what oi_env_shade reads
        self.H = self.W = surface.H
        self.transfer = transfer.view(1, _l.ENV_COEFFS, self.H, self.W)
        self._bounce = bounce                           # (3, 9, N), planar, or None: what oi_env_shade_bounce reads
        self.bounce = None if bounce is None else bounce.view(1, 3, _l.ENV_COEFFS, self.H, self.W)
        # glossy_samples: None = never mentioned (a glossy shade is refused), 0 = no lobe trace on purpose (V_spec = 1)
        self.glossy_samples, self.shininess, self.specular = glossy_samples, shininess, specular
        self._spec_vis = spec_vis                       # (N,) or None
        self.spec_visibility = None if spec_vis is None else spec_vis.view(1, 1, self.H, self.W)

    def shade(self, envs, bg=None, specular=None):
        """The view under each of `envs` (any number: launches of ENV_MAX_ENVS).
        EnvLight objects: -> {"image": (F, 3, H, W) = max(shading, 0) albedo on the mask, bg off it; "shading": (F, 3, H, W),
        not clamped}.  On a capture made with bounces=1 (oi_env_shade_bounce) shading = direct + indirect, and "indirect":
        (F, 3, H, W), the part that reached the point by way of the object itself, is returned too.
        EnvMap objects (every element; a mixed list is refused): the glossy path, image = max(shading, 0) albedo + specular
        and "specular": (F, 3, H, W) = k_s V_spec G_s(reflected view vector).  k_s = `specular`: None takes the generator's
        learned specular colour, a scalar or an RGB triple overrides it.  The maps' shininess must be the capture's.  A capture
        made with glossy_samples = 0 has V_spec = 1: the point's own horizon and every occluder are ignored."""
        from .envlight import EnvLight, EnvMap, stack_envs, stack_maps
        s = self.surface
        dev = s.ro.device
        seq = [envs] if isinstance(envs, (EnvLight, EnvMap)) else list(envs)
        glossy = any(isinstance(e, EnvMap) for e in seq)
        if glossy and not all(isinstance(e, EnvMap) for e in seq):
            raise ValueError("shade: EnvMap and EnvLight objects in one list (shade them in two calls)")
        bgv = _bg(bg, dev)
        if not glossy:
            if specular is not None:
                raise ValueError("shade: specular= needs EnvMap environments (an EnvLight has no glossy half)")
            ev = stack_envs(seq, dev)
            F, view = ev.shape[0], (s.res.status, s.res.hit_slot, s.rgb, s.n_hit, self._transfer)
            if self._bounce is None:
                names, launch = ops.ENV_SHADE_OUT, lambda a, b, out: ops.env_shade(*view, ev[a:b], bgv, out=out)
            else:
                names, launch = ops.ENV_BOUNCE_OUT, lambda a, b, out: ops.env_shade_bounce(*view, self._bounce, ev[a:b], bgv, out=out)
            out = _shade_chunks(s.ro, names, F, s.N, launch)
            return {k: v.view(F, 3, self.H, self.W) for k, v in out.items()}
        if self.glossy_samples is None:
            raise ValueError("shade: this capture has no reflection-lobe trace; capture_transfer(glossy_samples=S) traces one, "
                             "glossy_samples=0 with a shininess states that V_spec = 1 is meant")
        if any(e.shininess != self.shininess for e in seq):
            raise ValueError(f"shade: maps prefiltered for shininess {sorted({e.shininess for e in seq})}, the capture's lobe is "
                             f"{self.shininess:g}")
        ks = self.specular if specular is None else specular
        ks = torch.as_tensor(np.broadcast_to(np.asarray(ks, dtype=np.float32), (3,)).copy()).to(dev)
        F = len(seq)

        def launch(a, b, out):
            ev, maps, index, rot, _ = stack_maps(seq[a:b], dev)
            ops.env_shade_glossy(s.res.status, s.res.hit_slot, s.rgb, s.n_hit, self._transfer, ev, s.ro,
                                 s.res.hit_points if s.n_hit else None, s.grad, s.w2b, self._spec_vis, maps, index, rot, ks, bgv,
                                 out=out)
        out = _shade_chunks(s.ro, ops.ENV_GLOSSY_OUT, F, s.N, launch)
        return {k: v.view(F, 3, self.H, self.W) for k, v in out.items()}

    def stats(self):
        st = self.surface.stats()
        st["transfer_evals"] = self.surface.transfer_evals
        st["glossy_evals"] = self.surface.glossy_evals
        st["bounce_points"] = self.surface.bounce_points
        return st


def _check_glossy(gen, glossy_samples, shininess, what):
    """-> (glossy_samples or None, shininess or None, the learned specular colour or None), checked without touching `gen`
    unless a glossy capture is asked for and leaves a value to it."""
    if glossy_samples is None and shininess is None:
        return None, None, None
    if glossy_samples is None:
        raise ValueError(f"{what}: shininess={shininess!r} without glossy_samples (give glossy_samples=S for a lobe trace, or "
                         "glossy_samples=0 to state that V_spec = 1 is meant)")
    g = glossy_samples
    if not _is_count(g, 0):
        raise ValueError(f"{what}: glossy_samples={glossy_samples!r} (an integer, 0 <= glossy_samples <= {_l.OCCLUSION_MAX_SAMPLES})")
    from .relight import Light
    learned = None
    if shininess is None:
        learned = Light.from_module(gen.light)
        shininess = learned.shininess
    s = ops.check_shininess(shininess, what)
    return int(g), s, (learned or Light.from_module(gen.light)).specular


@torch.no_grad()
def capture_transfer(gen, z, b2w, transfer_samples=64, seed=0, bias=DEFAULT_BIAS, glossy_samples=None, shininess=None,
                     bounces=0, **trace_kw):
    """One view of `gen` (latent z, pose b2w: render_surface's) prepared for environment lighting: the primary trace, the full
    MLP pass at its hits, and `transfer_samples` (0 .. 256) cosine-weighted rays per visible point -- render_surface's ambient-
    occlusion rays for the same seed, followed to the exit of the unit sphere -- resolved into a 9-coefficient transfer vector
    per pixel.  transfer_samples == 0: the unshadowed closed form of the normal, nothing traced.
    Glossy environments (oi_amd.envlight.EnvMap): glossy_samples in 1 .. 256 also traces that many rays per visible point
    about the reflected view vector, distributed as cos^shininess, into spec_visibility; shininess None takes the generator's
    learned value.  glossy_samples = 0 prepares a glossy capture without that trace (V_spec = 1: no horizon, no occluder);
    it has to be given: a shininess without glossy_samples is refused.
    With both left at None the launches and outputs are those of a call without them, and the capture shades EnvLights only.
    bounces = 1 (the integer; with transfer_samples >= 1, not with the glossy keywords) follows the transfer rays to their
    nearest intersection with the object instead of to their first occluder, evaluates the normal and the albedo there in one
    more full MLP pass and folds ONE DIFFUSE interreflection bounce into a per-channel transfer, TransferCapture.bounce
    (include/oi_envbounce.h has the estimator and its approximations); the direct transfer is bit for bit that of bounces = 0,
    whose launches and outputs are those of a call without the keyword.
    trace_kw: tol, omega, max_steps, readback of sphere_trace.  -> TransferCapture."""
    samples, seed = _check_transfer(transfer_samples, seed, "capture_transfer")
    bounces = _check_bounces(bounces, samples, glossy_samples, shininess, "capture_transfer")
    g_samples, shin, spec = _check_glossy(gen, glossy_samples, shininess, "capture_transfer")
    dev = gen.it.device
    s = _Surface(gen, z.to(dev).reshape(1, -1), b2w, bias, trace_kw)
    transfer, bounce = s.transfer_bounce(samples, seed) if bounces else (s.transfer(samples, seed), None)
    g = s._shade(None, None, outputs=tuple(ops.SURFACE_OUT))
    maps = {_MAP_NAMES[k]: v for k, v in _maps(g, s.H, s.H).items()}
    vis = s.lobe_visibility(g_samples, shin, seed) if g_samples else None
    return TransferCapture(s, transfer, maps, samples, g_samples, shin, vis, spec, bounce)


@torch.no_grad()
def render_surface_env(gen, z, b2w, envs, transfer_samples=64, seed=0, bg=None, bias=DEFAULT_BIAS, glossy_samples=None,
                       shininess=None, specular=None, bounces=0, **trace_kw):
    """capture_transfer + shade: one view of `gen` under the environment lights `envs` (oi_amd.envlight.EnvLight objects, or
    EnvMap objects with glossy_samples given: capture_transfer's and shade's keywords pass through).
    -> render_surface's G-buffer keys (depth, position, normal_map, normal_object, albedo, mask), image (F, 3, H, W), shading
    (F, 3, H, W) (not clamped), transfer (1, 9, H, W), stats (with transfer_evals), trace (the primary TraceResult) and
    transfer_trace (ops.TraceState of the transfer_samples x n_hit rays, ray j * n_hit + i, or None); on the glossy path also
    specular (F, 3, H, W), spec_visibility (1, 1, H, W) or None and glossy_trace (the state of the lobe rays, or None); with
    bounces=1 also indirect (F, 3, H, W) and bounce (1, 3, 9, H, W)."""
    cap = capture_transfer(gen, z, b2w, transfer_samples, seed, bias, glossy_samples, shininess, bounces, **trace_kw)
    res = dict(cap.maps)
    res.update(cap.shade(envs, bg, specular))
    if cap.glossy_samples is not None:
        res["spec_visibility"] = cap.spec_visibility
        res["glossy_trace"] = cap.surface.glossy_state
    res["transfer"] = cap.transfer
    if cap.bounce is not None:
        res["bounce"] = cap.bounce
    res["transfer_trace"] = cap.surface.transfer_state
    res["stats"] = cap.stats()
    res["trace"] = cap.surface.res
    return res
