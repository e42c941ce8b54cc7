"""Relighting: one render of an instance, then the same instance under lights the caller chooses.

The shading of Generator.render_maps (generator.py:107-172; lighting.py:126-225) is a per-sample function of the compositing
weight, the raw SDF gradient, the albedo and the view direction, none of which depends on the light.  `capture` keeps those
tensors of one eval forward; `relight` shades and composites them under L lights per launch (oi_relight_fwd,
include/oi_relight.h) without running the network again.  The lights are the reference's directional Phong light with the
three colours widened to RGB.

    cap = capture(gen, z=z, b2w=b2w)                 # (B, 64) latents, (B, 4, 4) poses
    base = Light.from_module(gen.light)              # the trained light, exactly
    out = relight(cap, [base, base.replace(diffuse=(1.0, 0.5, 0.2))], outputs=("image", "specular_map"))
    out["image"]                                     # (L, B, 3, H, W)

LocalLight is the light that stands IN the world -- a position, an inverse-square falloff, an optional cone and size -- for the
traced surface and scenes (oi_amd.trace.render_surface, oi_amd.scene.render_scene; include/oi_local_light.h); the volume
relighter above takes directional Lights only."""
import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import generator as G
from . import lib as _l
from . import ops

# Generator.forward keys of the light-dependent maps and the kernel output each comes from; the last two are derived on
# the host as generator.py does them
_KERNEL_KEYS = {"image": "image", "image_no_bg": "image_no_bg", "shading_map": "shading", "diff_shading_map": "diffuse",
                "specular_map": "specular"}
MAP_KEYS = tuple(_KERNEL_KEYS) + ("amb_shading_map", "no_specular_map")
# the light-independent maps a capture keeps from its forward
CAPTURE_MAP_KEYS = ("color_map", "normal_map", "mask", "weight_sum_map", "z_map")
# bytes of kernel output one relight launch may allocate (the launch is split over its lights beyond that)
LAUNCH_OUTPUT_BYTES = 1 << 30


def _rgb(v, name):
    t = tuple(float(x) for x in (np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))))
    if not all(math.isfinite(x) for x in t):
        raise ValueError(f"Light.{name} must be finite, got {t}")
    return t


@dataclasses.dataclass(frozen=True)
class Light:
    """A directional Phong light.  `direction`: world frame, any non-zero length (normalised where it is used, as
    DirectionalLight.direction does); `ambient`, `diffuse`, `specular`: RGB (a scalar means grey); `shininess`: the
    specular exponent."""
    direction: Tuple[float, float, float]
    ambient: Tuple[float, float, float] = (0.33, 0.33, 0.33)
    diffuse: Tuple[float, float, float] = (0.66, 0.66, 0.66)
    specular: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    shininess: float = 10.0

    def __post_init__(self):
        d = tuple(float(x) for x in np.asarray(self.direction, dtype=np.float64).reshape(3))
        if not all(math.isfinite(x) for x in d) or math.sqrt(sum(x * x for x in d)) == 0.0:
            raise ValueError(f"Light.direction must be finite and non-zero, got {d}")
        object.__setattr__(self, "direction", d)
        for name in ("ambient", "diffuse", "specular"):
            object.__setattr__(self, name, _rgb(getattr(self, name), name))
        s = float(self.shininess)
        if not math.isfinite(s):
            raise ValueError(f"Light.shininess must be finite, got {s}")
        object.__setattr__(self, "shininess", s)

    @classmethod
    def from_module(cls, light):
        """The light of a DirectionalLightWithSpecularFixInit in these terms (lighting.py:23-52), fp32 as the compositing
        kernel forms it: ambient = sigmoid(a), diffuse = 1 - sigmoid(a), specular = max(s, 0), shininess and the
        (un-normalised) direction as stored."""
        f32 = np.float32
        a = f32(light.param_ambient.detach().float().cpu().item())
        amb = f32(1.0) / (f32(1.0) + np.exp(-a, dtype=f32))
        dif = f32(1.0) - amb
        spec = max(f32(light.param_specular.detach().float().cpu().item()), f32(0.0))
        d = light.param_direction.detach().float().cpu().numpy()
        return cls(direction=tuple(float(x) for x in d), ambient=(float(amb),) * 3, diffuse=(float(dif),) * 3,
                   specular=(float(spec),) * 3, shininess=float(light.param_shininess.detach().float().cpu().item()))

    def replace(self, **changes):
        """A copy with some fields changed (material and colour edits); colours may be given as scalars."""
        return dataclasses.replace(self, **changes)

    def packed(self):
        """The 16 floats of one light as oi_relight_fwd reads them."""
        return [*self.direction, 0.0, *self.ambient, 0.0, *self.diffuse, 0.0, *self.specular, self.shininess]


def stack_lights(lights, device="cuda"):
    """Lights -> the (L, 16) float32 array oi_relight_fwd reads (include/oi_relight.h)."""
    lights = [lights] if isinstance(lights, Light) else list(lights)
    if not lights:
        raise ValueError("relight: no lights given")
    for lt in lights:
        if not isinstance(lt, Light):
            raise TypeError(f"relight: expected Light objects, got {type(lt).__name__}")
    return torch.tensor([lt.packed() for lt in lights], dtype=torch.float32, device=device)


def _vec3(v, name):
    t = tuple(float(x) for x in np.asarray(v, dtype=np.float64).reshape(3))
    if not all(math.isfinite(x) for x in t):
        raise ValueError(f"LocalLight.{name} must be finite, got {t}")
    return t


@dataclasses.dataclass(frozen=True)
class LocalLight:
    """A Phong light that stands IN the world of a traced view or scene (include/oi_local_light.h; oi_amd.trace.render_surface
    and oi_amd.scene.render_scene take a list of them as `lights`): its direction differs per pixel, it falls off with the
    inverse square of the distance, and its shadow rays end at the light.
    position: world frame.  ambient, diffuse, specular (RGB; a scalar means grey), shininess: Light's; diffuse and specular
    are the colours at reference_distance (> 0) and scale as (reference_distance / distance)^2; ambient does not fall off.
    radius >= 0: the emitting sphere (0: a point): shadow samples are drawn over it, and the falloff is evaluated no nearer
    than max(radius, LOCAL_LIGHT_MIN_DISTANCE).  A spot light has cone_axis (world frame, pointing away from the light, any
    non-zero length) and the half-angles 0 < cone_inner < cone_outer <= pi in radians: full intensity inside the inner cone,
    none outside the outer one, a smoothstep of the angle's cosine between."""
    position: Tuple[float, float, float]
    ambient: Tuple[float, float, float] = (0.33, 0.33, 0.33)
    diffuse: Tuple[float, float, float] = (0.66, 0.66, 0.66)
    specular: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    shininess: float = 10.0
    radius: float = 0.0
    reference_distance: float = 1.0
    cone_axis: Optional[Tuple[float, float, float]] = None
    cone_inner: Optional[float] = None
    cone_outer: Optional[float] = None

    def __post_init__(self):
        object.__setattr__(self, "position", _vec3(self.position, "position"))
        for name in ("ambient", "diffuse", "specular"):
            try:
                object.__setattr__(self, name, _rgb(getattr(self, name), name))
            except ValueError as e:
                raise ValueError(str(e).replace("Light.", "LocalLight.", 1)) from None
        for name in ("shininess", "radius", "reference_distance"):
            v = float(getattr(self, name))
            if not math.isfinite(v):
                raise ValueError(f"LocalLight.{name} must be finite, got {v}")
            object.__setattr__(self, name, v)
        if self.radius < 0:
            raise ValueError(f"LocalLight.radius must be >= 0, got {self.radius}")
        if self.reference_distance <= 0:
            raise ValueError(f"LocalLight.reference_distance must be > 0, got {self.reference_distance}")
        cone = (self.cone_axis, self.cone_inner, self.cone_outer)
        if all(c is None for c in cone):
            return
        if self.cone_axis is None:
            raise ValueError("LocalLight: cone_inner / cone_outer without cone_axis (a cone needs its axis)")
        axis = _vec3(self.cone_axis, "cone_axis")
        if math.sqrt(sum(x * x for x in axis)) == 0.0:
            raise ValueError("LocalLight.cone_axis must be non-zero")
        object.__setattr__(self, "cone_axis", axis)
        if self.cone_inner is None or self.cone_outer is None:
            raise ValueError("LocalLight: a cone needs cone_inner and cone_outer (radians)")
        ci, co = float(self.cone_inner), float(self.cone_outer)
        if not (math.isfinite(ci) and math.isfinite(co) and 0 < ci < co <= math.pi):
            raise ValueError(f"LocalLight: cone_inner={ci}, cone_outer={co} (radians, 0 < cone_inner < cone_outer <= pi)")
        object.__setattr__(self, "cone_inner", ci)
        object.__setattr__(self, "cone_outer", co)

    @classmethod
    def from_light(cls, light, distance, centre=(0.0, 0.0, 0.0)):
        """The local light that stands at centre + distance * (light.direction / |direction|) with `light`'s colours at that
        distance (reference_distance = distance): near `centre` it approaches the directional light as the distance grows."""
        d = np.asarray(light.direction, dtype=np.float64)
        pos = np.asarray(centre, dtype=np.float64).reshape(3) + float(distance) * d / np.linalg.norm(d)
        return cls(position=tuple(pos), ambient=light.ambient, diffuse=light.diffuse, specular=light.specular,
                   shininess=light.shininess, reference_distance=float(distance))

    def replace(self, **changes):
        """A copy with some fields changed; colours may be given as scalars."""
        return dataclasses.replace(self, **changes)

    def packed(self):
        """The LOCAL_LIGHT_FLOATS floats of one light as include/oi_local_light.h lays them out."""
        if self.cone_axis is None:
            axis, cos_outer, cos_inner = (0.0, 0.0, 0.0), -2.0, 2.0     # cos_outer <= -1: no cone, the axis is not read
        else:
            # (cos(pi) is -1, the record's "no cone": the widest cone keeps its smoothstep one fp32 step above it)
            axis, cos_outer, cos_inner = self.cone_axis, max(math.cos(self.cone_outer), -1.0 + 2.0 ** -24), math.cos(self.cone_inner)
        return [*self.position, self.radius, *self.ambient, self.reference_distance, *self.diffuse, cos_outer, *self.specular,
                self.shininess, *axis, cos_inner]


def stack_local_lights(lights, device="cuda"):
    """LocalLights -> the (L, LOCAL_LIGHT_FLOATS) float32 array the local-light entries read (include/oi_local_light.h)."""
    lights = [lights] if isinstance(lights, LocalLight) else list(lights)
    if not lights:
        raise ValueError("stack_local_lights: no lights given")
    for lt in lights:
        if not isinstance(lt, LocalLight):
            raise TypeError(f"stack_local_lights: expected LocalLight objects, got {type(lt).__name__}")
    return torch.tensor([lt.packed() for lt in lights], dtype=torch.float32, device=device)


def local_lights_given(lights):
    """Is `lights` (None, a light or a sequence of lights) a set of LocalLights?  A list that mixes them with directional Lights
    is refused: the two kinds are shaded by different kernels."""
    if lights is None or isinstance(lights, Light):
        return False
    seq = [lights] if isinstance(lights, LocalLight) else list(lights)
    n = sum(isinstance(lt, LocalLight) for lt in seq)
    if n and n != len(seq):
        raise ValueError("lights: LocalLight and Light objects in one list (render them in two calls)")
    return n > 0


@dataclasses.dataclass
class Capture:
    """The light-independent state of one render.  Per-sample tensors are references to the forward's own outputs (no
    copy): weights, mid_z (N, T), gradients, albedo (N, T, 3) -- 32 bytes per sample, about 170 MB at 128 x 128 pixels
    and 256 + 64 samples per ray.  `maps`: the forward's light-independent maps (CAPTURE_MAP_KEYS, (B, C, H, W));
    `render_out`: everything the forward returned; `light`: the generator's light when the capture was taken."""
    weights: torch.Tensor
    gradients: torch.Tensor
    albedo: torch.Tensor
    mid_z: torch.Tensor
    rays_o: torch.Tensor
    rays_d: torch.Tensor
    w2b: torch.Tensor
    bg: torch.Tensor
    B: int
    H: int
    W: int
    maps: dict
    render_out: dict
    light: Light

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.weights, self.gradients, self.albedo, self.mid_z))


@torch.no_grad()
def capture(gen, z=None, w=None, b2w=None, bg=None, max_ray_batch=None):
    """One eval Generator.forward(bs=B, return_raw=True) -- several ray chunks when B * H * W exceeds the ray batch, as
    generator.py:286-305 does -- and a Capture of it.  z (B, z_dim) or w (B, style_dim): the latent; b2w (B, 4, 4): the
    poses; bg (B, 3) or (3,): the background colour of the forward and the default of `relight` (black when None; the
    forward then draws nothing from numpy).  Puts `gen` in eval mode, as inference.render_frames does."""
    if b2w is None:
        raise ValueError("capture: b2w (B, 4, 4) poses are required")
    if z is None and w is None:
        raise ValueError("capture: pass a latent z or a style vector w")
    gen.eval()
    gen.renderer.pack.check()
    dev = gen.it.device
    b2w = b2w.to(dev, torch.float32).reshape(-1, 4, 4)
    B = b2w.shape[0]
    bg = torch.zeros(B, 3, device=dev) if bg is None else torch.as_tensor(bg, dtype=torch.float32).to(dev).expand(B, 3)
    bg = bg.contiguous()
    data = {"b2w": b2w, "bg_color": bg}
    if w is not None:
        data.update(w=w.to(dev), z=None if z is None else z.to(dev))
    else:
        data["z"] = z.to(dev)
    old = G.MAX_RAY_BATCH_SIZE
    if max_ray_batch is not None:
        G.MAX_RAY_BATCH_SIZE = max_ray_batch
    try:
        blob = gen(bs=B, it=None, data=data, return_raw=True)["box"]
    finally:
        G.MAX_RAY_BATCH_SIZE = old
    raw, ro = blob["raw_render_out"], blob["render_out"]
    H = W = gen.resolution
    return Capture(weights=raw["weights"], gradients=raw["gradients"], albedo=raw["raw_color"], mid_z=raw["mid_z_vals"],
                   rays_o=blob["rays_info"]["rays_o"].reshape(-1, 3), rays_d=blob["rays_info"]["rays_d"].reshape(-1, 3),
                   w2b=blob["prior_info"]["w2b"].contiguous(), bg=bg, B=B, H=H, W=W,
                   maps={k: ro[k] for k in CAPTURE_MAP_KEYS}, render_out=ro, light=Light.from_module(gen.light))


@torch.no_grad()
def relight(cap, lights, outputs=("image",), bg=None):
    """The captured render under each of `lights` (a Light or a sequence of them).  -> {key: (L, B, 3, H, W)} for each key
    of `outputs`, named as Generator.forward names them (MAP_KEYS): image, image_no_bg, shading_map, diff_shading_map,
    specular_map, and amb_shading_map / no_specular_map derived as generator.py derives them.  bg: (B, 3) or (3,)
    background colour, default the capture's.  The lights are split over launches of at most OI_RELIGHT_MAX_LIGHTS, fewer
    when one launch's outputs would exceed LAUNCH_OUTPUT_BYTES."""
    for k in outputs:
        if k not in MAP_KEYS:
            raise ValueError(f"relight: unknown output {k!r} (one of {MAP_KEYS})")
    lights = [lights] if isinstance(lights, Light) else list(lights)
    dev = cap.weights.device
    lt = stack_lights(lights, dev)
    nl, B, H, W = lt.shape[0], cap.B, cap.H, cap.W
    bg = cap.bg if bg is None else torch.as_tensor(bg, dtype=torch.float32).to(dev).expand(B, 3).contiguous()
    need = {_KERNEL_KEYS[k] for k in outputs if k in _KERNEL_KEYS}
    if "no_specular_map" in outputs:
        need |= {"image_no_bg", "specular"}
    kernel_out = [k for k in ops.RELIGHT_OUT if k in need]
    res = {k: ops._new(cap.weights, nl, B, 3, H * W) for k in kernel_out}
    per_light = max(1, len(kernel_out)) * B * 3 * H * W * 4
    step = max(1, min(_l.RELIGHT_MAX_LIGHTS, LAUNCH_OUTPUT_BYTES // per_light))
    if kernel_out:
        for s in range(0, nl, step):
            e = min(nl, s + step)
            ops.relight_fwd(cap.weights, cap.gradients, cap.albedo, cap.mid_z, cap.rays_o, cap.rays_d, cap.w2b, lt[s:e], bg,
                            B, outputs=kernel_out, out={k: v[s:e] for k, v in res.items()})
    maps = {k: v.view(nl, B, 3, H, W) for k, v in res.items()}
    out = {}
    for k in outputs:
        if k in _KERNEL_KEYS:
            out[k] = maps[_KERNEL_KEYS[k]]
        elif k == "amb_shading_map":   # generator.py: ambient * weight_sum, per channel here
            amb = torch.tensor([lt_.ambient for lt_ in lights], dtype=torch.float32, device=dev)
            out[k] = amb[:, None, :, None, None] * cap.maps["weight_sum_map"][None]
        else:                          # no_specular_map: image_no_bg - specular_map (generator.py)
            out[k] = maps["image_no_bg"] - maps["specular"]
    return out
