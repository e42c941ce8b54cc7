"""Environment lights for the traced surface: 9 spherical-harmonic coefficients per colour (include/oi_envlight.h; DESIGN
section 4.18).

An EnvLight is the band 0 .. 2 projection of a radiance distribution over the sphere, in the WORLD frame, (9, 3): coefficient-
major, RGB, in the header's fixed basis order.  oi_amd.trace.capture_transfer traces the secondary rays of one view once; the
capture is then shaded under any number of EnvLights -- or rotations of one -- with a 9-term dot product per pixel and channel.

    env = EnvLight.from_equirect(img)                 # (3, He, We): projected by the GPU kernel (oi_env_project)
    cap = trace.capture_transfer(gen, z, b2w)         # one primary trace, one full MLP pass, one 64-sample occlusion trace
    out = cap.shade([env, env.rotated(R)])            # image / shading (2, 3, H, W)

An EnvLight carries the diffuse response only.  An EnvMap adds the Phong lobe of the learned material (include/oi_envgloss.h;
DESIGN section 4.20): the environment map convolved with relu(cos)^shininess once, looked up along the reflected view vector,
times a reflection-lobe visibility that capture_transfer(glossy_samples=...) traces with the view.

    env = EnvMap.from_equirect(img, shininess=10)     # the SH half as above, and the prefiltered map (oi_env_prefilter)
    cap = trace.capture_transfer(gen, z, b2w, glossy_samples=64)
    out = cap.shade([env, env.rotated(R)])            # image / shading / specular (2, 3, H, W); nothing is prefiltered again

capture_transfer(bounces=1) folds one diffuse interreflection bounce into a per-channel transfer (include/oi_envbounce.h;
DESIGN section 4.22): an EnvLight capture then also returns the indirect part of the shading.  In a scene of many instances
(oi_amd.scene.SceneSurface.capture_transfer(bounces=1); include/oi_scene_bounce.h) the bounce is between
the instances too: the nearest instance a transfer ray meets reflects its colour.

Bands above 2 of the diffuse term, more than one bounce and the bounce under an EnvMap are out of scope."""
import math
import warnings

import numpy as np
import torch

from . import lib as _l

N_COEFFS = _l.ENV_COEFFS
BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)
# the clamped-cosine kernel per band, divided by pi (Ramamoorthi & Hanrahan 2001): the unshadowed transfer is A_band y_c(n)
A_HAT = (1.0, 2.0 / 3.0, 0.25)

_K0 = 0.5 / math.sqrt(math.pi)
_K1 = math.sqrt(3.0 / (4.0 * math.pi))
_K2 = math.sqrt(15.0 / (4.0 * math.pi))
_K3 = math.sqrt(5.0 / (16.0 * math.pi))
_K4 = math.sqrt(15.0 / (16.0 * math.pi))


def sh_basis(d):
    """The header's basis at unit vectors d (..., 3), float64 -> (..., 9)."""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, _K0), _K1 * y, _K1 * z, _K1 * x, _K2 * x * y, _K2 * y * z, _K3 * (3.0 * z * z - 1.0),
                     _K2 * x * z, _K4 * (x * x - y * y)], -1)


def _fixed_directions(n=32):
    """A Fibonacci lattice on the sphere: fixed, and well-conditioned for the band 1 and band 2 solves below."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * math.pi * (3.0 - math.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], -1)


def sh_rotation(R):
    """The 9 x 9 matrix M with coefficients' = M coefficients for the rotated function f'(d) = f(R^T d) (R: a 3 x 3 world
    rotation, float64).  Block-diagonal (1, 3, 5): per band, the basis is evaluated at a fixed set of directions d_k and at
    R^T d_k, and Y M = Y_rot is solved in the least-squares sense -- exact, since a rotation maps each band onto itself."""
    R = np.asarray(R.detach().cpu().numpy() if torch.is_tensor(R) else R, dtype=np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError(f"sh_rotation: R of shape {R.shape} (a finite 3 x 3 rotation)")
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0:
        raise ValueError("sh_rotation: R is not a rotation (R R^T = 1, det R = +1)")
    d, solve = _rotation_solver()
    Yr = sh_basis(d @ R)                   # row k of d @ R is R^T d_k
    M = np.zeros((N_COEFFS, N_COEFFS))
    for (a, b), pinv in solve:
        M[a:b, a:b] = pinv @ Yr[:, a:b]
    return M


_SOLVER = []


def _rotation_solver():
    """The fixed directions and, per band, the pseudo-inverse of the basis there (the least-squares solve, done once)."""
    if not _SOLVER:
        d = _fixed_directions()
        Y = sh_basis(d)
        _SOLVER.append((d, [((a, b), np.linalg.pinv(Y[:, a:b])) for a, b in ((0, 1), (1, 4), (4, 9))]))
    return _SOLVER[0]


class EnvLight:
    """SH coefficients (9, 3) of an environment in the world frame (float64 on the host).  Fewer than 9 rows are padded
    with zeros (a band 0 .. 1 light); a (9,) vector means grey."""

    def __init__(self, coeffs):
        c = np.asarray(coeffs.detach().cpu().numpy() if torch.is_tensor(coeffs) else coeffs, dtype=np.float64)
        if c.ndim == 1:
            c = np.repeat(c[:, None], 3, axis=1)
        if c.ndim != 2 or c.shape[1] != 3 or not 1 <= c.shape[0] <= N_COEFFS:
            raise ValueError(f"EnvLight: coefficients of shape {c.shape} (at most {N_COEFFS} rows of RGB: bands 0 .. 2)")
        if not np.isfinite(c).all():
            raise ValueError("EnvLight: coefficients must be finite")
        self.coeffs = np.zeros((N_COEFFS, 3))
        self.coeffs[:c.shape[0]] = c

    @classmethod
    def constant(cls, rgb):
        """Radiance `rgb` from every direction: L_0 = 2 sqrt(pi) rgb, so an unoccluded point is shaded `rgb`."""
        c = np.zeros((N_COEFFS, 3))
        c[0] = 2.0 * math.sqrt(math.pi) * np.broadcast_to(np.asarray(rgb, dtype=np.float64), (3,))
        return cls(c)

    @classmethod
    def from_equirect(cls, img, device="cuda"):
        """An equirectangular radiance map (3, He, We) or (He, We, 3), numpy or tensor: row r at polar angle
        pi (r + 1/2) / He from +z, column c at azimuth 2 pi (c + 1/2) / We.  Projected on the GPU (oi_env_project)."""
        from . import ops
        t = _equirect_tensor(img, "EnvLight.from_equirect")
        t = t.to(device=device if not t.is_cuda else t.device, dtype=torch.float32).contiguous()
        return cls(ops.env_project(t[None])[0])

    @classmethod
    def from_lights(cls, lights):
        """The diffuse and ambient terms of directional lights (oi_amd.relight.Light objects) as one environment:
        L_c = pi diffuse y_c(direction / |direction|), plus 2 sqrt(pi) ambient on c = 0.  Band-limited: with the unshadowed
        transfer a light's max(n . l, 0) becomes 1/4 + cos / 2 + (5 / 32) (3 cos^2 - 1), at most 0.094 off.  The specular
        term has no diffuse counterpart and is DROPPED here; an EnvMap carries it."""
        from .relight import Light
        lights = [lights] if isinstance(lights, Light) else list(lights)
        c = np.zeros((N_COEFFS, 3))
        for lt in lights:
            if not isinstance(lt, Light):
                raise TypeError(f"EnvLight.from_lights: expected Light objects, got {type(lt).__name__}")
            d = np.asarray(lt.direction, dtype=np.float64)
            c += math.pi * sh_basis(d / np.linalg.norm(d))[:, None] * np.asarray(lt.diffuse)[None, :]
            c[0] += 2.0 * math.sqrt(math.pi) * np.asarray(lt.ambient)
        return cls(c)

    def rotated(self, R):
        """The environment turned by the world rotation R (3 x 3): radiance'(d) = radiance(R^T d).  Host, float64."""
        return EnvLight(sh_rotation(R) @ self.coeffs)

    def radiance(self, d):
        """The band-limited radiance towards unit vectors d (..., 3) -> (..., 3)."""
        return sh_basis(d) @ self.coeffs

    def __repr__(self):
        return f"EnvLight(L0={self.coeffs[0].tolist()})"


class EnvMap:
    """An environment for a glossy surface: `sh`, the EnvLight of its diffuse half; `map`, the radiance convolved with the
    Phong lobe of `shininess`, G_s(d) = (1 / pi) integral of L(w) relu(w . d)^s dw, float32 (3, Hp, Wp) on the header's
    equirectangular grid; `rotation`, the world rotation R (3, 3) float64 the environment has been turned by since the map
    was made: G'(d) = G(R^T d), so rotated() shares the map and composes R."""

    def __init__(self, sh, glossy_map, shininess, rotation=None):
        from . import ops
        if not isinstance(sh, EnvLight):
            raise TypeError(f"EnvMap: expected an EnvLight for the diffuse half, got {type(sh).__name__}")
        if not torch.is_tensor(glossy_map) or glossy_map.dim() != 3 or glossy_map.shape[0] != 3 or glossy_map.dtype != torch.float32:
            raise ValueError("EnvMap: the prefiltered map is a float32 tensor (3, Hp, Wp)")
        self.sh, self.map, self.shininess = sh, glossy_map, ops.check_shininess(shininess, "EnvMap")
        self.rotation = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64)
        self._host = None

    @classmethod
    def from_equirect(cls, img, shininess, size=(64, 128), device="cuda"):
        """EnvLight.from_equirect's image, projected (oi_env_project) and prefiltered to size = (Hp, Wp) (oi_env_prefilter) on
        the GPU.  The sum over the He x We pixels is a midpoint rule: it resolves the lobe only while a pixel is narrower
        than the lobe, and a warning is issued when He < 2 sqrt(shininess) (a constant 16 x 32 map at shininess 200 comes
        out 24 % off).  The warning speaks for directions away from the poles.  A lobe that reaches a pole needs a finer map than
        it implies, because the first band's midpoint cannot stand for the band: a constant 32 x 64 map at shininess 200 passes
        the rule (28.3 rows) and is within 4e-4 elsewhere, but the texels within 0.4 rad of a pole come out up to 9 % off (2 % at
        shininess 50); DESIGN section 4.20 has the figures."""
        from . import ops
        s = ops.check_shininess(shininess, "EnvMap.from_equirect")
        t = _equirect_tensor(img, "EnvMap.from_equirect")
        if t.shape[1] < 2.0 * math.sqrt(s):
            warnings.warn(f"EnvMap.from_equirect: a map of {t.shape[1]} rows is too coarse a quadrature for shininess {s:g} "
                          f"(He >= 2 sqrt(shininess) = {2.0 * math.sqrt(s):.1f}): the lobe falls between the pixels")
        t = t.to(device=device if not t.is_cuda else t.device, dtype=torch.float32).contiguous()
        sh = EnvLight(ops.env_project(t[None])[0])
        return cls(sh, ops.env_prefilter(t[None], s, size)[0], s)

    @classmethod
    def constant(cls, rgb, shininess):
        """Radiance `rgb` from every direction: the closed form G_s = rgb 2 / (s + 1) in a 1 x 1 map (host memory until a
        capture is shaded)."""
        from . import ops
        s = ops.check_shininess(shininess, "EnvMap.constant")
        g = np.broadcast_to(np.asarray(rgb, dtype=np.float64), (3,)) * 2.0 / (s + 1.0)
        return cls(EnvLight.constant(rgb), torch.tensor(g, dtype=torch.float32).view(3, 1, 1), s)

    def rotated(self, R):
        """The environment turned by the world rotation R: the SH half as EnvLight.rotated, the map shared, R composed."""
        M = sh_rotation(R)   # (checks R)
        R = np.asarray(R.detach().cpu().numpy() if torch.is_tensor(R) else R, dtype=np.float64)
        out = EnvMap(EnvLight(M @ self.sh.coeffs), self.map, self.shininess, R @ self.rotation)
        out._host = self._host
        return out

    def glossy(self, d):
        """G_s towards unit world vectors d (..., 3) -> (..., 3): oi_env_shade_glossy's lookup in float64 on the host."""
        if self._host is None:
            self._host = self.map.detach().cpu().numpy().astype(np.float64)
        g = self._host
        Hp, Wp = g.shape[1:]
        d = np.asarray(d, dtype=np.float64) @ self.rotation          # row k: R^T d_k
        theta = np.arccos(np.clip(d[..., 2], -1.0, 1.0))
        phi = np.arctan2(d[..., 1], d[..., 0])
        phi = np.where(phi < 0, phi + 2.0 * math.pi, phi)
        u, v = theta / math.pi * Hp - 0.5, phi / (2.0 * math.pi) * Wp - 0.5
        i0, j0 = np.floor(u), np.floor(v)
        fu, fv = (u - i0)[..., None], (v - j0)[..., None]
        i1 = np.clip(i0 + 1, 0, Hp - 1).astype(int)
        i0 = np.clip(i0, 0, Hp - 1).astype(int)
        j0 = np.mod(j0.astype(int), Wp)
        j1 = np.mod(j0 + 1, Wp)
        at = lambda i, j: np.moveaxis(g[:, i, j], 0, -1)
        top = at(i0, j0) + fv * (at(i0, j1) - at(i0, j0))
        bot = at(i1, j0) + fv * (at(i1, j1) - at(i1, j0))
        return top + fu * (bot - top)

    def __repr__(self):
        return f"EnvMap(shininess={self.shininess:g}, map={tuple(self.map.shape[1:])}, L0={self.sh.coeffs[0].tolist()})"


def _equirect_tensor(img, what):
    """An equirectangular image (3, He, We) or (He, We, 3), numpy or tensor -> a (3, He, We) tensor."""
    t = img if torch.is_tensor(img) else torch.as_tensor(np.asarray(img))
    if t.dim() != 3 or (t.shape[0] != 3 and t.shape[-1] != 3):
        raise ValueError(f"{what}: image of shape {tuple(t.shape)} (expected (3, He, We) or (He, We, 3))")
    return t if t.shape[0] == 3 else t.permute(2, 0, 1)


def stack_maps(envs, device="cuda"):
    """EnvMaps -> what oi_env_shade_glossy reads: the SH halves (F, 9, 3), the DISTINCT maps stacked (M, 3, Hp, Wp) --
    rotations of one map share one entry --, the F map indices (host integers) and the rotations (F, 3, 3), float32 on
    `device`; and the common shininess."""
    envs = [envs] if isinstance(envs, EnvMap) else list(envs)
    if not envs or not all(isinstance(e, EnvMap) for e in envs):
        raise TypeError("stack_maps: expected one or more EnvMap objects")
    if any(e.shininess != envs[0].shininess for e in envs):
        raise ValueError(f"stack_maps: the maps were prefiltered for different shininess values "
                         f"{sorted({e.shininess for e in envs})}; one launch has one")
    maps, index = {}, []
    for e in envs:
        index.append(maps.setdefault(id(e.map), (len(maps), e.map))[0])
    tensors = [m for _, m in maps.values()]
    if any(m.shape != tensors[0].shape for m in tensors):
        raise ValueError(f"stack_maps: maps of different sizes {sorted({tuple(m.shape[1:]) for m in tensors})} in one call")
    # (one map, the case of a rotation walk: a view of it, nothing is copied when it is on the device already)
    stack = tensors[0].to(device)[None] if len(tensors) == 1 else torch.stack([m.to(device) for m in tensors])
    rot = torch.tensor(np.stack([e.rotation for e in envs]), dtype=torch.float32, device=device)
    return stack_envs([e.sh for e in envs], device), stack, index, rot, envs[0].shininess


def stack_envs(envs, device="cuda"):
    """EnvLights -> the (F, 9, 3) float32 array oi_env_shade reads."""
    envs = [envs] if isinstance(envs, EnvLight) else list(envs)
    if not envs:
        raise ValueError("stack_envs: no environments given")
    for e in envs:
        if not isinstance(e, EnvLight):
            raise TypeError(f"stack_envs: expected EnvLight objects, got {type(e).__name__}")
    return torch.tensor(np.stack([e.coeffs for e in envs]), dtype=torch.float32, device=device)


def axis_rotation(axis, angle):
    """Rodrigues: the 3 x 3 rotation by `angle` radians about `axis` (float64)."""
    a = np.asarray(axis, dtype=np.float64).reshape(3)
    n = np.linalg.norm(a)
    if not np.isfinite(a).all() or n == 0:
        raise ValueError(f"axis_rotation: axis {tuple(a)} (finite and non-zero)")
    a = a / n
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)
