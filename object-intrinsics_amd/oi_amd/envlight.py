"""Environment lights for the traced surface: 9 spherical-harmonic coefficients per colour (include/oi_envlight.h; DESIGN
section 4.18).

An EnvLight is the band 0 .. 2 projection of a radiance distribution over the sphere, in the WORLD frame, (9, 3): coefficient-
major, RGB, in the header's fixed basis order.  oi_amd.trace.capture_transfer traces the secondary rays of one view once; the
capture is then shaded under any number of EnvLights -- or rotations of one -- with a 9-term dot product per pixel and channel.

    env = EnvLight.from_equirect(img)                 # (3, He, We): projected by the GPU kernel (oi_env_project)
    cap = trace.capture_transfer(gen, z, b2w)         # one primary trace, one full MLP pass, one 64-sample occlusion trace
    out = cap.shade([env, env.rotated(R)])            # image / shading (2, 3, H, W)

Only the diffuse response is modelled; glossy terms, bands above 2 and interreflection are out of scope."""
import math

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
        t = img if torch.is_tensor(img) else torch.as_tensor(np.asarray(img))
        if t.dim() != 3 or (t.shape[0] != 3 and t.shape[-1] != 3):
            raise ValueError(f"EnvLight.from_equirect: image of shape {tuple(t.shape)} (expected (3, He, We) or (He, We, 3))")
        if t.shape[0] != 3:
            t = t.permute(2, 0, 1)
        t = t.to(device=device if not t.is_cuda else t.device, dtype=torch.float32).contiguous()
        return cls(ops.env_project(t[None])[0])

    @classmethod
    def from_lights(cls, lights):
        """The diffuse and ambient terms of directional lights (oi_amd.relight.Light objects) as one environment:
        L_c = pi diffuse y_c(direction / |direction|), plus 2 sqrt(pi) ambient on c = 0.  Band-limited: with the unshadowed
        transfer a light's max(n . l, 0) becomes 1/4 + cos / 2 + (5 / 32) (3 cos^2 - 1), at most 0.094 off.  The specular
        term has no diffuse counterpart and is DROPPED."""
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
