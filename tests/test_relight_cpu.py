"""CPU checks of relighting (include/oi_relight.h, oi_amd.relight): the fp64 restatement against the oracle's shading, the
light conversion and packing, the light-walk schedule, the argument checks of the C ABI, and the coverage rule of the
new header (every writing entry point is called by the guarded GPU test)."""
import ast
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import oi_oracle as O
from conftest import ROOT
from helpers import cabi
from helpers.relight_ref import relight_ref

GPU_TEST = os.path.join(ROOT, "tests", "test_gpu_relight.py")


def _synthetic(B, hw, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = B * hw
    alpha = torch.rand(N, T, generator=g, dtype=torch.float64) * 0.2
    trans = torch.cumprod(torch.cat([torch.ones(N, 1, dtype=torch.float64), 1 - alpha[:, :-1]], 1), 1)
    return {
        "weights": alpha * trans,
        "grad": torch.randn(N, T, 3, generator=g, dtype=torch.float64),
        "rgb": torch.rand(N, T, 3, generator=g, dtype=torch.float64),
        "mid_z": 2.0 + 2.0 * torch.rand(N, T, generator=g, dtype=torch.float64).sort(1).values,
        "rays_o": torch.tensor([0.0, 0.0, -4.0], dtype=torch.float64) + 0.1 * torch.randn(N, 3, generator=g, dtype=torch.float64),
        "rays_d": torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
                                                + 0.2 * torch.randn(N, 3, generator=g, dtype=torch.float64), dim=-1),
    }


def _w2b(B, seed=1):
    from scipy.spatial.transform import Rotation as R
    rots = R.random(B, random_state=seed).as_matrix()
    m = torch.zeros(B, 4, 4, dtype=torch.float64)
    m[:, :3, :3] = torch.from_numpy(rots)
    m[:, :3, 3] = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64)
    m[:, 3, 3] = 1.0
    return m


@pytest.mark.parametrize("B", [1, 2])
def test_restatement_equals_oracle_render_maps_for_grey_lights(B):
    """relight_ref with grey colours is oi_oracle.render_maps (the reference's formulas) on the same per-sample data."""
    H, W_, T = 3, 4, 37
    s = _synthetic(B, H * W_, T)
    w2b = _w2b(B)
    bg = torch.rand(B, 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ro = {"weights": s["weights"], "gradients": s["grad"], "raw_color": s["rgb"], "mid_z_vals": s["mid_z"],
          "pts": s["rays_o"][:, None] + s["rays_d"][:, None] * s["mid_z"][..., None],
          "weight_sum": s["weights"].sum(1, keepdim=True), "color_fine": (s["weights"][..., None] * s["rgb"]).sum(1)}
    from oi_amd.relight import Light
    for a, spec, shin, d in ((-0.7, 0.3, 10.0, (0.0, 0.0, -1.0)), (0.4, 0.0, 3.0, (0.3, -0.5, 0.8)),
                             (1.2, 0.8, 1.5, (-1.0, 2.0, 0.5))):
        lsd = {"param_direction": torch.tensor(d, dtype=torch.float64), "param_ambient": torch.tensor(a, dtype=torch.float64),
               "param_specular": torch.tensor(spec, dtype=torch.float64), "param_shininess": torch.tensor(shin, dtype=torch.float64)}
        ref = O.render_maps(ro, s["rays_o"], lsd, w2b, bg, B, H, W_, return_raw=True)
        amb = 1.0 / (1.0 + math.exp(-a))
        lt = Light(direction=d, ambient=amb, diffuse=1.0 - amb, specular=spec, shininess=shin)
        got = relight_ref(s["weights"], s["grad"], s["rgb"], s["mid_z"], s["rays_o"], s["rays_d"], w2b,
                          torch.tensor([lt.packed()], dtype=torch.float64), bg, B)
        for k, rk in (("image", "image"), ("image_no_bg", "image_no_bg"), ("shading", "shading_map"),
                      ("diffuse", "diff_shading_map"), ("specular", "specular_map")):
            err = float((got[k][0].reshape(B, 3, H, W_) - ref[rk]).abs().max())
            assert err < 1e-12, (k, err)


def test_light_from_module_and_packing():
    from oi_amd.lighting import DirectionalLightWithSpecularFixInit
    from oi_amd.relight import Light, stack_lights
    m = DirectionalLightWithSpecularFixInit(direction=[0.3, -0.2, -2.0], ambient_color=0.2, diffuse_color=0.7,
                                            specular_color=0.25, shininess=7.5)
    lt = Light.from_module(m)
    f32 = np.float32
    a = f32(m.param_ambient.item())
    amb = f32(1) / (f32(1) + np.exp(-a, dtype=f32))
    assert lt.ambient == (float(amb),) * 3 and abs(lt.ambient[0] - 0.2 / 0.9) < 1e-6
    assert lt.diffuse == (float(f32(1) - amb),) * 3
    assert lt.specular == (float(f32(0.25)),) * 3 and lt.shininess == 7.5
    assert lt.direction == tuple(float(x) for x in m.param_direction.detach().numpy())   # as stored, not normalised
    with torch.no_grad():
        m.param_specular.fill_(-0.5)
    assert Light.from_module(m).specular == (0.0, 0.0, 0.0)   # max(s, 0)
    red = lt.replace(diffuse=(1.0, 0.0, 0.0), shininess=20)
    assert red.diffuse == (1.0, 0.0, 0.0) and red.shininess == 20.0 and red.direction == lt.direction
    assert lt.replace(ambient=0.5).ambient == (0.5, 0.5, 0.5)
    P = stack_lights([lt, red], device="cpu")
    assert P.shape == (2, 16) and P.dtype == torch.float32
    row = P[1].tolist()
    assert row[0:3] == pytest.approx(list(red.direction)) and row[3] == row[7] == row[11] == 0.0
    assert row[4:7] == pytest.approx(list(red.ambient)) and row[8:11] == [1.0, 0.0, 0.0]
    assert row[12:15] == pytest.approx(list(red.specular)) and row[15] == 20.0
    assert torch.equal(stack_lights(lt, device="cpu"), P[:1])


def test_invalid_lights_raise():
    from oi_amd.relight import Light, stack_lights
    with pytest.raises(ValueError):
        Light(direction=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        Light(direction=(0.0, float("nan"), 1.0))
    with pytest.raises(ValueError):
        Light(direction=(0.0, 0.0, 1.0), diffuse=(1.0, float("inf"), 0.0))
    with pytest.raises(ValueError):
        stack_lights([], device="cpu")


@pytest.mark.parametrize("axis", [(0, -1, 0), (1.0, 0.0, 0.0)])
def test_light_walk_schedule(axis):
    from oi_amd.inference import light_walk_directions
    from scipy.spatial.transform import Rotation as R
    d0 = np.array([0.3, -0.2, -2.0])
    n = 12
    dirs = light_walk_directions(d0, n, axis)
    assert dirs.shape == (n, 3)
    assert np.allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=1e-12)
    assert np.array_equal(dirs[0], d0 / np.linalg.norm(d0))
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    assert np.allclose(dirs @ ax, dirs[0] @ ax, atol=1e-12)   # a turn about the axis
    step = R.from_rotvec(ax * 2 * math.pi / n).as_matrix()
    for i in range(n):   # equal steps, and the step after the last frame is frame 0 again: one full turn
        assert np.allclose(step @ dirs[i], dirs[(i + 1) % n], atol=1e-12)


def _header_exports():
    return list(cabi.parse(cabi.read("oi_relight.h"))[0])


def _code_only(path):
    import io
    import tokenize
    with open(path) as fh:
        toks = [t for t in tokenize.generate_tokens(io.StringIO(fh.read()).readline)
                if t.type not in (tokenize.COMMENT, tokenize.STRING)]
    return " ".join(t.string for t in toks)


def test_every_relight_export_has_a_guarded_case():
    """test_bounds_coverage_cpu.py's rule for include/oi_hip.h, applied to include/oi_relight.h and its guarded GPU test."""
    names = _header_exports()
    assert names == ["oi_relight_fwd"]
    src = _code_only(GPU_TEST)
    assert 'pytest.mark.usefixtures("guarded_ops")' in open(GPU_TEST).read(), \
        "tests/test_gpu_relight.py must run under the guarded_ops fixture"
    path = os.path.join(ROOT, "object-intrinsics_amd", "oi_amd", "ops.py")
    text = open(path).read()
    wrappers = {n.name: ast.get_source_segment(text, n) for n in ast.parse(text).body if isinstance(n, ast.FunctionDef)}
    called = {f for f in wrappers if re.search(r"\bops \. %s \(" % f, src)}
    for n in names:
        if re.search(r"\. %s \(" % n, src):
            continue
        via = [f for f in called if re.search(r"\.%s\(" % n, wrappers[f])]
        assert via, f"{n}: no case of tests/test_gpu_relight.py calls it"
        assert not all(re.search(r"torch\.empty", wrappers[f]) for f in via), (n, via)


_lib = cabi.built_lib


def test_library_exports_every_relight_symbol():
    lib, L = _lib()
    assert cabi.check_header("oi_relight.h", lib) == (["oi_relight_fwd"], ["RelightParams"])
    text = cabi.read("oi_relight.h")
    assert int(re.search(r"#define OI_RELIGHT_LIGHT_FLOATS (\d+)", text).group(1)) == lib.RELIGHT_LIGHT_FLOATS
    assert int(re.search(r"#define OI_RELIGHT_MAX_LIGHTS (\d+)", text).group(1)) == lib.RELIGHT_MAX_LIGHTS


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    fake = ctypes.c_void_p(0x1000)

    def params(**kw):
        P = lib.RelightParams()
        for n in ("weights", "grad", "rgb", "mid_z", "rays_o", "rays_d", "w2b", "lights", "image"):
            setattr(P, n, fake)
        P.N, P.T, P.B, P.L = 12, 5, 2, 3
        for k, v in kw.items():
            setattr(P, k, v)
        return P

    cases = [(dict(N=13), "N % B"), (dict(L=0), "L=0"), (dict(L=lib.RELIGHT_MAX_LIGHTS + 1), "L="), (dict(T=0), "T=0"),
             (dict(B=0), "B=0"), (dict(N=0), "N=0"), (dict(weights=None), "null"), (dict(lights=None), "null"),
             (dict(w2b=None), "null")]
    for kw, text in cases:
        rc = L.oi_relight_fwd(ctypes.byref(params(**kw)), None)
        assert rc == -1, (kw, rc)
        msg = L.oi_last_error().decode()
        assert msg.startswith("oi_relight_fwd") and text in msg, (kw, msg)
    assert L.oi_relight_fwd(None, None) == -1
