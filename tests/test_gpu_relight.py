"""GPU tests of relighting (oi_relight_fwd, include/oi_relight.h; oi_amd.relight; inference.light_walk): the trained light
reproduces Generator.forward, grey lights reproduce a re-render, coloured lights match the fp64 restatement, results do
not depend on how lights are batched, limit shapes write exactly their outputs, bad arguments launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_modules as M
from conftest import load_golden, maxdiff, record_margin, sub_sd
from helpers.guarded import guarded_copy, guarded_ops  # noqa: F401  (fixture)
from helpers.relight_ref import relight_ref

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

BAR = 2e-6
MAPS = ("image", "image_no_bg", "shading_map", "diff_shading_map", "specular_map")
KERNEL_OUT = ("image", "image_no_bg", "shading", "diffuse", "specular")
BG = torch.tensor([[0.2, 0.5, 0.9], [0.7, 0.1, 0.3]])


def make_gen(precision, R=16, S=16, I=16):
    """The generator of test_gpu_modules.py (golden weights, the F5 colour head and light), with a visible specular term."""
    g = load_golden("f5_generator")
    gen = M.build_generator(R, S, I, 1, precision).eval()
    gen.color_network.load_state_dict(sub_sd(g, "color."))
    gen.light.load_state_dict(sub_sd(g, "light."))
    gen.it.fill_(int(g["it"]))
    with torch.no_grad():
        gen.light.param_specular.fill_(0.35)
        gen.light.param_shininess.fill_(6.0)
    return gen, g["z"], g["b2w"]


def coloured_lights(n, seed=0):
    from oi_amd.relight import Light
    rs = np.random.RandomState(seed)
    return [Light(direction=tuple(rs.randn(3)), ambient=tuple(0.3 * rs.rand(3)), diffuse=tuple(rs.rand(3)),
                  specular=tuple(0.5 * rs.rand(3)), shininess=float(1 + 20 * rs.rand())) for _ in range(n)]


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("chunked", [False, True])
def test_trained_light_reproduces_forward(precision, B, chunked):
    from oi_amd import relight as RL
    gen, z, b2w = make_gen(precision)
    cap = RL.capture(gen, z=z[:B], b2w=b2w[:B], bg=BG[:B], max_ray_batch=128 if chunked else None)
    assert cap.weights.shape == (B * 256, 32) and cap.gradients.shape == (B * 256, 32, 3)
    out = RL.relight(cap, RL.Light.from_module(gen.light), outputs=MAPS + ("amb_shading_map", "no_specular_map"))
    for k in MAPS + ("amb_shading_map", "no_specular_map"):
        assert out[k].shape == (1, B, 3, 16, 16), (k, out[k].shape)
        err = maxdiff(out[k][0], cap.render_out[k])
        record_margin(f"relight_forward[{precision},B={B},chunked={chunked}]", k, err)
        assert err < BAR, (k, err)
    assert float(cap.render_out["specular_map"].max()) > 1e-3   # the specular term is exercised


def test_grey_lights_equal_rerender():
    """Three lights of the reference's grey family: each relit image is a fresh forward with that light in gen.light."""
    from oi_amd import relight as RL
    gen, z, b2w = make_gen("f32")
    cap = RL.capture(gen, z=z, b2w=b2w, bg=BG)
    saved = {k: v.detach().clone() for k, v in gen.light.state_dict().items()}
    lights, refs = [], []
    for a, s, sh, d in ((-0.5, 0.4, 8.0, (0.4, -0.3, -1.0)), (0.8, 0.2, 3.0, (-0.7, 0.2, -0.4)), (0.0, 0.9, 20.0, (0.1, 0.9, -0.3))):
        with torch.no_grad():
            gen.light.param_ambient.fill_(a)
            gen.light.param_specular.fill_(s)
            gen.light.param_shininess.fill_(sh)
            gen.light.param_direction.copy_(torch.tensor(d))
            blob = gen(bs=2, it=None, data={"z": z.cuda(), "b2w": b2w.cuda(), "bg_color": BG.cuda()}, return_raw=True)["box"]
        lights.append(RL.Light.from_module(gen.light))
        refs.append({k: blob["render_out"][k].clone() for k in MAPS})
    gen.light.load_state_dict(saved)
    out = RL.relight(cap, lights, outputs=MAPS)
    for i, ref in enumerate(refs):
        for k in MAPS:
            err = maxdiff(out[k][i], ref[k])
            record_margin("relight_rerender", k, err)
            assert err < BAR, (i, k, err)


def _kernel(cap, lights, outputs=KERNEL_OUT, bg="capture"):
    from oi_amd import ops
    from oi_amd.relight import stack_lights
    return ops.relight_fwd(cap.weights, cap.gradients, cap.albedo, cap.mid_z, cap.rays_o, cap.rays_d, cap.w2b,
                           stack_lights(lights), cap.bg if bg == "capture" else bg, cap.B, outputs=outputs)


def test_coloured_lights_match_restatement():
    from oi_amd import relight as RL
    from oi_amd.relight import stack_lights
    gen, z, b2w = make_gen("f16x3")
    cap = RL.capture(gen, z=z, b2w=b2w, bg=BG)
    lights = coloured_lights(5)
    got = _kernel(cap, lights)
    ref = relight_ref(cap.weights, cap.gradients, cap.albedo, cap.mid_z, cap.rays_o, cap.rays_d, cap.w2b,
                      stack_lights(lights), cap.bg, cap.B)
    for k in KERNEL_OUT:
        err = maxdiff(got[k], ref[k])
        record_margin("relight_coloured_vs_fp64", k, err)
        assert err < BAR, (k, err)
    # the public maps are these outputs in (L, B, 3, H, W)
    out = RL.relight(cap, lights, outputs=("image", "diff_shading_map"))
    assert torch.equal(out["image"], got["image"].view(5, 2, 3, 16, 16))
    assert torch.equal(out["diff_shading_map"], got["diffuse"].view(5, 2, 3, 16, 16))


@pytest.mark.parametrize("outputs", [KERNEL_OUT, ("image",)])
def test_batch_invariance_and_determinism(outputs):
    from oi_amd import relight as RL
    gen, z, b2w = make_gen("f16x3")
    cap = RL.capture(gen, z=z, b2w=b2w, bg=BG)
    lights = coloured_lights(7, seed=1)
    a = _kernel(cap, lights, outputs)
    b = _kernel(cap, lights, outputs)
    for k in outputs:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k   # byte-identical runs
    for i, lt in enumerate(lights):
        one = _kernel(cap, [lt], outputs)
        for k in outputs:
            assert torch.equal(one[k][0].view(torch.int32), a[k][i].view(torch.int32)), (i, k)


def _synthetic(B, hw, T, seed):
    g = torch.Generator().manual_seed(seed)
    N = B * hw
    w = torch.rand(N, T, generator=g) / T
    rot = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    w2b = torch.zeros(B, 4, 4)
    w2b[:, :3, :3] = rot
    w2b[:, 3, 3] = 1.0
    return {"weights": w, "grad": torch.randn(N, T, 3, generator=g), "rgb": torch.rand(N, T, 3, generator=g),
            "mid_z": 2.0 + 2.0 * torch.rand(N, T, generator=g), "rays_o": torch.randn(N, 3, generator=g) * 0.1 + torch.tensor([0, 0, -4.0]),
            "rays_d": torch.nn.functional.normalize(torch.randn(N, 3, generator=g) * 0.2 + torch.tensor([0, 0, 1.0]), dim=-1),
            "w2b": w2b, "bg": torch.rand(B, 3, generator=g)}


LIMIT_CASES = ([(T, B, L, KERNEL_OUT, True) for T in (1, 63, 64, 65, 320, 400, 1600, 2049) for B in (1, 3) for L in (1, 256)] +
               [(T, 3, 5, tuple(o for o in KERNEL_OUT if o != drop), True) for T in (65, 2049) for drop in KERNEL_OUT] +
               [(T, 3, 5, KERNEL_OUT, False) for T in (65, 2049)] +
               [(T, 1, 9, ("image", "image_no_bg"), True) for T in (65, 2049)])


@pytest.mark.parametrize("T,B,L,outputs,with_bg", LIMIT_CASES)
def test_guarded_limit_shapes(T, B, L, outputs, with_bg):
    """Guarded inputs and outputs (the fixture checks at teardown): no store outside a buffer, every element of every
    requested output written, no input modified.  hw = 5 or 13 rays per element: never a multiple of the rays per block."""
    from oi_amd import ops
    from oi_amd.relight import stack_lights
    hw = 13 if B == 1 else 5
    s = {k: v.cuda() for k, v in _synthetic(B, hw, T, seed=T * 7 + B).items()}
    lights = stack_lights(coloured_lights(L, seed=L))
    ins = {k: guarded_copy(v, what=k) for k, v in s.items()}
    lt = guarded_copy(lights, what="lights")
    bg = ins["bg"] if with_bg else None
    got = ops.relight_fwd(ins["weights"], ins["grad"], ins["rgb"], ins["mid_z"], ins["rays_o"], ins["rays_d"], ins["w2b"], lt,
                          bg, B, outputs=outputs)
    assert set(got) == set(outputs)
    ref = relight_ref(s["weights"], s["grad"], s["rgb"], s["mid_z"], s["rays_o"], s["rays_d"], s["w2b"], lights,
                      s["bg"] if with_bg else None, B)
    for k in outputs:
        assert got[k].shape == (L, B, 3, hw)
        err = maxdiff(got[k], ref[k])
        record_margin("relight_limit_shapes", k, err)
        assert err < BAR, (T, B, L, k, err)


def test_light_walk():
    from oi_amd import inference
    from oi_amd import relight as RL
    gen, z, b2w = make_gen("f16x3")
    cap = RL.capture(gen, z=z[:1], b2w=b2w[:1])
    frames = inference.light_walk(gen, z[0], b2w[0], n_frames=3, keys=("image", "mask", "normal_map", "specular_map"))
    for k, c in (("image", 3), ("mask", 1), ("normal_map", 3), ("specular_map", 3)):
        assert frames[k].shape == (3, c, 16, 16), (k, frames[k].shape)
    err = maxdiff(frames["image"][0], cap.render_out["image"][0])
    record_margin("light_walk_frame0", "image", err)
    assert err < BAR, err
    for i in (1, 2):
        assert torch.equal(frames["mask"][i], frames["mask"][0])
        assert torch.equal(frames["normal_map"][i], frames["normal_map"][0])
        assert float((frames["image"][i] - frames["image"][0]).abs().max()) > 1e-3, i


def test_invalid_arguments_raise_before_launch():
    from oi_amd import lib, ops
    from oi_amd.relight import Light, stack_lights
    with pytest.raises(ValueError):
        Light(direction=(0.0, 0.0, 0.0))
    s = {k: v.cuda() for k, v in _synthetic(2, 5, 8, seed=0).items()}
    lights = stack_lights(coloured_lights(2))
    with pytest.raises(ValueError):   # N = 10 rays over B = 3 elements
        ops.relight_fwd(s["weights"], s["grad"], s["rgb"], s["mid_z"], s["rays_o"], s["rays_d"], s["w2b"], lights, None, 3)
    with pytest.raises(ValueError):   # L = 0
        ops.relight_fwd(s["weights"], s["grad"], s["rgb"], s["mid_z"], s["rays_o"], s["rays_d"], s["w2b"], lights[:0], None, 2)
    # the C entry itself: OI_ERR_INVALID_ARG, and the output is left as it was (no launch)
    L = lib.load()
    sentinel = torch.full((2, 2, 3, 5), 123.0, device="cuda")
    for kw in (dict(B=3), dict(L=0), dict(T=0)):
        P = lib.RelightParams()
        for n in ("weights", "grad", "rgb", "mid_z", "rays_o", "rays_d", "w2b"):
            setattr(P, n, ctypes.c_void_p(s[n].data_ptr()))
        P.lights, P.image = ctypes.c_void_p(lights.data_ptr()), ctypes.c_void_p(sentinel.data_ptr())
        P.N, P.T, P.B, P.L = 10, 8, 2, 2
        for k, v in kw.items():
            setattr(P, k, v)
        assert L.oi_relight_fwd(ctypes.byref(P), ops._stream()) == -1, kw
        assert L.oi_last_error().decode().startswith("oi_relight_fwd"), kw
    torch.cuda.synchronize()
    assert bool((sentinel == 123.0).all())
