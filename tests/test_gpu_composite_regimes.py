"""oi_composite_fwd / oi_composite_bwd (csrc/render.hip, csrc/render_bwd.hip) against the float64 restatement of
tests/helpers/composite_regimes.py in the regimes training reaches: saturated sigmoids, the alpha clips, the mask window,
the inv_s clamp, a switched-off specular term, shininess <= 1, true_cos across both relu kinks, degenerate gradients.

Inputs, reference, margins to the kinks and the fp32 floors are rehearsed on the CPU by tests/test_composite_regimes_cpu.py.
Every bar is the larger of the bar the project already holds the quantity to and 3x the committed fp32 floor of that regime
and tensor (`R.bar`); every error is max |a - ref| / max(1, max |ref|) (`R.rel_err`) and is reported through record_margin
under composite_regimes[<regime>]."""
import ctypes

import pytest
import torch

from conftest import record_margin
from helpers import composite_regimes as R
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]
NAMES = tuple(R.REGIMES)


def _check(case, name, tensor, got, ref, single=None):
    err = R.rel_err(got, ref)
    b, why = R.bar(name, tensor, single)
    record_margin(case, tensor if single is None else f"{single}: {tensor}", err)
    print(f"  {case} {'' if single is None else single + ': '}{tensor:14s} error {err:.3e}  bar {b:.3e} ({why})")
    assert bool(torch.isfinite(got).all()), (case, single, tensor)
    return None if err <= b else (tensor, err, b)


def _device_leaves(inp):
    c = lambda t: t.float().cuda().requires_grad_(True)
    return [c(inp["sdf"]), c(inp["grad"]), c(inp["rgb"]), c(inp["variance"]), c(inp["light"][0]), c(inp["light"][1]),
            c(inp["light"][2]), c(inp["direction"])]


def _run(inp, lv):
    from oi_amd.autograd_render import CompositeFunction
    light = torch.stack([lv[4], lv[5], lv[6]])
    dirn = lv[7] / torch.linalg.norm(lv[7])
    ldir = torch.einsum("bij,j->bi", inp["w2b"].cuda()[:, :3, :3], dirn)
    bg = None if inp["bg"] is None else inp["bg"].cuda()
    return CompositeFunction.run(lv[0], lv[1], lv[2], inp["dists"].cuda(), inp["mid_z"].cuda(), inp["rays_o"].cuda(),
                                 inp["rays_d"].cuda(), ldir, bg, lv[3], light, inp["car"], R.B)


def _kernel_grads(inp, single=None):
    lv = _device_leaves(inp)
    out = _run(inp, lv)
    g = torch.autograd.grad(R.loss_of(out, inp["cot"], single), lv, allow_unused=True)
    grads = {k: (torch.zeros_like(l) if t is None else t) for k, l, t in zip(R.GRADS, lv, g)}
    return out, grads


@pytest.mark.parametrize("name", NAMES)
def test_forward(name):
    from oi_amd import ops
    inp, ref, _ = R.case(name)
    case = f"composite_regimes[{name}]"
    c = lambda t: None if t is None else t.float().cuda()
    dirn = inp["direction"] / torch.linalg.norm(inp["direction"])
    ldir = torch.einsum("bij,j->bi", inp["w2b"][:, :3, :3], dirn)
    out = ops.composite_fwd(c(inp["sdf"]), c(inp["grad"]), c(inp["rgb"]), c(inp["dists"]), c(inp["mid_z"]), c(inp["rays_o"]),
                            c(inp["rays_d"]), c(ldir), c(inp["bg"]), c(inp["variance"]), c(inp["light"]), inp["car"], R.B)
    print()
    want = R.flat_outputs(ref)
    got = {k: out[k] for k in R.PER_SAMPLE + tuple(R.MAPS)}
    got.update({k: out["reduce4"][j] for j, k in enumerate(R.REDUCE)})
    missed = [m for m in (_check(case, name, k, got[k], want[k]) for k in want) if m]
    assert not missed, missed
    assert torch.equal(out["inside_sphere"].cpu().double(), ref["inside_sphere"])
    if name == "no_bg":   # bg == NULL: nothing is added to the image
        assert torch.equal(out["image"], out["image_no_bg"])


@pytest.mark.parametrize("name", NAMES)
def test_backward_all_cotangents(name):
    """Random cotangents on the 11 differentiable outputs plus weights on reduce4[0..2] (the eikonal sum, the mask count, the
    surface sum: the surface loss has no other gradient test)."""
    inp, _, ref = R.case(name)
    case = f"composite_regimes[{name}]"
    _, grads = _kernel_grads(inp)
    print()
    got, want = R.grad_tensors(inp, grads), R.grad_tensors(inp, ref)
    missed = [m for m in (_check(case, name, k, got[k], want[k]) for k in R.GRAD_TENSORS) if m]
    assert not missed, missed
    if name in ("clamped_hi", "clamped_lo"):   # inv_s sits on its clamp: it does not move with the variance
        assert float(grads["variance"]) == 0.0
    if name in ("no_specular", "zero_specular"):   # specular colour = max(param_specular, 0) is switched off
        assert float(grads["specular"]) == 0.0


@pytest.mark.parametrize("single", R.SINGLE_CASES)
@pytest.mark.parametrize("name", R.SINGLE_REGIMES)
def test_backward_one_cotangent(name, single):
    """One upstream gradient of oi_composite_grads non-NULL at a time (then one entry of g_reduce4 at a time): every term of
    the backward against the float64 gradient of that term alone, each with its own relative error."""
    inp = R.case(name)[0]
    ref = R.single_reference(name, single)
    case = f"composite_regimes[{name}]"
    _, grads = _kernel_grads(inp, single)
    print()
    got, want = R.grad_tensors(inp, grads), R.grad_tensors(inp, ref)
    missed = [m for m in (_check(case, name, k, got[k], want[k], single) for k in R.GRAD_TENSORS) if m]
    assert not missed, missed
    if single == "mask":   # clamp(W, 1e-3, 1 - 1e-3): rays outside the window take no gradient at all
        q = R.deciding(inp)
        outside = (~((q["W"] > 1e-3) & (q["W"] < 1 - 1e-3))).cuda()
        assert bool(outside.any())
        assert not bool(grads["sdf"][outside].any()) and not bool(grads["grad"][outside].any())


def test_backward_both_reduction_paths(guarded_ops):
    """oi_composite_bwd with ray_partials (per-ray partials + the reduce kernel: what ops.composite_bwd passes) and with
    ray_partials == NULL (wave -> block -> atomics), on `trained`: the per-sample gradients are the same bits, the scalar
    gradients meet their bars on both."""
    from oi_amd import lib, ops
    name = "trained"
    inp, _, ref = R.case(name)
    gs = guarded_ops
    L = lib.load()
    c = lambda t: gs.copy(t.float().contiguous().cuda(), "input")
    dirn = inp["direction"] / torch.linalg.norm(inp["direction"])
    ldir = torch.nn.functional.normalize(torch.einsum("bij,j->bi", inp["w2b"][:, :3, :3], dirn), dim=-1)
    P = lib.CompositeParams()
    keep = []
    for k, t in (("sdf", inp["sdf"]), ("grad", inp["grad"]), ("rgb", inp["rgb"]), ("dists", inp["dists"]), ("mid_z", inp["mid_z"]),
                 ("rays_o", inp["rays_o"]), ("rays_d", inp["rays_d"]), ("light_dir", ldir), ("bg", inp["bg"]),
                 ("variance", inp["variance"].reshape(1)), ("light", inp["light"])):
        keep.append(c(t))
        setattr(P, k, ctypes.c_void_p(keep[-1].data_ptr()))
    P.cos_anneal_ratio, P.N, P.T, P.B, P.image_planar = float(inp["car"]), R.N, R.T, R.B, 0
    cot = dict(inp["cot"], reduce4=torch.tensor(R.REDUCE_WEIGHTS + (0.0,)))
    res = {}
    for path in ("partials", "atomics"):
        G = lib.CompositeGrads()
        for k in ops.GRAD_IN:
            keep.append(c(cot[k]))
            setattr(G, "g_" + k, ctypes.c_void_p(keep[-1].data_ptr()))
        o = {"d_sdf": gs.empty((R.N, R.T), what=f"{path} d_sdf"), "d_grad": gs.empty((R.N, R.T, 3), what=f"{path} d_grad"),
             "d_rgb": gs.empty((R.N, R.T, 3), what=f"{path} d_rgb"), "d_variance": gs.zeros((1,), what=f"{path} d_variance"),
             "d_light": gs.zeros((3,), what=f"{path} d_light"), "d_light_dir": gs.zeros((R.B, 3), what=f"{path} d_light_dir")}
        for k, t in o.items():
            setattr(G, k, ctypes.c_void_p(t.data_ptr()))
        if path == "partials":
            o["ray_partials"] = gs.empty((R.N, 8), what="ray_partials")
            G.ray_partials = ctypes.c_void_p(o["ray_partials"].data_ptr())
        lib.check(L.oi_composite_bwd(ctypes.byref(P), ctypes.byref(G), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "oi_composite_bwd")
        res[path] = o
    a, b = res["partials"], res["atomics"]
    for k in ("d_sdf", "d_grad", "d_rgb"):
        assert torch.equal(a[k], b[k]), k
    # d_light_dir is the gradient on the UNIT direction of each element; the Jacobian of direction -> w2b direction / |.|
    # is autograd's (as in CompositeFunction.run)
    d = inp["direction"].double().clone().requires_grad_(True)
    u = torch.nn.functional.normalize(torch.einsum("bij,j->bi", inp["w2b"].double()[:, :3, :3], d / torch.linalg.norm(d)), dim=-1)
    print()
    missed = []
    for path, o in res.items():
        (d_dir,) = torch.autograd.grad(u, d, o["d_light_dir"].double().cpu(), retain_graph=True)
        got = {"d_variance": o["d_variance"][0], "d_ambient": o["d_light"][0], "d_specular": o["d_light"][1],
               "d_shininess": o["d_light"][2], "d_direction": d_dir}
        for k, v in got.items():
            m = _check(f"composite_regimes[{name}]", name, k, v, ref[k[2:]], single=None)
            if m:
                missed.append((path,) + m)
    assert not missed, missed
