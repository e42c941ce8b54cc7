"""The discriminator's backward kernels (csrc/disc_bwd.hip) and their composition (oi_amd/autograd_conv.py, the R1 double
backward, the one-pass and the two-pass discriminator step under ops.GradSink) against float64, in the regimes of
tests/helpers/disc_regimes.py: nn.Conv2d-initialised, grown and shrunk weights, white backgrounds, binary masks with exactly
zero pre-activations, dark images.

Operands, references, launch plans, fp32 floors and bars (3 x floor) come from tests/helpers/disc_bwd_regimes.py and are
rehearsed on the CPU by tests/test_disc_bwd_regimes_cpu.py, which also shows that each plausible kernel error is more than
3 x bar away.  Every measured error goes through record_margin under disc_bwd_regimes[<route>][<regime>] (DESIGN.md section
4.8 / 5, profiles/disc_bwd_regimes_margins.txt)."""
import pytest
import torch

from conftest import record_margin
from helpers import disc_bwd_regimes as Q
from helpers import disc_regimes as R
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

LAYER_CASES = [(n, r) for n in Q.NAMES for r in Q.routes_of(n)]
PLAIN = ("k1", "lds_store")   # one store (or one add into zeros) per element: the same bits on every call
_NETS = {}


def _report(route, name, errors):
    case = f"disc_bwd_regimes[{route}][{name}]"
    print()
    for key, e in errors.items():
        record_margin(case, key.split("/", 1)[1] if route != "net" else key, e)
        print(f"  {case} {key:28s} error {e:.3e}  floor {Q.FP32_FLOOR_BWD[name][key]:.3e}  bar {Q.bar(name, key):.3e}")
    return Q.judge(name, errors)


def _worst(a, b):
    return {k: max(v, b.get(k, 0.0)) for k, v in a.items()}


@pytest.mark.parametrize("name,route", LAYER_CASES)
def test_layer(guarded_ops, name, route):
    """One layer's backward on the float32 chain's data: mask on load, lrelu'(x) on output, x_slope on load, the fused launch,
    every weight gradient fresh and added into a prefilled accumulator."""
    from oi_amd import ops
    r, o = Q.LAYER_ROUTES[route], Q.layer_case(name, route)["o"]
    dp, wp = Q.plans(name, route)
    assert (dp["k_splits"], dp["cls"]) == r["dgrad"] and (wp["k_splits"], wp["cls"]) == r["wgrad"]
    x, ref, w, g = (guarded_ops.copy(o[k].cuda(), k) for k in ("x", "ref", "w", "g"))
    stride, pad, H = o["stride"], o["pad"], o["x"].shape[2]

    def prefilled(key):
        acc = guarded_ops.zeros(w.shape, what=f"acc {key}")
        acc.copy_(o["acc"][key])
        return acc

    def run():
        out = {"dgrad_m": ops.conv4x4_dgrad(g, w, H, H, stride, pad, mask_ref=ref, slope=Q.SLOPE),
               "dgrad_pre": ops.conv4x4_dgrad_pre(g, w, x, Q.SLOPE, stride, pad),
               "wgrad_m": ops.conv4x4_wgrad(g, x, stride, pad, mask_ref=ref, slope=Q.SLOPE)}
        acc = prefilled("wgrad_m")
        assert ops.conv4x4_wgrad(g, x, stride, pad, mask_ref=ref, slope=Q.SLOPE, acc=acc) is acc
        out["wgrad_m+acc"] = acc
        out["bwd_dx"], out["bwd_gw"] = ops.conv4x4_bwd(g, w, x, stride, pad, x_slope=Q.SLOPE)
        acc = prefilled("bwd_gw")
        dx2, gw2 = ops.conv4x4_bwd(g, w, x, stride, pad, acc=acc, x_slope=Q.SLOPE)
        assert gw2 is acc
        out["bwd_gw+acc"] = acc
        return out, dx2

    out, dx2 = run()
    errors = _worst(Q.layer_errors(name, route, out), Q.layer_errors(name, route, {"bwd_dx": dx2}))
    again, _ = run()
    same = [k for k in ("dgrad_m", "dgrad_pre", "bwd_dx") if dp["cls"] in PLAIN]
    same += [k for k in ("wgrad_m", "bwd_gw") if wp["cls"] in PLAIN] + [k for k in ("wgrad_m+acc", "bwd_gw+acc") if wp["cls"] == "k1"]
    for k in same:
        assert torch.equal(out[k], again[k]), f"{k}: a second call differs ({dp['cls']} / {wp['cls']})"
    v, rf, want = Q.layer_mask_mul(name, route)
    assert torch.equal(ops.lrelu_mask_mul(g, ref, Q.SLOPE).cpu(), want), "lrelu_mask_mul: not ref > 0 ? v : 0.2 v to the bit"
    bad = _report(route, name, errors)
    assert not bad, bad


def _net(name):
    if name not in _NETS:
        from oi_amd.discriminator import DCDiscriminator
        c = R.case(name)
        s = c["spec"]
        D = DCDiscriminator(in_dim=s["in_dim"], out_dim=s["out_dim"], n_feat=512, img_size=s["size"]).cuda()
        D.load_state_dict(c["wsd"])
        _NETS[name] = D
    return _NETS[name]


def _sign_report(name, idx):
    """The GPU's pre-activations of pool images `idx`, layer by layer (ops.conv4x4_fwd fed with its own sums): where a sign
    differs from the float64 chain's, a failure is a flipped kink and not a wrong gradient kernel."""
    from oi_amd import ops
    c = R.case(name)
    a, s, lines = c["x"][idx].cuda(), 1.0, []
    for l, (w, stride, pad) in enumerate(R._layers(c["wsd"])[:-1]):
        a = ops.conv4x4_fwd(a, w.cuda(), None, stride, pad, 1.0, x_slope=s, any_scale=True)
        s = Q.SLOPE
        u64 = c["u64"][l][idx]
        n = int((torch.sign(a.cpu().double()) != torch.sign(u64)).sum())
        lines.append(f"block {l}: {n} of {u64.numel()} signs differ from the float64 chain")
    return lines


@pytest.mark.parametrize("name", Q.NAMES)
def test_network(guarded_ops, name):
    """DCDiscriminator with the regime's weights on its clean images: d <c, D(x)> / dW, dR1 / dW (grad_wrt_input + autograd)
    and the discriminator step's weight gradients in the one-pass [real; fake] and the two-pass form, both under ops.GradSink
    into zeroed accumulators as GraphedDStep._backward runs them -- every parameter against float64."""
    import oi_amd.discriminator as DM
    from oi_amd import ops
    from oi_amd.losses import gan_losses, gan_losses_cat, grad_wrt_input
    c = R.case(name)
    real, fake = Q.batch(name)
    B, idx = len(real), list(real) + list(fake)
    D = _net(name)
    names = [k for k, _ in D.named_parameters()]
    params = [p for _, p in D.named_parameters()]
    assert names == list(c["wsd"])
    xr, xf = c["x"][list(real)].cuda(), c["x"][list(fake)].cuda()
    one = torch.ones((), device="cuda")
    errors = {}

    def sunk(loss):
        """The plain backward of a step: every weight's contributions added in place into a zeroed accumulator."""
        for p in params:
            p.grad = None
        sink = {p.data_ptr(): guarded_ops.zeros(p.shape, what="sink") for p in params}
        with ops.GradSink(sink):
            torch.autograd.backward(loss, grad_tensors=one, inputs=params)
        assert all(p.grad is None for p in params), "a convolution weight received a gradient outside the sink"
        return {k: sink[p.data_ptr()] for k, p in zip(names, params)}

    with torch.enable_grad():
        x = xr.clone().requires_grad_()
        assert DM.route(**D._facts(x))[1] == "pre"
        d = D(x)
        errors.update(Q.net_errors(name, "gw_plain", dict(zip(names, torch.autograd.grad(d, params, Q.cotangent(name).cuda())))))

        x = xr.clone().requires_grad_()
        gx = grad_wrt_input(D(x)[:, :1], x)
        r1 = gx.pow(2).reshape(B, -1).sum(1).mean()
        errors.update(Q.net_errors(name, "gw_r1", dict(zip(names, torch.autograd.grad(r1, params)))))

        # one pass over [real; fake], the selection cotangent keeps the fake half out of R1 (GraphedDStep._losses_cat)
        x = torch.cat([xr, xf]).requires_grad_()
        d = D(x)
        sel = torch.zeros_like(d)
        sel[:B, 0] = 1.0
        gx = grad_wrt_input(d, x, sel)
        assert not bool(gx[B:].any()), "the fake half has an R1 gradient"
        loss, _ = gan_losses_cat(d, B, None, gx, None, Q.REG_W)
        step_cat = Q.net_errors(name, "step", sunk(loss))

        # two passes (GraphedDStep._step_ops)
        x = xr.clone().requires_grad_()
        d_fake, d_real = D(xf), D(x)
        gx = grad_wrt_input(d_real[:, :1], x)
        loss, _ = gan_losses(d_real, d_fake, None, gx, None, Q.REG_W)
        step_two = Q.net_errors(name, "step", sunk(loss))
    for p in params:
        p.grad = None
    print(f"\n  {name}: step, one pass {({k: float(f'{v:.3g}') for k, v in step_cat.items()})}\n  two passes {({k: float(f'{v:.3g}') for k, v in step_two.items()})}")
    errors.update(_worst(step_cat, step_two))
    bad = _report("net", name, errors)
    if bad:
        bad += _sign_report(name, idx)
    assert not bad, bad
