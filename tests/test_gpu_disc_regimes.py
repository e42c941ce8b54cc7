"""The discriminator's four forward implementations (csrc/disc_small.hip, the fp32 split-K and the LDS-tiled F16X3 kernels of
csrc/disc.hip, csrc/disc_large.hip) and the pre-activation chain's input gradient against the float64 chain of
tests/helpers/disc_regimes.py, in every regime: unit scale (all the suite tested so far), nn.Conv2d's own initialisation, white
backgrounds, binary masks, dark images, shrunk and grown weights, and activations beyond the fp16 range.

Inputs, references, fp32 floors, the limb model, the bars (3 x floor for the fp32 routes, 3 x (model + floor) for the limb
routes) and the rule for `overflow` are rehearsed on the CPU by tests/test_disc_regimes_cpu.py, which also shows that each
plausible kernel error fails the assertions made here (`R.judge`).  Every measured error goes through record_margin under
disc_regimes[<route>][<regime>] (profiles/disc_regimes_margins.txt)."""
import pytest
import torch

from conftest import record_margin
from helpers import disc_regimes as R
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

NET_ROUTES = ("small_b1", "small_b4", "arena_b5", "arena_b32", "large_b16", "pre_b2", "pre_b32")
NET_CASES = ([(n, r) for n in R.NET64 for r in NET_ROUTES] + [(n, "small_b1") for n in ("unit_128", "default_init_128")]
             + [("overflow", r) for r in ("arena_b32", "pre_b32", "large_b16")])
_NETS = {}


def _report(route, name, outputs):
    case = f"disc_regimes[{route}][{name}]"
    kind = R.ROUTES[route]["kind"]
    print()
    for key, e in R.errors(route, name, outputs).items():
        record_margin(case, key, e)
        model = 0.0 if kind == "fp32" or key in ("dx", "logits_over") else R.LIMB_MODEL[kind][name][key]
        print(f"  {case} {key:13s} error {e:.3e}  floor {R.FP32_FLOOR[name][key]:.3e}  model {model:.3e}  bar {R.bar(route, name, key):.3e}")
    bad = R.judge(route, name, outputs)
    assert not bad, bad


@pytest.mark.parametrize("route", R.LAYER_ROUTES)
@pytest.mark.parametrize("name", R.NET64)
def test_layer(guarded_ops, name, route):
    """One block through ops.conv4x4_fwd, fed with the float32 chain's sums of its predecessor, with the LeakyReLU on load
    (x_slope 0.2) and without (1.0)."""
    from oi_amd import ops
    c, r = R.case(name), R.ROUTES[route]
    B, layer, any_scale = r["B"], r["layer"], r.get("any_scale", False)
    w, stride, pad = R._layers(c["wsd"])[layer]
    # (tests/test_disc_regimes_cpu.py: this batch is the smallest at which oi_conv4x4_fwd_arena's conditions select the kernel)
    assert R.tiled_launch(B, *R.block_shape(c["spec"]["in_dim"], layer), any_scale=any_scale) == r["launch"]
    wd = guarded_ops.copy(w.cuda(), "input")
    outputs = {}
    for s in (1.0, R.SLOPE):
        key = f"L{layer}/{s}"
        x = guarded_ops.copy(R.batch_of(c["inp"][key], B).cuda(), "input")
        y = ops.conv4x4_fwd(x, wd, None, stride, pad, 1.0, x_slope=s, any_scale=any_scale)
        if r["launch"] is not None:   # K never split, or two halves into zeros: the same bits on every call
            assert torch.equal(y, ops.conv4x4_fwd(x, wd, None, stride, pad, 1.0, x_slope=s, any_scale=any_scale)), key
        outputs[key] = y[R.compare(B)]
    _report(route, name, outputs)


def _net(name):
    if name not in _NETS:
        from oi_amd.discriminator import DCDiscriminator
        c = R.case(name)
        s = c["spec"]
        D = DCDiscriminator(in_dim=s["in_dim"], out_dim=s["out_dim"], n_feat=512, img_size=s["size"]).cuda()
        D.load_state_dict(c["wsd"])
        _NETS[name] = D
    return _NETS[name]


@pytest.mark.parametrize("name,route", NET_CASES)
def test_network(guarded_ops, name, route):
    """The whole network through DCDiscriminator.forward on the route the batch and the grad mode select."""
    import oi_amd.discriminator as DM
    c, B = R.case(name), R.ROUTES[route]["B"]
    D = _net(name)
    x = R.batch_of(c["x"], B).cuda()
    want = route.split("_")[0]
    grad = want == "pre"
    outputs = {}
    large_was = DM.LARGE_PATH
    try:
        DM.LARGE_PATH = want == "large"
        with torch.set_grad_enabled(grad):
            x.requires_grad_(grad)
            assert DM.route(**D._facts(x))[1] == want, route
            if want == "large":
                assert D._forward_large(x) is not None   # (the pack covers the network: no quiet general chain)
            d = D(x)
            if route == "pre_b2":
                outputs["dx"], = torch.autograd.grad(d[:, :1].sum(), x)
    finally:
        DM.LARGE_PATH = large_was
    assert tuple(d.shape) == (B, c["spec"]["out_dim"])
    outputs["logits"] = d.detach()[R.compare(B)]
    if name == "overflow":
        over = c["over"][R.ROUTES[route]["kind"]][torch.tensor(R.compare(B)) % R.POOL]
        print(f"\n  overflow {route}: images above 65504 {over.tolist()}, finite logits per image {torch.isfinite(outputs['logits']).sum(1).tolist()}")
    _report(route, name, outputs)
