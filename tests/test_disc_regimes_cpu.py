"""The rehearsal of tests/test_gpu_disc_regimes.py on the oracle alone (no GPU): the float64 chain of
tests/helpers/disc_regimes.py is the oracle, every regime is what its name says, the committed fp32 floors and limb-model
errors -- from which every bar of the GPU test follows -- are what a fresh computation gives, the regimes called "inside the
envelope" keep the project's forward bar relative to the rms of the logits and `dark` / `shrunk` do not, and every plausible
error of a limb kernel fails the assertions the GPU test makes (`R.judge`) in the regimes CAUGHT_BY names."""
import math

import pytest
import torch

import oi_oracle as O
from helpers import disc_regimes as R

NAMES = tuple(R.REGIMES)
ENVELOPE = tuple(n for n in R.NET64 if R.REGIMES[n]["envelope"])
FORWARD_BAR = 2e-5   # the project's forward bar (tests/test_gpu_modules.py), here relative to the rms of the reference


def _same_to_the_last_digit(fresh, committed):
    """Both printed as d.dde-xx: at most one unit of the last digit apart."""
    return abs(fresh - committed) <= 10.0 ** (math.floor(math.log10(committed)) - 2) * 1.0001


def test_layout_is_the_issue_s():
    assert set(R.FP32_FLOOR) == set(R.REGIMES) and set(R.LIMB_MODEL) == {"tiled", "large"}
    for kind in R.LIMB_MODEL:
        assert set(R.LIMB_MODEL[kind]) == set(R.NET64) | {"overflow"}
    assert ENVELOPE == ("unit", "default_init", "white_bg", "mask", "grown3", "grown8")
    assert [n for n in R.NET64 if R.REGIMES[n]["envelope"] is False] == ["dark", "shrunk"] and R.REGIMES["overflow"]["envelope"] is None
    assert (R.REGIMES["mask"]["in_dim"], R.REGIMES["mask"]["out_dim"]) == (1, 1)
    assert all((R.REGIMES[n]["in_dim"], R.REGIMES[n]["out_dim"]) == (3, 7) for n in NAMES if n != "mask")
    assert set(R.CAUGHT_BY) | set(R.NOT_DETECTABLE) == set(R.MUTATIONS) and not set(R.CAUGHT_BY) & set(R.NOT_DETECTABLE)
    assert len(R.NOT_DETECTABLE) <= 2 and not {"drop_xl_wh", "drop_xh_wl", "flush_lo"} & set(R.NOT_DETECTABLE)
    # three DIFFERENT pool images are compared at every batch a route uses
    for r in R.ROUTES.values():
        idx = [i % R.POOL for i in R.compare(r["B"])]
        assert len(set(idx)) == len(idx), r


def test_batches_are_the_first_that_select_each_kernel():
    """The batches of the GPU test against oi_conv4x4_fwd_arena's conditions (R.tiled_launch restates them)."""
    shape = lambda layer, in_dim=3: R.block_shape(in_dim, layer)
    for route in R.LAYER_ROUTES:
        r = R.ROUTES[route]
        assert R.tiled_launch(r["B"], *shape(r["layer"]), any_scale=r.get("any_scale", False)) == r["launch"], route
        assert (r["launch"] is None) == (r["kind"] == "fp32")
    assert {R.ROUTES[r]["launch"] for r in R.LAYER_ROUTES} == {(64, 2), (64, 1), (128, 1), None}
    # block 1 reaches the tiled kernel at batch 8, blocks 2 and 3 at 16 and 32, and not before; the first block and the head never
    for layer, first in ((1, 8), (2, 16), (3, 32)):
        assert all(R.tiled_launch(b, *shape(layer)) is None for b in range(1, first)) and R.tiled_launch(first, *shape(layer))
    for in_dim in (1, 3):
        assert all(R.tiled_launch(b, in_dim, 64, 64) is None for b in (5, 32, 64))
    assert all(R.tiled_launch(b, 512, 4, o, stride=1, pad=0) is None for b in (32, 64) for o in (1, 7))
    # the chains: every block on the fp32 kernel at batch 2 and 5 (either in_dim), blocks 1-3 on the tiled one at 32
    assert all(R.tiled_launch(b, *shape(l)) is None for b in (2, 5) for l in (1, 2, 3))
    assert all(R.tiled_launch(32, *shape(l)) for l in (1, 2, 3))
    assert R.ROUTES["arena_b32"]["kind"] == R.ROUTES["pre_b32"]["kind"] == "tiled"
    assert all(R.ROUTES[r]["kind"] == "fp32" for r in ("small_b1", "small_b4", "arena_b5", "pre_b2"))


@pytest.mark.parametrize("name", NAMES)
def test_float64_chain_is_the_oracle(name):
    c = R.case(name)
    dsd = {k: v.double() for k, v in c["wsd"].items()}
    assert torch.equal(c["u64"][-1].reshape(c["x"].shape[0], -1), O.dc_discriminator(dsd, c["x"].double()))
    assert all(u.dtype == torch.float32 for u in c["u32"]) and len(c["u64"]) == len(c["wsd"])
    # deterministic: a second build gives the same bits
    again = R.ref32(c["wsd"], c["x"])
    assert all(torch.equal(a, b) for a, b in zip(again, c["u32"]))


def test_limb_model_at_unit_scale_is_fp32_class():
    """The "22 bits" of the sources: at `unit` the two-limb arithmetic is within 4x the fp32 floor, layer by layer and for
    the logits of either route."""
    fl = R.measure_floor("unit")
    print()
    for kind in ("tiled", "large"):
        for k, v in R.measure_model("unit", kind).items():
            print(f"  unit {kind:5s} {k:7s} model {v:.2e}  floor {fl[k]:.2e}  ratio {v / fl[k]:.1f}")
            assert v <= 4 * fl[k], (kind, k, v, fl[k])


@pytest.mark.parametrize("name", NAMES)
def test_tables_are_the_committed_ones(name):
    """A fresh computation of the floors and the model errors equals the committed tables to the last printed digit; the
    float32 chain and the models themselves pass every assertion of the GPU test."""
    fresh = R.measure_floor(name)
    assert set(fresh) == set(R.FP32_FLOOR[name])
    print()
    for k, v in fresh.items():
        print(f"  {name} {k:13s} fp32 floor {v:.3e}  committed {R.FP32_FLOOR[name][k]:.2e}")
        assert _same_to_the_last_digit(v, R.FP32_FLOOR[name][k]), (name, k, v)
    if R.REGIMES[name]["size"] != 64:
        return
    for kind in ("tiled", "large"):
        fresh = R.measure_model(name, kind)
        assert set(fresh) == set(R.LIMB_MODEL[kind][name])
        for k, v in fresh.items():
            print(f"  {name} {kind:5s} {k:13s} model {v:.3e}  committed {R.LIMB_MODEL[kind][name][k]:.2e}")
            assert _same_to_the_last_digit(v, R.LIMB_MODEL[kind][name][k]), (name, kind, k, v)


@pytest.mark.parametrize("name", R.NET64 + ("overflow",))
def test_references_pass_the_gpu_test_s_assertions(name):
    c = R.case(name)
    P = c["x"].shape[0]
    for route, r in R.ROUTES.items():
        idx = torch.tensor(R.compare(r["B"])) % P
        if "layer" in r:
            if name == "overflow":
                continue
            for s in (1.0, R.SLOPE):
                key = f"L{r['layer']}/{s}"
                y = R.layer_floor(c, key) if r["kind"] == "fp32" else R.model_outputs(name, "tiled")[key]
                assert R.judge(route, name, {key: y[idx]}) == [], (route, key)
            continue
        if name == "overflow" and r["kind"] == "fp32":
            continue
        lg = c["u32"][-1].reshape(P, -1) if r["kind"] == "fp32" else R.model_outputs(name, r["kind"])["logits"]
        assert R.judge(route, name, {"logits": lg[idx]}) == [], route
    if name != "overflow":
        assert R.judge("pre_b2", name, {"dx": c["dx32"]}) == []


@pytest.mark.parametrize("name", R.NET64 + ("overflow",))
def test_regime_is_what_it_says(name):
    s = R.stats(name)
    c = R.case(name)
    print(f"\n{name}: seed {c['spec']['seed']} gain {c['gain']} {({k: float(f'{v:.3g}') for k, v in s.items()})}")
    lo, hi = {"unit": (1, 10), "default_init": (0.02, 0.3), "white_bg": (0.02, 0.5), "mask": (0.02, 0.3), "dark": (1e-3, 1e-2),
              "shrunk": (1e-3, 1e-2), "grown3": (50, 1e3), "grown8": (3e3, 6e4), "overflow": (R.F16_MAX, 1e8)}[name]
    assert lo < s["head_in_max"] < hi
    if name in ("default_init", "white_bg", "mask", "dark", "shrunk"):
        # nearly every limb operand has a subnormal lo limb; at `unit` most still do (weights of 0.01-0.1), at grown8 a third
        assert s["below_2^-3"] > 0.9 and s["below_3e-4"] > 0.01
    if name in ("dark", "shrunk"):
        assert s["logit_rms"] < 5e-4 and s["below_3e-4"] > 0.03
    if name == "grown8":
        assert s["below_2^-3"] < 0.5
    if name == "white_bg":
        assert 0.78 < s["one_pixels"] < 0.82 and float(c["x"].min()) < -0.99
    if name == "mask":
        x = c["x"]
        assert bool(((x == 0) | (x == 1)).all()) and s["zero_pixels"] >= 0.7 and not bool(x[R.MASK_ZERO_IMAGE].any())
        assert all(bool(x[i].any()) for i in range(x.shape[0]) if i != R.MASK_ZERO_IMAGE)
        # the all-zero image is among the compared ones of the batches 4, 5 and 16
        assert all(R.MASK_ZERO_IMAGE in [i % R.POOL for i in R.compare(B)] for B in (4, 5, 16))
    if name == "overflow":
        t, l = R.limb_carried(c["u32"], c["x"], "tiled"), R.limb_carried(c["u32"], c["x"], "large")
        assert bool((t[0::2] > R.F16_MAX).all()) and bool((l[1::2] < R.F16_MAX).all()) and bool((t <= l).all())
        assert all(bool(torch.isfinite(u).all()) for u in c["u32"])
        # the gain is the smallest of its grid: a step below, some bright image stays inside the fp16 range
        us = R.ref32(R.weights(c["spec"], c["gain"] - 0.25), c["x"])
        assert not bool((R.limb_carried(us, c["x"], "tiled")[0::2] > R.F16_MAX).all())
        for B in (16, 32):   # both populations are among the compared images
            par = {i % R.POOL % 2 for i in R.compare(B)}
            assert par == {0, 1}


@pytest.mark.parametrize("name", R.NET64)
def test_envelope(name):
    """Inside: model + floor <= 2e-5 at the logits of both limb routes (the headroom is printed).  `dark` and `shrunk` are
    outside: the arithmetic itself misses 2e-5 on the route that carries every layer on limbs, and on block 3 of the tiled one."""
    fl = R.FP32_FLOOR[name]
    print()
    for kind in ("tiled", "large"):
        m = R.LIMB_MODEL[kind][name]["logits"]
        print(f"  {name} {kind:5s} logits: model {m:.2e} + floor {fl['logits']:.2e} = {m + fl['logits']:.2e}  ({FORWARD_BAR / (m + fl['logits']):.1f}x headroom)")
        if R.REGIMES[name]["envelope"]:
            assert m + fl["logits"] <= FORWARD_BAR, (name, kind)
    if not R.REGIMES[name]["envelope"]:
        assert R.LIMB_MODEL["large"][name]["logits"] > FORWARD_BAR and R.LIMB_MODEL["tiled"][name][f"L3/{R.SLOPE}"] > FORWARD_BAR


def test_gradient_comparison_keeps_its_cap():
    for name in R.NET64:
        c = R.case(name)
        out = 1.0 - float(c["dx_keep"].double().mean())
        print(f"\n  {name}: {out:.4%} of the input pixels are kink-adjacent")
        assert out <= R.GRAD_CAP and tuple(c["dx_keep"].shape) == (2, 1, 64, 64)
    # the float64 gradient is the oracle's
    c = R.case("unit")
    x = c["x"][:2].double().requires_grad_(True)
    d = O.dc_discriminator({k: v.double() for k, v in c["wsd"].items()}, x)
    g, = torch.autograd.grad(d[:, :1].sum(), x)
    assert torch.equal(g, c["dx64"])


def _caught(mutation, name):
    """The routes on which the mutated model, judged as the GPU output is, breaks an assertion."""
    P = R.case(name)["x"].shape[0]
    hits = []
    for route in ("arena_b32", "large_b16", "L1_b8", "L2_b16", "L3_b32"):
        r = R.ROUTES[route]
        idx = torch.tensor(R.compare(r["B"])) % P
        out = R.model_outputs(name, r["kind"], mutation)
        for key in (("logits",) if "layer" not in r else (f"L{r['layer']}/1.0", f"L{r['layer']}/{R.SLOPE}")):
            if R.judge(route, name, {key: out[key][idx]}):
                hits.append(route if key == "logits" else f"{route}@{key[3:]}")
    return hits


@pytest.mark.parametrize("mutation", tuple(R.CAUGHT_BY))
def test_mutation_is_caught(mutation):
    """Judged exactly as the GPU output is, the mutated model fails on the whole-network routes of BOTH limb kernels in every
    regime CAUGHT_BY names (all of them inside the envelope)."""
    print()
    assert R.CAUGHT_BY[mutation] and set(R.CAUGHT_BY[mutation]) <= set(ENVELOPE)
    for name in R.CAUGHT_BY[mutation]:
        hits = _caught(mutation, name)
        print(f"  {mutation} in {name}: {hits}")
        assert {"arena_b32", "large_b16"} <= set(hits), (mutation, name, hits)


@pytest.mark.parametrize("mutation", tuple(R.NOT_DETECTABLE))
def test_mutation_listed_as_not_detectable_is_caught_nowhere(mutation):
    """(If one of these starts to be caught, it belongs in CAUGHT_BY.)"""
    assert all(not _caught(mutation, name) for name in R.NET64), mutation


def test_overflow_rule_rejects_finite_and_wrong():
    """The rule of `overflow`: the models (inf / -inf limbs) pass; a conversion that SATURATES at 65504 gives finite, wrong logits
    on the bright images and fails; so does a NaN on a dim image."""
    c = R.case("overflow")
    P = c["x"].shape[0]
    for route in ("arena_b32", "pre_b32", "large_b16"):
        r = R.ROUTES[route]
        idx = torch.tensor(R.compare(r["B"])) % P
        lg = R.model_outputs("overflow", r["kind"])["logits"]
        assert not bool(torch.isfinite(lg[0::2]).any()) and bool(torch.isfinite(lg[1::2]).all())
        assert R.judge(route, "overflow", {"logits": lg[idx]}) == []
        # saturating limbs: the chain with every limb-carried value clamped to the fp16 range
        us, a = [], c["x"]
        for i, (w, stride, pad) in enumerate(R._layers(c["wsd"])):
            limb = (0 < i < 4) if r["kind"] == "tiled" else True
            a = R.exact_conv(a.clamp(-R.F16_MAX, R.F16_MAX) if limb else a, w, 1.0, stride, pad)
            us.append(a)
            a = torch.nn.functional.leaky_relu(a, R.SLOPE)
        sat = us[-1].reshape(P, -1)
        assert bool(torch.isfinite(sat).all())
        bad = R.judge(route, "overflow", {"logits": sat[idx]})
        print(f"\n  {route}: saturating limbs -> {bad}")
        assert bad and all("above 65504" in b for b in bad)
        nan_dim = lg.clone()
        nan_dim[1::2] = float("nan")
        assert any("not finite" in b for b in R.judge(route, "overflow", {"logits": nan_dim[idx]}))
