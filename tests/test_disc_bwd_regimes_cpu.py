"""The rehearsal of tests/test_gpu_disc_bwd_regimes.py without a GPU: every regime has its clean images, the launch plans
select on every route the class of epilogue the route is named for, the committed fp32 floors -- from which every bar of the GPU
test follows -- are what a fresh computation gives, the float32 restatement passes its own bars with margin, every plausible
kernel error is more than 3 x bar away where CAUGHT_BY says, and the linear cotangent leaves a gradient in every regime."""
import math

import pytest
import torch

from helpers import disc_bwd_regimes as Q
from helpers import disc_regimes as R


def _same_to_the_last_digit(fresh, committed):
    """Both printed as d.dde-xx: at most one unit of the last digit apart."""
    return abs(fresh - committed) <= 10.0 ** (math.floor(math.log10(committed)) - 2) * 1.0001


@pytest.mark.parametrize("name", Q.NAMES)
def test_clean_images(name):
    """At least three of the six pool images (the only one of a 128 x 128 regime) have no kink-adjacent activation; the
    compared batches are made of those; `mask` has its zero image as a fake."""
    near, cl = Q.kink_adjacent(name), Q.clean(name)
    P = R.case(name)["x"].shape[0]
    real, fake = Q.batch(name)
    print(f"\n  {name}: kink-adjacent activations per image {near}, clean {cl}, real {real}, fake {fake}")
    assert len(cl) >= min(Q.MIN_CLEAN, P) and set(real) | set(fake) <= set(cl) and len(set(real)) == len(real)
    assert len(real) == len(fake) == (2 if P > 1 else 1)
    if name == "mask":
        assert fake[0] == R.MASK_ZERO_IMAGE and R.MASK_ZERO_IMAGE not in real
        # ... and the zero image is exactly zero in every layer of both chains: on the kink, not beside it
        c = R.case(name)
        assert all(not bool(u[R.MASK_ZERO_IMAGE].any()) for u in c["u64"] + c["u32"])
        assert R.MASK_ZERO_IMAGE in Q.layer_images(name)


def test_plans_select_the_class_of_every_route():
    seen = {"dgrad": set(), "wgrad": set()}
    for name in Q.NAMES:
        for route in Q.routes_of(name):
            r = Q.LAYER_ROUTES[route]
            dp, wp = Q.plans(name, route)
            assert (dp["k_splits"], dp["cls"]) == r["dgrad"] and (wp["k_splits"], wp["cls"]) == r["wgrad"], (name, route, dp, wp)
            seen["dgrad"].add(dp["cls"])
            seen["wgrad"].add(wp["cls"])
            for tag in r["first"]:
                kernel, cls = tag.split(":")
                assert r[kernel][1] == cls
    # every class of both kernels is reached, each named by exactly one route as its smallest
    assert seen["dgrad"] == seen["wgrad"] == set(Q.CLASSES)
    firsts = [t for r in Q.LAYER_ROUTES.values() for t in r["first"]]
    assert sorted(firsts) == sorted(f"{k}:{c}" for k in ("dgrad", "wgrad") for c in Q.CLASSES)
    # smallest: at batch 1 no layer of the 64 x 64 network has an atomics-only launch of either kernel, nor at batch 2 a
    # block before the third for the weight gradient; the data gradient has one only in the 128 x 128 network (Cout 32)
    s64, s128 = R.REGIMES["unit"], R.REGIMES["unit_128"]
    assert all(Q.wgrad_plan(1, *Q.layer_shape(s64, l))["cls"] != "atomic" for l in range(5))
    assert all(Q.wgrad_plan(2, *Q.layer_shape(s64, l))["cls"] != "atomic" for l in (0, 1))
    assert all(Q.dgrad_plan(b, *Q.layer_shape(s64, l))["cls"] != "atomic" for l in range(5) for b in (1, 2, 3, 4))
    assert Q.dgrad_plan(1, *Q.layer_shape(s128, 0))["cls"] == "atomic"
    # the ragged routes: 1 1/2 pixel tiles per parity class; 3 of a trip's 16 pixels, 7 (1) of 32 rows, a ragged channel trip
    dp, wp = Q.plans("unit", "b3_B3")
    assert dp["Mc"] == 48 and wp["P"] == 48
    dp, wp = Q.plans("unit", "head_B3")
    assert wp["P"] == 3 and Q.layer_shape(s64, 4)[2] == 7 and 7 % dp["trip"] != 0
    assert Q.layer_shape(s64, 0)[0] == 3   # block 0: 3 of a 32-channel tile


@pytest.mark.parametrize("name", Q.NAMES)
def test_tables_are_the_committed_ones(name):
    """A fresh computation of every floor equals the committed one to the last printed digit -- and with that the float32
    restatement passes its own bars with the margin of the factor 3."""
    fresh = Q.measure_floor(name)
    assert set(fresh) == set(Q.FP32_FLOOR_BWD[name])
    keys = {f"{r}/{k}" for r in Q.routes_of(name) for k in Q.LAYER_KEYS} | {f"{k}/{p}" for k in Q.NET_KEYS for p in R.case(name)["wsd"]}
    assert set(fresh) == keys
    print()
    for k, v in fresh.items():
        print(f"  {name} {k:28s} fp32 floor {v:.3e}  committed {Q.FP32_FLOOR_BWD[name][k]:.2e}")
        assert _same_to_the_last_digit(v, Q.FP32_FLOOR_BWD[name][k]), (name, k, v)
    assert Q.judge(name, fresh) == [] and all(v <= 0.34 * Q.bar(name, k) for k, v in fresh.items())


def test_layout():
    assert set(Q.FP32_FLOOR_BWD) == set(Q.NAMES) == set(R.NET64) | {"unit_128", "default_init_128"}
    assert set(Q.CAUGHT_BY) | set(Q.NOT_DETECTABLE) == set(Q.MUTATIONS) and not set(Q.CAUGHT_BY) & set(Q.NOT_DETECTABLE)
    assert len(Q.MUTATIONS) == 9
    for pairs in Q.CAUGHT_BY.values():
        assert pairs and all(n in Q.NAMES and (r == "net" or r in Q.routes_of(n)) for n, r in pairs)
    # every class of the weight-gradient kernel has its accumulate path held against a prefilled buffer
    assert {Q.LAYER_ROUTES[r]["wgrad"][1] for _, r in Q.CAUGHT_BY["acc_overwritten"]} == set(Q.CLASSES)


@pytest.mark.parametrize("name", Q.NAMES)
def test_layer_cases_are_what_they_say(name):
    for route in Q.routes_of(name):
        c = Q.layer_case(name, route)
        o = c["o"]
        assert all(o[k].dtype == torch.float32 for k in ("x", "ref", "w", "g")) and all(v.dtype == torch.float32 for v in o["acc"].values())
        assert all(v.dtype == torch.float64 for v in c["refs"].values()) and set(c["refs"]) == set(Q.LAYER_KEYS)
        assert all(s > 0 for s in c["scale"].values()), (name, route, c["scale"])
        for k in ("wgrad_m", "bwd_gw"):   # the prefill is of the gradient's own size: neither hides the other
            assert 0.5 < R.rms(o["acc"][k]) / c["scale"][k] < 2.0
        v, ref, want = Q.layer_mask_mul(name, route)
        assert torch.equal(want, torch.where(ref > 0, v, v * 0.2))
    if name == "mask":
        # exact zeros: in block 0's sums and, through the zero image, in every layer
        assert bool((Q.layer_case(name, "b0_B1")["o"]["ref"] == 0).any()) and bool((Q.layer_case(name, "b1_B1")["o"]["x"] == 0).any())
        o = Q.layer_case(name, "b3_B3")["o"]
        assert not bool(o["x"][1].any()) and not bool(o["ref"][1].any()) and bool(o["g"][1].any())


@pytest.mark.parametrize("name", Q.NAMES)
def test_linear_cotangent_leaves_a_gradient(name):
    """gw_plain is non-zero for every parameter in every regime (BCE(d, 1) alone is not: its gradient vanishes where the
    logits saturate), and so are the R1 and the step gradients."""
    c = Q.net_case(name)
    for key in Q.NET_KEYS:
        assert all(s > 0 and math.isfinite(s) for s in c["scale"][key].values()), (name, key, c["scale"][key])
    if name == "grown8":
        real, _ = Q.batch(name)
        d = R.case(name)["u64"][-1][list(real), 0].flatten()
        g = torch.sigmoid(d) - 1.0
        print(f"\n  grown8: logits {d.tolist()}, BCE(d, 1)' {g.tolist()}")
        assert bool((g == 0).all())


@pytest.mark.parametrize("mutation", tuple(Q.CAUGHT_BY))
def test_mutation_is_caught(mutation):
    print()
    for name, route in Q.CAUGHT_BY[mutation]:
        hits = Q.caught(name, route, mutation)
        print(f"  {mutation} in {name} / {route}: {hits}")
        assert hits, (mutation, name, route)
    if mutation == "acc_overwritten":
        assert all(set(k.split("/")[1] for k in Q.caught(n, r, mutation)) == {"wgrad_m+acc", "bwd_gw+acc"} for n, r in Q.CAUGHT_BY[mutation])
    if mutation == "mask_ge":   # only the exact zeros of `mask` tell `>` from `>=`
        assert not Q.caught("unit", "b0_B1", mutation) and not Q.caught("white_bg", "b0_B1", mutation)
    if mutation == "pre_per_split":   # one split: nothing to apply twice
        assert not Q.caught("unit", "head_B1", mutation)
