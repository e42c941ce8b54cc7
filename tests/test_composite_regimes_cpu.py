"""The rehearsal of tests/test_gpu_composite_regimes.py on the oracle alone (no GPU): every regime of
tests/helpers/composite_regimes.py populates the branch it is named for, keeps its margin to every kink, has finite float64
gradients, and the committed fp32 floors -- from which the GPU test's bars follow -- are what this torch build measures."""
import pytest
import torch

from helpers import composite_regimes as R

NAMES = tuple(R.REGIMES)


def test_regime_table_is_the_issue_s():
    inv_s = {k: float(torch.exp(torch.tensor(v["variance"] * 10.0, dtype=torch.float64))) for k, v in R.REGIMES.items()}
    assert abs(inv_s["base"] - 20.09) < 0.01 and abs(inv_s["sharp"] - 148.4) < 0.1 and abs(inv_s["trained"] - 1096.6) < 0.1
    assert inv_s["clamped_hi"] > 1e6 and inv_s["clamped_lo"] < 1e-6
    assert (R.B, R.H, R.W, R.T) == (2, 3, 4, 70) and R.N % 64 != 0 and R.T > 64
    assert set(R.POPULATION) == set(R.REGIMES) == set(R.FP32_FLOOR) and set(R.FP32_FLOOR_SINGLE) == set(R.SINGLE_REGIMES)
    assert len(R.COTANGENTS) == 11 and len(R.SINGLE_CASES) == 14


@pytest.mark.parametrize("name", NAMES)
def test_branch_populations_and_kink_margins(name):
    inp = R.case(name)[0]
    pop, mar = R.populations(inp), R.min_margins(inp)
    print(f"\n{name}: populations {pop}\n{name}: smallest distance to a kink {mar}")
    assert R.POPULATION[name](pop), pop
    for k, m in R.MARGIN.items():
        assert mar[k] >= m, (k, mar[k], m)
    s_bad, r_bad = R.offenders(inp)
    assert not bool(s_bad.any()) and not bool(r_bad.any())
    # the builder is deterministic: a second build gives the same bits
    again = R.build_inputs(name)
    for k in ("sdf", "grad", "rgb", "dists", "mid_z", "rays_o", "rays_d"):
        assert torch.equal(again[k], inp[k]), k


@pytest.mark.parametrize("name", NAMES)
def test_float64_reference_is_finite(name):
    inp, out, grads = R.case(name)
    for k, v in list(out.items()) + list(grads.items()):
        assert bool(torch.isfinite(v).all()), (name, k)
    # exact where the mathematics is exact, on the reference itself
    if name in ("clamped_hi", "clamped_lo"):
        assert float(grads["variance"]) == 0.0
    if name in ("no_specular", "zero_specular"):
        assert float(grads["specular"]) == 0.0
    if name == "no_bg":
        assert torch.equal(out["image"], out["image_no_bg"])
    if name in R.SINGLE_REGIMES:
        for single in R.SINGLE_CASES:
            for k, v in R.single_reference(name, single).items():
                assert bool(torch.isfinite(v).all()), (name, single, k)
        # the mask's gradient reaches the rays inside the clamp window only
        q = R.deciding(inp)
        outside = ~((q["W"] > 1e-3) & (q["W"] < 1 - 1e-3))
        assert not bool(R.single_reference(name, "mask")["sdf"][outside].any())


@pytest.mark.parametrize("mutate", ["tc_lt_1", "tc_lt_0"])
def test_kinks_regime_feels_both_relu_masks(mutate):
    """A backward without the `tc < 1` (or `tc < 0`) mask of iter_cos -- the restatement with that relu's derivative set to 1
    everywhere, values unchanged -- must move d_grad of `kinks` far past the bar the GPU test holds it to: the samples in each
    true_cos band sit where a gradient reaches them, not only behind the surface."""
    inp, out, grads = R.case("kinks")
    out_m, grads_m = R.evaluate(inp, torch.float64, mutate=mutate)
    assert torch.equal(out_m["weights"], out["weights"]) and torch.equal(out_m["image"], out["image"])
    moved = R.rel_err(R.grad_tensors(inp, grads_m)["d_grad"], R.grad_tensors(inp, grads)["d_grad"])
    b = R.bar("kinks", "d_grad")[0]
    print(f"\nkinks: dropping the {mutate} mask moves d_grad by {moved:.3e} of its scale (bar {b:.1e})")
    assert moved >= 100 * b, (mutate, moved, b)


def _check_floor(fresh, committed, what):
    for k, v in fresh.items():
        print(f"  {what} {k:14s} fp32 floor {v:.3e}  committed {committed[k]:.3e}  bar {max(R.project_bar(k), 3 * committed[k]):.3e}")
    assert set(fresh) == set(committed), what
    for k, v in fresh.items():
        assert v <= 1.5 * committed[k], (what, k, v, committed[k])


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_is_the_committed_one(name):
    """float32 restatement against the float64 one, every output map and every gradient: within 1.5x of the committed table
    (a torch build whose float32 arithmetic is noisier must fail here, not move the GPU test's bars silently)."""
    print()
    _check_floor(R.measure_floor(name), R.FP32_FLOOR[name], name)
    if name in R.SINGLE_REGIMES:
        for single in R.SINGLE_CASES:
            _check_floor(R.measure_floor(name, single), R.FP32_FLOOR_SINGLE[name][single], f"{name}/{single}")


def test_bars_are_the_project_s_or_three_floors():
    for name in NAMES:
        for t, fl in R.FP32_FLOOR[name].items():
            b, why = R.bar(name, t)
            assert b == max(R.project_bar(t), 3 * fl) and why == ("floor" if 3 * fl > R.project_bar(t) else "project")
