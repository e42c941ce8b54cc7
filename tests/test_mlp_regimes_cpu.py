"""CPU side of tests/helpers/mlp_regimes.py: the restatement IS the oracle, every cell holds the population it is named for,
the committed float32 floors are reproduced, no bar exceeds the project's existing bar, the unmutated f16x3 emulation meets
every bar, and every rehearsed mutation is caught by the cells that claim it."""
import math

import pytest
import torch

import oi_oracle as O
from helpers import mlp_regimes as M


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_is_the_oracle(dtype):
    """`init`: restate against O.sdf_forward / O.color_head on the style net's own gamma / beta: 1e-12 in float64, bit-equal
    in float32."""
    c = M.cell("init")
    sd, csd = ({k: v.to(dtype) for k, v in s.items()} for s in M.golden_sds())
    w = O.style_mlp(sd, _latents("init").to(dtype))
    if dtype == torch.float32:
        assert torch.equal(w, c["w"])
    # the cell's gamma / beta are float32 values: evaluate the oracle at the latents, the restatement at the cell
    with torch.no_grad():
        sdf, feat, grad = O.sdf_forward(sd, c["pts"].to(dtype), w, want_grad=True)
        rgb = O.color_head(csd, feat, grad, w)
        if dtype == torch.float64:
            # the oracle's float64 gamma differs from the cell's float32 gamma by rounding: hand the oracle's own to restate
            gb = [O.film_params(sd, f"pts_linears.{l}.", w) for l in range(8)] + [O.film_params(csd, "views_linears.", w)]
            c = dict(c, gamma=torch.stack([x[0] for x in gb], 1), beta=torch.stack([x[1] for x in gb], 1))
        r = M.restate(c, dtype)
    for k, ref in (("sdf", sdf.squeeze(-1)), ("feat", feat), ("grad", grad), ("rgb", rgb)):
        if dtype == torch.float32:
            assert torch.equal(r[k], ref), k
        else:
            assert float((r[k] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k


def _latents(name):
    g = torch.Generator().manual_seed(M._seed(name))
    return torch.randn(M.B, 64, generator=g)


def _floor_log2_max(w):
    return math.frexp(float(w.abs().max()))[1] - 1


def test_cells_have_the_shape_and_differ_between_elements():
    for name in M.CELLS:
        c = M.cell(name)
        assert c["pts"].shape == (M.B * M.N_PER, 3) and c["gamma"].shape == (M.B, 9, 128) == c["beta"].shape, name
        assert M.N_PER == 128 + 37
        assert not torch.equal(c["gamma"][0], c["gamma"][1]) and not torch.equal(c["beta"][0], c["beta"][1]), name
        assert all(bool(torch.isfinite(c[k]).all()) for k in M.LEAVES + ("pts",)), name


def test_golden_scales_take_two_values_and_distinct_scales_eight():
    """The gap the cell closes: at the golden weights floor(log2 max|W|) is -6, -6, -7 x 5 and -7 for the colour head."""
    c0, c1 = M.cell("init"), M.cell("distinct_scales")
    mats = lambda c: [c["wh"][m] for m in range(7)] + [c["wv"][:, :128]]
    assert [_floor_log2_max(w) for w in mats(c0)] == [-6, -6, -7, -7, -7, -7, -7, -7]
    e = [_floor_log2_max(w) for w in mats(c1)]
    assert len(set(e)) == 8, e
    # the function is unchanged, and the float32 restatement is bit-identical to init's
    r0, r1 = M.restate(c0, torch.float32), M.restate(c1, torch.float32)
    d0, d1 = M.reference("init"), M.reference("distinct_scales")
    for k in M.FWD_TENSORS:
        assert torch.equal(r0[k], r1[k]), k
        assert float((d0[k] - d1[k]).abs().max()) <= 1e-12 * max(1.0, float(d0[k].abs().max())), k
    # ... and so is the emulated f16x3 forward (scaled image, G, A and B are the same numbers)
    e0, e1 = M.emulate(c0), M.emulate(c1)
    for k in M.FWD_TENSORS:
        assert torch.equal(e0[k], e1[k]), k


def test_gamma_spread_population():
    g = M.cell("gamma_spread")["gamma"]
    assert float(g.min()) <= -19.0 and float(g.max()) >= 79.0
    for l in M.SPREAD_LAYERS:
        assert int((g[:, l] == 0).sum()) >= 2 * M.B and int(((g[:, l].abs() < 1e-2) & (g[:, l] != 0)).sum()) >= 3 * M.B, l
        assert int((g[:, l] < -1.0).sum()) >= M.B, l


def test_loose_bound_population():
    c = M.cell("loose_bound")
    for l in range(1, 7):
        g = c["gamma"][:, l].abs()
        top = g.max(-1).values
        rest = g.sort(-1).values[:, -2]
        # (the median moves by a rank when the row itself is replaced: 2 %)
        assert bool((top >= 2.0 ** 7 * g.median(-1).values * 0.98).all()) and bool((top > 20 * rest).all()), l
        f = int(g[0].argmax())
        assert float(c["wh"][l - 1][f].abs().max()) == 0.0 and float(c["bh"][l - 1][f]) == 0.0


def test_bound_met_ratio():
    """|W_7^T V_7| reaches H_BOUND x max|V_7| to 1 %: the a-priori scale of the reverse sweep has no slack left."""
    c = {k: v.double() if torch.is_tensor(v) else v for k, v in M.cell("bound_met").items()}
    a = c["pts"]
    for l in range(8):
        g, b = M._pp(c["gamma"][:, l]), M._pp(c["beta"][:, l])
        phi = g * (a @ M._weight(c, l).t() + M._bias(c, l)) + b
        a = torch.sin(phi)
    assert float((torch.cos(phi) - 1.0).abs().max()) < 1e-4
    V7 = c["wsig"] * g * torch.cos(phi)
    bound = c["wh"][6].abs().sum(0).max()            # largest absolute row sum of the transposed image
    ratio = (V7 @ c["wh"][6]).abs().max(-1).values / (bound * V7.abs().max(-1).values)
    assert float(ratio.min()) >= 0.99, float(ratio.min())


@pytest.mark.parametrize("name", ["quiet_outlier@1e4", "quiet_outlier@1e6"])
def test_quiet_outlier_sets_the_scale_and_stays_quiet(name):
    c, r = M.cell(name), float(name.split("@")[1])
    for l in M.OUTLIER_LAYERS:
        w = c["wh"][l - 1]
        assert int(w.abs().argmax()) == 5 * 128 + 7
        others = w.abs().flatten().sort().values[-2]
        assert float(w.abs().max() / others) > r / 20       # the second largest weight is ~10 medians
        # the outlier's own phase: |gamma x outlier x a| <= 1e-3 x median|W|
        assert float(c["gamma"][:, l, 5].abs().max() * w.abs().max()) <= 1.01e-3 * float(w.abs().median())


def test_dead_layer_reference():
    c, r = M.cell("dead_layer"), M.reference("dead_layer")
    assert float(c["gamma"][0, M.DEAD_LAYER].abs().max()) == 0.0 and float(c["gamma"][1, M.DEAD_LAYER].abs().min()) > 0.0
    s0 = r["sdf"][:M.N_PER]
    assert float(s0.max() - s0.min()) == 0.0 and float(r["grad"][:M.N_PER].abs().max()) == 0.0
    assert float(r["grad"][M.N_PER:].abs().max()) > 1e-3
    gb = M.reference_backward("dead_layer")
    for l in range(M.DEAD_LAYER):
        assert float(gb[f"gamma.{l}"][0].abs().max()) == 0.0 and float(gb[f"beta.{l}"][0].abs().max()) == 0.0
    assert float(gb[f"beta.{M.DEAD_LAYER}"][0].abs().max()) > 0.0


def test_far_points_and_wide_phase_population():
    p = M.cell("far_points")["pts"]
    assert float(p.abs().max()) > 0.95 * M.FAR and float(p[7].abs().max()) == 0.0
    assert all(torch.equal(p[300], p[300 + i]) for i in range(1, 4)) and 300 >= M.N_PER + 128   # second element, ragged tile
    c = M.cell("wide_phase")
    rows = list(M.WIDE_ROWS)
    assert len(rows) == 16
    rev = c["beta"][:, 7, rows].abs() / (2 * math.pi)
    assert float(rev.max()) > 40.0 and int((rev > 32.0).sum()) >= 4


@pytest.mark.parametrize("name", M.CELLS)
def test_floor_is_reproduced(name):
    fresh = M.measure_floor(name)
    assert set(fresh) == set(M.FP32_FLOOR[name]), name
    half_ulp = 2.0 ** -24    # a float32 error below half an ulp of the tensor's largest entry is luck of the summation order
    for k, v in fresh.items():
        ref = max(M.FP32_FLOOR[name][k], half_ulp)
        v = max(v, half_ulp)
        assert v <= 1.5 * ref and ref <= 1.5 * v, (name, k, v, ref)


def test_no_bar_exceeds_the_project_bar():
    """Forward tensors: 3 x floor itself stays at or below the project's bar (the cells' gains were tuned for it).  Backward
    tensors: the bar is min(3 x floor, 2e-5) (mlp_regimes.bar)."""
    pairs = [(n, t) for n in M.CELLS for t in M.FP32_FLOOR[n]]
    for n, t in pairs:
        assert M.bar(n, t) <= M.project_bar(t), (n, t, M.bar(n, t))
        if not t.startswith("d."):
            assert 3.0 * M.FP32_FLOOR[n][t] <= M.project_bar(t), (n, t)
    assert len(M.AT_PROJECT_BAR) <= len(pairs) // 4
    for n in M.CELLS:
        assert set(M.tensors_of(n)) <= set(M.FP32_FLOOR[n])
        assert (n in M.BWD_CELLS) == ("d.w0" in M.FP32_FLOOR[n])


@pytest.mark.parametrize("name", M.CELLS)
def test_emulation_meets_every_bar(name):
    e = M.errors(name, M.emulate(M.cell(name)))
    bad = {k: (v, M.bar(name, k)) for k, v in e.items() if v > M.bar(name, k)}
    assert not bad, bad
    if name == "dead_layer":
        assert float(M.emulate(M.cell(name))["grad"][:M.N_PER].abs().max()) == 0.0


def test_every_mutation_is_accounted_for():
    assert set(M.CAUGHT_BY) | set(M.NOT_DETECTABLE) == set(M.MUTATIONS)
    assert not set(M.CAUGHT_BY) & set(M.NOT_DETECTABLE) and len(M.NOT_DETECTABLE) <= 2
    assert all(cells and set(cells) <= set(M.CELLS) for cells in M.CAUGHT_BY.values())


@pytest.mark.parametrize("mutation,name", [(m, n) for m, cells in M.CAUGHT_BY.items() for n in cells])
def test_mutation_is_caught(mutation, name):
    """The mutated emulation, judged as the GPU output is, misses some tensor's bar by a factor of 3 at least."""
    e = M.errors(name, M.emulate(M.cell(name), mutation))
    worst = max(v / M.bar(name, k) for k, v in e.items())
    assert worst >= 3.0, (mutation, name, {k: f"{v:.2e} / {M.bar(name, k):.2e}" for k, v in e.items()})
