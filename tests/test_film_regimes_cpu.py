"""CPU side of tests/helpers/film_regimes.py: the restatements ARE the oracle, the hand-written backwards are its autograd,
every cell holds the population it is named for, the committed float32 floors are reproduced, no bar exceeds the project's
existing bar, every rehearsed mutation is caught by the cells that claim it, and the shapes chosen for the GPU test reach every
branch of the colour head's chunking rule (checked against the library's own workspace size)."""
import math

import pytest
import torch

import oi_oracle as O
from helpers import film_regimes as M


# ----------------------------------------------------------------------------------------------------------------------
# restatement = oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("B", M.FILM_FWD_B)
def test_film_restatement_is_the_oracle(dtype, B):
    """`init`: O.style_mlp and O.film_params of the golden state dicts: 1e-12 in float64, bit-equal in float32."""
    c = M.cell(f"init@{B}")
    sd, csd = ({k: v.to(dtype) for k, v in s.items()} for s in M.golden_sds())
    with torch.no_grad():
        w = O.style_mlp(sd, c["z"].to(dtype))
        gb = [O.film_params(sd, f"pts_linears.{l}.", w) for l in range(8)] + [O.film_params(csd, "views_linears.", w)]
        r = M.film_restate(c, dtype)
    ref = {"w": w, "gamma": torch.stack([x[0] for x in gb], 1), "beta": torch.stack([x[1] for x in gb], 1)}
    for k, v in ref.items():
        if dtype == torch.float32:
            assert torch.equal(r[k], v), k
        else:
            assert float((r[k] - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), k


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_colour_restatement_is_the_oracle(dtype):
    """`colour/init`: O.color_head on the style vector the cell's gamma / beta came from."""
    c = M.cell("colour/init")
    csd = {k: v.to(dtype) for k, v in M.golden_sds()[1].items()}
    with torch.no_grad():
        ref = O.color_head(csd, c["feat"].to(dtype), c["normals"].to(dtype), c["w"].to(dtype))
        if dtype == torch.float64:
            # the oracle's float64 gamma differs from the cell's float32 gamma by rounding: hand the oracle's own to restate
            g, b = O.film_params(csd, "views_linears.", c["w"].to(dtype))
            c = dict(c, gamma=g, beta=b)
        r = M.colour_restate(c, dtype)["rgb"]
    if dtype == torch.float32:
        assert torch.equal(r, ref)
    else:
        assert float((r - ref).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", ["init@33", "one_sided@1", "dead_units@33", "w_route@33", "layer_range@33", "batch_cancel@33"])
def test_film_backward_by_hand_is_autograd(name):
    c = M.cell(name)
    hand, auto = M.film_backward(c), M.reference_backward(name)
    assert set(hand) == set(auto) == set(M.film_backward_names(c))
    for k in auto:
        assert float((hand[k] - auto[k]).abs().max()) <= 1e-12 * max(1.0, float(auto[k].abs().max())), (name, k)


@pytest.mark.parametrize("name", ["colour/init", "colour/gamma_spread", "colour/steep_normals", "colour/trained_rgb@513"])
def test_colour_backward_by_hand_is_autograd(name):
    hand, auto = M.colour_backward(M.cell(name)), M.reference_backward(name)
    assert set(hand) == set(auto) == set(M.COLOUR_GRADS)
    for k in auto:
        assert hand[k].shape == auto[k].shape, k
        assert float((hand[k] - auto[k]).abs().max()) <= 1e-12 * max(1.0, float(auto[k].abs().max())), (name, k)


# ----------------------------------------------------------------------------------------------------------------------
# populations
# ----------------------------------------------------------------------------------------------------------------------
def test_film_cells_hold_their_population():
    g0 = M.reference("init@33")["gamma"]
    assert float(g0.min()) > 0.0 and float(M.reference("init@33")["w"].abs().max()) < 4.5      # the gap: gamma one-sided at init
    for B in M.FILM_FWD_B:
        r, r0 = M.reference(f"grown@{B}")["gamma"], M.reference(f"init@{B}")["gamma"]
        assert float(r.max() - r.min()) > 1.8 * float(r0.max() - r0.min()), B       # (one latent spans less than 33 do)
        f = M.film_restate(M.cell(f"one_sided@{B}"))
        neg, pos = f["pres"][M.ONE_SIDED_NEG[0]], f["pres"][M.ONE_SIDED_POS[0]]
        assert float(neg.max()) < 0.0 and float(pos.min()) > 0.0, (B, float(neg.max()), float(pos.min()))
        f = M.film_restate(M.cell(f"dead_units@{B}"))
        rows = list(M.DEAD_ROWS)
        assert float(f["pres"][M.DEAD_LAYER][:, rows].abs().max()) == 0.0 and float(f["hs"][M.DEAD_LAYER + 1][:, rows].abs().max()) == 0.0
        f32 = M.film_restate(M.cell(f"dead_units@{B}"), torch.float32)
        assert float(f32["pres"][M.DEAD_LAYER][:, rows].abs().max()) == 0.0
        c = M.cell(f"w_route@{B}")
        assert c["z"] is None and c["w"].shape == (B, 64)
    g = M.reference("grown@33")["gamma"]
    assert -30.0 < float(g.min()) < -15.0 and 70.0 < float(g.max()) < 100.0, (float(g.min()), float(g.max()))


def test_dead_units_backward_uses_slope_0_2():
    """torch.nn.functional.leaky_relu differentiates as x > 0 ? 1 : slope; the reference gradient of a dead row's bias is
    0.2 x the incoming gradient, not 1 x and not 0."""
    x = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(x, 0.2).sum().backward()
    assert x.grad.tolist() == [0.2, 0.2, 0.2]
    c = M.cell("dead_units@33")
    good, bad = M.film_backward(c), M.film_backward(c, mutate="slope_one_at_zero")
    rows = list(M.DEAD_ROWS)
    k = f"d_style_b.{M.DEAD_LAYER}"
    assert float(good[k][rows].abs().min()) > 0.0
    assert float((bad[k][rows] / good[k][rows] - 5.0).abs().max()) < 1e-9


def test_layer_range_and_batch_cancel_population():
    for B in M.FILM_BWD_B:
        c = M.cell(f"layer_range@{B}")
        mags = [float(c["cg"][:, l].abs().max()) for l in range(M.NL_ALL)]
        assert mags[M.ZERO_COT_LAYER] == 0.0 and float(c["cb"][:, M.ZERO_COT_LAYER].abs().max()) == 0.0
        assert mags[0] > 1e7 * mags[8] > 0.0 and float(c["cw"].abs().max()) > 0.0
        ref = M.reference_backward(f"layer_range@{B}")
        for k in ("d_gw", "d_gb", "d_bw", "d_bb"):
            assert float(ref[f"{k}.{M.ZERO_COT_LAYER}"].abs().max()) == 0.0
            assert float(ref[f"{k}.8"].abs().max()) > 0.0
    c = M.cell("batch_cancel")
    assert c["B"] == 33
    for k, s in (("cg", 15.0), ("cb", 0.25)):
        t = s * c[k].double()
        ratio = t.sum(0).abs() / t.abs().sum(0)
        assert 2e-4 < float(ratio.median()) < 5e-3, float(ratio.median())
    assert M.scale_of("batch_cancel", "d_gb.0") > 100.0 * float(M.reference_backward("batch_cancel@33")["d_gb.0"].abs().max())


def test_colour_cells_hold_their_population():
    r0 = M.reference("colour/init")["rgb"]
    assert 0.45 < float(r0.min()) and float(r0.max()) < 0.54                       # the gap: the sigmoid's flat middle
    for name in ("colour/trained_rgb", "colour/gamma_spread", "colour/steep_normals", "colour/quiet_element"):
        r = M.reference(name)["rgb"]
        assert 1e-4 < float(r.min()) < 3e-3 and 1 - 3e-3 < float(r.max()) < 1 - 1e-4, (name, float(r.min()), float(r.max()))
    c = M.cell("colour/saturated")
    r = M.colour_restate(c, torch.float32)["rgb"]
    assert float(r[:, 0].min()) == 1.0 and float(r[:, 2].min()) == 1.0 and 0.0 < float(r[:, 1].max()) < 1e-12
    c = M.cell("colour/gamma_spread")
    for f, target in M.PINNED:
        assert bool((c["gamma"][:, f] == target).all())
    gb = M.reference_backward("colour/gamma_spread")
    zero_rows = [f for f, t in M.PINNED if t == 0.0]
    assert float(gb["d_gamma"][:, zero_rows].abs().min()) > 0.0                    # d gamma lives at gamma = 0 ...
    assert float(gb["d_wv"][zero_rows].abs().max()) == 0.0 and float(gb["d_bv"][zero_rows].abs().max()) == 0.0   # ... alone
    c = M.cell("colour/steep_normals")
    nn = c["normals"].norm(dim=-1)
    n = c["normals"].shape[0]
    assert float(nn.max()) > 25.0 and int((nn == 0).sum()) == n // 10 and int((c["feat"].abs().sum(-1) == 0).sum()) == 1
    c = M.cell("colour/quiet_element")
    assert float(c["cot"][c["npe"]:].abs().max()) == 0.0 and float(c["cot"][:c["npe"]].abs().min()) > 0.0
    gb = M.reference_backward("colour/quiet_element")
    for k in ("d_gamma", "d_beta"):
        assert float(gb[k][1].abs().max()) == 0.0 and float(gb[k][0].abs().max()) > 0.0
    for name in M.colour_cells():
        c = M.cell(name)
        assert not torch.equal(c["gamma"][0], c["gamma"][1]) and not torch.equal(c["beta"][0], c["beta"][1]), name


# ----------------------------------------------------------------------------------------------------------------------
# floors and bars
# ----------------------------------------------------------------------------------------------------------------------
def test_every_cell_has_its_floors():
    assert sorted(M.FP32_FLOOR) == sorted(M.all_cells())
    for name in M.all_cells():
        c = M.cell(name)
        want = {"rgb", *M.COLOUR_GRADS} if name.startswith("colour/") else \
            {"w", "gamma", "beta", *(M.film_backward_names(c) if name in M.film_cells(True) else ())}
        assert set(M.FP32_FLOOR[name]) == want, name


@pytest.mark.parametrize("name", M.all_cells())
def test_floor_is_reproduced(name):
    fresh = M.measure_floor(name)
    assert set(fresh) == set(M.FP32_FLOOR[name]), name
    for k, v in fresh.items():
        half_ulp = M.ulp_floor(name, k) / 8.0    # an error below half an ulp of the largest entry is luck of the summation order
        ref, v = max(M.FP32_FLOOR[name][k], half_ulp), max(v, half_ulp)
        assert v <= 1.5 * ref and ref <= 1.5 * v, (name, k, v, ref)


def test_no_bar_exceeds_the_project_bar():
    """Every bar <= the bar of the test it joins; forward tensors and the colour head's feature / FiLM gradients also have
    3 x floor itself below it (the cells' gains were tuned for that); the bars that ARE the project's bar are few."""
    at_cap, total = [], 0
    for name in M.all_cells():
        for t, fl in M.FP32_FLOOR[name].items():
            total += 1
            assert M.bar(name, t) <= M.project_bar(t), (name, t, M.bar(name, t))
            if t in ("w", "gamma", "beta", "rgb", "d_feat", "d_normals", "d_gamma"):
                assert 3.0 * fl <= M.project_bar(t), (name, t, fl)
            if M.bar(name, t) == M.project_bar(t):
                at_cap.append((name, t))
    assert len(at_cap) <= total // 50, at_cap


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
def test_every_mutation_is_accounted_for():
    assert set(M.CAUGHT_BY) == set(M.MUTATIONS) and len(set(M.MUTATIONS)) == len(M.MUTATIONS) >= 12
    known = set(M.all_cells())
    for m, cells in M.CAUGHT_BY.items():
        assert cells and {M.canonical(n) for n in cells} <= known, m


@pytest.mark.parametrize("mutation,name", [(m, n) for m, cells in M.CAUGHT_BY.items() for n in cells])
def test_mutation_is_caught(mutation, name):
    """The mutated restatement, judged as the GPU output is, misses some tensor's bar by a factor of 3 at least."""
    e = M.mutated_errors(mutation, name)
    assert max(e.values()) >= 3.0, (mutation, name, {k: f"{v:.2f}" for k, v in e.items()})


def test_unmutated_float32_meets_every_bar():
    """The other direction: plain float32 of the restatement (not a variant the floors were taken from alone) passes."""
    for name in M.all_cells():
        if name.endswith(f"@{M.BIG_NPE}"):
            continue
        c = M.cell(name)
        with torch.no_grad():
            if name.startswith("colour/"):
                e = M.errors(name, M.colour_restate(c, torch.float32))
                e.update(M.backward_errors(name, M.colour_backward(c, torch.float32, block=64)))
            else:
                e = M.errors(name, M.film_restate(c, torch.float32))
                if name in M.film_cells(True):
                    e.update(M.backward_errors(name, M.film_backward(c, torch.float32)))
        bad = {k: (v, M.bar(name, k)) for k, v in e.items() if v > M.bar(name, k)}
        assert not bad, (name, bad)


def test_strided_placement_rehearsal():
    rows = torch.arange(2 * 128, dtype=torch.float64).view(2, 128)
    good, bad = M.place_strided(rows), M.place_strided(rows, mutate="d_gamma_stride_128")
    assert torch.equal(good[:, 8], rows) and bool(torch.isnan(good[:, :8]).all())
    assert torch.equal(bad[0, 8], rows[0]) and bool(torch.isnan(bad[1, 8]).all())


# ----------------------------------------------------------------------------------------------------------------------
# the chunking rule of csrc/color_head.hip
# ----------------------------------------------------------------------------------------------------------------------
def test_shapes_reach_every_chunking_branch():
    shapes = [(M.COLOUR_B, n) for n in (M.COLOUR_NPE,) + M.SHAPE_NPE + (M.BIG_NPE,)]
    cv = {s: M.carve(*s) for s in shapes}
    assert any(v["chunk_pts"] == 128 for v in cv.values())
    assert cv[(2, M.BIG_NPE)]["chunk_pts"] == 160 and 2 * M.BIG_NPE > 131072
    assert M.carve(2, 65536)["chunk_pts"] == 128                  # ... and it is the smallest such power-of-two-ish neighbourhood
    assert any(v["nchunk"] % 4 != 0 and v["nchunk"] > 4 for v in cv.values())
    tails = {v["tail"] for v in cv.values()}
    assert {1, 16, 17, 31, 32, 33} <= tails, sorted(tails)
    for (B, npe), v in cv.items():
        assert (v["nchunk"] - 1) * v["chunk_pts"] < npe <= v["nchunk"] * v["chunk_pts"] and v["chunk_pts"] % 32 == 0
    big = cv[(2, M.BIG_NPE)]
    assert big["nchunk"] == 413 and big["tail"] == 80 and 190e6 < big["total"] < 210e6     # 135 MB of per-point vectors, 61 MB of partials


def test_carve_agrees_with_the_library():
    """oi_color_head_bwd_workspace_bytes is a host function: the restated carve gives the library's own size."""
    from helpers import cabi
    _, L = cabi.built_lib()
    for npe in (M.COLOUR_NPE,) + M.SHAPE_NPE + (M.BIG_NPE, 65536, 4100):
        for B in (1, 2, 3):
            assert int(L.oi_color_head_bwd_workspace_bytes(B, npe)) == M.carve(B, npe)["total"], (B, npe)
    assert int(L.oi_color_head_bwd_workspace_bytes(0, 5)) == 0
