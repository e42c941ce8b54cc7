"""The rehearsal of tests/test_gpu_upsample_regimes.py on the oracle alone (no GPU): the restatement of
tests/helpers/upsample_regimes.py is the oracle, every regime populates the branches it is named for on every step, the
margins cover the float32 error they are derived from, the caps on undecided samples hold, the committed fp32 floors -- from
which the GPU test's bars follow -- are what this torch build measures, and every mutation of the restatement is caught by
the regimes CAUGHT_BY names when it is judged exactly as the GPU output is."""
import pytest
import torch

import oi_oracle as O
from helpers import upsample_regimes as U

NAMES = tuple(U.REGIMES)


def test_shapes_are_the_issue_s():
    sc = {n: [s["S"] + i * s["n_new"] for i in range(s["K"])] for n, s in U.REGIMES.items()}
    assert sc["chain_64"] == [64, 80, 96, 112] and U.REGIMES["chain_64"]["n_new"] * 4 == 64
    all_sc = {v for l in sc.values() for v in l}
    assert {65, 66} <= all_sc                                              # Sc - 1 = 64 and 65: one against two scan chunks
    n_new = {s["n_new"] for s in U.REGIMES.values()}
    assert {9, 16, 64, 65, 140} <= n_new
    assert 64.0 * 2 ** (U.REGIMES["steep"]["K"] - 1) == 2048.0
    for n, s in U.REGIMES.items():
        assert 25 <= len(s["impacts"]) <= 30 and len(s["impacts"]) % U.RAYS_PER_WORKGROUP != 0, n
    assert U.REGIMES["wide"]["n_new"] > 64 and U.REGIMES["wide"]["S"] - 1 > 64
    assert set(U.POPULATION) == set(U.REGIMES) == set(U.FP32_FLOOR)
    assert set(U.CAUGHT_BY) | set(U.NOT_DETECTABLE) == set(U.MUTATIONS) and not set(U.CAUGHT_BY) & set(U.NOT_DETECTABLE)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_the_oracle(name):
    """Unmutated, `restate` is O.up_sample_weights + O.sample_pdf_det + O.merge_sorted bit for bit, in both precisions; its
    z_new (the running maximum) is the sorted raw list to within one ulp."""
    ch = U.case(name)
    for st in ch["steps"]:
        for dt, key in ((torch.float64, "r64"), (torch.float32, "r32")):
            ro, rd, z, sdf = (t.to(dt) for t in (ch["ro"], ch["rd"], st["z"], st["sdf"]))
            nt = torch.get_num_threads()
            torch.set_num_threads(1)
            try:
                w = O.up_sample_weights(ro, rd, z, sdf, st["inv_s"])
                zn = O.sample_pdf_det(z, w, st["n_new"])
            finally:
                torch.set_num_threads(nt)
            r = st[key]
            assert torch.equal(r["w5"], w + 1e-5) and torch.equal(r["z_raw"], zn), (name, st["i"], dt)
            assert torch.equal(r["z_merged"], O.merge_sorted(z, r["z_new"])[0])
            srt = torch.sort(zn, -1).values
            assert bool(((r["z_new"] - srt).abs().double() <= U.ulp32(srt) * (1 if dt == torch.float32 else 2.0 ** -29)).all())
        # the inputs of a step are the float32 chain's, sorted
        assert st["z"].dtype == torch.float32 and bool((st["z"][:, 1:] >= st["z"][:, :-1]).all())


@pytest.mark.parametrize("name", NAMES)
def test_branch_populations_and_caps(name):
    ch = U.case(name)
    print()
    for st in ch["steps"]:
        p = U.populations(ch, st)
        print(f"{name}[{st['i']}]: {p}")
        assert U.POPULATION[name](p, st["i"]), (name, st["i"], p)
        # cap: at most 2 % of the samples of a (regime, step) are undecided ...
        assert p["undecided"] <= U.CAP_UNDECIDED, (name, st["i"], p["undecided"])
        # ... and no population loses more than a quarter of its members that way
        for k, m in U.population_members(st).items():
            n = int(m.sum())
            kept = int((m & st["decided"]).sum())
            print(f"   population {k}: {kept} of {n} samples decided")
            if n and k not in U.CAP_EXEMPT:
                assert kept >= (1 - U.CAP_POPULATION) * n, (name, st["i"], k, kept, n)
    # deterministic: a second build gives the same bits
    again = U.build_chain(name, ch["seed"])
    for a, b in zip(again["steps"], ch["steps"]):
        assert torch.equal(a["z"], b["z"]) and torch.equal(a["sdf"], b["sdf"]) and torch.equal(a["decided"], b["decided"])


def test_flat_branch_is_reached_and_float32_cannot_decide_it():
    """`flat` holds >= 8 samples in a bracket with den < 1e-5 (float64); their den is closer to the threshold than the
    float32 grid of the CDF near 1, and the float32 restatement itself leaves the branch on some flat sections."""
    st = U.case("flat")["steps"][0]
    r64, r32 = st["r64"], st["r32"]
    flat = r64["den"] < 1e-5
    assert int(flat.sum()) >= 8
    assert float((1e-5 - r64["den"][flat]).max()) < float(U.ulp32(torch.tensor(0.998)))
    inc64, inc32 = r64["cdf"][:, 1:] - r64["cdf"][:, :-1], r32["cdf"][:, 1:] - r32["cdf"][:, :-1]
    sec = (inc64 < 1e-5) & (r64["cdf"][:, 1:] > 0.99)
    flips = int((sec & (inc32 >= 1e-5)).sum())
    print(f"\nflat: {int(sec.sum())} flat sections, {flips} of them not flat in float32; {int(flat.sum())} flat samples")
    assert flips > 0
    assert not bool((flat & st["decided"]).any())


@pytest.mark.parametrize("name", NAMES)
def test_margins_cover_the_fp32_error(name):
    """MARGIN's floors against the float32 restatement's measured error in the same quantity: 3x for the radius; for the CDF
    and den the floor covers the rays that miss the unit sphere (well-conditioned), every ray takes 3x its own error where
    that is larger (by construction of `decided`)."""
    ch = U.case(name)
    for st in ch["steps"]:
        r64, r32 = st["r64"], st["r32"]
        e_r = float(torch.maximum((r32["r0"].double() - r64["r0"]).abs().max(), (r32["r1"].double() - r64["r1"]).abs().max()))
        assert 3 * e_r <= U.MARGIN["radius"], (name, st["i"], e_r)
        e_cdf = (r32["cdf"].double() - r64["cdf"]).abs().max(-1).values
        inc = lambda r: (r["cdf"][:, 1:] - r["cdf"][:, :-1]).double()
        e_den = (inc(r32) - inc(r64)).abs().max(-1).values
        easy = (st["cls"] == U.CLASSES.index("unit_miss"))
        print(f"\n{name}[{st['i']}]: fp32 error radius {e_r:.2e}; cdf easy rays {float(e_cdf[easy].max()):.2e} / all "
              f"{float(e_cdf.max()):.2e}; den easy {float(e_den[easy].max()):.2e} / all {float(e_den.max()):.2e}")
        assert 3 * float(e_cdf[easy].max()) <= U.MARGIN["knot"] and float(e_den[easy].max()) <= U.MARGIN["den"]
        # decided samples keep 3x their ray's own error from the knots and from the den threshold
        d = st["decided"]
        gap = torch.minimum(r64["u"] - r64["c_below"], r64["c_above"] - r64["u"])
        assert bool((gap[d] >= (3 * e_cdf)[:, None].expand_as(gap)[d]).all())
        assert bool(((r64["den"] - 1e-5).abs()[d] >= (3 * e_den)[:, None].expand_as(gap)[d]).all())
        # ... and the float32 restatement indeed makes the reference's choice on every one of them
        assert torch.equal(r32["below"][d], r64["below"][d]), (name, st["i"])
        assert torch.equal((r32["den"] < 1e-5)[d], (r64["den"] < 1e-5)[d])


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_is_the_committed_one(name):
    """A fresh measurement within 1.5x of the committed table (a torch build whose float32 arithmetic is noisier must fail
    here, not move the GPU test's bars silently); the float32 restatement itself passes every assertion of the GPU test."""
    fresh = U.measure_floor(name)
    assert set(fresh) == set(U.FP32_FLOOR[name])
    print()
    for i, d in fresh.items():
        for c, v in d.items():
            print(f"  {name}[{i}] {c:10s} fp32 floor {v:.3e}  committed {U.FP32_FLOOR[name][i][c]:.3e}  bar {U.bar(name, i, c):.3e}")
            assert v <= 1.5 * U.FP32_FLOOR[name][i][c], (name, i, c, v)
    for st in U.case(name)["steps"]:
        assert U.judge(name, st["i"], st["r32"]["z_new"], st["r32"]["z_merged"]) == []


def _caught(mutation, name):
    ch = U.case(name)
    hits = []
    for st in ch["steps"]:
        r = U.restate(ch["ro"], ch["rd"], st["z"], st["sdf"], st["n_new"], st["inv_s"], torch.float32, mutate=mutation)
        bad = U.judge(name, st["i"], r["z_new"], r["z_merged"], value_factor=3.0)
        if bad:
            hits.append((st["i"], sorted({k for k, _ in bad})))
    return hits


@pytest.mark.parametrize("mutation", tuple(U.CAUGHT_BY))
def test_mutation_is_caught(mutation):
    """The float32 restatement with one plausible kernel error, judged exactly as the GPU output is (structural, bracket,
    value bar x 3), fails in every regime CAUGHT_BY names."""
    print()
    for name in U.CAUGHT_BY[mutation]:
        hits = _caught(mutation, name)
        print(f"  {mutation} in {name}: {hits}")
        assert hits, (mutation, name)


@pytest.mark.parametrize("mutation", tuple(U.NOT_DETECTABLE))
def test_mutation_listed_as_not_detectable_is_caught_nowhere(mutation):
    """(If one of these starts to be caught, it belongs in CAUGHT_BY.)"""
    assert all(not _caught(mutation, name) for name in NAMES), mutation
