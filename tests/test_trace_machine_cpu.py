"""The rehearsal of tests/helpers/trace_machine.py, restatement alone: the fused multiply-add is exact, the cases between them
take every transition of include/oi_trace.h:23-37 at least 8 times and leave no ray out, the restatement agrees with the float64
tracers the project already trusts (helpers.trace_ref.trace, helpers.occlusion_ref.trace_anyhit) on the well-conditioned
cases and with closed forms in float64 on the radial fields and the jump, and every mutation of MUTATIONS changes a compared
word in each case CAUGHT_BY names for it.  tests/test_gpu_trace_machine.py then holds the kernels to the same restatement
bit for bit."""
import collections
import fractions
import functools

import numpy as np
import pytest

from helpers import occlusion_ref as OC
from helpers import trace_machine as TM
from helpers import trace_ref as T

MIN_TAKEN = 8


@functools.lru_cache(maxsize=None)
def rehearse(name, anyhit):
    c = TM.CASES[name]
    return TM.run32(c, c.n_fixed or TM.REHEARSAL_N, anyhit)


# ---------------------------------------------------------------------------------------------------------------------
# the fused multiply-add
# ---------------------------------------------------------------------------------------------------------------------
def _fma_rational(a, b, c):
    """fmaf by another road: the exact sum as a Fraction, rounded to float32 by comparing it with its two float32 neighbours."""
    x = fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))
    if x == 0:
        return np.float32(float(a) * float(b) + float(c))
    g = np.float32(float(x))                                   # a float32 near x (twice rounded: a neighbour at worst)
    cands = sorted({g, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))}, key=float)
    best = None
    for q in cands:
        if not np.isfinite(q):
            continue
        err = abs(fractions.Fraction(float(q)) - x)
        even = (int(np.array(q).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, q)
    return best[1]


def test_fma32_is_exact_where_float64_rounds_twice():
    """a b = 64 (1 + 2^-12) (1 - 2^-12 + 2^-24) = 64 + 2^-30 exactly and c = 2^30, where float32 numbers are 128 apart: the sum
    lies 2^-30 above the tie 2^30 + 64 and rounds UP.  float64 (numbers 2^-22 apart there) first rounds it onto the tie, and
    the tie then goes to the even neighbour, DOWN."""
    a, b, c = np.float32(8.0 * (1.0 + 2.0 ** -12)), np.float32(8.0 * (1.0 - 2.0 ** -12 + 2.0 ** -24)), np.float32(2.0 ** 30)
    assert fractions.Fraction(float(a)) * fractions.Fraction(float(b)) == 64 + fractions.Fraction(1, 2 ** 30)
    assert TM.fma32(a, b, c) == np.float32(2.0 ** 30 + 128.0) == _fma_rational(a, b, c)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(2.0 ** 30)


def test_fma32_against_rational_arithmetic():
    rs = np.random.RandomState(0)
    with np.errstate(all="ignore"):
        for i in range(4000):
            a, b = np.float32(rs.randn()), np.float32(rs.randn() * 10.0 ** rs.randint(-3, 4))
            kind = i % 4
            if kind == 0:                                  # ordinary magnitudes
                c = np.float32(rs.randn())
            elif kind == 1:                                # cancellation: c = -(a b) within a few ulps
                c = -np.float32(a * b) * np.float32(1.0 + rs.randint(-4, 5) * 2.0 ** -23)
            elif kind == 2:                                # the product far below c's last bit, near or on a tie
                c = np.float32(np.float64(a) * np.float64(b) * rs.choice([2.0 ** 24, 2.0 ** 25, 2.0 ** -24, 2.0 ** 29]))
            else:                                          # subnormal results
                c = np.float32(rs.randn() * 1e-38)
                a = np.float32(a * 1e-19)
                b = np.float32(rs.randn() * 1e-19)
            got, want = TM.fma32(a, b, c), _fma_rational(a, b, c)
            assert got.tobytes() == want.tobytes(), (a, b, c, got, want)
    # signs of an exact zero, infinities, NaN
    z = TM.fma32(np.float32(0.0), np.float32(-1.0), np.float32(0.0))
    assert z == 0 and not np.signbit(z)
    z = TM.fma32(np.float32(0.0), np.float32(-1.0), np.float32(-0.0))
    assert z == 0 and np.signbit(z)
    z = TM.fma32(np.float32(2.0), np.float32(-1.5), np.float32(3.0))
    assert z == 0 and not np.signbit(z)
    assert np.isinf(TM.fma32(np.float32(3e38), np.float32(2.0), np.float32(0.0)))
    assert np.isnan(TM.fma32(np.float32(np.inf), np.float32(0.0), np.float32(1.0)))
    assert TM.fma32(np.float32(np.inf), np.float32(1.0), np.float32(1.0)) == np.inf
    # point_at is three of them
    o, d, t = np.float32([0.1, -0.2, -3.0]), np.float32([0.01, 0.3, 0.95]), np.float32(2.37)
    assert TM.point_at(o, d, t).tobytes() == np.array([_fma_rational(t, d[i], o[i]) for i in range(3)], np.float32).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_every_transition_is_taken_and_no_ray_is_left_out():
    total = {False: collections.Counter(), True: collections.Counter()}
    rows = []
    for name, c in TM.CASES.items():
        for anyhit in (False, True):
            st, history = rehearse(name, anyhit)
            total[anyhit].update(st.events)
            n = st.N
            # every ray is in every comparison: it ends in a terminal state, and the evaluations add up to the counts
            assert st.status.max() <= TM.NONFINITE and len(st.status) == n == (c.n_fixed or TM.REHEARSAL_N)
            assert int(st.steps.sum()) == int(st.counts[:st.k].sum()) and st.steps.min() >= 1
            assert len(history) == st.k + 1 <= c.max_steps + 1
            assert int((st.status == TM.LIMIT).sum()) == (int(st.counts[st.k]) if st.k == c.max_steps else 0)
            if anyhit:
                assert not any(st.events[k] for k in TM.FULL_ONLY), (name, st.events)
            else:
                assert st.events["anyhit_hit"] == 0
        rows.append((name, rehearse(name, False)[0].events, rehearse(name, True)[0].events))
    print("| case | " + " | ".join(TM.TRANSITIONS) + " |")
    for name, full, anyh in rows:
        print(f"| `{name}` | " + " | ".join(str(anyh[k] if k == "anyhit_hit" else full[k]) for k in TM.TRANSITIONS) + " |")
    print("| all | " + " | ".join(str(total[k == "anyhit_hit"][k]) for k in TM.TRANSITIONS) + " |")
    for k in TM.TRANSITIONS:
        assert total[k == "anyhit_hit"][k] >= MIN_TAKEN, (k, total[k == "anyhit_hit"][k])
    for k in TM.TRANSITIONS:                              # the any-hit form takes every transition it has
        if k not in TM.FULL_ONLY:
            assert total[True][k] >= MIN_TAKEN, (k, total[True][k])
    # the cases named for a transition take it in every ray that can
    hits = lambda name: int((rehearse(name, False)[0].status == TM.HIT).sum())
    for name in ("jump@1.0", "jump@0.5", "jump@1.5"):
        ev = rehearse(name, False)[0].events
        assert ev["adjacent_end"] == hits(name) >= 24 and ev["midpoint_fallback"] >= ev["adjacent_end"]
        assert ev["hit_tol_march"] == ev["hit_tol_refine"] == 0
    assert rehearse("sphere@1.5", False)[0].events["hit_tol_refine"] == hits("sphere@1.5") >= 24
    st = rehearse("min_step", False)[0]
    assert st.events["march_step"] == 0 and st.events["min_step"] == int(st.steps.sum()) and (st.status == TM.MISS).all()
    st = rehearse("limit1024", False)[0]
    assert (st.status == TM.LIMIT).all() and (st.steps == 1024).all() and st.counts[1024] == 8 == st.N and st.k == 1024
    for name in ("far_exact@1.0", "far_exact@0.5"):
        st = rehearse(name, False)[0]
        assert st.events["far_equal_alive"] == st.N and (st.status == TM.MISS).all()
    assert rehearse("inf_core", False)[0].events["nonfinite_march"] >= MIN_TAKEN
    assert rehearse("nan_ball", False)[0].events["nonfinite_refine"] >= MIN_TAKEN
    ev = rehearse("start_inside", False)[0].events
    assert ev["start_inside"] >= MIN_TAKEN and ev["hit_tol_first_negative"] >= MIN_TAKEN


def test_bound_policies_and_batches_cover_the_cases():
    assert {c.policy for c in TM.CASES.values()} == {"exact", "N", "third"}
    assert {n for pair in TM.BATCHES for n in pair} == set(TM.CASES)
    for a, b in TM.BATCHES:
        assert TM.CASES[a].omega == TM.CASES[b].omega and TM.CASES[a].tol == TM.CASES[b].tol and TM.CASES[a].field_name != "away"
        assert len({TM.CASES[a].field_name, TM.CASES[b].field_name, TM.AWAY.field_name}) == 3      # a different field per element
        assert TM.CASES[a].max_steps <= TM.CASES[b].max_steps or TM.CASES[a].n_fixed
    c = TM.CASES["jump@1.5"]
    bounds, previous = [], 600
    for k, count in enumerate([600, 410, 300, 220, 150, 90, 40]):
        previous = c.bound(k, count, 600, previous)
        bounds.append(previous)
    assert bounds == [600, 600, 600, 220, 220, 220, 40]           # refreshed every third step, stale in between
    assert TM.CASES["jump@0.5"].bound(5, 3, 600, 600) == 600 and TM.CASES["jump@1.0"].bound(5, 3, 600, 9) == 3
    # the away element ends on its first step
    st, _ = TM.run32(TM.AWAY, 64, False)
    assert st.k == 1 and (st.status == TM.MISS).all() and (st.steps == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# against the float64 tracers
# ---------------------------------------------------------------------------------------------------------------------
CONDITIONED = [n for n, c in TM.CASES.items() if c.conditioned]
GUARD, T_BAR = 1e-6, 1e-5


@pytest.mark.parametrize("anyhit", [False, True], ids=["full", "anyhit"])
@pytest.mark.parametrize("name", CONDITIONED)
def test_agrees_with_the_float64_tracers(name, anyhit):
    """Equal status for every ray whose float64 samples all keep ||s| - tol| > 1e-6, and |t32 - t64| <= 1e-5 on hits."""
    c = TM.CASES[name]
    st, _ = rehearse(name, anyhit)
    o, d, near, far = (a.astype(np.float64) for a in c.rays(st.N))
    ref = OC.trace_anyhit if anyhit else T.trace
    compared, worst = 0, 0.0
    for r in range(st.N):
        margin = [np.inf]

        def field(p):
            s = c.field64(p)
            margin[0] = min(margin[0], float(np.abs(np.abs(s) - c.tol).min()))
            return s
        t64, s64, _, _ = ref(field, o[r:r + 1], d[r:r + 1], near[r:r + 1], far[r:r + 1], tol=c.tol, omega=c.omega, max_steps=c.max_steps)
        if margin[0] <= GUARD:
            continue
        compared += 1
        assert st.status[r] == s64[0], (name, r, st.status[r], s64[0])
        if s64[0] == TM.HIT:
            worst = max(worst, abs(float(st.t[r]) - t64[0]))
    print(f"{name} {'anyhit' if anyhit else 'full'}: {compared} of {st.N} rays compared, worst |t32 - t64| on hits {worst:.3e}")
    assert compared >= 0.9 * st.N
    assert worst <= T_BAR


# ---------------------------------------------------------------------------------------------------------------------
# against closed forms
# ---------------------------------------------------------------------------------------------------------------------
IMPACT = 0.6 * TM.R


@pytest.mark.parametrize("name", [n for n, c in TM.CASES.items() if c.slope is not None])
def test_radial_hits_lie_at_the_ray_sphere_root(name):
    """A HIT has |f32(field(p))| <= tol at the float32 point p = fmaf(t, d, o), whose components are each within 2^-24 |p| of
    o + t d; the field's slope in p is at most `hi`, so the exact field along the ray is within tol + hi sqrt(3) 2^-24 |p| of 0 at
    t (the field's own rounding, 2^-24 tol, is nothing).  Along the ray the field's slope is at least m = lo cos, cos =
    sqrt(1 - (b / r)^2) >= sqrt(1 - (b / (R - 1e-4))^2) for a point within 1e-4 of the sphere, which every point with |field|
    <= 2e-5 is (lo >= 1); b <= 0.6 R gives cos >= 0.8 and hi sqrt(3) / m <= 2.8 x 1.74 / 0.8 < 8.  So
    |t - root| <= tol / m + 8 x 2^-24 max|p|."""
    c = TM.CASES[name]
    lo, hi = c.slope
    assert lo >= 1.0 and hi * np.sqrt(3.0) / (lo * 0.8) < 8.0
    checked = 0
    for anyhit in (False, True):
        st, _ = rehearse(name, anyhit)
        o, d, near, far = c.rays(st.N)
        root, b = TM.sphere_root(o, d)
        sel = (st.status == TM.HIT) & (b <= IMPACT)
        if anyhit:                                       # an occluder's t is a sample inside the body, not the root
            sel &= np.array([abs(float(v)) <= c.tol for v in c.field(np.stack([TM.point_at(o[r], d[r], st.t[r]) for r in range(st.N)]))])
        m = lo * np.sqrt(np.maximum(1.0 - (b / (TM.R - 1e-4)) ** 2, 0.64))       # (0.64: the rays outside `sel`, not judged)
        pmax = np.abs(o.astype(np.float64) + st.t.astype(np.float64)[:, None] * d.astype(np.float64)).max(-1)
        bound = c.tol / m + 8 * 2.0 ** -24 * pmax
        err = np.abs(st.t.astype(np.float64) - root)
        print(name, "anyhit" if anyhit else "full", "hits checked", int(sel.sum()), "worst |t - root| / bound", float((err / bound)[sel].max(initial=0.0)))
        assert (err[sel] <= bound[sel]).all()
        checked += int(sel.sum())
    assert checked >= MIN_TAKEN


@pytest.mark.parametrize("name", ["jump@1.0", "jump@0.5", "jump@1.5"])
def test_jump_hits_lie_at_the_ray_sphere_root(name):
    """The bracket ends as adjacent float32 numbers whose points lie on either side of the sphere: t_hi is within one ulp of
    t <= 4 (2.4e-7) of a t whose ROUNDED point changes side, and rounding moves a point by at most sqrt(3) 2^-24 |p| < 3 x 2^-24
    |p|, which is 3 x 2^-24 |p| / cos along the ray: 1.2e-7 at cos >= 0.8 (b <= 0.6 R).  2e-6 holds both with room."""
    c = TM.CASES[name]
    st, _ = rehearse(name, False)
    o, d, _, _ = c.rays(st.N)
    root, b = TM.sphere_root(o, d)
    sel = (st.status == TM.HIT) & (b <= IMPACT)
    err = np.abs(st.t.astype(np.float64) - root)[sel]
    print(name, "hits checked", int(sel.sum()), "worst |t - root|", float(err.max(initial=0.0)))
    assert sel.sum() >= MIN_TAKEN and (err <= 2e-6).all()
    assert float(st.t[sel].max()) <= 4.0


# ---------------------------------------------------------------------------------------------------------------------
# mutations
# ---------------------------------------------------------------------------------------------------------------------
def test_caught_by_names_every_mutation():
    assert set(TM.CAUGHT_BY) == set(TM.MUTATIONS) and all(set(v) <= set(TM.CASES) and v for v in TM.CAUGHT_BY.values())


@pytest.mark.parametrize("mutation,name", [(m, n) for m in TM.MUTATIONS for n in TM.CAUGHT_BY[m]])
def test_mutation_is_caught(mutation, name):
    """The mutated restatement differs from the true one in a word the GPU test compares: (t, status, steps) of a ray or the
    in-flight state (the set in flight, bracket, side) after some step."""
    c = TM.CASES[name]
    anyhit = mutation == "anyhit_refines"
    st, history = rehearse(name, anyhit)
    mt, mhistory = TM.run32(c, st.N, anyhit, mutate=mutation)
    final = lambda s: (s.t.tobytes(), s.status.tobytes(), s.steps.tobytes())
    first = next((k for k, (a, b) in enumerate(zip(history, mhistory)) if a != b), None)
    rays = int(((st.t != mt.t) | (st.status != mt.status) | (st.steps != mt.steps)).sum())
    print(mutation, name, "first differing step", first, "rays with other final words", rays)
    assert first is not None or len(history) != len(mhistory) or final(st) != final(mt)


def test_mutations_spare_the_cases_that_do_not_reach_their_line():
    """The other direction, so CAUGHT_BY is not vacuous: a mutation of the REFINE phase leaves a case without a bracket bit for
    bit alone."""
    for mutation in ("wrong_end_halved", "no_midpoint", "hit_at_t_lo", "t_hi_where_t_lo", "side_not_stored"):
        st, history = rehearse("far_exact@1.0", False)
        mt, mhistory = TM.run32(TM.CASES["far_exact@1.0"], st.N, False, mutate=mutation)
        assert history == mhistory
