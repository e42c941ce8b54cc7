"""The ray state machine of csrc/trace_common.h (trace_step_rays<ANYHIT>, point_at; include/oi_trace.h:23-37), restated
one step at a time in float32 with the kernel's operations in the kernel's order, and the fields, rays and cases on which
tests/test_trace_machine_cpu.py rehearses it and tests/test_gpu_trace_machine.py holds the four step entries to it bit for
bit.  Plain numpy, nothing of oi_amd.

* `fma32(a, b, c)`: the fused multiply-add of three float32 numbers, EXACT: the sum a b + c is formed as an integer over a power
  of two (Python integers) and rounded once, to nearest even, subnormals and overflow included.  A float64 product and sum
  rounded to float32 rounds twice; tests/test_trace_machine_cpu.py shows a triple on which that differs.
* `begin32`, `step32`, `finish32`: oi_trace_begin, one oi_trace_step / oi_occlusion_step, oi_trace_finish.  Every other
  operation is a single float32 operation of numpy's float32 scalars, which round as the device does: `fabsf(v) <= tol`,
  `t += fmaxf(omega * v, tol)` with the product rounded on its own, `t > far`, `s_lo / (s_lo - s_hi)` as an IEEE division (the
  build passes no fast-math flag), `fmaf(t_hi - t_lo, q, t_lo)`, `0.5f * (t_lo + t_hi)`, the two strict-inside tests, the
  halvings, and the sample point `fmaf(t, d, o)` per component.  The state is the kernel's: t, status, steps, bracket[4], side
  per ray, the rays in flight (ascending: the header leaves the slot order open) and counts[k].  `events` counts the
  transitions taken.
* `FIELDS`: plain functions of float32 points, evaluated in float64 and rounded to float32.  The same array goes to the kernel
  and to the restatement, so the field's own accuracy does not matter.
* `CASES`: a field with rays, tol, omega, a step limit and a bound policy ("exact": counts[k] every step, "N": N always,
  "third": refreshed every third step).  `BATCHES`: E = 3 elements with a different field each; the middle one (a constant
  field of 50) ends every ray on its first step and rides along.
* `MUTATIONS`: one wrong line each of `step32`; `CAUGHT_BY` names the case whose bit comparison exposes each one (rehearsed
  on the CPU).

What the comparison found on the MI355X: nothing.  All four entries match the restatement in every word of every step in every
case, size and bound policy; the two branches that had never run under a test that would notice (the mid-point fall-back and
the adjacent-numbers ending) do what the header says, and so does the Illinois bookkeeping.  No kernel was changed.

Rays are tests/test_gpu_trace.py::_bundle's 'mixed' kind (from 3 units away at a disc of radius 0.9) with near / far = the
closest approach -+ 1, so the sphere of radius 0.5 the fields are built on is met by a third of them.
"""
import collections
import math
import types

import numpy as np

MISS, HIT, LIMIT, START_INSIDE, NONFINITE = 0, 1, 2, 3, 4          # OI_TRACE_* of include/oi_trace.h
MARCH, REFINE = 16, 17
MAX_STEPS, COUNT_WORDS = 1024, 1026
F32 = np.float32
TOL = 1e-5
R = 0.5                     # the radius every field is built on
SEED = 3

TRANSITIONS = ("hit_tol_march", "hit_tol_refine", "hit_tol_first_negative", "march_step", "min_step", "miss", "far_equal_alive",
               "start_inside", "nonfinite_march", "nonfinite_refine", "bracket_closure", "lo_replaced", "hi_replaced", "lo_halved",
               "hi_halved", "midpoint_fallback", "adjacent_end", "anyhit_hit", "limit")
FULL_ONLY = ("hit_tol_refine", "nonfinite_refine", "bracket_closure", "lo_replaced", "hi_replaced", "lo_halved", "hi_halved",
             "midpoint_fallback", "adjacent_end")


# ---------------------------------------------------------------------------------------------------------------------
# exact fused multiply-add
# ---------------------------------------------------------------------------------------------------------------------
def _round_to_f32(num, k):
    """num / 2^k (integers, num != 0) rounded once to the nearest float32, ties to even."""
    a = abs(num)
    e_lsb = max(a.bit_length() - 24 - k, -149)          # exponent of the last kept bit (-149: the subnormals' spacing)
    shift = e_lsb + k
    if shift <= 0:
        q = a << -shift
    else:
        q, rem, half = a >> shift, a & ((1 << shift) - 1), 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
    if q.bit_length() + e_lsb > 128:
        return math.copysign(math.inf, num)
    return math.copysign(math.ldexp(float(q), e_lsb), num)   # q <= 2^24: exact in float64, and a float32 number


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 numbers, exactly rounded."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))      # inf / NaN: the product is exact or special, so is the sum
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    num = na * nb * dc + nc * da * db
    if num == 0:
        return F32(a * b + c)                            # an exact zero: its sign is IEEE's, and a * b is exact in float64
    return F32(_round_to_f32(num, (da * db * dc).bit_length() - 1))


def point_at(o, d, t):
    """point_at of trace_common.h: fmaf(t, d, o) per component.  o, d (3,) float32 -> (3,) float32."""
    return np.array([fma32(t, d[0], o[0]), fma32(t, d[1], o[1]), fma32(t, d[2], o[2])], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the machine
# ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("wrong_end_halved", "side_not_stored", "ge_at_far", "no_min_step", "t_hi_where_t_lo", "no_midpoint", "hit_at_t_lo",
             "steps_not_on_last", "nonfinite_after_tol", "anyhit_refines")


def begin32(o, d, near, far):
    """oi_trace_begin: t = near, MARCH, steps 0, bracket (near, 0, near, 0), side 0, every ray active, counts[0] = N."""
    o, d = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    n = len(o)
    st = types.SimpleNamespace(N=n, o=o, d=d, near=np.asarray(near, dtype=np.float32).reshape(n).copy(),
                               far=np.asarray(far, dtype=np.float32).reshape(n).copy())
    st.t = st.near.copy()
    st.status = np.full(n, MARCH, dtype=np.uint8)
    st.steps = np.zeros(n, dtype=np.uint16)
    st.bracket = np.zeros((n, 4), dtype=np.float32)
    st.bracket[:, 0] = st.bracket[:, 2] = st.near
    st.side = np.zeros(n, dtype=np.uint8)
    st.active = np.arange(n, dtype=np.int64)
    st.points = np.stack([point_at(o[r], d[r], st.t[r]) for r in range(n)]) if n else np.zeros((0, 3), np.float32)
    st.counts = np.zeros(COUNT_WORDS, dtype=np.int32)
    st.counts[0] = n
    st.k = 0
    st.events = collections.Counter()
    return st


def step32(st, sdf_of_slot, k, tol, omega, anyhit, mutate=None):
    """Step k of trace_step_rays<anyhit> (trace_common.h:138-220) on sdf_of_slot[j] = the sdf at st.points[j], the sample of ray
    st.active[j].  Updates st in place: the per-ray words, the rays in flight (ascending), their points and counts[k + 1]."""
    assert k == st.k and 0 <= k < MAX_STEPS and (mutate is None or mutate in MUTATIONS)
    tol, omega = F32(tol), F32(omega)
    sdf = np.asarray(sdf_of_slot, dtype=np.float32).reshape(-1)
    assert len(sdf) >= len(st.active)
    ev, alive, half = st.events, [], F32(0.5)
    with np.errstate(all="ignore"):
        for j, r in enumerate(st.active):
            v, t, status = sdf[j], st.t[r], int(st.status[r])
            n_eval = int(st.steps[r]) + 1
            live = False
            finite = bool(np.isfinite(v))
            if mutate == "nonfinite_after_tol":                      # the tolerance first, as !(|v| > tol): a NaN is a HIT
                within = not abs(v) > tol
                finite = finite or within
            else:
                within = finite and bool(abs(v) <= tol)
            if not finite:
                ev["nonfinite_march" if status == MARCH else "nonfinite_refine"] += 1
                status = NONFINITE
            elif within:
                ev["hit_tol_march" if status == MARCH else "hit_tol_refine"] += 1
                if status == MARCH and n_eval == 1 and v < 0:
                    ev["hit_tol_first_negative"] += 1
                status = HIT
            elif status == MARCH and v > 0:
                if not anyhit:
                    st.bracket[r, 0], st.bracket[r, 1] = t, v
                step = omega * v                                      # rounded on its own
                ev["min_step" if step < tol else "march_step"] += 1
                t = t + (step if mutate == "no_min_step" else max(step, tol))
                if (t >= st.far[r]) if mutate == "ge_at_far" else (t > st.far[r]):
                    ev["miss"] += 1
                    status = MISS
                else:
                    live = True
                    if t == st.far[r]:
                        ev["far_equal_alive"] += 1
            elif status == MARCH and n_eval == 1:
                ev["start_inside"] += 1
                status = START_INSIDE
            elif anyhit and mutate != "anyhit_refines":
                ev["anyhit_hit"] += 1
                status = HIT
            else:
                t_lo, s_lo = st.bracket[r, 0], st.bracket[r, 1]
                side = 0
                if status == MARCH:                                   # the first negative sample closes the bracket
                    ev["bracket_closure"] += 1
                    t_hi, s_hi, status = t, v, REFINE
                else:
                    t_hi, s_hi, side = st.bracket[r, 2], st.bracket[r, 3], int(st.side[r])
                    if v > 0:
                        ev["lo_replaced"] += 1
                        if side == 1:
                            ev["hi_halved"] += 1
                            if mutate != "wrong_end_halved":
                                s_hi = s_hi * half
                        t_lo, s_lo, side = t, v, 1
                        if mutate == "wrong_end_halved" and int(st.side[r]) == 1:
                            s_lo = s_lo * half
                    else:
                        ev["hi_replaced"] += 1
                        if side == 2:
                            ev["lo_halved"] += 1
                            if mutate != "wrong_end_halved":
                                s_lo = s_lo * half
                        t_hi, s_hi, side = t, v, 2
                        if mutate == "wrong_end_halved" and int(st.side[r]) == 2:
                            s_hi = s_hi * half
                t = fma32(t_hi - t_lo, s_lo / (s_lo - s_hi), t_lo)
                if not (t > t_lo and t < t_hi) and mutate != "no_midpoint":
                    ev["midpoint_fallback"] += 1
                    t = half * (t_lo + t_hi)
                if not (t > t_lo and t < t_hi):                       # the ends are adjacent numbers
                    ev["adjacent_end"] += 1
                    t = t_lo if mutate == "hit_at_t_lo" else t_hi
                    status = HIT
                else:
                    live = True
                    st.bracket[r] = (t_hi if mutate == "t_hi_where_t_lo" else t_lo, s_lo, t_hi, s_hi)
                    if mutate != "side_not_stored":
                        st.side[r] = side
            if live or mutate != "steps_not_on_last":
                st.steps[r] = n_eval
            st.t[r], st.status[r] = t, status
            if live:
                alive.append(r)
    st.active = np.array(alive, dtype=np.int64)
    st.points = np.stack([point_at(st.o[r], st.d[r], st.t[r]) for r in alive]) if alive else np.zeros((0, 3), np.float32)
    st.counts[k + 1] = len(alive)
    st.k = k + 1
    return st


def finish32(st):
    """oi_trace_finish: rays in flight -> LIMIT; -> the hit rays (ascending) and their points, point_at at the final t."""
    flying = st.status >= MARCH
    st.events["limit"] += int(flying.sum())
    st.status[flying] = LIMIT
    st.active = np.zeros(0, dtype=np.int64)
    hits = np.nonzero(st.status == HIT)[0]
    st.hit_index = hits
    st.hit_points = np.stack([point_at(st.o[r], st.d[r], st.t[r]) for r in hits]) if len(hits) else np.zeros((0, 3), np.float32)
    st.counts[COUNT_WORDS - 1] = len(hits)
    return st


def snapshot(st):
    """The words the header's contract covers, as bytes: t, status, steps of every ray, the rays in flight, their bracket and
    side."""
    a = st.active
    return (st.t.tobytes(), st.status.tobytes(), st.steps.tobytes(), a.tobytes(), st.bracket[a].tobytes(), st.side[a].tobytes())


def run32(case, n, anyhit, mutate=None, max_steps=None):
    """A whole trace of `case` on n rays through the restatement alone.  -> the finished state and one snapshot per step."""
    o, d, near, far = case.rays(n)
    st = begin32(o, d, near, far)
    history = [snapshot(st)]
    limit = case.max_steps if max_steps is None else max_steps
    while len(st.active) and st.k < limit:
        step32(st, case.field(st.points), st.k, case.tol, case.omega, anyhit, mutate)
        history.append(snapshot(st))
    return finish32(st), history


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
def bundle(n, seed=SEED):
    """tests/test_gpu_trace.py::_bundle(n, seed, 'mixed') as float32 numpy, with near / far = the closest approach -+ 1."""
    rs = np.random.RandomState(seed)
    o = np.tile(np.array([[0.0, 0.0, -3.0]]), (n, 1)) + 0.02 * rs.randn(n, 3)
    ang = rs.rand(n) * 2 * np.pi
    rad = 0.9 * np.sqrt(rs.rand(n))
    d = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.zeros(n)], -1) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o, d = o.astype(np.float32), d.astype(np.float32)
    mid = closest_approach(o, d)
    return o, d, (mid - 1.0).astype(np.float32), (mid + 1.0).astype(np.float32)


def closest_approach(o, d):
    o, d = o.astype(np.float64), d.astype(np.float64)
    return -(o * d).sum(-1) / (d * d).sum(-1)


def sphere_root(o, d, radius=R):
    """float64: the first root of |o + t d| = radius (NaN for a ray that passes the sphere) and the ray's impact parameter."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    a, b, c = (d * d).sum(-1), (o * d).sum(-1), (o * o).sum(-1) - radius * radius
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        root = (-b - np.sqrt(disc)) / a
    return root, np.sqrt(np.maximum((o * o).sum(-1) - b * b / a, 0.0))


# ---------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------
BAND, STEEP = 0.05, 2.8          # slope 2.8 (the header's figure) within 0.05 of the surface, slope 1 outside
INF_CORE = 0.47
NAN_DEPTH, NAN_CENTRE, NAN_RADIUS = 0.02, np.array([0.0, 0.0, -R]), 0.35


def _radius(p):
    return np.linalg.norm(np.asarray(p, dtype=np.float64), axis=-1)


def _band_g(u):
    return np.where(np.abs(u) < BAND, STEEP * u, u + np.sign(u) * (STEEP - 1.0) * BAND)


def sphere64(p):
    return _radius(p) - R


def jump64(p):
    return np.where(_radius(p) > R, 0.3, -0.3)


def ripple64(p):
    p = np.asarray(p, dtype=np.float64)
    return _radius(p) - R + 0.12 * np.sin(25.0 * p[..., 0]) * np.cos(19.0 * p[..., 1])


def band64(p):
    return _band_g(_radius(p) - R)


def inf_core64(p):
    r = _radius(p)
    return np.where(r < INF_CORE, np.inf, _band_g(r - R))


def nan_ball64(p):
    """The jump, with NaN in the part of a ball about the sphere's near pole that lies less than NAN_DEPTH under the surface:
    marching steps of 0.3 seldom land there, the shrinking bracket's negative samples always do."""
    p = np.asarray(p, dtype=np.float64)
    r = _radius(p)
    bad = (r < R) & (r > R - NAN_DEPTH) & (np.linalg.norm(p - NAN_CENTRE, axis=-1) < NAN_RADIUS)
    return np.where(bad, np.nan, jump64(p))


def _const(c):
    return lambda p: np.full(len(p), c, dtype=np.float64)


FIELDS64 = {"sphere": sphere64, "jump": jump64, "ripple": ripple64, "band": band64, "inf_core": inf_core64, "nan_ball": nan_ball64,
            "const_2e-5": _const(2e-5), "const_0.25": _const(0.25), "away": _const(50.0)}


def _f32(fn):
    def field(p):
        with np.errstate(all="ignore"):
            return np.asarray(fn(np.asarray(p, dtype=np.float32).reshape(-1, 3)), dtype=np.float64).astype(np.float32)
    return field


FIELDS = {k: _f32(v) for k, v in FIELDS64.items()}


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def _plain(o, d, near, far):
    return near, far


def _short(length):
    return lambda o, d, near, far: (near, (near.astype(np.float64) + length).astype(np.float32))


def _unit(o, d, near, far):
    return np.zeros_like(near), np.ones_like(far)


def _inside(o, d, near, far):
    """Of the rays that meet the sphere, the even ones start 4e-6 behind the surface (the first sample is negative and within
    tol: HIT wins over START_INSIDE), the odd ones 0.8 further along than usual (those with a chord longer than 0.4 start
    inside the body)."""
    root, _ = sphere_root(o, d)
    meets = np.isfinite(root)
    even = (np.arange(len(near)) % 2) == 0
    n64 = near.astype(np.float64)
    n64 = np.where(meets & even, root + 4e-6, np.where(meets, n64 + 0.8, n64))
    return n64.astype(np.float32), far


class Case:
    def __init__(self, name, field, omega, max_steps=160, policy="exact", window=_plain, n_fixed=None, tol=TOL, conditioned=False,
                 slope=None):
        self.name, self.field_name, self.field, self.field64 = name, field, FIELDS[field], FIELDS64[field]
        self.omega, self.tol, self.max_steps, self.policy, self.window, self.n_fixed = omega, tol, max_steps, policy, window, n_fixed
        self.conditioned = conditioned          # no jump, no non-finite value: compared with the float64 tracers
        self.slope = slope                      # radial fields: (smallest, largest) d field / d radius at the surface
        self._rays = {}

    def rays(self, n):
        """o, d (n, 3), near, far (n,) float32; computed once per n and never modified."""
        if n not in self._rays:
            o, d, near, far = bundle(n)
            near, far = self.window(o, d, near, far)
            for a in (o, d, near, far):
                a.setflags(write=False)
            self._rays[n] = (o, d, near, far)
        return self._rays[n]

    def bound(self, k, count, n, previous):
        """The `bound` argument of step k: count = counts[k] (live[k] for a batch), previous = step k - 1's bound."""
        if self.policy == "N":
            return n
        if self.policy == "third" and k % 3 != 0:
            return previous
        return count


CASES = {c.name: c for c in (
    Case("jump@1.0", "jump", 1.0, policy="exact"),
    Case("jump@0.5", "jump", 0.5, policy="N"),
    Case("jump@1.5", "jump", 1.5, policy="third"),
    Case("sphere@1.5", "sphere", 1.5, policy="third", conditioned=True, slope=(1.0, 1.0)),
    Case("ripple@1.0", "ripple", 1.0, policy="exact", conditioned=True),
    Case("ripple@1.5", "ripple", 1.5, policy="N", conditioned=True),
    Case("ripple_cut", "ripple", 1.5, max_steps=4, policy="exact"),
    Case("band@1.0", "band", 1.0, policy="third", conditioned=True, slope=(1.0, STEEP)),
    Case("min_step", "const_2e-5", 0.25, max_steps=64, policy="exact", window=_short(3e-4)),
    Case("limit1024", "const_2e-5", 0.25, max_steps=1024, policy="third", window=_short(0.02), n_fixed=8),
    Case("sphere@0.25", "sphere", 0.25, policy="N", conditioned=True, slope=(1.0, 1.0)),
    Case("far_exact@1.0", "const_0.25", 1.0, policy="N", window=_unit),
    Case("far_exact@0.5", "const_0.25", 0.5, policy="third", window=_unit),
    Case("inf_core", "inf_core", 1.0, policy="exact"),
    Case("nan_ball", "nan_ball", 1.0, policy="N"),
    Case("start_inside", "sphere", 1.0, policy="third", window=_inside, conditioned=True, slope=(1.0, 1.0)),
)}
AWAY = Case("away", "away", 1.0)      # every ray misses on its first sample

# E = 3: (first, last) share omega, the step limit is the first one's and the two fields differ; the middle element is AWAY.
# Every case is in one of them.
BATCHES = (("jump@1.0", "ripple@1.0"), ("band@1.0", "inf_core"), ("far_exact@1.0", "start_inside"), ("nan_ball", "jump@1.0"),
           ("jump@1.5", "sphere@1.5"), ("ripple@1.5", "sphere@1.5"), ("ripple_cut", "jump@1.5"), ("jump@0.5", "far_exact@0.5"),
           ("limit1024", "sphere@0.25"), ("min_step", "sphere@0.25"))

SIZES = (1, 64, 257, 600)             # 600: three workgroups of 256
REHEARSAL_N = 96

# the case whose bit comparison exposes each mutation (tests/test_trace_machine_cpu.py rehearses every pair)
CAUGHT_BY = {
    "wrong_end_halved": ("jump@1.0", "jump@0.5", "jump@1.5", "ripple@1.0"),
    "side_not_stored": ("jump@1.0", "jump@1.5", "ripple@1.5"),
    "ge_at_far": ("far_exact@1.0", "far_exact@0.5"),
    "no_min_step": ("min_step", "limit1024"),
    "t_hi_where_t_lo": ("jump@1.0", "sphere@1.5", "band@1.0"),
    "no_midpoint": ("jump@1.0", "jump@0.5", "jump@1.5"),
    "hit_at_t_lo": ("jump@1.0", "jump@0.5", "jump@1.5"),
    "steps_not_on_last": ("sphere@1.5", "far_exact@1.0", "start_inside"),
    "nonfinite_after_tol": ("nan_ball",),
    "anyhit_refines": ("jump@1.0", "sphere@1.5", "band@1.0"),      # the any-hit form
}
