"""The ray state machine on the MI355X, one step at a time and bit for bit: the four C entries that run trace_step_rays
(csrc/trace_common.h) -- oi_trace_step, oi_occlusion_step, oi_trace_batch_step, oi_trace_batch_step_anyhit -- on guarded
buffers through the C ABI, against the float32 restatement of tests/helpers/trace_machine.py.  The sdf is an input of the step
entries: the host evaluates the case's field at the points the kernel left, uploads it, and gives the same numbers to the
restatement, so every word the kernel must produce is known.  After EVERY step t, status and steps of every ray, bracket and side
of the rays in flight, counts, live, the active list (as a set) and the compacted points are compared with no tolerance; after
the finish entry the LIMIT states, hit_slot, the hit list (as a set) and the hit points.  The cases and what each is for:
tests/helpers/trace_machine.py, rehearsed by tests/test_trace_machine_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import guarded
from helpers import trace_machine as TM
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

# entry -> (any-hit form, batched)
ENTRIES = {"oi_trace_step": (False, False), "oi_occlusion_step": (True, False), "oi_trace_batch_step": (False, True),
           "oi_trace_batch_step_anyhit": (True, True)}
W = TM.COUNT_WORDS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _p(t_):
    return ctypes.c_void_p(t_.data_ptr())


class Device:
    """The arrays of E elements of N rays (include/oi_trace_batch.h's layout; E = 1 is include/oi_trace.h's state) in guarded,
    poisoned buffers, and the entries of one form."""

    def __init__(self, entry, rays):
        from oi_amd import lib, ops
        self.entry, (self.anyhit, self.batch) = entry, ENTRIES[entry]
        self.L, self.lib, self.stream = lib.load(), lib, ops._stream()
        self.E, self.N = len(rays), len(rays[0][0])
        E, N = self.E, self.N
        assert self.batch or E == 1
        g = lambda sh, dt=torch.float32, what="?", mw=True: guarded_empty(sh, dt, what=what, must_write=mw)
        up = lambda i, what: guarded_copy(torch.from_numpy(np.stack([r[i] for r in rays])).cuda(), what)
        # (the 16-bit step counts and the partly written lists carry guards only: tests/test_gpu_trace.py::_guarded_pass)
        self.arr = dict(rays_o=up(0, "rays_o"), rays_d=up(1, "rays_d"), near_=up(2, "near"), far_=up(3, "far"), t=g((E, N), what="t"),
                        status=g((E, N), torch.uint8, "status"), steps=g((E, N), torch.int16, "steps", False),
                        bracket=g((E, N, 4), what="bracket"), side=g((E, N), torch.uint8, "side"),
                        active=g((E, 2, N), torch.int32, "active", False), points=g((E, N, 3), what="points"),
                        counts=g((E, W), torch.int32, "counts"))
        self.live = g((W,), torch.int32, "live") if self.batch else None
        S = lib.TraceState()
        S.N = N
        for k_, v_ in self.arr.items():
            setattr(S, k_, _p(v_))
        if self.batch:
            self.c = lib.TraceBatch()
            self.c.s, self.c.E, self.c.live = S, E, _p(self.live)
        else:
            self.c = S
        self.ref = ctypes.byref(self.c)

    def begin(self):
        return (self.L.oi_trace_batch_begin if self.batch else self.L.oi_trace_begin)(self.ref, self.stream)

    def step(self, sdf, bound, k, tol, omega):
        return getattr(self.L, self.entry)(self.ref, _p(sdf), int(bound), int(k), float(tol), float(omega), self.stream)

    def read(self):
        out = {k: v.cpu().numpy() for k, v in self.arr.items() if k not in ("rays_o", "rays_d", "near_", "far_")}
        out["live"] = self.live.cpu().numpy() if self.batch else out["counts"].max(0)
        return out


def compare(dev, states, k, where):
    """The device's words against the restatements' after k steps.  -> nothing; fails with the number of differing words."""
    d = dev.read()
    bad = []

    def same(what, e, got, want):
        got, want = _bits(got), _bits(want)
        n = int((got != want).sum()) if got.shape == want.shape else -1
        if n:
            idx = np.argwhere(got != want)[:4].tolist() if n > 0 else "shape"
            bad.append(f"{what}[e={e}]: {n} word(s) differ, first at {idx}")

    for e, st in enumerate(states):
        assert st.k == k
        a = st.active
        same("t", e, d["t"][e], st.t)
        same("status", e, d["status"][e], st.status)
        same("steps", e, d["steps"][e].astype(np.uint16), st.steps)
        same("side of the rays in flight", e, d["side"][e][a], st.side[a])
        if not dev.anyhit:
            same("bracket of the rays in flight", e, d["bracket"][e][a], st.bracket[a])
        same("counts", e, d["counts"][e], st.counts)                 # counts[k] = the rays in flight, later words 0
        act = d["active"][e, k & 1, :len(a)].astype(np.int64)
        order = np.argsort(act, kind="stable")
        same("active (as a set)", e, act[order], a)
        same("points", e, d["points"][e, :len(a)][order], st.points)
    live = np.max([st.counts for st in states], axis=0)
    same("live", "-", d["live"], live)
    assert not bad, f"{dev.entry} {where}, after {k} step(s):\n  " + "\n  ".join(bad)


def drive(entry, cases, N, max_steps):
    """The loop of the header through the C ABI: begin, then per step read the points back, evaluate each element's field on
    the host, upload, step, compare; then the finish entry (and the gather for a batch)."""
    anyhit, batch = ENTRIES[entry]
    lead = cases[0]
    where = f"[{', '.join(c.name for c in cases)}; N={N}]"
    rays = [c.rays(N) for c in cases]
    dev = Device(entry, rays)
    E = dev.E
    states = [TM.begin32(*r) for r in rays]
    assert dev.begin() == 0
    compare(dev, states, 0, where)
    bound, k = N, 0
    while k < max_steps:
        count = max(len(st.active) for st in states)                  # == counts[k] / live[k] on the device: just compared
        if count == 0:
            break
        bound = lead.bound(k, count, N, bound)
        assert count <= bound <= N
        pts = dev.arr["points"][:, :bound].cpu().numpy()
        act = dev.arr["active"][:, k & 1].cpu().numpy()
        host = np.full((E, N), np.nan, dtype=np.float32)              # past the bound: never read
        for e, c in enumerate(cases):
            host[e, :bound] = c.field(pts[e])                         # stale slots (count_e .. bound) hold earlier, valid points
        sdf = guarded_copy(torch.from_numpy(host if batch else host[0, :bound].copy()).cuda(), "sdf")
        assert dev.step(sdf, bound, k, lead.tol, lead.omega) == 0, dev.L.oi_last_error()
        for e, st in enumerate(states):
            slot_of = np.empty(N, dtype=np.int64)
            slot_of[act[e, :len(st.active)]] = np.arange(len(st.active))
            TM.step32(st, host[e, slot_of[st.active]], k, lead.tol, lead.omega, anyhit)
        k += 1
        compare(dev, states, k, where)
        guarded.current().maybe_flush()
    return dev, states, k, where


def finish(dev, states, k, where):
    g = lambda sh, dt=torch.float32, what="?", mw=True: guarded_empty(sh, dt, what=what, must_write=mw)
    E, N, L = dev.E, dev.N, dev.L
    hit_index, hit_slot = g((E, N), torch.int32, "hit_index", False), g((E, N), torch.int32, "hit_slot")
    hit_points = None
    if dev.batch:
        assert L.oi_trace_batch_finish(dev.ref, _p(hit_index), _p(hit_slot), dev.stream) == 0
    else:
        hit_points = g((N, 3), what="hit_points", mw=False)
        assert L.oi_trace_finish(dev.ref, _p(hit_index), _p(hit_points), _p(hit_slot), dev.stream) == 0
    for st in states:
        TM.finish32(st)
    d = dev.read()
    n_hit = [len(st.hit_index) for st in states]
    assert d["counts"][:, -1].tolist() == n_hit, where
    assert int(d["live"][-1]) == max(n_hit)
    n_pad = max(n_hit)
    if dev.batch and n_pad:
        padded = g((E, n_pad, 3), what="hit_points_padded")
        assert L.oi_trace_batch_gather(dev.ref, _p(hit_index), n_pad, _p(padded), dev.stream) == 0
        padded = padded.cpu().numpy()
    hi, hs = hit_index.cpu().numpy(), hit_slot.cpu().numpy()
    for e, st in enumerate(states):
        assert np.array_equal(d["status"][e], st.status), (where, e)                       # rays in flight -> LIMIT
        assert np.array_equal(_bits(d["t"][e]), _bits(st.t)) and np.array_equal(d["steps"][e].astype(np.uint16), st.steps)
        assert np.array_equal(d["counts"][e], st.counts), (where, e)
        idx = hi[e, :n_hit[e]].astype(np.int64)
        order = np.argsort(idx, kind="stable")
        assert np.array_equal(idx[order], st.hit_index), (where, e)                        # the hit list, as a set
        want_slot = np.full(dev.N, -1, dtype=np.int64)
        want_slot[idx] = np.arange(n_hit[e])
        assert np.array_equal(hs[e], want_slot), (where, e)
        if n_hit[e]:
            pts = padded[e, :n_hit[e]] if dev.batch else hit_points[:n_hit[e]].cpu().numpy()
            assert np.array_equal(_bits(pts[order]), _bits(st.hit_points)), (where, e)     # point_at, bit for bit
        if dev.batch and n_pad:
            assert not _bits(padded[e, n_hit[e]:]).any()                                   # the padding: the coordinate origin
    return d


SINGLE = [pytest.param(entry, name, n, id=f"{entry}-{name}-N{n}") for entry, (_, batch) in ENTRIES.items() if not batch
          for name, c in TM.CASES.items() for n in ((c.n_fixed,) if c.n_fixed else TM.SIZES)]


@pytest.mark.parametrize("entry,name,N", SINGLE)
def test_single_trace_step_by_step(entry, name, N):
    c = TM.CASES[name]
    dev, states, k, where = drive(entry, [c], N, c.max_steps)
    assert k <= c.max_steps and (k == c.max_steps or not len(states[0].active))
    if c.max_steps == TM.MAX_STEPS:
        # k = OI_TRACE_MAX_STEPS is refused with nothing launched: the state is what it was
        assert len(states[0].active) == N == 8 and k == 1024 and states[0].counts[1024] == 8
        sdf = guarded_copy(torch.zeros(N).cuda(), "sdf")
        assert dev.step(sdf, N, TM.MAX_STEPS, c.tol, c.omega) < 0 and b"k=1024" in dev.L.oi_last_error()
        compare(dev, states, k, where + " after the refused step")
    d = finish(dev, states, k, where)
    if c.max_steps == TM.MAX_STEPS:
        assert (d["status"] == TM.LIMIT).all() and (d["steps"] == 1024).all()


def _batch_sizes(pair):
    fixed = [TM.CASES[n].n_fixed for n in pair if TM.CASES[n].n_fixed]
    return (fixed[0],) if fixed else TM.SIZES


BATCHED = [pytest.param(entry, pair, n, id=f"{entry}-{pair[0]}+{pair[1]}-N{n}") for entry, (_, batch) in ENTRIES.items() if batch
           for pair in TM.BATCHES for n in _batch_sizes(pair)]


@pytest.mark.parametrize("entry,pair,N", BATCHED)
def test_batched_trace_step_by_step(entry, pair, N):
    """E = 3, a different field per element; the middle element ends on its first step and rides along."""
    a, b = (TM.CASES[n] for n in pair)
    limit = a.max_steps
    dev, states, k, where = drive(entry, [a, TM.AWAY, b], N, limit)
    assert states[1].counts[0] == N and not states[1].counts[1:].any() and (states[1].status == TM.MISS).all()
    assert k > 1 or N == 1
    if limit == TM.MAX_STEPS:
        assert k == 1024 and len(states[0].active) == N and not len(states[2].active)
        sdf = guarded_copy(torch.zeros(3, N).cuda(), "sdf")
        assert dev.step(sdf, N, TM.MAX_STEPS, a.tol, a.omega) < 0 and b"k=1024" in dev.L.oi_last_error()
        compare(dev, states, k, where + " after the refused step")
    finish(dev, states, k, where)
