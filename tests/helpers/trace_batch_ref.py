"""Numpy restatement of the batched sphere trace (include/oi_trace_batch.h) on top of the fp64 state
machine of tests/helpers/trace_ref.py, plus the views and rays the CPU rehearsal and the GPU tests share.  Nothing here
touches the code under test.

`trace_segments` is the segmented loop: E elements of N rays, each compacted within its own segment of a (E, N, 3) point
array, per-element counts, live[k] = max_e counts[e][k], and the host's bound -- the last live word it read, by the rule of
oi_amd.trace (every step while live > READBACK_DENSE, every READBACK_SPARSE steps after that, or every `readback` steps).
Every element's rays are advanced by T.trace ITSELF: one T.trace per element runs in its own thread and asks for the sdf of
its compacted points; the loop here writes them into the element's segment, evaluates the first `bound` slots of EVERY
segment (the stale slots included, as the kernel does) and hands each element the first counts[e][k] values."""
import functools
import queue
import threading

import numpy as np

from helpers import mesh_attr_ref as A
from helpers import trace_ref as T

READBACK_DENSE, READBACK_SPARSE = 1024, 4          # oi_amd.trace's
MAX_ELEMS = 1024                                   # OI_TRACE_BATCH_MAX_ELEMS

# the batch of the tests: seeds 0, 1, 2 with mixed poses, 48 x 48 rays each
BATCH_VIEWS = ((0, "centre"), (1, "off"), (2, "centre"))
# five frames for surface_frames(batch=3): a full group and a partial one
FRAME_VIEWS = BATCH_VIEWS + ((0, "off"), (1, "centre"))


def trace_segments(sdf_fns, o, d, near, far, tol=T.TOL, omega=T.OMEGA, max_steps=T.MAX_STEPS, readback="auto"):
    """o, d (E, N, 3), near, far (E, N), one sdf function per element.  -> dict: per element T.trace's (t, status, steps),
    counts (steps + 1, E), live, bounds (the host's bound per step), n_evals = E * sum(bounds), fresh_evals = E * sum(live)
    (what a host that always knew live[k] would spend)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    E, N = o.shape[:2]
    req, ans, results = [queue.Queue() for _ in range(E)], [queue.Queue() for _ in range(E)], [None] * E

    def run(e):
        def fn(pts):
            req[e].put(pts)
            return ans[e].get()
        try:
            results[e] = T.trace(fn, o[e], d[e], near[e], far[e], tol, omega, max_steps)
        finally:
            req[e].put(None)

    threads = [threading.Thread(target=run, args=(e,), daemon=True) for e in range(E)]
    for th in threads:
        th.start()
    points = o + np.asarray(near, dtype=np.float64)[..., None] * d       # oi_trace_batch_begin: every slot holds a valid point
    done = [False] * E
    counts, live, bounds = [], [], []
    bound, since, k = N, 0, 0
    while True:
        cnt = [0] * E
        for e in range(E):
            if done[e]:
                continue
            p = req[e].get()
            if p is None:
                done[e] = True
                continue
            cnt[e] = len(p)
            points[e, :len(p)] = p                                       # element e's survivors, densely, in its own segment
        counts.append(cnt)
        live.append(max(cnt))
        if k > 0:                                                        # the host's read-back, by its rule
            every = (1 if bounds[-1] > READBACK_DENSE else READBACK_SPARSE) if readback == "auto" else int(readback)
            if since >= every and k < max_steps:
                bound, since = live[k], 0
        if not (k < max_steps and bound > 0):
            break
        assert live[k] <= bound <= N, (k, live[k], bound)
        bounds.append(bound)
        for e in range(E):
            s = np.asarray(sdf_fns[e](points[e, :bound]))                 # the pass evaluates every element's first `bound` slots
            assert np.isfinite(s).all()
            if cnt[e]:
                ans[e].put(s[:cnt[e]])                                   # the step ignores slots at or above counts[e][k]
        k += 1
        since += 1
    for th in threads:
        th.join(timeout=60)
        assert not th.is_alive()
    return {"rays": results, "counts": np.array(counts), "live": live, "bounds": bounds, "n_evals": E * sum(bounds),
            "fresh_evals": E * sum(live), "n_steps": k}


def batch_rays(views=BATCH_VIEWS):
    """The oracle's rays of the views, stacked: o, d (E, N, 3), near, far (E, N)."""
    r = [T.view_rays(p) for _, p in views]
    return tuple(np.stack([v[i] for v in r]) for i in range(4))


def away_rays(n, seed=7, span=0.05):
    """n rays that start 3 units from the centre and point AWAY from the unit sphere, traced over [0, span]: o, d (n, 3),
    near, far (n,) float64.  The rehearsal checks on the oracle that all of them miss on their first sample."""
    rs = np.random.RandomState(seed)
    o = np.tile(np.array([[0.0, 0.0, -3.0]]), (n, 1)) + 0.02 * rs.randn(n, 3)
    d = np.tile(np.array([[0.0, 0.0, -1.0]]), (n, 1)) + 0.05 * rs.randn(n, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o, d, np.zeros(n), np.full(n, span)


@functools.lru_cache(maxsize=None)
def rehearse(views=BATCH_VIEWS, readback="auto"):
    """The segmented loop on the oracle's fields and rays of `views` (computed once and shared: do not modify)."""
    o, d, near, far = batch_rays(views)
    flds = [T.Field(s) for s, _ in views]
    out = trace_segments([f.sdf for f in flds], o, d, near, far, readback=readback)
    out["inputs"] = (flds, o, d, near, far)
    return out


def latents(views=BATCH_VIEWS):
    """(E, 64) float32 torch tensor of the views' seeded latents."""
    import torch
    return torch.cat([A.latent(s).reshape(1, -1) for s, _ in views]).float()
