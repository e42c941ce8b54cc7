"""CPU checks of the batched sphere trace (include/oi_trace_batch.h, oi_amd.trace.sphere_trace_batch / render_surfaces,
oi_amd.inference.surface_frames(batch=E)): the REHEARSAL of the segmented loop on the fp64 oracle alone
(tests/helpers/trace_batch_ref.py) for the views tests/test_gpu_trace_batch.py uses, header <=> library <=> binding, and the
refusals that need no GPU.

Rehearsal results (oracle alone, float64, golden weights, E = 3 views of 48 x 48 rays: seeds 0, 1, 2 with poses centre, off,
centre; defaults tol 1e-5, omega 1, 64 steps):

    per ray the segmented loop gives T.trace's t, status and steps of that element alone, whatever the read-back
    live[k] = 2304, 2304, 2304, 1878, 1301, 910, 709, 555, ...; the loop runs all 64 steps (every view leaves rays at LIMIT)
    n_evals against fresh_evals = E * sum_k live[k] = 49,992 (a host that always knew live[k]): 49,992 read every step,
    54,927 by the 'auto' rule (1.10 x, 7.9 per ray), 121,008 read every 16th step (2.42 x)
    the away-pointing rays (3 units out, pointing outwards, traced over [0, 0.05]) all miss on their first sample"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import trace_batch_ref as B
from helpers import trace_ref as T

KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)


def test_segmented_loop_equals_the_single_trace_per_element():
    r = B.rehearse()
    flds, o, d, near, far = r["inputs"]
    E, N = o.shape[:2]
    assert (E, N) == (3, T.R_VIEW ** 2)
    singles = [T.trace(flds[e].sdf, o[e], d[e], near[e], far[e]) for e in range(E)]
    for e in range(E):
        t, status, steps, in_flight = singles[e]
        bt, bs, bsteps, bflight = r["rays"][e]
        assert np.array_equal(bt, t) and np.array_equal(bs, status) and np.array_equal(bsteps, steps) and bflight == in_flight
        # the inputs chosen for the GPU tests: no START_INSIDE, no NONFINITE, LIMIT within the cap, every view has hits
        assert not (status == T.START_INSIDE).any() and not (status == T.NONFINITE).any()
        assert (status == T.LIMIT).sum() <= T.LIMIT_CAP * N and (status == T.HIT).sum() > 0.15 * N
        # per-element counts are the element's rays in flight
        col = r["counts"][:, e]
        assert col[:len(in_flight)].tolist() == in_flight and not col[len(in_flight):].any()
    live = r["live"]
    assert live[0] == N and all(a >= b for a, b in zip(live, live[1:]))
    assert live == [max(c) for c in r["counts"].tolist()]
    fresh = E * sum(max((s[3][k] if k < len(s[3]) else 0) for s in singles) for k in range(T.MAX_STEPS))
    assert r["fresh_evals"] == fresh                       # E * sum_k max_e in_flight_e[k]: the figure of the GPU cost test
    assert all(l <= b <= N for l, b in zip(live, r["bounds"]))
    assert fresh <= r["n_evals"] <= 2 * fresh              # the host rule's stale bounds stay within the factor of the cost test
    print("segmented rehearsal: live", live[:12], "...", live[-1], "steps", r["n_steps"], "n_evals", r["n_evals"], "fresh", fresh,
          "ratio", r["n_evals"] / fresh, "per ray", r["n_evals"] / (E * N))


def test_a_stale_bound_changes_the_cost_and_not_the_rays():
    auto, every, stale = B.rehearse(), B.rehearse(readback=1), B.rehearse(readback=16)
    for e in range(3):
        for a, b, c in zip(auto["rays"][e][:3], every["rays"][e][:3], stale["rays"][e][:3]):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    assert every["n_evals"] == every["fresh_evals"] == auto["fresh_evals"] == stale["fresh_evals"]
    assert every["n_evals"] <= auto["n_evals"] <= stale["n_evals"] and every["n_evals"] < stale["n_evals"]
    print("n_evals: every step", every["n_evals"], "auto", auto["n_evals"], "every 16th", stale["n_evals"])


def test_ragged_elements_and_an_element_that_ends_at_once():
    """N = 130 rays of two views plus an element of away-pointing rays: its count is 0 from step 1 on, the others march as
    they do alone."""
    flds, o, d, near, far = B.rehearse()["inputs"]
    pick = np.linspace(0, o.shape[1] - 1, 130).astype(int)
    ao, ad, an, af = B.away_rays(130)
    O_ = np.stack([o[0, pick], ao, o[2, pick]])
    D_ = np.stack([d[0, pick], ad, d[2, pick]])
    near_, far_ = np.stack([near[0, pick], an, near[2, pick]]), np.stack([far[0, pick], af, far[2, pick]])
    fns = [flds[0].sdf, flds[1].sdf, flds[2].sdf]
    r = B.trace_segments(fns, O_, D_, near_, far_)
    t, status, steps, in_flight = r["rays"][1]
    assert (status == T.MISS).all() and (steps == 1).all() and in_flight == [130]        # every away ray misses on its first sample
    assert r["counts"][0].tolist() == [130, 130, 130] and not r["counts"][1:, 1].any() and r["counts"][1, 0] > 0
    for e in (0, 2):
        alone = T.trace(fns[e], O_[e], D_[e], near_[e], far_[e])
        assert all(np.array_equal(a, b) for a, b in zip(alone[:3], r["rays"][e][:3]))
    # all elements away: one step, then nothing in flight
    r0 = B.trace_segments(fns, np.stack([ao] * 3), np.stack([ad] * 3), np.stack([an] * 3), np.stack([af] * 3))
    assert r0["live"][:2] == [130, 0] and all((x[1] == T.MISS).all() for x in r0["rays"])
    # the margin of that miss on the oracle: the sdf 3 units out against the 0.05 the rays are traced over
    s = np.concatenate([f.sdf(ao) for f in flds])
    print("sdf at the away origins: min", s.min(), "max", s.max())
    assert s.min() > 10 * 0.05


_lib = cabi.built_lib


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_trace_batch.h", lib)
    assert sorted(names) == ["oi_sdf_mlp_fwd_segments", "oi_trace_batch_begin", "oi_trace_batch_finish", "oi_trace_batch_gather",
                             "oi_trace_batch_step"]
    text = cabi.read("oi_trace_batch.h")
    assert int(re.search(r"#define OI_TRACE_BATCH_MAX_ELEMS (\d+)", text).group(1)) == lib.TRACE_BATCH_MAX_ELEMS == B.MAX_ELEMS == 1024
    assert mirrors == ["TraceBatch"] and [f[0] for f in lib.TraceBatch._fields_] == ["s", "E", "live"]
    assert lib.TraceBatch._fields_[0][1] is lib.TraceState
    from oi_amd import trace
    assert (trace.READBACK_DENSE, trace.READBACK_SPARSE) == (B.READBACK_DENSE, B.READBACK_SPARSE)
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"trace_batch.hip"' in src


def invalid_argument_cases(lib, L, f, arrays=None):
    """(call, entry, text of the message) of the refusals; f: a non-null pointer for every array (never dereferenced: each
    call returns before any launch), arrays: {field: pointer} to use instead for the state."""
    arrays = arrays or {}
    keep = []

    def batch(E=3, N=5, live=f, **kw):
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = N, E, live
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, kw.get(n, arrays.get(n, f)))
        keep.append(b)
        return ctypes.byref(b)

    seg = lambda **kw: L.oi_sdf_mlp_fwd_segments(kw.get("pts", f), f, f, f, kw.get("sdf", f), kw.get("B", 3), kw.get("n", 4),
                                                 kw.get("stride", 8), kw.get("prec", 4), 0, None)
    return [(lambda: seg(n=9, stride=8), "oi_sdf_mlp_fwd_segments", "stride=8"),
            (lambda: seg(n=0), "oi_sdf_mlp_fwd_segments", "n=0"),
            (lambda: seg(B=0), "oi_sdf_mlp_fwd_segments", "B=0"),
            (lambda: seg(B=1024, n=1, stride=1 << 21), "oi_sdf_mlp_fwd_segments", "2^31"),
            (lambda: seg(pts=None), "oi_sdf_mlp_fwd_segments", "null pointer"),
            (lambda: seg(prec=9), "oi_sdf_mlp_fwd_segments", "bad precision"),
            (lambda: L.oi_trace_batch_begin(None, None), "oi_trace_batch_begin", "null batch"),
            (lambda: L.oi_trace_batch_begin(batch(E=0), None), "oi_trace_batch_begin", "E=0"),
            (lambda: L.oi_trace_batch_begin(batch(E=1025), None), "oi_trace_batch_begin", "E=1025"),
            (lambda: L.oi_trace_batch_begin(batch(N=0), None), "oi_trace_batch_begin", "N=0"),
            (lambda: L.oi_trace_batch_begin(batch(E=1024, N=1 << 21), None), "oi_trace_batch_begin", "2^31"),
            (lambda: L.oi_trace_batch_begin(batch(t=None), None), "oi_trace_batch_begin", "null pointer"),
            (lambda: L.oi_trace_batch_begin(batch(live=None), None), "oi_trace_batch_begin", "null live"),
            (lambda: L.oi_trace_batch_step(batch(), f, 6, 0, 1e-5, 1.0, None), "oi_trace_batch_step", "bound=6"),
            (lambda: L.oi_trace_batch_step(batch(), f, -1, 0, 1e-5, 1.0, None), "oi_trace_batch_step", "bound=-1"),
            (lambda: L.oi_trace_batch_step(batch(), f, 5, 1024, 1e-5, 1.0, None), "oi_trace_batch_step", "k=1024"),
            (lambda: L.oi_trace_batch_step(batch(), f, 5, 0, 0.0, 1.0, None), "oi_trace_batch_step", "tol"),
            (lambda: L.oi_trace_batch_step(batch(), None, 5, 0, 1e-5, 1.0, None), "oi_trace_batch_step", "null sdf"),
            (lambda: L.oi_trace_batch_step(batch(E=1025), f, 5, 0, 1e-5, 1.0, None), "oi_trace_batch_step", "E=1025"),
            (lambda: L.oi_trace_batch_step(batch(points=None), f, 5, 0, 1e-5, 1.0, None), "oi_trace_batch_step", "null pointer"),
            (lambda: L.oi_trace_batch_finish(batch(), None, f, None), "oi_trace_batch_finish", "null output"),
            (lambda: L.oi_trace_batch_finish(batch(E=0), f, f, None), "oi_trace_batch_finish", "E=0"),
            (lambda: L.oi_trace_batch_gather(batch(), f, 6, f, None), "oi_trace_batch_gather", "n_pad=6"),
            (lambda: L.oi_trace_batch_gather(batch(), f, 2, None, None), "oi_trace_batch_gather", "null pointer"),
            (lambda: L.oi_trace_batch_gather(batch(counts=None), f, 2, f, None), "oi_trace_batch_gather", "null pointer")]


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    for call, entry, text in invalid_argument_cases(lib, L, f):
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)
    b = lib.TraceBatch()
    b.s.N, b.E, b.live = 5, 3, f
    for n, _ in lib.TraceState._fields_[1:]:
        setattr(b.s, n, f)
    assert L.oi_trace_batch_step(ctypes.byref(b), None, 0, 3, 1e-5, 1.0, None) == 0       # bound = 0: success, nothing launched
    assert L.oi_trace_batch_gather(ctypes.byref(b), None, 0, None, None) == 0            # n_pad = 0: nothing launched


def test_python_argument_checks():
    from oi_amd import inference, lib, trace
    from oi_amd.fields import ShapeNetwork, ColorNetwork, FieldPack
    for bad in (0, 1.5, True, 2000, None, -3):
        with pytest.raises(ValueError, match="batch"):
            inference.surface_frames(None, [], [], batch=bad)
    pack = FieldPack(ShapeNetwork(None, **KW), ColorNetwork(**KW))
    ro, rd, z = torch.zeros(2, 5, 3), torch.ones(2, 5, 3), torch.zeros(2, 64)
    with pytest.raises(lib.OiHipError):   # no CPU path
        trace.sphere_trace_batch(pack, ro, rd, z=z)
    with pytest.raises(ValueError, match=r"\(E, N, 3\)"):
        trace.sphere_trace_batch(pack, ro[0], rd[0], z=z)
    with pytest.raises(ValueError, match="one row per element"):
        trace.sphere_trace_batch(pack, ro, rd, z=torch.zeros(3, 64))
    with pytest.raises(ValueError, match="latent"):
        trace.sphere_trace_batch(pack, ro, rd)
    with pytest.raises(ValueError, match="max_steps"):
        trace.sphere_trace_batch(pack, ro, rd, z=z, max_steps=0)
    with pytest.raises(ValueError, match="readback"):
        trace.sphere_trace_batch(pack, ro, rd, z=z, readback=0)
