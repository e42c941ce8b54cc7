"""CPU-only checks of the adaptive anti-aliasing of the traced renderer (include/oi_aa.h): the C ABI of the
new header, the default pattern, the classifier's restatement (tests/helpers/aa_ref.py) on one synthetic surface per criterion,
the rehearsal of the classification on the fp64 oracle tracer alone, and the host layer's refusals.  No GPU."""
import os

import numpy as np
import pytest

from helpers import aa_ref as AR
from helpers import cabi
from helpers import trace_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["oi_aa_begin", "oi_aa_classify", "oi_aa_resolve"]
R_AA = 24                 # the rehearsal's and the GPU tests' view
FLAGGED_CAP = 0.25        # share of the pixels the defaults may flag on the test views (measured on the oracle: 0.167 - 0.174)


def test_header_declares_three_entries_and_no_struct():
    lib, L = cabi.built_lib()
    names, mirrors = cabi.check_header("oi_aa.h", lib)
    assert sorted(names) == ENTRIES and mirrors == []
    for n in ENTRIES:
        assert hasattr(L, n)
    text = cabi.read("oi_aa.h")
    assert "struct" not in text
    assert "#define OI_AA_MAX_SAMPLES 64" in text and lib.AA_MAX_SAMPLES == AR.MAX_SAMPLES == 64
    assert "#define OI_AA_DEFAULT_PLANE 0.5f" in text and lib.AA_DEFAULT_PLANE == AR.DEFAULT_PLANE == 0.5
    assert "#define OI_AA_DEFAULT_COS 0.5f" in text and lib.AA_DEFAULT_COS == AR.DEFAULT_COS == 0.5
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"aa.hip"' in src and "include/oi_aa.h" in src


@pytest.mark.parametrize("S", range(2, 65))
def test_default_pattern(S):
    from oi_amd import trace
    pat = trace.aa_pattern_r2(S)
    assert pat.dtype == np.float32 and pat.shape == (S, 2) and np.array_equal(pat, AR.r2_pattern(S))
    assert not pat[0].any()
    assert (pat >= -0.5).all() and (pat < 0.5).all()
    assert len({tuple(r) for r in pat.tolist()}) == S
    assert np.array_equal(pat[:-1], trace.aa_pattern_r2(S - 1))          # a prefix: more samples refine the same pattern


def _columns(flags, a):
    """The columns a (H, W) flag image marks, which must be marked in every row."""
    img = flags.reshape(a["H"], a["W"])
    assert np.array_equal(img.all(0), img.any(0))
    return tuple(np.nonzero(img.any(0))[0].tolist())


@pytest.mark.parametrize("name", AR.SYNTHETIC)
def test_classifier_on_synthetic_surfaces(name):
    a, expected = AR.synthetic(name)
    assert (a["status"] == AR.HIT).all()                                 # hit pixels only: the silhouette criterion is silent
    mask, plane, normal = AR.classify(**a, parts=True)
    assert not mask.any()
    assert _columns(AR.classify(**a), a) == tuple(expected)
    if name == "plane":
        assert not plane.any() and not normal.any()
    if name == "step":                                                   # face-on: both sides see the jump, the normals agree
        assert _columns(plane, a) == expected and not normal.any()
    if name == "grazing_step":
        # the plane criterion alone flags both sides, and only through the far side's normal: the near side's is perpendicular
        # to the jump
        assert _columns(plane, a) == expected
        H, W = a["H"], a["W"]
        inv = np.argsort(a["hit_slot"])                                   # hit k is pixel inv[k]
        pts, g = np.empty((H * W, 3), np.float32), np.empty((H * W, 3), np.float32)
        pts[inv], g[inv] = a["hit_points"], a["grad"]
        near, far = 2 * W + expected[0], 2 * W + expected[1]
        u = (pts[far] - pts[near]).astype(np.float64)
        sees = lambda n: (g[n].astype(np.float64) @ u) ** 2 > 0.25 * (g[n].astype(np.float64) @ g[n]) * (u @ u)
        assert sees(far) and not sees(near)
    if name == "crease90":                                               # the normal criterion alone: the plane test silenced
        assert _columns(normal, a) == expected
        assert _columns(AR.classify(**a, plane=0.99), a) == expected
    if name == "crease30":
        assert not plane.any() and not normal.any()
        assert _columns(AR.classify(**a, cos=0.9), a) == (3, 4)          # cos 30 degrees = 0.866 < 0.9


_REHEARSED = {}


def rehearsed(seed, pose):
    """The oracle's primary trace of a 24 x 24 view as the classifier's inputs (fp32), and the mask."""
    if (seed, pose) not in _REHEARSED:
        fld, ro, rd, near, far, w2b, t, status, steps = T.rehearse_primary(seed, pose, R_AA)["_state"]
        hit = status == T.HIT
        pts = ro[hit] + t[hit, None] * rd[hit]
        _, grad, _ = fld.full(pts)
        slot = np.full(len(status), -1, np.int32)
        slot[hit] = np.arange(int(hit.sum()), dtype=np.int32)
        _REHEARSED[(seed, pose)] = dict(status=status.astype(np.uint8), hit_slot=slot, hit_points=np.asarray(pts, np.float32),
                                        grad=np.asarray(grad, np.float32), H=R_AA, W=R_AA)
    return _REHEARSED[(seed, pose)]


@pytest.mark.parametrize("seed,pose", T.VIEWS)
def test_rehearsal_on_the_oracle(seed, pose):
    a = rehearsed(seed, pose)
    mask, plane, normal = AR.classify(**a, parts=True)
    flagged = AR.classify(**a)
    hit = (a["status"] == AR.HIT).reshape(R_AA, R_AA)
    differs = np.zeros_like(hit)                                          # a pixel whose mask differs from a neighbour's
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = slice(max(0, -dy), R_AA - max(0, dy)), slice(max(0, -dx), R_AA - max(0, dx))
            yq, xq = slice(max(0, dy), R_AA - max(0, -dy)), slice(max(0, dx), R_AA - max(0, -dx))
            differs[ys, xs] |= hit[ys, xs] != hit[yq, xq]
    share = flagged.mean()
    print(f"aa rehearsal seed={seed} {pose}: flagged {int(flagged.sum())} of {flagged.size} ({share:.3f}), silhouette {int(mask.sum())}, "
          f"plane only {int((plane & ~mask).sum())}, normal only {int((normal & ~mask).sum())}")
    assert np.array_equal(mask, differs.reshape(-1)) and flagged[differs.reshape(-1)].all()
    assert 0 < share <= FLAGGED_CAP


def test_refusals_need_no_gpu():
    from oi_amd import inference, trace
    from oi_amd.relight import LocalLight
    ok = [[0.0, 0.0], [0.25, -0.25]]
    bad = [dict(aa_samples=0), dict(aa_samples=65), dict(aa_samples=2.0), dict(aa_samples=True), dict(aa_samples="4"),
           dict(aa_plane=1.0), dict(aa_plane=-0.1), dict(aa_plane=float("nan")), dict(aa_plane="0.5"),
           dict(aa_cos=1.0), dict(aa_cos=-1e-3), dict(aa_cos=float("inf")), dict(aa_adaptive=1),
           dict(aa_samples=2, aa_pattern=[[0.1, 0.0], [0.2, 0.2]]),                       # row 0 is not the centre
           dict(aa_samples=2, aa_pattern=[[0.0, 0.0], [0.6, 0.0]]),                       # outside the pixel
           dict(aa_samples=2, aa_pattern=[[0.0, 0.0], [float("nan"), 0.0]]),
           dict(aa_samples=3, aa_pattern=ok), dict(aa_samples=2, aa_pattern=[0.0, 0.0, 0.1, 0.1]),
           dict(aa_samples=1, aa_pattern=ok)]
    for kw in bad:                                                        # before the generator is touched: there is none
        with pytest.raises(ValueError, match="render_surface"):
            trace.render_surface(None, None, None, **kw)
        with pytest.raises(ValueError, match="surface_light_walk"):
            inference.surface_light_walk(None, None, None, **kw)
        with pytest.raises(ValueError, match="surface_light_orbit"):
            inference.surface_light_orbit(None, None, None, LocalLight(position=(0.0, 0.0, 2.0)), **kw)
        with pytest.raises(ValueError, match="surface_frames"):
            inference.surface_frames(None, [], [], **kw)
    with pytest.raises(ValueError, match="batch"):
        inference.surface_frames(None, [], [], batch=2, aa_samples=4)
    assert trace._check_aa(1, True, 0.5, 0.5, None, "x") is None            # aa_samples == 1: no stage at all
    aa = trace._check_aa(2, False, 0.0, 0.25, ok, "x")
    assert (aa.S, aa.adaptive, aa.plane, aa.cos) == (2, False, 0.0, 0.25) and np.array_equal(aa.offsets, np.asarray(ok, np.float32))
    assert np.array_equal(trace._check_aa(8, True, 0.5, 0.5, None, "x").offsets, AR.r2_pattern(8))
