"""CPU checks of the diffuse interreflection bounce between the instances of a scene (include/oi_scene_bounce.h; oi_amd.scene;
DESIGN section 4.26): header <=> library <=> binding, the C ABI's refusals (checked on the host before any launch), the Python
refusals, the properties of the restatement the GPU tests compare against (tests/helpers/scene_bounce_ref.py: the furnace, E = 1
against the single view's restatement, the winner's invariance, chunked == unchunked), and the CONDITIONS the GPU test's
analytic two-sphere scene must satisfy on float64 alone: sphere 1 wins enough of sphere 0's rays, few enough rays are excluded,
and the red sphere colours the white one red."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import bounce_ref as B
from helpers import cabi
from helpers import env_ref as EV
from helpers import scene_bounce_ref as SB
from helpers import scene_light_ref as SL
from helpers import scene_ref as SR
from helpers import trace_ref as T
from test_scene_cpu import fake_gen
from test_scene_light_cpu import _stub_scene

ENTRIES = ["oi_scene_bounce_nearest", "oi_scene_bounce_resolve", "oi_scene_bounce_visible"]
# the headers this one was not allowed to grow, and the number of entries other tests pin for them
PINNED = (("oi_scene_light.h", 7), ("oi_scene_gloss.h", 3), ("oi_envbounce.h", 2), ("oi_scene.h", 7), ("oi_envlight.h", 5),
          ("oi_trace_batch.h", 5))
FINAL = (T.MISS, T.HIT, T.LIMIT, T.START_INSIDE, T.NONFINITE, T.BACKFACING)

_lib = cabi.built_lib


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_scene_bounce.h", lib)
    # no struct of its own: plain arguments, and oi_trace_batch.h's batch bound as POINTER of its mirror
    assert sorted(names) == ENTRIES == lib.symbols("oi_scene_bounce.h") and mirrors == []
    _, structs = cabi.parse(cabi.read("oi_scene_bounce.h"))
    assert sorted(structs) == []
    assert lib.SIGS["oi_scene_bounce.h"]["oi_scene_bounce_visible"][1][0] == ctypes.POINTER(lib.TraceBatch)
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"scene_bounce.hip"' in src and "include/oi_scene_bounce.h" in src
    for header, n in PINNED:
        assert len(lib.symbols(header)) == n, header
    text = cabi.read("oi_scene_bounce.h")
    assert not re.search(r"#\s*define\s+OI_", re.sub(r"#define OI_SCENE_BOUNCE_H_", "", text))      # it borrows every limit
    flat = " ".join(text.split())
    # the winner rule and the approximations are the header's to state
    for phrase in ("THE WINNER OF A SAMPLE", "in ANY element", "smallest t", "LOWEST * element index wins", "APPROXIMATIONS", "ONE bounce",
                   "DIFFUSE", "own occlusion is ignored", "OVER-estimates", "UNDER-estimates", "the furnace", "THE SEQUENCE",
                   "oi_trace_batch_step", "oi_scene_transfer_resolve"):
        assert phrase in flat, phrase
    # the per-sample term is one function, included by both kernels' sources
    csrc = os.path.join(ROOT, "object-intrinsics_amd", "csrc")
    for name in ("envbounce.hip", "scene_bounce.hip"):
        body = open(os.path.join(csrc, name)).read()
        assert '#include "bounce_common.h"' in body and "bounce_sample(" in body and "normal_transfer(" not in body, name


def invalid_argument_cases(lib, L, f, arrays=None):
    """(call, entry, text of the message) of the refusals; f: a non-null pointer for every array (never dereferenced: each
    call returns before any launch), arrays: {field: pointer} to use instead for the state."""
    arrays = arrays or {}
    keep = []

    def batch(E=3, N=24, live=f, **kw):
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = N, E, live
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, kw.get(n, arrays.get(n, f)))
        keep.append(b)
        return ctypes.byref(b)

    near = lambda status=f, t=f, E=3, Nr=24, winner=f: L.oi_scene_bounce_nearest(status, t, E, Nr, winner, None)
    vis = lambda b=None, winner=f, index=f, slot=f: L.oi_scene_bounce_visible(batch() if b is None else b, winner, index, slot, None)

    def res(winner=f, sel=f, d=f, grad2=f, rgb2=f, n_pad2=5, owner=f, ray=f, slot=f, offset=f, w2b=f, E=3, N=16, S=4, j0=1, Sc=3,
            n_vis=8, sS=9, last=1, out=f):
        """Defaults: E = 3 elements of 16 primary rays, S = 4 strata, the chunk [1, 4), n_vis = 8: 24 rays per element."""
        return L.oi_scene_bounce_resolve(winner, sel, d, grad2, rgb2, n_pad2, owner, ray, slot, offset, w2b, E, N, S, j0, Sc, n_vis, sS,
                                         last, out, None)

    A, B_, C = "oi_scene_bounce_nearest", "oi_scene_bounce_visible", "oi_scene_bounce_resolve"
    return [(lambda: near(E=0), A, "E=0"),
            (lambda: near(E=1025), A, "E=1025"),
            (lambda: near(Nr=0), A, "N=0"),
            (lambda: near(E=2, Nr=1 << 30), A, "E * N < 2^31"),
            (lambda: near(status=None), A, "null pointer"),
            (lambda: near(t=None), A, "null pointer"),
            (lambda: near(winner=None), A, "null pointer"),
            (lambda: L.oi_scene_bounce_visible(None, f, f, f, None), B_, "null batch"),
            (lambda: vis(batch(E=0)), B_, "E=0"),
            (lambda: vis(batch(E=1025)), B_, "E=1025"),
            (lambda: vis(batch(N=0)), B_, "N=0"),
            (lambda: vis(batch(E=2, N=1 << 30)), B_, "E * N < 2^31"),
            (lambda: vis(batch(live=None)), B_, "null live"),
            (lambda: vis(batch(counts=None)), B_, "null pointer in the state"),
            (lambda: vis(winner=None), B_, "null pointer"),
            (lambda: vis(index=None), B_, "null pointer"),
            (lambda: vis(slot=None), B_, "null pointer"),
            (lambda: res(S=0), C, "S=0"),
            (lambda: res(S=257), C, "S=257"),
            (lambda: res(j0=-1), C, "j0=-1"),
            (lambda: res(Sc=0), C, "Sc=0"),
            (lambda: res(j0=2), C, "j0=2, Sc=3, S=4"),
            (lambda: res(E=0), C, "E=0"),
            (lambda: res(E=1025), C, "E=1025"),
            (lambda: res(N=0), C, "N=0"),
            (lambda: res(E=2, N=1 << 30), C, "E * N < 2^31"),
            (lambda: res(sS=0), C, "scene S=0"),
            (lambda: res(sS=32769), C, "scene S=32769"),
            (lambda: res(n_vis=0), C, "n_vis=0"),
            (lambda: res(n_vis=49), C, "n_vis=49"),
            (lambda: res(E=1, N=1 << 30, n_vis=1 << 30, S=4, j0=0, Sc=2), C, "E * L * Sc * n_vis < 2^31"),      # Sc * n_vis = 2^31
            (lambda: res(n_pad2=-1), C, "n_pad2=-1"),
            (lambda: res(n_pad2=25), C, "n_pad2=25"),
            (lambda: res(grad2=None), C, "null grad2 / rgb2 with n_pad2=5"),
            (lambda: res(rgb2=None), C, "null grad2 / rgb2 with n_pad2=5"),
            (lambda: res(winner=None), C, "null pointer"),
            (lambda: res(sel=None), C, "null pointer"),
            (lambda: res(d=None), C, "null pointer"),
            (lambda: res(owner=None), C, "null pointer"),
            (lambda: res(ray=None), C, "null pointer"),
            (lambda: res(slot=None), C, "null pointer"),
            (lambda: res(offset=None), C, "null pointer"),
            (lambda: res(w2b=None), C, "null pointer"),
            (lambda: res(out=None), C, "null pointer")]


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    cases = invalid_argument_cases(lib, L, f)
    assert {e for _, e, _ in cases} == set(ENTRIES)
    for call, entry, text in cases:
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)


def test_python_refusals():
    from oi_amd import inference, scene
    from oi_amd.envlight import EnvLight, EnvMap
    gen = fake_gen()
    z, centre = torch.zeros(64), T.pose("centre")
    for entry in (lambda **kw: scene.render_scene_env(gen, [z], [centre], [], **kw),
                  lambda **kw: inference.scene_env_walk(gen, [z], [centre], EnvLight.constant(1.0), **kw),
                  lambda **kw: _stub_scene().capture_transfer(**kw)):
        for bad in (True, 2, "1", -1, 1.0):
            with pytest.raises(ValueError, match="bounces="):
                entry(transfer_samples=4, bounces=bad)
        with pytest.raises(ValueError, match="bounces=1 with transfer_samples=0"):
            entry(transfer_samples=0, bounces=1)
        with pytest.raises(ValueError, match="bounces=1 with glossy_samples / shininess"):
            entry(transfer_samples=4, bounces=1, glossy_samples=4, shininess=10.0)
        with pytest.raises(ValueError, match="bounces=1 with glossy_samples / shininess"):
            entry(transfer_samples=4, bounces=1, glossy_samples=0)
        with pytest.raises(ValueError, match="bounces=1 with glossy_samples / shininess"):
            entry(transfer_samples=4, bounces=1, shininess=10.0)
    # the keyword is appended after the existing ones
    import inspect
    assert list(inspect.signature(scene.SceneSurface.capture_transfer).parameters)[-1] == "bounces"
    assert inspect.signature(scene.SceneSurface.capture_transfer).parameters["bounces"].default == 0
    assert inspect.signature(scene.render_scene_env).parameters["bounces"].default == 0
    assert inspect.signature(inference.scene_env_walk).parameters["bounces"].default == 0
    # an EnvMap on a bounce capture: unreachable through capture_transfer, guarded all the same
    c = scene.SceneTransfer.__new__(scene.SceneTransfer)
    c.scene, c.S, c.glossy_samples, c.shininess, c.specular = _stub_scene(), 9, None, None, None
    c._bounce = torch.zeros(3, 9, 81)
    m = EnvMap.__new__(EnvMap)
    m.shininess = 10.0
    with pytest.raises(ValueError, match="EnvMap environments on a capture made with bounces=1"):
        c.shade([m])
    # a chunk of one sample that does not fit: refused naming the counts, before anything is launched
    with pytest.raises(ValueError, match=r"2 instances x 1 lights x 150 visible points = 300 rays per sample"):
        _stub_scene()._sampled("SceneSurface.capture_transfer", 16, 0, 299, None, distance=float("inf"), anyhit=False)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
def random_case(rs, E, S, n_vis, M, N=16, statuses=FINAL, p_hit=0.5, n_pad2=None, front=None, tie=0.2, tiny_grad=0.05):
    """A random finished state of S samples of sum(n_vis) visible points against E elements, with everything
    oi_scene_bounce_resolve reads.  n_vis: visible points per element; M >= sum(n_vis) scene pixels, the rest off the mask.
    statuses: the final statuses drawn beside HIT; front True / False: every winner's gradient faces / backs its ray; n_pad2: the
    padded row length (default the largest selection; 0: nothing selected is kept); tie: share of rays whose t is equal in two
    elements; tiny_grad: share of secondary gradients of length ~1e-9."""
    n = int(sum(n_vis))
    assert M >= n and max(n_vis) <= N
    offset = SR.offsets(n_vis)
    owner, owner_ray, vis_slot = np.full(M, -1), np.full(M, -1), np.full((E, N), -1)
    pix = rs.permutation(M)[:n]
    g = 0
    for e, nv in enumerate(n_vis):
        rays = rs.permutation(N)[:nv]
        vis_slot[e, rays] = np.arange(nv)
        owner[pix[g:g + nv]], owner_ray[pix[g:g + nv]] = e, rays
        g += nv
    other = [s for s in statuses if s != T.HIT]
    status = np.where(rs.rand(E, S, n) < p_hit, T.HIT, rs.choice(other, size=(E, S, n))).astype(np.uint8)
    t = (rs.rand(E, S, n) * 3 + 0.1).astype(np.float32)
    if E > 1:
        same = rs.rand(S, n) < tie
        a, b = rs.randint(0, E, (S, n)), rs.randint(0, E, (S, n))
        for e in range(E):
            t[e] = np.where(same & (b == e), np.take_along_axis(t, a[None], 0)[0], t[e])
    d = rs.randn(E, S, n, 3)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    w2b = np.stack([T.pose(k).double().numpy() for k in ("centre", "off", "centre")][:E] + [np.eye(4)] * max(0, E - 3)).astype(np.float32)
    w2b = w2b[rs.permutation(E)]
    winner = SB.winners(status, t)
    sel = SB.selection(winner.reshape(-1), E)
    pad = max(len(r) for r in sel) if n_pad2 is None else n_pad2
    sel_slot = np.full((E, S * n), -1, dtype=np.int32)
    for e, rays in enumerate(sel):
        sel_slot[e, rays] = rs.permutation(len(rays))                        # the kernel's order is not fixed either
    grad2 = rs.randn(E, max(pad, 1), 3).astype(np.float32)
    if front is not None:
        for e, rays in enumerate(sel):
            k = sel_slot[e, rays]
            ok = k < pad
            sign = -1.0 if front else 1.0
            grad2[e, k[ok]] = sign * d.reshape(E, -1, 3)[e, rays[ok]] * (0.5 + rs.rand(int(ok.sum()), 1)) + 0.05 * rs.randn(int(ok.sum()), 3)
    small = rs.rand(E, max(pad, 1)) < tiny_grad
    grad2[small] *= 1e-9
    rgb2 = rs.rand(E, max(pad, 1), 3).astype(np.float32)
    return dict(E=E, S=S, n=n, M=M, N=N, owner=owner, owner_ray=owner_ray, vis_slot=vis_slot, offset=offset, status=status, t=t,
                rays_d=d, w2b=w2b, winner=winner, sel_slot=sel_slot.reshape(E, S, n), n_pad2=pad,
                grad2=grad2[:, :pad] if pad else None, rgb2=rgb2[:, :pad] if pad else None)


def chunks_of(c, cuts):
    """The case's state cut into chunks of samples, as oi_scene_bounce_resolve takes them (each chunk with its own winner and
    slot lists; the gathered rows are the case's, shared)."""
    out, j0 = [], 0
    for k in cuts:
        out.append(dict(winner=c["winner"][j0:j0 + k], sel_slot=c["sel_slot"][:, j0:j0 + k], rays_d=c["rays_d"][:, j0:j0 + k],
                        grad2=c["grad2"], rgb2=c["rgb2"]))
        j0 += k
    assert j0 == c["S"]
    return out


def resolved(c, cuts=None):
    return SB.resolve(chunks_of(c, cuts or [c["S"]]), c["owner"], c["owner_ray"], c["vis_slot"], c["offset"], c["w2b"], c["S"])


def test_restatement_furnace():
    """White albedo at the secondary points, a constant environment: T0_0 + T1[ch][0] is y_0 -- the shading 1 -- to 1e-12 on every
    pixel whose S samples are all free or front-face winners, below it elsewhere; over E in {1, 2, 3}."""
    rs = np.random.RandomState(3)
    L0 = 2.0 * np.sqrt(np.pi)
    seen_full = seen_less = 0
    for E in (1, 2, 3):
        for statuses, front in (((T.MISS, T.HIT), True), (FINAL, None)):
            c = random_case(rs, E, 5, [7, 4, 6][:E], 40, statuses=statuses, front=front, tiny_grad=0.0)
            c["rgb2"] = np.ones_like(c["rgb2"])
            T1, _, ndds, fronts = resolved(c)
            on, g = SL.pixel_points(c["owner"], c["owner_ray"], c["vis_slot"], c["offset"])
            free = SL.escaped(c["status"])[:, g]                              # (S, pixels)
            T0_0 = free.mean(0) * EV.basis(np.array([0.0, 0.0, 1.0]))[0]
            shade = L0 * (T0_0[None] + T1[:, 0, on])                          # (3, pixels)
            full = (free | fronts[0]).all(0)
            assert np.abs(shade[:, full] - 1.0).max(initial=0.0) <= 1e-12
            assert (shade[:, ~full] < 1.0 - 0.5 / c["S"]).all()
            assert not (free & fronts[0]).any()                               # a sample is free or a winner, never both
            if front:
                assert full.all()
            seen_full += int(full.sum())
            seen_less += int((~full).sum())
            assert not T1[:, :, c["owner"] < 0].any()
    assert seen_full > 20 and seen_less > 20


def test_restatement_one_element_is_the_single_view_estimator():
    rs = np.random.RandomState(5)
    for S in (1, 4):
        c = random_case(rs, 1, S, [9], 20)
        T1, mag, _, fronts = resolved(c)
        n = c["n"]
        on, g = SL.pixel_points(c["owner"], c["owner_ray"], c["vis_slot"], c["offset"])
        hit_slot = np.full(c["M"], -1)
        hit_slot[on] = g
        slot2 = np.where(c["winner"] == 0, c["sel_slot"][0], -1).reshape(-1)
        ref, ref_mag, _, ref_front = B.resolve(c["status"][0].reshape(-1), c["rays_d"][0].reshape(-1, 3), slot2, c["grad2"][0], c["rgb2"][0],
                                               hit_slot, n, S, c["w2b"][0])
        assert np.abs(T1 - ref).max() <= 1e-15 and np.abs(mag - ref_mag).max() <= 1e-15
        assert np.array_equal(fronts[0], ref_front[:, g]) and fronts[0].any() and (~fronts[0]).any()


def test_restatement_winner_rule():
    rs = np.random.RandomState(9)
    E, S, n = 3, 6, 50
    c = random_case(rs, E, S, [20, 14, 16], 60, N=25, tie=0.4)
    st, t, w = c["status"], c["t"], c["winner"]
    # against a per-ray loop
    for j in range(S):
        for g in range(n):
            if any(st[e, j, g] not in (T.MISS, T.HIT) for e in range(E)):
                want = -1                                                     # LIMIT, START_INSIDE, NONFINITE, BACKFACING in ANY element
            else:
                hits = [(float(t[e, j, g]), e) for e in range(E) if st[e, j, g] == T.HIT]
                want = min(hits)[1] if hits else -1                            # equal t: the lowest element index
            assert w[j, g] == want
    ties = sum(1 for j in range(S) for g in range(n) if w[j, g] >= 0 and
               sum(1 for e in range(E) if st[e, j, g] == T.HIT and t[e, j, g] == t[w[j, g], j, g]) > 1)
    assert ties > 5 and (w < 0).any() and all((w == e).any() for e in range(E))
    # a LIMIT in any element kills the sample, whatever the others hold
    st2 = st.copy()
    st2[1] = np.where(rs.rand(S, n) < 0.5, T.LIMIT, st2[1])
    w2 = SB.winners(st2, t)
    assert (w2[st2[1] == T.LIMIT] == -1).all() and np.array_equal(w2[st2[1] != T.LIMIT], w[st2[1] != T.LIMIT])
    # invariance under a permutation of the elements that keeps the order of tied ones: without ties any permutation
    t3 = (rs.rand(E, S, n) * 3 + 0.1).astype(np.float32)
    w3 = SB.winners(st, t3)
    for perm in ([2, 0, 1], [1, 2, 0], [2, 1, 0]):
        wp = SB.winners(st[perm], t3[perm])
        back = np.where(wp >= 0, np.asarray(perm)[np.maximum(wp, 0)], -1)
        assert np.array_equal(back, w3), perm
    # ... and with ties between elements 0 and 2 only, the permutations that keep 0 before 2
    t4 = t3.copy()
    t4[2] = np.where(rs.rand(S, n) < 0.5, t4[0], t4[2])
    w4 = SB.winners(st, t4)
    for perm in ([1, 0, 2], [0, 2, 1]):
        wp = SB.winners(st[perm], t4[perm])
        assert np.array_equal(np.where(wp >= 0, np.asarray(perm)[np.maximum(wp, 0)], -1), w4), perm
    # the selection: a partition of the won rays
    sel = SB.selection(w.reshape(-1), E)
    assert sum(len(r) for r in sel) == int((w >= 0).sum())
    counts = [len(r) for r in sel]
    index = np.full((E, S * n), -7)
    for e, rays in enumerate(sel):
        index[e, c["sel_slot"].reshape(E, -1)[e, rays]] = rays
    assert SB.slots_consistent(w.reshape(-1), index, c["sel_slot"].reshape(E, -1), counts) is None
    bad = c["sel_slot"].reshape(E, -1).copy()
    bad[0, sel[0][0]], bad[0, sel[0][1]] = bad[0, sel[0][1]], bad[0, sel[0][0]]
    assert SB.slots_consistent(w.reshape(-1), index, bad, counts) is not None


def test_restatement_chunks_and_zero_albedo():
    rs = np.random.RandomState(13)
    for E in (1, 2, 3):
        c = random_case(rs, E, 7, [8, 5, 6][:E], 30)
        whole, mag, _, fronts = resolved(c)
        assert fronts[0].any() and np.abs(whole).max() > 0
        for cuts in ([1] * 7, [3, 4], [6, 1], [2, 2, 3]):
            part, pmag, _, _ = resolved(c, cuts)
            assert np.abs(part - whole).max() <= 1e-15 and np.abs(pmag - mag).max() <= 1e-15, cuts
        z = dict(c, rgb2=np.zeros_like(c["rgb2"]))
        T1, zmag, _, _ = resolved(z)
        assert not T1.any() and not zmag.any()
        # n_pad2 = 0: nothing gathered, nothing added
        e0 = dict(c, grad2=None, rgb2=None)
        assert not resolved(e0)[0].any()
        # a row shorter than the selection: the slots behind it are skipped, nothing is read outside
        short = max(1, c["n_pad2"] // 2)
        s = dict(c, grad2=c["grad2"][:, :short], rgb2=c["rgb2"][:, :short])
        T1s, _, _, fs = resolved(s)
        assert fs[0].sum() < fronts[0].sum() and np.abs(T1s).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# the analytic two-sphere scene on float64 alone
# ---------------------------------------------------------------------------------------------------------------------
def test_analytic_scene_rehearsal():
    """The GPU test's analytic two-sphere scene on float64 ALONE, seed 7 (scene_bounce_ref.AN_SEED), S = 16 and 64: sphere 1
    wins at least scene_light_ref.BLOCKED_FLOOR of sphere 0's rays; the facing rays excluded -- in the band |closest approach -
    0.5| < 1e-3 or with |n . d| < 1e-3 at the secondary hit -- are at most 1 %; and the red sphere colours the white one: for
    sphere 0's points with a winner, T1[red][0] > T1[green][0] > 0."""
    sc = SR.analytic_scene()
    cf = SR.analytic_closed_form(sc)
    pts = SL.analytic_points(sc, cf)
    on0 = pts["e"] == 0
    for S in SB.AN_SAMPLES:
        a = SB.analytic_bounce(sc, pts, S, SB.AN_SEED)
        won1 = (a["winner"][:, on0] == 1)
        share = won1.sum() / won1.size
        excluded = a["excluded"][a["facing"]].mean()
        print(f"analytic rehearsal: bounce S={S} seed={SB.AN_SEED}: points {len(on0)}, on sphere 0 {int(on0.sum())}; sphere-0 rays won by "
              f"sphere 1 {int(won1.sum())} of {won1.size} ({share:.4f}); facing rays {int(a['facing'].sum())}, excluded "
              f"{int(a['excluded'].sum())} ({excluded:.5f}); winners on a back face {int(((a['winner'] >= 0) & ~a['front']).sum())}")
        assert share >= SL.BLOCKED_FLOOR
        assert excluded <= SB.EXCLUDED_CAP
        assert not (a["winner"][:, on0] == 0).any()                          # a convex sphere never meets its own biased rays
        assert (a["front"] == (a["winner"] >= 0)).all()                      # a nearest intersection from outside is a front face
        lit = on0 & (a["winner"] >= 0).any(0)
        red, green = a["T1"][0, 0], a["T1"][1, 0]
        assert lit.sum() > 10 and (red[lit] > green[lit]).all() and (green[lit] > 0).all()
        assert not a["T1"][:, :, ~(a["winner"] >= 0).any(0)].any()
        # (sphere 1 stands between the camera and sphere 0: its visible points face away from sphere 0 and win nothing there)
        assert not ((pts["e"] == 1) & (a["winner"] == 0).any(0)).any()
