"""CPU checks of the batched secondary rays (include/oi_occlusion_batch.h; oi_amd.trace.render_surfaces(batch_secondary=True);
DESIGN section 4.32): header <=> library <=> binding, the C ABI's refusals (checked on the host before any launch, the
pointers never dereferenced), the keyword validation, the chunk and group planner against a brute-force enumeration, and the
defaults that keep every existing call on the per-view path."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import cabi
from helpers import trace_batch_ref as B
from helpers import trace_ref as T
from test_scene_cpu import fake_gen

ENTRIES = ["oi_occlusion_batch_begin", "oi_occlusion_batch_resolve", "oi_surface_shade_batch"]

_lib = cabi.built_lib


def test_header_library_and_binding_agree():
    lib, L = _lib()
    names, mirrors = cabi.check_header("oi_occlusion_batch.h", lib)
    assert sorted(names) == ENTRIES == lib.symbols("oi_occlusion_batch.h")
    assert mirrors == []                                             # no struct of its own
    _, structs = cabi.parse(text := cabi.read("oi_occlusion_batch.h"))
    assert structs == {}
    for name in ("SHADOW", "CAP", "HEMISPHERE", "LOCAL"):
        assert int(re.search(rf"#define OI_OCCLUSION_BATCH_{name} (\d+)", text).group(1)) == getattr(lib, f"OCCLUSION_BATCH_{name}")
    src = open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert '"occlusion_batch.hip"' in src and "include/oi_occlusion_batch.h" in src
    # nothing was added to the headers whose entry lists other tests pin
    for header, n in (("oi_trace.h", 6), ("oi_occlusion.h", 5), ("oi_trace_batch.h", 5), ("oi_scene_light.h", 7),
                      ("oi_local_light.h", 4), ("oi_scene.h", 7)):
        assert len(lib.symbols(header)) == n, header


def invalid_argument_cases(lib, L, f):
    """(call, entry, text of the message) of the refusals; f: a non-null pointer for every array (never dereferenced: each
    call returns before any launch)."""
    keep = []

    def batch(E=3, N=48, live=f, **kw):
        b = lib.TraceBatch()
        b.s.N, b.E, b.live = N, E, live
        for n, _ in lib.TraceState._fields_[1:]:
            setattr(b.s, n, kw.get(n, f))
        keep.append(b)
        return ctypes.byref(b)

    def begin(b=None, mode=1, hp=f, hi=f, counts=f, N=64, n_pad=8, Lt=2, S=4, j0=1, Sc=3, lights=f, radius=f, w2b=f, bias=1e-2,
              distance=0.5):
        """Defaults: E = 3 views, L = 2 lights, S = 4 strata, the chunk [1, 4), n_pad = 8: 2 * 3 * 8 = 48 rays per view."""
        return L.oi_occlusion_batch_begin(batch() if b is None else b, mode, hp, f, hi, counts, N, n_pad, Lt, S, j0, Sc, lights,
                                          radius, w2b, bias, distance, 7, None)

    res = lambda st=f, slot=f, counts=f, E=3, N=64, n_pad=8, Lt=2, S=4, j0=1, Sc=3, last=1, count=f, out=f: \
        L.oi_occlusion_batch_resolve(st, slot, counts, E, N, n_pad, Lt, S, j0, Sc, last, count, out, None)

    def shade(E=3, n_pad=8, N=64, Lt=1, image=f, lights=f, w2b=f, hp=f, local=0, null=False):
        P = lib.SurfaceAoParams()
        P.N, P.n_hit, P.L = N, 0, Lt
        for n in ("rays_o", "rays_d", "t", "status", "hit_slot", "grad", "rgb"):
            setattr(P, n, f)
        P.hit_points, P.w2b, P.lights, P.image = hp, w2b, lights, image
        keep.append(P)
        return L.oi_surface_shade_batch(None if null else ctypes.byref(P), E, n_pad, local, None)

    inf, nan = float("inf"), float("nan")
    return [(lambda: L.oi_occlusion_batch_begin(None, 1, f, f, f, f, 64, 8, 2, 4, 1, 3, f, f, f, 1e-2, 0.5, 7, None),
             "oi_occlusion_batch_begin", "null batch"),
            (lambda: begin(batch(E=0)), "oi_occlusion_batch_begin", "E=0"),
            (lambda: begin(batch(E=1025)), "oi_occlusion_batch_begin", "E=1025"),
            (lambda: begin(batch(live=None)), "oi_occlusion_batch_begin", "null live"),
            (lambda: begin(batch(status=None)), "oi_occlusion_batch_begin", "null pointer in the state"),
            (lambda: begin(mode=4), "oi_occlusion_batch_begin", "mode=4"),
            (lambda: begin(mode=-1), "oi_occlusion_batch_begin", "mode=-1"),
            (lambda: begin(Lt=0), "oi_occlusion_batch_begin", "L=0"),
            (lambda: begin(Lt=257), "oi_occlusion_batch_begin", "L=257"),
            (lambda: begin(S=0), "oi_occlusion_batch_begin", "S=0"),
            (lambda: begin(S=257), "oi_occlusion_batch_begin", "S=257"),
            (lambda: begin(j0=-1), "oi_occlusion_batch_begin", "j0=-1"),
            (lambda: begin(Sc=0), "oi_occlusion_batch_begin", "Sc=0"),
            (lambda: begin(j0=2), "oi_occlusion_batch_begin", "j0=2, Sc=3, S=4"),
            (lambda: begin(mode=0), "oi_occlusion_batch_begin", "S=4, Sc=3 with the hard shadow ray"),
            (lambda: begin(mode=2), "oi_occlusion_batch_begin", "L=2 with the hemisphere"),
            (lambda: begin(N=0), "oi_occlusion_batch_begin", "N=0"),
            (lambda: begin(N=1 << 30), "oi_occlusion_batch_begin", "2^31"),
            (lambda: begin(n_pad=0), "oi_occlusion_batch_begin", "n_pad=0"),
            (lambda: begin(n_pad=65), "oi_occlusion_batch_begin", "n_pad=65"),
            (lambda: begin(Sc=2), "oi_occlusion_batch_begin", "must be L * Sc * n_pad"),
            (lambda: begin(bias=-1.0), "oi_occlusion_batch_begin", "bias"),
            (lambda: begin(bias=inf), "oi_occlusion_batch_begin", "bias"),
            (lambda: begin(bias=nan), "oi_occlusion_batch_begin", "bias"),
            (lambda: begin(batch(N=24), mode=2, Lt=1, distance=0.0), "oi_occlusion_batch_begin", "distance"),
            (lambda: begin(batch(N=24), mode=2, Lt=1, distance=nan), "oi_occlusion_batch_begin", "distance"),
            (lambda: begin(hp=None), "oi_occlusion_batch_begin", "null input pointer"),
            (lambda: begin(hi=None), "oi_occlusion_batch_begin", "null input pointer"),
            (lambda: begin(counts=None), "oi_occlusion_batch_begin", "null input pointer"),
            (lambda: begin(lights=None), "oi_occlusion_batch_begin", "null input pointer (lights, w2b)"),
            (lambda: begin(mode=3, w2b=None), "oi_occlusion_batch_begin", "null input pointer (lights, w2b)"),
            (lambda: begin(radius=None), "oi_occlusion_batch_begin", "null radius"),
            (lambda: res(E=0), "oi_occlusion_batch_resolve", "E=0"),
            (lambda: res(Lt=257), "oi_occlusion_batch_resolve", "L=257"),
            (lambda: res(S=257), "oi_occlusion_batch_resolve", "S=257"),
            (lambda: res(j0=2), "oi_occlusion_batch_resolve", "j0=2"),
            (lambda: res(Sc=0), "oi_occlusion_batch_resolve", "Sc=0"),
            (lambda: res(n_pad=0), "oi_occlusion_batch_resolve", "n_pad=0"),
            (lambda: res(n_pad=65), "oi_occlusion_batch_resolve", "n_pad=65"),
            (lambda: res(E=1024, N=1 << 20, n_pad=1 << 20, Lt=256, S=256, j0=0, Sc=256), "oi_occlusion_batch_resolve", "2^31"),
            (lambda: res(st=None), "oi_occlusion_batch_resolve", "null pointer"),
            (lambda: res(slot=None), "oi_occlusion_batch_resolve", "null pointer"),
            (lambda: res(counts=None), "oi_occlusion_batch_resolve", "null pointer"),
            (lambda: res(count=None), "oi_occlusion_batch_resolve", "null pointer"),
            (lambda: res(out=None), "oi_occlusion_batch_resolve", "null pointer"),
            (lambda: shade(null=True), "oi_surface_shade_batch", "null params"),
            (lambda: shade(E=0), "oi_surface_shade_batch", "E=0"),
            (lambda: shade(E=1025), "oi_surface_shade_batch", "E=1025"),
            (lambda: shade(N=0), "oi_surface_shade_batch", "N=0"),
            (lambda: shade(n_pad=-1), "oi_surface_shade_batch", "n_pad=-1"),
            (lambda: shade(n_pad=65), "oi_surface_shade_batch", "n_pad=65"),
            (lambda: shade(Lt=0), "oi_surface_shade_batch", "L=0"),
            (lambda: shade(Lt=257), "oi_surface_shade_batch", "L=257"),
            (lambda: shade(lights=None), "oi_surface_shade_batch", "L=1"),
            (lambda: shade(w2b=None), "oi_surface_shade_batch", "null input pointer"),
            (lambda: shade(hp=None), "oi_surface_shade_batch", "null hit arrays with n_hit=8")]


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
    # the resolve of a chunk that is not the last takes no map
    # (refused only for what it would read: a null count)
    assert L.oi_occlusion_batch_resolve(f, f, f, 3, 64, 8, 2, 4, 1, 3, 0, None, None, None) == -1


def test_defaults_keep_the_per_view_path():
    from oi_amd import inference, trace
    for fn in (trace.render_surfaces, inference.surface_frames):
        p = inspect.signature(fn).parameters
        assert p["batch_secondary"].default is False and p["max_secondary_rays"].default is None, fn.__name__
    from oi_amd import scene
    assert trace.MAX_SECONDARY_RAYS == scene.MAX_SHADOW_RAYS


def test_keyword_validation():
    from oi_amd import inference, trace
    gen = fake_gen()
    z, centre = torch.zeros(64), T.pose("centre")
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="batch_secondary"):
            trace.render_surfaces(gen, [z], [centre], batch_secondary=bad)
        with pytest.raises(ValueError, match="batch_secondary"):
            inference.surface_frames(gen, [z], [centre], batch=2, batch_secondary=bad)
    for bad in (0, -1, 1.5, True, "many", float("nan")):
        with pytest.raises(ValueError, match="max_secondary_rays"):
            trace.render_surfaces(gen, [z], [centre], batch_secondary=True, max_secondary_rays=bad)
        with pytest.raises(ValueError, match="max_secondary_rays"):
            trace.render_surfaces(gen, [z], [centre], max_secondary_rays=bad)              # checked whether or not it is used
        with pytest.raises(ValueError, match="max_secondary_rays"):
            inference.surface_frames(gen, [z], [centre], batch=2, batch_secondary=True, max_secondary_rays=bad)
    with pytest.raises(ValueError, match="batch_secondary=True with batch=1"):
        inference.surface_frames(gen, [z], [centre], batch_secondary=True)
    # a single view that does not fit: refused naming the three counts
    with pytest.raises(ValueError, match=r"1 view x 2 lights x 150 hit slots = L \* n_pad = 300 rays per sample of one view \(at "
                                         r"most max_secondary_rays=299"):
        trace.plan_secondary(3, 2, 4, 150, 299)
    with pytest.raises(ValueError, match=r"L \* n_pad = 2147483648 rays per sample of one view .* below 2\^31"):
        trace.plan_secondary(1, 2, 1, 1 << 30, 1 << 40)
    assert trace.plan_secondary(3, 2, 4, 150, 300) == ([(0, 1), (1, 2), (2, 3)], [(0, 1), (1, 1), (2, 1), (3, 1)])


def _brute_force(E, L, S, n_pad, cap):
    """Every (E_g, Sc) with E_g * L * Sc * n_pad <= cap; the plan is the one with the most views per group and then the most
    samples per chunk (samples are split first), or None when not even (1, 1) fits."""
    fits = [(g, c) for g in range(1, E + 1) for c in range(1, S + 1) if g * L * c * n_pad <= cap]
    return max(fits) if fits else None


def test_planner_against_brute_force():
    from oi_amd import trace
    seen = set()
    for E, L, S, n_pad in itertools.product((1, 2, 3, 5), (1, 2, 3), (1, 2, 3, 4, 7), (1, 2, 5)):
        for cap in sorted({1, 2, 3, 5, 6, 7, 10, 11, 12, 15, 29, 30, 31, 59, 60, 100, 210, 1 << 24, E * L * n_pad, E * L * n_pad - 1,
                           L * n_pad, L * n_pad - 1, E * L * S * n_pad, E * L * S * n_pad - 1} - {0}):
            best = _brute_force(E, L, S, n_pad, cap)
            if best is None:
                with pytest.raises(ValueError, match=rf"1 view x {L} lights x {n_pad} hit slots"):
                    trace.plan_secondary(E, L, S, n_pad, cap)
                seen.add("refused")
                continue
            groups, chunks = trace.plan_secondary(E, L, S, n_pad, cap)
            g, c = best
            # consecutive groups that cover the views once, of the brute-force size but for the last
            assert groups[0][0] == 0 and groups[-1][1] == E and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
            assert all(b - a == g for a, b in groups[:-1]) and 1 <= groups[-1][1] - groups[-1][0] <= g
            assert max(b - a for a, b in groups) == g
            # chunks in increasing j0 that cover the samples once
            assert chunks[0][0] == 0 and sum(n for _, n in chunks) == S and all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
            assert all(n == c for _, n in chunks[:-1]) and 1 <= chunks[-1][1] <= c and max(n for _, n in chunks) == c
            assert all((b - a) * L * n * n_pad <= cap for a, b in groups for _, n in chunks)
            assert g == E or c == 1                                   # the views are split only when one sample of all does not fit
            seen.add("whole" if (g, c) == (E, S) else "samples" if g == E else "groups")
            if g == E and c == 1 and S > 1:
                seen.add("one sample per chunk")
            if g == 1 and E > 1:
                seen.add("groups of 1")
    assert seen == {"refused", "whole", "samples", "groups", "one sample per chunk", "groups of 1"}
    assert trace.plan_secondary(3, 2, 4, 0, 1) == ([], [])                                # no view has a hit: nothing to plan
    # the 2^31 limit of one batch holds whatever the cap
    groups, chunks = trace.plan_secondary(4, 1, 8, 1 << 29, 1 << 40)
    assert groups == [(0, 3), (3, 4)] and chunks == [(j, 1) for j in range(8)]


def test_chunk_rule_is_the_three_rules_it_replaced():
    """trace.sample_chunks, the one chunk rule, against the three it replaced, restated here as they stood -- the sample loops
    of SceneSurface._sampled and GroundSurface._sampled and plan_secondary's sample split: equal chunks, and refusals equal word
    for word.  The grid holds per > cap, caps beyond 2^31 (so that the 2^31 bound decides) and samples that are no multiple of
    the chunk."""
    from oi_amd import trace
    seen = set()

    def outcome(fn):
        try:
            return fn()
        except ValueError as e:
            return str(e)

    def old_loop(S, per, cap, refusal):
        chunk = min(int(S), min(int(cap), (1 << 31) - 1) // per)
        if chunk < 1:
            raise ValueError(refusal)
        return [(j0, min(chunk, int(S) - j0)) for j0 in range(0, int(S), chunk)]

    def old_plan(E, L, S, n_pad, max_secondary_rays, what="render_surfaces"):
        cap, per = min(int(max_secondary_rays), (1 << 31) - 1), L * n_pad
        if per > cap:
            raise ValueError(f"{what}: 1 view x {L} lights x {n_pad} hit slots = L * n_pad = {per} rays per sample of one view (at most "
                             f"max_secondary_rays={max_secondary_rays} and below 2^31)")
        group, chunk = (E, min(S, cap // (E * per))) if E * per <= cap else (cap // per, 1)
        return ([(a, min(E, a + group)) for a in range(0, E, group)], [(j0, min(chunk, S - j0)) for j0 in range(0, S, chunk)])

    for E, L, S, n in itertools.product((1, 2, 7), (1, 2, 256), (1, 4, 256), (1, 150, 1 << 20)):
        per = E * L * n
        for cap in (per - 1, per, 1 << 24, 1 << 40):
            tail = f"(at most max_shadow_rays={cap} and below 2^31; inference.scene_light_walk splits the lights)"
            for what, rays in (("SceneSurface.ambient", f"{E} instances x {L} lights x {n} visible points = {per} rays per sample"),
                               ("GroundSurface.ambient", f"{E} instances x {L} lights x {n} ground points = E * L * n_g = {per} rays per sample")):
                old = outcome(lambda: old_loop(S, per, cap, f"{what}: {rays} {tail}"))
                assert outcome(lambda: trace.sample_chunks(S, per, cap, what, rays)) == old, (E, L, S, n, cap)
            seen.add("refused" if isinstance(old, str) else "whole" if len(old) == 1 else "ragged" if old[-1][1] != old[0][1] else "even")
            if not isinstance(old, str) and min(cap, (1 << 31) - 1) // per != cap // per:
                seen.add("2^31 decides")
            old = outcome(lambda: old_plan(E, L, S, n, cap))
            assert outcome(lambda: trace.plan_secondary(E, L, S, n, cap)) == old, (E, L, S, n, cap)
            seen.add("plan refused" if isinstance(old, str) else "plan groups" if len(old[0]) > 1 else "plan samples")
    assert seen == {"refused", "whole", "ragged", "even", "2^31 decides", "plan refused", "plan groups", "plan samples"}


def test_the_away_view_of_the_gpu_test_misses_on_the_oracle():
    """tests/test_gpu_occlusion_batch.py builds its view without a hit from trace_batch_ref.away_rays(130), repeated to the
    view's 48 x 48 rays: on the oracle's fields every one of the 130 misses on its first sample (float64)."""
    o, d, near, far = B.away_rays(130)
    for seed in (0, 1, 2):
        t, status, steps, in_flight = T.trace(T.Field(seed).sdf, o, d, near, far)
        assert (status == T.MISS).all() and (steps == 1).all()
    assert np.resize(np.arange(130), T.R_VIEW ** 2).max() == 129
