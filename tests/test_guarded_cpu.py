"""Self-test of the guarded-buffer helper (tests/helpers/guarded.py) on the CPU: every defect it exists to catch is made
by hand -- always through the arena, i.e. inside the allocation -- and must be reported with the right offset."""
import pytest
import torch

from helpers import guarded as G


def _arena_view(gs, t):
    """(arena, body offset) of a guarded tensor: the legal way to reach its guards."""
    for e in gs._live:
        if e.arena.data_ptr() + e.off == t.data_ptr():
            return e.arena, e.off
    raise AssertionError("not a guarded tensor")


def test_layout_alignment_and_patterns():
    gs = G.GuardSet()
    for shape, dt in (((7,), torch.float32), ((3, 5), torch.int32), ((13,), torch.uint8)):
        t = gs.empty(shape, dt, "cpu", "t")
        a, off = _arena_view(gs, t)
        nb = t.numel() * t.element_size()
        assert t.is_contiguous() and t.shape == shape and t.dtype == dt
        assert t.data_ptr() % G.BODY_ALIGN == 0 and off >= G.GUARD_BYTES and a.numel() - off - nb >= G.GUARD_BYTES
        # the guard after the body starts at its last byte + 1
        assert bytes(a[off + nb:off + nb + 4].tolist()) == G._word_bytes(G.GUARD_WORD)[(off + nb) % 4:] + \
            G._word_bytes(G.GUARD_WORD)[:(off + nb) % 4]
        if dt is torch.float32 and t.numel():
            assert bool(torch.isnan(t).all())
    assert gs.empty((0,), torch.float32, "cpu", "empty").numel() == 0
    msgs = gs.check()
    assert len(msgs) == 3 and all("never written" in m for m in msgs), msgs   # only the three unwritten bodies


def test_clean_buffers_pass():
    gs = G.GuardSet()
    out = gs.empty((5, 3), torch.float32, "cpu", "out")
    out.copy_(torch.arange(15.0).view(5, 3))
    z = gs.zeros((4,), torch.float32, "cpu", "acc")
    z += 1
    inp = gs.copy(torch.randn(9), "inp")
    s = gs.scratch(100, "cpu", "scratch")
    s[:10] = 3
    _ = inp * 2
    assert gs.check() == []


@pytest.mark.parametrize("dt", [torch.float32, torch.int32, torch.uint8])
def test_store_one_element_past_the_end_is_named(dt):
    gs = G.GuardSet()
    t = gs.empty((10,), dt, "cpu", "myop out")
    t.fill_(1)
    a, off = _arena_view(gs, t)
    isz = t.element_size()
    a[off + 10 * isz:off + 11 * isz].view(dt).fill_(2)   # element 10 of a 10-element buffer, through the arena
    msgs = gs.check()
    assert len(msgs) == 1 and "myop out" in msgs[0] and "AFTER" in msgs[0] and "end+0" in msgs[0], msgs
    assert f"byte {10 * isz} of the buffer" in msgs[0], msgs


def test_store_before_the_start_is_named():
    gs = G.GuardSet()
    t = gs.empty((8,), torch.float32, "cpu", "pre")
    t.fill_(0)
    a, off = _arena_view(gs, t)
    a[off - 8:off - 4].view(torch.float32).fill_(5.0)   # element -2
    msgs = gs.check()
    assert len(msgs) == 1 and "BEFORE" in msgs[0] and "body-5" in msgs[0], msgs


def test_store_far_past_the_end_is_counted():
    gs = G.GuardSet()
    t = gs.empty((3, 4), torch.float32, "cpu", "far")
    t.fill_(0)
    a, off = _arena_view(gs, t)
    a[off + 48 + 4096:off + 48 + 4096 + 64].fill_(0)   # 64 bytes, 4 KiB behind the end
    msgs = gs.check()
    assert len(msgs) == 1 and "end+4096" in msgs[0], msgs
    assert "64 byte(s)" in msgs[0] or "byte(s) changed" in msgs[0]


@pytest.mark.parametrize("dt", [torch.float32, torch.int32])
def test_unwritten_element_is_flagged(dt):
    gs = G.GuardSet()
    t = gs.empty((6, 7), dt, "cpu", "partial")
    t.view(-1)[:29] = 1
    t.view(-1)[30:] = 1          # element 29 never written
    msgs = gs.check()
    assert len(msgs) == 1 and "never written" in msgs[0] and "1 element(s)" in msgs[0] and "element 29 " in msgs[0], msgs


def test_unwritten_element_not_flagged_when_exempt_or_scratch():
    gs = G.GuardSet()
    gs.empty((6,), torch.float32, "cpu", "partial by contract", must_write=False)
    keep = gs.scratch(64, "cpu", "scratch")
    assert gs.check() == [] and keep.numel() == 64


def test_modified_input_is_flagged():
    gs = G.GuardSet()
    src = torch.randn(4, 5)
    inp = gs.copy(src, "x")
    assert torch.equal(inp, src) and inp.data_ptr() != src.data_ptr()
    inp[2, 3] = -1.0
    msgs = gs.check()
    assert len(msgs) == 1 and "input modified" in msgs[0] and f"byte {(2 * 5 + 3) * 4}" in msgs[0], msgs


def test_input_guard_is_checked_with_its_own_word():
    gs = G.GuardSet()
    inp = gs.copy(torch.arange(6, dtype=torch.int32), "idx")
    a, off = _arena_view(gs, inp)
    assert bytes(a[off - 4:off].tolist()) == G._word_bytes(G.INPUT_GUARD_WORD)
    a[off + 24] = 0
    msgs = gs.check()
    assert len(msgs) == 1 and "AFTER" in msgs[0] and "end+0" in msgs[0], msgs


def test_retired_buffers_are_checked_and_released():
    gs = G.GuardSet()
    gs.FLUSH_COUNT = 4
    for i in range(10):
        t = gs.empty((16,), torch.float32, "cpu", f"loop {i}")
        if i != 7:
            t.zero_()
        del t
        gs.maybe_flush()
    assert len(gs._retired) < 4 and not gs._live
    msgs = gs.close()
    assert len(msgs) == 1 and "loop 7" in msgs[0], msgs


def test_module_level_helpers_use_the_current_set():
    gs = G.GuardSet()
    G._current.append(gs)
    try:
        t = G.guarded_empty((3,), torch.float32, "cpu", "m")
        c = G.guarded_copy(torch.ones(2), "c")
        t.fill_(1)
        assert G.check() == [] and c.sum() == 2
    finally:
        G._current.remove(gs)


def test_buffer_reached_through_another_view_is_not_retired_early():
    """The handed-out tensor is dropped but a reshaped view of it lives on (and is written later): the buffer must stay
    live until that view is gone, and the late write must count."""
    gs = G.GuardSet()
    gs.FLUSH_COUNT = 1
    t = gs.empty((4, 3), torch.float32, "cpu", "reshaped")
    v = t.view(12)
    del t
    gs.maybe_flush()
    assert len(gs._busy) == 1 and gs.problems == []
    v.fill_(1.0)                      # written after the first handle was gone
    del v
    gs.flush()
    assert gs.problems == [] and not gs._busy and not gs._live and gs.n_checked == 1
