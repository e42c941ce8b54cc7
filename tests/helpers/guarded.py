"""Guarded, poisoned buffers for kernel tests.

Every buffer handed out here is a contiguous view into a larger arena:

    [ guard >= 256 KiB | pad to 256 B | body (exactly the requested bytes) | guard 256 KiB ]

The guards hold a signalling-NaN word a kernel never produces; the body of an OUTPUT holds another one ("poison"), the body
of an INPUT a copy of the caller's tensor behind guards of a third word.  `check()` then reports, per op and buffer:
  * any changed byte in either guard (a store past the end / before the start of the buffer), with the first bad byte's
    offset from the body's start (before) or end (after) and how many bytes changed;
  * any output element still holding the poison word (an element the kernel never wrote);
  * any changed byte of an input's body (kernels must not write their inputs).
GPU arithmetic quiets NaNs, so a surviving poison word really is an unwritten element; a poison word that turns up in
another output is a raw copy from an unwritten or out-of-range element.  A tail that READS past an input gets a NaN.

The guards are larger than one tile's output (a 128-point tile of 128-float features is 64 KiB): an overrun stays inside
the arena and never reaches another allocation.  Works on any device (the self-test runs on the CPU).

`guarded_ops` is a pytest fixture that routes oi_amd.ops' output allocators (_new, _new_acc, _zeros_split) through a
guard for the duration of one test.  Modules opt in with `from helpers.guarded import guarded_ops` plus
`pytestmark = [..., pytest.mark.usefixtures("guarded_ops")]` (or per test); a test opts out with
`@pytest.mark.unguarded("<one-line reason>")` (no test needs to today; the marker is not registered, so a run with
--strict-markers would first need it added to the suite's marker list)."""
import struct
import sys
import threading
import weakref

import pytest
import torch

GUARD_WORD = 0x7F8DEAD1         # guards around outputs and scratch
POISON_WORD = 0x7F8B0D1E        # body of an output that must be written in full
INPUT_GUARD_WORD = 0x7F85A5A5   # guards around inputs
GUARD_BYTES = 256 * 1024
BODY_ALIGN = 256

# Outputs that are only partly written BY CONTRACT, keyed by (oi_amd.ops function, text of the allocating source line).
# Their guards are still checked; their bodies are poisoned but may keep poison.  Each entry: the reason and the line of
# include/oi_hip.h that states the contract.  Anything partly written that is not listed here fails the test.
PARTIAL_WRITE_EXEMPT = {
    ("composite_fwd", "partials = _new(dists, L.oi_composite_num_blocks(N), 8)"):
        "block partials: slots [3] and [7] of each block's 8 are padding, never written or read "
        "(include/oi_hip.h:351-353 defines [0..2] and [4..6] only)",
}

_KIND_OUT, _KIND_ZERO, _KIND_SCRATCH, _KIND_INPUT = "out", "zero", "scratch", "input"


def _word_bytes(word):
    return struct.pack("<I", word)


class _Entry:
    __slots__ = ("arena", "off", "nbytes", "kind", "what", "itemsize", "snapshot", "guard_word", "must_write", "dtype",
                 "base_uses")


class GuardSet:
    """A collection of guarded buffers and the failures found in them so far."""

    # retired (garbage-collected) buffers are checked and released in batches: memory stays bounded in long loops
    FLUSH_COUNT = 256
    FLUSH_BYTES = 1 << 30

    def __init__(self):
        self._live = []          # weak handles of entries whose tensor is alive (checked at teardown)
        self._retired = []
        self._retired_bytes = 0
        self._busy = []          # retired, but another view of the buffer is still alive (re-examined at every flush)
        self._patterns = {}
        self._lock = threading.RLock()
        self.problems = []       # strings, one per defect found
        self.n_checked = 0

    # ------------------------------------------------------------------ allocation
    def _pattern(self, device, word, nbytes):
        """uint8 tensor of at least nbytes + 4 bytes repeating `word` (little endian), cached per device / word."""
        key = (str(device), word)
        p = self._patterns.get(key)
        if p is None or p.numel() < nbytes + 4:
            n = max(nbytes + 4, GUARD_BYTES + 4)
            n = (n + 3) // 4 * 4
            p = torch.tensor(list(_word_bytes(word)), dtype=torch.uint8).repeat(n // 4).to(device)
            self._patterns[key] = p
        return p

    def _fill(self, region, start, word):
        """Fill `region` (uint8 view starting at arena byte `start`) with `word`, phase taken from the arena offset."""
        n = region.numel()
        if n:
            ph = start % 4
            region.copy_(self._pattern(region.device, word, n + ph)[ph:ph + n])

    def _arena(self, nbytes, device, guard_word):
        device = torch.device(device)
        arena = torch.empty(GUARD_BYTES + BODY_ALIGN + nbytes + GUARD_BYTES, dtype=torch.uint8, device=device)
        base = arena.data_ptr()
        off = GUARD_BYTES + (-(base + GUARD_BYTES)) % BODY_ALIGN
        self._fill(arena, 0, guard_word)
        return arena, off

    @staticmethod
    def _uses(arena):
        """References to the arena's storage (the arena tensor, every view of it, this query's own handle)."""
        return torch._C._storage_Use_Count(arena.untyped_storage()._cdata)

    def _in_use(self, e):
        """Some view of the buffer is still alive: the handed-out tensor is gone, but e.g. a reshaped view of it is not."""
        return self._uses(e.arena) > e.base_uses

    def _register(self, t, e):
        with self._lock:
            self._live.append(e)
            # the entry is checked and released once its tensor is gone (or at teardown, whichever comes first)
            weakref.finalize(t, self._retire, e)

    def _retire(self, e):
        with self._lock:
            try:
                self._live.remove(e)
            except ValueError:
                return
            self._retired.append(e)
            self._retired_bytes += e.arena.numel()

    def empty(self, shape, dtype=torch.float32, device="cuda", what="?", must_write=True):
        """An OUTPUT: poisoned body (every element must be written unless must_write=False), guard words around it."""
        return self._make(shape, dtype, device, what, _KIND_OUT if must_write else _KIND_SCRATCH, POISON_WORD)

    def zeros(self, shape, dtype=torch.float32, device="cuda", what="?"):
        """A zero-initialised accumulate-output: guards only."""
        return self._make(shape, dtype, device, what, _KIND_ZERO, None)

    def scratch(self, nbytes, device="cuda", what="?"):
        """Working memory of exactly nbytes bytes: guards only (its body is poisoned but may keep poison)."""
        return self._make((int(nbytes),), torch.uint8, device, what, _KIND_SCRATCH, POISON_WORD)

    def _make(self, shape, dtype, device, what, kind, body_word):
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * itemsize
        arena, off = self._arena(nbytes, device, GUARD_WORD)
        base_uses = self._uses(arena)
        body = arena[off:off + nbytes]
        if body_word is None:
            body.zero_()
        else:
            self._fill(body, off, body_word)
        t = body.view(dtype).view(shape)
        e = _Entry()
        e.arena, e.off, e.nbytes, e.kind, e.what, e.itemsize = arena, off, nbytes, kind, what, itemsize
        e.snapshot, e.guard_word, e.must_write, e.dtype = None, GUARD_WORD, kind == _KIND_OUT, dtype
        e.base_uses = base_uses
        self._register(t, e)
        return t

    def copy(self, t, what="input"):
        """An INPUT: a copy of `t` behind input guards; its body must be bit-identical at check time."""
        src = t.detach().contiguous()
        nbytes = src.numel() * src.element_size()
        arena, off = self._arena(nbytes, src.device, INPUT_GUARD_WORD)
        base_uses = self._uses(arena)
        body = arena[off:off + nbytes]
        if nbytes:
            body.copy_(src.reshape(-1).view(torch.uint8))
        out = body.view(src.dtype).view(src.shape)
        e = _Entry()
        e.arena, e.off, e.nbytes, e.kind, e.what, e.itemsize = arena, off, nbytes, _KIND_INPUT, what, src.element_size()
        e.snapshot, e.guard_word, e.must_write, e.dtype = body.clone(), INPUT_GUARD_WORD, False, src.dtype
        e.base_uses = base_uses
        self._register(out, e)
        return out

    # ------------------------------------------------------------------ checking
    def _stats(self, e):
        """Device tensor [6] int64: (bad bytes, first bad) of the guard before, the guard after, the body."""
        a, off, nb = e.arena, e.off, e.nbytes
        end = off + nb
        pat = self._pattern(a.device, e.guard_word, max(off, a.numel() - end))
        bad_pre = a[:off] != pat[:off]
        ph = end % 4
        bad_post = a[end:] != pat[ph:ph + a.numel() - end]
        body = a[off:end]
        if e.kind == _KIND_INPUT:
            bad_body = body != e.snapshot
        elif e.must_write and nb:
            w = body.view(torch.int32) if e.itemsize == 4 else None
            if w is not None:
                # element granularity: a 4-byte element still holding the poison word was never written
                bad_body = w == struct.unpack("<i", _word_bytes(POISON_WORD))[0]
            else:
                bad_body = body == self._pattern(a.device, POISON_WORD, nb)[:nb]
        else:
            bad_body = None
        z = torch.zeros((), dtype=torch.int64, device=a.device)
        out = []
        for m, last in ((bad_pre, True), (bad_post, False), (bad_body, False)):
            if m is None or m.numel() == 0:
                out += [z, z]
                continue
            cnt = m.sum()
            if last:   # before the body: the bad byte CLOSEST to it (the start of an underrun)
                idx = m.numel() - 1 - m.flip(0).to(torch.uint8).argmax()
            else:
                idx = m.to(torch.uint8).argmax()
            out += [cnt.to(torch.int64), idx.to(torch.int64)]
        return torch.stack(out)

    def _report(self, e, s):
        n_pre, i_pre, n_post, i_post, n_body, i_body = (int(v) for v in s)
        msgs = []
        if n_pre:
            msgs.append(f"{e.what}: {n_pre} byte(s) changed in the guard BEFORE the buffer, the nearest at body-"
                        f"{e.off - i_pre} (a store before element 0)")
        if n_post:
            msgs.append(f"{e.what}: {n_post} byte(s) changed in the guard AFTER the buffer ({e.nbytes} bytes), the first at end+"
                        f"{i_post} = byte {e.nbytes + i_post} of the buffer (a store past its end)")
        if n_body:
            if e.kind == _KIND_INPUT:
                msgs.append(f"{e.what}: input modified: {n_body} byte(s) differ, the first at byte {i_body}")
            else:
                unit = e.itemsize if e.itemsize == 4 else 1
                msgs.append(f"{e.what}: {n_body} element(s) never written (still poison), the first at element {i_body} "
                            f"(byte {i_body * unit}) of {e.nbytes // unit}")
        return msgs

    def _check_entries(self, entries):
        if not entries:
            return []
        dev_entries = {}
        for e in entries:
            dev_entries.setdefault(e.arena.device, []).append(e)
        msgs = []
        for dev, es in dev_entries.items():
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            stats = torch.stack([self._stats(e) for e in es]).cpu()   # one transfer per device
            for e, s in zip(es, stats):
                msgs += self._report(e, s)
        self.n_checked += len(entries)
        return msgs

    def flush(self):
        """Check the retired buffers and release them (skipped while the current stream captures a graph)."""
        if _capturing_anywhere():
            return
        with self._lock:
            es, self._retired, self._retired_bytes = self._retired + self._busy, [], 0
            # a buffer whose first handle is gone but that another view still reaches is not done yet: it waits (and is
            # checked at teardown at the latest), so a later write or accumulation into it is still seen
            self._busy = [e for e in es if self._in_use(e)]
            es = [e for e in es if not self._in_use(e)]
        self.problems += self._check_entries(es)

    def maybe_flush(self):
        if len(self._retired) >= self.FLUSH_COUNT or self._retired_bytes >= self.FLUSH_BYTES:
            self.flush()

    def check(self):
        """Synchronise and check every buffer (live and retired); returns and accumulates the list of defects."""
        with self._lock:
            es = self._retired + self._busy + list(self._live)
            self._retired, self._retired_bytes, self._busy = [], 0, []
        msgs = self._check_entries(es)
        self.problems += msgs
        return msgs

    def close(self):
        """Final check; drops every reference to the arenas (tensors still alive keep their own storage)."""
        self.check()
        with self._lock:
            self._live = []
            self._patterns = {}
        return self.problems


def _capturing_anywhere():
    return torch.cuda.is_available() and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


# ---------------------------------------------------------------------------------------------------------------------
# module-level convenience: one default set (the fixture installs its own for each test)
# ---------------------------------------------------------------------------------------------------------------------
_current = [GuardSet()]


def current():
    return _current[-1]


def guarded_empty(shape, dtype=torch.float32, device="cuda", what="?", must_write=True):
    return current().empty(shape, dtype, device, what, must_write)


def guarded_zeros(shape, dtype=torch.float32, device="cuda", what="?"):
    return current().zeros(shape, dtype, device, what)


def guarded_scratch(nbytes, device="cuda", what="?"):
    return current().scratch(nbytes, device, what)


def guarded_copy(t, what="input"):
    return current().copy(t, what)


def check():
    return current().check()


def assert_clean(gs=None):
    """Check now and fail the test with every defect found so far."""
    gs = gs or current()
    gs.check()
    if gs.problems:
        msg = "\n  ".join(gs.problems[:40])
        more = "" if len(gs.problems) <= 40 else f"\n  ... {len(gs.problems) - 40} more"
        pytest.fail(f"guarded buffers: {len(gs.problems)} defect(s)\n  {msg}{more}", pytrace=False)


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
def _caller_label():
    """'<ops function> <ops.py:line> <source>' of the oi_amd.ops line that allocates."""
    import linecache
    f = sys._getframe(2)
    src = linecache.getline(f.f_code.co_filename, f.f_lineno).strip()
    return f.f_code.co_name, f"ops.{f.f_code.co_name} (ops.py:{f.f_lineno}: {src})", src


def _exempt(fn, src):
    for (op, line), _why in PARTIAL_WRITE_EXEMPT.items():
        if op == fn and src.startswith(line):
            return True
    return False


@pytest.fixture
def guarded_ops(request):
    """For one test: every output oi_amd.ops allocates through _new / _new_acc / _zeros_split is a guarded arena view.
      _new          poisoned body, every element must be written (PARTIAL_WRITE_EXEMPT aside)
      _new_acc      poisoned body, every element must be written: the launcher clears it itself (ops.py _new_acc) --
                    unless a ZeroPool is active, which then serves it as before
      _zeros_split  zero body, guards only (one arena per tensor instead of one shared flat buffer)
    While the current stream captures a graph the original allocators run (a fill recorded into the capture would change
    the graph).  At teardown every buffer is checked; any defect fails the test, naming the op and the buffer."""
    marker = request.node.get_closest_marker("unguarded")
    if marker is not None:
        yield None
        return
    from oi_amd import ops
    gs = GuardSet()
    orig_new, orig_acc, orig_split = ops._new, ops._new_acc, ops._zeros_split

    def _dev(ref):
        return ref if isinstance(ref, torch.device) else ref.device

    def g_new(ref, *shape):
        if _capturing_anywhere():
            return orig_new(ref, *shape)
        gs.maybe_flush()
        fn, label, src = _caller_label()
        return gs.empty(shape, torch.float32, _dev(ref), label, must_write=not _exempt(fn, src))

    def g_new_acc(ref, *shape):
        if _capturing_anywhere() or ops._active_pool() is not None:
            return orig_acc(ref, *shape)
        gs.maybe_flush()
        fn, label, src = _caller_label()
        return gs.empty(shape, torch.float32, _dev(ref), label + " [accumulate-output]", must_write=not _exempt(fn, src))

    def g_zeros_split(dev, *shapes):
        if _capturing_anywhere() or ops._active_pool() is not None:
            return orig_split(dev, *shapes)
        gs.maybe_flush()
        _, label, _ = _caller_label()
        return [gs.zeros(sh, torch.float32, dev, f"{label} [zeroed #{i}]") for i, sh in enumerate(shapes)]

    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "_new", g_new)
    mp.setattr(ops, "_new_acc", g_new_acc)
    mp.setattr(ops, "_zeros_split", g_zeros_split)
    _current.append(gs)
    try:
        yield gs
    finally:
        mp.undo()
        _current.remove(gs)
    gs.close()
    if gs.problems:
        msg = "\n  ".join(gs.problems[:40])
        pytest.fail(f"guarded buffers: {len(gs.problems)} defect(s) in {gs.n_checked} buffers\n  {msg}", pytrace=False)
