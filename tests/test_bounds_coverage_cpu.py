"""Every entry point of include/oi_hip.h that writes device memory is CALLED by a guarded case of tests/test_gpu_bounds.py,
or listed below with the reason it is not.  A new kernel without a guarded case fails here, on the CPU.

A case calls an entry either through the C ABI (`L.oi_x(...)`, its buffers from the GuardSet) or through the oi_amd.ops
wrapper that launches it (`ops.f(...)`); the wrapper must then take every output from ops._new / _new_acc / _zeros_split --
what the guarded_ops fixture replaces -- and none from torch.empty.  Names in comments or docstrings do not count."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Entry points that write no device memory of the caller's: queries, host-only calls, test hooks, plan create / destroy.
EXEMPT = {
    "oi_version": "query: no device memory",
    "oi_arch": "query: no device memory",
    "oi_last_error": "query: thread-local host string",
    "oi_mlp_packed_bytes": "sizing query",
    "oi_mlp_scratch_bytes": "sizing query (the per-precision oi_mlp_scratch_bytes_prec sizes every guarded scratch)",
    "oi_disc_fwd_small_workspace_floats": "sizing query",
    "oi_disc_fwd_small128_workspace_floats": "sizing query",
    "oi_disc_large_packed_bytes": "sizing query",
    "oi_disc_large_workspace_bytes": "sizing query",
    "oi_ada_geom_sep_supported": "shape query",
    "oi_outputs_prezeroed_stream": "host-side per-stream declaration: no device write",
    "oi_ada_theta_xint_scale": "host only (writes HOST arrays, no HIP call)",
    "oi_disc_graph_create": "graph create: stores arguments, no HIP call",
    "oi_disc_graph_create128": "graph create: stores arguments, no HIP call",
    "oi_disc_graph_destroy": "graph destroy: frees the library's own plan",
    "oi_selftest_cu_slots": "test hook (tests/test_gpu_kernels.py::test_cu_slot_exclusive)",
    "oi_selftest_sincos": "test hook (tests/test_gpu_kernels.py::test_device_sincos_accuracy)",
    "oi_selftest_q24": "test hook (tests/test_gpu_kernels.py::test_q24_slot_format_round_trip)",
}


def _code_only(path):
    """The source without comments and docstrings / string literals (names there are no calls)."""
    import io
    import tokenize
    with open(path) as fh:
        toks = [t for t in tokenize.generate_tokens(io.StringIO(fh.read()).readline)
                if t.type not in (tokenize.COMMENT, tokenize.STRING)]
    return " ".join(t.string for t in toks)


def _ops_wrappers():
    """{oi_amd.ops function name: its source} (module-level functions)."""
    path = os.path.join(ROOT, "object-intrinsics_amd", "oi_amd", "ops.py")
    with open(path) as fh:
        text = fh.read()
    tree = ast.parse(text)
    return {n.name: ast.get_source_segment(text, n) for n in tree.body if isinstance(n, ast.FunctionDef)}


def _exports():
    with open(os.path.join(ROOT, "include", "oi_hip.h")) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"^\s*(?:const\s+)?(?:int|size_t|void|char)\s*\*?\s*(oi_\w+)\s*\(", text, re.M)


def test_header_exports_are_parsed():
    names = _exports()
    assert len(names) == len(set(names)) and len(names) > 90
    for n in ("oi_sdf_mlp_fwd", "oi_mc_emit", "oi_multi_copy", "oi_version", "oi_disc_graph_destroy"):
        assert n in names


def test_every_writing_export_has_a_guarded_case():
    src = _code_only(os.path.join(ROOT, "tests", "test_gpu_bounds.py"))
    wrappers = _ops_wrappers()
    called_wrappers = {f for f in wrappers if re.search(r"\bops \. %s \(" % f, src)}
    names = _exports()
    missing, unguarded = [], []
    for n in names:
        if n in EXEMPT or re.search(r"\. %s \(" % n, src):
            continue
        via = [f for f in called_wrappers if re.search(r"\.%s\(" % n, wrappers[f])]
        if not via:
            missing.append(n)
        elif all(re.search(r"torch\.empty", wrappers[f]) for f in via):
            unguarded.append((n, via))
    assert not missing, f"entry points no case of tests/test_gpu_bounds.py calls (or an exemption): {missing}"
    assert not unguarded, f"entry points reached only through ops wrappers that allocate with torch.empty: {unguarded}"
    stale = [n for n in EXEMPT if n not in names]
    assert not stale, f"exemptions for entry points the header no longer declares: {stale}"
