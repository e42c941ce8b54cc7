"""Gap census of the shipped f16x3 forward kernel, sdf_mlp_full3_kernel<false> (csrc/mlp_fwd3.hip), on the listing that
the build's own flags produce (tools/isa_gaps.py; no GPU).  The kernel runs one wave per SIMD, so whatever vector issue
work does not fit the 24 hideable cycles of an MFMA gap is added to the tile time; the epilogues are therefore written in
three stages per k-step window and pinned by source order.  A compiler update that re-bunches them, packs
fp32 pairs beside the MFMAs again or starts spilling would cost time without failing any numerical test: this one fails.

Compiles one translation unit to assembly (about 10 s); skipped where hipcc is absent."""
import importlib.util
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "object-intrinsics_amd")
KERNEL = "sdf_mlp_full3_kernelILb0E"
PARENT_EXCESS = 20728     # the same census before the epilogues were spread (1,631 gaps, cost 40,932, 600 packed fp32 in them)
SHIPPED_EXCESS = 10896    # this kernel as shipped; about 5,700 of it are the three exposed sections (no MFMA to hide behind)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    build = _load("oi_build_flags", os.path.join(PKG, "build.py"))
    try:
        hipcc = build._hipcc()
    except RuntimeError:
        hipcc = None
    if not hipcc or not (os.path.exists(hipcc) if os.path.isabs(hipcc) else shutil.which(hipcc)):
        pytest.skip("hipcc not found")
    gaps = _load("isa_gaps", os.path.join(ROOT, "tools", "isa_gaps.py"))
    out = str(tmp_path_factory.mktemp("isa") / "mlp_fwd3.s")
    cmd = [hipcc, *build.FLAGS, *build.EXTRA.get("mlp_fwd3.hip", []), "--cuda-device-only", "-S",
           os.path.join(PKG, "csrc", "mlp_fwd3.hip"), "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    res = gaps.parse(out, [KERNEL])
    assert len(res) == 1, list(res)
    c = next(iter(res.values()))
    print({k: v for k, v in c.items() if k != "gap_costs"})
    return c


def test_mfma_count(census):
    """17 layer products x 32 k-steps x 3 limb products."""
    assert census["mfma"] == 1632 and census["gaps"] == 1631


def test_no_spilled_register(census):
    assert census["vgpr_spill_count"] == 0 and census["sgpr_spill_count"] == 0


def test_no_packed_fp32_in_the_mfma_shadow(census):
    """v_pk_*_f32 beside an MFMA issues slower than the two scalar instructions it replaces; sections marked as exposed
    (oi-exposed-begin / oi-exposed-end in the listing) may hold them."""
    assert census["pk_shadow"] == 0, census["pk_ops"]


def test_excess_over_the_hideable_issue_budget(census):
    bound = SHIPPED_EXCESS * 1.10
    assert census["excess"] <= bound, (
        f"issue cost in excess of 24 cycles per MFMA gap: {census['excess']} > {bound:.0f} "
        f"(shipped {SHIPPED_EXCESS}; before the epilogues were spread over the gaps it was {PARENT_EXCESS})")
