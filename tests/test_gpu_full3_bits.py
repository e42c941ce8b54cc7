"""The register-resident f16x3 forward kernel (csrc/mlp_fwd3.hip: sdf, d sdf/dx, albedo, features) reproduces the
recorded output BITS of tests/golden/full3_bits.npz: every uint32 word of call (a) -- B = 2, 165 points per element: a full
128-point tile, a ragged 37, both elements, feature output -- and the SHA-256 digest of every output of call (b) -- 66,000
points = 516 workgroups, the feature slots indexed by compute unit as in the benchmark.  The inputs are seeded draws
(gamma and beta included: the fixture depends on this kernel and the weight packing only).

Scheduling work on this kernel (instruction order, register allocation, build flags) must leave every bit in place; the
kernel has no atomics and reproduced its own bits from run to run when the fixture was recorded.

A pull request that DELIBERATELY changes this kernel's arithmetic re-records the fixture with
tools/record_full3_bits.py on the GPU and says so in its description."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("record_full3_bits", os.path.join(ROOT, "tools", "record_full3_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture_npz():
    with np.load(os.path.join(GOLDEN, "full3_bits.npz")) as f:
        return {k: np.asarray(f[k]) for k in f.files}


@pytest.fixture(scope="module")
def packed(rec):
    return rec.pack_f16x3()


def test_fixture_inputs_are_the_seeded_draws(rec, fixture_npz):
    """The stored inputs of call (a) are what tools/record_full3_bits.py draws today (a changed recipe must re-record)."""
    inp = rec.make_inputs()
    for k in ("a_pts", "a_gamma", "a_beta"):
        assert np.array_equal(inp[k].view(np.uint32), fixture_npz[k].view(np.uint32)), k


def test_call_a_ragged_two_elements_words(rec, fixture_npz, packed):
    """(a): sdf, gradient, albedo and features, word for word (inputs taken from the fixture itself)."""
    out = rec.run_call(packed, fixture_npz["a_pts"], fixture_npz["a_gamma"], fixture_npz["a_beta"], rec.A_B, True)
    for k in rec.OUTPUTS_A:
        ref = fixture_npz["a_out_" + k]
        assert out[k].shape == ref.shape and out[k].dtype == np.uint32, k
        ndiff = int((out[k] != ref).sum())
        assert ndiff == 0, f"{k}: {ndiff} of {ref.size} words differ from the recording at {fixture_npz['commit']}"


def test_call_b_cu_slot_path_digests(rec, fixture_npz, packed):
    """(b): 516 workgroups > F3_WG_SLOTS, the path the benchmark takes; SHA-256 of each output."""
    inp = rec.make_inputs()
    out = rec.run_call(packed, inp["b_pts"], inp["b_gamma"], inp["b_beta"], rec.B_B, False)
    assert out["sdf"].shape == (rec.B_N,) and out["grad"].shape == (rec.B_N, 3) == out["rgb"].shape
    for k in rec.OUTPUTS_B:
        assert rec.digest(out[k]) == str(fixture_npz["b_sha256_" + k]), f"{k}: digest differs from the recording"
