"""Records the output BITS of sdf_mlp_full3_kernel (csrc/mlp_fwd3.hip, f16x3 operands, gradient + albedo) as the
fixture tests/golden/full3_bits.npz, which tests/test_gpu_full3_bits.py replays and compares word for word.

    python tools/record_full3_bits.py [--out tests/golden/full3_bits.npz] [--check]

Run it on the GPU at the commit whose arithmetic is the reference (a pull request that changes the kernel's arithmetic on
purpose re-records the fixture and says so).  --check records nothing: it replays the calls and reports whether the
existing fixture is reproduced (exit status 1 if not) -- run at the recording commit it answers "does the kernel reproduce
its own bits from run to run".

The fixture depends on this kernel and on the weight packing only: gamma and beta are drawn here, not taken from the
FiLM kernel.
  call (a)  B = 2, 165 points per element = one full 128-point tile + a ragged 37 (tail lanes, both elements), feature
            output requested.  Stored: the inputs and the four outputs as raw uint32 words.
  call (b)  B = 1, 66,000 points = 516 workgroups > F3_WG_SLOTS = 512: the feature slots are indexed by compute unit, the
            path the benchmark takes; no feature output.  Stored: a SHA-256 digest per output."""
import argparse
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "object-intrinsics_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "full3_bits.npz")
A_B, A_N = 2, 165
B_B, B_N = 1, 66000
OUTPUTS_A = ("sdf", "grad", "rgb", "feat")
OUTPUTS_B = ("sdf", "grad", "rgb")


def make_inputs():
    """Seeded inputs of both calls (numpy float32).  gamma ~ 30 (1 + 0.2 n), beta ~ 0.5 n: the scale of the FiLM rows
    that the mapping network produces for the golden weights (phases of tens of radians)."""
    rng = np.random.default_rng(0)
    out = {}
    for tag, B, n in (("a", A_B, A_N), ("b", B_B, B_N)):
        out[tag + "_pts"] = rng.uniform(-0.9, 0.9, size=(B * n, 3)).astype(np.float32)
        out[tag + "_gamma"] = (30.0 * (1.0 + 0.2 * rng.standard_normal((B, 9, 128)))).astype(np.float32)
        out[tag + "_beta"] = (0.5 * rng.standard_normal((B, 9, 128))).astype(np.float32)
    return out


def _load_golden(name):
    import torch
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return {k: torch.from_numpy(np.asarray(f[k])) for k in f.files}


def pack_f16x3():
    """The golden weights packed for the f16x3 kernels (device tensor)."""
    from oi_amd import lib, ops
    from oi_amd.params import stack_field_params
    lib.load()
    P = stack_field_params({k: v.cuda() for k, v in _load_golden("weights_sdf").items()},
                           {k: v.cuda() for k, v in _load_golden("weights_color").items()})
    return ops.mlp_pack_weights(P["w0"], P["b0"], P["wh"], P["bh"], P["wsig"], P["bsig"], P["wv"], P["bv"], P["wrgb"],
                                P["brgb"], lib.OI_PREC_F16X3)


def run_call(packed, pts, gamma, beta, B, want_feat):
    """One ops.sdf_mlp_fwd call in the f16x3 precision with want_grad and want_rgb -> {name: uint32 ndarray}."""
    import torch
    from oi_amd import lib, ops
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pts, gamma, beta)]
    sdf, grad, rgb, feat, _ = ops.sdf_mlp_fwd(t[0], packed, t[1], t[2], B, lib.OI_PREC_F16X3, fast_trig=False, want_grad=True,
                                              want_rgb=True, want_feat=want_feat)
    torch.cuda.synchronize()
    out = {"sdf": sdf, "grad": grad, "rgb": rgb}
    if want_feat:
        out["feat"] = feat
    return {k: np.ascontiguousarray(v.detach().cpu().numpy()).view(np.uint32) for k, v in out.items()}


def digest(words):
    return hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest()


def replay(packed=None, inputs=None):
    """Both calls -> (outputs of (a) as uint32 words, {name: digest} of (b))."""
    inp = make_inputs() if inputs is None else inputs
    packed = pack_f16x3() if packed is None else packed
    a = run_call(packed, inp["a_pts"], inp["a_gamma"], inp["a_beta"], A_B, True)
    b = run_call(packed, inp["b_pts"], inp["b_gamma"], inp["b_beta"], B_B, False)
    return a, {k: digest(b[k]) for k in OUTPUTS_B}


def compare(fix, a, b):
    """Names of the outputs that differ from the fixture (empty = reproduced)."""
    bad = [f"a_{k}" for k in OUTPUTS_A if not np.array_equal(np.asarray(fix["a_out_" + k]), a[k])]
    bad += [f"b_{k}" for k in OUTPUTS_B if str(fix["b_sha256_" + k]) != b[k]]
    return bad


def _commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return os.environ.get("OI_COMMIT", "unknown")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--check", action="store_true", help="compare against the existing fixture instead of writing one")
    ap.add_argument("--commit", default=None, help="commit hash to store (default: git rev-parse HEAD, or $OI_COMMIT)")
    args = ap.parse_args()
    inp = make_inputs()
    a, b = replay(inputs=inp)
    for k, v in a.items():
        assert np.isfinite(v.view(np.float32)).all(), f"call (a): {k} is not finite"
    if args.check:
        with np.load(args.out) as fix:
            bad = compare(fix, a, b)
            print(f"fixture of commit {fix['commit']}: " + ("reproduced bit for bit" if not bad else "DIFFERS in " + ", ".join(bad)))
        sys.exit(1 if bad else 0)
    rec = {"a_pts": inp["a_pts"], "a_gamma": inp["a_gamma"], "a_beta": inp["a_beta"],
           "commit": np.array(args.commit or _commit())}
    for k in OUTPUTS_A:
        rec["a_out_" + k] = a[k]
    for k in OUTPUTS_B:
        rec["b_sha256_" + k] = np.array(b[k])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out} ({os.path.getsize(args.out)} bytes) at commit {rec['commit']}")
    for k in OUTPUTS_B:
        print(f"  (b) {k}: {b[k]}")


if __name__ == "__main__":
    main()
