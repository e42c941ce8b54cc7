"""oi_upsample / oi_upsample_mid / oi_merge_sorted (csrc/render.hip) against the float64 restatement of
tests/helpers/upsample_regimes.py, on every step of every regime: chains of a trained-sign field with hits, grazing rays and
misses, more than one scan chunk in sections and in new samples, forward noise, clustered samples with the -1e3 clamp active,
ties, the flat branch of the inverse CDF, the unit-sphere mask, rays without a surface.

Inputs, reference, populations, margins, caps and fp32 floors are rehearsed on the CPU by tests/test_upsample_regimes_cpu.py,
which also shows that each plausible kernel error fails the assertions made here (`R.judge`).  Value bar per (regime, step,
ray class) = 3x the committed fp32 floor, floored per sample at 4 ulp of z; the kernel's error is reported through
record_margin under upsample_regimes[<regime>][<step>] (profiles/upsample_regimes_margins.txt)."""
import numpy as np
import pytest
import torch

import oi_oracle as O
from conftest import record_margin
from helpers import upsample_regimes as R
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name,i", R.cases())
def test_step(guarded_ops, name, i):
    from oi_amd import ops
    ch = R.case(name)
    st = ch["steps"][i]
    n_new, inv_s, last_dist = st["n_new"], st["inv_s"], ch["last_dist"]
    ro, rd, z, sdf = (guarded_ops.copy(t.contiguous().cuda(), "input") for t in (ch["ro"], ch["rd"], st["z"], st["sdf"]))
    z_new, pts_new, z_m = ops.upsample(ro, rd, z, sdf, n_new, inv_s, merge=True)
    case = f"upsample_regimes[{name}][{i}]"
    print()
    for cls, (err, n) in R.cell_errors(st, z_new).items():
        record_margin(case, cls, err)
        print(f"  {case} {cls:10s} error {err:.3e}  floor {R.FP32_FLOOR[name][i][cls]:.3e}  bar {R.bar(name, i, cls):.3e}  decided {n}")
    # structural (all samples), bracket and value (decided samples)
    bad = R.judge(name, i, z_new, z_m)
    assert not bad, bad
    # the same launch without the merge writes the same z_new
    z_only, _, none = ops.upsample(ro, rd, z, sdf, n_new, inv_s, merge=False)
    assert none is None and torch.equal(_bits(z_only), _bits(z_new))
    # oi_upsample_mid == oi_upsample + oi_midpoints, bit for bit
    d_a = ops.midpoints(ro, rd, z_m, last_dist)
    b = ops.upsample(ro, rd, z, sdf, n_new, inv_s, mid_last_dist=last_dist)
    for what, x, y in zip(("z_new", "pts_new", "z_merged", "dists", "mid_z", "mid_pts"), (z_new, pts_new, z_m) + tuple(d_a),
                          tuple(b[:3]) + tuple(b[3])):
        assert torch.equal(_bits(x), _bits(y)), what
    dists, mid_z, mid_pts = (t.cpu() for t in b[3])
    assert bool((dists[:, -1] == torch.tensor(last_dist, dtype=torch.float32)).all()) and bool((dists >= 0).all())
    ro64, rd64 = ch["ro"].double(), ch["rd"].double()
    along = lambda zz: ro64[:, None] + rd64[:, None] * zz.double().cpu()[..., None]
    assert float((pts_new.cpu().double() - along(z_new)).abs().max()) < 1e-6
    assert float((mid_pts.double() - along(mid_z)).abs().max()) < 1e-6
    # oi_merge_sorted with the step's payload: keys exactly the oracle's, (key, payload) pairs as multisets where keys tie
    sdf_new = guarded_ops.copy(st["sdf_new"].contiguous().cuda(), "input")
    zo, so = ops.merge_sorted(z, sdf, z_new, sdf_new)
    zr, sr = O.merge_sorted(st["z"], z_new.cpu(), st["sdf"], st["sdf_new"])
    assert torch.equal(zo.cpu(), zr) and torch.equal(_bits(zo), _bits(z_m))
    a = np.stack([zo.cpu().numpy(), so.cpu().numpy()], -1)
    r = np.stack([zr.numpy(), sr.numpy()], -1)
    for k in range(a.shape[0]):
        ia, ir = np.lexsort((a[k, :, 1], a[k, :, 0])), np.lexsort((r[k, :, 1], r[k, :, 0]))
        assert np.array_equal(a[k][ia], r[k][ir]), k
    if name in ("ties", "flat"):   # the merge really met equal keys
        assert bool((zo[:, 1:] == zo[:, :-1]).any())
