"""CPU checks of narrow-band mesh extraction (include/oi_mesh_band.h, oi_amd.mesh.sdf_lattice_band):
the rule restated in float64 (tests/helpers/band_ref.py) on analytic fields with a known bound on the gradient, header <=>
library <=> binding, the refusals that need no device, and the REHEARSAL of the rule on the fp64 oracle with the golden
weights at the lattices tests/test_gpu_mesh_band.py uses.

Rehearsal (oracle alone, float64, box [-1, 1]^3, lipschitz = the default 20, latents 0 - 2, iso 0 and 0.05 on u = -sdf).
The lattices the issue proposed, 128^3 and (97, 102, 131), have NO inactive block at the default bound (threshold
|scale| G m = 1.36 .. 2.46, above every |u| in the box), so the GPU lattices are the larger 512^3 and (485, 510, 655), where
every case has at least a quarter of its blocks inactive (measured here: 512^3 block 8 0.279 .. 0.384, block 4 0.700 .. 0.757;
(485, 510, 655) block 8 0.331 .. 0.436, block 4 0.720 .. 0.774; inactive blocks above the level exist only for block 4, a few
hundred).  A dense float64 field of 1.3e8 points is out of reach of the oracle, and so are the points of the active blocks; the
rehearsal evaluates the block centres (all of them up to 3e5 blocks, a random 1e5 beyond, the inactive share then being that
of the sample) and, per latent and iso, 17 000 random cells with a corner in an inactive block, all eight corners:
no such cell is crossed by the level and the corner has its centre's sign."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from helpers import band_ref as R
from helpers import cabi
from helpers import mc_numpy as M

BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
GPU_LATTICES = [(512, 512, 512), (485, 510, 655)]     # tests/test_gpu_mesh_band.py imports these


def _sphere(P, c=(0.05, -0.1, 0.0), r=0.55):
    return np.linalg.norm(P - np.asarray(c), axis=-1) - r


def _torus(P, R0=0.5, r0=0.2):
    q = np.sqrt(P[:, 0] ** 2 + P[:, 1] ** 2) - R0
    return np.sqrt(q * q + P[:, 2] ** 2) - r0


def _two_spheres(P):
    return np.minimum(_sphere(P, (-0.3, 0.0, 0.1), 0.35), _sphere(P, (0.35, 0.1, -0.05), 0.3))


# name -> (field, the exact bound G on its gradient)
FIELDS = {"sphere": (_sphere, 1.0), "torus": (_torus, 1.0), "two_spheres": (_two_spheres, 1.0),
          "sphere_x3": (lambda P: 3.0 * _sphere(P), 3.0)}
LATTICES = [(33, 33, 33), (97, 102, 131), (130, 9, 40)]


@pytest.mark.parametrize("block", [4, 8])
@pytest.mark.parametrize("res", LATTICES)
@pytest.mark.parametrize("name", sorted(FIELDS))
def test_rule_on_analytic_fields(name, res, block):
    f, G = FIELDS[name]
    some_inactive = False
    for scale in (1.0, -1.0):
        for iso in (0.0, 0.05):
            b = R.band(f, BMIN, BMAX, res, iso, scale, G, block)
            dense, field, inact = b["dense"], b["field"], b["inactive_points"]
            assert b["active"] + b["inactive_above"] + b["inactive_below"] == b["blocks"] == int(np.prod(R.n_blocks(res, block)))
            # every corner of every level-crossing cell lies in an active block
            assert not (R.crossed_corners(dense, iso) & inact).any()
            # every point of an inactive block has its centre's sign
            assert np.array_equal((dense > iso)[inact], (field > iso)[inact])
            assert np.array_equal(field[~inact], dense[~inact])
            # the guard's slope is a lower bound of the true constant
            assert b["max_slope"] <= G * (1 + 1e-12)
            some_inactive |= bool(inact.any())
            va, ta = M.marching_cubes(field, iso)
            vb, tb = M.marching_cubes(dense, iso)
            assert len(tb) > 0
            assert np.array_equal(ta, tb) and va.tobytes() == vb.tobytes()
    if res == (97, 102, 131) and block == 4:
        assert some_inactive   # the comparison is not vacuous where the lattice is fine enough


def test_distance_bound_and_centres():
    h = np.array([0.1, 0.1, 0.1])
    for b in (4, 8):
        assert abs(R.distance_bound(h, b) - np.sqrt(3) * 0.1 * (1 + (b - 1) / 2)) < 1e-15
    h = np.array([0.3, 0.04, 0.1])
    assert abs(R.distance_bound(h, 4) - np.linalg.norm(h) * 2.5) < 1e-15
    cax = R.centre_axes((-1, 0, 2), (1, 1, 4), (9, 5, 8), 4)
    assert [len(c) for c in cax] == [3, 2, 2]
    assert np.allclose(cax[0], -1 + (np.array([1.5, 5.5, 9.5])) * 0.25)      # the ragged block's centre lies outside the box
    assert np.allclose(cax[2], 2 + np.array([1.5, 5.5]) * (2 / 7))
    # a non-finite centre value keeps its block active
    uc = np.array([[[5.0, np.nan], [np.inf, -5.0]]])
    c = R.classify(uc, 0.0, 1.0, 1.0, (0.01,) * 3, 4)
    assert c["inactive"].tolist() == [[[True, False], [False, True]]] and (c["inactive_above"], c["inactive_below"]) == (1, 1)


def test_slope_guard_fires_when_the_bound_is_halved():
    f, G = FIELDS["sphere_x3"]
    for block in (4, 8):
        b = R.band(f, BMIN, BMAX, (33, 33, 33), 0.0, 1.0, G / 2, block)
        assert b["max_slope"] > G / 2, b["max_slope"]
        assert R.band(f, BMIN, BMAX, (33, 33, 33), 0.0, 1.0, G, block)["max_slope"] <= G


# ---------------------------------------------------------------------------------------------------------------------
# header <=> library <=> binding, refusals
# ---------------------------------------------------------------------------------------------------------------------
_lib = cabi.built_lib


def test_library_exports_every_mesh_band_symbol():
    lib, L = _lib()
    names, _ = cabi.check_header("oi_mesh_band.h", lib)
    assert sorted(names) == ["oi_band_classify", "oi_band_workspace_bytes", "oi_sdf_lattice_band"]
    text = cabi.read("oi_mesh_band.h")
    assert int(re.search(r"#define OI_BAND_MIN_RES (\d+)", text).group(1)) == lib.BAND_MIN_RES
    assert int(re.search(r"#define OI_BAND_MAX_RES (\d+)", text).group(1)) == lib.BAND_MAX_RES
    assert '"mesh_band.hip"' in open(os.path.join(ROOT, "object-intrinsics_amd", "build.py")).read()
    assert L.oi_band_workspace_bytes(512, 512, 512, 4) == 4 * 128 ** 3 + 256
    assert L.oi_band_workspace_bytes(5, 4, 9, 8) == 256 + 256


def test_c_abi_rejects_invalid_arguments_before_launching():
    """Checked on the host before any HIP call: these run without a device (the pointers are never dereferenced)."""
    lib, L = _lib()
    f = ctypes.c_void_p(0x1000)
    cnt, sl = (ctypes.c_longlong * 4)(), ctypes.c_float()

    def classify(B=1, n=(16, 16, 16), block=4, h=(0.1, 0.1, 0.1), iso=0.0, scale=1.0, G=1.0, nbytes=1 << 20, coarse=f):
        return L.oi_band_classify(coarse, B, n[0], n[1], n[2], block, h[0], h[1], h[2], iso, scale, G, f, f, nbytes, cnt,
                                  ctypes.byref(sl), None)

    def band(B=1, n=(16, 16, 16), block=4, n_active=3, lst=f, prec=4):
        return L.oi_sdf_lattice_band(f, f, f, B, f, f, f, n[0], n[1], n[2], block, lst, n_active, 1.0, f, prec, 0, None)

    nan, inf = float("nan"), float("inf")
    cases = [(lambda: classify(B=2), "oi_band_classify", "B=2"), (lambda: classify(block=5), "oi_band_classify", "block=5"),
             (lambda: classify(n=(1, 16, 16)), "oi_band_classify", "lattice 1 x 16 x 16"),
             (lambda: classify(n=(16, 1025, 16)), "oi_band_classify", "lattice 16 x 1025 x 16"),
             (lambda: classify(G=0.0), "oi_band_classify", "lipschitz"), (lambda: classify(G=nan), "oi_band_classify", "lipschitz"),
             (lambda: classify(G=-1.0), "oi_band_classify", "lipschitz"), (lambda: classify(G=inf), "oi_band_classify", "lipschitz"),
             (lambda: classify(h=(0.1, 0.0, 0.1)), "oi_band_classify", "spacings"),
             (lambda: classify(scale=0.0), "oi_band_classify", "scale"), (lambda: classify(iso=nan), "oi_band_classify", "iso"),
             (lambda: classify(coarse=None), "oi_band_classify", "null"),
             (lambda: classify(nbytes=64), "oi_band_classify", "workspace"),
             (lambda: band(B=2), "oi_sdf_lattice_band", "B=2"), (lambda: band(block=16), "oi_sdf_lattice_band", "block=16"),
             (lambda: band(n=(16, 16, 1)), "oi_sdf_lattice_band", "lattice 16 x 16 x 1"),
             (lambda: band(n_active=65), "oi_sdf_lattice_band", "n_active=65"),
             (lambda: band(n_active=-1), "oi_sdf_lattice_band", "n_active=-1"),
             (lambda: band(lst=None), "oi_sdf_lattice_band", "null"), (lambda: band(prec=9), "oi_sdf_lattice_band", "precision")]
    for call, entry, text in cases:
        assert call() == -1, (entry, text)
        msg = L.oi_last_error().decode()
        assert msg.startswith(entry) and text in msg, (entry, text, msg)
    assert L.oi_band_workspace_bytes(16, 16, 16, 5) == 0 and L.oi_band_workspace_bytes(1, 16, 16, 4) == 0
    assert band(n_active=0, lst=None) == 0    # nothing to launch


def test_python_refusals_need_no_device():
    from oi_amd import mesh
    from oi_amd.fields import ShapeNetwork
    net = ShapeNetwork(None, D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
    z = torch.zeros(1, 64)
    call = lambda **kw: mesh.sdf_lattice_band(net, BMIN, BMAX, kw.pop("res", 16), 0.0, z=kw.pop("z", z), **kw)
    with pytest.raises(ValueError, match="batch of 2"):
        call(z=torch.zeros(2, 64))
    with pytest.raises(ValueError, match="block=5"):
        call(block=5)
    for bad in (0, 0.0, float("nan"), -3.0, float("inf"), True):
        with pytest.raises(ValueError, match="lipschitz"):
            call(lipschitz=bad)
    with pytest.raises(ValueError, match="lattice 16 x 1 x 16"):
        call(res=(16, 1, 16))
    with pytest.raises(ValueError, match="latent"):
        mesh.sdf_lattice_band(net, BMIN, BMAX, 16, 0.0)
    with pytest.raises(ValueError, match="band=True"):
        mesh._level_field(net, BMIN, BMAX, 16, 0.0, z, None, False, 3.0, None, "extract_geometry")
    assert mesh.DEFAULT_BLOCK in (4, 8) and mesh.DEFAULT_LIPSCHITZ == 20.0


# ---------------------------------------------------------------------------------------------------------------------
# rehearsal on the oracle (see the module docstring)
# ---------------------------------------------------------------------------------------------------------------------
N_CELLS, MAX_CENTRES = 17000, 100000   # per latent and iso: 6 x 17 000 = 102 000 designated corners per case


@pytest.mark.parametrize("block", [4, 8])
@pytest.mark.parametrize("res", GPU_LATTICES)
def test_rehearsal_on_the_oracle(res, block):
    import oi_oracle as O
    from helpers import mesh_attr_ref as A
    from oi_amd import mesh
    G = mesh.DEFAULT_LIPSCHITZ
    sd, _ = A.golden_state()
    h = R.spacings(BMIN, BMAX, res)
    nb = R.n_blocks(res, block)
    cax = R.centre_axes(BMIN, BMAX, res, block)
    ax = R.axes(BMIN, BMAX, res)
    thr = G * R.distance_bound(h, block)
    nblk = int(np.prod(nb))
    for seed in (0, 1, 2):
        rs = np.random.RandomState(100 + seed)
        w = O.style_mlp(sd, A.latent(seed).double())
        u_at = lambda P: -A.field(sd, None, w, P)[0]
        ids = np.arange(nblk) if nblk <= 3 * MAX_CENTRES else np.sort(rs.choice(nblk, MAX_CENTRES, replace=False))
        bi, bj, bk = np.unravel_index(ids, nb)
        uc = u_at(np.stack([cax[0][bi], cax[1][bj], cax[2][bk]], -1))
        assert np.isfinite(uc).all()
        for iso in (0.0, 0.05):
            inactive = np.abs(uc - iso) > thr
            n_above, n_below = int((inactive & (uc > iso)).sum()), int((inactive & (uc < iso)).sum())
            print(f"rehearsal {res} block {block} latent {seed} iso {iso}: {len(ids)} of {nblk} centres, threshold {thr:.3f}, "
                  f"inactive above {n_above} below {n_below} ({inactive.mean():.3f})")
            assert inactive.mean() >= 0.25, (res, block, seed, iso, float(inactive.mean()))
            # random cells with a corner p in an inactive block: p is a random point of a random inactive block (inside the
            # lattice), the cell a random one of the eight around p
            pick = rs.choice(np.flatnonzero(inactive), N_CELLS)
            p = np.stack([b_ * block + rs.randint(0, block, N_CELLS) for b_ in (bi[pick], bj[pick], bk[pick])], -1)
            n = np.asarray(res)
            p = np.minimum(p, n - 1)                                   # ragged last blocks
            origin = np.clip(p - rs.randint(0, 2, (N_CELLS, 3)), 0, n - 2)
            corners = origin[:, None, :] + np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)])[None]
            P = np.stack([ax[a][corners[..., a]] for a in range(3)], -1)
            inside = (u_at(P.reshape(-1, 3)).reshape(N_CELLS, 8) > iso)
            crossed = inside.any(1) != inside.all(1)
            assert not crossed.any(), (res, block, seed, iso, int(crossed.sum()))
            assert np.array_equal(inside[:, 0], uc[pick] > iso)        # with no crossing: every corner has the centre's sign
