"""Narrow-band mesh extraction on the MI355X (include/oi_mesh_band.h; oi_amd.mesh.sdf_lattice_band; the band= keyword of the
mesh entries): the band field against the dense field of the same call -- bit-equal in active blocks, the
same side of the level everywhere else -- the counts against the fp64 restatement (tests/helpers/band_ref.py) fed with the
GPU's own coarse values, and the meshes, records and files against the dense path's, byte for byte.

The lattices are those of tests/test_mesh_band_cpu.py's rehearsal: at the default lipschitz the smaller ones the feature was
first proposed with (128^3, (97, 102, 131)) have no inactive block at all, and the comparison would be vacuous."""
import ctypes
import os

import numpy as np
import pytest
import torch

import test_gpu_modules as GM
from conftest import GOLDEN, load_golden, sub_sd
from helpers import band_ref as R
from helpers.guarded import GuardSet
from test_mesh_band_cpu import BMAX, BMIN, GPU_LATTICES

pytestmark = [pytest.mark.gpu]

KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
_NETS, _DENSE = {}, {}


def shape_net(precision):
    if precision not in _NETS:
        from oi_amd.fields import ShapeNetwork
        net = ShapeNetwork(os.path.join(GOLDEN, "weights_sdf.npz"), **KW).cuda()
        net._own_pack().set_precision(precision)
        _NETS[precision] = net
    return _NETS[precision]


def latent(seed):
    return torch.randn(1, 64, generator=torch.Generator().manual_seed(seed)).cuda()


def dense_field(precision, res, seed):
    """The dense u = -sdf of the same call, computed once per (precision, lattice, latent) and never modified."""
    from oi_amd import mesh
    key = (precision, tuple(res), seed)
    if key not in _DENSE:
        if len(_DENSE) >= 4:   # at most ~2.5 GB of reference fields alive
            _DENSE.pop(next(iter(_DENSE)))
        _DENSE[key] = mesh.sdf_lattice(shape_net(precision), BMIN, BMAX, res, z=latent(seed), scale=-1.0)
    return _DENSE[key]


def active_points(info, res):
    """bool (nx, ny, nz): the point lies in a block of the active list."""
    nb = R.n_blocks(res, info.block)
    m = torch.zeros(int(np.prod(nb)), dtype=torch.bool, device="cuda")
    m[info.active_list.long()] = True
    m = m.view(nb)
    for a in range(3):
        m = m.repeat_interleave(info.block, dim=a)
    return m[:res[0], :res[1], :res[2]]


def check_field(precision, res, seed, iso, block):
    from oi_amd import mesh
    dense = dense_field(precision, res, seed)
    field, info = mesh.sdf_lattice_band(shape_net(precision), BMIN, BMAX, res, iso, z=latent(seed), scale=-1.0, block=block)
    assert field.shape == dense.shape == (1,) + tuple(res)
    act = active_points(info, res)
    assert int(info.active_list.numel()) == info.active_blocks == len(torch.unique(info.active_list))
    # bit-equal at every point of an active block
    assert torch.equal(field[0].view(torch.int32)[act], dense[0].view(torch.int32)[act])
    # the same side of the level at every other point
    assert torch.equal((field[0] > iso)[~act], (dense[0] > iso)[~act])
    # exact counts: the restatement on the GPU's own coarse values
    ref = R.classify(info.coarse.cpu().numpy(), iso, -1.0, info.lipschitz, R.spacings(BMIN, BMAX, res), block)
    assert (info.blocks, info.active_blocks, info.inactive_above, info.inactive_below) == \
        (ref["blocks"], ref["active"], ref["inactive_above"], ref["inactive_below"])
    assert info.points_evaluated == info.blocks + info.active_blocks * block ** 3
    assert abs(info.max_slope - ref["max_slope"]) <= 1e-6 * ref["max_slope"] and info.max_slope <= info.lipschitz
    ids = np.flatnonzero(~ref["inactive"].reshape(-1))
    assert np.array_equal(np.sort(info.active_list.cpu().numpy()), ids)
    print(f"{precision} {res} latent {seed} iso {iso} block {block}: inactive {info.inactive_blocks} of {info.blocks} "
          f"(above {info.inactive_above}, below {info.inactive_below}), slope {info.max_slope:.3f}")
    assert info.inactive_blocks >= 0.25 * info.blocks
    return field, info


def test_library_exports_the_band_entries():
    from oi_amd import lib
    L = ctypes.CDLL(lib.LIB_PATH)
    for n in ("oi_sdf_lattice_band", "oi_band_classify", "oi_band_workspace_bytes"):
        assert hasattr(L, n), n


@pytest.mark.parametrize("block", [4, 8])
@pytest.mark.parametrize("iso", [0.0, 0.05])
@pytest.mark.parametrize("seed", [0, 2])
@pytest.mark.parametrize("res", GPU_LATTICES)
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_band_field_against_the_dense_field(precision, res, seed, iso, block):
    check_field(precision, res, seed, iso, block)


def test_band_field_bf16():
    check_field("bf16", GPU_LATTICES[1], 0, 0.0, 4)


def test_two_calls_are_byte_identical():
    from oi_amd import mesh
    net, res = shape_net("f16x3"), GPU_LATTICES[1]
    a, ia = mesh.sdf_lattice_band(net, BMIN, BMAX, res, 0.0, z=latent(0), scale=-1.0, block=4)
    b, ib = mesh.sdf_lattice_band(net, BMIN, BMAX, res, 0.0, z=latent(0), scale=-1.0, block=4)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(torch.sort(ia.active_list).values, torch.sort(ib.active_list).values)
    assert (ia.active_blocks, ia.inactive_above, ia.inactive_below, ia.max_slope) == \
        (ib.active_blocks, ib.inactive_above, ib.inactive_below, ib.max_slope)


@pytest.mark.parametrize("block", [4, 8])
@pytest.mark.parametrize("res", [(2, 2, 2), (5, 4, 9), (9, 17, 3)])
def test_tiny_and_ragged_lattices_through_guarded_buffers(res, block):
    """Every block is active (the threshold is far above every value): the block-list point source and its ragged ends write
    the whole field, bit-equal to the dense one, and nothing beyond it."""
    from oi_amd import lib, mesh
    from oi_amd.ops import _p, _stream
    L = lib.load()
    net = shape_net("f16x3")
    pack = net._own_pack()
    z = latent(1)
    dense = mesh.sdf_lattice(net, BMIN, BMAX, res, z=z, scale=-1.0)
    gs = GuardSet()
    with torch.no_grad():
        _, gamma, beta = pack.film(z=z)
    gamma, beta, packed = gs.copy(gamma.contiguous(), "gamma"), gs.copy(beta.contiguous(), "beta"), pack.packed()
    ax = [gs.copy(a, "axis") for a in mesh._axes(BMIN, BMAX, res, "cuda")]
    cax = [gs.copy(torch.from_numpy(c.astype(np.float32)).cuda(), "centre axis") for c in R.centre_axes(BMIN, BMAX, res, block)]
    nb = R.n_blocks(res, block)
    coarse = gs.empty(nb, what="coarse")
    st, fast = _stream(), int(bool(pack.fast_trig))
    assert L.oi_sdf_lattice(_p(packed), _p(gamma), _p(beta), 1, _p(cax[0]), _p(cax[1]), _p(cax[2]), *nb, -1.0, _p(coarse),
                            pack.prec, fast, st) == 0
    nbytes = L.oi_band_workspace_bytes(*res, block)
    ws = gs.scratch(nbytes, what="workspace")
    field = gs.empty(res, what="field")
    counts, slope = (ctypes.c_longlong * 4)(), ctypes.c_float()
    h = R.spacings(BMIN, BMAX, res)
    assert L.oi_band_classify(_p(coarse), 1, *res, block, h[0], h[1], h[2], 0.0, -1.0, mesh.DEFAULT_LIPSCHITZ, _p(field), _p(ws),
                              nbytes, counts, ctypes.byref(slope), st) == 0, L.oi_last_error()
    assert list(counts) == [int(np.prod(nb)), int(np.prod(nb)), 0, 0]
    assert L.oi_sdf_lattice_band(_p(packed), _p(gamma), _p(beta), 1, _p(ax[0]), _p(ax[1]), _p(ax[2]), *res, block, _p(ws),
                                 counts[1], -1.0, _p(field), pack.prec, fast, st) == 0, L.oi_last_error()
    assert torch.equal(field.view(torch.int32), dense[0].view(torch.int32))
    problems = gs.close()
    assert not problems, problems
    # and through the Python entry
    f2, info = mesh.sdf_lattice_band(net, BMIN, BMAX, res, 0.0, z=z, scale=-1.0, block=block)
    assert torch.equal(f2.view(torch.int32), dense.view(torch.int32)) and info.inactive_blocks == 0


def _renderer(precision):
    r = GM.make_renderer(load_golden("weights_color"), 16, 16, 1, precision)
    r.sdf_network._own_pack().set_precision(precision)
    return r


@pytest.mark.parametrize("res", GPU_LATTICES)
@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_extract_geometry_band_is_byte_identical(precision, res):
    r = _renderer(precision)
    z = latent(0)
    bmin, bmax = torch.tensor(BMIN), torch.tensor(BMAX)
    # extract_geometry takes one resolution: the cubic lattice through the method, the anisotropic one through its steps
    from oi_amd import mesh
    if len(set(res)) == 1:
        v0, t0 = r.extract_geometry(bmin, bmax, res[0], threshold=0.0, z=z)
        v1, t1 = r.extract_geometry(bmin, bmax, res[0], threshold=0.0, z=z, band=True)
    else:
        u0, _ = mesh._level_field(r.pack, bmin, bmax, res, 0.0, z, None, False, None, None, "test")
        u1, info = mesh._level_field(r.pack, bmin, bmax, res, 0.0, z, None, True, None, None, "test")
        assert info.inactive_blocks >= 0.25 * info.blocks
        (v0, t0), (v1, t1) = ([a.cpu().numpy() for a in mesh.marching_cubes(u, 0.0)] for u in (u0, u1))
    assert len(t0) > 100000
    assert v0.tobytes() == v1.tobytes() and t0.tobytes() == t1.tobytes()


def test_extract_intrinsic_mesh_band_records_are_byte_identical():
    from oi_amd import mesh
    r = _renderer("f16x3")
    z = latent(2)
    a = mesh.extract_intrinsic_mesh(r, z=z, resolution=512, threshold=0.05, refine=2, want_record=True)
    b = mesh.extract_intrinsic_mesh(r, z=z, resolution=512, threshold=0.05, refine=2, want_record=True, band=True)
    assert a.band is None and b.band.inactive_blocks >= 0.25 * b.band.blocks
    assert len(a.record) > 100000
    assert torch.equal(a.record, b.record) and torch.equal(a.triangles, b.triangles)
    v0 = r.extract_intrinsic_geometry(torch.tensor(BMIN), torch.tensor(BMAX), 512, threshold=0.05, z=z, band=True)
    assert np.array_equal(v0[0], a.positions.cpu().numpy().astype(np.float64))


def test_export_mesh_band_writes_the_same_file(tmp_path):
    from oi_amd import inference
    g = load_golden("f5_generator")
    gen = GM.build_generator(16, 16, 16, 1, "f16x3").eval()
    gen.color_network.load_state_dict(sub_sd(g, "color."))
    z = g["z"]
    pa, pb = tmp_path / "dense.ply", tmp_path / "band.ply"
    inference.export_mesh(gen, z[0], str(pa), resolution=512)
    m = inference.export_mesh(gen, z[0], str(pb), resolution=512, band=True)
    assert m.band is not None and m.band.active_blocks < m.band.blocks
    assert pa.stat().st_size > 1 << 20 and pa.read_bytes() == pb.read_bytes()


def test_refusals_come_before_any_launch():
    from oi_amd import mesh
    net = shape_net("f16x3")
    z = latent(0)
    for kw, text in ((dict(z=torch.cat([z, z])), "batch of 2"), (dict(block=5), "block=5"), (dict(lipschitz=0.0), "lipschitz"),
                     (dict(lipschitz=float("nan")), "lipschitz"), (dict(lipschitz=-2.0), "lipschitz"),
                     (dict(res=(64, 1, 64)), "lattice 64 x 1 x 64")):
        kw = dict(kw)
        before = torch.cuda.memory_allocated()
        with pytest.raises(ValueError, match=text):
            mesh.sdf_lattice_band(net, BMIN, BMAX, kw.pop("res", 64), 0.0, z=kw.pop("z", z), **kw)
        assert torch.cuda.memory_allocated() == before   # nothing was allocated, let alone launched
    r = _renderer("f16x3")
    with pytest.raises(ValueError, match="block=5"):
        r.extract_geometry(torch.tensor(BMIN), torch.tensor(BMAX), 64, z=z, band=True, block=5)


def test_slope_guard_refuses_a_wrong_bound():
    from oi_amd import mesh
    r = _renderer("f16x3")
    z = latent(0)
    with pytest.raises(ValueError, match=r"slope .* above lipschitz=0.05"):
        mesh.sdf_lattice_band(r.pack, BMIN, BMAX, 128, 0.0, z=z, scale=-1.0, lipschitz=0.05)
    with pytest.raises(ValueError, match="slope"):
        r.extract_geometry(torch.tensor(BMIN), torch.tensor(BMAX), 128, z=z, band=True, lipschitz=0.05)


def test_non_finite_field_keeps_every_block_active_and_marching_cubes_refuses():
    """A pack with one NaN weight: every centre value is NaN, so every block is active, the field is the dense NaN field and
    marching cubes fails with its own error (OI_ERR_INVALID_ARG); nothing faults."""
    from oi_amd import lib, mesh
    from oi_amd.fields import ShapeNetwork
    net = ShapeNetwork(os.path.join(GOLDEN, "weights_sdf.npz"), **KW).cuda()
    with torch.no_grad():
        net.pts_linears[3].weight[5, 7] = float("nan")
    net._own_pack().set_precision("f16x3")
    res = (40, 33, 21)
    field, info = mesh.sdf_lattice_band(net, BMIN, BMAX, res, 0.0, z=latent(0), scale=-1.0)
    assert info.active_blocks == info.blocks and info.inactive_blocks == 0 and info.max_slope == 0.0
    assert not bool(torch.isfinite(field).any())
    with pytest.raises(lib.OiHipError, match="non-finite"):
        mesh.marching_cubes(field[0], 0.0)
