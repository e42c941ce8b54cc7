"""Mesh extraction on the MI355X: the lattice SDF kernel (oi_sdf_lattice) against the sdf-only path and the oracle, the GPU
marching cubes (oi_mc_count / oi_mc_emit) against the numpy restatement of tests/helpers/mc_numpy.py, and
NeuSRenderer.extract_geometry end to end.  Golden weights: tests/golden/weights_sdf.npz."""
import os

import numpy as np
import pytest
import torch

import oi_oracle as O
from conftest import GOLDEN
from helpers import mc_numpy as M
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)


def shape_net(precision="f16x3"):
    from oi_amd.fields import ShapeNetwork
    net = ShapeNetwork(os.path.join(GOLDEN, "weights_sdf.npz"), **KW).cuda()
    net._own_pack().set_precision(precision)
    return net


def latent(seed, B=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 64, generator=g).cuda()


def meshgrid_points(bmin, bmax, res):
    xs, ys, zs = (torch.linspace(bmin[a], bmax[a], res[a], device="cuda") for a in range(3))
    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
    return torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1).contiguous()


BMIN, BMAX, RES = (-1.1, -0.7, -0.9), (0.95, 1.2, 0.6), (33, 64, 17)


@pytest.mark.parametrize("precision", ["f16x3", "bf16", "f32", "bf16x3", "bf16x6"])
def test_lattice_matches_sdf_path_bit_for_bit(precision):
    from oi_amd import mesh
    net = shape_net(precision)
    z = latent(0)
    field = mesh.sdf_lattice(net, BMIN, BMAX, RES, z=z)
    assert field.shape == (1,) + RES
    with torch.no_grad():
        ref = net.sdf(meshgrid_points(BMIN, BMAX, RES), z).view(RES)
    assert torch.equal(field[0], ref), float((field[0] - ref).abs().max())
    neg = mesh.sdf_lattice(net, BMIN, BMAX, RES, z=z, scale=-1.0)
    assert torch.equal(neg, -field)


def test_lattice_matches_oracle():
    from oi_amd import mesh
    net = shape_net("f16x3")
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    z = latent(1)
    field = mesh.sdf_lattice(net, BMIN, BMAX, RES, z=z)[0].cpu().reshape(-1)
    ref = O.sdf_forward(sd, meshgrid_points(BMIN, BMAX, RES).cpu(), O.style_mlp(sd, z.cpu()))[0].squeeze(-1)
    assert float((field - ref).abs().max()) < 1e-4


def test_lattice_batch_equals_single_calls():
    from oi_amd import mesh
    net = shape_net()
    z = latent(2, B=2)
    both = mesh.sdf_lattice(net, BMIN, BMAX, RES, z=z)
    for b in range(2):
        assert torch.equal(both[b], mesh.sdf_lattice(net, BMIN, BMAX, RES, z=z[b:b + 1])[0])


def test_extract_fields_matches_reference_chunk_loop():
    from oi_amd import mesh
    net = shape_net()
    z = latent(0)
    bmin, bmax, R = torch.tensor([-1.0, -1, -1]), torch.tensor([1.0, 1, 1]), 80  # two chunks per axis, one ragged
    q = lambda p: -net.sdf(p, z)
    u = mesh.extract_fields(bmin, bmax, R, q)
    # the reference's loop (renderer.py:15-31), restated
    N = 64
    X, Y, Z = (torch.linspace(bmin[a], bmax[a], R, device="cuda").split(N) for a in range(3))
    ref = np.zeros([R, R, R], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    ref[xi * N: xi * N + len(xs), yi * N: yi * N + len(ys), zi * N: zi * N + len(zs)] = \
                        q(pts).reshape(len(xs), len(ys), len(zs)).cpu().numpy()
    assert u.dtype == np.float32 and u.shape == (R, R, R)
    assert np.array_equal(u, ref)
    lat = mesh.sdf_lattice(net, bmin, bmax, R, z=z, scale=-1.0)[0].cpu().numpy()
    assert np.array_equal(u, lat)


def _analytic(name, R=64):
    g = np.arange(R, dtype=np.float64)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    c = (R - 1) / 2
    if name == "sphere":
        return (0.35 * R - np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2)).astype(np.float32)
    u = np.random.default_rng(7).standard_normal((R, R, R)).astype(np.float32)
    u[:2], u[-2:], u[:, :2], u[:, -2:], u[:, :, :2], u[:, :, -2:] = -1, -1, -1, -1, -1, -1
    return u


def _golden_field(R=64, seed=0):
    from oi_amd import mesh
    return mesh.sdf_lattice(shape_net(), (-1.0,) * 3, (1.0,) * 3, R, z=latent(seed), scale=-1.0)[0]


@pytest.mark.parametrize("threshold", [0.0, 0.05])
@pytest.mark.parametrize("name", ["sphere", "noise", "golden"])
def test_gpu_marching_cubes_matches_numpy(name, threshold):
    from oi_amd import mesh
    u = _golden_field().cpu().numpy() if name == "golden" else _analytic(name)
    vr, tr = M.marching_cubes(u, threshold)
    v, t = mesh.marching_cubes(torch.from_numpy(u).cuda(), threshold)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda and t.is_cuda
    assert len(tr) > 100
    assert np.array_equal(t.cpu().numpy().astype(np.int64), tr)
    assert float(np.abs(v.cpu().numpy() - vr).max()) <= 1e-6
    vn, tn = mesh.marching_cubes(u, threshold)  # numpy in, numpy out
    assert vn.dtype == np.float64 and tn.dtype == np.int64
    assert np.array_equal(tn, tr) and np.array_equal(vn, v.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_golden_field_mesh_closed_and_volume(seed):
    from oi_amd import mesh
    R = 96
    u = _golden_field(R, seed)
    v, t = mesh.marching_cubes(u, 0.0)
    v, t = v.cpu().numpy().astype(np.float64), t.cpu().numpy()
    assert M.directed_edges_balanced(t)
    vol = M.signed_volume(v, t)
    inside = int((u > 0).sum())
    assert vol > 0
    assert abs(vol - inside) < 0.03 * inside, (vol, inside)


def test_marching_cubes_deterministic_and_edge_cases():
    from oi_amd import mesh, lib
    u = torch.from_numpy(_analytic("noise")).cuda()
    a = mesh.marching_cubes(u, 0.0)
    b = mesh.marching_cubes(u, 0.0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    v, t = mesh.marching_cubes(np.full((9, 10, 11), -1.0, dtype=np.float32), 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t = mesh.marching_cubes(torch.full((9, 10, 11), 1.0, device="cuda"), 0.0)
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3)
    bad = u.clone()
    bad[30, 31, 32] = float("nan")
    with pytest.raises(lib.OiHipError, match="non-finite"):
        mesh.marching_cubes(bad, 0.0)
    big = torch.zeros(1025, 2, 2, device="cuda")
    before = torch.cuda.memory_allocated()
    with pytest.raises(lib.OiHipError, match="2..1024"):
        mesh.marching_cubes(big, 0.0)
    assert torch.cuda.memory_allocated() == before  # refused before the workspace is allocated
    with pytest.raises(lib.OiHipError):
        mesh.marching_cubes(torch.zeros(1, 8, 8, device="cuda"), 0.0)


def test_renderer_extract_geometry_end_to_end():
    from oi_amd import mesh
    from oi_amd.fields import ColorNetwork, SingleVarianceNetwork
    from oi_amd.renderer import NeuSRenderer
    net = shape_net()
    r = NeuSRenderer(None, net, SingleVarianceNetwork(0.3).cuda(), ColorNetwork(**KW).cuda(), 16, 16, 0, 1, 0)
    z = latent(0)
    bmin, bmax = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    v, t = r.extract_geometry(bmin, bmax, 72, threshold=0.0, z=z)
    vr, tr = mesh.extract_geometry(bmin, bmax, 72, 0.0, lambda p: -net.sdf(p, z))
    assert v.dtype == np.float64 and t.dtype == np.int64 and len(t) > 1000
    assert np.array_equal(t, tr) and np.array_equal(v, vr)
    assert v.min() >= -1.0 and v.max() <= 1.0
