"""Intrinsic mesh export on the MI355X (include/oi_mesh_attr.h; oi_amd.mesh.vertex_attributes / extract_intrinsic_mesh;
NeuSRenderer.extract_intrinsic_geometry; oi_amd.inference.export_mesh).  The reference is always the fp64 CPU oracle
(oracle/oi_oracle.py through tests/helpers/mesh_attr_ref.py) on the golden weights and the seeded latents 0, 1, 2, evaluated
AT THE POSITIONS THE LIBRARY RETURNS.  The caps on flagged vertices and disagreeing faces (zero) come from the rehearsal of
tests/test_mesh_attrs_cpu.py on the oracle alone."""
import ctypes

import numpy as np
import pytest
import torch

import oi_oracle as O
import test_gpu_modules as M
from conftest import load_golden, record_margin, sub_sd
from helpers import mesh_attr_ref as A
from helpers.guarded import guarded_copy, guarded_empty, guarded_ops  # noqa: F401  (fixture)
from helpers.relight_ref import relight_ref

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]

SDF_BAR = 1e-4      # F1: sdf parity (and 1e-4 of the largest gradient entry for the gradient)
RGB_BAR = 2e-5      # F2: albedo parity
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
# bf16 rows carry 3x the measured worst.  Measured on one MI355X, seeds 0, 1, 2, threshold 0: the worst
# oracle residual |sdf| / |grad| after two steps, per resolution (test_on_the_surface_bf16 has the other figures)
BF16_MEASURED_WORST = {64: 1.080e-3, 128: 1.076e-3}


def renderer(precision):
    r = M.make_renderer(load_golden("weights_color"), 16, 16, 1, precision)
    r.sdf_network._own_pack().set_precision(precision)
    return r


_ORACLE = {}


def oracle(seed):
    """pos (V, 3) -> oracle (sdf, grad, albedo) in float64 for the seeded latent."""
    if "sd" not in _ORACLE:
        _ORACLE["sd"] = A.golden_state()
    sd, csd = _ORACLE["sd"]
    w = O.style_mlp(sd, A.latent(seed).double())
    return lambda pos: A.field(sd, csd, w, pos.detach().cpu().double().numpy() if torch.is_tensor(pos) else pos)


def residual_at(seed, m, threshold):
    s, g, _ = oracle(seed)(m.positions)
    return np.abs(s + threshold) / np.linalg.norm(g, axis=-1)


def _surface_case(precision, R, seed, threshold):
    from oi_amd import mesh
    r = renderer(precision)
    z = A.latent(seed).cuda()
    m2 = mesh.extract_intrinsic_mesh(r, z=z, resolution=R, threshold=threshold, refine=2)
    m0 = mesh.extract_intrinsic_mesh(r, z=z, resolution=R, threshold=threshold, refine=0)
    ok = (m2.flags == 0).cpu().numpy()
    r2, r0 = residual_at(seed, m2, threshold), residual_at(seed, m0, threshold)
    case = f"mesh_on_surface[{precision},R={R},seed={seed},thr={threshold}]"
    stats = {"median_refine0": float(np.median(r0)), "median_refine2": float(np.median(r2[ok])), "worst_refine2": float(r2[ok].max()),
             "worst_refine0": float(r0.max())}
    for k, v in stats.items():
        record_margin(case, k, v)
    print(case, stats, "V", len(ok), "flagged", int((~ok).sum()))
    assert m2.residual.shape == (3, len(ok)) and m0.residual.shape == (1, len(ok))
    return stats, int((~ok).sum()), len(ok)


@pytest.mark.parametrize("seed,threshold", [(0, 0.0), (1, 0.0), (2, 0.0), (0, 0.05)])
@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_on_the_surface(precision, R, seed, threshold):
    """Oracle |sdf + threshold| / |grad| at the returned positions: inside the sdf parity bar for every unflagged vertex after
    two steps, and its median strictly below that of the marching-cubes vertices (refine = 0)."""
    stats, flagged, V = _surface_case(precision, R, seed, threshold)
    assert V > 2000
    assert flagged == 0                                   # the rehearsal's count
    assert stats["worst_refine2"] < SDF_BAR, stats
    assert stats["median_refine2"] < stats["median_refine0"], stats


@pytest.mark.parametrize("R", [64, 128])
def test_on_the_surface_bf16(R):
    """bf16 (one bf16 MFMA per contraction): measured, recorded, bar = 3 x the measured worst as every bf16 row of DESIGN
    section 5.  Measured on one MI355X (seeds 0, 1, 2; oracle residual at the returned positions):
        R = 64    median 2.8e-4 .. 3.9e-4 at refine = 0 -> 1.3e-4 .. 2.0e-4 at refine = 2, worst 1.080e-3, no vertex flagged
        R = 128   median 1.4e-4 .. 1.7e-4 at refine = 0 -> 1.2e-4 .. 2.0e-4 at refine = 2, worst 1.076e-3, no vertex flagged
    The steps converge onto the bf16 field's own zero set, which lies about 2e-4 from the oracle's: at 128^3 that is as far as
    the marching-cubes vertices already are, so in this mode the refinement does not lower the median there (seed 0: 1.35e-4
    -> 2.05e-4).  No median condition is asserted for bf16, only the bar on the worst vertex and zero flags."""
    worst = 0.0
    for seed in (0, 1, 2):
        stats, flagged, _ = _surface_case("bf16", R, seed, 0.0)
        worst = max(worst, stats["worst_refine2"])
        assert flagged == 0
    print("bf16 worst residual after two steps", R, worst)
    assert worst < 3 * BF16_MEASURED_WORST[R], worst


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_attributes_are_the_fields(precision, seed):
    from oi_amd import mesh
    r = renderer(precision)
    z = A.latent(seed).cuda()
    m = mesh.extract_intrinsic_mesh(r, z=z, resolution=64, refine=2)
    s, g, c = oracle(seed)(m.positions)
    gmax, gmin = float(np.abs(g).max()), float(np.linalg.norm(g, axis=-1).min())
    nbar = SDF_BAR * gmax / gmin
    print(f"largest gradient entry {gmax:.4f}, smallest |grad| {gmin:.4f}: bar on the unit normals {nbar:.3e}")
    case = f"mesh_attributes[{precision},seed={seed}]"
    n_err = float(np.abs(m.normals.cpu().numpy() - A.unit(g)).max())
    a_err = float(np.abs(m.albedo.cpu().numpy() - c).max())
    record_margin(case, "normals", n_err)
    record_margin(case, "albedo", a_err)
    print(case, "normals", n_err, "albedo", a_err)
    assert n_err < nbar and a_err < RGB_BAR
    assert float((m.normals.norm(dim=-1) - 1).abs().max()) < 1e-6
    # the residual rows are the field's own: the last one against the oracle at the final positions (sdf bar / smallest |grad|)
    assert float(np.abs(m.residual[-1].cpu().numpy() - np.abs(s) / np.linalg.norm(g, axis=-1)).max()) < 2 * SDF_BAR / gmin
    # the drop-in modules' un-fused call pattern on the same points
    net, col = r.sdf_network, r.color_network
    with torch.no_grad():
        pts = m.positions.clone()
        w = net.style(z)
        gr = net.gradient(pts, z=z, w=w)
        feat = net(pts, z=z, w=w)[:, 1:]
        rgb = col(pts, gr, None, feat, w=w)
    g_err = float(np.abs(gr.cpu().numpy() - g).max())
    record_margin(case, "unfused_gradient", g_err)
    assert g_err < SDF_BAR * gmax
    assert float(np.abs(A.unit(gr.cpu().double().numpy()) - m.normals.cpu().numpy()).max()) < nbar
    u_err = float(np.abs(rgb.cpu().numpy() - c).max())
    record_margin(case, "unfused_albedo", u_err)
    assert u_err < RGB_BAR and float((rgb - m.albedo).abs().max()) < RGB_BAR


@pytest.mark.parametrize("res,bmin,bmax", [(64, BMIN, BMAX), ((33, 64, 17), (-1.1, -0.7, -0.9), (0.95, 1.2, 0.6))])
def test_refine_zero_returns_the_marching_cubes_vertices(res, bmin, bmax):
    from oi_amd import mesh
    r = renderer("f16x3")
    z = A.latent(0).cuda()
    u = mesh.sdf_lattice(r.pack, bmin, bmax, res, z=z, scale=-1.0)[0]
    vi, tris = mesh.marching_cubes(u, 0.0)
    m = mesh.vertex_attributes(r.pack, vi, bmin, bmax, res, z=z, refine=0)
    assert len(vi) > 500
    assert m.residual.shape == (1, len(vi)) and m.flags.dtype == torch.uint8 and not bool(m.flags.any())
    rs = np.array((res,) * 3 if np.isscalar(res) else res, dtype=np.float64)
    ref = vi.cpu().double().numpy() / (rs - 1.0)[None] * (np.array(bmax) - np.array(bmin))[None] + np.array(bmin)[None]
    if np.isscalar(res):
        assert np.array_equal(ref, mesh.to_world(vi.cpu().double().numpy(), np.array(bmin), np.array(bmax), res))
    # fp32 rounding of the bounds: torch.linspace's axis value (step, product, sum: 1.5 ulp), the index-space i + t (0.5 ulp
    # of the span), the edge difference and the fused interpolation (1 ulp) -- 3 ulp of the largest magnitude on the axis,
    # taken as 4
    span = np.maximum(np.array(bmax) - np.array(bmin), np.maximum(np.abs(bmin), np.abs(bmax)))
    err = np.abs(m.positions.cpu().double().numpy() - ref)
    print("refine=0 position error / ulp(span)", (err.max(0) / (span * 2.0 ** -23)))
    assert (err <= 4 * span[None] * 2.0 ** -23).all()
    # a vertex on a lattice plane is that plane's axis value, bit for bit
    ax = [torch.linspace(bmin[a], bmax[a], int(rs[a]), device="cuda") for a in range(3)]
    for a in range(3):
        on = vi[:, a] == vi[:, a].floor()
        assert torch.equal(m.positions[on, a], ax[a][vi[on, a].long()])


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("R,threshold", [(64, 0.0), (128, 0.0), (64, 0.05)])
def test_safeguards_limit_and_winding(precision, R, threshold):
    """No flagged vertex (the rehearsal's count), no vertex further than half a cell per axis from its marching-cubes
    position, every face above 1 % of the median area wound with its vertex normals, triangles those of marching_cubes."""
    from oi_amd import mesh
    r = renderer(precision)
    for seed in (0, 1, 2):
        z = A.latent(seed).cuda()
        m2 = mesh.extract_intrinsic_mesh(r, z=z, resolution=R, threshold=threshold, refine=2)
        m0 = mesh.extract_intrinsic_mesh(r, z=z, resolution=R, threshold=threshold, refine=0)
        assert int((m2.flags != 0).sum()) == 0 and int((m0.flags != 0).sum()) == 0
        half = np.float32(0.5 * 2.0 / (R - 1))
        shift = (m2.positions - m0.positions).abs().cpu().numpy()
        assert (shift <= half * (1 + 2.0 ** -22)).all(), shift.max() / half   # the kernel's own fp32 comparison, 2 ulp
        u = mesh.sdf_lattice(r.pack, BMIN, BMAX, R, z=z, scale=-1.0)[0]
        _, tris = mesh.marching_cubes(u, threshold)
        assert m2.triangles.dtype == torch.int32 and torch.equal(m2.triangles, tris) and torch.equal(m0.triangles, tris)
        for m in (m2, m0):
            judged, bad = A.winding_disagreements(m.positions.cpu().numpy(), tris.cpu().numpy(), m.normals.cpu().numpy())
            assert judged > 0.95 * len(tris) and bad == 0, (seed, judged, bad)


def _guarded_pass(V, seed):
    """The four entries through the C ABI on guarded buffers, against the float64 restatement."""
    from oi_amd import lib, ops
    L = lib.load()
    rs = np.random.RandomState(seed)
    n = (9, 7, 5)
    ax = [torch.linspace(-1.0, 1.0 + 0.1 * a, n[a]) for a in range(3)]
    vi = np.stack([rs.randint(0, n[a], V) for a in range(3)], -1).astype(np.float32)
    axis = rs.randint(0, 3, V)
    t = rs.rand(V).astype(np.float32)
    for a in range(3):
        on = (axis == a) & (vi[:, a] < n[a] - 1)
        vi[on, a] += t[on]
    if V >= 1:
        vi[0] = [n[0] - 1, n[1] - 1, n[2] - 1]      # the last lattice point: t = 0 on the last plane of every axis
    vi_g = guarded_copy(torch.from_numpy(vi).cuda(), "verts_index")
    ax_g = [guarded_copy(a.cuda(), f"axis{i}") for i, a in enumerate(ax)]
    pos = guarded_empty((V, 3), what="pos")
    flags = guarded_empty((V,), torch.uint8, what="flags")
    p = lambda t_: ctypes.c_void_p(t_.data_ptr())
    st = ops._stream()
    assert L.oi_mesh_vertex_world(p(vi_g), V, p(ax_g[0]), p(ax_g[1]), p(ax_g[2]), *n, p(pos), p(flags), st) == 0
    ax64 = [a.double().numpy() for a in ax]
    ref0 = A.vertex_world(vi, ax64)
    assert np.abs(pos.cpu().double().numpy() - ref0).max() <= 2 * 2.0 ** -23 * 1.2
    assert np.array_equal(pos[0].cpu().numpy(), np.array([a[-1].item() for a in ax], dtype=np.float32))
    assert not bool(flags.any())
    # a Newton step with every kind of vertex: ordinary, zero gradient, NaN sdf, inf gradient, a step past the limit
    pos0 = guarded_copy(pos, "pos0")
    s = (0.02 * rs.randn(V)).astype(np.float32)
    g = rs.randn(V, 3).astype(np.float32)
    kind = np.arange(V) % 5
    g[kind == 1] = 0.0
    s[kind == 2] = np.nan
    g[kind == 3, 1] = np.inf
    s[kind == 4] = 5.0
    lim = A.half_cell(ax64).astype(np.float32)
    s_g, g_g = guarded_copy(torch.from_numpy(s).cuda(), "sdf"), guarded_copy(torch.from_numpy(g).cuda(), "grad")
    res = guarded_empty((V,), what="residual")
    thr = 0.01
    assert L.oi_mesh_newton(p(pos), p(pos0), p(s_g), p(g_g), V, thr, float(lim[0]), float(lim[1]), float(lim[2]), p(res),
                            p(flags), st) == 0
    p0 = pos0.cpu().double().numpy()
    q, rres, rflags = A.newton_step(p0, p0, s.astype(np.float64) + np.float64(np.float32(thr)), g.astype(np.float64),
                                    lim.astype(np.float64))
    got_f = flags.cpu().numpy()
    sure = np.abs(np.abs(q - p0) - lim[None]).min(-1) > 1e-5       # not within rounding of the limit
    assert np.array_equal(got_f[sure | (rflags != A.FLAG_LIMIT) & (rflags != 0)], rflags[sure | (rflags != A.FLAG_LIMIT) & (rflags != 0)])
    if V >= 5:
        assert set(np.unique(got_f)) == {0, A.FLAG_NONFINITE, A.FLAG_SMALL_GRADIENT, A.FLAG_LIMIT}
    moved = got_f == 0
    got_p = pos.cpu().numpy()
    assert np.array_equal(got_p[~moved], pos0.cpu().numpy()[~moved])          # a flagged vertex keeps its position
    assert np.abs(got_p[moved] - q[moved]).max(initial=0.0) < 1e-6
    fin = np.isfinite(rres)
    assert np.allclose(res.cpu().numpy()[fin], rres[fin], rtol=1e-5, atol=0) and np.isinf(res.cpu().numpy()[kind == 1]).all()
    # finalize with the record, and the record alone
    c = (rs.rand(V, 3) * 1.4 - 0.2).astype(np.float32)
    g2 = rs.randn(V, 3).astype(np.float32)
    s2 = (1e-3 * rs.randn(V)).astype(np.float32)
    c_g, g2_g, s2_g = (guarded_copy(torch.from_numpy(a).cuda(), w_) for a, w_ in ((c, "rgb"), (g2, "grad2"), (s2, "sdf2")))
    normals, albedo, res2 = guarded_empty((V, 3), what="normals"), guarded_empty((V, 3), what="albedo"), guarded_empty((V,), what="residual2")
    record = guarded_empty((V, 27), torch.uint8, what="record", must_write=False)    # compared byte for byte below
    assert L.oi_mesh_attr_finalize(p(pos), p(s2_g), p(g2_g), p(c_g), V, thr, p(normals), p(albedo), p(res2), p(record), st) == 0
    assert np.abs(normals.cpu().numpy() - A.unit(g2.astype(np.float64))).max(initial=0.0) < 1e-6
    assert np.array_equal(albedo.cpu().numpy(), c)
    assert np.allclose(res2.cpu().numpy(), np.abs(s2.astype(np.float64) + np.float32(thr)) / np.linalg.norm(g2.astype(np.float64), axis=-1), rtol=1e-5)
    exp = np.empty(V, dtype=A.RECORD_DTYPE)
    exp["p"], exp["n"] = got_p, normals.cpu().numpy()
    exp["c"] = np.rint(np.clip(c, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(record.cpu().numpy().reshape(-1), exp.view(np.uint8).reshape(-1))
    record2 = guarded_empty((V, 27), torch.uint8, what="record2", must_write=False)
    assert L.oi_mesh_vertex_record(p(pos), p(normals), p(c_g), V, p(record2), st) == 0
    assert torch.equal(record2, record)
    return pos, flags


@pytest.mark.parametrize("V", [1, 37, 1000, 4097])
def test_guarded_shapes(V):
    """V = 1000 and 4097 are no multiples of the MLP's 128-point tile (nor of the 256 vertices of a workgroup here)."""
    from oi_amd import mesh
    _guarded_pass(V, seed=V)
    # the whole chain, MLP passes included, on the first V vertices of a real mesh: every output a guarded arena view
    r = renderer("f16x3")
    z = A.latent(0).cuda()
    u = mesh.sdf_lattice(r.pack, BMIN, BMAX, 64, z=z, scale=-1.0)[0]
    vi, _ = mesh.marching_cubes(u, 0.0)
    sub = guarded_copy(vi[:V], "verts_index")
    a = mesh.vertex_attributes(r.pack, sub, BMIN, BMAX, 64, z=z, refine=2, want_record=True)
    b = mesh.vertex_attributes(r.pack, sub, BMIN, BMAX, 64, z=z, refine=2, want_record=True)
    assert a.positions.shape == (V, 3) and a.residual.shape == (3, V) and a.record.shape == (V, 27) and a.flags.shape == (V,)
    for k in ("positions", "normals", "albedo", "residual", "flags", "record"):       # identical launches: identical bytes
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(x.view(torch.uint8) if x.dtype != torch.uint8 else x, y.view(torch.uint8) if y.dtype != torch.uint8 else y), k
    assert float(a.residual[-1].max()) < SDF_BAR


def test_no_crossing_gives_empty_arrays():
    from oi_amd import mesh
    r = renderer("f16x3")
    z = A.latent(0).cuda()
    m = mesh.extract_intrinsic_mesh(r, z=z, resolution=24, threshold=50.0, refine=2, want_record=True)   # u = -sdf never reaches 50
    assert tuple(m.positions.shape) == (0, 3) and tuple(m.normals.shape) == (0, 3) and tuple(m.albedo.shape) == (0, 3)
    assert tuple(m.residual.shape) == (3, 0) and tuple(m.flags.shape) == (0,) and tuple(m.triangles.shape) == (0, 3)
    assert tuple(m.record.shape) == (0, 27)
    v, t, n, c = r.extract_intrinsic_geometry(torch.tensor(BMIN), torch.tensor(BMAX), 24, threshold=50.0, z=z)
    assert v.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3) and c.shape == (0, 3)


def test_newton_entry_flags_a_zero_gradient_and_keeps_the_position():
    """The guard exercised through its inputs: g = 0 handed to the Newton entry."""
    from oi_amd import ops, lib
    V = 70
    pos = torch.randn(V, 3, device="cuda")
    pos0, keep = pos.clone(), pos.clone()
    flags = torch.zeros(V, dtype=torch.uint8, device="cuda")
    res = ops._new(pos, V)
    ops.mesh_newton(pos, pos0, torch.full((V,), 0.01, device="cuda"), torch.zeros(V, 3, device="cuda"), 0.0, (0.1, 0.1, 0.1), res, flags)
    assert torch.equal(pos, keep) and bool((flags == lib.MESH_FLAG_SMALL_GRADIENT).all()) and bool(torch.isinf(res).all())
    # sticky: an ordinary step afterwards moves the vertex and keeps the bit
    g = torch.zeros(V, 3, device="cuda")
    g[:, 0] = 1.0
    ops.mesh_newton(pos, pos0, torch.full((V,), 0.01, device="cuda"), g, 0.0, (0.1, 0.1, 0.1), res, flags)
    assert bool((flags == lib.MESH_FLAG_SMALL_GRADIENT).all()) and float((pos[:, 0] - (keep[:, 0] - 0.01)).abs().max()) < 1e-6


def test_renderer_extract_intrinsic_geometry():
    from oi_amd import mesh
    r = renderer("f16x3")
    z = A.latent(1).cuda()
    bmin, bmax = torch.tensor(BMIN), torch.tensor(BMAX)
    v, t, n, c = r.extract_intrinsic_geometry(bmin, bmax, 64, threshold=0.0, z=z)
    v0, t0 = r.extract_geometry(bmin, bmax, 64, threshold=0.0, z=z)
    assert v.dtype == np.float64 and t.dtype == np.int64 and n.dtype == np.float32 and c.dtype == np.float32
    assert np.array_equal(t, t0) and v.shape == v0.shape == n.shape == c.shape
    assert np.abs(v - v0).max() <= 0.5 * 2.0 / 63 * (1 + 1e-6)
    m = mesh.extract_intrinsic_mesh(r, z=z, resolution=64)
    assert np.array_equal(v, m.positions.cpu().numpy().astype(np.float64)) and np.array_equal(n, m.normals.cpu().numpy())


def make_gen(precision="f16x3"):
    g = load_golden("f5_generator")
    gen = M.build_generator(16, 16, 16, 1, precision).eval()
    gen.color_network.load_state_dict(sub_sd(g, "color."))
    gen.light.load_state_dict(sub_sd(g, "light."))
    with torch.no_grad():
        gen.light.param_specular.fill_(0.35)
        gen.light.param_shininess.fill_(6.0)
    return gen, g["z"]


def _ply_arrays(path):
    v, t, props = A.read_ply(path)
    assert props == [("x", "float"), ("y", "float"), ("z", "float"), ("nx", "float"), ("ny", "float"), ("nz", "float"),
                     ("red", "uchar"), ("green", "uchar"), ("blue", "uchar")]
    return (np.stack([v["x"], v["y"], v["z"]], -1), np.stack([v["nx"], v["ny"], v["nz"]], -1),
            np.stack([v["red"], v["green"], v["blue"]], -1), t)


def test_export_mesh(tmp_path):
    from oi_amd import inference
    from oi_amd.relight import Light, stack_lights
    gen, z = make_gen()
    path = str(tmp_path / "rose.ply")
    m = inference.export_mesh(gen, z[0], path, resolution=64, refine=2)
    pos, nrm, col, tris = _ply_arrays(path)
    V = len(pos)
    assert V == len(m.positions) > 2000 and np.array_equal(tris, m.triangles.cpu().numpy())
    assert np.array_equal(pos, m.positions.cpu().numpy()) and np.array_equal(nrm, m.normals.cpu().numpy())
    alb = m.albedo.cpu().numpy()
    assert np.array_equal(col, np.rint(np.clip(alb, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8))
    assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=-1) - 1).max() < 1e-6
    assert int((m.flags != 0).sum()) == 0
    # with the trained light: the fp64 restatement of the shading (tests/helpers/relight_ref.py), view along the normal
    light = Light.from_module(gen.light)
    lit = str(tmp_path / "rose_lit.ply")
    ml = inference.export_mesh(gen, z[0], lit, resolution=64, refine=2, light=light)
    assert torch.equal(ml.positions, m.positions) and torch.equal(ml.albedo, m.albedo)
    n64 = ml.normals.double()
    ref = relight_ref(torch.ones(V, 1).cuda(), n64.view(V, 1, 3), ml.albedo.view(V, 1, 3), torch.ones(V, 1).cuda(),
                    ml.positions.double() + n64, -n64, torch.eye(4)[None].cuda(), stack_lights(light), None, 1)
    err = float((ml.shaded.double() - ref["image_no_bg"][0, 0].t()).abs().max())
    record_margin("mesh_export_shaded", "vertex_colour", err)
    print("shaded vertex colours vs fp64", err)
    assert err < 2e-6
    assert float((ml.shaded - ml.albedo).abs().max()) > 1e-2      # the light did something
    _, nrm_l, col_l, _ = _ply_arrays(lit)
    sh = ml.shaded.cpu().numpy()
    assert np.array_equal(col_l, np.rint(np.clip(sh, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8))
    assert np.array_equal(nrm_l, nrm)
    # a caller-supplied eye
    eye = (0.0, 0.0, -3.0)
    sv = inference.shade_vertices(ml.positions, ml.normals, ml.albedo, light, eye=eye)
    e = torch.tensor(eye, dtype=torch.float64).cuda().expand(V, 3)
    d = ml.positions.double() - e
    ref = relight_ref(torch.ones(V, 1).cuda(), n64.view(V, 1, 3), ml.albedo.view(V, 1, 3), d.norm(dim=-1, keepdim=True), e,
                      d / d.norm(dim=-1, keepdim=True), torch.eye(4)[None].cuda(), stack_lights(light), None, 1)
    assert float((sv.double() - ref["image_no_bg"][0, 0].t()).abs().max()) < 2e-6


def test_export_mesh_refuses_a_nan_weight_before_any_launch(tmp_path):
    from oi_amd import inference, lib
    gen, z = make_gen()
    with torch.no_grad():
        gen.renderer.sdf_network.pts_linears[3].weight[5, 7] = float("nan")
    path = tmp_path / "bad.ply"
    with pytest.raises(lib.OiHipError, match="oi_mlp_pack_status"):
        inference.export_mesh(gen, z[0], str(path), resolution=32)
    assert not path.exists()
