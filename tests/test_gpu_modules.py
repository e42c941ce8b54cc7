"""GPU parity of the drop-in modules (oi_amd.renderer / generator / fields) against the golden
vectors produced by the reference itself (F1, F4, F5) and against the oracle on larger inputs."""
import os

import numpy as np
import pytest
import torch

import oi_oracle as O
from conftest import GOLDEN, load_golden, maxdiff, sub_sd, record_margin
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]
NET_KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
SDF_NPZ = os.path.join(GOLDEN, "weights_sdf.npz")


def make_renderer(col_sd, S, I, K, precision="f32", variance=0.3):
    from oi_amd.fields import ShapeNetwork, ColorNetwork, SingleVarianceNetwork
    from oi_amd.renderer import NeuSRenderer
    sdf = ShapeNetwork(checkpoint_path=SDF_NPZ, **NET_KW).cuda()
    col = ColorNetwork(**NET_KW)
    col.load_state_dict(col_sd)
    col = col.cuda()
    dev = SingleVarianceNetwork(variance).cuda()
    return NeuSRenderer(None, sdf, dev, col, n_samples=S, n_importance=I, n_outside=0, up_sample_steps=K, perturb=0,
                        precision=precision)


def test_state_dict_keys_match_reference(sdf_sd, col_sd):
    from oi_amd.fields import ShapeNetwork, ColorNetwork
    assert set(ShapeNetwork(None, **NET_KW).state_dict().keys()) == set(sdf_sd.keys())
    assert set(ColorNetwork(**NET_KW).state_dict().keys()) == set(col_sd.keys())
    for k, v in ShapeNetwork(None, **NET_KW).state_dict().items():
        assert v.shape == sdf_sd[k].shape, k


def test_shape_network_api(col_sd):
    g = load_golden("f1_film_siren")
    r = make_renderer(col_sd, 16, 16, 1)
    net = r.sdf_network
    with torch.no_grad():
        w = net.style(g["z"].cuda())
        assert maxdiff(w.cpu(), g["w"]) < 1e-5
        out = net(g["pts"].cuda(), z=g["z"].cuda(), w=w)
        assert out.shape == (1024, 129)
        assert maxdiff(out[:, :1].cpu(), g["sdf"]) < 2e-5 and maxdiff(out[:, 1:].cpu(), g["feat"]) < 1e-4
        assert maxdiff(net.sdf(g["pts"].cuda(), z=g["z"].cuda(), w=w).cpu(), g["sdf"]) < 2e-5
        gr = net.gradient(g["pts"].cuda(), z=g["z"].cuda(), w=w)
        assert maxdiff(gr.cpu(), g["grad"]) < 1e-4 * float(g["grad"].abs().max())


def test_s_val_is_a_reported_value_and_the_variance_gradient_comes_from_compositing(col_sd):
    """Stated deviation (renderer._inv_s): the reference's `s_val` entry carries a graph to the variance parameter
    (renderer.py:404) that no loss of the path uses; ours is a detached, cached report.  The variance gradient itself is
    owned by the compositing kernel and arrives through every differentiable output."""
    g = load_golden("f4_render")
    r = make_renderer(col_sd, 16, 16, 1, "f16x3")
    r.deviation_network.variance.requires_grad_(True)
    out = r.render(g["rays_o"].cuda(), g["rays_d"].cuda(), g["near"].cuda(), g["far"].cuda(), perturb_overwrite=0,
                   cos_anneal_ratio=0.5, z=None, w=g["w"].cuda())
    assert not out["s_val"].requires_grad and out["s_val"].grad_fn is None
    assert abs(float(out["s_val"][0, 0]) - float(torch.exp(torch.tensor(-3.0)))) < 1e-6   # 1 / exp(10 * 0.3)
    (out["color_fine"].sum() + out["weight_sum"].sum()).backward()
    gv = r.deviation_network.variance.grad
    assert gv is not None and bool(torch.isfinite(gv).all()) and float(gv.abs().sum()) > 0


KEYS = ("s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights", "gradient_error", "inside_sphere",
        "mid_z_vals", "surface_loss", "sdf", "pts_norm", "pts", "color_fine", "raw_color")


# f32 = the 1e-4 parity path of the north star.  bf16x3 (hi/lo split operands on the bf16 matrix cores) carries
# ~2^-16 relative error per product; amplified by the gamma~30 FiLM phases it reaches 3e-4 (relative) on
# d sdf/dx and stays within 2e-4 on every other renderer output -- stated here and in DESIGN.md.
# bf16x6 (3-way bf16 split, the 6 products of weight >= 2^-24) and f16x3 (2-way fp16 split of power-of-two scaled
# operands, 3 products, 2^-22 per product): fp32-class contractions -> the same 1e-4 bar as f32.
@pytest.mark.parametrize("precision,tol", [("f32", 1e-4), ("bf16x6", 1e-4), ("f16x3", 1e-4), ("bf16x3", 2e-4)])
@pytest.mark.parametrize("tag,car", [("c0p0", 0.0), ("c0p5", 0.5), ("c1p0", 1.0)])
def test_render_golden_f4(col_sd, tag, car, precision, tol):
    """NeuSRenderer.render on identical rays / weights: every key of the returned dict within 1e-4."""
    g = load_golden("f4_render")
    r = make_renderer(col_sd, 16, 16, 1, precision)
    with torch.no_grad():
        out = r.render(g["rays_o"].cuda(), g["rays_d"].cuda(), g["near"].cuda(), g["far"].cuda(), perturb_overwrite=0,
                       cos_anneal_ratio=car, z=None, w=g["w"].cuda())
    for k in KEYS:
        ref = g[f"{tag}_{k}"]
        assert tuple(out[k].shape) == tuple(ref.shape), (k, out[k].shape, ref.shape)
        scale = max(1.0, float(ref.abs().max())) if k == "gradients" else 1.0
        if precision == "bf16x3" and k == "gradients":
            scale *= 2.5
        assert maxdiff(out[k].cpu(), ref) < tol * scale, (k, maxdiff(out[k].cpu(), ref))


# ---- bf16 operand mode (BASELINE.json configs[1] names it): ONE bf16 MFMA per product, unreduced v_sin / v_cos.
# Tolerances are on the MAPS (per-ray outputs) and are measurements: `record_margin` collects the error of every key,
# tools/grad_margin.py prints them (profiles/r4_bf16_margins.txt), each tolerance is ~3x the worst measured error.
# Per-SAMPLE outputs are not compared: the coarse pass runs in bf16 too, importance sampling is discontinuous in the sdf
# (searchsorted bins), so individual samples move -- the integrals over the ray do not.
# measured (MI355X, profiles/r4_bf16_margins.txt): color_fine 6.7e-4, weight_sum 1.3e-3, weight_max 1.2e-2 (a single sample's
# weight: not an integral over the ray), s_val exact
BF16_RAY_TOL = {"color_fine": 2.5e-3, "weight_sum": 5e-3, "weight_max": 4e-2, "s_val": 1e-6}


@pytest.mark.parametrize("tag,car", [("c0p0", 0.0), ("c0p5", 0.5), ("c1p0", 1.0)])
def test_render_golden_f4_bf16_maps(col_sd, tag, car):
    """NeuSRenderer.render in precision="bf16" against the reference's own F4 outputs: every per-ray key."""
    g = load_golden("f4_render")
    r = make_renderer(col_sd, 16, 16, 1, "bf16")
    with torch.no_grad():
        out = r.render(g["rays_o"].cuda(), g["rays_d"].cuda(), g["near"].cuda(), g["far"].cuda(), perturb_overwrite=0,
                       cos_anneal_ratio=car, z=None, w=g["w"].cuda())
    for k, tol in BF16_RAY_TOL.items():
        ref = g[f"{tag}_{k}"]
        assert tuple(out[k].shape) == tuple(ref.shape), (k, out[k].shape, ref.shape)
        assert bool(torch.isfinite(out[k]).all()), k
        err = maxdiff(out[k].cpu(), ref)
        record_margin("render_f4_bf16_mode_vs_reference", k, err)
        assert err < tol, (k, err)
    # mean absolute error of the colour: the worst ray is a silhouette ray, the image as a whole is far closer
    mae = float((out["color_fine"].cpu() - g[f"{tag}_color_fine"]).abs().mean())
    record_margin("render_f4_bf16_mode_vs_reference", "color_fine(mean)", mae)
    assert mae < 4e-4, mae   # measured 1.0e-4


# worst pixel, measured: image 1.4e-3, mask 1.8e-3, normal_map 6.8e-3 (unnormalised gradient, |.| up to ~16), shading 1.4e-3,
# z_map 2.3e-2 (depth in scene units at a silhouette pixel), colour 9.8e-4, specular 1.3e-3; every mean 15x or more below
BF16_MAP_TOL = {"image": 5e-3, "mask": 6e-3, "weight_sum_map": 6e-3, "normal_map": 2.5e-2, "shading_map": 5e-3, "z_map": 7e-2,
                "color_map": 4e-3, "image_no_bg": 5e-3, "diff_shading_map": 5e-3, "specular_map": 5e-3,
                "no_specular_map": 3e-3, "amb_shading_map": 2e-3, "z_min": 1e-5}


def test_generator_golden_f5_bf16_maps():
    """Generator.forward in precision="bf16" vs the reference's own F5 maps (worst pixel and mean absolute error)."""
    g = load_golden("f5_generator")
    gen = build_generator(16, 16, 16, 1, "bf16").eval()
    gen.color_network.load_state_dict(sub_sd(g, "color."))
    gen.light.load_state_dict(sub_sd(g, "light."))
    gen.it.fill_(int(g["it"]))
    np.random.seed(12)
    with torch.no_grad():
        blob = gen(bs=2, it=None, data={"z": g["z"].cuda(), "b2w": g["b2w"].cuda()}, return_raw=True)["box"]
    assert maxdiff(blob["rays_info"]["rays_o"].cpu(), g["rays_o"]) < 1e-5   # (not MLP outputs: exact as in every mode)
    for k, v in blob["render_out"].items():
        ref = g["map_" + k]
        assert tuple(v.shape) == tuple(ref.shape) and bool(torch.isfinite(v).all()), k
        err, mae = maxdiff(v.cpu(), ref), float((v.cpu() - ref).abs().mean())
        record_margin("generator_f5_bf16_mode_vs_reference", k, err)
        record_margin("generator_f5_bf16_mode_vs_reference", k + "(mean)", mae)
        assert err < BF16_MAP_TOL.get(k, 5e-3), (k, err)
        assert mae < 0.15 * BF16_MAP_TOL.get(k, 5e-3), (k, mae)
    err = abs(float(blob["loss"]["eikonal"]) - float(g["eikonal"]))
    record_margin("generator_f5_bf16_mode_vs_reference", "eikonal", err)
    assert err < 6e-4, err   # measured 1.7e-4


@pytest.mark.parametrize("K,I", [(1, 64), (4, 64), (2, 32)])
def test_render_vs_oracle_hierarchical(sdf_sd, col_sd, K, I):
    """More rays, 2 elements, K up-sampling steps, vs the oracle."""
    S = 64
    g = torch.Generator().manual_seed(K)
    N = 2 * 150
    ro = torch.tensor([0.0, 0.0, -3.0]).expand(N, 3) + 0.05 * torch.randn(N, 3, generator=g)
    rd = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(N, 3, generator=g), dim=-1)
    near, far = O.near_far_from_sphere(ro, rd)
    w = O.style_mlp(sdf_sd, torch.randn(2, 64, generator=g))
    ref = O.render(sdf_sd, col_sd, torch.tensor(0.3), ro, rd, near, far, w, S, I, K, 0.25)
    r = make_renderer(col_sd, S, I, K)
    with torch.no_grad():
        out = r.render(ro.cuda(), rd.cuda(), near.cuda(), far.cuda(), perturb_overwrite=0, cos_anneal_ratio=0.25,
                       w=w.cuda())
    # Importance sampling is discontinuous in its inputs (searchsorted bins, the `den < 1e-5` and
    # `radius < 1` switches, inv_s up to 512): fp32 round-off differences between two correct
    # implementations move a few samples of a few rays by more than 1e-4.  Per-stage exactness on
    # identical inputs is pinned in test_gpu_kernels.py::test_upsample_*; here: >= 97 % of the rays agree
    # sample-for-sample, and those rays agree in everything downstream.
    dz = (out["mid_z_vals"].cpu() - ref["mid_z_vals"]).abs().max(-1).values
    ok = dz < 1e-4
    assert ok.float().mean() >= 0.97, float(ok.float().mean())
    # alpha = f(sdf * inv_s) with inv_s doubling per up-sampling step (64 * 2^(K-1) in the last one): an fp32-level
    # sdf difference of ~2e-6 between two correct MLP evaluations moves a weight by ~ inv_s * 2e-6 * 0.25, i.e.
    # ~6e-5 at K <= 2 and ~2.6e-4 at K = 4 -- the bound scales with K accordingly.
    tol = 2e-4 if K <= 2 else 4e-4
    for k in ("weights", "color_fine", "weight_sum", "sdf", "raw_color"):
        assert maxdiff(out[k].cpu()[ok], ref[k][ok]) < tol, (k, maxdiff(out[k].cpu()[ok], ref[k][ok]))
    assert abs(float(out["color_fine"].cpu().mean()) - float(ref["color_fine"].mean())) < 1e-4


def example_cfg(R):
    fov, img, img_scene = 10.0, 256, 1588
    cam_dist = float(1 / np.tan(0.5 * fov * np.pi / 180))
    scene_fov = float(2 * np.arctan(img_scene / img * np.tan(0.5 * fov * np.pi / 180)) * 180 / np.pi)
    return cam_dist, scene_fov, int(R * img_scene / img)


def build_generator(R, S, I, K, precision="f32"):
    """Built from a config whose __target__ strings are the REFERENCE's (configs/train.yaml): the
    oi_amd config seam redirects them."""
    from oi_amd.config import build_from_config
    cam_dist, scene_fov, scene_res = example_cfg(R)
    net = lambda t, **kw: {"__target__": t, "kwargs": kw}
    cfg = net("src.models.generator.Generator",
              color_network=net("src.models.fields.ColorNetwork", **NET_KW),
              sdf_network=net("src.models.fields.ShapeNetwork", checkpoint_path=SDF_NPZ, **NET_KW),
              deviation_network=net("src.third_party.neus.models.fields.SingleVarianceNetwork", init_val=0.3),
              light_network=net("src.utils.prior.build_directional_light_optimizable", cam_loc=None, light_loc=None,
                                ambient_color=0.33, diffuse_color=0.66, specular_color=0, shininess=10),
              camera=net("src.models.camera_network.Camera", cam_dist=cam_dist, resolution=scene_res, fov=scene_fov),
              z_dim=64, resolution=R, scene_resolution=scene_res,
              renderer=net("src.third_party.neus.models.renderer.NeuSRenderer", n_importance=I, n_outside=0,
                           n_samples=S, perturb=1, up_sample_steps=K),
              anneal_end=50000,
              pose_prior=net("src.utils.pose_sampler.Plane", cam_loc=[0, -1, 0], rot_degree_range_scale=360,
                             rot_roll_degree_range_scale=20, xy_range_scale=[6, 3.5]))
    gen = build_from_config(cfg)
    gen.renderer.pack.set_precision(precision)
    return gen.cuda()


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
def test_generator_golden_f5(precision):
    """Full Generator.forward(return_raw=True) vs the reference's own output (rays, maps, stats)."""
    g = load_golden("f5_generator")
    gen = build_generator(16, 16, 16, 1, precision).eval()
    gen.color_network.load_state_dict(sub_sd(g, "color."))
    gen.light.load_state_dict(sub_sd(g, "light."))
    gen.it.fill_(int(g["it"]))
    np.random.seed(12)  # the background colour is the first numpy draw of the forward (prior.py:15)
    with torch.no_grad():
        blob = gen(bs=2, it=None, data={"z": g["z"].cuda(), "b2w": g["b2w"].cuda()}, return_raw=True)["box"]
    assert maxdiff(blob["rays_info"]["rays_o"].cpu(), g["rays_o"]) < 1e-5
    assert maxdiff(blob["rays_info"]["rays_d"].cpu(), g["rays_d"]) < 2e-6
    assert maxdiff(blob["prior_info"]["c2b"].cpu(), g["c2b"]) < 1e-5
    assert maxdiff(blob["latent_info"]["w"].cpu(), g["w"]) < 1e-5
    for k, v in blob["render_out"].items():
        ref = g["map_" + k]
        assert tuple(v.shape) == tuple(ref.shape), (k, v.shape, ref.shape)
        assert maxdiff(v.cpu(), ref) < 1e-4, (k, maxdiff(v.cpu(), ref))
    for k in ("weights", "mid_z_vals", "weight_sum", "color_fine", "sdf"):
        assert maxdiff(blob["raw_render_out"][k].cpu(), g["raw_" + k]) < 1e-4, k
    assert maxdiff(blob["loss"]["eikonal"].cpu(), g["eikonal"]) < 1e-4
    for k in ("surface", "s_val", "cdf", "weight_max", "weight_sum"):
        assert abs(float(blob["stats"][k]) - float(g["stat_" + k])) < 1e-4, k
    for k in ("light/ambient", "light/diffuse", "light/specular", "material/shininess"):
        assert abs(float(blob["stats"][k]) - float(g["stat_" + k.replace("/", "_")])) < 1e-5, k
    # STATED DEVIATION, pinned: the reference returns these four (and nothing else of `stats`) as Python floats through
    # .item() -- four host syncs per forward (generator.py:219-222); here every stat is a detached 0-dim DEVICE tensor, like
    # the reference's own loss entries of the same dict (gan_pose_trainer.py:126-139 mixes both), and float(x) at logging
    # time is the caller's sync.  Same values, same keys; with a gradient recorded they still carry no graph.
    gen.train()
    blob_t = gen(bs=2, it=None, data={})["box"]   # (training mode samples its own poses, as the reference's does: generator.py:178)
    for st in (blob["stats"], blob_t["stats"]):
        for k in ("light/ambient", "light/diffuse", "light/specular", "material/shininess", "s_val", "cdf", "weight_max", "weight_sum"):
            v = st[k]
            assert isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 and not v.requires_grad, (k, type(v))
            assert isinstance(float(v), float) and f"{float(v):.4f}"
    gen.eval()


@pytest.mark.parametrize("bs,train", [(1, True), (2, True), (2, False)])
def test_generator_fused_prep_launch_matches_the_separate_launches(monkeypatch, bs, train):
    """No-grad forward with host-sampled poses: pose upload + rays + light direction + style MLP / FiLM parameters + coarse
    samples in ONE launch (oi_prep_render, pose block by value) against the copy + oi_gen_rays_light + oi_film_params +
    oi_coarse_samples chain: same numpy / torch draws, every map, statistic and pose tensor bit for bit."""
    import oi_amd.generator as G
    gen = build_generator(16, 16, 16, 1, "f16x3")
    gen = gen.train() if train else gen.eval()

    monkeypatch.setattr(G, "ONE_DRAW", False)   # (the two generator calls of the separate chain; the one-launch draw of round 6 has
    #                                              its own test: test_step_tail_blob_in_prep_bit_identical_and_one_draw_jitter)

    def run(fused):
        monkeypatch.setattr(G, "PREP_MAX_B", 8 if fused else 0)
        np.random.seed(5)
        torch.manual_seed(5)
        with torch.no_grad():
            return gen(bs=bs, it=3, data={}, return_raw=True)["box"]

    a, b = run(True), run(False)
    assert a["render_out"]["image"].is_contiguous()
    for k in a["render_out"]:
        assert torch.equal(a["render_out"][k], b["render_out"][k]), k
    for k in ("c2b", "b2w", "w2b"):
        assert torch.equal(a["prior_info"][k], b["prior_info"][k]), k
    for k in ("rays_o", "rays_d", "near", "far", "light_dir", "x_offset", "y_offset"):
        assert torch.equal(a["rays_info"][k], b["rays_info"][k]), k
    assert torch.equal(a["latent_info"]["w"], b["latent_info"]["w"]) and torch.equal(a["latent_info"]["z"], b["latent_info"]["z"])
    for k in ("weights", "mid_z_vals", "sdf", "gradients"):
        assert torch.equal(a["raw_render_out"][k], b["raw_render_out"][k]), k
    for k, v in a["stats"].items():
        assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["stats"][k])), k
    assert torch.equal(a["loss"]["eikonal"], b["loss"]["eikonal"])


def test_generator_multi_chunk_matches_single(monkeypatch):
    """Eval-time ray chunking (generator.py:281-305) does not change the image."""
    import oi_amd.generator as G
    gen = build_generator(16, 8, 8, 1).eval()
    g = load_golden("f5_generator")
    data = {"z": g["z"].cuda(), "b2w": g["b2w"].cuda()}
    np.random.seed(1)
    with torch.no_grad():
        a = gen(bs=2, it=0, data=dict(data))["box"]["render_out"]
        monkeypatch.setattr(G, "MAX_RAY_BATCH_SIZE", 2 * 100)
        np.random.seed(1)
        b = gen(bs=2, it=0, data=dict(data))["box"]["render_out"]
    for k in a:
        assert maxdiff(a[k], b[k]) < 1e-6, k


@pytest.mark.parametrize("pct", [0.1, 0.5, 0.9])
def test_augment_pipe_golden_f8(pct):
    """AugmentPipe(xint=1, scale=1) with the reference's deterministic debug_percentile hook."""
    from oi_amd.augment import AugmentPipe
    g = load_golden("f8_augment")
    aug = AugmentPipe(xint=1, scale=1).cuda()
    assert maxdiff(aug.Hz_geom.cpu(), g["Hz_geom"]) < 1e-7
    tag = str(pct).replace(".", "p")
    with torch.no_grad():
        for key in ("32", "64"):
            y = aug(g["x" + key].cuda(), debug_percentile=pct)
            ref = g[f"y{key}_{tag}"]
            assert tuple(y.shape) == tuple(ref.shape)
            assert maxdiff(y.cpu(), ref) < 2e-5, (key, maxdiff(y.cpu(), ref))


@pytest.mark.parametrize("tag,res,nf,cin,cout", [("r16c3_", 16, 32, 3, 7), ("r64c3_", 64, 64, 3, 7), ("r64c1_", 64, 32, 1, 1)])
def test_dc_discriminator_module_golden_f7(tag, res, nf, cin, cout):
    from oi_amd.discriminator import DCDiscriminator
    g = load_golden("f7_discriminator")
    D = DCDiscriminator(in_dim=cin, out_dim=cout, n_feat=nf, img_size=res)
    D.load_state_dict(sub_sd(g, tag + "w."))
    D = D.cuda()
    with torch.no_grad():
        d = D(g[tag + "x"].cuda(), it=3)
    assert maxdiff(d.cpu(), g[tag + "d"]) < 2e-5


def test_ada_discriminator_view_shapes():
    from oi_amd.config import build_from_config
    cfg = {"__target__": "src.models.discriminator.ADADiscriminatorView",
           "kwargs": dict(aug={"__target__": "src.third_party.ada.augment.AugmentPipe", "kwargs": {"scale": 1, "xint": 1}},
                          aug_p=1, img_size=64, in_dim=3, last_bias=False, n_feat=512, out_dim=7, out_dim_latent=0,
                          out_dim_position=6)}
    D = build_from_config(cfg).cuda()
    assert sum(p.numel() for p in D.parameters()) == 2812928
    with torch.no_grad():
        out = D(torch.rand(3, 3, 64, 64, device="cuda"), it=0)
    assert out.shape == (3, 7) and torch.isfinite(out).all()
    assert D.get_resolution() == 64


def test_inference_walks_and_depth_multiplier():
    """Inference driver: camera / latent walk frames at 2x resolution and 2x depth, multi-chunk."""
    from oi_amd import inference
    g = load_golden("f5_generator")
    gen = build_generator(32, 16, 16, 1).eval()   # "test_resolution 32, depth x2" of a 16^2 / 8+8 training config
    z0, z1 = g["z"][0], g["z"][1]
    np.random.seed(0)
    fr = inference.camera_walk(gen, z0, g["b2w"][0], n_frames=3, max_ray_batch=300)
    assert fr["image"].shape == (3, 3, 32, 32) and torch.isfinite(fr["image"]).all()
    assert float((fr["image"][0] - fr["image"][1]).abs().max()) > 1e-3        # the view changes
    np.random.seed(0)
    one = inference.camera_walk(gen, z0, g["b2w"][0], n_frames=1)
    assert maxdiff(one["mask"][0], fr["mask"][0]) < 1e-6                        # chunking does not change a frame
    lw = inference.latent_walk(gen, z0, z1, g["b2w"][0], n_frames=3)
    assert float((lw["normal_map"][0] - lw["normal_map"][2]).abs().max()) > 1e-3
    # hipGraph replay of the same walk (multi-chunk too): masks / normals do not depend on the random background
    gw = inference.camera_walk(gen, z0, g["b2w"][0], n_frames=3, max_ray_batch=300, graphed=True)
    assert torch.equal(gw["mask"], fr["mask"]) and torch.equal(gw["normal_map"], fr["normal_map"])
    kw = {"renderer": {"kwargs": {"n_importance": 4, "n_samples": 16}}, "resolution": 128, "scene_resolution": 794,
          "camera": {"kwargs": {"resolution": 794}}}
    kw2 = inference.scale_config(kw, 128, test_resolution=256, depth_multiplier=16)
    assert kw2["renderer"]["kwargs"] == {"n_importance": 64, "n_samples": 256} and kw2["resolution"] == 256
    assert kw2["scene_resolution"] == 1588 and kw["resolution"] == 128


# ---------------------------------------------------------------- fused optimiser / EMA steps
def _param_set(seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(128, 3), (128,), (7, 128, 128), (512, 256, 4, 4), (1,), (5000,)]
    return [torch.randn(s, generator=g).cuda().requires_grad_() for s in shapes]


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_fused_optimizer_matches_torch(kind):
    """Five steps of the configs/train.yaml optimisers: FusedAdam(lr 2e-5, betas (0, 0.9)) / FusedRMSprop(lr 1e-4)
    vs torch.optim on identical gradients; state_dict layouts interchange."""
    from oi_amd.optim import FusedAdam, FusedRMSprop
    pa, pb = _param_set(0), _param_set(0)
    if kind == "adam":
        oa, ob = FusedAdam(pa, lr=2e-5, betas=(0.0, 0.9)), torch.optim.Adam(pb, lr=2e-5, betas=(0.0, 0.9))
    else:
        oa, ob = FusedRMSprop(pa, lr=1e-4), torch.optim.RMSprop(pb, lr=1e-4)
    g = torch.Generator().manual_seed(1)
    for it in range(5):
        for x, y in zip(pa, pb):
            gr = torch.randn(x.shape, generator=g).cuda() * (10.0 ** (it - 2))
            x.grad, y.grad = gr.clone(), gr.clone()
        if it == 2:
            pa[4].grad = pb[4].grad = None  # a parameter without gradient is skipped
        oa.step()
        ob.step()
    for x, y in zip(pa, pb):
        assert maxdiff(x, y) <= 2e-7 * max(1.0, float(y.abs().max())), (x.shape, maxdiff(x, y))
    sa, sb = oa.state_dict(), ob.state_dict()
    for k in sb["state"]:
        assert set(sa["state"][k]) == set(sb["state"][k])
        for name, v in sb["state"][k].items():
            assert maxdiff(sa["state"][k][name].float().cpu(), v.float().cpu()) <= 1e-6 * max(1.0, float(v.abs().max())), name
    # a torch optimiser checkpoint loads into the fused one (and keeps stepping)
    oa.load_state_dict(sb)
    oa.step()


def test_fused_adam_deepcopy_and_pickle_keep_the_step_counts():
    """The step counts live in Python ints between observations (optim._StepCounts): copy.deepcopy / pickle must see them
    -- a copy that restarted Adam's bias correction at step 1 with warm moments would take a different third step."""
    import copy, pickle
    from oi_amd.optim import FusedAdam
    pa, pb = _param_set(2), _param_set(2)
    oa, ob = FusedAdam(pa, lr=1e-3, betas=(0.5, 0.9)), torch.optim.Adam(pb, lr=1e-3, betas=(0.5, 0.9))
    g = torch.Generator().manual_seed(4)
    grads = [[torch.randn(x.shape, generator=g).cuda() for x in pa] for _ in range(3)]
    for it in range(2):
        for x, y, gr in zip(pa, pb, grads[it]):
            x.grad, y.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
    oc = copy.deepcopy(oa)
    od = pickle.loads(pickle.dumps(oa))
    for o in (oc, od):
        steps = {float(st["step"]) for st in o.state.values()}
        assert steps == {2.0}, steps
    for y, gr in zip(pb, grads[2]):
        y.grad = gr.clone()
    ob.step()
    for o in (oc, od):
        ps = [p for grp in o.param_groups for p in grp["params"]]
        for x, gr in zip(ps, grads[2]):
            x.grad = gr.clone()
        o.step()
        for x, y in zip(ps, pb):
            assert maxdiff(x, y) <= 2e-7 * max(1.0, float(y.abs().max())), (x.shape, maxdiff(x, y))


def test_ema_update_matches_reference_rule():
    """p_ema <- p.lerp(p_ema, beta), buffers copied (src/utils/ema.py:26-32): one oi_multi_lerp launch."""
    from oi_amd.ema import EMA
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.BatchNorm1d(30), torch.nn.Linear(30, 7)).cuda()
    ema = EMA(m, 0.9)
    before = [p.clone() for p in ema.module.parameters()]
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn_like(p))
        m[1].running_mean.add_(1.5)
    ema.update(0)
    for pe, b, p in zip(ema.module.parameters(), before, m.parameters()):
        assert maxdiff(pe, p.detach().lerp(b, 0.9)) <= 2e-7 * max(1.0, float(p.abs().max()))
    assert maxdiff(ema.module[1].running_mean, m[1].running_mean) == 0.0


def test_fused_step_invalidates_packed_weight_images():
    """The fused optimiser / EMA kernels write parameters through raw pointers; the MFMA weight images
    (fields.FieldPack) are cached on Tensor._version, so the writes must be counted like in-place torch ops --
    otherwise every render after the first optimiser step would still use the initial weights."""
    from oi_amd.ema import EMA
    from oi_amd.optim import FusedAdam
    gen = build_generator(8, 8, 8, 1, "f16x3").eval()
    data = {"z": torch.randn(1, 64, device="cuda"), "b2w": torch.eye(4, device="cuda")[None],
            "bg_color": torch.zeros(1, 3, device="cuda")}
    render = lambda g: g(bs=1, it=0, data=dict(data))["box"]["render_out"]["image"].clone()
    with torch.no_grad():
        before = render(gen)
    ema = EMA(gen, 0.5)
    with torch.no_grad():
        assert maxdiff(render(ema.module), before) == 0.0
    params = list(gen.parameters())
    v0 = [p._version for p in params]
    opt = FusedAdam(params, lr=1e-2, betas=(0.0, 0.9))
    g = torch.Generator().manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).cuda()
    opt.step()
    assert all(p._version > v for p, v in zip(params, v0))
    with torch.no_grad():
        cached = render(gen)                  # through the version-keyed cache
        gen.renderer.pack.invalidate()
        fresh = render(gen)                   # images rebuilt from scratch
    assert maxdiff(cached, fresh) == 0.0
    assert maxdiff(cached, before) > 1e-3     # lr 1e-2 sign steps move every weight: the image must change
    ema.update(0)
    with torch.no_grad():
        e_cached = render(ema.module)
        ema.module.renderer.pack.invalidate()
        e_fresh = render(ema.module)
    assert maxdiff(e_cached, e_fresh) == 0.0
    assert maxdiff(e_cached, before) > 1e-4


def test_forward_glue_fast_paths_match_tensor_paths():
    """The no-grad forward folds scalar glue into existing launches / version-keyed caches: light direction from the
    ray kernel, cached light + variance scalars, host-side iteration counter.  Each must equal the tensor path."""
    gen = build_generator(8, 8, 8, 1, "f16x3").eval()
    with torch.no_grad():
        gen.light.param_direction.copy_(torch.tensor([0.3, -0.8, 0.5]))
    prior = gen.sample_prior(3, {})
    rays = gen.gen_rays_at({}, prior, with_light=True)
    assert maxdiff(rays["light_dir"], prior["light"].direction()) < 1e-6
    ref = gen.gen_rays_at({}, prior)
    for k in ("rays_o", "rays_d", "near", "far"):
        assert maxdiff(rays[k], ref[k]) == 0.0
    # iteration counter: host-side between observations, the buffer is right whenever it can be observed
    with torch.no_grad():
        blob = gen(bs=1, it=7, data={})["box"]
    assert int(gen.state_dict()["it"]) == 7 and gen.iteration() == 7
    gen.it.fill_(3)                      # external write (what load_state_dict / EMA buffer copies do)
    assert gen.iteration() == 3
    # one-launch render statistics (oi_render_stats) vs the reference's tensor expressions on the raw outputs
    with torch.no_grad():
        blob = gen(bs=2, it=None, data={}, return_raw=True)["box"]
    raw = blob["raw_render_out"]
    for k, ref in (("cdf", raw["cdf_fine"][:, :1].mean()), ("weight_max", raw["weight_max"].mean()),
                   ("weight_sum", raw["weight_sum"].mean())):
        assert abs(float(blob["stats"][k]) - float(ref)) < 1e-6, k
    inside = (raw["pts_norm"] < 1.2).float()
    eik = (inside * (torch.linalg.norm(raw["gradients"], dim=-1) - 1.0) ** 2).sum() / (inside.sum() + 1e-5)
    assert abs(float(blob["loss"]["eikonal"]) - float(eik)) < 1e-5 * max(1.0, float(eik))
    assert abs(float(blob["stats"]["surface"]) - float(torch.exp(-100.0 * raw["sdf"].abs()).mean())) < 1e-6
    # cached scalars follow parameter updates
    for rep in range(2):
        with torch.no_grad():
            blob = gen(bs=1, it=None, data={})["box"]
        v = gen.deviation_network.variance.detach()
        amb = torch.sigmoid(gen.light.param_ambient.detach())
        assert abs(float(blob["stats"]["s_val"]) - float(1.0 / torch.exp(10 * v).clamp(1e-6, 1e6))) < 1e-7
        assert abs(float(blob["stats"]["light/ambient"]) - float(amb)) < 1e-7
        assert abs(float(blob["stats"]["light/diffuse"]) - float(1 - amb)) < 1e-7
        assert abs(float(blob["stats"]["light/specular"]) - max(0.0, float(gen.light.param_specular))) < 1e-7
        with torch.no_grad():
            gen.deviation_network.variance.add_(0.05)
            gen.light.param_ambient.add_(0.3)
            gen.light.param_specular.add_(0.2)


def test_fused_ema_matches_reference_formula():
    from oi_amd.ema import EMA
    net = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Linear(53, 5000)).cuda()
    ema = EMA(net, 0.999)
    ref = [p.detach().clone() for p in net.parameters()]
    for it in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn_like(p))
        ema.update(it)
        ref = [p.detach().lerp(r, 0.999) for p, r in zip(net.parameters(), ref)]  # ema.py:29
    for a, b in zip(ema.module.parameters(), ref):
        assert maxdiff(a, b) <= 1e-6


def test_host_pose_algebra_matches_device_path():
    """Training-mode forward computes w2b / c2b / crop offsets on the host (fp32 numpy) and ships one buffer; the
    eval path (poses given on the device) runs the reference's tensor arithmetic: identical within fp32 round-off."""
    gen = build_generator(16, 8, 8, 1)
    gen.train()
    np.random.seed(3)
    prior_h = gen.sample_prior(3, {})
    rays_h = gen.gen_rays_at({}, prior_h)
    gen.eval()
    prior_d = gen.sample_prior(3, {"b2w": prior_h["b2w"].clone()})
    rays_d = gen.gen_rays_at({}, prior_d)
    for k in ("b2w", "w2b", "c2b"):
        assert maxdiff(prior_h[k], prior_d[k]) < 1e-5, k
    for k in ("x_offset", "y_offset"):
        assert maxdiff(rays_h[k], rays_d[k]) < 2e-4 * max(1.0, float(rays_d[k].abs().max())), k
    for k in ("rays_o", "rays_d", "near", "far"):
        assert maxdiff(rays_h[k], rays_d[k]) < 1e-5, k
    assert maxdiff(prior_h["light"].direction(), prior_d["light"].direction()) < 1e-6


@pytest.mark.parametrize("N", [1, 33])
def test_render_ragged_ray_counts(sdf_sd, col_sd, N):
    """Ray counts that fill neither a wavefront tile (32 points) nor a workgroup: tail lanes are masked, not dropped."""
    g = torch.Generator().manual_seed(N)
    ro = torch.tensor([0.0, 0.0, -3.0]).expand(N, 3) + 0.05 * torch.randn(N, 3, generator=g)
    rd = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.2 * torch.randn(N, 3, generator=g), dim=-1)
    near, far = O.near_far_from_sphere(ro, rd)
    w = O.style_mlp(sdf_sd, torch.randn(1, 64, generator=g))
    ref = O.render(sdf_sd, col_sd, torch.tensor(0.3), ro, rd, near, far, w, 16, 16, 1, 0.5)
    r = make_renderer(col_sd, 16, 16, 1, "f16x3")
    with torch.no_grad():
        out = r.render(ro.cuda(), rd.cuda(), near.cuda(), far.cuda(), perturb_overwrite=0, cos_anneal_ratio=0.5, w=w.cuda())
    for k in ("weights", "color_fine", "weight_sum", "sdf", "mid_z_vals"):
        assert tuple(out[k].shape) == tuple(ref[k].shape)
        assert maxdiff(out[k].cpu(), ref[k]) < 1e-4, (k, maxdiff(out[k].cpu(), ref[k]))


def test_render_rejects_empty_and_unsplittable_batches(col_sd):
    r = make_renderer(col_sd, 16, 16, 1, "f16x3")
    e = torch.zeros(0, 3).cuda()
    with pytest.raises(ValueError):
        r.render(e, e, torch.zeros(0, 1).cuda(), torch.zeros(0, 1).cuda(), perturb_overwrite=0, w=torch.zeros(1, 64).cuda())
    x = torch.zeros(3, 3).cuda()
    with pytest.raises(ValueError):
        r.render(x, x, torch.zeros(3, 1).cuda(), torch.ones(3, 1).cuda(), perturb_overwrite=0, w=torch.zeros(2, 64).cuda())


def test_graphed_forward_matches_eager():
    """hipGraph replay of the eval forward == the eager forward, frame after frame with new poses / latents."""
    from oi_amd.graphed import GraphedForward
    gen = build_generator(16, 16, 16, 1, "f16x3")
    gen.eval()
    np.random.seed(5)
    gf = GraphedForward(gen, bs=1, it=1000, return_raw=True).recapture()
    g = torch.Generator().manual_seed(0)
    for frame in range(3):
        b2w = torch.tensor(np.asarray(gen.pose_prior(1), dtype=np.float32)).cuda()
        z = torch.randn(1, 64, generator=g).cuda()
        bg = torch.rand(1, 3, generator=g).cuda()
        out = {k: v.clone() for k, v in gf(b2w, z, bg).items()}
        with torch.no_grad():
            ref = gen(bs=1, it=1000, data={"b2w": b2w, "z": z, "bg_color": bg}, return_raw=True)["box"]["render_out"]
        for k in ("image", "mask", "normal_map", "shading_map", "z_map"):
            assert torch.equal(out[k], ref[k]), (frame, k, maxdiff(out[k], ref[k]))


# ------------------------------------------------------------------ round-2 fixtures (oracle/gen_golden_r2.py)
@pytest.mark.parametrize("S", [16, 32])
def test_k4_sampling_stage_by_stage_golden_f10(col_sd, S):
    """up_sample_steps = 4 against the reference's own intermediates: every stage is fed the REFERENCE's previous
    z / sdf, so a discontinuous bin switch cannot hide a difference -- 100 % of the rays within 1e-4 at every stage,
    then every key of render() on the reference's final samples within 1e-4 (renderer.py:137-197, 400-413)."""
    from oi_amd import ops
    from oi_amd.autograd import sdf_mlp
    g = load_golden("f10_render_k4")
    t = f"s{S}_"
    r = make_renderer(col_sd, S, S, 4, "f16x3")
    ro, rd = g["rays_o"].cuda(), g["rays_d"].cuda()
    w = g["w"].cuda()
    _, gamma, beta = r.pack.film(w=w)
    N = ro.shape[0]
    with torch.no_grad():
        for i in range(4):
            zb, sb = g[f"{t}z_before{i}"].cuda(), g[f"{t}sdf_before{i}"].cuda()
            last = i == 3
            z_new, pts_new, z_m = ops.upsample(ro, rd, zb, sb, S // 4, 64.0 * 2 ** i, merge=last)
            assert maxdiff(z_new.cpu(), g[f"{t}z_new{i}"]) < 1e-4, (i, maxdiff(z_new.cpu(), g[f"{t}z_new{i}"]))
            if last:
                assert maxdiff(z_m.cpu(), g[f"{t}z_after{i}"]) < 1e-4
            else:  # merge the REFERENCE's new samples (with this implementation's sdf at them)
                zn = g[f"{t}z_new{i}"].cuda()
                p = (ro[:, None, :] + rd[:, None, :] * zn[..., None]).reshape(-1, 3)
                sdf_new = sdf_mlp(r.pack, p, gamma, beta, 1, False, False, False)[0].view(N, -1)
                zo, so = ops.merge_sorted(zb, sb, zn, sdf_new)
                assert maxdiff(zo.cpu(), g[f"{t}z_after{i}"]) == 0.0
                assert maxdiff(so.cpu(), g[f"{t}sdf_after{i}"]) < 2e-5
        z_fin = g[f"{t}z_after3"].cuda()
        r.sample_z = lambda *a, **k: (z_fin, None) if k.get("with_mid") else z_fin   # the final stage on the reference's own samples
        out = r.render(ro, rd, g["near"].cuda(), g["far"].cuda(), perturb_overwrite=0,
                       cos_anneal_ratio=float(g["cos_anneal_ratio"]), w=w)
    for k in KEYS:
        ref = g[f"{t}render_{k}"]
        scale = max(1.0, float(ref.abs().max())) if k == "gradients" else 1.0
        assert maxdiff(out[k].cpu(), ref) < 1e-4 * scale, (k, maxdiff(out[k].cpu(), ref))


@pytest.mark.parametrize("graphed", [False, True])
def test_inference_frame_golden_f11(graphed):
    """One frame of the inference driver against the reference: Generator.forward(return_raw=True) in eval mode with given
    z / b2w at 32 x 32, 16+16 samples (depth x2 of an 8+8 config), rendered in four ray chunks
    (scripts/test.py:274-281, src/utils/test.py:131-155, generator.py:286-305)."""
    from oi_amd import inference
    g = load_golden("f11_inference")
    gen = build_generator(32, 16, 16, 1, "f16x3").eval()
    gen.color_network.load_state_dict(sub_sd(g, "color."))
    gen.light.load_state_dict(sub_sd(g, "light."))
    gen.it.fill_(int(g["it"]))
    keys = ("image", "mask", "normal_map", "shading_map")
    np.random.seed(22)  # the background colour is the first numpy draw of the forward (prior.py:15)
    fr = inference.render_frames(gen, [g["z"][0]], [g["b2w"][0]], keys=keys, max_ray_batch=int(g["max_ray_batch"]),
                                 graphed=graphed)
    for k in keys:
        if graphed and k == "image":
            continue  # the captured graph composites over a fixed black background
        ref = g["map_" + k][0]
        assert tuple(fr[k][0].shape) == tuple(ref.shape), (k, fr[k][0].shape, ref.shape)
        assert maxdiff(fr[k][0].cpu(), ref) < 1e-4, (k, maxdiff(fr[k][0].cpu(), ref))


def test_graphed_discriminator_forward_matches_eager():
    """oi_amd.graphed.GraphedDForward: the no-grad ADA-discriminator forward replayed from a hipGraph (static padding
    margins, augmentation parameters drawn on the host in the eager order) against the eager forward from the same
    numpy state, over several replays with different inputs."""
    from oi_amd.config import build_from_config
    from oi_amd.graphed import GraphedDForward
    net = lambda t, **kw: {"__target__": t, "kwargs": kw}
    torch.manual_seed(3)
    disc = build_from_config(net("src.models.discriminator.ADADiscriminatorView",
                                 aug=net("src.third_party.ada.augment.AugmentPipe", scale=1, xint=1), aug_p=1, img_size=32,
                                 in_dim=3, last_bias=False, n_feat=64, out_dim=7, out_dim_latent=0, out_dim_position=6)).cuda().eval()
    gd = GraphedDForward(disc)
    g = torch.Generator().manual_seed(5)
    for i in range(4):
        x = torch.rand(2, 3, 32, 32, generator=g).cuda()
        np.random.seed(100 + i)
        with torch.no_grad():
            want = disc(x, it=0).clone()
        np.random.seed(100 + i)
        got = gd(x).clone()
        assert maxdiff(got, want) < 2e-4 * max(1.0, float(want.abs().max())), (i, maxdiff(got, want))


@pytest.mark.parametrize("B,with_aug,launch", [(1, True, "graph"), (3, True, "graph"), (2, False, "graph"), (1, True, "eager"),
                                               (4, False, "eager")])
def test_library_graph_discriminator_forward_bit_identical(B, with_aug, launch, monkeypatch):
    """oi_disc_graph_*: the batch <= 4 forward of the 64 x 64 network as a hipGraph owned by the library; the image pointer and
    the augmentation matrices are kernel-node parameters updated per launch.  Against the five eager launches
    (oi_disc_fwd_small, static margins) from the same numpy state: bit-identical, over calls with different images AT
    DIFFERENT ADDRESSES and different draws; GraphedDForward takes this path for such shapes."""
    from oi_amd.config import build_from_config
    from oi_amd.graphed import GraphedDForward
    from oi_amd import ops
    net = lambda t, **kw: {"__target__": t, "kwargs": kw}
    torch.manual_seed(4)
    cfg = dict(img_size=64, in_dim=3, last_bias=True, n_feat=512, out_dim=7)
    if with_aug:
        disc = build_from_config(net("src.models.discriminator.ADADiscriminatorView", out_dim_latent=0, out_dim_position=6,
                                     aug=net("src.third_party.ada.augment.AugmentPipe", scale=1, xint=1), aug_p=1, **cfg)).cuda().eval()
    else:
        disc = build_from_config(net("src.models.discriminator.DCDiscriminator", **cfg)).cuda().eval()
    monkeypatch.setenv("OI_DISC_LAUNCH", launch)   # "graph": hipGraph replay with updated node parameters | "eager": launch by launch
    gd = GraphedDForward(disc)
    g = torch.Generator().manual_seed(6)
    keep = []
    for i in range(4):
        x = torch.rand(B, 3, 64, 64, generator=g).cuda()
        keep.append(x)   # (keeps every image alive: each call sees a new pointer)
        np.random.seed(200 + i)
        with torch.no_grad():
            if with_aug:
                th = disc.aug.theta_fast(B, 64, 64)   # (one seed from numpy's stream -> the library's draws: what gd(x) does)
                want = disc._forward_small(x, f12=disc.aug.Hz_geom, theta_np=th, margins=disc.aug.static_margins(64, 64)).clone()
            else:
                want = disc(x).clone()
        np.random.seed(200 + i)
        got = gd(x).clone()
        assert gd._lib is not None and isinstance(gd._lib, ops.DiscGraph) and gd._lib.eager == (launch == "eager")
        assert torch.equal(got, want), (i, maxdiff(got, want))
    assert len({t.data_ptr() for t in keep}) == 4
    # the module's own forward keeps its plans outside its attributes: a discriminator that has run still deep-copies
    import copy
    with torch.no_grad():
        disc(keep[0])
        twin = copy.deepcopy(disc)
        np.random.seed(5); a = disc(keep[1]).clone()
        np.random.seed(5); b = twin(keep[1]).clone()
    assert torch.equal(a, b)


@pytest.mark.parametrize("launch", ["graph", "eager"])
def test_library_graph_takes_the_canvas_form_when_the_footprint_does_not_fit(launch):
    """ops.DiscGraph holds two captured variants with the augmentation: canvas built inside the first kernel (footprint fits its
    LDS tile) and canvas from memory (it does not: e.g. a zoom-out by 2.5).  The choice is made per launch from the matrices;
    both give what oi_disc_fwd_small gives with the matrices in device memory (always the canvas form), bit for bit, also when
    the two kinds of launch alternate."""
    from oi_amd import ops
    D = _ada_disc(3, 7).cuda().eval()
    H = W = 64
    m = D.aug.static_margins(H, W)
    plan = ops.DiscGraph((2, 3, H, W), torch.device("cuda"), [l.weight for l in D.blocks], D.conv_out.weight, D.conv_out.bias,
                         f12=D.aug.Hz_geom, margins=m, launch=launch)
    g = torch.Generator().manual_seed(11)
    for i, scales in enumerate([(1.0, 0.4), (0.4, 0.4), (1.1, 0.9), (0.4, 1.0)]):   # per image of the batch
        x = torch.rand(2, 3, H, W, generator=g).cuda()
        Gs = O.ada_G_inv(2, 64, 64, torch.tensor([[0.124, 0.0], [0.0, -0.124]], dtype=torch.float64),
                         torch.tensor(scales, dtype=torch.float64), dtype=torch.float64).numpy().astype(np.float32)
        th = D.aug.theta_for(Gs, m, H, W)
        got = plan(x, th).clone()
        with torch.no_grad():
            want = D._forward_small(x, f12=D.aug.Hz_geom, theta_dev=torch.from_numpy(th).cuda(), margins=m)
        assert torch.equal(got, want), (i, scales, maxdiff(got, want))


def test_stack_cache_equals_torch_stack_forward_and_backward():
    """params.StackCache (one gather launch per parameter version, no launch for the differentiable stack) against
    params.stack_field_params (torch.stack): same values, same per-parameter gradients, refreshed after an optimiser step,
    and a graph that saved the OLD contents refuses to run backward."""
    from oi_amd.optim import FusedAdam
    from oi_amd.params import stack_field_params
    gen = build_generator(8, 8, 8, 1, "f16x3")
    pack = gen.renderer.pack
    sd, csd = pack._sds()
    ref = stack_field_params(sd, csd)
    got = pack.stacked()
    assert set(got) == set(ref)
    for k in ref:
        assert got[k].shape == ref[k].shape and maxdiff(got[k].detach(), ref[k].detach()) == 0.0, k
    # gradients: a random linear functional of every stacked entry
    torch.manual_seed(0)
    cot = {k: torch.randn_like(v) for k, v in ref.items()}
    params = list(sd.values()) + list(csd.values())
    g_ref = torch.autograd.grad(sum((ref[k] * cot[k]).sum() for k in ref), params, allow_unused=True)
    g_got = torch.autograd.grad(sum((got[k] * cot[k]).sum() for k in got), params, allow_unused=True)
    for p, a, b in zip(params, g_got, g_ref):
        assert (a is None) == (b is None)
        if a is not None:
            assert maxdiff(a, b) == 0.0
    # an optimiser step changes the parameters: the next request sees the new values (one gather launch) ...
    stale = pack.stacked()
    opt = FusedAdam(params, lr=1e-2, betas=(0.0, 0.9))
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    with torch.no_grad():
        new = pack.stacked()
        ref2 = stack_field_params(sd, csd)
    for k in ref2:
        assert maxdiff(new[k], ref2[k]) == 0.0 and (k not in ("gw", "wh") or maxdiff(new[k], ref[k].detach()) > 1e-3), k
    # ... and a graph built on the old contents fails loudly instead of differentiating with the new ones
    with pytest.raises(RuntimeError, match="modified (by an )?inplace"):
        (stale["gw"] * stale["gw"]).sum().backward()


def test_light_direction_fused_matches_tensor_path():
    """oi_light_dir_fwd / _bwd against direction -> batch_direction -> F.normalize with autograd (lighting.py:35-39, 115-119)."""
    from oi_amd.lighting import DirectionalLightWithSpecularFixInit
    torch.manual_seed(5)
    light = DirectionalLightWithSpecularFixInit(direction=[0.3, -0.5, 0.8]).cuda()
    B = 5
    w2b = torch.eye(4, device="cuda").repeat(B, 1, 1)
    w2b[:, :3, :3] = torch.linalg.qr(torch.randn(B, 3, 3, device="cuda"))[0] * torch.tensor([1.0, 0.7, 1.3, 1.0, 0.2], device="cuda")[:, None, None]
    cot = torch.randn(B, 3, device="cuda")
    ref = torch.nn.functional.normalize(light.batch_direction(w2b), dim=-1, eps=1e-6)
    (g_ref,) = torch.autograd.grad((ref * cot).sum(), light.param_direction)
    got = light.batch_direction_unit(w2b)
    (g_got,) = torch.autograd.grad((got * cot).sum(), light.param_direction)
    assert maxdiff(got.detach(), ref.detach()) < 3e-7
    assert maxdiff(g_got, g_ref) < 1e-6 * max(1.0, float(g_ref.abs().max()))


# ---------------------------------------------------------------- round 4: the five-launch discriminator forward (batch <= 4)
def _ada_disc(in_dim, out_dim, aug_p=1.0):
    from oi_amd.discriminator import ADADiscriminator
    torch.manual_seed(in_dim * 10 + out_dim)
    return ADADiscriminator(aug={"__target__": "src.third_party.ada.augment.AugmentPipe", "kwargs": {"xint": 1, "scale": 1}},
                            aug_p=aug_p, in_dim=in_dim, out_dim=out_dim, n_feat=512, img_size=64, last_bias=(out_dim == 1))


@pytest.mark.parametrize("B,in_dim,out_dim", [(1, 3, 7), (3, 3, 7), (4, 1, 1)])
def test_small_batch_discriminator_forward_vs_oracle_and_general_path(monkeypatch, B, in_dim, out_dim):
    """csrc/disc_small.hip (ADA geometry + 4 conv blocks + head in five launches, fixed summation order) against the fp64
    oracle (augment.py:284-301 + discriminator.py:57-85) and against the general path of csrc/disc.hip; bit-reproducible."""
    import oi_amd.discriminator as DM
    D = _ada_disc(in_dim, out_dim).cuda().eval()
    dsd = {k: v.detach().cpu().double() for k, v in D.state_dict().items() if "aug." not in k}
    x0 = torch.rand(B, in_dim, 64, 64, generator=torch.Generator().manual_seed(B))
    # (a) no augmentation: the plain network
    with torch.no_grad():
        monkeypatch.setattr(DM, "SMALL_PATH", True)
        d_small = DM.DCDiscriminator.forward(D, x0.cuda())
        d_again = DM.DCDiscriminator.forward(D, x0.cuda())
        monkeypatch.setattr(DM, "SMALL_PATH", False)
        d_gen = DM.DCDiscriminator.forward(D, x0.cuda())
    ref = O.dc_discriminator(dsd, x0.double())
    scale = max(1.0, float(ref.abs().max()))
    assert d_small.shape == (B, out_dim) and torch.equal(d_small, d_again)
    assert maxdiff(d_small.cpu(), ref) < 2e-5 * scale and maxdiff(d_small, d_gen) < 2e-5 * scale
    # (b) with the augmentation: identical numpy draws for both paths (FAST_ADA off: the small plan with host matrices at the
    # static margins | the pipe at margins fitted to the draw + the general chain), and the oracle at a pinned percentile.
    # Measured on an MI355X against the bar of 2e-5 (scale 1: these logits are O(1e-3)): 6.0e-8 / 5.7e-8 / 3.4e-8 at B = 1 / 3 / 4
    monkeypatch.setattr(DM, "FAST_ADA", False)
    with torch.no_grad():
        monkeypatch.setattr(DM, "SMALL_PATH", True)
        np.random.seed(3)
        a_small = D(x0.cuda())
        monkeypatch.setattr(DM, "SMALL_PATH", False)
        np.random.seed(3)
        a_gen = D(x0.cuda())
    monkeypatch.setattr(DM, "FAST_ADA", True)
    print(f"small plan vs pipe + general chain, B={B}: {maxdiff(a_small, a_gen):.3e} (bar {2e-5 * scale:.1e})")
    assert maxdiff(a_small, a_gen) < 2e-5 * scale, maxdiff(a_small, a_gen)
    assert not torch.equal(a_small, a_gen)     # really a second path
    assert maxdiff(a_small, d_small) > 1e-4    # the augmentation did something
    pct = 0.7
    p = torch.tensor(pct, dtype=torch.float64)
    G = O.ada_G_inv(B, 64, 64, ((p * 2 - 1) * 0.125).expand(B, 2), torch.exp2(torch.erfinv(p * 2 - 1) * 0.2).expand(B), dtype=torch.float64)
    ref_a = O.dc_discriminator(dsd, O.ada_geometric(x0.double(), G)[0])
    monkeypatch.setattr(DM, "SMALL_PATH", True)
    orig = D.aug.sample_G_inv
    monkeypatch.setattr(D.aug, "sample_G_inv", lambda im, _pct=None: orig(im, pct))
    with torch.no_grad():
        a_pct = D(x0.cuda())
    assert maxdiff(a_pct.cpu(), ref_a) < 5e-5 * scale, maxdiff(a_pct.cpu(), ref_a)
    # (c) the sampling matrix from device memory (what a captured graph passes): same result as by value
    H = W = 64
    Gi = orig(x0, pct)
    th = torch.from_numpy(D.aug.theta_for(Gi, D.aug.static_margins(H, W), H, W)).cuda()
    with torch.no_grad():
        a_dev = D(x0.cuda(), aug_theta=th)
    assert maxdiff(a_dev.cpu(), ref_a) < 5e-5 * scale
    # (d) canvas built inside the first kernel (matrix by value, footprint fits: 4 launches) == canvas from memory (matrix in
    # device memory: 5 launches), bit for bit, over scales from 0.6 to 1.7 and integer shifts; a scale whose footprint does not
    # fit the LDS tile (0.4) takes the canvas form by itself
    m = D.aug.static_margins(H, W)
    for i, (sc, tx, ty) in enumerate([(1.0, 0.0, 0.0), (0.62, 1.0, -1.0), (1.7, -1.0, 0.0), (0.85, 0.0, 1.0), (0.4, 1.0, 1.0)]):
        Gs = O.ada_G_inv(B, 64, 64, torch.tensor([[tx * 0.124, ty * 0.124]], dtype=torch.float64).expand(B, 2),
                         torch.full((B,), sc, dtype=torch.float64), dtype=torch.float64).numpy().astype(np.float32)
        th_np = D.aug.theta_for(Gs, m, H, W)
        with torch.no_grad():
            by_value = D._forward_small(x0.cuda(), f12=D.aug.Hz_geom, theta_np=th_np, margins=m)
            from_mem = D._forward_small(x0.cuda(), f12=D.aug.Hz_geom, theta_dev=torch.from_numpy(th_np).cuda(), margins=m)
        assert torch.equal(by_value, from_mem), (i, sc, maxdiff(by_value, from_mem))


@pytest.mark.parametrize("B,in_dim,out_dim,view", [(16, 3, 7, True), (64, 3, 7, True), (24, 1, 1, False)])
def test_large_batch_discriminator_forward_vs_oracle(B, in_dim, out_dim, view):
    """Batch >= 16 without gradient (csrc/disc_large.hip: NHWC fp16 limb planes, packed weight images, fixed-order split-K) for the
    64 x 64 / n_feat 512 network: (a) the fp64 oracle on a subset of the images, with and without ADA at a pinned percentile;
    (b) the general chain it replaces; (c) bit-reproducible; (d) follows a weight update (the pack is keyed by parameter
    versions); (e) a network the kernels do not cover keeps the general chain."""
    import oi_amd.discriminator as DM
    from oi_amd.config import build_from_config
    torch.manual_seed(B)
    aug = {"__target__": "src.third_party.ada.augment.AugmentPipe", "kwargs": {"scale": 1, "xint": 1}}
    common = dict(aug=aug, aug_p=1, in_dim=in_dim, out_dim=out_dim, n_feat=512, img_size=64, last_bias=False)
    cfg = ({"__target__": "src.models.discriminator.ADADiscriminatorView", "kwargs": dict(out_dim_position=6, out_dim_latent=0, **common)}
           if view else {"__target__": "src.models.discriminator.ADADiscriminator", "kwargs": common})
    D = build_from_config(cfg).cuda().eval()
    with torch.no_grad():   # variance-preserving weights: O(1) logits (the default initialisation gives 1e-3)
        for p_ in D.parameters():
            fan_in = p_[0].numel()
            p_.copy_((torch.rand_like(p_) * 2 - 1) * (6.0 / (1.04 * fan_in)) ** 0.5)
    x = torch.rand(B, in_dim, 64, 64, device="cuda")
    dsd = {k: v.detach().double().cpu() for k, v in D.state_dict().items() if "aug." not in k}
    sub = [0, B // 2, B - 1]
    with torch.no_grad():
        # ---- no augmentation: DCDiscriminator.forward
        plain = DM.DCDiscriminator.forward(D, x)
        ref = O.dc_discriminator(dsd, x[sub].double().cpu())
        assert float(ref.abs().max()) > 0.05
        assert maxdiff(plain[sub].cpu(), ref) < 2e-5, maxdiff(plain[sub].cpu(), ref)
        DM.LARGE_PATH = False
        try:
            general = DM.DCDiscriminator.forward(D, x)
        finally:
            DM.LARGE_PATH = True
        assert maxdiff(plain, general) < 2e-5 and not torch.equal(plain, general)   # (another summation order: really another path)
        assert torch.equal(plain, DM.DCDiscriminator.forward(D, x))
        # ---- with ADA at a pinned percentile
        pct = 0.7
        orig = D.aug.forward
        D.aug.forward = lambda im: orig(im, debug_percentile=pct)
        d = D(x)
        p = torch.tensor(pct)
        G = O.ada_G_inv(3, 64, 64, ((p * 2 - 1) * 0.125).expand(3, 2), torch.exp2(torch.erfinv(p * 2 - 1) * 0.2).expand(3)).double()
        refa = O.dc_discriminator(dsd, O.ada_geometric(x[sub].double().cpu(), G)[0])
        assert maxdiff(d[sub].cpu(), refa) < 2e-5, maxdiff(d[sub].cpu(), refa)
        del D.aug.forward
        # ---- a weight update is picked up
        D.blocks[2].weight.mul_(0.5)
        dsd2 = {k: v.detach().double().cpu() for k, v in D.state_dict().items() if "aug." not in k}
        assert maxdiff(DM.DCDiscriminator.forward(D, x)[sub].cpu(), O.dc_discriminator(dsd2, x[sub].double().cpu())) < 2e-5
        # ---- not covered (n_feat 64: 8 -> 16 -> 32 -> 64 channels): the general chain answers
        D2 = build_from_config({"__target__": "src.models.discriminator.ADADiscriminator",
                                "kwargs": dict(common, n_feat=64, in_dim=in_dim, out_dim=1)}).cuda().eval()
        d2 = DM.DCDiscriminator.forward(D2, x)
        dsd3 = {k: v.detach().double().cpu() for k, v in D2.state_dict().items() if "aug." not in k}
        assert maxdiff(d2[sub].cpu(), O.dc_discriminator(dsd3, x[sub].double().cpu())) < 2e-5


def test_graphed_large_batch_discriminator_follows_weight_updates():
    """GraphedDForward at batch 16 (a captured hipGraph, not the library plan): the captured forward must read the LIVE
    parameters -- csrc/disc_large.hip's packed weight images are eager allocations keyed on parameter versions and are therefore
    never recorded into a capture (advisor, round 5: a replay after an optimiser step read the stale pack, and the next eager
    forward freed it under the graph).  Replay, change a weight in place, replay, run an eager batch-16 forward (which rebuilds the
    pack), replay again: each replay equals the eager answer for the weights of that moment."""
    import oi_amd.discriminator as DM
    from oi_amd.config import build_from_config
    from oi_amd.graphed import GraphedDForward
    torch.manual_seed(11)
    aug = {"__target__": "src.third_party.ada.augment.AugmentPipe", "kwargs": {}}   # (no geometric branch: the chain alone)
    D = build_from_config({"__target__": "src.models.discriminator.ADADiscriminator",
                           "kwargs": dict(aug=aug, aug_p=1, in_dim=3, out_dim=1, n_feat=512, img_size=64, last_bias=False)}).cuda().eval()
    with torch.no_grad():
        for p_ in D.parameters():
            p_.copy_((torch.rand_like(p_) * 2 - 1) * (6.0 / (1.04 * p_[0].numel())) ** 0.5)
    x = torch.rand(16, 3, 64, 64, device="cuda")
    gd = GraphedDForward(D)

    def eager_general():
        DM.LARGE_PATH = False
        try:
            with torch.no_grad():
                return DM.DCDiscriminator.forward(D, x).clone()
        finally:
            DM.LARGE_PATH = True

    TOL = 2e-5   # (the bar of test_large_batch_discriminator_forward_vs_oracle; the weight updates below move the logits by > 1e-3)
    got0 = gd(x).clone()
    assert gd._lib is None and gd.graph is not None
    assert maxdiff(got0, eager_general()) < TOL        # the capture holds the general chain (split-K atomics: not bit-stable)
    with torch.no_grad():
        D.blocks[1].weight.mul_(0.5)
        D.conv_out.weight.add_(0.01)
    want1 = eager_general()
    assert maxdiff(want1, got0) > 1e-3                  # (the update matters)
    got1 = gd(x).clone()
    assert maxdiff(got1, want1) < TOL, maxdiff(got1, want1)
    with torch.no_grad():
        large = DM.DCDiscriminator.forward(D, x)        # eager: rebuilds the pack, frees the previous one
        assert maxdiff(large, want1) < 2e-5
        D.blocks[3].weight.mul_(1.25)
        DM.DCDiscriminator.forward(D, x)
    got2 = gd(x).clone()
    assert maxdiff(got2, got1) > 1e-3
    torch.cuda.synchronize()
    assert maxdiff(got2, eager_general()) < TOL


@pytest.mark.parametrize("B,in_dim,out_dim,view", [(1, 3, 7, True), (4, 1, 1, False)])
def test_ada_discriminator_eager_forward_draws_in_the_library(B, in_dim, out_dim, view, monkeypatch):
    """The reference's own call -- ADADiscriminator.forward (src/models/discriminator.py:98-100) without gradient, batch <= 4, the
    shipped xint + scale augmentation -- is ONE library call from the second call on (oi_disc_graph_launch_ada: draws, matrices,
    four launches).  (a) bit-identical to the explicit route (the same seed's matrices from oi_ada_theta_xint_scale handed to
    oi_disc_fwd_small) and seeded by numpy's stream; (b) against the fp64 oracle with the augmentation the library drew;
    (c) follows an in-place weight update; (d) a pinned debug_percentile (instance override) or FAST_ADA = False takes the numpy
    route; (e) the module still deep-copies, and the copy draws the same augmentation from the same numpy state."""
    import copy
    import oi_amd.discriminator as DM
    D = _ada_disc(in_dim, out_dim).cuda().eval()   # (ADADiscriminatorView adds constructor arguments only: same forward)
    with torch.no_grad():
        for p_ in D.parameters():
            p_.copy_((torch.rand_like(p_) * 2 - 1) * (6.0 / (1.04 * p_[0].numel())) ** 0.5)
    H = W = 64
    m = D.aug.static_margins(H, W)
    g = torch.Generator().manual_seed(21)
    dsd = {k: v.detach().double().cpu() for k, v in D.state_dict().items() if "aug." not in k}
    for i in range(3):
        x = torch.rand(B, in_dim, H, W, generator=g).cuda()
        np.random.seed(300 + i)
        with torch.no_grad():
            got = D(x, it=0).clone()
        assert (DM._FAST_ADA.get(D) is not None) and got.shape == (B, out_dim)
        np.random.seed(300 + i)
        th, ts = D.aug.theta_fast(B, H, W, with_draws=True)
        with torch.no_grad():
            want = D._forward_small(x, f12=D.aug.Hz_geom, theta_np=th, margins=m)
        assert torch.equal(got, want), (i, maxdiff(got, want))
        # the oracle on the augmentation the library drew: G_inv = T(-round(t W)) S(1 / s)  (augment.py:213-230)
        t64, s64 = torch.from_numpy(ts[:, :2].astype(np.float64)), torch.from_numpy(ts[:, 2].astype(np.float64))
        G = O.ada_G_inv(B, H, W, t64, s64, dtype=torch.float64)
        ref = O.dc_discriminator(dsd, O.ada_geometric(x.double().cpu(), G)[0])
        assert maxdiff(got.cpu(), ref) < 2e-5 * max(1.0, float(ref.abs().max())), (i, maxdiff(got.cpu(), ref))
    # (c) in-place update: same plan, live weights
    with torch.no_grad():
        D.blocks[2].weight.mul_(0.5)
        np.random.seed(7); a = D(x).clone()
        np.random.seed(7); th = D.aug.theta_fast(B, H, W)
        assert torch.equal(a, D._forward_small(x, f12=D.aug.Hz_geom, theta_np=th, margins=m))
        # (e) deep copy
        twin = copy.deepcopy(D)
        np.random.seed(7); b = twin(x).clone()
        assert torch.equal(a, b)
        # (d) the numpy route: switched off, or debug_percentile pinned by an instance override
        monkeypatch.setattr(DM, "FAST_ADA", False)
        np.random.seed(8); c = D(x).clone()
        np.random.seed(8)
        th_np = D.aug.theta_for(D.aug.sample_G_inv(x, None), m, H, W)
        assert DM._FAST_ADA.get(D) is None and torch.equal(c, D._forward_small(x, f12=D.aug.Hz_geom, theta_np=th_np, margins=m))
        monkeypatch.setattr(DM, "FAST_ADA", True)
        D(x)
        assert DM._FAST_ADA.get(D) is not None
        orig = D.aug.sample_G_inv
        D.aug.sample_G_inv = lambda im, _pct=None: orig(im, 0.7)
        d = D(x).clone()
        th_p = D.aug.theta_for(orig(x, 0.7), m, H, W)
        assert torch.equal(d, D._forward_small(x, f12=D.aug.Hz_geom, theta_np=th_p, margins=m))


def _o1_weights(D):
    with torch.no_grad():   # variance-preserving weights: O(1) logits (the default initialisation gives 1e-3)
        for p_ in D.parameters():
            p_.copy_((torch.rand_like(p_) * 2 - 1) * (6.0 / (1.04 * p_[0].numel())) ** 0.5)
    return D


def _numpy_draw_routes(D, x, seed):
    """From numpy's draws for `seed`: (the pipe's explicit launches at margins fitted to the draw + the general chain, the small
    plan with the same draws' matrices at the static margins)."""
    import oi_amd.discriminator as DM
    import oi_amd.ops as OPS
    B, _, H, W = x.shape
    np.random.seed(seed)
    G = D.aug.sample_G_inv(x, None)
    mf, m = D.aug.margins_for(G, H, W), D.aug.static_margins(H, W)
    xa = OPS.ada_geom_fwd(x, torch.from_numpy(D.aug.theta_for(G, mf, H, W)).cuda(), D.aug.Hz_geom, mf)
    small = D._forward_small(x, f12=D.aug.Hz_geom, theta_np=D.aug.theta_for(G, m, H, W), margins=m).clone()
    small_path, DM.SMALL_PATH = DM.SMALL_PATH, False
    try:
        return DM.DCDiscriminator.forward(D, xa).clone(), small
    finally:
        DM.SMALL_PATH = small_path


@pytest.mark.parametrize("B", [1, 4])
def test_ada_discriminator_reads_the_switches_on_every_call(B, monkeypatch):
    """Once a library-drawn call has filled the memo (DM._FAST_ADA[D]), FAST_ADA / SMALL_PATH = False still take the next call
    off that route -- nothing is popped by hand -- and the route answers again when the switch is set back.  FAST_ADA off: the
    small plan with numpy's draws, bit for bit; SMALL_PATH off: the pipe + the general chain (2e-5 x scale, the bar of
    test_small_batch_discriminator_forward_vs_oracle_and_general_path), and not the small plan's bits."""
    import oi_amd.discriminator as DM
    D = _o1_weights(_ada_disc(3, 7).cuda().eval())
    H = W = 64
    m = D.aug.static_margins(H, W)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(B)).cuda()

    def call(seed):
        np.random.seed(seed)
        return D(x).clone()

    with torch.no_grad():
        a = call(5)
        assert DM._FAST_ADA.get(D) is not None
        np.random.seed(5)
        assert torch.equal(a, D._forward_small(x, f12=D.aug.Hz_geom, theta_np=D.aug.theta_fast(B, H, W), margins=m))
        general, small = _numpy_draw_routes(D, x, 5)
        scale = max(1.0, float(general.abs().max()))
        monkeypatch.setattr(DM, "FAST_ADA", False)
        b = call(5)
        assert torch.equal(b, small) and not torch.equal(b, a)
        monkeypatch.setattr(DM, "FAST_ADA", True)
        assert torch.equal(call(5), a) and DM._FAST_ADA.get(D) is not None
        monkeypatch.setattr(DM, "SMALL_PATH", False)
        c = call(5)
        assert maxdiff(c, general) < 2e-5 * scale and not torch.equal(c, small) and not torch.equal(c, a), maxdiff(c, general)
        monkeypatch.setattr(DM, "SMALL_PATH", True)
        assert torch.equal(call(5), a) and DM._FAST_ADA.get(D) is not None


def test_shipped_128_discriminator_reads_small_path_128_on_every_call(monkeypatch, tag="v_"):
    """The same for SMALL_PATH_128 on the shipped 128 x 128 network (F14's weights) at batch 1."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oi_amd.discriminator as DM
    from test_gpu_backward import _f14_net
    g = load_golden("f14_discriminator_128")
    D, _, _ = _f14_net(g, tag, 1)
    del D.aug.forward                        # (_f14_net pins the percentile through `forward`)
    D = D.eval()
    x = g[f"{tag}b1_x"].cuda()
    with torch.no_grad():
        np.random.seed(5); a = D(x).clone()
        assert DM._FAST_ADA.get(D) is not None
        general, small = _numpy_draw_routes(D, x, 5)
        monkeypatch.setattr(DM, "SMALL_PATH_128", False)
        np.random.seed(5); c = D(x).clone()
        assert maxdiff(c, general) < 2e-5 * max(1.0, float(general.abs().max())), maxdiff(c, general)
        assert not torch.equal(c, small) and not torch.equal(c, a)
        monkeypatch.setattr(DM, "SMALL_PATH_128", True)
        np.random.seed(5)
        assert torch.equal(D(x), a) and DM._FAST_ADA.get(D) is not None


def test_ada_discriminator_memo_follows_replaced_parameters():
    """A Parameter OBJECT replaced after the memo was filled -- by assignment, then by load_state_dict(assign=True) -- is the
    one the next call reads: bit-equal to the explicit route on the live weights, and not the old weights' answer (the memo
    keeps no Parameter; it compares the live addresses each call)."""
    import oi_amd.discriminator as DM
    D = _o1_weights(_ada_disc(3, 7).cuda().eval())
    B, H, W = 1, 64, 64
    m = D.aug.static_margins(H, W)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(2)).cuda()

    def both(seed):
        np.random.seed(seed); got = D(x).clone()
        np.random.seed(seed); th = D.aug.theta_fast(B, H, W)
        return got, D._forward_small(x, f12=D.aug.Hz_geom, theta_np=th, margins=m)

    with torch.no_grad():
        before, want = both(9)
        assert DM._FAST_ADA.get(D) is not None and torch.equal(before, want)
        old = D.blocks[2].weight
        D.blocks[2].weight = torch.nn.Parameter(0.5 * old.detach())
        got, want = both(9)
        assert torch.equal(got, want) and maxdiff(got, before) > 1e-4, maxdiff(got, before)
        assert DM._FAST_ADA.get(D) is not None
        sd2 = {k: (0.5 * v if k == "blocks.0.weight" else v).detach().clone() for k, v in D.state_dict().items()}
        D.load_state_dict(sd2, assign=True)
        got2, want2 = both(9)
        assert torch.equal(got2, want2) and maxdiff(got2, got) > 1e-4, maxdiff(got2, got)


@pytest.mark.parametrize("B,in_dim,out_dim", [(64, 3, 7), (16, 1, 1)])
def test_ada_discriminator_large_batch_forward_draws_in_the_library(B, in_dim, out_dim, monkeypatch):
    """ADADiscriminator.forward without gradient at batch >= 16, the shipped xint + scale augmentation: parameters drawn inside the
    library from one seed of numpy's stream, the matrices in the arguments of ONE augmentation launch (oi_ada_geom_sep_fwd), then
    csrc/disc_large.hip.  (a) equal to the explicit route (the same seed's matrices, the two-launch augmentation, the same
    network path) within the separable form's rounding; (b) against the fp64 oracle with the augmentation the library drew;
    (c) FAST_ADA = False or a pinned debug_percentile takes the numpy route."""
    import oi_amd.discriminator as DM
    import oi_amd.ops as OPS
    D = _ada_disc(in_dim, out_dim).cuda().eval()
    with torch.no_grad():
        for p_ in D.parameters():
            p_.copy_((torch.rand_like(p_) * 2 - 1) * (6.0 / (1.04 * p_[0].numel())) ** 0.5)
    H = W = 64
    m = D.aug.static_margins(H, W)
    x = torch.rand(B, in_dim, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    calls = []
    real = OPS.ada_geom_sep_host
    monkeypatch.setattr(OPS, "ada_geom_sep_host", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    np.random.seed(41)
    with torch.no_grad():
        got = D(x, it=0).clone()
    assert calls == [1] and got.shape == (B, out_dim)
    np.random.seed(41)
    th, ts = D.aug.theta_fast(B, H, W, with_draws=True)
    assert np.all(th[:, 0, 1] == 0) and np.all(th[:, 1, 0] == 0) and np.any(ts[:, 2] != 1)
    with torch.no_grad():
        xa = OPS.ada_geom_fwd(x, torch.from_numpy(th).cuda(), D.aug.Hz_geom, m)          # two launches, device matrices
        want = DM.DCDiscriminator.forward(D, xa)
    assert maxdiff(got, want) < 2e-5 * max(1.0, float(want.abs().max())), maxdiff(got, want)
    if B <= 16:
        dsd = {k: v.detach().double().cpu() for k, v in D.state_dict().items() if "aug." not in k}
        t64, s64 = torch.from_numpy(ts[:, :2].astype(np.float64)), torch.from_numpy(ts[:, 2].astype(np.float64))
        ref = O.dc_discriminator(dsd, O.ada_geometric(x.double().cpu(), O.ada_G_inv(B, H, W, t64, s64, dtype=torch.float64))[0])
        assert maxdiff(got.cpu(), ref) < 2e-5 * max(1.0, float(ref.abs().max())), maxdiff(got.cpu(), ref)
    with torch.no_grad():
        monkeypatch.setattr(DM, "FAST_ADA", False)
        np.random.seed(8); c = D(x).clone()
        np.random.seed(8)
        G = D.aug.sample_G_inv(x, None)
        mf = D.aug.margins_for(G, H, W)
        xa = OPS.ada_geom_fwd(x, torch.from_numpy(D.aug.theta_for(G, mf, H, W)).cuda(), D.aug.Hz_geom, mf)
        assert calls == [1] and maxdiff(c, DM.DCDiscriminator.forward(D, xa)) < 2e-5 * max(1.0, float(c.abs().max()))
        monkeypatch.setattr(DM, "FAST_ADA", True)
        orig = D.aug.sample_G_inv
        D.aug.sample_G_inv = lambda im, _pct=None: orig(im, 0.7)
        D(x)
        assert calls == [1]


def test_step_tail_blob_in_prep_bit_identical_and_one_draw_jitter():
    """Round 6, the no-grad fused forward (generator._prep_fused): (a) the per-element blobs of the f16x3 MLP kernel formed by the
    prep launch's FiLM workgroups (oi_prep_render f3_blob + oi_sdf_mlp_fwd_ex OI_MLP_BLOB_READY) against the call's own blob
    launch: every map of a seeded forward bit-identical, in eval and in training mode (two-call draws); (b) one generator launch
    for latents + jitter: the prep kernel's normal -> uniform map equals the normal CDF evaluated by torch (same coarse samples to
    two ulp of z), the jitter it implies is uniform on [0, 1) (mean / variance over 8,192 rays), and a forward drawn
    that way renders the same distribution of maps (finite, silhouette fraction within 2 % of the two-call forward's)."""
    import oi_amd.generator as GM
    from oi_amd import ops
    gen = build_generator(32, 16, 16, 1, "f16x3")
    keys = ("image", "mask", "shading_map", "color_map", "weight_sum_map")

    def forward(train, blob_in_prep, one_draw, seed=11):
        gen.train(train)
        GM.F3_BLOB_IN_PREP, GM.ONE_DRAW = blob_in_prep, one_draw
        torch.manual_seed(seed)
        np.random.seed(seed)
        try:
            with torch.no_grad():
                out = gen(bs=2, it=0, data={})["box"]
        finally:
            GM.F3_BLOB_IN_PREP, GM.ONE_DRAW = True, True
        return {k: out["render_out"][k].clone() for k in keys}, out["loss"]["eikonal"].clone()

    for train in (False, True):
        a, ea = forward(train, True, False)
        b, eb = forward(train, False, False)
        for k in keys:
            assert torch.equal(a[k], b[k]), (train, k, maxdiff(a[k], b[k]))
        assert torch.equal(ea, eb)
    # (b) the kernel's map of a normal draw to the jitter
    B, R, S = 2, 64, 16
    N = B * R * R
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(N, device="cuda", generator=g)
    u = (0.5 * torch.erfc(-x.double() * 0.5 ** 0.5)).clamp(max=0.99999994).float()
    pose = gen.pose_prior(B).astype(np.float32)
    cam = gen._camera_host()
    w2b = np.linalg.inv(pose).astype(np.float32)
    c2b = (w2b @ cam["c2w"]).astype(np.float32)
    xy = gen._crop_offsets_host(pose, cam)
    kw = dict(b2w=pose, w2b=w2b, c2b=c2b, offs=xy, bg=np.zeros((B, 3), np.float32), kinv=gen._kinv(x.device), R=R, S=S,
              light_direction=gen.light.param_direction, film_P=gen.renderer.pack.film_stacked(differentiable=False),
              z=torch.randn(B, 64, device="cuda", generator=g))
    with torch.no_grad():
        p_n = ops.prep_render(jitter=x, jitter_normal=True, **kw)
        p_u = ops.prep_render(jitter=u, jitter_normal=False, **kw)
        p_0 = ops.prep_render(jitter=None, **kw)
    sec = 2.0 / S
    assert maxdiff(p_n["z_coarse"], p_u["z_coarse"]) < 2e-6   # (z is ~11: one ulp is 9.5e-7; the two uniforms differ by an ulp of theirs)
    jit = ((p_n["z_coarse"] - p_0["z_coarse"])[:, 0].double() / sec + 0.5).cpu().numpy()    # the uniform the kernel used
    assert jit.min() >= -1e-4 and jit.max() <= 1 + 1e-4
    assert abs(jit.mean() - 0.5) < 5 * (1 / 12 / N) ** 0.5 and abs(jit.var() - 1 / 12) < 5 * (1 / 180 / N) ** 0.5
    # a forward drawn with one launch: same kind of picture
    c, _ = forward(True, True, True)
    d, _ = forward(True, True, False)
    for k in keys:
        assert bool(torch.isfinite(c[k]).all())
    assert abs(float((c["mask"] > 0.5).float().mean()) - float((d["mask"] > 0.5).float().mean())) < 0.02


@pytest.mark.parametrize("tag,B", [("v_", 1), ("v_", 2), ("m_", 1), ("m_", 2)])
def test_shipped_128_discriminators_small_batch_forward_f14(tag, B, monkeypatch):
    """Round 6: the batch <= 4 no-grad forward of csrc/disc_small.hip covers the SHIPPED discriminators (configs/train.yaml:78-102:
    128 x 128, 3 | 1 -> 32 -> 64 -> 128 -> 256 -> 512 -> 7 | 1): oi_disc_fwd_small128 / oi_disc_graph_create128 -- the augmentation
    kernel with 32 output channels, d_conv_c32_kernel for the 32 -> 64 block, then the 64 x 64 network's conv 2..4 + head.
    (a) the reference's own logits (F14, ADA at the fixture's pinned percentile) at 2e-5; (b) the general chain it replaces at
    2e-5, and really another path; (c) bit-reproducible; (d) the library-drawn augmentation (ADADiscriminator.forward's one-call
    route) equals the explicit route for the same seed, bit for bit, and follows an in-place weight update."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oi_amd.discriminator as DM
    from test_gpu_backward import _f14_net
    g = load_golden("f14_discriminator_128")
    D, wsd, pct = _f14_net(g, tag, B)
    del D.aug.forward                        # (_f14_net pins the percentile through `forward`: here through sample_G_inv,
    orig = D.aug.sample_G_inv                #  which keeps ADADiscriminator.forward on its small-batch branch)
    D.aug.sample_G_inv = lambda im, _pct=None: orig(im, pct)
    D = D.eval()
    t = f"{tag}b{B}_"
    x = g[t + "x"].cuda()
    with torch.no_grad():
        assert D._small_ok(x)
        d = D(x).clone()
        assert len(DM._SMALL_PLANS.get(D, {})) == 1 and next(iter(DM._SMALL_PLANS[D].values())).big
        assert maxdiff(d.cpu(), g[t + "d"]) < 2e-5 * max(1.0, float(g[t + "d"].abs().max())), maxdiff(d.cpu(), g[t + "d"])
        assert torch.equal(d, D(x))
        monkeypatch.setattr(DM, "SMALL_PATH_128", False)
        general = D(x).clone()
        monkeypatch.setattr(DM, "SMALL_PATH_128", True)
        assert maxdiff(d, general) < 2e-5 * max(1.0, float(general.abs().max())) and not torch.equal(d, general)
        # (d) the one-call route with the draws made inside the library
        del D.aug.sample_G_inv
        H = W = 128
        m = D.aug.static_margins(H, W)
        np.random.seed(31)
        a = D(x).clone()
        assert DM._FAST_ADA.get(D) is not None
        np.random.seed(31)
        th = D.aug.theta_fast(B, H, W)
        assert torch.equal(a, D._forward_small(x, f12=D.aug.Hz_geom, theta_np=th, margins=m))
        D.blocks[1].weight.mul_(0.5)
        np.random.seed(32); b = D(x).clone()
        np.random.seed(32); th = D.aug.theta_fast(B, H, W)
        assert torch.equal(b, D._forward_small(x, f12=D.aug.Hz_geom, theta_np=th, margins=m)) and maxdiff(a, b) > 1e-4
