"""Compositing + Phong shading (csrc/render.hip composite_fwd_kernel, csrc/render_bwd.hip) in the regimes training reaches.

Three things live here, all plain torch on the CPU:

* `restate`: compositing, the Phong maps and the three global sums as ONE function of (sdf, grad, rgb, variance, light
  parameters, light direction), built from the oracle pieces tests/test_gpu_backward.py::test_composite_backward_vs_oracle
  uses (O.inv_s_from_variance, O.transmittance_weights, O.render_maps).  It runs in float64 (the reference) and in float32
  (the reference's own arithmetic noise: the "fp32 floor").  dists, mid_z, the rays, w2b, bg and cos_anneal_ratio are
  constants of that function.
* `REGIMES` / `build_inputs`: named, seeded input builders on an analytic field, with the share of samples / rays each
  regime must put into the branch it is named for (`POPULATION`) and a margin between every sample's deciding quantity
  and the kink next to it (`MARGIN`).
* `FP32_FLOOR` / `FP32_FLOOR_SINGLE` and `bar`: the committed fp32 floors and the bar that follows from them.

The field.  p = rays_o + rays_d * mid_z, r = |p|,  sdf = (r - 0.6) + noise,  grad = (p / r) s + noise with a per-sample
scale s > 0: the sphere of tests/test_gpu_bounds.py::test_composite_ragged in the sign convention a trained network has
(positive outside, gradient outwards).  With the other sign and inv_s in the hundreds both sigmoids are 0 in front of the
surface, alpha = 1e-5 / 1e-5 = 1 at the first sample of EVERY ray and no ray misses or grazes: the populations `trained`
asks for would not exist (at inv_s = 20 already every ray has W > 1 - 1e-3).  `kinks` replaces p / r by a random direction
on the samples within 0.06 of the surface: with the outward gradient true_cos >= 1 only occurs where the ray LEAVES the
sphere, behind the surface, where the transmittance is ~0 and the `tc < 1` mask cannot be felt by any gradient.  Its
population condition therefore also counts, per true_cos band, the samples with influence T_i P (1 - P) > 1e-3, and
tests/test_composite_regimes_cpu.py shows that dropping either relu mask from the restatement moves d_grad far past its bar.

The lower alpha clip.  z is sorted, so dists >= 0, the previous cdf is never below the next one and raw alpha =
(P - N + 1e-5) / (P + 1e-5) >= 1e-5 / (1 + 1e-5) > 0: the clip at 0 (render_bwd.hip `raw > 0.f`) cannot be reached by a
sorted ray.  `sharp` and `trained` therefore carry sections of NEGATIVE length (dists is an input of the kernel and a
constant here), 3 % of all and 40 % of those within 0.03 of the surface, where the two sigmoids differ: there raw < 0 and
alpha == 0 exactly.

The upper alpha clip is no kink of the gradient: 1 - raw = N / (P + 1e-5) exactly, and every derivative of raw carries
that factor, so the gradient goes to 0 continuously as raw -> 1 and a float32 evaluation that rounds raw to 1 changes
nothing measurable.  No margin is kept there; alpha == 1 exactly (N underflows, or 1 - raw < 2^-53) is plentiful.

param_specular at exactly 0.  The light's specular colour is clamp(param_specular, min=0).  torch's clamp passes the
upstream gradient AT the boundary, the kernel (`p.light[1] > 0.f`) does not: both are one-sided derivatives of the same
function.  The expected value is 0 (the `zero_specular` regime asserts it exactly), so the restatement hands
relu(param_specular) -- the same values everywhere, derivative 0 at 0 -- to O.light_terms, whose clamp then is the identity.
"""
import functools
import math

import torch

import oi_oracle as O

B, H, W, T = 2, 3, 4, 70   # N = 24 rays (no multiple of the 4 rays of a workgroup x 64), T crosses the 64-lane scan once
N = B * H * W
S_COARSE = 35              # the last section is 2 / S long (renderer.py:219-225)

PER_SAMPLE = ("weights", "cdf", "alpha", "inside_sphere", "pts_norm")
MAPS = {"weight_sum": 1, "weight_max": 1, "color_fine": 3, "image_no_bg": 3, "image": 3, "shading": 1, "normal": 3,
        "mask": 1, "z_map": 1, "specular_map": 1, "diffuse_map": 1}
REDUCE = ("reduce4[0]", "reduce4[1]", "reduce4[2]")
# the 11 upstream gradients of oi_composite_grads (include/oi_hip.h), then g_reduce4
COTANGENTS = ("weights", "weight_sum", "color_fine", "image_no_bg", "image", "shading", "normal", "mask", "z_map",
              "specular_map", "diffuse_map")
SINGLE_CASES = COTANGENTS + REDUCE
GRADS = ("sdf", "grad", "rgb", "variance", "ambient", "specular", "shininess", "direction")
REDUCE_WEIGHTS = (0.7, 0.3, 0.05)   # of reduce4[0..2] in the all-cotangents loss
SINGLE_REGIMES = ("base", "trained", "degenerate")

# Distance every deciding quantity keeps from its kink (absolute).  A float32 evaluation of these quantities is off by
# ~1e-7 x their magnitude (<= 2.5 for true_cos) and, for W at inv_s = 1e3, by ~inv_s x 6e-8 x |sdf| ~ 3e-5 per alpha.
MARGIN = {"W": 1e-4, "raw": 2e-6, "true_cos": 1e-4, "ndl": 1e-4, "vr": 1e-4, "pts_norm": 1e-5}

BASE_LIGHT = (-0.4, 0.35, 6.0)
_D = dict(light=BASE_LIGHT, car=0.37, sdf_noise=2e-3, scale=(0.9, 1.1), grad_noise=0.1, neg_dists=0.0,
          degenerate=False, bg=True, random_axis_near=0.0)
REGIMES = {
    "base": dict(_D, variance=0.3, sdf_noise=1e-2, seed=101),
    "sharp": dict(_D, variance=0.5, neg_dists=0.03, seed=102),
    "trained": dict(_D, variance=0.7, car=1.0, neg_dists=0.03, sdf_noise=5e-4, seed=103),
    "clamped_hi": dict(_D, variance=1.4, seed=104),
    "clamped_lo": dict(_D, variance=-1.4, seed=105),
    "no_specular": dict(_D, variance=0.5, light=(-0.4, -0.2, 6.0), car=0.0, seed=106),
    "zero_specular": dict(_D, variance=0.5, light=(-0.4, 0.0, 6.0), car=0.0, seed=107),
    "flat_lobe_0.5": dict(_D, variance=0.5, light=(1.5, 0.35, 0.5), seed=108),
    "flat_lobe_1.0": dict(_D, variance=0.5, light=(1.5, 0.35, 1.0), seed=109),
    "kinks": dict(_D, variance=0.5, car=0.5, scale=(0.2, 2.5), random_axis_near=0.06, seed=110),
    "degenerate": dict(_D, variance=0.5, degenerate=True, seed=111),
    "no_bg": dict(_D, variance=0.5, bg=False, seed=112),
}

# Impact parameter of the 12 rays of one element against the sphere of radius 0.6: solid hits, grazing rays on either
# side of the surface, misses.
IMPACT = (0.0, 0.15, 0.3, 0.45, 0.55, 0.59, 0.598, 0.601, 0.603, 0.606, 0.7, 0.85)


def rel_err(a, ref):
    """The one metric of this module and of the GPU test: max |a - ref| / max(1, max |ref|)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    if a.numel() == 0:
        return 0.0
    return float((a.reshape(ref.shape) - ref).abs().max() / max(1.0, float(ref.abs().max())))


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _from_map(m):
    return m.permute(0, 2, 3, 1).reshape(N, -1)


def _relu_unmasked(x):
    """relu's values with derivative 1 everywhere: what a backward that dropped the relu's mask computes."""
    return torch.relu(x).detach() + x - x.detach()


def restate(sdf, grad, rgb, variance, light, direction, c, mutate=None):
    """-> {name: tensor} in the kernel's layouts: the per-sample outputs (N, T), the maps (N, c) and "reduce4" (3,).
    sdf (N, T), grad / rgb (N, T, 3), variance 0-d, light = (ambient, specular, shininess) 0-d each, direction (3,);
    c: the constants (dists, mid_z, rays_o, rays_d, w2b, bg or None, car) in the dtype of the leaves.
    mutate = "tc_lt_1" / "tc_lt_0": the same values, with the gradient mask of that relu of iter_cos dropped (a deliberately
    WRONG backward, for the CPU rehearsal's proof that a regime would notice it)."""
    relu1 = _relu_unmasked if mutate == "tc_lt_1" else torch.relu
    relu0 = _relu_unmasked if mutate == "tc_lt_0" else torch.relu
    car, dists, mid_z, ro, rd = c["car"], c["dists"], c["mid_z"], c["rays_o"], c["rays_d"]
    pts = ro[:, None, :] + rd[:, None, :] * mid_z[..., None]
    inv_s = O.inv_s_from_variance(variance)
    true_cos = (rd[:, None, :] * grad).sum(-1)
    ic = -(relu1(-true_cos * 0.5 + 0.5) * (1 - car) + relu0(-true_cos) * car)
    pc = torch.sigmoid((sdf - ic * dists * 0.5) * inv_s)
    nc = torch.sigmoid((sdf + ic * dists * 0.5) * inv_s)
    raw = (pc - nc + 1e-5) / (pc + 1e-5)
    alpha = raw.clamp(0, 1)
    wts = O.transmittance_weights(alpha)
    pn = torch.linalg.norm(pts, dim=-1)
    relax = (pn < 1.2).to(sdf.dtype)
    gnorm = torch.linalg.norm(grad, dim=-1)
    lsd = {"param_direction": direction, "param_ambient": light[0], "param_specular": torch.relu(light[1]),
           "param_shininess": light[2]}
    ro_dict = {"pts": pts, "weights": wts, "weight_sum": wts.sum(-1, keepdim=True), "gradients": grad, "raw_color": rgb,
               "color_fine": (rgb * wts[..., None]).sum(1), "mid_z_vals": mid_z}
    bg = c["bg"] if c["bg"] is not None else torch.zeros(B, 3, dtype=sdf.dtype)
    maps = O.render_maps(ro_dict, ro, lsd, c["w2b"], bg, B, H, W, return_raw=True)
    out = {"weights": wts, "cdf": pc, "alpha": alpha, "inside_sphere": (pn < 1.0).to(sdf.dtype), "pts_norm": pn,
           "weight_sum": _from_map(maps["weight_sum_map"]), "weight_max": wts.max(-1, keepdim=True)[0],
           "color_fine": _from_map(maps["color_map"]), "image_no_bg": _from_map(maps["image_no_bg"]),
           "image": _from_map(maps["image"]), "shading": _from_map(maps["shading_map"])[:, :1],
           "normal": _from_map(maps["normal_map"]), "mask": _from_map(maps["mask"]), "z_map": _from_map(maps["z_map"]),
           "specular_map": _from_map(maps["specular_map"])[:, :1],
           "diffuse_map": _from_map(maps["diff_shading_map"])[:, :1],
           "reduce4": torch.stack([(relax * (gnorm - 1) ** 2).sum(), relax.sum(), torch.exp(-100.0 * sdf.abs()).sum()])}
    out["_raw"], out["_true_cos"] = raw, true_cos   # (deciding quantities, for `deciding`)
    return out


def constants(inp, dtype):
    c = {k: inp[k].to(dtype) for k in ("dists", "mid_z", "rays_o", "rays_d", "w2b")}
    c["bg"] = None if inp["bg"] is None else inp["bg"].to(dtype)
    c["car"] = inp["car"]
    return c


def leaves(inp, dtype):
    """The eight differentiable inputs in the order of GRADS."""
    mk = lambda t: t.to(dtype).clone().requires_grad_(True)
    return [mk(inp["sdf"]), mk(inp["grad"]), mk(inp["rgb"]), mk(inp["variance"]), mk(inp["light"][0]), mk(inp["light"][1]),
            mk(inp["light"][2]), mk(inp["direction"])]


def evaluate(inp, dtype=torch.float64, single=None, mutate=None):
    """-> (outputs, {name of GRADS: gradient}) of the restatement in `dtype`.  single=None: the loss takes every cotangent of
    `inp["cot"]` and REDUCE_WEIGHTS; single = one name of SINGLE_CASES: that term alone (reduce4[j] with weight 1)."""
    lv = leaves(inp, dtype)
    out = restate(lv[0], lv[1], lv[2], lv[3], (lv[4], lv[5], lv[6]), lv[7], constants(inp, dtype), mutate)
    loss = loss_of(out, inp["cot"], single)
    g = torch.autograd.grad(loss, lv, allow_unused=True)
    grads = {k: (torch.zeros_like(l) if t is None else t) for k, l, t in zip(GRADS, lv, g)}
    return {k: v.detach() for k, v in out.items()}, grads


def loss_of(out, cot, single=None):
    """sum_k <out[k], cot[k]> (+ the reduce4 terms); `out` from `restate` or from the kernel (any device)."""
    r4 = out["reduce4"]
    if single is None:
        loss = sum((out[k] * cot[k].to(out[k])).sum() for k in COTANGENTS)
        return loss + sum(wj * r4[j] for j, wj in enumerate(REDUCE_WEIGHTS))
    if single in REDUCE:
        return r4[REDUCE.index(single)] * 1.0
    return (out[single] * cot[single].to(out[single])).sum()


def flat_outputs(out):
    """{tensor name: tensor} of everything the forward is compared on (PER_SAMPLE + MAPS + REDUCE)."""
    d = {k: out[k] for k in PER_SAMPLE + tuple(MAPS)}
    for j, k in enumerate(REDUCE):
        d[k] = out["reduce4"][j]
    return d


# ----------------------------------------------------------------------------------------------------------------------
# the regimes
# ----------------------------------------------------------------------------------------------------------------------
def deciding(inp):
    """Every quantity a branch of the kernels decides on, from the float64 restatement."""
    d = torch.float64
    lv = [t.detach() for t in leaves(inp, d)]
    c = constants(inp, d)
    out = restate(lv[0], lv[1], lv[2], lv[3], (lv[4], lv[5], lv[6]), lv[7], c)
    grad, ro, rd = lv[1], c["rays_o"], c["rays_d"]
    pts = ro[:, None, :] + rd[:, None, :] * c["mid_z"][..., None]
    ldir = O.light_terms({"param_direction": lv[7], "param_ambient": lv[4], "param_specular": lv[5],
                          "param_shininess": lv[6]}, c["w2b"])[0]
    F = torch.nn.functional
    l = F.normalize(ldir, dim=-1, eps=1e-6).repeat_interleave(N // B, 0)[:, None, :]
    n = F.normalize(grad, dim=-1, eps=1e-6)
    ndl = (n * l).sum(-1)
    view = F.normalize(ro[:, None, :] - pts, dim=-1, eps=1e-6)
    vr = (view * (-l + 2.0 * ndl[..., None] * n)).sum(-1)
    return {"W": out["weight_sum"][:, 0], "raw": out["_raw"], "alpha": out["alpha"], "true_cos": out["_true_cos"], "ndl": ndl,
            "vr": vr, "al": torch.relu(vr) * (ndl > 0), "pts_norm": out["pts_norm"], "gnorm": torch.linalg.norm(grad, dim=-1),
            "sdf": lv[0], "inv_s_raw": torch.exp(lv[3] * 10.0), "influence": _influence(out)}


def _influence(out):
    """T_i P_i (1 - P_i): transmittance in front of the sample times the slope of its sigmoid -- what every gradient that
    passes through the sample's iter_cos is proportional to."""
    om = 1.0 - out["alpha"] + 1e-7
    Ti = torch.cumprod(torch.cat([torch.ones_like(om[:, :1]), om], -1), -1)[:, :-1]
    return Ti * out["cdf"] * (1 - out["cdf"])


def _near(x, *kinks, m):
    bad = torch.zeros_like(x, dtype=torch.bool)
    for k in kinks:
        bad |= (x - k).abs() < m
    return bad


def offenders(inp):
    """-> (samples (N, T) bool, rays (N,) bool) whose deciding quantity lies within MARGIN of a kink, other than the exact
    values `inp["special"]` put there on purpose; plus the samples on which the ORACLE's own gradient is NaN."""
    q = deciding(inp)
    sp = inp["special"]
    zero_g, tiny_g = sp["grad_zero"], sp["grad_tiny"]
    tc_bad = _near(q["true_cos"], 0.0, 1.0, m=MARGIN["true_cos"]) & ~zero_g & ~tiny_g
    # |grad| = 5e-7: true_cos is ~1e-7 by construction; its SIGN decides, and stays decided at 1e-8 (fp32 is off by ~1e-13 there)
    tc_bad |= tiny_g & (q["true_cos"].abs() < 1e-8)
    ndl_bad = _near(q["ndl"], 0.0, m=MARGIN["ndl"]) & ~zero_g   # grad == 0: n = 0 and n.l == 0 exactly, on purpose
    vr_bad = _near(q["vr"], 0.0, m=MARGIN["vr"])
    raw_bad = _near(q["raw"], 0.0, m=MARGIN["raw"])
    s_bad = tc_bad | ndl_bad | vr_bad | raw_bad
    if float(inp["light"][2]) < 1.0:
        # shininess < 1, n.l <= 0 and v.r > 0: al = relu(v.r) * 0 = 0, torch's pow'(0) = inf, inf * (n.l > 0) = NaN and the
        # relu behind it (v.r > 0) lets the NaN through: the oracle has no gradient there, the sample leaves the regime.
        # (With v.r <= 0 relu's backward replaces the inf by 0 and the sample stays: the backfacing al == 0 population.)
        s_bad |= (q["ndl"] <= 0) & (q["vr"] > 0)
    r_bad = _near(q["W"], 1e-3, 1.0 - 1e-3, m=MARGIN["W"])
    return s_bad, r_bad


def _rays(g):
    b = torch.tensor(IMPACT, dtype=torch.float64).repeat(B)
    phi = 2 * math.pi * torch.rand(N, generator=g, dtype=torch.float64)
    Q = torch.linalg.qr(torch.randn(N, 3, 3, generator=g, dtype=torch.float64)).Q
    o_loc = torch.stack([b * torch.cos(phi), b * torch.sin(phi), torch.full_like(b, -3.0)], -1)
    ro = torch.einsum("nij,nj->ni", Q, o_loc).float()
    rd = Q[:, :, 2].float()
    return ro, rd


def build_inputs(name):
    """The regime's inputs (float32 tensors: what the kernel gets; the float64 reference converts the same values),
    deterministic from its seed.  Offending samples are redrawn here; nothing is masked later."""
    spec = REGIMES[name]
    g = torch.Generator().manual_seed(spec["seed"])
    ro, rd = _rays(g)
    near, far = O.near_far_from_sphere(ro, rd)
    z = torch.empty(N, T)
    todo = torch.ones(N, dtype=torch.bool)
    for _ in range(100):   # rows whose |p| comes within MARGIN of the 1.0 / 1.2 masks are drawn again
        k = int(todo.sum())
        if k == 0:
            break
        z[todo] = torch.sort(near[todo] + (far[todo] - near[todo]) * torch.rand(k, T, generator=g), -1).values
        dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), 2.0 / S_COARSE)], -1)
        mid = z + dists * 0.5
        pn = torch.linalg.norm(ro.double()[:, None] + rd.double()[:, None] * mid.double()[..., None], dim=-1)
        todo = _near(pn, 1.0, 1.2, m=MARGIN["pts_norm"]).any(-1)
    assert not bool(todo.any()), name
    p = ro.double()[:, None] + rd.double()[:, None] * mid.double()[..., None]
    r = torch.linalg.norm(p, dim=-1)
    if spec["neg_dists"] > 0:
        flip = (torch.rand(N, T, generator=g) < spec["neg_dists"]) | (((r - 0.6).abs() < 0.03) & (torch.rand(N, T, generator=g) < 0.4))
        flip[:, -1] = False
        dists = torch.where(flip, -dists, dists)
    lo, hi = spec["scale"]
    special = {k: torch.zeros(N, T, dtype=torch.bool) for k in ("grad_zero", "grad_tiny", "sdf_zero")}
    if spec["degenerate"]:
        pick = torch.rand(N, T, generator=g)
        special = {"grad_zero": pick < 0.05, "grad_tiny": (pick >= 0.05) & (pick < 0.10), "sdf_zero": (pick >= 0.10) & (pick < 0.15)}

    def draw(shape_like):
        k = shape_like.shape[0]
        return (torch.randn(k, generator=g, dtype=torch.float64), lo + (hi - lo) * torch.rand(k, generator=g, dtype=torch.float64),
                torch.randn(k, 3, generator=g, dtype=torch.float64))

    sdf = torch.empty(N, T)
    grad = torch.empty(N, T, 3)
    inp = {"rays_o": ro, "rays_d": rd, "dists": dists, "mid_z": mid, "car": spec["car"], "special": special,
           "variance": torch.tensor(spec["variance"]), "light": torch.tensor(spec["light"]),
           "direction": torch.tensor([0.3, -0.5, -0.8]), "rgb": torch.rand(N, T, 3, generator=g)}
    w2b = torch.eye(4).repeat(B, 1, 1)
    w2b[:, :3, :3] = torch.linalg.qr(torch.randn(B, 3, 3, generator=g)).Q
    inp["w2b"] = w2b
    inp["bg"] = torch.rand(B, 3, generator=g) if spec["bg"] else None
    inp["cot"] = {k: torch.randn(N, T, generator=g) if k == "weights" else torch.randn(N, MAPS[k], generator=g) for k in COTANGENTS}
    redo = torch.ones(N, T, dtype=torch.bool)
    for it in range(200):
        idx = redo.nonzero(as_tuple=True)
        if idx[0].numel() == 0:
            break
        e_s, e_k, e_g = draw(idx[0])
        sdf[idx] = ((r[idx] - 0.6) + spec["sdf_noise"] * e_s).float()
        axis = p[idx] / r[idx][:, None]
        if spec["random_axis_near"] > 0:   # (`kinks`: every true_cos band next to the surface, in front of the hit too)
            rnd = torch.nn.functional.normalize(torch.randn(axis.shape, generator=g, dtype=torch.float64), dim=-1)
            near_s = (r[idx] - 0.6).abs() < spec["random_axis_near"]
            axis = torch.where(near_s[:, None], rnd, axis)
            e_k = torch.where(near_s, 0.5 * (e_k + hi), e_k)   # the upper half of the scale range: true_cos >= 1 needs |grad| > 1
        if it >= 10:
            # no redraw of the noise moves these (the oracle's NaN samples of shininess < 1 are a matter of geometry): the
            # field's direction gives way to a random one there
            axis = torch.nn.functional.normalize(torch.randn(axis.shape, generator=g, dtype=torch.float64), dim=-1)
        grad[idx] = (axis * e_k[:, None] + spec["grad_noise"] * e_g).float()
        sdf[special["sdf_zero"]] = 0.0
        grad[special["grad_zero"]] = 0.0
        tiny = special["grad_tiny"]
        grad[tiny] = (torch.nn.functional.normalize(grad[tiny].double(), dim=-1) * 5e-7).float()
        inp["sdf"], inp["grad"] = sdf, grad
        s_bad, r_bad = offenders(inp)
        redo = s_bad | r_bad[:, None]
    assert not bool(redo.any()), (name, int(redo.sum()))
    return inp


def populations(inp):
    """Shares (of samples, or numbers of rays) in the branches the regimes are named for, from the float64 restatement."""
    q = deciding(inp)
    Wt, tc, sp = q["W"], q["true_cos"], inp["special"]
    f = lambda m: float(m.double().mean())
    felt = q["influence"] > 1e-3
    return {"rays_W_below": int((Wt < 1e-3).sum()), "rays_W_window": int(((Wt > 1e-3) & (Wt < 1 - 1e-3)).sum()),
            "rays_W_above": int((Wt > 1 - 1e-3).sum()),
            "alpha_eq_0": int((q["alpha"] == 0).sum()), "alpha_eq_1": int((q["alpha"] == 1).sum()),
            "tc_below_0": f(tc < 0), "tc_0_to_1": f((tc >= 0) & (tc < 1)), "tc_above_1": f(tc >= 1),
            "tc_below_0_felt": f((tc < 0) & felt), "tc_0_to_1_felt": f((tc >= 0) & (tc < 1) & felt), "tc_above_1_felt": f((tc >= 1) & felt),
            "backfacing_al_0": f((q["ndl"] <= 0) & (q["al"] == 0)), "al_positive": f(q["al"] > 0),
            "grad_zero": f(q["gnorm"] == 0), "grad_tiny": f((q["gnorm"] > 0) & (q["gnorm"] <= 1e-6)), "sdf_zero": f(q["sdf"] == 0),
            "inv_s_raw": float(q["inv_s_raw"]), "specular": float(inp["light"][1]), "shininess": float(inp["light"][2]),
            "bg_null": inp["bg"] is None}


def min_margins(inp):
    """Smallest distance of any (non-special) sample to each kink: what `offenders` keeps above MARGIN."""
    q, sp = deciding(inp), inp["special"]
    plain = ~sp["grad_zero"] & ~sp["grad_tiny"]
    mn = lambda x, *ks: min(float((x - k).abs().min()) for k in ks)
    return {"W": mn(q["W"], 1e-3, 1 - 1e-3), "raw": mn(q["raw"], 0.0), "true_cos": mn(q["true_cos"][plain], 0.0, 1.0),
            "ndl": mn(q["ndl"][~sp["grad_zero"]], 0.0), "vr": mn(q["vr"], 0.0), "pts_norm": mn(q["pts_norm"], 1.0, 1.2)}


# what each regime must contain (p = populations(inp))
POPULATION = {
    "base": lambda p: p["rays_W_window"] >= 3 and 15 < p["inv_s_raw"] < 25,
    "sharp": lambda p: 140 < p["inv_s_raw"] < 155 and p["alpha_eq_0"] >= 5 and p["alpha_eq_1"] >= 5,
    "trained": lambda p: (1000 < p["inv_s_raw"] < 1200 and min(p["rays_W_below"], p["rays_W_window"], p["rays_W_above"]) >= 3
                          and p["alpha_eq_0"] >= 5 and p["alpha_eq_1"] >= 5),
    "clamped_hi": lambda p: p["inv_s_raw"] > 1e6,
    "clamped_lo": lambda p: p["inv_s_raw"] < 1e-6,
    "no_specular": lambda p: p["specular"] < 0 and p["al_positive"] >= 0.1,
    "zero_specular": lambda p: p["specular"] == 0 and p["al_positive"] >= 0.1,
    "flat_lobe_0.5": lambda p: p["shininess"] == 0.5 and p["backfacing_al_0"] >= 0.1 and p["al_positive"] >= 0.1,
    "flat_lobe_1.0": lambda p: p["shininess"] == 1.0 and p["backfacing_al_0"] >= 0.1 and p["al_positive"] >= 0.1,
    # (felt: with influence T_i P (1 - P) > 1e-3, where a wrong mask of iter_cos reaches d_grad)
    "kinks": lambda p: (min(p["tc_below_0"], p["tc_0_to_1"], p["tc_above_1"]) >= 0.1
                        and min(p["tc_below_0_felt"], p["tc_0_to_1_felt"], p["tc_above_1_felt"]) >= 0.01),
    "degenerate": lambda p: min(p["grad_zero"], p["grad_tiny"], p["sdf_zero"]) >= 0.04,
    "no_bg": lambda p: p["bg_null"],
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(inputs, float64 outputs, float64 gradients of the all-cotangents loss): built once, shared, never modified."""
    inp = build_inputs(name)
    out, grads = evaluate(inp, torch.float64)
    return inp, out, grads


@functools.lru_cache(maxsize=None)
def single_reference(name, single):
    return evaluate(case(name)[0], torch.float64, single)[1]


def grad_tensors(inp, grads):
    """{"d_" + name: tensor} as compared and reported.  d_grad is split: the samples on the n = g / 1e-6 path (|grad| <= 1e-6)
    carry gradients 1e5 times the others' and would set the scale of the whole tensor; they are "d_grad_eps", a tensor of
    their own (empty outside `degenerate`)."""
    d = {"d_" + k: grads[k].detach().cpu() for k in GRADS}
    eps = torch.linalg.norm(inp["grad"].double(), dim=-1) <= 1e-6
    d["d_grad"], d["d_grad_eps"] = d["d_grad"][~eps], d["d_grad"][eps]
    return d


GRAD_TENSORS = tuple("d_" + k for k in GRADS) + ("d_grad_eps",)


# ----------------------------------------------------------------------------------------------------------------------
# the fp32 floor
# ----------------------------------------------------------------------------------------------------------------------
def measure_floor(name, single=None):
    """rel_err of the float32 restatement against the float64 one, {tensor: error}: outputs (single=None only) and "d_" +
    GRADS.  One thread: the order of torch's sums, and with it the last bits, must not depend on the machine."""
    inp = case(name)[0]
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        o32, g32 = evaluate(inp, torch.float32, single)
    finally:
        torch.set_num_threads(nt)
    if single is None:
        _, o64, g64 = case(name)
        fl = {k: rel_err(v, flat_outputs(o64)[k]) for k, v in flat_outputs(o32).items()}
    else:
        g64, fl = single_reference(name, single), {}
    t32, t64 = grad_tensors(inp, g32), grad_tensors(inp, g64)
    fl.update({k: rel_err(t32[k], t64[k]) for k in GRAD_TENSORS})
    return fl


# bars the project already holds these quantities to (tests/test_gpu_bounds.py::test_composite_ragged: 1e-5 per sample,
# 2e-5 for maps and sums, 2e-5 for per-sample gradients; tests/test_gpu_backward.py COMPOSITE_BWD_TOL for the scalars)
def project_bar(tensor):
    if tensor in PER_SAMPLE:
        return 1e-5
    if tensor in MAPS or tensor in REDUCE or tensor in ("d_sdf", "d_grad", "d_grad_eps", "d_rgb"):
        return 2e-5
    assert tensor in ("d_variance", "d_ambient", "d_specular", "d_shininess", "d_direction"), tensor
    return 1.2e-3


def bar(name, tensor, single=None):
    """-> (bar, "project" | "floor"): the larger of the project's bar and 3x the committed fp32 floor (tests/conftest.py:
    "<= 3x the native-fp32 error")."""
    fl = FP32_FLOOR[name][tensor] if single is None else FP32_FLOOR_SINGLE[name][single][tensor]
    pb = project_bar(tensor)
    return (pb, "project") if pb >= 3.0 * fl else (3.0 * fl, "floor")


# Measured by `measure_floor` (torch CPU, one thread); tests/test_composite_regimes_cpu.py keeps a fresh measurement within
# 1.5x of these.  FP32_FLOOR[regime][tensor]; FP32_FLOOR_SINGLE[regime][cotangent][d_tensor].
FP32_FLOOR = {
    "base": {"weights": 2.327e-07, "cdf": 9.925e-08, "alpha": 9.319e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.379e-07,
        "weight_sum": 5.437e-07, "weight_max": 2.327e-07, "color_fine": 4.003e-07, "image_no_bg": 1.861e-07, "image": 3.363e-07,
        "shading": 2.891e-07, "normal": 4.712e-07, "mask": 5.437e-07, "z_map": 6.495e-07, "specular_map": 3.833e-08,
        "diffuse_map": 9.621e-08, "reduce4[0]": 1.786e-09, "reduce4[1]": 0.000e+00, "reduce4[2]": 9.362e-08, "d_sdf": 2.564e-06,
        "d_grad": 4.475e-07, "d_rgb": 6.612e-07, "d_variance": 3.428e-06, "d_ambient": 6.833e-07, "d_specular": 6.853e-08,
        "d_shininess": 1.382e-09, "d_direction": 3.587e-07, "d_grad_eps": 0.000e+00},
    "sharp": {"weights": 3.293e-07, "cdf": 7.899e-08, "alpha": 1.264e-06, "inside_sphere": 0.000e+00, "pts_norm": 1.338e-07,
        "weight_sum": 4.077e-07, "weight_max": 3.293e-07, "color_fine": 2.032e-07, "image_no_bg": 1.902e-07, "image": 3.166e-07,
        "shading": 3.043e-07, "normal": 3.211e-07, "mask": 4.077e-07, "z_map": 3.616e-07, "specular_map": 1.569e-07,
        "diffuse_map": 1.562e-07, "reduce4[0]": 1.931e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 5.445e-08, "d_sdf": 4.793e-07,
        "d_grad": 3.797e-07, "d_rgb": 2.844e-07, "d_variance": 1.464e-05, "d_ambient": 9.787e-08, "d_specular": 1.671e-06,
        "d_shininess": 8.913e-09, "d_direction": 6.554e-07, "d_grad_eps": 0.000e+00},
    "trained": {"weights": 2.318e-07, "cdf": 8.472e-08, "alpha": 3.157e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.292e-07,
        "weight_sum": 3.282e-07, "weight_max": 2.318e-07, "color_fine": 2.376e-07, "image_no_bg": 1.958e-07, "image": 2.681e-07,
        "shading": 2.045e-07, "normal": 2.229e-07, "mask": 2.778e-07, "z_map": 2.462e-07, "specular_map": 1.164e-07,
        "diffuse_map": 9.514e-08, "reduce4[0]": 3.042e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 2.191e-08, "d_sdf": 8.275e-07,
        "d_grad": 6.523e-07, "d_rgb": 1.603e-07, "d_variance": 1.183e-05, "d_ambient": 1.063e-07, "d_specular": 7.093e-07,
        "d_shininess": 2.565e-08, "d_direction": 4.864e-07, "d_grad_eps": 0.000e+00},
    "clamped_hi": {"weights": 2.026e-07, "cdf": 6.920e-174, "alpha": 2.980e-13, "inside_sphere": 0.000e+00, "pts_norm": 1.363e-07,
        "weight_sum": 2.923e-07, "weight_max": 2.026e-07, "color_fine": 2.292e-07, "image_no_bg": 1.839e-07, "image": 2.314e-07,
        "shading": 2.131e-07, "normal": 2.070e-07, "mask": 1.287e-08, "z_map": 2.736e-07, "specular_map": 6.992e-08,
        "diffuse_map": 7.331e-08, "reduce4[0]": 8.247e-09, "reduce4[1]": 0.000e+00, "reduce4[2]": 1.005e-07, "d_sdf": 9.377e-08,
        "d_grad": 6.955e-07, "d_rgb": 1.327e-07, "d_variance": 0.000e+00, "d_ambient": 1.314e-07, "d_specular": 5.409e-07,
        "d_shininess": 2.624e-08, "d_direction": 4.450e-07, "d_grad_eps": 0.000e+00},
    "clamped_lo": {"weights": 1.185e-07, "cdf": 4.453e-08, "alpha": 1.187e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.283e-07,
        "weight_sum": 4.007e-07, "weight_max": 9.521e-08, "color_fine": 2.860e-07, "image_no_bg": 1.698e-07, "image": 2.437e-07,
        "shading": 2.680e-07, "normal": 3.228e-07, "mask": 4.007e-07, "z_map": 1.251e-06, "specular_map": 4.142e-08,
        "diffuse_map": 1.073e-07, "reduce4[0]": 9.368e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 5.372e-08, "d_sdf": 8.247e-08,
        "d_grad": 4.247e-07, "d_rgb": 5.004e-07, "d_variance": 0.000e+00, "d_ambient": 2.481e-07, "d_specular": 5.971e-07,
        "d_shininess": 1.040e-08, "d_direction": 2.849e-07, "d_grad_eps": 0.000e+00},
    "no_specular": {"weights": 3.399e-07, "cdf": 8.840e-08, "alpha": 8.205e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.309e-07,
        "weight_sum": 4.042e-07, "weight_max": 3.399e-07, "color_fine": 2.722e-07, "image_no_bg": 2.178e-07, "image": 3.194e-07,
        "shading": 2.133e-07, "normal": 2.581e-07, "mask": 2.170e-07, "z_map": 3.306e-07, "specular_map": 0.000e+00,
        "diffuse_map": 1.136e-07, "reduce4[0]": 4.735e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 5.615e-08, "d_sdf": 8.965e-07,
        "d_grad": 4.534e-07, "d_rgb": 2.492e-07, "d_variance": 1.103e-05, "d_ambient": 3.383e-07, "d_specular": 0.000e+00,
        "d_shininess": 0.000e+00, "d_direction": 1.724e-07, "d_grad_eps": 0.000e+00},
    "zero_specular": {"weights": 3.369e-07, "cdf": 8.556e-08, "alpha": 8.800e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.414e-07,
        "weight_sum": 3.573e-07, "weight_max": 3.369e-07, "color_fine": 3.749e-07, "image_no_bg": 1.698e-07, "image": 1.978e-07,
        "shading": 2.866e-07, "normal": 2.466e-07, "mask": 3.335e-07, "z_map": 3.382e-07, "specular_map": 0.000e+00,
        "diffuse_map": 1.384e-07, "reduce4[0]": 1.710e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 1.701e-08, "d_sdf": 1.669e-06,
        "d_grad": 3.252e-07, "d_rgb": 3.098e-07, "d_variance": 2.018e-05, "d_ambient": 1.463e-07, "d_specular": 0.000e+00,
        "d_shininess": 0.000e+00, "d_direction": 4.669e-07, "d_grad_eps": 0.000e+00},
    "flat_lobe_0.5": {"weights": 3.850e-07, "cdf": 1.251e-07, "alpha": 1.047e-06, "inside_sphere": 0.000e+00, "pts_norm": 1.639e-07,
        "weight_sum": 3.727e-07, "weight_max": 3.850e-07, "color_fine": 4.076e-07, "image_no_bg": 4.871e-07, "image": 3.590e-07,
        "shading": 3.713e-07, "normal": 2.979e-07, "mask": 3.727e-07, "z_map": 4.040e-07, "specular_map": 7.937e-08,
        "diffuse_map": 9.403e-08, "reduce4[0]": 7.899e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 2.009e-08, "d_sdf": 6.151e-07,
        "d_grad": 8.963e-07, "d_rgb": 2.041e-07, "d_variance": 5.012e-05, "d_ambient": 3.572e-07, "d_specular": 2.039e-08,
        "d_shininess": 4.745e-07, "d_direction": 6.988e-07, "d_grad_eps": 0.000e+00},
    "flat_lobe_1.0": {"weights": 2.613e-07, "cdf": 8.424e-08, "alpha": 7.219e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.268e-07,
        "weight_sum": 4.754e-07, "weight_max": 2.613e-07, "color_fine": 3.385e-07, "image_no_bg": 3.003e-07, "image": 2.222e-07,
        "shading": 4.181e-07, "normal": 3.937e-07, "mask": 4.754e-07, "z_map": 5.531e-07, "specular_map": 1.008e-07,
        "diffuse_map": 7.033e-08, "reduce4[0]": 7.533e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 4.162e-08, "d_sdf": 8.101e-07,
        "d_grad": 3.521e-07, "d_rgb": 1.986e-07, "d_variance": 1.484e-05, "d_ambient": 1.483e-07, "d_specular": 2.189e-07,
        "d_shininess": 4.711e-08, "d_direction": 1.248e-07, "d_grad_eps": 0.000e+00},
    "kinks": {"weights": 3.601e-07, "cdf": 1.240e-07, "alpha": 6.602e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.466e-07,
        "weight_sum": 3.797e-07, "weight_max": 3.601e-07, "color_fine": 3.128e-07, "image_no_bg": 2.134e-07, "image": 2.460e-07,
        "shading": 2.697e-07, "normal": 2.200e-07, "mask": 3.187e-07, "z_map": 4.876e-07, "specular_map": 8.638e-08,
        "diffuse_map": 1.440e-07, "reduce4[0]": 2.574e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 7.505e-08, "d_sdf": 3.733e-07,
        "d_grad": 5.112e-07, "d_rgb": 2.763e-07, "d_variance": 5.834e-06, "d_ambient": 3.955e-07, "d_specular": 5.434e-07,
        "d_shininess": 2.903e-08, "d_direction": 5.320e-07, "d_grad_eps": 0.000e+00},
    "degenerate": {"weights": 1.751e-07, "cdf": 8.274e-08, "alpha": 6.518e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.507e-07,
        "weight_sum": 3.300e-07, "weight_max": 1.751e-07, "color_fine": 3.105e-07, "image_no_bg": 2.313e-07, "image": 2.373e-07,
        "shading": 2.597e-07, "normal": 2.029e-07, "mask": 2.390e-07, "z_map": 3.747e-07, "specular_map": 1.228e-07,
        "diffuse_map": 1.062e-07, "reduce4[0]": 4.617e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 1.564e-08, "d_sdf": 3.190e-07,
        "d_grad": 5.355e-07, "d_rgb": 2.337e-07, "d_variance": 2.492e-05, "d_ambient": 2.305e-08, "d_specular": 4.919e-07,
        "d_shininess": 3.242e-08, "d_direction": 4.104e-07, "d_grad_eps": 5.704e-07},
    "no_bg": {"weights": 4.340e-07, "cdf": 8.483e-08, "alpha": 6.788e-07, "inside_sphere": 0.000e+00, "pts_norm": 1.487e-07,
        "weight_sum": 3.388e-07, "weight_max": 4.340e-07, "color_fine": 2.889e-07, "image_no_bg": 2.237e-07, "image": 2.237e-07,
        "shading": 3.035e-07, "normal": 2.309e-07, "mask": 3.131e-07, "z_map": 4.102e-07, "specular_map": 1.844e-08,
        "diffuse_map": 1.529e-07, "reduce4[0]": 1.266e-08, "reduce4[1]": 0.000e+00, "reduce4[2]": 1.344e-08, "d_sdf": 5.456e-07,
        "d_grad": 3.256e-07, "d_rgb": 4.307e-07, "d_variance": 3.240e-05, "d_ambient": 3.488e-07, "d_specular": 6.877e-08,
        "d_shininess": 3.162e-08, "d_direction": 1.824e-07, "d_grad_eps": 0.000e+00},
}
FP32_FLOOR_SINGLE = {
    "base": {
        "weights": {"d_sdf": 9.671e-07, "d_grad": 4.021e-07, "d_rgb": 0.000e+00, "d_variance": 1.521e-05, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "weight_sum": {"d_sdf": 1.514e-06, "d_grad": 1.035e-07, "d_rgb": 0.000e+00, "d_variance": 4.561e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "color_fine": {"d_sdf": 1.365e-06, "d_grad": 1.227e-07, "d_rgb": 5.273e-07, "d_variance": 4.904e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "image_no_bg": {"d_sdf": 1.416e-06, "d_grad": 1.778e-07, "d_rgb": 2.396e-07, "d_variance": 5.206e-06, "d_ambient": 2.355e-07,
            "d_specular": 9.284e-08, "d_shininess": 6.475e-09, "d_direction": 6.415e-07, "d_grad_eps": 0.000e+00},
        "image": {"d_sdf": 1.003e-06, "d_grad": 1.385e-07, "d_rgb": 1.675e-07, "d_variance": 8.021e-06, "d_ambient": 5.525e-07,
            "d_specular": 8.073e-08, "d_shininess": 1.171e-10, "d_direction": 4.398e-07, "d_grad_eps": 0.000e+00},
        "shading": {"d_sdf": 3.226e-06, "d_grad": 1.059e-07, "d_rgb": 0.000e+00, "d_variance": 4.283e-07, "d_ambient": 1.038e-07,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 2.162e-07, "d_grad_eps": 0.000e+00},
        "normal": {"d_sdf": 1.244e-06, "d_grad": 3.158e-07, "d_rgb": 0.000e+00, "d_variance": 1.036e-05, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "mask": {"d_sdf": 2.338e-06, "d_grad": 8.799e-08, "d_rgb": 0.000e+00, "d_variance": 1.066e-05, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "z_map": {"d_sdf": 9.497e-06, "d_grad": 1.774e-07, "d_rgb": 0.000e+00, "d_variance": 9.502e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "specular_map": {"d_sdf": 2.612e-07, "d_grad": 3.187e-08, "d_rgb": 0.000e+00, "d_variance": 1.688e-06, "d_ambient": 0.000e+00,
            "d_specular": 8.269e-08, "d_shininess": 4.016e-09, "d_direction": 3.238e-08, "d_grad_eps": 0.000e+00},
        "diffuse_map": {"d_sdf": 6.154e-07, "d_grad": 9.034e-08, "d_rgb": 0.000e+00, "d_variance": 1.198e-05, "d_ambient": 7.042e-09,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 5.282e-07, "d_grad_eps": 0.000e+00},
        "reduce4[0]": {"d_sdf": 0.000e+00, "d_grad": 2.120e-07, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "reduce4[1]": {"d_sdf": 0.000e+00, "d_grad": 0.000e+00, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "reduce4[2]": {"d_sdf": 5.966e-08, "d_grad": 0.000e+00, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
    },
    "trained": {
        "weights": {"d_sdf": 4.127e-07, "d_grad": 2.245e-07, "d_rgb": 0.000e+00, "d_variance": 2.453e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "weight_sum": {"d_sdf": 7.140e-07, "d_grad": 2.475e-07, "d_rgb": 0.000e+00, "d_variance": 5.641e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "color_fine": {"d_sdf": 3.439e-07, "d_grad": 2.433e-07, "d_rgb": 1.749e-07, "d_variance": 8.212e-08, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "image_no_bg": {"d_sdf": 7.351e-07, "d_grad": 4.312e-07, "d_rgb": 1.424e-07, "d_variance": 1.436e-05, "d_ambient": 3.751e-08,
            "d_specular": 2.471e-07, "d_shininess": 1.210e-08, "d_direction": 5.825e-07, "d_grad_eps": 0.000e+00},
        "image": {"d_sdf": 1.033e-06, "d_grad": 1.691e-07, "d_rgb": 2.588e-07, "d_variance": 1.017e-05, "d_ambient": 1.402e-07,
            "d_specular": 3.032e-09, "d_shininess": 2.297e-09, "d_direction": 3.395e-07, "d_grad_eps": 0.000e+00},
        "shading": {"d_sdf": 3.089e-07, "d_grad": 4.628e-07, "d_rgb": 0.000e+00, "d_variance": 4.134e-07, "d_ambient": 7.075e-08,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 8.705e-08, "d_grad_eps": 0.000e+00},
        "normal": {"d_sdf": 5.573e-07, "d_grad": 6.985e-07, "d_rgb": 0.000e+00, "d_variance": 3.316e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "mask": {"d_sdf": 5.150e-07, "d_grad": 4.744e-07, "d_rgb": 0.000e+00, "d_variance": 3.950e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "z_map": {"d_sdf": 4.040e-07, "d_grad": 3.790e-07, "d_rgb": 0.000e+00, "d_variance": 6.080e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "specular_map": {"d_sdf": 7.829e-07, "d_grad": 8.048e-07, "d_rgb": 0.000e+00, "d_variance": 5.465e-08, "d_ambient": 0.000e+00,
            "d_specular": 2.654e-07, "d_shininess": 9.321e-09, "d_direction": 4.464e-07, "d_grad_eps": 0.000e+00},
        "diffuse_map": {"d_sdf": 3.200e-07, "d_grad": 3.434e-07, "d_rgb": 0.000e+00, "d_variance": 1.019e-06, "d_ambient": 6.036e-08,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 1.523e-07, "d_grad_eps": 0.000e+00},
        "reduce4[0]": {"d_sdf": 0.000e+00, "d_grad": 1.790e-07, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "reduce4[1]": {"d_sdf": 0.000e+00, "d_grad": 0.000e+00, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "reduce4[2]": {"d_sdf": 7.383e-08, "d_grad": 0.000e+00, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
    },
    "degenerate": {
        "weights": {"d_sdf": 1.930e-07, "d_grad": 5.463e-07, "d_rgb": 0.000e+00, "d_variance": 1.889e-05, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 1.318e-07},
        "weight_sum": {"d_sdf": 2.907e-07, "d_grad": 8.837e-08, "d_rgb": 0.000e+00, "d_variance": 1.631e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 2.548e-08},
        "color_fine": {"d_sdf": 4.044e-07, "d_grad": 2.980e-07, "d_rgb": 1.246e-07, "d_variance": 3.990e-05, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 7.108e-08},
        "image_no_bg": {"d_sdf": 4.206e-07, "d_grad": 1.006e-06, "d_rgb": 1.489e-07, "d_variance": 5.243e-06, "d_ambient": 1.286e-07,
            "d_specular": 4.549e-07, "d_shininess": 1.252e-08, "d_direction": 3.795e-07, "d_grad_eps": 4.736e-07},
        "image": {"d_sdf": 2.854e-07, "d_grad": 6.227e-07, "d_rgb": 1.062e-07, "d_variance": 1.202e-05, "d_ambient": 5.028e-08,
            "d_specular": 6.873e-08, "d_shininess": 1.638e-08, "d_direction": 2.210e-07, "d_grad_eps": 4.862e-07},
        "shading": {"d_sdf": 3.019e-07, "d_grad": 1.834e-07, "d_rgb": 0.000e+00, "d_variance": 1.282e-06, "d_ambient": 1.053e-07,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 1.338e-07, "d_grad_eps": 9.598e-07},
        "normal": {"d_sdf": 8.397e-07, "d_grad": 1.507e-07, "d_rgb": 0.000e+00, "d_variance": 8.558e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 1.552e-07},
        "mask": {"d_sdf": 3.230e-07, "d_grad": 1.121e-07, "d_rgb": 0.000e+00, "d_variance": 3.288e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 5.640e-08},
        "z_map": {"d_sdf": 3.877e-07, "d_grad": 3.482e-07, "d_rgb": 0.000e+00, "d_variance": 4.325e-06, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 2.019e-07},
        "specular_map": {"d_sdf": 9.868e-07, "d_grad": 2.053e-07, "d_rgb": 0.000e+00, "d_variance": 1.965e-07, "d_ambient": 0.000e+00,
            "d_specular": 4.988e-08, "d_shininess": 7.360e-09, "d_direction": 9.693e-08, "d_grad_eps": 4.290e-08},
        "diffuse_map": {"d_sdf": 2.378e-07, "d_grad": 6.129e-08, "d_rgb": 0.000e+00, "d_variance": 1.588e-06, "d_ambient": 1.268e-07,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 2.332e-07, "d_grad_eps": 6.156e-07},
        "reduce4[0]": {"d_sdf": 0.000e+00, "d_grad": 1.740e-07, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 7.116e-08},
        "reduce4[1]": {"d_sdf": 0.000e+00, "d_grad": 0.000e+00, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
        "reduce4[2]": {"d_sdf": 6.161e-08, "d_grad": 0.000e+00, "d_rgb": 0.000e+00, "d_variance": 0.000e+00, "d_ambient": 0.000e+00,
            "d_specular": 0.000e+00, "d_shininess": 0.000e+00, "d_direction": 0.000e+00, "d_grad_eps": 0.000e+00},
    },
}
