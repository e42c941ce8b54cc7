"""The style network, the FiLM heads (csrc/mlp.hip film_params_kernel, film_heads_bwd_kernel, style_bwd_kernel; the copy in
csrc/render.hip prep_render_kernel) and the stand-alone colour head (csrc/color_head.hip) in the regimes a trained model
reaches.  All plain torch on the CPU, nothing of oi_amd.  tests/helpers/mlp_regimes.py takes gamma and beta as kernel inputs;
this file holds the kernels that PRODUCE them, and the head that consumes the last pair, to the same kind of reference.

* `cell(name)`: explicit float32 tensors built from tests/golden/weights_sdf.npz / weights_color.npz by seeded, documented
  transforms (seeds: zlib.crc32 of the cell's full name).  A film cell is `<regime>[@B]`, a colour cell `colour/<regime>[@npe]`.
* `film_restate` / `colour_restate`: oi_oracle.style_mlp, film_params and color_head with every weight as an argument.
  Unmutated they are the oracle to 1e-12 in float64 and bit for bit in float32 (tests/test_film_regimes_cpu.py).  float64 is the
  reference, autograd through float64 the backward reference, float32 the reference's own arithmetic noise.
* `film_backward` / `colour_backward`: the same backward written out by hand (the kernels' identities: no division by gamma,
  per-chunk partial sums), because a mutation is one wrong LINE; unmutated they equal float64 autograd to 1e-12.
* `FP32_FLOOR[cell][tensor]`: worst float32-versus-float64 error over the float32 variants listed under "What float32 may
  do" below, measured on one thread by `measure_floor` and committed; `bar` = 3 x floor (tests/conftest.py: "<= 3x the
  native-fp32 error"), never above the project's existing bar of the tensor (PROJECT_BAR) and never below 4 ulp of the
  tensor's largest entry (a bar below the format's own step is luck of an order of summation; mlp_regimes.BAR_MIN_BACKWARD).
* `MUTATIONS`, `CAUGHT_BY`: one wrong line each, rehearsed on the CPU; each exceeds 3 x bar in the cells CAUGHT_BY names.

Error measures.  w, gamma, beta, rgb: max |a - ref|.  Gradients: max |a - ref| / max(1, max |ref|), the measure of
tests/test_gpu_backward.py -- per FiLM layer and per style layer, because a stacked tensor would hide its small layers
(`layer_range` scales the cotangents of layer l by 10^(2 - l)).  One exception, `batch_cancel`: d_gb = 15 sum_b d_gamma_b and
d_bb = 0.25 sum_b d_beta_b are there sums of 33 terms of alternating sign that cancel to ~1e-3 of sum_b |term|; a float32 sum
is accurate to a few ulp of sum |term|, NOT of the result, so these two are measured against max(1, max_f sum_b |term|).

Statements the kernels are held to
----------------------------------
* leaky_relu at a pre-activation of exactly 0 (`dead_units`: four rows of style layer 1 and their bias are 0): the forward
  gives 0 and the BACKWARD USES SLOPE 0.2 -- torch.nn.functional.leaky_relu differentiates as `x > 0 ? 1 : 0.2`, and so do the
  kernels (`acc > 0.f ? 1.0f : 0.2f`).
* d_gamma of the colour head is formed without dividing by gamma (sum_i Wv[f][i] D_e[f][i] + bv[f] D_e[f][131]): at gamma = 0
  (`colour/gamma_spread`) it is the only non-zero gradient of the row.
* a cotangent of exactly 0 gives exactly 0: `layer_range` (one FiLM layer), `colour/quiet_element` (one batch element).

What float32 may do (the variants `measure_floor` takes the worst of)
--------------------------------------------------------------------
* torch's own float32 evaluation of the restatement and of its autograd;
* the style / head products as ONE fma chain in the order k = 0..63, with `15 x + 30` both as a product and a sum and as one
  fma (a compiler may contract it);
* the colour head with every sine and cosine off by a seeded uniform +-2.5e-7, the bound
  tests/test_gpu_kernels.py::test_device_sincos_accuracy holds the device to for |x| <= 100 (all phases here are below 100);
* sums over points in another ORDER: partial sums of 128-point blocks added one after the other in float32 (the colour head
  adds per-chunk partials in a fixed order of its own); d_brgb, d_bv / d_beta as one float32 running sum over four seeded
  permutations (mlp_regimes._summation_order_errors).

What was measured differently from the issue's sketch
-----------------------------------------------------
* `colour/trained_rgb`: k = 400 saturates (the issue says so); k = RGB_GAIN with a bias spread of +-RGB_BIAS covers about
  [1e-3, 1 - 1e-3] and keeps every backward bar at or below 5e-6.
* `grown`: see GROWN_STYLE / GROWN_HEAD.

* The workspace of the large colour case (B = 2, npe = 66000) is 198 MB (135 MB of per-point vectors, 61 MB of chunk
  partials), not about 140 MB.
* d_z of oi_film_params_bwd is computed FROM d_w, which the heads accumulate with atomics: it is order-dependent too and is
  held to the bar, not to bit-identity; with d_w fixed (ops.style_bwd) it is bit-identical, and the test demands that.
* No kernel failed: no fault was found, MUTATIONS holds rehearsals only.

Measured on the MI355X
----------------------
For every call and tensor kind the (cell, layer) that used the largest share of its bar; all 1072 (call, cell, tensor) entries:
profiles/film_regimes_margins.txt.  The forward errors EQUAL their floors where the fma-chain variant is the worst one: the
kernels' float32 arithmetic is that chain, bit for bit.

  call               tensor      cell                        GPU error     floor       bar  of bar
  forward            w           grown@1                      1.01e-06  1.01e-06  3.04e-06    0.33
  forward            gamma       grown@3                      1.13e-05  1.13e-05  3.40e-05    0.33
  forward            beta        init@33                      1.16e-07  1.16e-07  3.47e-07    0.33
  FieldPack.film     w           grown@1                      1.01e-06  1.01e-06  3.04e-06    0.33
  FieldPack.film     gamma       grown@3                      1.13e-05  1.13e-05  3.40e-05    0.33
  FieldPack.film     beta        init@33                      1.16e-07  1.16e-07  3.47e-07    0.33
  prep_render        w           grown@1                      1.01e-06  1.01e-06  3.04e-06    0.33
  prep_render        gamma       grown@3                      1.13e-05  1.13e-05  3.40e-05    0.33
  prep_render        beta        init@33                      1.16e-07  1.16e-07  3.47e-07    0.33
  backward           d_gw.1      init@1                       3.37e-07  1.74e-07  5.23e-07    0.64
  backward           d_gb.3      dead_units@33                3.02e-07  1.29e-07  4.77e-07    0.63
  backward           d_bw.4      init@1                       3.26e-07  1.60e-07  4.80e-07    0.68
  backward           d_bb.7      one_sided@33                 2.38e-07  1.17e-07  4.77e-07    0.50
  backward           d_w         one_sided@33                 2.24e-07  2.38e-07  7.14e-07    0.31
  backward           d_style_w.2 grown@1                      3.24e-07  2.12e-07  6.35e-07    0.51
  backward           d_style_b.1 one_sided@1                  2.32e-07  1.82e-07  5.47e-07    0.42
  backward           d_z         dead_units@1                 3.42e-07  2.81e-07  8.42e-07    0.41
  style_bwd          d_style_w.2 grown@1                      3.24e-07  2.12e-07  6.35e-07    0.51
  style_bwd          d_style_b.0 one_sided@33                 3.16e-07  2.39e-07  7.16e-07    0.44
  style_bwd          d_z         dead_units@1                 3.42e-07  2.81e-07  8.42e-07    0.41
  colour             rgb         colour/quiet_element@165     3.78e-07  3.95e-07  1.18e-06    0.32
  colour             d_feat      colour/trained_rgb@33        2.70e-07  2.21e-07  6.62e-07    0.41
  colour             d_normals   colour/quiet_element@165     1.93e-07  1.67e-07  5.00e-07    0.39
  colour             d_gamma     colour/trained_rgb@1         8.91e-09  5.07e-09  1.52e-08    0.59
  colour             d_beta      colour/trained_rgb@1         4.55e-08  2.60e-08  7.80e-08    0.58
  colour             d_wv        colour/trained_rgb@1         8.03e-07  4.65e-07  1.39e-06    0.58
  colour             d_bv        colour/trained_rgb@1         7.27e-07  4.58e-07  1.37e-06    0.53
  colour             d_wrgb      colour/trained_rgb@1         1.43e-07  1.19e-07  3.57e-07    0.40
  colour             d_brgb      colour/saturated@165         3.05e-12  3.05e-12  9.16e-12    0.33
  colour (npe 66000) d_brgb      colour/trained_rgb@66000     7.14e-07  1.17e-05  5.00e-06    0.14
  colour stride 1152 d_gamma     colour/trained_rgb           4.93e-08  5.57e-08  1.67e-07    0.29
  colour stride 1152 d_beta      colour/trained_rgb           4.55e-07  5.06e-07  1.52e-06    0.30
"""
import functools
import math
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import oi_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
C, NL_ALL = 128, 9

# the project's existing bars: test_film_params (w, gamma, beta), test_color_network_forward_standalone_golden_f2 (rgb),
# test_film_params_backward_vs_oracle (film / style gradients), COLOR_HEAD_BWD_TOL (colour-head gradients)
PROJECT_BAR = {"w": 1e-5, "gamma": 1e-4, "beta": 1e-5, "rgb": 2e-5, "film_backward": 2e-5, "colour_backward": 5e-6}
ULP4 = 4 * 2.0 ** -23

FILM_FWD_CELLS = ("init", "grown", "one_sided", "dead_units", "w_route")
FILM_BWD_CELLS = FILM_FWD_CELLS + ("layer_range", "batch_cancel")
FILM_FWD_B = (1, 3, 33)
FILM_BWD_B = (1, 33)
GROWN_STYLE = 1.25       # grown: style weights x 1.25 per layer (|w| x ~2) ...
GROWN_HEAD = 1.35        # ... head weights x 1.35: gamma then spans about [-20, 80] (test_film_cells_hold_their_population)
ONE_SIDED_NEG, ONE_SIDED_POS = (0, -7.0), (2, 6.0)     # (style layer, bias shift)
ONE_SIDED_HEAD = 0.5     # one_sided: |w| reaches 13; head weights x 0.5 keep gamma within [-25, 82] and its floor below 1e-4 / 3
DEAD_LAYER, DEAD_ROWS = 1, (3, 17, 40, 63)
PSI = 0.5                # w_route: truncation
ZERO_COT_LAYER = 5       # layer_range: the FiLM layer whose cotangents are exactly 0
CANCEL_SIGMA = 5e-3      # batch_cancel: relative spread of the alternating terms

COLOUR_CELLS = ("init", "trained_rgb", "saturated", "gamma_spread", "steep_normals", "quiet_element")
COLOUR_B, COLOUR_NPE = 2, 165
SHAPE_NPE = (1, 16, 17, 31, 32, 33, 127, 129, 152, 513)
BIG_NPE = 66000          # B npe just above 131072: the smallest shape at which carve() leaves chunks of 128 points
RGB_GAIN, RGB_BIAS = 40.0, 2.0
SATURATED_BIAS = (30.0, -30.0, 100.0)
PINNED = ((3, 0.0), (17, 3e-3), (40, -7e-3), (77, -12.0), (101, 80.0), (127, 0.0))     # colour/gamma_spread: (row, gamma)
STEEP = 30.0
TRIG_EPS = 2.5e-7
FILM_STRIDE_ALL = NL_ALL * C     # 1152: layer 8 of a [B][9][128] tensor in place


def _seed(name):
    return zlib.crc32(name.encode())


def _golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return {k: torch.from_numpy(np.asarray(f[k])) for k in f.files}


@functools.lru_cache(maxsize=None)
def golden_sds():
    return _golden("weights_sdf"), _golden("weights_color")


def stacked(sd, csd):
    """The six stacked arrays oi_film_params takes (oi_amd.params.stack_field_params, restated)."""
    head = lambda part, kind: torch.stack([sd[f"pts_linears.{l}.{part}.{kind}"] for l in range(8)] +
                                          [csd[f"views_linears.{part}.{kind}"]])
    return {"style_w": torch.stack([sd[f"style.{i}.weight"] for i in range(3)]),
            "style_b": torch.stack([sd[f"style.{i}.bias"] for i in range(3)]),
            "gw": head("gamma", "weight"), "gb": head("gamma", "bias"), "bw": head("beta", "weight"), "bb": head("beta", "bias")}


FILM_PARAMS = ("style_w", "style_b", "gw", "gb", "bw", "bb")


def split_name(name):
    """'colour/trained_rgb@513' -> ('colour', 'trained_rgb', 513); 'grown' -> ('film', 'grown', None)."""
    fam, rest = ("colour", name[7:]) if name.startswith("colour/") else ("film", name)
    regime, _, n = rest.partition("@")
    return fam, regime, (int(n) if n else None)


# ----------------------------------------------------------------------------------------------------------------------
# film cells
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mean_w():
    """w-bar of the truncation trick: the mean style vector of 1024 seeded latents at the golden weights."""
    g = torch.Generator().manual_seed(_seed("w_route/mean"))
    return O.style_mlp(golden_sds()[0], torch.randn(1024, 64, generator=g)).mean(0)


def _film_build(regime, B):
    name = f"{regime}@{B}"
    g = torch.Generator().manual_seed(_seed(name))
    c = {k: v.clone() for k, v in stacked(*golden_sds()).items()}
    c.update(name=name, regime=regime, B=B, w=None, z=torch.randn(B, 64, generator=g),    # latents are always N(0, 1)
             cg=torch.randn(B, NL_ALL, C, generator=g), cb=torch.randn(B, NL_ALL, C, generator=g),
             cw=torch.randn(B, 64, generator=g))
    if regime == "init":
        pass
    elif regime == "grown":
        c["style_w"] *= GROWN_STYLE
        c["gw"] *= GROWN_HEAD
        c["bw"] *= GROWN_HEAD
    elif regime == "one_sided":
        for l, shift in (ONE_SIDED_NEG, ONE_SIDED_POS):
            c["style_b"][l] += shift
        c["gw"] *= ONE_SIDED_HEAD
        c["bw"] *= ONE_SIDED_HEAD
    elif regime == "dead_units":
        rows = list(DEAD_ROWS)
        c["style_w"][DEAD_LAYER][rows] = 0.0
        c["style_b"][DEAD_LAYER][rows] = 0.0
    elif regime == "w_route":
        wbar = mean_w()
        c["w"] = wbar + PSI * (O.style_mlp(golden_sds()[0], c["z"]) - wbar)      # formed on the host; no style MLP runs
        c["z"] = None
    elif regime == "layer_range":
        for l in range(NL_ALL):
            s = 0.0 if l == ZERO_COT_LAYER else 10.0 ** (2 - l)
            c["cg"][:, l] *= s
            c["cb"][:, l] *= s
    elif regime == "batch_cancel":
        sign = torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)])
        amp = torch.tensor([(B // 2) / ((B + 1) // 2) if b % 2 == 0 else 1.0 for b in range(B)])    # 17 x 16/17 against 16 x 1
        for k in ("cg", "cb"):
            base = torch.randn(NL_ALL, C, generator=g)
            c[k] = (sign * amp)[:, None, None] * base * (1.0 + CANCEL_SIGMA * torch.randn(B, NL_ALL, C, generator=g))
    else:
        raise KeyError(regime)
    return c


def _lrelu_fwd(pre):
    return F.leaky_relu(pre, 0.2)


def film_restate(c, dtype=torch.float64, mutate=None, leaves=False, nl=NL_ALL, l0=0):
    """-> dict(w (B,64), gamma (B,nl,128), beta (B,nl,128)[, leaves, pres, hs]): oi_oracle.style_mlp and film_params on the
    cell's weights, FiLM layers l0 .. l0 + nl - 1.  leaves=True: the parameters and z (or w) require grad."""
    t = {k: c[k].to(dtype) for k in FILM_PARAMS}
    src = c["z"] if c["z"] is not None else c["w"]
    src = src.to(dtype)
    if leaves:
        t = {k: v.clone().requires_grad_(True) for k, v in t.items()}
        src = src.clone().requires_grad_(True)
    h, pres, hs = src, [], [src]
    if c["z"] is not None:
        for i in range(3):
            pre = h @ t["style_w"][i].t() + t["style_b"][i]
            h = _lrelu_fwd(pre)
            pres.append(pre)
            hs.append(h)
    w = h
    gs, bs = [], []
    for l in range(l0, l0 + nl):
        lb = max(l - 1, 0) if mutate == "layer_reads_previous_gb" else l
        pg = w @ t["gw"][l].t() + t["gb"][lb]
        pb = w @ t["bw"][l].t() + t["bb"][l]
        gs.append(0.25 * pg if mutate == "quarter_on_gamma" else 15.0 * pg + 30.0)
        bs.append(15.0 * pb + 30.0 if mutate == "affine_on_beta" else 0.25 * pb + 0.0)
    out = {"w": w, "gamma": torch.stack(gs, 1) if nl else None, "beta": torch.stack(bs, 1) if nl else None, "pres": pres, "hs": hs}
    if leaves:
        out["leaves"] = dict(t, src=src)
    return out


def _fma(a, b, c_):
    """float32 fma: one rounding (through float64: the product of two float32 is exact there)."""
    return (a.double() * b.double() + c_.double()).float()


def film_chain32(c, contract):
    """The float32 forward as one fma chain per output in the order k = 0..63 (a kernel's natural order); contract: `15 x + 30`
    and `0.25 x + 0` as one fma."""
    t = {k: c[k].float() for k in FILM_PARAMS}

    def chain(h, W):                               # h (B, 64), W (M, 64) -> (B, M)
        acc = torch.zeros(h.shape[0], W.shape[0])
        for k in range(64):
            acc = _fma(h[:, k:k + 1].expand(-1, W.shape[0]), W[:, k][None].expand(h.shape[0], -1), acc)
        return acc

    if c["z"] is not None:
        h = c["z"].float()
        for i in range(3):
            h = _lrelu_fwd(chain(h, t["style_w"][i]) + t["style_b"][i])
    else:
        h = c["w"].float()
    gs, bs = [], []
    for l in range(NL_ALL):
        pg, pb = chain(h, t["gw"][l]) + t["gb"][l], chain(h, t["bw"][l]) + t["bb"][l]
        gs.append(_fma(torch.full_like(pg, 15.0), pg, torch.full_like(pg, 30.0)) if contract else 15.0 * pg + 30.0)
        bs.append(0.25 * pb + 0.0)
    return {"w": h, "gamma": torch.stack(gs, 1), "beta": torch.stack(bs, 1)}


FILM_MUTATIONS_FWD = ("affine_on_beta", "quarter_on_gamma", "layer_reads_previous_gb")
FILM_MUTATIONS_BWD = ("slope_one_at_zero", "slope_from_wrong_layer", "d_w_assigned", "d_gb_misses_last_element")


def film_backward(c, dtype=torch.float64, mutate=None):
    """The backward of <cg, gamma> + <cb, beta> + <cw, w> by hand, as the kernels form it (csrc/mlp.hip) -> {tensor: gradient}
    with the names of `film_backward_names`."""
    t = {k: c[k].to(dtype) for k in FILM_PARAMS + ("cg", "cb", "cw")}
    with torch.no_grad():
        f = film_restate(c, dtype)
        w = f["w"]
        dg, db = 15.0 * t["cg"], 0.25 * t["cb"]
        out = {}
        for l in range(NL_ALL):
            out[f"d_gw.{l}"], out[f"d_bw.{l}"] = dg[:, l].t() @ w, db[:, l].t() @ w
            out[f"d_gb.{l}"] = (dg[:-1, l] if mutate == "d_gb_misses_last_element" else dg[:, l]).sum(0)
            out[f"d_bb.{l}"] = db[:, l].sum(0)
        d_w = torch.zeros_like(w) if mutate == "d_w_assigned" else t["cw"].clone()
        for l in range(NL_ALL):                    # accumulated layer by layer (atomics over l on the device)
            d_w = d_w + dg[:, l] @ t["gw"][l] + db[:, l] @ t["bw"][l]
        out["d_w"] = d_w
        if c["z"] is None:
            return out
        dh = d_w
        for l in (2, 1, 0):
            if mutate == "slope_one_at_zero":
                pos = f["pres"][l] >= 0
            elif mutate == "slope_from_wrong_layer":
                pos = f["hs"][l] > 0               # the layer's INPUT (the post-activation of the layer before; z for layer 0)
            else:
                pos = f["pres"][l] > 0             # exactly 0 -> 0.2 (module docstring)
            dp = dh * torch.where(pos, torch.ones((), dtype=dtype), torch.full((), 0.2, dtype=dtype))
            out[f"d_style_b.{l}"] = dp.sum(0)
            out[f"d_style_w.{l}"] = dp.t() @ f["hs"][l]
            dh = dp @ t["style_w"][l]
        out["d_z"] = dh
    return out


def film_backward_names(c):
    n = [f"{k}.{l}" for k in ("d_gw", "d_gb", "d_bw", "d_bb") for l in range(NL_ALL)] + ["d_w"]
    if c["z"] is not None:
        n += [f"{k}.{l}" for k in ("d_style_w", "d_style_b") for l in range(3)] + ["d_z"]
    return n


def film_autograd(c, dtype=torch.float64):
    """Autograd through `film_restate` -> the tensors of `film_backward_names`."""
    f = film_restate(c, dtype, leaves=True)
    loss = (f["gamma"] * c["cg"].to(dtype)).sum() + (f["beta"] * c["cb"].to(dtype)).sum() + (f["w"] * c["cw"].to(dtype)).sum()
    lv = f["leaves"]
    from_z = c["z"] is not None
    wanted = [lv["gw"], lv["gb"], lv["bw"], lv["bb"], f["w"] if from_z else lv["src"]] + ([lv["style_w"], lv["style_b"], lv["src"]] if from_z else [])
    gr = torch.autograd.grad(loss, wanted)
    out = {}
    for k, g in zip(("d_gw", "d_gb", "d_bw", "d_bb"), gr[:4]):
        for l in range(NL_ALL):
            out[f"{k}.{l}"] = g[l]
    out["d_w"] = gr[4]
    if from_z:
        for l in range(3):
            out[f"d_style_w.{l}"], out[f"d_style_b.{l}"] = gr[5][l], gr[6][l]
        out["d_z"] = gr[7]
    return out


def split_film_grads(r):
    """ops.film_params_bwd's dict -> the tensors of `film_backward_names` (CPU)."""
    out = {}
    for k in ("d_gw", "d_gb", "d_bw", "d_bb"):
        for l in range(r[k].shape[0]):
            out[f"{k}.{l}"] = r[k][l].detach().cpu()
    out["d_w"] = r["d_w"].detach().cpu()
    if "d_style_w" in r:
        for l in range(3):
            out[f"d_style_w.{l}"], out[f"d_style_b.{l}"] = r["d_style_w"][l].detach().cpu(), r["d_style_b"][l].detach().cpu()
    if "d_z" in r:
        out["d_z"] = r["d_z"].detach().cpu()
    return out


# ----------------------------------------------------------------------------------------------------------------------
# colour cells
# ----------------------------------------------------------------------------------------------------------------------
COLOUR_PARAMS = ("wv", "bv", "wrgb", "brgb")
COLOUR_LEAVES = ("feat", "normals", "gamma", "beta") + COLOUR_PARAMS
COLOUR_GRADS = ("d_feat", "d_normals", "d_gamma", "d_beta", "d_wv", "d_bv", "d_wrgb", "d_brgb")


def _trained_rgb(c):
    c["wrgb"] *= RGB_GAIN
    c["brgb"] = torch.tensor([-RGB_BIAS, 0.0, RGB_BIAS])


def _colour_build(regime, npe):
    name = f"colour/{regime}@{npe}"
    g = torch.Generator().manual_seed(_seed(name))
    sd, csd = golden_sds()
    B, n = COLOUR_B, COLOUR_B * npe
    w = O.style_mlp(sd, torch.randn(B, 64, generator=g))
    gamma, beta = O.film_params(csd, "views_linears.", w)
    c = {"name": name, "regime": regime, "B": B, "npe": npe, "w": w, "gamma": gamma.contiguous(), "beta": beta.contiguous(),
         "feat": torch.rand(n, C, generator=g) * 2.0 - 1.0,                       # features are sines: [-1, 1]
         "normals": torch.randn(n, 3, generator=g) * 3.0,                         # raw d sdf/dx, as test_gpu_backward feeds it
         "wv": csd["views_linears.weight"].clone(), "bv": csd["views_linears.bias"].clone(),
         "wrgb": csd["rgb_linear.weight"].clone(), "brgb": csd["rgb_linear.bias"].clone(),
         "cot": torch.randn(n, 3, generator=g)}
    if regime == "init":
        pass
    elif regime == "trained_rgb":
        _trained_rgb(c)
    elif regime == "saturated":
        c["brgb"] = torch.tensor(SATURATED_BIAS)
    elif regime == "gamma_spread":
        _trained_rgb(c)
        for f, target in PINNED:
            c["gamma"][:, f] = target
    elif regime == "steep_normals":
        _trained_rgb(c)
        idx = torch.randperm(n, generator=g)
        k = max(n // 10, 1)
        c["normals"][idx[:k]] *= STEEP / 3.0 / 3.0                                  # N(0, 3) -> N(0, 10): |n| up to about 30
        c["normals"][idx[k:2 * k]] = 0.0
        c["feat"][idx[2 * k]] = 0.0
    elif regime == "quiet_element":
        _trained_rgb(c)
        c["cot"][npe:] = 0.0
    else:
        raise KeyError(regime)
    return c


def _pp(v, npe):
    return v.repeat_interleave(npe, dim=0)     # as O._per_point


def colour_restate(c, dtype=torch.float64, leaves=False, mutate=None, noise=None):
    """-> dict(rgb (n,3), phi, a, pre[, leaves]): oi_oracle.color_head with gamma / beta and every weight as arguments.
    noise: a torch.Generator -- every sine is off by a uniform +-TRIG_EPS (the device's bound)."""
    t = {k: c[k].to(dtype) for k in COLOUR_LEAVES}
    if leaves:
        t = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    gam, bet = t["gamma"], t["beta"]
    if mutate == "film_row_of_previous_element":
        gam, bet = gam.roll(1, 0), bet.roll(1, 0)
    g, b = _pp(gam, c["npe"]), _pp(bet, c["npe"])
    u = torch.cat([t["feat"], t["normals"]], -1) @ t["wv"].t() + t["bv"]
    phi = g * u + b
    a = torch.sin(phi)
    if noise is not None:
        a = a + ((torch.rand(a.shape, generator=noise) * 2.0 - 1.0) * TRIG_EPS).to(dtype)
    pre = a @ t["wrgb"].t() + t["brgb"]
    out = {"rgb": torch.sigmoid(pre), "phi": phi, "a": a, "pre": pre, "u": u, "g": g}
    if leaves:
        out["leaves"] = t
    return out


COLOUR_MUTATIONS = ("film_row_of_previous_element", "sigmoid_derivative_is_o", "d_gamma_divides_by_gamma",
                    "chunk_drops_last_point", "chunk_4_and_later_not_added", "d_gamma_stride_128")


def carve(B, npe):
    """csrc/color_head.hip carve(), restated: -> dict(chunk_pts, nchunk, tail, tiles, total).  ~1024 workgroups for the point
    GEMM, chunks of whole register batches (32 points), at least 128 points, never straddling a batch element."""
    n = B * npe
    tiles = (npe + 127) // 128
    cp = (n + 1023) // 1024
    cp = (cp + 31) // 32 * 32
    cp = max(cp, 128)
    nchunk = (npe + cp - 1) // cp
    al = lambda b: (b + 255) // 256 * 256
    total = 2 * al(n * C * 4) + al(n * 16) + al(B * nchunk * C * 144 * 4) + al(B * tiles * 4 * 16)
    return {"chunk_pts": cp, "nchunk": nchunk, "tail": npe - (nchunk - 1) * cp, "tiles": tiles, "total": total}


def colour_backward(c, dtype=torch.float64, mutate=None, noise=None, block=None):
    """The backward of <cot, rgb> by hand with the identities of csrc/color_head.hip -> {tensor of COLOUR_GRADS: gradient}.
    The weight-side sums run per element over chunks of carve()'s size (block: another chunk size), the partials are added one
    after the other in `dtype`."""
    t = {k: c[k].to(dtype) for k in COLOUR_LEAVES + ("cot",)}
    B, npe = c["B"], c["npe"]
    with torch.no_grad():
        f = colour_restate(c, dtype, mutate=mutate, noise=noise)
        o = f["rgb"]
        dpre = t["cot"] * (o if mutate == "sigmoid_derivative_is_o" else o * (1.0 - o))
        cosphi = torch.cos(f["phi"])
        if noise is not None:
            cosphi = cosphi + ((torch.rand(cosphi.shape, generator=noise) * 2.0 - 1.0) * TRIG_EPS).to(dtype)
        dphi = (dpre @ t["wrgb"]) * cosphi
        du = f["g"] * dphi
        dc = du @ t["wv"]
        out = {"d_feat": dc[:, :C], "d_normals": dc[:, C:]}
        cin1 = torch.cat([t["feat"], t["normals"], torch.ones(B * npe, 1, dtype=dtype)], -1)      # [c | 1]
        cp = block or carve(B, npe)["chunk_pts"]
        gam = t["gamma"].roll(1, 0) if mutate == "film_row_of_previous_element" else t["gamma"]
        d_wv1 = torch.zeros(C, C + 4, dtype=dtype)
        d_wrgb = torch.zeros(3, C, dtype=dtype)
        d_brgb = torch.zeros(3, dtype=dtype)
        d_gamma, d_beta = [], []
        wvb = torch.cat([t["wv"], t["bv"][:, None]], -1)                                         # [Wv | bv]
        for e in range(B):
            D = torch.zeros(C, C + 4, dtype=dtype)
            E = torch.zeros(3, C, dtype=dtype)
            for ci, p0 in enumerate(range(0, npe, cp)):
                p1 = min(p0 + cp, npe)
                if mutate == "chunk_drops_last_point":
                    p1 -= 1
                if mutate == "chunk_4_and_later_not_added" and ci >= 4:
                    continue
                s = slice(e * npe + p0, e * npe + p1)
                D = D + dphi[s].t() @ cin1[s]
                E = E + dpre[s].t() @ f["a"][s]
                d_brgb = d_brgb + dpre[s].sum(0)
            d_wv1 = d_wv1 + gam[e][:, None] * D
            d_wrgb = d_wrgb + E
            if mutate == "d_gamma_divides_by_gamma":
                s = slice(e * npe, (e + 1) * npe)
                d_gamma.append(((du[s] / f["g"][s]) * ((f["phi"][s] - _pp(t["beta"], npe)[s]) / f["g"][s])).sum(0))
            else:
                d_gamma.append((wvb * D).sum(-1))
            d_beta.append(D[:, C + 3])
        out.update(d_wv=d_wv1[:, :C + 3], d_bv=d_wv1[:, C + 3], d_wrgb=d_wrgb, d_brgb=d_brgb,
                   d_gamma=torch.stack(d_gamma), d_beta=torch.stack(d_beta))
    return out


def place_strided(rows, mutate=None, poison=float("nan")):
    """(B, 128) rows -> the (B, 9, 128) tensor a caller with d_film_stride = 1152 receives at layer 8, the other layers
    poisoned; `d_gamma_stride_128` writes element e at 128 e instead of 1152 e."""
    B = rows.shape[0]
    buf = torch.full((B * NL_ALL * C,), poison, dtype=rows.dtype)
    base = 8 * C
    stride = C if mutate == "d_gamma_stride_128" else FILM_STRIDE_ALL
    for e in range(B):
        buf[base + e * stride: base + e * stride + C] = rows[e]
    return buf.view(B, NL_ALL, C)


def colour_autograd(c, dtype=torch.float64):
    f = colour_restate(c, dtype, leaves=True)
    gr = torch.autograd.grad((f["rgb"] * c["cot"].to(dtype)).sum(), [f["leaves"][k] for k in COLOUR_LEAVES])
    return dict(zip(COLOUR_GRADS, gr))


# ----------------------------------------------------------------------------------------------------------------------
# cells, references
# ----------------------------------------------------------------------------------------------------------------------
def canonical(name):
    fam, regime, n = split_name(name)
    if fam == "colour":
        return f"colour/{regime}@{COLOUR_NPE if n is None else n}"
    return f"{regime}@{(33 if regime == 'batch_cancel' else 3) if n is None else n}"


@functools.lru_cache(maxsize=None)
def _cell(name):
    fam, regime, n = split_name(name)
    return _colour_build(regime, n) if fam == "colour" else _film_build(regime, n)


def cell(name):
    """The cell's tensors (float32), built once, shared, never modified.  'grown' = 'grown@3', 'colour/init' = 'colour/init@165'."""
    return _cell(canonical(name))


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 forward of the cell, computed once and shared."""
    c = cell(name)
    with torch.no_grad():
        if split_name(name)[0] == "colour":
            return {"rgb": colour_restate(c)["rgb"]}
        f = film_restate(c)
        return {k: f[k] for k in ("w", "gamma", "beta")}


@functools.lru_cache(maxsize=None)
def reference_backward(name):
    """float64 autograd of the cell, computed once and shared."""
    c = cell(name)
    return colour_autograd(c) if split_name(name)[0] == "colour" else film_autograd(c)


def film_cells(backward=False):
    """Every film cell name the GPU test runs."""
    if not backward:
        return [f"{r}@{B}" for r in FILM_FWD_CELLS for B in FILM_FWD_B]
    return [f"{r}@{B}" for r in FILM_BWD_CELLS for B in FILM_BWD_B if not (r == "batch_cancel" and B == 1)]


def colour_cells(big=False):
    return [f"colour/{r}@{COLOUR_NPE}" for r in COLOUR_CELLS] + [f"colour/trained_rgb@{n}" for n in SHAPE_NPE] + \
        ([f"colour/trained_rgb@{BIG_NPE}"] if big else [])


def all_cells():
    return sorted(set(film_cells()) | set(film_cells(True))) + colour_cells(big=True)


# ----------------------------------------------------------------------------------------------------------------------
# errors, floors, bars
# ----------------------------------------------------------------------------------------------------------------------
def _finite(a):
    return bool(torch.isfinite(a).all())


def scale_of(name, tensor):
    """The denominator of a gradient's error: max(1, max |ref|) -- or max(1, max_f sum_b |term|) for d_gb / d_bb of
    batch_cancel (module docstring)."""
    c = cell(name)
    if c.get("regime") == "batch_cancel" and tensor.split(".")[0] in ("d_gb", "d_bb"):
        k, l = tensor.split(".")
        terms = (15.0 * c["cg"] if k == "d_gb" else 0.25 * c["cb"]).double()[:, int(l)]
        return max(1.0, float(terms.abs().sum(0).max()))
    return max(1.0, float(reference_backward(name)[tensor].abs().max()))


def errors(name, cand):
    """{tensor: error} of a candidate's forward outputs (w, gamma, beta / rgb) against float64: max |a - ref|; not finite: inf."""
    out = {}
    for k, ref in reference(name).items():
        if cand.get(k) is None:
            continue
        a = cand[k].detach().double().cpu()
        out[k] = float((a - ref).abs().max()) if _finite(a) else math.inf
    return out


def backward_errors(name, grads):
    ref = reference_backward(name)
    out = {}
    for k in ref:
        if grads.get(k) is None:
            continue
        a = grads[k].detach().double().cpu()
        out[k] = float((a - ref[k]).abs().max()) / scale_of(name, k) if _finite(a) else math.inf
    return out


def _seq_sum32(terms, gen, times=4):
    """(n, m) float64 terms -> worst |float32 running sum - exact| over `times` seeded permutations, per column."""
    exact = terms.sum(0)
    worst = torch.zeros_like(exact)
    for _ in range(times):
        seq = np.cumsum(terms.float()[torch.randperm(terms.shape[0], generator=gen)].numpy(), axis=0, dtype=np.float32)[-1]
        worst = torch.maximum(worst, (torch.from_numpy(seq).double() - exact).abs())
    return worst


def measure_floor(name):
    """{tensor: worst float32-versus-float64 error over the variants of the module docstring}, on one thread (the order of
    torch's sums must not depend on the machine)."""
    c = cell(name)
    fam = split_name(name)[0]
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    worst = {}

    def take(d):
        for k, e in d.items():
            worst[k] = max(worst.get(k, 0.0), e)
    try:
        with torch.no_grad():
            if fam == "film":
                take(errors(name, film_restate(c, torch.float32)))
                take(errors(name, film_chain32(c, False)))
                take(errors(name, film_chain32(c, True)))
            else:
                take(errors(name, colour_restate(c, torch.float32)))
                for s in range(2):
                    take(errors(name, colour_restate(c, torch.float32, noise=torch.Generator().manual_seed(_seed(name) + s))))
        if fam == "film":
            if name in film_cells(True):
                take(backward_errors(name, film_autograd(c, torch.float32)))
                take(backward_errors(name, film_backward(c, torch.float32)))
                if c["regime"] == "batch_cancel":
                    # d_gb / d_bb as ONE float32 running sum over the batch (the natural order of a kernel), four seeded orders:
                    # where the terms cancel, the order decides the error (everywhere else the 4-ulp floor of `bar` covers it)
                    gen = torch.Generator().manual_seed(_seed(name + "/summation order"))
                    for l in range(NL_ALL):
                        for k, terms in ((f"d_gb.{l}", 15.0 * c["cg"][:, l]), (f"d_bb.{l}", 0.25 * c["cb"][:, l])):
                            for _ in range(4):
                                seq = np.cumsum(terms[torch.randperm(c["B"], generator=gen)].numpy(), axis=0, dtype=np.float32)[-1]
                                take(backward_errors(name, {k: torch.from_numpy(seq)}))
        else:
            take(backward_errors(name, colour_autograd(c, torch.float32)))
            take(backward_errors(name, colour_backward(c, torch.float32)))
            take(backward_errors(name, colour_backward(c, torch.float32, block=128)))
            for s in range(2):
                take(backward_errors(name, colour_backward(c, torch.float32, noise=torch.Generator().manual_seed(_seed(name) + 7 + s))))
            # the order of a float32 running sum over the points: d_brgb (one term per point), d_beta / d_bv (dphi)
            ref = colour_restate(c)
            dpre = c["cot"].double() * ref["rgb"] * (1.0 - ref["rgb"])
            gen = torch.Generator().manual_seed(_seed(name + "/summation order"))
            take({"d_brgb": float(_seq_sum32(dpre, gen).max()) / scale_of(name, "d_brgb")})
            dphi = (dpre @ c["wrgb"].double()) * torch.cos(ref["phi"])
            e = max(float(_seq_sum32(dphi[i * c["npe"]:(i + 1) * c["npe"]], gen, 2).max()) for i in range(c["B"]))
            take({"d_beta": e / scale_of(name, "d_beta")})
    finally:
        torch.set_num_threads(nt)
    return worst


def project_bar(tensor):
    if tensor in PROJECT_BAR:
        return PROJECT_BAR[tensor]
    return PROJECT_BAR["colour_backward" if tensor in COLOUR_GRADS else "film_backward"]


def ulp_floor(name, tensor):
    """4 ulp of the tensor's largest entry, in the tensor's error measure."""
    if tensor in ("w", "gamma", "beta", "rgb"):
        return ULP4 * float(reference(name)[tensor].abs().max())
    c = cell(name)
    if c.get("regime") == "batch_cancel" and tensor.split(".")[0] in ("d_gb", "d_bb"):
        k, l = tensor.split(".")       # the partial sums of cancelling terms are as large as one term: 4 ulp of the largest
        terms = (15.0 * c["cg"] if k == "d_gb" else 0.25 * c["cb"]).double()[:, int(l)]
        return ULP4 * float(terms.abs().max()) / scale_of(name, tensor)
    return ULP4 * min(1.0, float(reference_backward(name)[tensor].abs().max()))


def bar(name, tensor):
    """3 x the committed float32 floor, at least 4 ulp of the tensor's largest entry, at most the project's existing bar."""
    name = canonical(name)
    return min(max(3.0 * FP32_FLOOR[name][tensor], ulp_floor(name, tensor)), project_bar(tensor))


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
MUTATIONS = FILM_MUTATIONS_FWD + FILM_MUTATIONS_BWD + COLOUR_MUTATIONS


def mutated_errors(mutation, name):
    """{tensor: error / bar} of the float64 restatement with one wrong line, judged as the GPU output is."""
    c = cell(name)
    out = {}
    if mutation in FILM_MUTATIONS_FWD:
        with torch.no_grad():
            e = errors(name, film_restate(c, mutate=mutation))
    elif mutation in FILM_MUTATIONS_BWD:
        e = backward_errors(name, film_backward(c, mutate=mutation))
    elif mutation == "d_gamma_stride_128":
        g = colour_backward(c)
        got = place_strided(g["d_gamma"], mutate=mutation)[:, 8]
        e = backward_errors(name, {"d_gamma": got})
    else:
        with torch.no_grad():
            e = errors(name, colour_restate(c, mutate=mutation))
        e.update(backward_errors(name, colour_backward(c, mutate=mutation)))
    for k, v in e.items():
        b = bar(name, k)               # (0 where the reference is exactly 0: then only exactly 0 passes)
        out[k] = v / b if b > 0 else (0.0 if v == 0 else math.inf)
    return out


# Which cells catch which mutation at 3 x bar (tests/test_film_regimes_cpu.py::test_mutation_is_caught demands every entry).
CAUGHT_BY = {
    "affine_on_beta": ("init@3", "grown@33", "w_route@1"),
    "quarter_on_gamma": ("init@3", "grown@33", "w_route@1"),
    "layer_reads_previous_gb": ("init@3", "grown@1", "one_sided@33"),
    # the four dead rows of style layer 1: slope 1 instead of 0.2 in d_style_b.1 / d_style_w.1
    "slope_one_at_zero": ("dead_units@1", "dead_units@33"),
    # layer 0 all negative, layer 2 all positive: the neighbour's sign is wrong for every unit
    "slope_from_wrong_layer": ("one_sided@1", "one_sided@33", "init@33"),
    "d_w_assigned": ("layer_range@1", "layer_range@33", "w_route@33"),
    "d_gb_misses_last_element": ("batch_cancel@33", "init@33", "layer_range@1"),
    "film_row_of_previous_element": ("colour/init", "colour/gamma_spread", "colour/trained_rgb@17"),
    # at the golden weights o = 0.5 and o (1 - o) = 0.25 = o / 2: the flat middle; the trained head separates them
    "sigmoid_derivative_is_o": ("colour/trained_rgb", "colour/steep_normals", "colour/init"),
    "d_gamma_divides_by_gamma": ("colour/gamma_spread",),
    "chunk_drops_last_point": ("colour/trained_rgb", "colour/trained_rgb@129", "colour/trained_rgb@1"),
    "chunk_4_and_later_not_added": ("colour/trained_rgb@513",),
    "d_gamma_stride_128": ("colour/trained_rgb", "colour/gamma_spread"),
}

# Measured by `measure_floor` (torch CPU, one thread); tests/test_film_regimes_cpu.py keeps a fresh measurement within 1.5x.
FP32_FLOOR = {
    "batch_cancel@33": {
        "w": 1.291e-06, "gamma": 6.905e-06, "beta": 9.186e-08, "d_gw.0": 5.433e-07, "d_gw.1": 4.524e-07,
        "d_gw.2": 5.114e-07, "d_gw.3": 4.763e-07, "d_gw.4": 5.273e-07, "d_gw.5": 5.094e-07, "d_gw.6": 5.572e-07,
        "d_gw.7": 4.855e-07, "d_gw.8": 5.326e-07, "d_gb.0": 2.223e-08, "d_gb.1": 2.152e-08, "d_gb.2": 2.338e-08,
        "d_gb.3": 2.567e-08, "d_gb.4": 1.504e-08, "d_gb.5": 1.860e-08, "d_gb.6": 1.905e-08, "d_gb.7": 1.880e-08,
        "d_gb.8": 1.725e-08, "d_bw.0": 5.076e-07, "d_bw.1": 4.570e-07, "d_bw.2": 5.124e-07, "d_bw.3": 5.036e-07,
        "d_bw.4": 4.806e-07, "d_bw.5": 5.384e-07, "d_bw.6": 5.585e-07, "d_bw.7": 5.038e-07, "d_bw.8": 4.993e-07,
        "d_bb.0": 2.174e-08, "d_bb.1": 1.254e-08, "d_bb.2": 1.622e-08, "d_bb.3": 3.117e-08, "d_bb.4": 2.846e-08,
        "d_bb.5": 2.272e-08, "d_bb.6": 4.196e-08, "d_bb.7": 2.935e-08, "d_bb.8": 2.402e-08, "d_w": 2.665e-07,
        "d_style_w.0": 3.108e-07, "d_style_b.0": 5.017e-07, "d_style_w.1": 3.384e-07, "d_style_b.1": 4.219e-07,
        "d_style_w.2": 5.142e-07, "d_style_b.2": 3.636e-07, "d_z": 4.266e-07,
    },
    "dead_units@1": {
        "w": 5.615e-07, "gamma": 5.163e-06, "beta": 8.763e-08, "d_gw.0": 1.264e-07, "d_gw.1": 1.472e-07,
        "d_gw.2": 1.122e-07, "d_gw.3": 1.162e-07, "d_gw.4": 1.239e-07, "d_gw.5": 1.194e-07, "d_gw.6": 1.161e-07,
        "d_gw.7": 1.206e-07, "d_gw.8": 1.171e-07, "d_gb.0": 3.994e-08, "d_gb.1": 5.357e-08, "d_gb.2": 2.719e-08,
        "d_gb.3": 3.673e-08, "d_gb.4": 3.968e-08, "d_gb.5": 3.779e-08, "d_gb.6": 3.207e-08, "d_gb.7": 3.887e-08,
        "d_gb.8": 3.769e-08, "d_bw.0": 1.170e-07, "d_bw.1": 1.187e-07, "d_bw.2": 1.123e-07, "d_bw.3": 1.119e-07,
        "d_bw.4": 1.083e-07, "d_bw.5": 1.080e-07, "d_bw.6": 1.117e-07, "d_bw.7": 1.151e-07, "d_bw.8": 1.036e-07,
        "d_bb.0": 0.000e+00, "d_bb.1": 0.000e+00, "d_bb.2": 0.000e+00, "d_bb.3": 0.000e+00, "d_bb.4": 0.000e+00,
        "d_bb.5": 0.000e+00, "d_bb.6": 0.000e+00, "d_bb.7": 0.000e+00, "d_bb.8": 0.000e+00, "d_w": 2.749e-07,
        "d_style_w.0": 2.784e-07, "d_style_b.0": 2.935e-07, "d_style_w.1": 2.871e-07, "d_style_b.1": 2.650e-07,
        "d_style_w.2": 2.711e-07, "d_style_b.2": 3.030e-07, "d_z": 2.806e-07,
    },
    "dead_units@3": {
        "w": 5.839e-07, "gamma": 4.505e-06, "beta": 8.375e-08,
    },
    "dead_units@33": {
        "w": 1.275e-06, "gamma": 7.349e-06, "beta": 1.153e-07, "d_gw.0": 3.249e-07, "d_gw.1": 2.628e-07,
        "d_gw.2": 2.615e-07, "d_gw.3": 2.648e-07, "d_gw.4": 2.554e-07, "d_gw.5": 3.313e-07, "d_gw.6": 2.745e-07,
        "d_gw.7": 2.260e-07, "d_gw.8": 3.232e-07, "d_gb.0": 9.700e-08, "d_gb.1": 1.017e-07, "d_gb.2": 9.844e-08,
        "d_gb.3": 1.292e-07, "d_gb.4": 1.009e-07, "d_gb.5": 1.428e-07, "d_gb.6": 9.414e-08, "d_gb.7": 1.012e-07,
        "d_gb.8": 1.104e-07, "d_bw.0": 2.823e-07, "d_bw.1": 2.722e-07, "d_bw.2": 2.828e-07, "d_bw.3": 2.638e-07,
        "d_bw.4": 2.754e-07, "d_bw.5": 2.044e-07, "d_bw.6": 2.442e-07, "d_bw.7": 2.298e-07, "d_bw.8": 2.552e-07,
        "d_bb.0": 1.601e-07, "d_bb.1": 1.057e-07, "d_bb.2": 1.361e-07, "d_bb.3": 1.085e-07, "d_bb.4": 1.116e-07,
        "d_bb.5": 8.702e-08, "d_bb.6": 1.352e-07, "d_bb.7": 7.188e-08, "d_bb.8": 1.067e-07, "d_w": 2.249e-07,
        "d_style_w.0": 3.823e-07, "d_style_b.0": 2.939e-07, "d_style_w.1": 4.647e-07, "d_style_b.1": 2.787e-07,
        "d_style_w.2": 3.162e-07, "d_style_b.2": 3.241e-07, "d_z": 4.142e-07,
    },
    "grown@1": {
        "w": 1.013e-06, "gamma": 1.018e-05, "beta": 1.953e-07, "d_gw.0": 2.448e-07, "d_gw.1": 2.409e-07,
        "d_gw.2": 2.303e-07, "d_gw.3": 2.342e-07, "d_gw.4": 2.340e-07, "d_gw.5": 2.441e-07, "d_gw.6": 2.370e-07,
        "d_gw.7": 2.284e-07, "d_gw.8": 2.379e-07, "d_gb.0": 3.607e-08, "d_gb.1": 5.074e-08, "d_gb.2": 3.790e-08,
        "d_gb.3": 4.845e-08, "d_gb.4": 4.304e-08, "d_gb.5": 2.906e-08, "d_gb.6": 3.463e-08, "d_gb.7": 4.954e-08,
        "d_gb.8": 4.212e-08, "d_bw.0": 2.456e-07, "d_bw.1": 2.379e-07, "d_bw.2": 2.417e-07, "d_bw.3": 2.421e-07,
        "d_bw.4": 2.430e-07, "d_bw.5": 2.384e-07, "d_bw.6": 2.461e-07, "d_bw.7": 2.379e-07, "d_bw.8": 2.443e-07,
        "d_bb.0": 0.000e+00, "d_bb.1": 0.000e+00, "d_bb.2": 0.000e+00, "d_bb.3": 0.000e+00, "d_bb.4": 0.000e+00,
        "d_bb.5": 0.000e+00, "d_bb.6": 0.000e+00, "d_bb.7": 0.000e+00, "d_bb.8": 0.000e+00, "d_w": 2.074e-07,
        "d_style_w.0": 2.322e-07, "d_style_b.0": 2.375e-07, "d_style_w.1": 2.615e-07, "d_style_b.1": 2.287e-07,
        "d_style_w.2": 2.118e-07, "d_style_b.2": 2.093e-07, "d_z": 6.897e-07,
    },
    "grown@3": {
        "w": 2.374e-06, "gamma": 1.133e-05, "beta": 1.994e-07,
    },
    "grown@33": {
        "w": 2.436e-06, "gamma": 1.670e-05, "beta": 2.795e-07, "d_gw.0": 3.691e-07, "d_gw.1": 3.918e-07,
        "d_gw.2": 2.568e-07, "d_gw.3": 4.063e-07, "d_gw.4": 2.909e-07, "d_gw.5": 2.750e-07, "d_gw.6": 2.164e-07,
        "d_gw.7": 2.515e-07, "d_gw.8": 2.065e-07, "d_gb.0": 1.135e-07, "d_gb.1": 9.665e-08, "d_gb.2": 1.073e-07,
        "d_gb.3": 1.357e-07, "d_gb.4": 1.131e-07, "d_gb.5": 7.336e-08, "d_gb.6": 7.750e-08, "d_gb.7": 9.569e-08,
        "d_gb.8": 1.032e-07, "d_bw.0": 2.813e-07, "d_bw.1": 2.710e-07, "d_bw.2": 2.895e-07, "d_bw.3": 2.918e-07,
        "d_bw.4": 2.676e-07, "d_bw.5": 3.266e-07, "d_bw.6": 2.448e-07, "d_bw.7": 2.164e-07, "d_bw.8": 2.383e-07,
        "d_bb.0": 9.982e-08, "d_bb.1": 9.007e-08, "d_bb.2": 1.055e-07, "d_bb.3": 9.027e-08, "d_bb.4": 7.846e-08,
        "d_bb.5": 9.865e-08, "d_bb.6": 1.013e-07, "d_bb.7": 8.631e-08, "d_bb.8": 9.623e-08, "d_w": 2.646e-07,
        "d_style_w.0": 3.995e-07, "d_style_b.0": 2.939e-07, "d_style_w.1": 2.740e-07, "d_style_b.1": 3.397e-07,
        "d_style_w.2": 2.665e-07, "d_style_b.2": 1.978e-07, "d_z": 3.706e-07,
    },
    "init@1": {
        "w": 6.561e-07, "gamma": 5.331e-06, "beta": 6.725e-08, "d_gw.0": 1.808e-07, "d_gw.1": 1.743e-07,
        "d_gw.2": 1.644e-07, "d_gw.3": 1.662e-07, "d_gw.4": 1.699e-07, "d_gw.5": 1.720e-07, "d_gw.6": 1.726e-07,
        "d_gw.7": 1.788e-07, "d_gw.8": 1.621e-07, "d_gb.0": 4.459e-08, "d_gb.1": 4.395e-08, "d_gb.2": 3.155e-08,
        "d_gb.3": 4.784e-08, "d_gb.4": 3.745e-08, "d_gb.5": 3.164e-08, "d_gb.6": 4.340e-08, "d_gb.7": 2.164e-08,
        "d_gb.8": 5.008e-08, "d_bw.0": 1.685e-07, "d_bw.1": 1.712e-07, "d_bw.2": 1.573e-07, "d_bw.3": 1.724e-07,
        "d_bw.4": 1.599e-07, "d_bw.5": 1.676e-07, "d_bw.6": 1.671e-07, "d_bw.7": 1.650e-07, "d_bw.8": 1.733e-07,
        "d_bb.0": 0.000e+00, "d_bb.1": 0.000e+00, "d_bb.2": 0.000e+00, "d_bb.3": 0.000e+00, "d_bb.4": 0.000e+00,
        "d_bb.5": 0.000e+00, "d_bb.6": 0.000e+00, "d_bb.7": 0.000e+00, "d_bb.8": 0.000e+00, "d_w": 2.243e-07,
        "d_style_w.0": 1.095e-07, "d_style_b.0": 1.080e-07, "d_style_w.1": 2.541e-07, "d_style_b.1": 2.551e-07,
        "d_style_w.2": 2.348e-07, "d_style_b.2": 2.243e-07, "d_z": 2.906e-07,
    },
    "init@3": {
        "w": 9.416e-07, "gamma": 6.283e-06, "beta": 9.636e-08,
    },
    "init@33": {
        "w": 1.596e-06, "gamma": 7.817e-06, "beta": 1.157e-07, "d_gw.0": 2.335e-07, "d_gw.1": 2.483e-07,
        "d_gw.2": 2.618e-07, "d_gw.3": 2.057e-07, "d_gw.4": 2.113e-07, "d_gw.5": 3.115e-07, "d_gw.6": 2.236e-07,
        "d_gw.7": 1.984e-07, "d_gw.8": 2.164e-07, "d_gb.0": 1.071e-07, "d_gb.1": 8.613e-08, "d_gb.2": 1.257e-07,
        "d_gb.3": 1.197e-07, "d_gb.4": 9.083e-08, "d_gb.5": 1.577e-07, "d_gb.6": 1.014e-07, "d_gb.7": 6.887e-08,
        "d_gb.8": 1.112e-07, "d_bw.0": 1.760e-07, "d_bw.1": 2.605e-07, "d_bw.2": 2.890e-07, "d_bw.3": 2.299e-07,
        "d_bw.4": 1.587e-07, "d_bw.5": 2.600e-07, "d_bw.6": 2.447e-07, "d_bw.7": 2.142e-07, "d_bw.8": 2.773e-07,
        "d_bb.0": 6.680e-08, "d_bb.1": 1.093e-07, "d_bb.2": 9.811e-08, "d_bb.3": 7.921e-08, "d_bb.4": 7.703e-08,
        "d_bb.5": 1.034e-07, "d_bb.6": 8.680e-08, "d_bb.7": 1.137e-07, "d_bb.8": 1.028e-07, "d_w": 2.129e-07,
        "d_style_w.0": 3.622e-07, "d_style_b.0": 3.481e-07, "d_style_w.1": 3.906e-07, "d_style_b.1": 3.487e-07,
        "d_style_w.2": 3.407e-07, "d_style_b.2": 3.051e-07, "d_z": 4.620e-07,
    },
    "layer_range@1": {
        "w": 5.731e-07, "gamma": 4.145e-06, "beta": 8.905e-08, "d_gw.0": 1.819e-07, "d_gw.1": 2.032e-07,
        "d_gw.2": 1.734e-07, "d_gw.3": 1.733e-07, "d_gw.4": 1.734e-07, "d_gw.5": 0.000e+00, "d_gw.6": 1.627e-09,
        "d_gw.7": 1.693e-10, "d_gw.8": 1.646e-11, "d_gb.0": 2.661e-08, "d_gb.1": 3.425e-08, "d_gb.2": 2.451e-08,
        "d_gb.3": 2.481e-08, "d_gb.4": 1.304e-08, "d_gb.5": 0.000e+00, "d_gb.6": 1.746e-10, "d_gb.7": 1.455e-11,
        "d_gb.8": 1.592e-12, "d_bw.0": 1.733e-07, "d_bw.1": 1.737e-07, "d_bw.2": 1.734e-07, "d_bw.3": 2.213e-08,
        "d_bw.4": 2.834e-09, "d_bw.5": 0.000e+00, "d_bw.6": 2.001e-11, "d_bw.7": 2.507e-12, "d_bw.8": 2.780e-13,
        "d_bb.0": 0.000e+00, "d_bb.1": 0.000e+00, "d_bb.2": 0.000e+00, "d_bb.3": 0.000e+00, "d_bb.4": 0.000e+00,
        "d_bb.5": 0.000e+00, "d_bb.6": 0.000e+00, "d_bb.7": 0.000e+00, "d_bb.8": 0.000e+00, "d_w": 2.856e-07,
        "d_style_w.0": 4.990e-07, "d_style_b.0": 5.080e-07, "d_style_w.1": 3.803e-07, "d_style_b.1": 3.315e-07,
        "d_style_w.2": 4.218e-07, "d_style_b.2": 4.242e-07, "d_z": 3.794e-07,
    },
    "layer_range@33": {
        "w": 1.234e-06, "gamma": 8.148e-06, "beta": 1.071e-07, "d_gw.0": 2.596e-07, "d_gw.1": 3.347e-07,
        "d_gw.2": 2.431e-07, "d_gw.3": 2.750e-07, "d_gw.4": 1.964e-07, "d_gw.5": 0.000e+00, "d_gw.6": 1.084e-08,
        "d_gw.7": 1.096e-09, "d_gw.8": 1.094e-10, "d_gb.0": 1.119e-07, "d_gb.1": 1.477e-07, "d_gb.2": 8.020e-08,
        "d_gb.3": 1.591e-07, "d_gb.4": 8.708e-08, "d_gb.5": 0.000e+00, "d_gb.6": 3.339e-09, "d_gb.7": 1.897e-10,
        "d_gb.8": 2.174e-11, "d_bw.0": 2.638e-07, "d_bw.1": 2.408e-07, "d_bw.2": 2.201e-07, "d_bw.3": 1.732e-07,
        "d_bw.4": 2.040e-08, "d_bw.5": 0.000e+00, "d_bw.6": 1.815e-10, "d_bw.7": 1.810e-11, "d_bw.8": 2.192e-12,
        "d_bb.0": 1.159e-07, "d_bb.1": 9.572e-08, "d_bb.2": 1.060e-07, "d_bb.3": 4.361e-08, "d_bb.4": 4.629e-09,
        "d_bb.5": 0.000e+00, "d_bb.6": 6.108e-11, "d_bb.7": 4.036e-12, "d_bb.8": 4.823e-13, "d_w": 3.280e-07,
        "d_style_w.0": 3.421e-07, "d_style_b.0": 2.729e-07, "d_style_w.1": 3.242e-07, "d_style_b.1": 2.744e-07,
        "d_style_w.2": 3.833e-07, "d_style_b.2": 4.105e-07, "d_z": 4.080e-07,
    },
    "one_sided@1": {
        "w": 1.495e-06, "gamma": 1.858e-05, "beta": 3.221e-07, "d_gw.0": 1.226e-07, "d_gw.1": 1.256e-07,
        "d_gw.2": 1.314e-07, "d_gw.3": 1.165e-07, "d_gw.4": 9.637e-08, "d_gw.5": 1.236e-07, "d_gw.6": 1.307e-07,
        "d_gw.7": 1.177e-07, "d_gw.8": 9.337e-08, "d_gb.0": 3.794e-08, "d_gb.1": 3.759e-08, "d_gb.2": 3.793e-08,
        "d_gb.3": 4.026e-08, "d_gb.4": 3.186e-08, "d_gb.5": 4.235e-08, "d_gb.6": 4.801e-08, "d_gb.7": 4.963e-08,
        "d_gb.8": 2.044e-08, "d_bw.0": 1.195e-07, "d_bw.1": 1.026e-07, "d_bw.2": 9.398e-08, "d_bw.3": 7.929e-08,
        "d_bw.4": 8.671e-08, "d_bw.5": 9.650e-08, "d_bw.6": 8.563e-08, "d_bw.7": 1.099e-07, "d_bw.8": 1.099e-07,
        "d_bb.0": 0.000e+00, "d_bb.1": 0.000e+00, "d_bb.2": 0.000e+00, "d_bb.3": 0.000e+00, "d_bb.4": 0.000e+00,
        "d_bb.5": 0.000e+00, "d_bb.6": 0.000e+00, "d_bb.7": 0.000e+00, "d_bb.8": 0.000e+00, "d_w": 1.179e-07,
        "d_style_w.0": 2.478e-07, "d_style_b.0": 2.526e-07, "d_style_w.1": 2.344e-07, "d_style_b.1": 1.824e-07,
        "d_style_w.2": 1.581e-07, "d_style_b.2": 1.179e-07, "d_z": 3.133e-07,
    },
    "one_sided@3": {
        "w": 1.852e-06, "gamma": 1.750e-05, "beta": 3.390e-07,
    },
    "one_sided@33": {
        "w": 2.521e-06, "gamma": 2.293e-05, "beta": 3.293e-07, "d_gw.0": 1.915e-07, "d_gw.1": 2.407e-07,
        "d_gw.2": 1.727e-07, "d_gw.3": 1.471e-07, "d_gw.4": 2.498e-07, "d_gw.5": 1.811e-07, "d_gw.6": 2.013e-07,
        "d_gw.7": 2.268e-07, "d_gw.8": 2.315e-07, "d_gb.0": 1.045e-07, "d_gb.1": 1.079e-07, "d_gb.2": 7.133e-08,
        "d_gb.3": 7.961e-08, "d_gb.4": 1.260e-07, "d_gb.5": 9.697e-08, "d_gb.6": 1.370e-07, "d_gb.7": 1.039e-07,
        "d_gb.8": 9.989e-08, "d_bw.0": 2.332e-07, "d_bw.1": 1.468e-07, "d_bw.2": 2.362e-07, "d_bw.3": 1.605e-07,
        "d_bw.4": 1.920e-07, "d_bw.5": 2.132e-07, "d_bw.6": 1.616e-07, "d_bw.7": 1.895e-07, "d_bw.8": 1.510e-07,
        "d_bb.0": 1.117e-07, "d_bb.1": 8.053e-08, "d_bb.2": 9.281e-08, "d_bb.3": 1.102e-07, "d_bb.4": 1.404e-07,
        "d_bb.5": 8.330e-08, "d_bb.6": 1.253e-07, "d_bb.7": 1.175e-07, "d_bb.8": 7.775e-08, "d_w": 2.381e-07,
        "d_style_w.0": 3.362e-07, "d_style_b.0": 2.388e-07, "d_style_w.1": 6.082e-07, "d_style_b.1": 4.274e-07,
        "d_style_w.2": 2.688e-07, "d_style_b.2": 3.409e-07, "d_z": 4.258e-07,
    },
    "w_route@1": {
        "w": 0.000e+00, "gamma": 3.201e-06, "beta": 3.721e-08, "d_gw.0": 6.599e-08, "d_gw.1": 8.135e-08,
        "d_gw.2": 6.747e-08, "d_gw.3": 6.707e-08, "d_gw.4": 4.287e-08, "d_gw.5": 6.308e-08, "d_gw.6": 4.106e-08,
        "d_gw.7": 5.196e-08, "d_gw.8": 5.335e-08, "d_gb.0": 3.820e-08, "d_gb.1": 3.561e-08, "d_gb.2": 4.273e-08,
        "d_gb.3": 2.918e-08, "d_gb.4": 4.582e-08, "d_gb.5": 3.518e-08, "d_gb.6": 3.159e-08, "d_gb.7": 3.727e-08,
        "d_gb.8": 2.783e-08, "d_bw.0": 2.827e-08, "d_bw.1": 2.906e-08, "d_bw.2": 3.922e-08, "d_bw.3": 3.918e-08,
        "d_bw.4": 3.878e-08, "d_bw.5": 3.976e-08, "d_bw.6": 3.487e-08, "d_bw.7": 5.065e-08, "d_bw.8": 2.656e-08,
        "d_bb.0": 0.000e+00, "d_bb.1": 0.000e+00, "d_bb.2": 0.000e+00, "d_bb.3": 0.000e+00, "d_bb.4": 0.000e+00,
        "d_bb.5": 0.000e+00, "d_bb.6": 0.000e+00, "d_bb.7": 0.000e+00, "d_bb.8": 0.000e+00, "d_w": 2.488e-07,
    },
    "w_route@3": {
        "w": 0.000e+00, "gamma": 4.959e-06, "beta": 4.593e-08,
    },
    "w_route@33": {
        "w": 0.000e+00, "gamma": 5.903e-06, "beta": 5.397e-08, "d_gw.0": 1.232e-07, "d_gw.1": 9.483e-08,
        "d_gw.2": 2.120e-07, "d_gw.3": 1.429e-07, "d_gw.4": 2.024e-07, "d_gw.5": 2.064e-07, "d_gw.6": 1.397e-07,
        "d_gw.7": 1.777e-07, "d_gw.8": 1.385e-07, "d_gb.0": 1.412e-07, "d_gb.1": 7.040e-08, "d_gb.2": 1.115e-07,
        "d_gb.3": 1.146e-07, "d_gb.4": 1.176e-07, "d_gb.5": 1.177e-07, "d_gb.6": 1.739e-07, "d_gb.7": 9.120e-08,
        "d_gb.8": 7.267e-08, "d_bw.0": 2.364e-07, "d_bw.1": 1.595e-07, "d_bw.2": 1.381e-07, "d_bw.3": 1.077e-07,
        "d_bw.4": 1.545e-07, "d_bw.5": 1.402e-07, "d_bw.6": 1.282e-07, "d_bw.7": 2.083e-07, "d_bw.8": 1.711e-07,
        "d_bb.0": 8.865e-08, "d_bb.1": 9.088e-08, "d_bb.2": 1.160e-07, "d_bb.3": 6.716e-08, "d_bb.4": 1.470e-07,
        "d_bb.5": 1.609e-07, "d_bb.6": 1.144e-07, "d_bb.7": 1.154e-07, "d_bb.8": 9.470e-08, "d_w": 2.758e-07,
    },
    "colour/init@165": {
        "rgb": 6.076e-08, "d_feat": 7.990e-09, "d_normals": 6.807e-09, "d_gamma": 3.878e-09, "d_beta": 4.016e-08,
        "d_wv": 5.836e-07, "d_bv": 4.059e-07, "d_wrgb": 6.727e-07, "d_brgb": 7.135e-07,
    },
    "colour/trained_rgb@165": {
        "rgb": 4.693e-07, "d_feat": 3.181e-07, "d_normals": 2.348e-07, "d_gamma": 5.573e-08, "d_beta": 5.057e-07,
        "d_wv": 6.776e-07, "d_bv": 6.516e-07, "d_wrgb": 6.152e-07, "d_brgb": 4.557e-07,
    },
    "colour/saturated@165": {
        "rgb": 1.068e-13, "d_feat": 4.515e-15, "d_normals": 4.280e-15, "d_gamma": 1.618e-15, "d_beta": 2.153e-14,
        "d_wv": 3.643e-12, "d_bv": 1.213e-12, "d_wrgb": 3.841e-12, "d_brgb": 3.054e-12,
    },
    "colour/gamma_spread@165": {
        "rgb": 4.797e-07, "d_feat": 2.651e-07, "d_normals": 1.949e-07, "d_gamma": 5.713e-08, "d_beta": 4.019e-07,
        "d_wv": 9.896e-07, "d_bv": 3.035e-07, "d_wrgb": 6.964e-07, "d_brgb": 1.078e-06,
    },
    "colour/steep_normals@165": {
        "rgb": 4.387e-07, "d_feat": 3.535e-07, "d_normals": 1.823e-07, "d_gamma": 8.869e-08, "d_beta": 5.169e-07,
        "d_wv": 6.169e-07, "d_bv": 4.362e-07, "d_wrgb": 1.033e-06, "d_brgb": 6.638e-07,
    },
    "colour/quiet_element@165": {
        "rgb": 3.950e-07, "d_feat": 3.387e-07, "d_normals": 1.667e-07, "d_gamma": 8.238e-08, "d_beta": 6.742e-07,
        "d_wv": 5.712e-07, "d_bv": 6.617e-07, "d_wrgb": 6.737e-07, "d_brgb": 6.924e-07,
    },
    "colour/trained_rgb@1": {
        "rgb": 1.762e-07, "d_feat": 5.120e-08, "d_normals": 2.651e-08, "d_gamma": 5.069e-09, "d_beta": 2.600e-08,
        "d_wv": 4.648e-07, "d_bv": 4.577e-07, "d_wrgb": 1.190e-07, "d_brgb": 4.713e-08,
    },
    "colour/trained_rgb@16": {
        "rgb": 4.225e-07, "d_feat": 2.277e-07, "d_normals": 1.288e-07, "d_gamma": 2.510e-08, "d_beta": 2.448e-07,
        "d_wv": 4.315e-07, "d_bv": 3.989e-07, "d_wrgb": 6.126e-07, "d_brgb": 2.136e-07,
    },
    "colour/trained_rgb@17": {
        "rgb": 4.064e-07, "d_feat": 1.908e-07, "d_normals": 9.236e-08, "d_gamma": 1.527e-08, "d_beta": 1.625e-07,
        "d_wv": 7.305e-07, "d_bv": 3.347e-07, "d_wrgb": 5.054e-07, "d_brgb": 2.357e-07,
    },
    "colour/trained_rgb@31": {
        "rgb": 4.063e-07, "d_feat": 1.886e-07, "d_normals": 1.563e-07, "d_gamma": 2.780e-08, "d_beta": 3.651e-07,
        "d_wv": 4.149e-07, "d_bv": 3.447e-07, "d_wrgb": 4.379e-07, "d_brgb": 4.297e-07,
    },
    "colour/trained_rgb@32": {
        "rgb": 3.560e-07, "d_feat": 5.489e-07, "d_normals": 2.761e-07, "d_gamma": 3.150e-08, "d_beta": 4.750e-07,
        "d_wv": 5.986e-07, "d_bv": 7.665e-07, "d_wrgb": 4.487e-07, "d_brgb": 3.710e-07,
    },
    "colour/trained_rgb@33": {
        "rgb": 4.010e-07, "d_feat": 2.207e-07, "d_normals": 1.405e-07, "d_gamma": 2.406e-08, "d_beta": 3.554e-07,
        "d_wv": 5.774e-07, "d_bv": 5.649e-07, "d_wrgb": 4.653e-07, "d_brgb": 4.045e-07,
    },
    "colour/trained_rgb@127": {
        "rgb": 3.790e-07, "d_feat": 2.714e-07, "d_normals": 1.820e-07, "d_gamma": 5.483e-08, "d_beta": 5.644e-07,
        "d_wv": 7.257e-07, "d_bv": 5.299e-07, "d_wrgb": 4.764e-07, "d_brgb": 1.414e-06,
    },
    "colour/trained_rgb@129": {
        "rgb": 6.876e-07, "d_feat": 3.395e-07, "d_normals": 1.636e-07, "d_gamma": 6.287e-08, "d_beta": 5.243e-07,
        "d_wv": 4.164e-07, "d_bv": 5.831e-07, "d_wrgb": 4.794e-07, "d_brgb": 1.036e-06,
    },
    "colour/trained_rgb@152": {
        "rgb": 4.672e-07, "d_feat": 3.295e-07, "d_normals": 2.521e-07, "d_gamma": 6.783e-08, "d_beta": 5.383e-07,
        "d_wv": 8.263e-07, "d_bv": 4.863e-07, "d_wrgb": 6.414e-07, "d_brgb": 2.739e-07,
    },
    "colour/trained_rgb@513": {
        "rgb": 5.163e-07, "d_feat": 3.538e-07, "d_normals": 1.959e-07, "d_gamma": 1.219e-07, "d_beta": 5.025e-07,
        "d_wv": 4.322e-07, "d_bv": 5.513e-07, "d_wrgb": 7.898e-07, "d_brgb": 2.256e-06,
    },
    "colour/trained_rgb@66000": {
        "rgb": 8.684e-07, "d_feat": 5.786e-07, "d_normals": 3.758e-07, "d_gamma": 7.341e-07, "d_beta": 1.211e-05,
        "d_wv": 6.225e-07, "d_bv": 6.769e-07, "d_wrgb": 8.068e-07, "d_brgb": 1.169e-05,
    },
}
