"""The FiLM-SIREN MLP kernels (csrc/mlp.hip, mlp_fwd3.hip, mlp_bwd.hip) in the regimes a trained field reaches.  All plain
torch on the CPU, nothing of oi_amd:

* `cell(name)`: explicit tensors (w0, b0, wh[7], bh[7], wsig, bsig, wv, bv, wrgb, brgb, gamma[B][9][128], beta[B][9][128],
  pts[B n][3]) built from the committed golden weights by seeded, documented transforms; B = 2 and n = 165 per element (one
  full 128-point tile and a ragged 37), the two elements carry different gamma / beta.  gamma and beta are KERNEL INPUTS
  here (not the style net's outputs), so d_gamma and d_beta are compared directly.
* `restate(cell, dtype)`: oi_oracle.sdf_forward / color_head with gamma and beta as arguments -> sdf, feat, grad, rgb.
  Unmutated it is the oracle to 1e-12 in float64 and bit for bit in float32 (tests/test_mlp_regimes_cpu.py).  float64 is the
  reference and autograd through it the backward reference; float32 is the reference's own arithmetic noise.
* `floor_model(cell, seed)`: a float32 restatement that carries the two error sources the kernels legitimately have: every
  sine and cosine is off by a seeded uniform +-2.5e-7 (the bound tests/test_gpu_kernels.py::test_device_sincos_accuracy holds
  the device to for |x| <= 100; 3e-7 in the cell whose phases exceed that), and the phase is formed the kernels' way, in
  revolutions: A = gamma / 2 pi, B = (gamma b + beta) / 2 pi, one fma, one frac (csrc/f3_blob.h).
* `FP32_FLOOR[cell][tensor]`: the worst of plain float32 and four seeds of `floor_model`, measured on one thread and
  committed; `bar` = 3 x that (tests/conftest.py: "<= 3x the native-fp32 error").  Every cell's gain was tuned on the CPU
  until its bars stay at or below the project's existing bar of the tensor (PROJECT_BAR): the regimes test is never looser
  than the tests it joins.
* `emulate(cell, mutate)`: the f16x3 number format in torch -- image scales, fp16 limbs, three products, phases in
  revolutions, and the reverse sweep of mlp_fwd3.hip with its a-priori power-of-two scales -- and `MUTATIONS`: one wrong
  line each.  `CAUGHT_BY` names the cells that expose each mutation at 3 x bar (rehearsed on the CPU).

What the arithmetic allows, and what the cells do about it
----------------------------------------------------------
End to end the network amplifies error by the product of its FiLM gains: gamma ~ 60 everywhere puts the float32 floor of sdf
at 2e-5 (the project's bar), hidden weights x 2 at 1.1e-5.  A cell that stresses one layer therefore keeps the others at
ordinary gain, the gains the issue's sketch started from were lowered where the floor demanded it (GROWN, WIDE_BETA below), and
every cell's bar is checked against PROJECT_BAR on the CPU.
Power-of-two rescaling (`distinct_scales`: W_l, b_l x 2^j, gamma_l x 2^-j) leaves every float32 product, the scaled fp16
image, G = gamma 2^-k, A and B unchanged bit for bit -- but it makes the eight image scales, H_BOUND x max|G| and F3_GMAX of
neighbouring layers differ by up to 2^14, so that a kernel, blob writer or backward that reads a neighbour's entry is off by
orders of magnitude instead of by nothing (at the golden weights the scales take two values and the bounds lie within 15 %).
The a-priori bound of the reverse sweep, U = H_BOUND x max|G| x measured max|V|, is met when W >= 0, V is constant and
cos(phi) = 1 (`bound_met`), and overstated by 2^7 for every row but one in `loose_bound`; an outlier weight sets the image
scale alone and pushes every other weight's lo limb towards the fp16 subnormals (`quiet_outlier@r`: at r = 1e4 the ordinary
weights sit at 2^-13 of the maximum, hi limb ~1, lo limb subnormal; the error this leaves is 1.2e-7 in the emulation).
An adjoint that is exactly 0 (`dead_layer`: gamma_4 = 0) has no exponent to normalise by: the kernels clamp (`eb < 14`).
The same cell found a fault next to that clamp: the a-priori scale of V_4 is taken from max|G_4| = 0, pow2_for answered
2^126, the accumulator times 2^126 overflowed and inf x (G cos = 0) made d sdf/dx (and with it rgb and every gradient of the
backward) NaN for the whole element; mutation `scale_of_zero_bound` keeps that line rehearsed.
The phase in revolutions is reduced by one exact v_fract; `wide_phase` drives 16 rows of layer 7 to +-41 revolutions, where
float32 holds the phase to 3.8e-6 revolutions only: those rows are judged as their own tensor (`feat_wide`) with their own
floor, and their weight in sdf / rgb is 1e-3 so that the other tensors keep ordinary bars.
"""
import functools
import math
import os
import zlib

import numpy as np
import torch

import oi_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
B, N_PER, C = 2, 165, 128
PARAMS = ("w0", "b0", "wh", "bh", "wsig", "bsig", "wv", "bv", "wrgb", "brgb")
LEAVES = PARAMS + ("gamma", "beta")
FWD_TENSORS = ("sdf", "feat", "grad", "rgb")
INV_2PI = 0.15915494309189533577

BAR_MIN_BACKWARD = 4 * 2.0 ** -23
# the project's existing bars (tests/test_gpu_kernels.py::test_sdf_mlp_golden, tests/test_gpu_backward.py)
PROJECT_BAR = {"sdf": 2e-5, "grad": 1e-4, "rgb": 2e-5, "feat": 1e-4, "feat_wide": 1e-4, "backward": 2e-5}

CELLS = ("init", "distinct_scales", "grown", "gamma_spread", "loose_bound", "bound_met", "quiet_outlier@1e4",
         "quiet_outlier@1e6", "dead_layer", "far_points", "wide_phase")
# Backward cells.  `bound_met` is not one: cos(phi_7) = 1 to 1e-4 needs |phi_7| <= 0.014, so a_8 = sin(phi_7) ~ 1e-3, and the
# 2.5e-7 ABSOLUTE error the device's sine is allowed is 2.5e-4 of it: the float32 floor of d wsig is 6.5e-4 and of d wv 1.6e-4
# (the f16x3 backward measured 2.8e-4 and 2.6e-4 on the MI355X, inside that floor), thirty times the project's 2e-5.  No gain
# of the cell changes that, so by the floor condition the cell leaves the backward set; its forward and d sdf/dx stay.
BWD_CELLS = ("init", "distinct_scales", "gamma_spread", "loose_bound", "dead_layer", "quiet_outlier@1e4")
J_SCALES = (-3, 5, -1, 8, 0, 2, -6)     # distinct_scales: layers 1..7
J_COLOUR = 4
PINNED = ((3, 0.0), (17, 3e-3), (40, -7e-3), (77, -12.0), (101, 1e-4), (127, 0.0))   # gamma_spread rows (feature, gamma)
SPREAD_LAYERS = (0, 1, 4, 7, 8)
# gamma_spread: with [-20, 80] in all five layers float32 autograd is 2.1e-5 off in d_beta of layer 0 (and > 2e-5 / 3 in 18 more
# backward tensors): above the project's bar.  Layer 0 and the colour head keep [-20, 80], the hidden layers 1, 4, 7 get half
# of it; every backward floor is then below 2e-5 / 3 (forward: feat 8e-6).
SPREAD_HALVED = (1, 4, 7)
OUTLIER_LAYERS = (1, 3, 6)
WIDE_ROWS = tuple(range(5, 128, 8))     # 16 rows of layer 7
DEAD_LAYER = 4
FAR = 3.0            # far_points: |x| <= 3 keeps the floor condition (feat 2.6e-5 against 3.3e-5)
GROWN = 1.35         # grown: hidden weights x 1.5 put the float32 floor of feat at 5.4e-5 (> 1e-4 / 3), x 1.35 at 3.1e-5
WIDE_BETA = 256.0    # wide_phase: +-300 rad put the floor of the wide rows at 3.9e-5; 256 rad = 40.7 revolutions at 3.3e-5


def _seed(name):
    return zlib.crc32(name.encode())


def _golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return {k: torch.from_numpy(np.asarray(f[k])) for k in f.files}


@functools.lru_cache(maxsize=None)
def golden_sds():
    return _golden("weights_sdf"), _golden("weights_color")


def _base(name, pscale=1.0):
    """Golden weights, gamma / beta of two seeded latents (oi_oracle.film_params), points uniform in [-pscale, pscale]^3."""
    sd, csd = golden_sds()
    g = torch.Generator().manual_seed(_seed(name))
    w = O.style_mlp(sd, torch.randn(B, 64, generator=g))
    gb = [O.film_params(sd, f"pts_linears.{l}.", w) for l in range(8)] + [O.film_params(csd, "views_linears.", w)]
    c = {"w0": sd["pts_linears.0.weight"].clone(), "b0": sd["pts_linears.0.bias"].clone(),
         "wh": torch.stack([sd[f"pts_linears.{l}.weight"] for l in range(1, 8)]),
         "bh": torch.stack([sd[f"pts_linears.{l}.bias"] for l in range(1, 8)]),
         "wsig": sd["sigma_linear.weight"].reshape(-1).clone(), "bsig": sd["sigma_linear.bias"].reshape(-1).clone(),
         "wv": csd["views_linears.weight"].clone(), "bv": csd["views_linears.bias"].clone(),
         "wrgb": csd["rgb_linear.weight"].clone(), "brgb": csd["rgb_linear.bias"].clone(),
         "gamma": torch.stack([x[0] for x in gb], 1).contiguous(), "beta": torch.stack([x[1] for x in gb], 1).contiguous(),
         "pts": (torch.rand(B * N_PER, 3, generator=g) * 2.0 - 1.0) * pscale, "w": w, "name": name, "cot": name}
    return c, g


def _build(name):
    if name == "init":
        return _base("init")[0]
    if name == "distinct_scales":
        c = _base("init")[0]                       # the SAME function as `init`, rescaled by powers of two
        c["name"] = name
        for l, j in zip(range(1, 8), J_SCALES):
            c["wh"][l - 1] *= 2.0 ** j
            c["bh"][l - 1] *= 2.0 ** j
            c["gamma"][:, l] *= 2.0 ** -j
        c["wv"] *= 2.0 ** J_COLOUR
        c["bv"] *= 2.0 ** J_COLOUR
        c["gamma"][:, 8] *= 2.0 ** -J_COLOUR
        return c
    if name == "grown":
        c, _ = _base(name, pscale=1.2)
        c["wh"] *= GROWN
        return c
    if name == "gamma_spread":
        c, g = _base(name)
        for l in SPREAD_LAYERS:
            # the spread of test_mlp_backward_gamma_through_zero: gamma over about [-20, 80] ...
            c["gamma"][:, l] = c["gamma"][:, l] + 24.0 * torch.randn(B, C, generator=g)
            c["gamma"][:, l].clamp_(-20.0, 80.0)
            if l in SPREAD_HALVED:
                c["gamma"][:, l] *= 0.5            # ... over [-10, 40] in the hidden layers (floor condition, see SPREAD_HALVED)
            for f, target in PINNED:               # ... and the pinned rows: exactly 0, |gamma| < 1e-2, negative
                c["gamma"][:, l, f] = target
        return c
    if name == "loose_bound":
        c, _ = _base(name)
        for l in range(1, 7):
            f = 11 + 13 * l
            c["wh"][l - 1][f] = 0.0
            c["bh"][l - 1][f] = 0.0
            c["gamma"][:, l, f] = 2.0 ** 7 * c["gamma"][:, l].abs().median(-1).values
        return c
    if name == "bound_met":
        c, _ = _base(name)
        c["wh"][6] = c["wh"][6].abs()
        c["bh"][6] = 0.0
        c["gamma"][:, 7] = 0.01
        c["beta"][:, 7] = 0.0
        c["wsig"][:] = c["wsig"].abs().mean()
        return c
    if name.startswith("quiet_outlier@"):
        r = float(name.split("@")[1])
        c, _ = _base(name)
        for l in OUTLIER_LAYERS:
            c["wh"][l - 1][5][7] = r * c["wh"][l - 1].abs().median()
            c["gamma"][:, l, 5] = 1e-3 / r
        return c
    if name == "dead_layer":
        c, _ = _base(name)
        c["gamma"][0, DEAD_LAYER] = 0.0
        return c
    if name == "far_points":
        c, _ = _base(name, pscale=FAR)
        c["pts"][7] = 0.0                          # x = 0 exactly
        c["pts"][300:304] = c["pts"][300].clone()  # four coincident points (second element, its ragged tile)
        return c
    if name == "wide_phase":
        c, g = _base(name)
        rows = list(WIDE_ROWS)
        c["beta"][:, 7, rows] = (torch.rand(B, len(rows), generator=g) * 2.0 - 1.0) * WIDE_BETA
        c["beta"][0, 7, rows[0]], c["beta"][1, 7, rows[1]] = WIDE_BETA, -WIDE_BETA
        c["wsig"][rows] *= 1e-3
        c["wv"][:, rows] *= 1e-3
        return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cell(name):
    """The cell's tensors (float32), built once, shared, never modified."""
    return _build(name)


def cotangents(name):
    """(cs, cg, cr) of the backward loss <cs, sdf> + <cg, grad> + <cr, rgb> (tests/test_gpu_backward.py)."""
    g = torch.Generator().manual_seed(_seed(cell(name)["cot"] + "/cotangents"))   # (distinct_scales: init's)
    n = B * N_PER
    return torch.randn(n, generator=g), 0.1 * torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _pp(v):
    return v.repeat_interleave(N_PER, dim=0)     # as O._per_point


def _weight(t, l):
    return t["w0"] if l == 0 else t["wh"][l - 1]


def _bias(t, l):
    return t["b0"] if l == 0 else t["bh"][l - 1]


def restate(c, dtype=torch.float64, leaves=False):
    """-> dict(sdf (n,), feat (n,128), grad (n,3), rgb (n,3)[, leaves]).  O.sdf_forward(want_grad=True) and O.color_head with
    gamma / beta as arguments; leaves=True: every tensor of LEAVES requires grad (returned under "leaves")."""
    t = {k: c[k].to(dtype) for k in LEAVES + ("pts",)}
    if leaves:
        t = {k: (v.clone().requires_grad_(True) if k in LEAVES else v) for k, v in t.items()}
    a = t["pts"]
    cs = []
    for l in range(8):
        g, b = _pp(t["gamma"][:, l]), _pp(t["beta"][:, l])
        u = a @ _weight(t, l).t() + _bias(t, l)
        phi = g * u + b
        a = torch.sin(phi)
        cs.append(g * torch.cos(phi))
    wsig = t["wsig"].view(1, C)
    sdf = a @ wsig.t() + t["bsig"]
    gvec = wsig.expand(a.shape[0], -1)
    for l in reversed(range(8)):
        gvec = (gvec * cs[l]) @ _weight(t, l)
    g, b = _pp(t["gamma"][:, 8]), _pp(t["beta"][:, 8])
    u = torch.cat([a, gvec], -1) @ t["wv"].t() + t["bv"]
    rgb = torch.sigmoid(torch.sin(g * u + b) @ t["wrgb"].t() + t["brgb"])
    out = {"sdf": sdf.squeeze(-1), "feat": a, "grad": gvec, "rgb": rgb}
    if leaves:
        out["leaves"] = {k: t[k] for k in LEAVES}
    return out


def backward_names():
    return ["w0", "b0"] + [f"wh.{l}" for l in range(1, 8)] + [f"bh.{l}" for l in range(1, 8)] + \
        ["wsig", "bsig", "wv", "bv", "wrgb", "brgb"] + [f"gamma.{l}" for l in range(9)] + [f"beta.{l}" for l in range(9)]


def split_grads(g):
    """{leaf: gradient} -> {tensor name of backward_names(): gradient}: hidden layers and FiLM layers one by one (rel_err is
    relative to the tensor's largest entry: a stacked tensor would hide its small layers)."""
    out = {k: g[k] for k in ("w0", "b0", "wsig", "bsig", "wv", "bv", "wrgb", "brgb")}
    for l in range(1, 8):
        out[f"wh.{l}"], out[f"bh.{l}"] = g["wh"][l - 1], g["bh"][l - 1]
    for l in range(9):
        out[f"gamma.{l}"], out[f"beta.{l}"] = g["gamma"][:, l], g["beta"][:, l]
    return out


def loss_of(out, cot):
    cs, cg, cr = (x.to(out["sdf"].dtype) for x in cot)
    return (out["sdf"] * cs).sum() + (out["grad"] * cg).sum() + (out["rgb"] * cr).sum()


def backward_of(fn, c, **kw):
    """Autograd of the backward loss through `fn` (restate / floor_model) -> {name: gradient}."""
    out = fn(c, leaves=True, **kw)
    names = list(LEAVES)
    gr = torch.autograd.grad(loss_of(out, cotangents(c["name"])), [out["leaves"][k] for k in names])
    return split_grads(dict(zip(names, gr)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 restatement of the cell, computed once and shared."""
    with torch.no_grad():
        return {k: v for k, v in restate(cell(name), torch.float64).items()}


@functools.lru_cache(maxsize=None)
def reference_backward(name):
    return backward_of(restate, cell(name), dtype=torch.float64)


# ----------------------------------------------------------------------------------------------------------------------
# the floor model
# ----------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c_):
    """float32 fma: one rounding (through float64: the product of two float32 is exact there)."""
    return (a.double() * b.double() + c_.double()).float()


def trig_eps(name):
    return 3e-7 if name == "wide_phase" else 2.5e-7


def _frac(x):
    return x - torch.floor(x)


def floor_model(c, seed=0, leaves=False):
    """float32 restatement with the kernels' legitimate error sources (module docstring) -> as `restate`."""
    gen = torch.Generator().manual_seed(_seed(c["name"]) ^ (0x9E3779B1 * (seed + 1) & 0x7FFFFFFF))
    eps = trig_eps(c["name"])
    t = {k: c[k].float() for k in LEAVES + ("pts",)}
    if leaves:
        t = {k: (v.clone().requires_grad_(True) if k in LEAVES else v) for k, v in t.items()}
    noise = lambda ref: (torch.rand(ref.shape, generator=gen) * 2.0 - 1.0) * eps

    def film(l, u, gam, bet, bias):
        A = _pp(gam) * INV_2PI
        Bv = _pp(_fma(gam, bias.expand_as(gam), bet) * INV_2PI)
        r = _frac(_fma(A, u, Bv))
        ang = r.double() * (2.0 * math.pi)
        return (torch.sin(ang).float() + noise(r)), (torch.cos(ang).float() + noise(r))

    a = t["pts"]
    cs = []
    for l in range(8):
        sn, co = film(l, a @ _weight(t, l).t(), t["gamma"][:, l], t["beta"][:, l], _bias(t, l))
        a = sn
        cs.append(_pp(t["gamma"][:, l]) * co)
    wsig = t["wsig"].view(1, C)
    sdf = a @ wsig.t() + t["bsig"]
    gvec = wsig.expand(a.shape[0], -1)
    for l in reversed(range(8)):
        gvec = (gvec * cs[l]) @ _weight(t, l)
    h, _ = film(8, torch.cat([a, gvec], -1) @ t["wv"].t(), t["gamma"][:, 8], t["beta"][:, 8], t["bv"])
    rgb = torch.sigmoid(h @ t["wrgb"].t() + t["brgb"])
    out = {"sdf": sdf.squeeze(-1), "feat": a, "grad": gvec, "rgb": rgb}
    if leaves:
        out["leaves"] = {k: t[k] for k in LEAVES}
    return out


# ----------------------------------------------------------------------------------------------------------------------
# errors, floors, bars
# ----------------------------------------------------------------------------------------------------------------------
def tensors_of(name):
    return FWD_TENSORS + (("feat_wide",) if name == "wide_phase" else ())


def _maxabs(a, b):
    a = a.detach().double().cpu()
    if not bool(torch.isfinite(a).all()):
        return math.inf
    return float((a - b).abs().max()) if a.numel() else 0.0


def errors(name, cand):
    """{tensor: error} of a candidate's forward outputs (any subset of sdf, feat, grad, rgb) against the float64 restatement,
    in the project's measures: max |.| for sdf, feat, rgb; max |.| / max(1, max |grad|) for grad.  A non-finite output: inf."""
    ref = reference(name)
    out = {}
    for k in FWD_TENSORS:
        if cand.get(k) is None:
            continue
        a, b = cand[k], ref[k]
        if k == "feat" and name == "wide_phase":
            rows = list(WIDE_ROWS)
            rest = [f for f in range(C) if f not in rows]
            out["feat_wide"] = _maxabs(a[:, rows], b[:, rows])
            a, b = a[:, rest], b[:, rest]
        e = _maxabs(a, b)
        out[k] = e / max(1.0, float(ref["grad"].abs().max())) if k == "grad" else e
    return out


def rel_err(a, b):
    """tests/test_gpu_backward.py's measure; a reference of exactly 0 admits exactly 0 (-> 0.0, anything else inf)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if not bool(torch.isfinite(a).all()):
        return math.inf
    m = float(b.abs().max())
    if m == 0.0:
        return 0.0 if float(a.abs().max()) == 0.0 else math.inf
    return float((a - b).abs().max() / m)


def backward_errors(name, grads):
    ref = reference_backward(name)
    return {k: rel_err(grads[k], ref[k]) for k in backward_names() if k in grads}


def measure_floor(name, backward=None):
    """{tensor: worst error of plain float32 and four seeds of floor_model}; on one thread (the order of torch's sums must
    not depend on the machine).  Backward tensors (cells of BWD_CELLS) are prefixed "d."."""
    c = cell(name)
    backward = (name in BWD_CELLS) if backward is None else backward
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            runs = [restate(c, torch.float32)] + [floor_model(c, s) for s in range(4)]
        worst = {}
        for r in runs:
            for k, e in errors(name, r).items():
                worst[k] = max(worst.get(k, 0.0), e)
        if backward:
            bruns = [backward_of(restate, c, dtype=torch.float32)] + [backward_of(floor_model, c, seed=s) for s in range(4)]
            for r in bruns:
                for k, e in backward_errors(name, r).items():
                    worst["d." + k] = max(worst.get("d." + k, 0.0), e)
            for k, e in _summation_order_errors(name).items():
                worst["d." + k] = max(worst["d." + k], e)
    finally:
        torch.set_num_threads(nt)
    return worst


def _summation_order_errors(name):
    """d bsig and d brgb are plain sums over the 330 points of one float32 term each (cs; cr rgb (1 - rgb)), |sum| ~ 15 out of
    sum |.| ~ 260.  torch's CPU sum is pairwise and lands within 1e-8 of the float64 value by luck of its order; the kernels add
    in an order of their own (a wave tree, then atomics between workgroups, which differs from run to run).  The third legitimate
    error source of the backward is therefore the ORDER of a float32 sum: the worst of four seeded permutations summed one
    term after the other, the least favourable order a kernel could take."""
    ref = reference(name)
    cs, _, cr = cotangents(name)
    terms = {"bsig": cs.double()[:, None], "brgb": cr.double() * ref["rgb"] * (1.0 - ref["rgb"])}
    g = torch.Generator().manual_seed(_seed(name + "/summation order"))
    out = {}
    for k, t in terms.items():
        exact = t.sum(0)
        worst = 0.0
        for _ in range(4):
            # (numpy: its float32 cumsum rounds every partial sum to float32; torch's accumulates in double on the CPU)
            seq = np.cumsum(t.float()[torch.randperm(t.shape[0], generator=g)].numpy(), axis=0, dtype=np.float32)[-1]
            worst = max(worst, float((torch.from_numpy(seq).double() - exact).abs().max() / exact.abs().max()))
        out[k] = worst
    return out


def project_bar(tensor):
    return PROJECT_BAR["backward"] if tensor.startswith("d.") else PROJECT_BAR[tensor]


def bar(name, tensor):
    """3 x the committed float32 floor; the pairs of AT_PROJECT_BAR are judged at the project's existing bar."""
    if (name, tensor) in AT_PROJECT_BAR:
        return project_bar(tensor)
    b = 3.0 * FP32_FLOOR[name][tensor]
    if not tensor.startswith("d."):
        return b
    # backward tensors.  Capped at the project's 2e-5: float32 autograd of the floor model is up to 9e-6 off at the golden
    # weights (`init`: d b0, d beta_0, d gamma_0..2), which no gain of a cell can change, and the bar must never be looser
    # than before.  Floored at 4 ulp of float32 relative to the tensor's largest entry (a bar below the format's own step is
    # luck of an order of summation; see also _summation_order_errors).
    return max(min(b, PROJECT_BAR["backward"]), BAR_MIN_BACKWARD)


# ----------------------------------------------------------------------------------------------------------------------
# the f16x3 number format
# ----------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("no_image_scale", "neighbour_scale", "neighbour_bound", "neighbour_gmax", "drop_w_lo", "drop_a_lo", "bias_not_in_B",
             "adjoint_fixed_scale", "bound_is_max_not_rowsum", "zero_adjoint_nan", "no_fract", "scale_of_zero_bound")


def _limbs(v):
    """float32 -> (hi, lo) fp16 limbs as float64; an overflow is inf, as .half() makes it."""
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double(), lo.double()


def _image_scale(w, mutate):
    """(2^k, 2^-k) with max |w| 2^k in [2^13, 2^14) (csrc/mlp.hip image_scale; the exponent field is clamped at 14)."""
    if mutate == "no_image_scale":
        return 1.0, 1.0
    mx = float(w.abs().max())
    e = max(math.frexp(mx)[1] - 1, 14 - 127) if mx > 0 else 14 - 127
    return 2.0 ** (13 - e), 2.0 ** (e - 13)


def _pow2_for(U, mutate):
    """U (n,) float32 -> sg (n,) with U sg in [2^14, 2^15) (csrc/mlp_fwd3.hip pow2_for; exponent field clamped to [64, 253]:
    sg multiplies the accumulator, <= 2^37, BEFORE G cos does, so a bound of 0 -- max|G| = 0, a dead layer -- must not give
    2^126.  `scale_of_zero_bound` is the clamp at 15 the kernel shipped with: acc sg = inf, inf x 0 = NaN)."""
    if mutate == "zero_adjoint_nan":
        return torch.exp2(14.0 - torch.floor(torch.log2(U.double()))).float()     # log2(0) = -inf -> sg = inf
    _, e = torch.frexp(U)
    lo = 15 if mutate == "scale_of_zero_bound" else 64
    eb = (e - 1 + 127).clamp(lo, 253)
    eb = torch.where(U == 0, torch.full_like(eb, lo), eb)
    return torch.ldexp(torch.ones_like(U), 141 - eb)


def _prod3(xh, xl, wh_, wl_, mutate):
    """x (n, K) limbs times image (M, K) limbs: the three products, accumulated in float64, rounded to float32."""
    acc = xh @ wh_.t()
    if mutate != "drop_a_lo":
        acc = acc + xl @ wh_.t()
    if mutate != "drop_w_lo":
        acc = acc + xh @ wl_.t()
    return acc.float()


def _sin_rev(phi, mutate, cos=False):
    """sin / cos of a phase in revolutions (float32) by one v_fract and the hardware sine: exact, rounded to float32."""
    if mutate == "no_fract":
        arg = phi.double()
        arg = torch.where(arg.abs() > 32.0, arg * (1.0 + 2e-5), arg)   # the unreduced argument loses 2e-5 beyond +-32
    else:
        arg = _frac(phi).double()
    ang = arg * (2.0 * math.pi)
    return (torch.cos(ang) if cos else torch.sin(ang)).float()


@torch.no_grad()
def emulate(c, mutate=None):
    """The f16x3 forward (grad + rgb + feat) and the reverse sweep for d sdf/dx -> as `restate`, float32."""
    assert mutate is None or mutate in MUTATIONS, mutate
    t = {k: c[k].float() for k in LEAVES + ("pts",)}
    n = t["pts"].shape[0]
    # images: m = l - 1 for layers 1..7, 8 = colour
    mats = [t["wh"][l - 1] for l in range(1, 8)] + [t["wv"][:, :C]]
    sc = [_image_scale(w, mutate) for w in mats]
    img = [_limbs(w * s) for w, (s, _) in zip(mats, sc)]
    scaled = [w * s for w, (s, _) in zip(mats, sc)]
    inv = [1.0] + [sc[m][1] for m in range(8)]            # inv[l] = 2^-k of layer l's image (layer 0: 1)
    if mutate == "neighbour_scale":                       # 2^-k of image m + 1 (the header entry behind the right one)
        inv = [1.0] + [sc[m + 1][1] if m < 6 else sc[0][1] if m == 6 else sc[7][1] for m in range(8)]
    # H_BOUND of the 16 images: largest absolute row sum (0..6 forward, 7..13 transposed, 14 colour, 15 colour transposed)
    rs = (lambda w: w.abs().max()) if mutate == "bound_is_max_not_rowsum" else (lambda w: w.abs().double().sum(1).max().float())
    bound = [rs(scaled[m]) for m in range(7)] + [rs(scaled[m].t()) for m in range(7)] + [rs(scaled[7]), rs(scaled[7].t())]
    G = [_pp(t["gamma"][:, l]) * inv[l] for l in range(9)]
    gmax = [_pp(t["gamma"][:, l].abs().max(-1, keepdim=True).values * inv[l])[:, 0] for l in range(9)]
    A = [g * INV_2PI for g in G]

    def Bof(l, bias):
        gam, bet = t["gamma"][:, l], t["beta"][:, l]
        if mutate == "bias_not_in_B":
            return _pp(bet * INV_2PI)
        return _pp(_fma(gam, bias.expand_as(gam), bet) * INV_2PI)

    # forward
    phase = []
    u = t["pts"] @ t["w0"].t()
    phi = _fma(A[0], u, Bof(0, t["b0"]))
    phase.append(phi)
    a = _sin_rev(phi, mutate)
    for l in range(1, 8):
        ah, al = _limbs(a)
        acc = _prod3(ah, al, *img[l - 1], mutate)
        phi = _fma(A[l], acc, Bof(l, t["bh"][l - 1]))
        phase.append(phi)
        a = _sin_rev(phi, mutate)
    feat = a
    sdf = (feat.double() @ t["wsig"].double() + t["bsig"].double()).float()
    # reverse sweep
    g9 = G[7] * t["wsig"]
    gmax9 = _pp((t["gamma"][:, 7] * inv[7] * t["wsig"]).abs().max(-1, keepdim=True).values)[:, 0]
    sg = _pow2_for(gmax9 * 2.0, mutate)
    run = 1.0 / sg.double()
    V = (g9 * _sin_rev(phase[7], mutate, cos=True)) * sg[:, None]
    for l in range(7, 0, -1):
        m = torch.ones(n) if mutate == "adjoint_fixed_scale" else V.abs().max(-1).values
        vh, vl = _limbs(V)
        acc = _prod3(vh, vl, img[l - 1][0].t(), img[l - 1][1].t(), mutate)
        bnd = bound[6 + l + (1 if mutate == "neighbour_bound" else 0)]
        gm = gmax[l if mutate == "neighbour_gmax" else l - 1]
        sg = _pow2_for(m * (bnd * gm), mutate)
        run = run / sg.double()
        V = (acc * sg[:, None]) * (G[l - 1] * _sin_rev(phase[l - 1], mutate, cos=True))
    grad = ((V.double() @ t["w0"].double()) * run[:, None]).float()
    # colour head: features through image 14, the gradient's three columns on the VALU, brought to the image's scale
    fh, fl = _limbs(feat)
    acc = _prod3(fh, fl, *img[7], mutate)
    d = (grad.double() @ t["wv"][:, C:].double().t()).float()
    u = acc + d * sc[7][0]
    h = _sin_rev(_fma(A[8], u, Bof(8, t["bv"])), mutate)
    rgb = torch.sigmoid((h.double() @ t["wrgb"].double().t() + t["brgb"].double()).float())
    return {"sdf": sdf, "feat": feat, "grad": grad, "rgb": rgb}


# Mutations no cell can expose at 3 x bar, with the arithmetic reason.
NOT_DETECTABLE = {}

# Which cells catch which mutation (the mutated emulation judged as the GPU output is, some tensor's error >= 3 x bar):
# tests/test_mlp_regimes_cpu.py::test_mutation_is_caught demands every entry.
CAUGHT_BY = {
    # layers rescaled by 2^-6 and 2^-3 put the unscaled lo limb deep into the fp16 subnormals (init: 3.7 x bar only)
    "no_image_scale": ("distinct_scales",),
    "neighbour_scale": ("init", "distinct_scales", "grown", "loose_bound", "quiet_outlier@1e4"),
    # H_BOUND of a scaled image is (row sum / max) 2^13.x: ~60 x 2^13 for ordinary weights, ~2^13 where an outlier is the
    # maximum -- the only cells where a neighbour's entry is wrong by more than the 3.5 bits of slack (fp16 overflow -> inf)
    "neighbour_bound": ("quiet_outlier@1e4", "quiet_outlier@1e6"),
    # max|G| differs between neighbours by 2^7 (loose_bound: layers 6 | 7), by 3000 (bound_met: gamma_7 = 0.01) or by r
    "neighbour_gmax": ("loose_bound", "bound_met", "quiet_outlier@1e4", "quiet_outlier@1e6"),
    "drop_w_lo": ("init", "distinct_scales", "grown", "gamma_spread", "quiet_outlier@1e4", "far_points", "wide_phase"),
    "drop_a_lo": ("init", "distinct_scales", "grown", "gamma_spread", "quiet_outlier@1e4", "far_points", "wide_phase"),
    "bias_not_in_B": ("init", "distinct_scales", "gamma_spread", "bound_met"),
    "adjoint_fixed_scale": ("init", "distinct_scales", "loose_bound", "bound_met"),
    "bound_is_max_not_rowsum": ("init", "bound_met", "loose_bound"),
    "zero_adjoint_nan": ("dead_layer",),
    "scale_of_zero_bound": ("dead_layer",),
    "no_fract": ("wide_phase",),
}

# (cell, tensor) pairs judged at the project's existing bar: {(cell, tensor): (measured error, reason)}
AT_PROJECT_BAR = {}

# Measured by `measure_floor` (torch CPU, one thread); tests/test_mlp_regimes_cpu.py keeps a fresh measurement within 1.5x.
FP32_FLOOR = {
    "init": {
        "sdf": 2.560e-07, "feat": 6.899e-06, "grad": 6.923e-06, "rgb": 8.516e-08, "d.w0": 2.526e-06,
        "d.b0": 8.678e-06, "d.wh.1": 3.680e-06, "d.wh.2": 3.283e-06, "d.wh.3": 4.168e-06, "d.wh.4": 4.276e-06,
        "d.wh.5": 3.574e-06, "d.wh.6": 4.080e-06, "d.wh.7": 2.393e-06, "d.bh.1": 5.293e-06, "d.bh.2": 2.597e-06,
        "d.bh.3": 2.820e-06, "d.bh.4": 5.107e-06, "d.bh.5": 2.923e-06, "d.bh.6": 2.955e-06, "d.bh.7": 1.903e-06,
        "d.wsig": 1.756e-06, "d.bsig": 4.201e-07, "d.wv": 1.971e-06, "d.bv": 1.516e-06, "d.wrgb": 1.314e-06,
        "d.brgb": 5.112e-07, "d.gamma.0": 6.850e-06, "d.gamma.1": 7.358e-06, "d.gamma.2": 7.234e-06, "d.gamma.3": 4.734e-06,
        "d.gamma.4": 6.196e-06, "d.gamma.5": 4.718e-06, "d.gamma.6": 4.287e-06, "d.gamma.7": 2.729e-06, "d.gamma.8": 1.330e-06,
        "d.beta.0": 8.942e-06, "d.beta.1": 3.405e-06, "d.beta.2": 4.410e-06, "d.beta.3": 3.688e-06, "d.beta.4": 3.937e-06,
        "d.beta.5": 3.941e-06, "d.beta.6": 2.815e-06, "d.beta.7": 2.820e-06, "d.beta.8": 1.310e-06,
    },
    "distinct_scales": {
        "sdf": 2.355e-07, "feat": 5.895e-06, "grad": 4.372e-06, "rgb": 8.516e-08, "d.w0": 3.799e-06,
        "d.b0": 8.156e-06, "d.wh.1": 3.581e-06, "d.wh.2": 3.295e-06, "d.wh.3": 3.439e-06, "d.wh.4": 3.619e-06,
        "d.wh.5": 4.022e-06, "d.wh.6": 4.041e-06, "d.wh.7": 2.210e-06, "d.bh.1": 4.059e-06, "d.bh.2": 2.797e-06,
        "d.bh.3": 2.472e-06, "d.bh.4": 4.134e-06, "d.bh.5": 3.557e-06, "d.bh.6": 2.828e-06, "d.bh.7": 1.750e-06,
        "d.wsig": 2.054e-06, "d.bsig": 2.515e-07, "d.wv": 2.142e-06, "d.bv": 1.835e-06, "d.wrgb": 1.750e-06,
        "d.brgb": 1.267e-07, "d.gamma.0": 7.319e-06, "d.gamma.1": 5.660e-06, "d.gamma.2": 5.708e-06, "d.gamma.3": 3.075e-06,
        "d.gamma.4": 5.732e-06, "d.gamma.5": 4.829e-06, "d.gamma.6": 4.829e-06, "d.gamma.7": 3.626e-06, "d.gamma.8": 2.009e-06,
        "d.beta.0": 8.651e-06, "d.beta.1": 2.914e-06, "d.beta.2": 3.384e-06, "d.beta.3": 3.754e-06, "d.beta.4": 3.331e-06,
        "d.beta.5": 3.652e-06, "d.beta.6": 2.704e-06, "d.beta.7": 2.319e-06, "d.beta.8": 1.721e-06,
    },
    "grown": {
        "sdf": 2.363e-06, "feat": 3.090e-05, "grad": 6.208e-06, "rgb": 4.899e-07,
    },
    "gamma_spread": {
        "sdf": 3.945e-07, "feat": 8.174e-06, "grad": 2.176e-06, "rgb": 7.337e-08, "d.w0": 3.678e-06,
        "d.b0": 2.282e-06, "d.wh.1": 1.663e-06, "d.wh.2": 2.330e-06, "d.wh.3": 2.369e-06, "d.wh.4": 2.264e-06,
        "d.wh.5": 2.086e-06, "d.wh.6": 2.433e-06, "d.wh.7": 2.898e-06, "d.bh.1": 3.795e-06, "d.bh.2": 2.493e-06,
        "d.bh.3": 3.314e-06, "d.bh.4": 3.549e-06, "d.bh.5": 2.959e-06, "d.bh.6": 2.706e-06, "d.bh.7": 2.784e-06,
        "d.wsig": 2.603e-06, "d.bsig": 5.525e-06, "d.wv": 1.733e-06, "d.bv": 2.534e-06, "d.wrgb": 1.495e-06,
        "d.brgb": 6.182e-07, "d.gamma.0": 2.588e-06, "d.gamma.1": 3.433e-06, "d.gamma.2": 3.023e-06, "d.gamma.3": 3.243e-06,
        "d.gamma.4": 2.304e-06, "d.gamma.5": 3.789e-06, "d.gamma.6": 5.570e-06, "d.gamma.7": 1.880e-06, "d.gamma.8": 1.119e-06,
        "d.beta.0": 3.017e-06, "d.beta.1": 3.695e-06, "d.beta.2": 2.443e-06, "d.beta.3": 3.194e-06, "d.beta.4": 3.532e-06,
        "d.beta.5": 2.224e-06, "d.beta.6": 3.263e-06, "d.beta.7": 2.444e-06, "d.beta.8": 1.673e-06,
    },
    "loose_bound": {
        "sdf": 2.501e-07, "feat": 6.477e-06, "grad": 3.011e-06, "rgb": 1.061e-07, "d.w0": 5.984e-06,
        "d.b0": 5.543e-06, "d.wh.1": 3.404e-06, "d.wh.2": 2.655e-06, "d.wh.3": 4.087e-06, "d.wh.4": 3.867e-06,
        "d.wh.5": 2.764e-06, "d.wh.6": 3.124e-06, "d.wh.7": 2.570e-06, "d.bh.1": 5.242e-06, "d.bh.2": 2.277e-06,
        "d.bh.3": 3.657e-06, "d.bh.4": 5.408e-06, "d.bh.5": 2.920e-06, "d.bh.6": 4.747e-06, "d.bh.7": 2.017e-06,
        "d.wsig": 2.786e-06, "d.bsig": 7.848e-07, "d.wv": 1.942e-06, "d.bv": 1.586e-06, "d.wrgb": 1.578e-06,
        "d.brgb": 8.988e-07, "d.gamma.0": 3.410e-06, "d.gamma.1": 5.520e-06, "d.gamma.2": 4.287e-06, "d.gamma.3": 3.397e-06,
        "d.gamma.4": 4.989e-06, "d.gamma.5": 3.261e-06, "d.gamma.6": 2.795e-06, "d.gamma.7": 2.203e-06, "d.gamma.8": 1.293e-06,
        "d.beta.0": 4.360e-06, "d.beta.1": 4.954e-06, "d.beta.2": 3.890e-06, "d.beta.3": 3.802e-06, "d.beta.4": 3.666e-06,
        "d.beta.5": 2.929e-06, "d.beta.6": 4.522e-06, "d.beta.7": 2.506e-06, "d.beta.8": 1.465e-06,
    },
    "bound_met": {
        "sdf": 6.495e-08, "feat": 4.364e-07, "grad": 2.114e-08, "rgb": 6.223e-08,
    },
    "quiet_outlier@1e4": {
        "sdf": 2.656e-07, "feat": 6.490e-06, "grad": 4.196e-06, "rgb": 9.206e-08, "d.w0": 7.828e-06,
        "d.b0": 7.874e-06, "d.wh.1": 4.674e-06, "d.wh.2": 6.585e-06, "d.wh.3": 5.007e-06, "d.wh.4": 3.582e-06,
        "d.wh.5": 4.137e-06, "d.wh.6": 3.960e-06, "d.wh.7": 2.445e-06, "d.bh.1": 4.844e-06, "d.bh.2": 5.472e-06,
        "d.bh.3": 4.717e-06, "d.bh.4": 3.522e-06, "d.bh.5": 4.772e-06, "d.bh.6": 2.373e-06, "d.bh.7": 2.484e-06,
        "d.wsig": 1.958e-06, "d.bsig": 2.964e-07, "d.wv": 1.942e-06, "d.bv": 8.023e-07, "d.wrgb": 1.558e-06,
        "d.brgb": 2.936e-07, "d.gamma.0": 3.581e-06, "d.gamma.1": 9.260e-06, "d.gamma.2": 3.533e-06, "d.gamma.3": 1.076e-05,
        "d.gamma.4": 3.659e-06, "d.gamma.5": 4.254e-06, "d.gamma.6": 1.918e-06, "d.gamma.7": 1.303e-06, "d.gamma.8": 1.231e-06,
        "d.beta.0": 6.202e-06, "d.beta.1": 3.898e-06, "d.beta.2": 4.840e-06, "d.beta.3": 3.959e-06, "d.beta.4": 3.609e-06,
        "d.beta.5": 4.020e-06, "d.beta.6": 2.838e-06, "d.beta.7": 2.883e-06, "d.beta.8": 1.058e-06,
    },
    "quiet_outlier@1e6": {
        "sdf": 2.316e-07, "feat": 6.401e-06, "grad": 2.067e-06, "rgb": 7.971e-08,
    },
    "dead_layer": {
        "sdf": 1.901e-07, "feat": 6.769e-06, "grad": 1.763e-06, "rgb": 7.696e-08, "d.w0": 6.396e-06,
        "d.b0": 5.742e-06, "d.wh.1": 4.884e-06, "d.wh.2": 3.111e-06, "d.wh.3": 4.143e-06, "d.wh.4": 3.778e-06,
        "d.wh.5": 3.877e-06, "d.wh.6": 3.336e-06, "d.wh.7": 3.866e-06, "d.bh.1": 4.041e-06, "d.bh.2": 4.066e-06,
        "d.bh.3": 4.366e-06, "d.bh.4": 3.429e-06, "d.bh.5": 3.327e-06, "d.bh.6": 3.697e-06, "d.bh.7": 2.771e-06,
        "d.wsig": 2.678e-06, "d.bsig": 6.477e-07, "d.wv": 1.109e-06, "d.bv": 1.498e-06, "d.wrgb": 1.614e-06,
        "d.brgb": 4.443e-07, "d.gamma.0": 3.524e-06, "d.gamma.1": 5.345e-06, "d.gamma.2": 3.708e-06, "d.gamma.3": 4.405e-06,
        "d.gamma.4": 1.743e-06, "d.gamma.5": 3.201e-06, "d.gamma.6": 3.066e-06, "d.gamma.7": 5.689e-06, "d.gamma.8": 2.158e-06,
        "d.beta.0": 5.917e-06, "d.beta.1": 4.378e-06, "d.beta.2": 3.847e-06, "d.beta.3": 5.644e-06, "d.beta.4": 4.012e-06,
        "d.beta.5": 4.590e-06, "d.beta.6": 4.094e-06, "d.beta.7": 3.126e-06, "d.beta.8": 1.405e-06,
    },
    "far_points": {
        "sdf": 3.915e-06, "feat": 2.573e-05, "grad": 1.578e-05, "rgb": 6.229e-07,
    },
    "wide_phase": {
        "sdf": 2.295e-07, "feat_wide": 3.215e-05, "feat": 6.767e-06, "grad": 2.031e-06, "rgb": 8.753e-08,
    },
}
