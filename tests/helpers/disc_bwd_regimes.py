"""The discriminator's backward kernels (csrc/disc_bwd.hip: oi_conv4x4_dgrad[_masked|_pre], oi_conv4x4_wgrad[_masked],
oi_conv4x4_bwd_pre, oi_lrelu_mask_mul) and their composition (oi_amd/autograd_conv.py) in the regimes of
tests/helpers/disc_regimes.py (`R`: its seeds, weights, images and chains are used as they are).  All plain torch on the CPU:

* `clean(name)`: the pool images without a kink-adjacent activation in any block (the rule of R._kink_keep: the float32 and
  the float64 chain disagree on a sign, or 0 < |u| < 3 x the layer's fp32 floor x rms).  D is per-sample, so a batch of clean
  images has every LeakyReLU on the same side in any arithmetic within the bar; a sum that is exactly 0 in both chains
  (`mask`: windows of zeros, the whole zero image) is ON the kink everywhere and stays in: the derivative there is the slope.
  `batch(name)`: the (real, fake) pool indices of the network cases, clean images only; `mask` has the zero image as a fake.
* layer cases (`layer_case`): one layer's backward on DATA -- x = the float32 chain's pre-activation below the layer (the
  image for block 0), ref = the layer's own pre-activation, w, and g = the gradient that a seeded cotangent on the logits
  leaves at the layer along the float32 chain (R.grad32).  `layer_outputs` states every quantity the GPU test takes from the
  kernels, in float64 (the reference) or in float32 with every bit defined (the floor):
      dgrad_m      conv_t(mask_ref(g), w)               ops.conv4x4_dgrad(mask_ref=ref, slope 0.2)
      dgrad_pre    conv_t(g, w) lrelu'(x)               ops.conv4x4_dgrad_pre(x_slope 0.2)
      wgrad_m      wgrad(mask_ref(g), x) [+acc]         ops.conv4x4_wgrad(mask_ref=ref, slope 0.2, acc)
      bwd_dx       = dgrad_pre,  bwd_gw  wgrad(g, lrelu(x)) [+acc]       ops.conv4x4_bwd(x_slope 0.2, acc)
  `acc`: a seeded non-zero tensor of the gradient's own rms that the kernel adds to.
* `dgrad_plan` / `wgrad_plan`: make_dgrad / make_wgrad of csrc/disc_bwd.hip restated: the K splits and the class of the
  epilogue they select ("k1" one plain store; "lds_store" four splits summed in LDS, plain store; "lds_atomic" a multiple
  of four above four, LDS sums then atomics; "atomic" anything else, atomics only).  `LAYER_ROUTES`: the smallest (network,
  layer, batch) that selects each class of either kernel, the stride-1 head and the ragged tails.
* network cases (`net_grads`): float64 autograd over the chain on `batch(name)` -- gw_plain d <c, D(x)> / dW for a seeded
  cotangent c on all logits (not BCE: its gradient is exactly zero where the logits saturate, `grown8`), gw_r1 dR1/dW with
  R1 = mean_b |d sum D(x)[:, 0] / dx|^2 (the double backward), step the gradient of BCE(real, 1) + BCE(fake, 0) + 10 R1(real).
* `err` = max |y - ref| / rms(ref) (R.err); `FP32_FLOOR_BWD`: the committed error of the float32 restatement (R.conv32,
  R.conv_t32, R.head_t32, `wgrad32`, `sigmoid32`: exact short sums, one rounding, a plain float32 loop over the long axis); bar = 3 x floor, the suite's rule (tests/conftest.py).  A reference whose rms is 0
  must be met exactly.  Nothing here is computed from a kernel's output.
* `MUTATIONS` / `CAUGHT_BY` / `NOT_DETECTABLE`: plausible kernel errors as mutations of the float64 restatement and the
  (regime, route) in which each exceeds 3 x bar (tests/test_disc_bwd_regimes_cpu.py rehearses it).
"""
import functools

import torch
import torch.nn.functional as F

from helpers import disc_regimes as R

SLOPE = R.SLOPE
REG_W = 10.0
MIN_CLEAN = 3
NAMES = R.NET64 + ("unit_128", "default_init_128")
CLASSES = ("k1", "lds_store", "lds_atomic", "atomic")
LAYER_KEYS = ("dgrad_m", "dgrad_pre", "wgrad_m", "wgrad_m+acc", "bwd_dx", "bwd_gw", "bwd_gw+acc")
NET_KEYS = ("gw_plain", "gw_r1", "step")

MUTATIONS = ("mask_ge", "pre_dropped", "pre_per_split", "no_x_slope", "drop_tail", "acc_overwritten", "mask_twice",
             "fake_in_r1", "slope_001")


# ----------------------------------------------------------------------------------------------------------------------
# clean images
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kink_adjacent(name):
    """Per pool image: the number of kink-adjacent activations over all blocks."""
    c = R.case(name)
    n = torch.zeros(c["x"].shape[0], dtype=torch.long)
    for u64, u32 in zip(c["u64"][:-1], c["u32"][:-1]):
        s = R.rms(u64)
        near = (torch.sign(u64) != torch.sign(u32.double())) | ((u64.abs() < 3 * R.err(u32, u64, s) * s) & (u64 != 0))
        n += near.flatten(1).sum(1)
    return tuple(int(v) for v in n)


def clean(name):
    return tuple(i for i, n in enumerate(kink_adjacent(name)) if n == 0)


def batch(name):
    """(real, fake) pool indices of the network cases: clean images only (at least MIN_CLEAN of a pool of six; the single
    image of a 128 x 128 regime serves as both)."""
    cl = clean(name)
    P = R.case(name)["x"].shape[0]
    assert len(cl) >= min(MIN_CLEAN, P), (name, cl)
    if P == 1:
        return (0,), (0,)
    if name == "mask":
        nz = [i for i in cl if i != R.MASK_ZERO_IMAGE]
        assert R.MASK_ZERO_IMAGE in cl and len(nz) >= 2
        return (nz[0], nz[1]), (R.MASK_ZERO_IMAGE, nz[2 % len(nz)])
    return (cl[0], cl[1]), (cl[2], cl[3 % len(cl)])


# ----------------------------------------------------------------------------------------------------------------------
# the launch plans (csrc/disc_bwd.hip: make_dgrad, make_wgrad)
# ----------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def split_class(k):
    return "k1" if k == 1 else "lds_store" if k == 4 else "lds_atomic" if k % 4 == 0 else "atomic"


def dgrad_plan(B, Cin, H, Cout, stride, pad):
    """make_dgrad restated -> k_splits, its class, the output channels per split, the pixels of a parity class."""
    Hc = _cdiv(H, stride)
    Mc = B * Hc * Hc
    tiles = stride * stride * _cdiv(Mc, 32) * _cdiv(Cin, 32)
    k = 1
    while tiles * k < 2048 and Cout // (k * 2) >= 16:
        k *= 2
    cps = _cdiv(Cout, k)
    cps += cps & 1
    k = _cdiv(Cout, cps)
    return dict(k_splits=k, cls=split_class(k), per_split=cps, Mc=Mc, Hc=Hc, trip=8 if stride == 2 else 4)


def wgrad_plan(B, Cin, H, Cout, stride, pad):
    """make_wgrad restated -> k_splits, its class, the pixels per split, the pixels in all."""
    Ho = (H + 2 * pad - 4) // stride + 1
    P = B * Ho * Ho
    tiles = _cdiv(Cout, 32) * _cdiv(Cin, 2)
    k = 1
    while tiles * k < 2048 and P // (k * 2) >= 64:
        k *= 2
    pps = (_cdiv(P, k) + 7) & ~7
    k = _cdiv(P, pps)
    return dict(k_splits=k, cls=split_class(k), per_split=pps, P=P, trip=16)


def layer_shape(spec, layer):
    """(Cin, H, Cout, stride, pad) of layer `layer` (the last one: the head) of the regime's network."""
    ch = (spec["in_dim"],) + R.CH[spec["size"]]
    if layer == len(ch) - 1:
        return ch[-1], 4, spec["out_dim"], 1, 0
    return ch[layer], spec["size"] >> layer, ch[layer + 1], 2, 1


# route -> network, layer (4: the head of the 64 x 64 network), batch, and what the plans must say there: (k_splits, class) of
# the data-gradient and of the weight-gradient kernel.  `first`: the classes this route is the smallest to select.
LAYER_ROUTES = {
    "b2_B1": dict(size=64, layer=2, B=1, dgrad=(16, "lds_atomic"), wgrad=(1, "k1"), first=("wgrad:k1",)),
    "b1_B1": dict(size=64, layer=1, B=1, dgrad=(8, "lds_atomic"), wgrad=(4, "lds_store"), first=("wgrad:lds_store", "dgrad:lds_atomic")),
    "b0_B1": dict(size=64, layer=0, B=1, dgrad=(4, "lds_store"), wgrad=(16, "lds_atomic"), first=("wgrad:lds_atomic", "dgrad:lds_store")),
    "b2_B2": dict(size=64, layer=2, B=2, dgrad=(16, "lds_atomic"), wgrad=(2, "atomic"), first=("wgrad:atomic",)),
    "head_B1": dict(size=64, layer=4, B=1, dgrad=(1, "k1"), wgrad=(1, "k1"), first=("dgrad:k1",)),
    "b3_B1": dict(size=64, layer=3, B=1, dgrad=(32, "lds_atomic"), wgrad=(1, "k1"), first=()),
    "b3_B3": dict(size=64, layer=3, B=3, dgrad=(32, "lds_atomic"), wgrad=(1, "k1"), first=()),    # 48 pixels per parity class: 1 1/2 tiles
    "head_B3": dict(size=64, layer=4, B=3, dgrad=(1, "k1"), wgrad=(1, "k1"), first=()),           # 3 of 16 K-steps, Cout 7 (1) of 32 rows
    "b0_128_B1": dict(size=128, layer=0, B=1, dgrad=(2, "atomic"), wgrad=(64, "lds_atomic"), first=("dgrad:atomic",)),
}
LAYER_IMAGES = {"mask": (0, R.MASK_ZERO_IMAGE, 1)}   # (the zero image is the second of a batch of three)


def routes_of(name):
    size = R.REGIMES[name]["size"]
    return tuple(r for r, v in LAYER_ROUTES.items() if v["size"] == size)


def plans(name, route):
    r = LAYER_ROUTES[route]
    sh = layer_shape(R.REGIMES[name], r["layer"])
    return dgrad_plan(r["B"], *sh), wgrad_plan(r["B"], *sh)


# ----------------------------------------------------------------------------------------------------------------------
# one layer: float64 and defined-bit float32
# ----------------------------------------------------------------------------------------------------------------------
def dgrad64(g, w, stride, pad):
    return F.conv_transpose2d(g, w, stride=stride, padding=pad)


def wgrad64(g, x, stride, pad):
    return torch.nn.grad.conv2d_weight(x, (g.shape[1], x.shape[1], 4, 4), g, stride=stride, padding=pad)


def dgrad32(g, w, stride, pad):
    return R.conv_t32(g, w) if stride == 2 else R.head_t32(g.reshape(g.shape[0], -1), w)


def wgrad32(g, x, stride, pad):
    """The weight gradient with every bit defined.  An element has no short axis to sum exactly (R.conv32 has its 16 taps):
    it is one sum over the output pixels of all images.  So every product is rounded once (the float32 product of two float32
    values is their exact product rounded) and the pixels are added in a plain float32 loop, in order -- multiply and add as
    two operations, never fused."""
    B, Cin = x.shape[:2]
    Cout, Ho, Wo = g.shape[1:]
    cols = F.unfold(x.float(), 4, padding=pad, stride=stride)   # (B, Cin * 16, Ho * Wo): copies, no arithmetic
    gf = g.float().reshape(B, Cout, Ho * Wo)
    acc = torch.zeros(Cout, Cin * 16)
    for b in range(B):
        for p in range(Ho * Wo):
            acc.add_(gf[b, :, p, None] * cols[b, None, :, p])
    return acc.view(Cout, Cin, 4, 4)


def _lmask(ref, slope, ge=False):
    one = torch.ones((), dtype=ref.dtype)
    return torch.where((ref >= 0) if ge else (ref > 0), one, torch.full((), slope, dtype=ref.dtype))


def _drop_tail(g, dp, wp, stride):
    """`drop_tail`: what the kernels would compute without their last K split (k_splits > 1) or without the ragged end of
    their only one -> (g for the data gradient, g for the weight gradient, keep mask of the data gradient's pixels)."""
    B, Cout, Ho, Wo = g.shape
    gd, gw = g.clone(), g.clone()
    n_cut = (dp["k_splits"] - 1) * dp["per_split"] if dp["k_splits"] > 1 else Cout - Cout % dp["trip"]
    gd[:, n_cut:] = 0
    P = wp["P"]
    p_cut = (wp["k_splits"] - 1) * wp["per_split"] if wp["k_splits"] > 1 else P - P % wp["trip"]
    flat = gw.permute(0, 2, 3, 1).reshape(P, Cout).clone()
    flat[p_cut:] = 0
    gw = flat.view(B, Ho, Wo, Cout).permute(0, 3, 1, 2).contiguous()
    Hc = dp["Hc"]
    H = Hc * stride if stride == 2 else Hc
    iy = torch.arange(H)
    m = ((torch.arange(B).view(B, 1, 1) * Hc + (iy // stride).view(1, H, 1)) * Hc + (iy // stride).view(1, 1, H))
    keep = (m < dp["Mc"] - dp["Mc"] % 32).view(B, 1, H, H)
    return gd, gw, keep


def layer_outputs(o, f32=False, mutate=None, dp=None, wp=None):
    """{key: tensor} of LAYER_KEYS from the operands `o` (x, ref, w, g, acc, stride, pad): float64 expressions of exactly
    these float32 operands, or (`f32`) the float32 restatement.  `mutate`: a deliberately wrong float64 restatement."""
    assert mutate is None or (mutate in MUTATIONS and not f32)
    dt = torch.float32 if f32 else torch.float64
    x, ref, w, g = (o[k].to(dt) for k in ("x", "ref", "w", "g"))
    stride, pad = o["stride"], o["pad"]
    sl = 0.01 if mutate == "slope_001" else SLOPE
    ge = mutate == "mask_ge"
    dg, wg = (dgrad32, wgrad32) if f32 else (dgrad64, wgrad64)
    g_d = g_w = g
    keep = None
    if mutate == "drop_tail":
        g_d, g_w, keep = _drop_tail(g, dp, wp, stride)
    mr = _lmask(ref, sl, ge)
    if mutate == "mask_twice":
        mr = mr * mr
    mx = _lmask(x, sl, ge)
    if mutate == "pre_dropped":
        mx = torch.ones_like(mx)
    elif mutate == "pre_per_split":
        mx = mx ** dp["k_splits"]
    ax = x if mutate == "no_x_slope" else torch.where(x > 0, x, x * sl)
    out = {"dgrad_m": dg(g_d * mr, w, stride, pad), "dgrad_pre": dg(g_d, w, stride, pad) * mx,
           "wgrad_m": wg(g_w * mr, x, stride, pad), "bwd_gw": wg(g_w, ax, stride, pad)}
    if keep is not None:
        out["dgrad_m"], out["dgrad_pre"] = out["dgrad_m"] * keep, out["dgrad_pre"] * keep
    out["bwd_dx"] = out["dgrad_pre"]
    if "acc" in o:
        for k in ("wgrad_m", "bwd_gw"):
            out[k + "+acc"] = out[k] if mutate == "acc_overwritten" else o["acc"][k].to(dt) + out[k]
    return out


def layer_images(name):
    P = R.case(name)["x"].shape[0]
    return tuple(LAYER_IMAGES.get(name, (0, 1, 2)))[:min(3, P)]


@functools.lru_cache(maxsize=None)
def _layer_grads(name):
    """The gradient at every layer's pre-activation of the images `layer_images(name)`, float32 chain, seeded cotangent."""
    c = R.case(name)
    idx = list(layer_images(name))
    cot = torch.randn(len(idx), c["spec"]["out_dim"], generator=torch.Generator().manual_seed(c["spec"]["seed"] * 13 + 5))
    return R.grad32(c["wsd"], [u[idx] for u in c["u32"]], cot, per_layer=True)


@functools.lru_cache(maxsize=None)
def layer_case(name, route):
    """The operands of one layer case (fp32: x, ref, w, g, acc {key: prefill}, stride, pad), its float64 references `refs`
    and their rms `scale`.  Built once, shared, never modified."""
    r, c = LAYER_ROUTES[route], R.case(name)
    l, B = r["layer"], r["B"]
    idx = list(layer_images(name)[:B])
    assert len(idx) == B
    w, stride, pad = R._layers(c["wsd"])[l]
    o = dict(x=(c["x"] if l == 0 else c["u32"][l - 1])[idx].contiguous(), ref=c["u32"][l][idx].contiguous(), w=w,
             g=_layer_grads(name)[l][:B].contiguous(), stride=stride, pad=pad)
    refs = layer_outputs(o)
    base = torch.randn(w.shape, generator=torch.Generator().manual_seed(c["spec"]["seed"] * 17 + l))
    o["acc"] = {k: (base * (R.rms(refs[k]) or 1.0)).float() for k in ("wgrad_m", "bwd_gw")}
    refs.update({k + "+acc": o["acc"][k].double() + refs[k] for k in o["acc"]})
    return dict(o=o, refs=refs, scale={k: R.rms(v) for k, v in refs.items()})


def layer_mask_mul(name, route):
    """oi_lrelu_mask_mul on the case's data: (v, ref, expected) -- exact: one fp32 product per element."""
    o = layer_case(name, route)["o"]
    return o["g"], o["ref"], torch.where(o["ref"] > 0, o["g"], o["g"] * SLOPE)


# ----------------------------------------------------------------------------------------------------------------------
# the network: float64 autograd, and float32 autograd over the defined-bit convolutions
# ----------------------------------------------------------------------------------------------------------------------
_INPUT_ONLY = [0]


class _C32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride, pad):
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pad)
        return R.conv32(x, w, stride, pad)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = _T32.apply(gy, w, *ctx.cfg) if ctx.needs_input_grad[0] else None
        gw = _W32.apply(gy, x, *ctx.cfg) if ctx.needs_input_grad[1] and not _INPUT_ONLY[0] else None
        return gx, gw, None, None


class _T32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, w, stride, pad):
        ctx.save_for_backward(g, w)
        ctx.cfg = (stride, pad)
        return dgrad32(g, w, stride, pad)

    @staticmethod
    def backward(ctx, ggx):
        g, w = ctx.saved_tensors
        d_g = _C32.apply(ggx, w, *ctx.cfg) if ctx.needs_input_grad[0] else None
        d_w = _W32.apply(g, ggx, *ctx.cfg) if ctx.needs_input_grad[1] else None
        return d_g, d_w, None, None


class _W32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, stride, pad):
        ctx.save_for_backward(g, x)
        ctx.cfg = (stride, pad)
        return wgrad32(g, x, stride, pad)

    @staticmethod
    def backward(ctx, ggw):
        g, x = ctx.saved_tensors
        d_g = _C32.apply(x, ggw, *ctx.cfg) if ctx.needs_input_grad[0] else None
        d_x = _T32.apply(g, ggw, *ctx.cfg) if ctx.needs_input_grad[1] else None
        return d_g, d_x, None, None


def _logits(ws, x, f32):
    a = x
    L = R._layers(ws)
    for i, (w, stride, pad) in enumerate(L):
        u = _C32.apply(a, w, stride, pad) if f32 else F.conv2d(a, w, stride=stride, padding=pad)
        a = F.leaky_relu(u, SLOPE)
    return u.reshape(x.shape[0], -1)


def _input_grad(d, x, sel):
    _INPUT_ONLY[0] += 1
    try:
        gx, = torch.autograd.grad(d, x, sel, create_graph=True)
    finally:
        _INPUT_ONLY[0] -= 1
    return gx


def sigmoid32(d):
    """1 / (1 + exp(-d)) in float32 with every bit defined: three float32 operations, each the float64 result rounded."""
    e = torch.exp(-d.double()).float()
    s = (1.0 + e.double()).float()
    return (1.0 / s.double()).float()


@functools.lru_cache(maxsize=None)
def cotangent(name):
    """The seeded cotangent (B real, out_dim) of gw_plain."""
    s = R.case(name)["spec"]
    return torch.randn(len(batch(name)[0]), s["out_dim"], generator=torch.Generator().manual_seed(s["seed"] * 19 + 3))


def net_grads(name, f32=False, mutate=None):
    """{"gw_plain" | "gw_r1" | "step": {parameter: gradient}} on `batch(name)`: float64 autograd over the chain, or (`f32`)
    float32 autograd over the defined-bit convolutions.  `mutate` "fake_in_r1": the fake half enters R1."""
    assert mutate in (None, "fake_in_r1") and not (mutate and f32)
    c = R.case(name)
    dt = torch.float32 if f32 else torch.float64
    real, fake = batch(name)
    B = len(real)
    ws = {k: v.to(dt).clone().requires_grad_() for k, v in c["wsd"].items()}
    wl = list(ws.values())
    named = lambda gs: {k: g.detach() for k, g in zip(ws, gs)}
    out = {}
    xr = c["x"][list(real)].to(dt).requires_grad_()
    d = _logits(ws, xr, f32)
    out["gw_plain"] = named(torch.autograd.grad(d, wl, cotangent(name).to(dt), retain_graph=True))
    sel = torch.zeros_like(d)
    sel[:, 0] = 1.0
    gx = _input_grad(d, xr, sel)
    out["gw_r1"] = named(torch.autograd.grad(gx, wl, (2.0 / B) * gx.detach()))
    xa = c["x"][list(real) + list(fake)].to(dt).requires_grad_()
    d = _logits(ws, xa, f32)
    sel = torch.zeros_like(d)
    sel[:(2 * B if mutate == "fake_in_r1" else B), 0] = 1.0
    gx = _input_grad(d, xa, sel)
    p = sigmoid32(d.detach()[:, 0]) if f32 else torch.sigmoid(d.detach()[:, 0])
    gd = torch.zeros_like(d)
    gd[:, 0] = torch.cat([p[:B] - 1.0, p[B:]]) / B   # BCE's derivative on the logits (float32: p - 1 and / B are exact here)
    out["step"] = named(torch.autograd.grad([d, gx], wl, [gd, (REG_W * 2.0 / B) * gx.detach()]))
    return out


@functools.lru_cache(maxsize=None)
def net_case(name):
    """`refs` {key: {parameter: float64 gradient}}, `scale` their rms; built once, shared, never modified."""
    refs = net_grads(name)
    return dict(refs=refs, scale={k: {p: R.rms(g) for p, g in v.items()} for k, v in refs.items()})


# ----------------------------------------------------------------------------------------------------------------------
# errors, floors, bars
# ----------------------------------------------------------------------------------------------------------------------
def err(y, ref, scale):
    """R.err; a reference of rms 0 must be met exactly (0.0 then, else inf)."""
    if scale == 0.0:
        return 0.0 if bool((y.detach().cpu() == 0).all()) else float("inf")
    return R.err(y, ref, scale)


def layer_errors(name, route, outputs):
    """{"<route>/<key>": err} of a candidate's {key: tensor}."""
    c = layer_case(name, route)
    return {f"{route}/{k}": err(y, c["refs"][k], c["scale"][k]) for k, y in outputs.items()}


def net_errors(name, key, grads):
    """{"<key>/<parameter>": err} of a candidate's {parameter: gradient} for the network quantity `key`."""
    c = net_case(name)
    return {f"{key}/{p}": err(g, c["refs"][key][p], c["scale"][key][p]) for p, g in grads.items()}


def measure_floor(name):
    """{key: err(float32 restatement, float64 reference)}: every key of FP32_FLOOR_BWD[name]."""
    out = {}
    for route in routes_of(name):
        out.update(layer_errors(name, route, layer_outputs(layer_case(name, route)["o"], f32=True)))
    for key, grads in net_grads(name, f32=True).items():
        out.update(net_errors(name, key, grads))
    return out


def bar(name, key):
    """3 x the committed fp32 floor; the network's step has one reference for both of its forms."""
    return 3.0 * FP32_FLOOR_BWD[name][key]


def judge(name, errors):
    """-> list of messages, one per measured error above its bar."""
    return [f"{k}: error {e:.3e} above the bar {bar(name, k):.3e}" for k, e in errors.items() if not e <= bar(name, k)]


def mutation_errors(name, route, mutation):
    """{key: err(mutated float64 restatement, float64 reference)} of one layer case, or (`route` "net") of the step."""
    if route == "net":
        return net_errors(name, "step", net_grads(name, mutate=mutation)["step"])
    dp, wp = plans(name, route)
    return layer_errors(name, route, layer_outputs(layer_case(name, route)["o"], mutate=mutation, dp=dp, wp=wp))


def caught(name, route, mutation):
    """The keys on which the mutation exceeds 3 x bar."""
    return [k for k, e in mutation_errors(name, route, mutation).items() if e > 3.0 * bar(name, k)]


# Measured by `measure_floor` (every bit of the float32 restatement is defined: R.conv32); tests/test_disc_bwd_regimes_cpu.py keeps
# a fresh computation within the last printed digit.  Keys: "<route>/<quantity>" of a layer case, "<quantity>/<parameter>" of a
# network case.  (`default_init_128`, step: one image is both real and fake and its logit is 0.0069, so the plain gradient is
# (sigmoid(d) - 1) G + sigmoid(d) G = 0.0034 G from two halves of 0.5 G each: the halves' own float32 noise is enlarged 150 times,
# and half an ulp on each of the two float32 cotangents alone moves conv_out's gradient by 1.6e-4 of its rms.  The arithmetic
# of that cell is ill-conditioned, not the kernels; its floors of 3e-4 ... 3e-3 say so.)
FP32_FLOOR_BWD = {
    "unit": {
        "b2_B1/dgrad_m": 3.08e-06, "b2_B1/dgrad_pre": 3.32e-06, "b2_B1/wgrad_m": 3.30e-06, "b2_B1/bwd_gw": 4.11e-06, "b2_B1/bwd_dx":
        3.32e-06, "b2_B1/wgrad_m+acc": 2.42e-06, "b2_B1/bwd_gw+acc": 3.01e-06, "b1_B1/dgrad_m": 2.09e-06, "b1_B1/dgrad_pre":
        3.57e-06, "b1_B1/wgrad_m": 4.55e-06, "b1_B1/bwd_gw": 6.30e-06, "b1_B1/bwd_dx": 3.57e-06, "b1_B1/wgrad_m+acc": 3.10e-06,
        "b1_B1/bwd_gw+acc": 4.08e-06, "b0_B1/dgrad_m": 1.09e-06, "b0_B1/dgrad_pre": 1.16e-06, "b0_B1/wgrad_m": 3.77e-06,
        "b0_B1/bwd_gw": 3.47e-06, "b0_B1/bwd_dx": 1.16e-06, "b0_B1/wgrad_m+acc": 2.67e-06, "b0_B1/bwd_gw+acc": 2.29e-06,
        "b2_B2/dgrad_m": 3.18e-06, "b2_B2/dgrad_pre": 4.94e-06, "b2_B2/wgrad_m": 4.43e-06, "b2_B2/bwd_gw": 6.26e-06, "b2_B2/bwd_dx":
        4.94e-06, "b2_B2/wgrad_m+acc": 3.35e-06, "b2_B2/bwd_gw+acc": 4.40e-06, "head_B1/dgrad_m": 4.17e-07, "head_B1/dgrad_pre":
        5.44e-07, "head_B1/wgrad_m": 3.68e-07, "head_B1/bwd_gw": 3.76e-07, "head_B1/bwd_dx": 5.44e-07, "head_B1/wgrad_m+acc":
        5.05e-07, "head_B1/bwd_gw+acc": 5.68e-07, "b3_B1/dgrad_m": 3.21e-06, "b3_B1/dgrad_pre": 3.97e-06, "b3_B1/wgrad_m": 1.61e-06,
        "b3_B1/bwd_gw": 2.58e-06, "b3_B1/bwd_dx": 3.97e-06, "b3_B1/wgrad_m+acc": 1.34e-06, "b3_B1/bwd_gw+acc": 1.87e-06,
        "b3_B3/dgrad_m": 3.94e-06, "b3_B3/dgrad_pre": 5.05e-06, "b3_B3/wgrad_m": 4.79e-06, "b3_B3/bwd_gw": 5.61e-06, "b3_B3/bwd_dx":
        5.05e-06, "b3_B3/wgrad_m+acc": 3.32e-06, "b3_B3/bwd_gw+acc": 3.82e-06, "head_B3/dgrad_m": 5.48e-07, "head_B3/dgrad_pre":
        5.64e-07, "head_B3/wgrad_m": 6.56e-07, "head_B3/bwd_gw": 7.23e-07, "head_B3/bwd_dx": 5.64e-07, "head_B3/wgrad_m+acc":
        5.28e-07, "head_B3/bwd_gw+acc": 5.74e-07, "gw_plain/blocks.0.weight": 7.74e-06, "gw_plain/blocks.1.weight": 1.65e-05,
        "gw_plain/blocks.2.weight": 7.08e-06, "gw_plain/blocks.3.weight": 4.56e-06, "gw_plain/conv_out.weight": 4.16e-06,
        "gw_r1/blocks.0.weight": 6.35e-06, "gw_r1/blocks.1.weight": 6.60e-06, "gw_r1/blocks.2.weight": 5.30e-06,
        "gw_r1/blocks.3.weight": 4.30e-06, "gw_r1/conv_out.weight": 6.61e-06, "step/blocks.0.weight": 4.90e-06,
        "step/blocks.1.weight": 1.54e-05, "step/blocks.2.weight": 2.01e-05, "step/blocks.3.weight": 9.88e-06,
        "step/conv_out.weight": 8.10e-06
    },
    "default_init": {
        "b2_B1/dgrad_m": 3.30e-06, "b2_B1/dgrad_pre": 3.95e-06, "b2_B1/wgrad_m": 3.15e-06, "b2_B1/bwd_gw": 4.05e-06, "b2_B1/bwd_dx":
        3.95e-06, "b2_B1/wgrad_m+acc": 2.17e-06, "b2_B1/bwd_gw+acc": 2.86e-06, "b1_B1/dgrad_m": 2.25e-06, "b1_B1/dgrad_pre":
        2.79e-06, "b1_B1/wgrad_m": 7.30e-06, "b1_B1/bwd_gw": 1.07e-05, "b1_B1/bwd_dx": 2.79e-06, "b1_B1/wgrad_m+acc": 5.26e-06,
        "b1_B1/bwd_gw+acc": 8.18e-06, "b0_B1/dgrad_m": 1.44e-06, "b0_B1/dgrad_pre": 1.41e-06, "b0_B1/wgrad_m": 3.57e-06,
        "b0_B1/bwd_gw": 3.25e-06, "b0_B1/bwd_dx": 1.41e-06, "b0_B1/wgrad_m+acc": 2.61e-06, "b0_B1/bwd_gw+acc": 2.29e-06,
        "b2_B2/dgrad_m": 4.33e-06, "b2_B2/dgrad_pre": 5.18e-06, "b2_B2/wgrad_m": 5.18e-06, "b2_B2/bwd_gw": 6.46e-06, "b2_B2/bwd_dx":
        5.18e-06, "b2_B2/wgrad_m+acc": 3.52e-06, "b2_B2/bwd_gw+acc": 4.67e-06, "head_B1/dgrad_m": 2.79e-07, "head_B1/dgrad_pre":
        3.60e-07, "head_B1/wgrad_m": 3.48e-07, "head_B1/bwd_gw": 4.19e-07, "head_B1/bwd_dx": 3.60e-07, "head_B1/wgrad_m+acc":
        4.82e-07, "head_B1/bwd_gw+acc": 5.47e-07, "b3_B1/dgrad_m": 3.27e-06, "b3_B1/dgrad_pre": 4.06e-06, "b3_B1/wgrad_m": 2.04e-06,
        "b3_B1/bwd_gw": 2.17e-06, "b3_B1/bwd_dx": 4.06e-06, "b3_B1/wgrad_m+acc": 1.27e-06, "b3_B1/bwd_gw+acc": 1.69e-06,
        "b3_B3/dgrad_m": 4.25e-06, "b3_B3/dgrad_pre": 7.44e-06, "b3_B3/wgrad_m": 3.55e-06, "b3_B3/bwd_gw": 4.26e-06, "b3_B3/bwd_dx":
        7.44e-06, "b3_B3/wgrad_m+acc": 2.23e-06, "b3_B3/bwd_gw+acc": 3.12e-06, "head_B3/dgrad_m": 3.66e-07, "head_B3/dgrad_pre":
        4.65e-07, "head_B3/wgrad_m": 6.98e-07, "head_B3/bwd_gw": 7.47e-07, "head_B3/bwd_dx": 4.65e-07, "head_B3/wgrad_m+acc":
        7.49e-07, "head_B3/bwd_gw+acc": 7.90e-07, "gw_plain/blocks.0.weight": 8.39e-06, "gw_plain/blocks.1.weight": 1.51e-05,
        "gw_plain/blocks.2.weight": 8.22e-06, "gw_plain/blocks.3.weight": 4.95e-06, "gw_plain/conv_out.weight": 7.18e-06,
        "gw_r1/blocks.0.weight": 4.22e-06, "gw_r1/blocks.1.weight": 6.82e-06, "gw_r1/blocks.2.weight": 7.17e-06,
        "gw_r1/blocks.3.weight": 5.57e-06, "gw_r1/conv_out.weight": 7.63e-06, "step/blocks.0.weight": 1.15e-05,
        "step/blocks.1.weight": 2.44e-05, "step/blocks.2.weight": 1.34e-05, "step/blocks.3.weight": 8.79e-06,
        "step/conv_out.weight": 1.94e-05
    },
    "white_bg": {
        "b2_B1/dgrad_m": 2.32e-06, "b2_B1/dgrad_pre": 4.50e-06, "b2_B1/wgrad_m": 2.76e-06, "b2_B1/bwd_gw": 3.57e-06, "b2_B1/bwd_dx":
        4.50e-06, "b2_B1/wgrad_m+acc": 1.90e-06, "b2_B1/bwd_gw+acc": 2.57e-06, "b1_B1/dgrad_m": 2.16e-06, "b1_B1/dgrad_pre":
        2.75e-06, "b1_B1/wgrad_m": 5.79e-06, "b1_B1/bwd_gw": 6.70e-06, "b1_B1/bwd_dx": 2.75e-06, "b1_B1/wgrad_m+acc": 4.19e-06,
        "b1_B1/bwd_gw+acc": 4.98e-06, "b0_B1/dgrad_m": 1.21e-06, "b0_B1/dgrad_pre": 1.44e-06, "b0_B1/wgrad_m": 5.04e-06,
        "b0_B1/bwd_gw": 4.61e-06, "b0_B1/bwd_dx": 1.44e-06, "b0_B1/wgrad_m+acc": 3.47e-06, "b0_B1/bwd_gw+acc": 3.25e-06,
        "b2_B2/dgrad_m": 3.17e-06, "b2_B2/dgrad_pre": 6.16e-06, "b2_B2/wgrad_m": 4.54e-06, "b2_B2/bwd_gw": 5.56e-06, "b2_B2/bwd_dx":
        6.16e-06, "b2_B2/wgrad_m+acc": 3.27e-06, "b2_B2/bwd_gw+acc": 3.99e-06, "head_B1/dgrad_m": 3.10e-07, "head_B1/dgrad_pre":
        4.57e-07, "head_B1/wgrad_m": 3.30e-07, "head_B1/bwd_gw": 2.86e-07, "head_B1/bwd_dx": 4.57e-07, "head_B1/wgrad_m+acc":
        3.49e-07, "head_B1/bwd_gw+acc": 3.72e-07, "b3_B1/dgrad_m": 4.02e-06, "b3_B1/dgrad_pre": 3.32e-06, "b3_B1/wgrad_m": 1.93e-06,
        "b3_B1/bwd_gw": 2.19e-06, "b3_B1/bwd_dx": 3.32e-06, "b3_B1/wgrad_m+acc": 1.60e-06, "b3_B1/bwd_gw+acc": 1.47e-06,
        "b3_B3/dgrad_m": 5.56e-06, "b3_B3/dgrad_pre": 4.62e-06, "b3_B3/wgrad_m": 3.47e-06, "b3_B3/bwd_gw": 4.91e-06, "b3_B3/bwd_dx":
        4.62e-06, "b3_B3/wgrad_m+acc": 2.62e-06, "b3_B3/bwd_gw+acc": 3.56e-06, "head_B3/dgrad_m": 3.08e-07, "head_B3/dgrad_pre":
        6.33e-07, "head_B3/wgrad_m": 5.30e-07, "head_B3/bwd_gw": 5.46e-07, "head_B3/bwd_dx": 6.33e-07, "head_B3/wgrad_m+acc":
        4.62e-07, "head_B3/bwd_gw+acc": 5.96e-07, "gw_plain/blocks.0.weight": 7.02e-06, "gw_plain/blocks.1.weight": 1.09e-05,
        "gw_plain/blocks.2.weight": 6.04e-06, "gw_plain/blocks.3.weight": 4.49e-06, "gw_plain/conv_out.weight": 4.86e-06,
        "gw_r1/blocks.0.weight": 5.90e-06, "gw_r1/blocks.1.weight": 7.02e-06, "gw_r1/blocks.2.weight": 5.61e-06,
        "gw_r1/blocks.3.weight": 4.43e-06, "gw_r1/conv_out.weight": 7.24e-06, "step/blocks.0.weight": 8.58e-06,
        "step/blocks.1.weight": 1.70e-05, "step/blocks.2.weight": 1.47e-05, "step/blocks.3.weight": 9.19e-06,
        "step/conv_out.weight": 1.69e-05
    },
    "mask": {
        "b2_B1/dgrad_m": 2.13e-06, "b2_B1/dgrad_pre": 3.95e-06, "b2_B1/wgrad_m": 1.98e-06, "b2_B1/bwd_gw": 2.60e-06, "b2_B1/bwd_dx":
        3.95e-06, "b2_B1/wgrad_m+acc": 1.45e-06, "b2_B1/bwd_gw+acc": 1.77e-06, "b1_B1/dgrad_m": 2.11e-06, "b1_B1/dgrad_pre":
        2.80e-06, "b1_B1/wgrad_m": 4.09e-06, "b1_B1/bwd_gw": 5.37e-06, "b1_B1/bwd_dx": 2.80e-06, "b1_B1/wgrad_m+acc": 2.83e-06,
        "b1_B1/bwd_gw+acc": 3.60e-06, "b0_B1/dgrad_m": 1.07e-06, "b0_B1/dgrad_pre": 2.21e-06, "b0_B1/wgrad_m": 1.80e-06,
        "b0_B1/bwd_gw": 1.80e-06, "b0_B1/bwd_dx": 2.21e-06, "b0_B1/wgrad_m+acc": 1.28e-06, "b0_B1/bwd_gw+acc": 1.27e-06,
        "b2_B2/dgrad_m": 3.01e-06, "b2_B2/dgrad_pre": 5.59e-06, "b2_B2/wgrad_m": 1.98e-06, "b2_B2/bwd_gw": 2.60e-06, "b2_B2/bwd_dx":
        5.59e-06, "b2_B2/wgrad_m+acc": 1.45e-06, "b2_B2/bwd_gw+acc": 1.77e-06, "head_B1/dgrad_m": 1.23e-07, "head_B1/dgrad_pre":
        1.27e-07, "head_B1/wgrad_m": 3.33e-07, "head_B1/bwd_gw": 1.84e-07, "head_B1/bwd_dx": 1.27e-07, "head_B1/wgrad_m+acc":
        2.96e-07, "head_B1/bwd_gw+acc": 2.42e-07, "b3_B1/dgrad_m": 3.27e-06, "b3_B1/dgrad_pre": 3.81e-06, "b3_B1/wgrad_m": 1.43e-06,
        "b3_B1/bwd_gw": 1.57e-06, "b3_B1/bwd_dx": 3.81e-06, "b3_B1/wgrad_m+acc": 1.11e-06, "b3_B1/bwd_gw+acc": 1.25e-06,
        "b3_B3/dgrad_m": 4.33e-06, "b3_B3/dgrad_pre": 4.93e-06, "b3_B3/wgrad_m": 2.32e-06, "b3_B3/bwd_gw": 3.06e-06, "b3_B3/bwd_dx":
        4.93e-06, "b3_B3/wgrad_m+acc": 1.64e-06, "b3_B3/bwd_gw+acc": 2.24e-06, "head_B3/dgrad_m": 2.03e-07, "head_B3/dgrad_pre":
        1.65e-07, "head_B3/wgrad_m": 4.44e-07, "head_B3/bwd_gw": 4.23e-07, "head_B3/bwd_dx": 1.65e-07, "head_B3/wgrad_m+acc":
        3.75e-07, "head_B3/bwd_gw+acc": 3.00e-07, "gw_plain/blocks.0.weight": 2.89e-06, "gw_plain/blocks.1.weight": 7.59e-06,
        "gw_plain/blocks.2.weight": 5.98e-06, "gw_plain/blocks.3.weight": 4.53e-06, "gw_plain/conv_out.weight": 3.60e-06,
        "gw_r1/blocks.0.weight": 3.68e-06, "gw_r1/blocks.1.weight": 6.37e-06, "gw_r1/blocks.2.weight": 5.67e-06,
        "gw_r1/blocks.3.weight": 4.78e-06, "gw_r1/conv_out.weight": 2.56e-06, "step/blocks.0.weight": 3.75e-06,
        "step/blocks.1.weight": 9.93e-06, "step/blocks.2.weight": 7.56e-06, "step/blocks.3.weight": 5.20e-06,
        "step/conv_out.weight": 5.10e-06
    },
    "dark": {
        "b2_B1/dgrad_m": 2.35e-06, "b2_B1/dgrad_pre": 3.92e-06, "b2_B1/wgrad_m": 3.33e-06, "b2_B1/bwd_gw": 4.72e-06, "b2_B1/bwd_dx":
        3.92e-06, "b2_B1/wgrad_m+acc": 2.43e-06, "b2_B1/bwd_gw+acc": 3.54e-06, "b1_B1/dgrad_m": 1.82e-06, "b1_B1/dgrad_pre":
        2.24e-06, "b1_B1/wgrad_m": 5.11e-06, "b1_B1/bwd_gw": 6.10e-06, "b1_B1/bwd_dx": 2.24e-06, "b1_B1/wgrad_m+acc": 3.63e-06,
        "b1_B1/bwd_gw+acc": 4.14e-06, "b0_B1/dgrad_m": 1.04e-06, "b0_B1/dgrad_pre": 1.92e-06, "b0_B1/wgrad_m": 7.47e-06,
        "b0_B1/bwd_gw": 5.68e-06, "b0_B1/bwd_dx": 1.92e-06, "b0_B1/wgrad_m+acc": 5.21e-06, "b0_B1/bwd_gw+acc": 4.06e-06,
        "b2_B2/dgrad_m": 2.71e-06, "b2_B2/dgrad_pre": 4.50e-06, "b2_B2/wgrad_m": 3.92e-06, "b2_B2/bwd_gw": 6.32e-06, "b2_B2/bwd_dx":
        4.50e-06, "b2_B2/wgrad_m+acc": 2.91e-06, "b2_B2/bwd_gw+acc": 4.48e-06, "head_B1/dgrad_m": 3.21e-07, "head_B1/dgrad_pre":
        4.23e-07, "head_B1/wgrad_m": 2.36e-07, "head_B1/bwd_gw": 3.14e-07, "head_B1/bwd_dx": 4.23e-07, "head_B1/wgrad_m+acc":
        3.25e-07, "head_B1/bwd_gw+acc": 3.80e-07, "b3_B1/dgrad_m": 4.76e-06, "b3_B1/dgrad_pre": 4.50e-06, "b3_B1/wgrad_m": 2.18e-06,
        "b3_B1/bwd_gw": 2.09e-06, "b3_B1/bwd_dx": 4.50e-06, "b3_B1/wgrad_m+acc": 1.32e-06, "b3_B1/bwd_gw+acc": 1.59e-06,
        "b3_B3/dgrad_m": 5.02e-06, "b3_B3/dgrad_pre": 6.18e-06, "b3_B3/wgrad_m": 3.84e-06, "b3_B3/bwd_gw": 4.15e-06, "b3_B3/bwd_dx":
        6.18e-06, "b3_B3/wgrad_m+acc": 2.85e-06, "b3_B3/bwd_gw+acc": 2.98e-06, "head_B3/dgrad_m": 4.23e-07, "head_B3/dgrad_pre":
        4.48e-07, "head_B3/wgrad_m": 5.31e-07, "head_B3/bwd_gw": 7.21e-07, "head_B3/bwd_dx": 4.48e-07, "head_B3/wgrad_m+acc":
        4.65e-07, "head_B3/bwd_gw+acc": 5.09e-07, "gw_plain/blocks.0.weight": 7.50e-06, "gw_plain/blocks.1.weight": 9.75e-06,
        "gw_plain/blocks.2.weight": 7.66e-06, "gw_plain/blocks.3.weight": 3.97e-06, "gw_plain/conv_out.weight": 4.27e-06,
        "gw_r1/blocks.0.weight": 5.84e-06, "gw_r1/blocks.1.weight": 6.43e-06, "gw_r1/blocks.2.weight": 6.04e-06,
        "gw_r1/blocks.3.weight": 4.75e-06, "gw_r1/conv_out.weight": 6.91e-06, "step/blocks.0.weight": 7.80e-06,
        "step/blocks.1.weight": 1.19e-05, "step/blocks.2.weight": 1.06e-05, "step/blocks.3.weight": 8.25e-06,
        "step/conv_out.weight": 1.26e-05
    },
    "shrunk": {
        "b2_B1/dgrad_m": 2.77e-06, "b2_B1/dgrad_pre": 3.26e-06, "b2_B1/wgrad_m": 3.26e-06, "b2_B1/bwd_gw": 3.50e-06, "b2_B1/bwd_dx":
        3.26e-06, "b2_B1/wgrad_m+acc": 2.48e-06, "b2_B1/bwd_gw+acc": 2.48e-06, "b1_B1/dgrad_m": 2.57e-06, "b1_B1/dgrad_pre":
        2.95e-06, "b1_B1/wgrad_m": 6.10e-06, "b1_B1/bwd_gw": 6.71e-06, "b1_B1/bwd_dx": 2.95e-06, "b1_B1/wgrad_m+acc": 4.46e-06,
        "b1_B1/bwd_gw+acc": 4.87e-06, "b0_B1/dgrad_m": 1.04e-06, "b0_B1/dgrad_pre": 1.13e-06, "b0_B1/wgrad_m": 3.40e-06,
        "b0_B1/bwd_gw": 3.37e-06, "b0_B1/bwd_dx": 1.13e-06, "b0_B1/wgrad_m+acc": 2.46e-06, "b0_B1/bwd_gw+acc": 2.49e-06,
        "b2_B2/dgrad_m": 4.40e-06, "b2_B2/dgrad_pre": 3.81e-06, "b2_B2/wgrad_m": 5.98e-06, "b2_B2/bwd_gw": 5.75e-06, "b2_B2/bwd_dx":
        3.81e-06, "b2_B2/wgrad_m+acc": 4.08e-06, "b2_B2/bwd_gw+acc": 4.20e-06, "head_B1/dgrad_m": 2.95e-07, "head_B1/dgrad_pre":
        4.58e-07, "head_B1/wgrad_m": 5.09e-07, "head_B1/bwd_gw": 3.83e-07, "head_B1/bwd_dx": 4.58e-07, "head_B1/wgrad_m+acc":
        4.62e-07, "head_B1/bwd_gw+acc": 5.11e-07, "b3_B1/dgrad_m": 4.77e-06, "b3_B1/dgrad_pre": 3.38e-06, "b3_B1/wgrad_m": 1.92e-06,
        "b3_B1/bwd_gw": 2.87e-06, "b3_B1/bwd_dx": 3.38e-06, "b3_B1/wgrad_m+acc": 1.35e-06, "b3_B1/bwd_gw+acc": 1.96e-06,
        "b3_B3/dgrad_m": 4.06e-06, "b3_B3/dgrad_pre": 5.59e-06, "b3_B3/wgrad_m": 3.26e-06, "b3_B3/bwd_gw": 4.40e-06, "b3_B3/bwd_dx":
        5.59e-06, "b3_B3/wgrad_m+acc": 2.31e-06, "b3_B3/bwd_gw+acc": 3.04e-06, "head_B3/dgrad_m": 4.38e-07, "head_B3/dgrad_pre":
        6.06e-07, "head_B3/wgrad_m": 6.40e-07, "head_B3/bwd_gw": 7.33e-07, "head_B3/bwd_dx": 6.06e-07, "head_B3/wgrad_m+acc":
        5.16e-07, "head_B3/bwd_gw+acc": 6.25e-07, "gw_plain/blocks.0.weight": 7.30e-06, "gw_plain/blocks.1.weight": 1.06e-05,
        "gw_plain/blocks.2.weight": 7.58e-06, "gw_plain/blocks.3.weight": 5.59e-06, "gw_plain/conv_out.weight": 6.85e-06,
        "gw_r1/blocks.0.weight": 6.49e-06, "gw_r1/blocks.1.weight": 6.91e-06, "gw_r1/blocks.2.weight": 5.85e-06,
        "gw_r1/blocks.3.weight": 5.14e-06, "gw_r1/conv_out.weight": 8.21e-06, "step/blocks.0.weight": 9.79e-06,
        "step/blocks.1.weight": 1.84e-05, "step/blocks.2.weight": 1.33e-05, "step/blocks.3.weight": 1.21e-05,
        "step/conv_out.weight": 1.73e-05
    },
    "grown3": {
        "b2_B1/dgrad_m": 3.44e-06, "b2_B1/dgrad_pre": 3.61e-06, "b2_B1/wgrad_m": 2.97e-06, "b2_B1/bwd_gw": 4.90e-06, "b2_B1/bwd_dx":
        3.61e-06, "b2_B1/wgrad_m+acc": 2.28e-06, "b2_B1/bwd_gw+acc": 3.72e-06, "b1_B1/dgrad_m": 1.96e-06, "b1_B1/dgrad_pre":
        4.25e-06, "b1_B1/wgrad_m": 5.53e-06, "b1_B1/bwd_gw": 6.48e-06, "b1_B1/bwd_dx": 4.25e-06, "b1_B1/wgrad_m+acc": 3.90e-06,
        "b1_B1/bwd_gw+acc": 4.42e-06, "b0_B1/dgrad_m": 2.02e-06, "b0_B1/dgrad_pre": 1.51e-06, "b0_B1/wgrad_m": 2.67e-06,
        "b0_B1/bwd_gw": 4.12e-06, "b0_B1/bwd_dx": 1.51e-06, "b0_B1/wgrad_m+acc": 1.83e-06, "b0_B1/bwd_gw+acc": 2.89e-06,
        "b2_B2/dgrad_m": 3.59e-06, "b2_B2/dgrad_pre": 3.78e-06, "b2_B2/wgrad_m": 3.78e-06, "b2_B2/bwd_gw": 6.15e-06, "b2_B2/bwd_dx":
        3.78e-06, "b2_B2/wgrad_m+acc": 2.69e-06, "b2_B2/bwd_gw+acc": 4.16e-06, "head_B1/dgrad_m": 2.60e-07, "head_B1/dgrad_pre":
        4.82e-07, "head_B1/wgrad_m": 3.00e-07, "head_B1/bwd_gw": 3.44e-07, "head_B1/bwd_dx": 4.82e-07, "head_B1/wgrad_m+acc":
        3.17e-07, "head_B1/bwd_gw+acc": 4.55e-07, "b3_B1/dgrad_m": 3.89e-06, "b3_B1/dgrad_pre": 5.62e-06, "b3_B1/wgrad_m": 2.49e-06,
        "b3_B1/bwd_gw": 2.24e-06, "b3_B1/bwd_dx": 5.62e-06, "b3_B1/wgrad_m+acc": 2.02e-06, "b3_B1/bwd_gw+acc": 1.56e-06,
        "b3_B3/dgrad_m": 4.02e-06, "b3_B3/dgrad_pre": 5.66e-06, "b3_B3/wgrad_m": 3.01e-06, "b3_B3/bwd_gw": 5.39e-06, "b3_B3/bwd_dx":
        5.66e-06, "b3_B3/wgrad_m+acc": 2.09e-06, "b3_B3/bwd_gw+acc": 3.85e-06, "head_B3/dgrad_m": 4.54e-07, "head_B3/dgrad_pre":
        4.87e-07, "head_B3/wgrad_m": 4.87e-07, "head_B3/bwd_gw": 8.39e-07, "head_B3/bwd_dx": 4.87e-07, "head_B3/wgrad_m+acc":
        4.61e-07, "head_B3/bwd_gw+acc": 8.42e-07, "gw_plain/blocks.0.weight": 4.40e-06, "gw_plain/blocks.1.weight": 1.08e-05,
        "gw_plain/blocks.2.weight": 8.00e-06, "gw_plain/blocks.3.weight": 4.73e-06, "gw_plain/conv_out.weight": 4.98e-06,
        "gw_r1/blocks.0.weight": 4.62e-06, "gw_r1/blocks.1.weight": 6.80e-06, "gw_r1/blocks.2.weight": 6.47e-06,
        "gw_r1/blocks.3.weight": 4.71e-06, "gw_r1/conv_out.weight": 6.46e-06, "step/blocks.0.weight": 5.45e-06,
        "step/blocks.1.weight": 7.82e-06, "step/blocks.2.weight": 6.03e-06, "step/blocks.3.weight": 5.31e-06,
        "step/conv_out.weight": 7.14e-06
    },
    "grown8": {
        "b2_B1/dgrad_m": 3.00e-06, "b2_B1/dgrad_pre": 3.76e-06, "b2_B1/wgrad_m": 3.75e-06, "b2_B1/bwd_gw": 4.74e-06, "b2_B1/bwd_dx":
        3.76e-06, "b2_B1/wgrad_m+acc": 2.75e-06, "b2_B1/bwd_gw+acc": 3.35e-06, "b1_B1/dgrad_m": 1.82e-06, "b1_B1/dgrad_pre":
        2.83e-06, "b1_B1/wgrad_m": 4.80e-06, "b1_B1/bwd_gw": 6.80e-06, "b1_B1/bwd_dx": 2.83e-06, "b1_B1/wgrad_m+acc": 3.50e-06,
        "b1_B1/bwd_gw+acc": 4.72e-06, "b0_B1/dgrad_m": 1.31e-06, "b0_B1/dgrad_pre": 2.07e-06, "b0_B1/wgrad_m": 6.14e-06,
        "b0_B1/bwd_gw": 4.75e-06, "b0_B1/bwd_dx": 2.07e-06, "b0_B1/wgrad_m+acc": 4.37e-06, "b0_B1/bwd_gw+acc": 3.36e-06,
        "b2_B2/dgrad_m": 3.31e-06, "b2_B2/dgrad_pre": 4.16e-06, "b2_B2/wgrad_m": 5.61e-06, "b2_B2/bwd_gw": 7.09e-06, "b2_B2/bwd_dx":
        4.16e-06, "b2_B2/wgrad_m+acc": 4.14e-06, "b2_B2/bwd_gw+acc": 5.34e-06, "head_B1/dgrad_m": 4.33e-07, "head_B1/dgrad_pre":
        4.59e-07, "head_B1/wgrad_m": 3.82e-07, "head_B1/bwd_gw": 4.38e-07, "head_B1/bwd_dx": 4.59e-07, "head_B1/wgrad_m+acc":
        4.98e-07, "head_B1/bwd_gw+acc": 5.58e-07, "b3_B1/dgrad_m": 3.88e-06, "b3_B1/dgrad_pre": 4.11e-06, "b3_B1/wgrad_m": 2.04e-06,
        "b3_B1/bwd_gw": 2.14e-06, "b3_B1/bwd_dx": 4.11e-06, "b3_B1/wgrad_m+acc": 1.56e-06, "b3_B1/bwd_gw+acc": 1.83e-06,
        "b3_B3/dgrad_m": 4.07e-06, "b3_B3/dgrad_pre": 4.30e-06, "b3_B3/wgrad_m": 2.74e-06, "b3_B3/bwd_gw": 5.04e-06, "b3_B3/bwd_dx":
        4.30e-06, "b3_B3/wgrad_m+acc": 2.01e-06, "b3_B3/bwd_gw+acc": 3.91e-06, "head_B3/dgrad_m": 5.78e-07, "head_B3/dgrad_pre":
        4.82e-07, "head_B3/wgrad_m": 6.39e-07, "head_B3/bwd_gw": 7.18e-07, "head_B3/bwd_dx": 4.82e-07, "head_B3/wgrad_m+acc":
        5.43e-07, "head_B3/bwd_gw+acc": 5.83e-07, "gw_plain/blocks.0.weight": 7.24e-06, "gw_plain/blocks.1.weight": 1.27e-05,
        "gw_plain/blocks.2.weight": 6.96e-06, "gw_plain/blocks.3.weight": 4.17e-06, "gw_plain/conv_out.weight": 4.85e-06,
        "gw_r1/blocks.0.weight": 5.15e-06, "gw_r1/blocks.1.weight": 5.89e-06, "gw_r1/blocks.2.weight": 5.38e-06,
        "gw_r1/blocks.3.weight": 4.86e-06, "gw_r1/conv_out.weight": 6.42e-06, "step/blocks.0.weight": 5.94e-06,
        "step/blocks.1.weight": 6.86e-06, "step/blocks.2.weight": 5.59e-06, "step/blocks.3.weight": 4.98e-06,
        "step/conv_out.weight": 6.07e-06
    },
    "unit_128": {
        "b0_128_B1/dgrad_m": 1.09e-06, "b0_128_B1/dgrad_pre": 1.25e-06, "b0_128_B1/wgrad_m": 7.93e-06, "b0_128_B1/bwd_gw": 5.70e-06,
        "b0_128_B1/bwd_dx": 1.25e-06, "b0_128_B1/wgrad_m+acc": 5.68e-06, "b0_128_B1/bwd_gw+acc": 4.03e-06,
        "gw_plain/blocks.0.weight": 8.50e-06, "gw_plain/blocks.1.weight": 1.19e-05, "gw_plain/blocks.2.weight": 1.03e-05,
        "gw_plain/blocks.3.weight": 7.03e-06, "gw_plain/blocks.4.weight": 4.72e-06, "gw_plain/conv_out.weight": 4.54e-06,
        "gw_r1/blocks.0.weight": 6.49e-06, "gw_r1/blocks.1.weight": 9.81e-06, "gw_r1/blocks.2.weight": 5.95e-06,
        "gw_r1/blocks.3.weight": 6.37e-06, "gw_r1/blocks.4.weight": 6.22e-06, "gw_r1/conv_out.weight": 7.41e-06,
        "step/blocks.0.weight": 8.77e-06, "step/blocks.1.weight": 1.54e-05, "step/blocks.2.weight": 1.38e-05,
        "step/blocks.3.weight": 1.08e-05, "step/blocks.4.weight": 6.81e-06, "step/conv_out.weight": 1.14e-05
    },
    "default_init_128": {
        "b0_128_B1/dgrad_m": 1.34e-06, "b0_128_B1/dgrad_pre": 1.21e-06, "b0_128_B1/wgrad_m": 8.17e-06, "b0_128_B1/bwd_gw": 7.57e-06,
        "b0_128_B1/bwd_dx": 1.21e-06, "b0_128_B1/wgrad_m+acc": 5.67e-06, "b0_128_B1/bwd_gw+acc": 5.39e-06,
        "gw_plain/blocks.0.weight": 9.49e-06, "gw_plain/blocks.1.weight": 1.11e-05, "gw_plain/blocks.2.weight": 8.59e-06,
        "gw_plain/blocks.3.weight": 7.90e-06, "gw_plain/blocks.4.weight": 6.06e-06, "gw_plain/conv_out.weight": 4.48e-06,
        "gw_r1/blocks.0.weight": 7.22e-06, "gw_r1/blocks.1.weight": 8.04e-06, "gw_r1/blocks.2.weight": 6.54e-06,
        "gw_r1/blocks.3.weight": 6.29e-06, "gw_r1/blocks.4.weight": 5.94e-06, "gw_r1/conv_out.weight": 9.88e-06,
        "step/blocks.0.weight": 6.78e-04, "step/blocks.1.weight": 2.80e-03, "step/blocks.2.weight": 1.81e-03,
        "step/blocks.3.weight": 1.13e-03, "step/blocks.4.weight": 5.19e-04, "step/conv_out.weight": 2.83e-04
    },
}

# mutation -> the (regime, route) pairs in which the mutated float64 restatement is more than 3 x bar away from the reference on
# some key (route "net": the network's step); tests/test_disc_bwd_regimes_cpu.py::test_mutation_is_caught demands every pair.
#   mask_ge          the mask is `ref >= 0`: differs only AT zero -- `mask` alone has exact zeros (block 0's sums over a window of
#                    zeros, the zero image in every layer); the weight gradient cannot see it at block 0 (the input under such a
#                    sum is zero as well), the data gradients do
#   pre_dropped      lrelu'(x) of dgrad_pre / the fused launch is left out (block 0: only where the image has non-positive pixels)
#   pre_per_split    lrelu'(x) is applied by every K split AND to their sum: slope^k_splits (invisible at k_splits 1: the head)
#   no_x_slope       the fused launch's weight gradient reads x instead of lrelu(x)
#   drop_tail        the last K split is lost (k_splits > 1), or the ragged end of the only one, or the last partial pixel tile
#   acc_overwritten  the prefilled accumulator is overwritten (every class of the weight-gradient kernel)
#   mask_twice       the mask is written out first and applied again on load: slope^2
#   fake_in_r1       the one-pass step's selection cotangent covers the fake half as well
#   slope_001        0.01 for 0.2
CAUGHT_BY = {
    "mask_ge": (("mask", "b0_B1"), ("mask", "b1_B1"), ("mask", "b3_B3"), ("mask", "head_B3")),
    "pre_dropped": (("unit", "b1_B1"), ("white_bg", "b0_B1"), ("default_init", "head_B1")),
    "pre_per_split": (("unit", "b1_B1"), ("mask", "b0_B1"), ("grown8", "b3_B3")),
    "no_x_slope": (("unit", "b2_B1"), ("white_bg", "b0_B1"), ("dark", "head_B3")),
    "drop_tail": (("unit", "b2_B2"), ("default_init", "head_B3"), ("shrunk", "b3_B3"), ("unit_128", "b0_128_B1")),
    "acc_overwritten": (("unit", "b2_B1"), ("grown3", "b1_B1"), ("mask", "b0_B1"), ("dark", "b2_B2")),
    "mask_twice": (("unit", "b1_B1"), ("default_init_128", "b0_128_B1")),
    "fake_in_r1": tuple((n, "net") for n in NAMES),
    "slope_001": (("unit", "b3_B1"), ("white_bg", "b0_B1"), ("mask", "head_B1")),
}
# Mutations no regime or route can expose at 3 x bar, with the reason: none.  (What a single route cannot see is said above.)
NOT_DETECTABLE = {}
