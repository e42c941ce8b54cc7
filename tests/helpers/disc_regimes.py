"""The discriminator convolutions (csrc/disc.hip, csrc/disc_small.hip, csrc/disc_large.hip) at the operand scales a training
run reaches.  All plain torch on the CPU:

* `REGIMES` / `case`: named, seeded (weights, images) pairs for the 64 x 64 / n_feat 512 network (in_dim 3 / out_dim 7;
  `mask`: in_dim 1 / out_dim 1) and, as `unit_128` / `default_init_128`, the shipped 128 x 128 five-block network.  A regime
  holds a POOL of images; image i of a batch of any size is pool image i % POOL, and a test compares images `compare(B)`
  (all for B <= 5, else 0, B / 2, B - 1: three different pool images for every batch used).  Weights are
  O.seeded_conv_weights times a per-layer gain, or nn.Conv2d's own initialisation under a fixed seed.
* three chains, each returning every layer's PRE-activation: `chain(.., float64)` is O.dc_discriminator (the reference),
  `chain(.., float32)` the same chain in float32, the reference's own arithmetic noise (the "fp32 floor"; through `conv32`,
  a float32 convolution whose every bit is defined, so that the committed tables hold on any machine; `grad32` is its
  input gradient), `limb_model` the documented two-limb arithmetic with fp64 accumulation: hi = fp16(v), lo = fp16(v - hi), products xh wh + xh wl + xl wh, the LeakyReLU where the
  kernel has it (kind "tiled": conv4x4_tiled_f16x3_kernel on blocks 1-3, applied in fp32 to the predecessor's fp32 sums while
  they are loaded, the first block and the head on the fp32 kernels; kind "large": csrc/disc_large.hip, every block on limbs
  re-formed from the fp32 sums after the LeakyReLU, the head on fp32(hi + lo) with fp32 weights).
* per-layer cases ("L1/0.2": block 1 with x_slope 0.2) take their input from the float32 chain: a layer is tested on its own.
* `err`, `FP32_FLOOR`, `LIMB_MODEL`, `bar`, `judge`: err = max |y - ref| / rms(ref) with the rms of the whole pool; the
  committed floors and model errors; bar = 3 x floor (fp32 routes) or 3 x (model + floor) (limb routes), the factor being
  the suite's rule (tests/conftest.py: "<= 3x the native-fp32 error"; it covers the fp32 accumulation order the model leaves
  out); the assertions the GPU test makes on a candidate.  Nothing here is computed from a kernel's output.
* `MUTATIONS`, `CAUGHT_BY`, `NOT_DETECTABLE`: plausible kernel errors as mutations of `limb_model`, and which regime's bar
  exposes each (tests/test_disc_regimes_cpu.py rehearses it).

`overflow`: images of two brightnesses (even pool images x 1, odd x 0.01) under the smallest gain (grid of 0.25) at which
every bright image has an input of blocks 1-3 above 65504 (where the fp16 hi limb is inf and the lo limb -inf) while every
input of every layer of the dim images stays below and the float32 chain stays finite.  The source's claim is judged there:
an image with a limb-carried value above 65504 has every logit non-finite (or right to the fp32 bar), never finite and wrong.
"""
import functools
import math

import torch
import torch.nn.functional as F

import oi_oracle as O

POOL = 6
F16_MAX = 65504.0
CH = {64: (64, 128, 256, 512), 128: (32, 64, 128, 256, 512)}
SLOPE = 0.2

_D = dict(size=64, in_dim=3, out_dim=7, weights="seeded", gain=1.0, images="uniform", envelope=True, pool=POOL)
REGIMES = {
    "unit": dict(_D, seed=301),                                                   # the control: what the suite tested so far
    "default_init": dict(_D, weights="conv2d", seed=302),
    "white_bg": dict(_D, weights="conv2d", images="white_bg", seed=303),          # [-1, 1], 80 % exactly 1.0
    "mask": dict(_D, weights="conv2d", images="mask", in_dim=1, out_dim=1, seed=4304),
    "dark": dict(_D, weights="conv2d", images="dark", envelope=False, seed=305),  # images x 0.05
    "shrunk": dict(_D, gain=0.2, envelope=False, seed=306),
    "grown3": dict(_D, gain=3.0, seed=307),
    "grown8": dict(_D, gain=8.0, seed=308),
    "overflow": dict(_D, gain=None, images="two_levels", envelope=None, seed=309),
    "unit_128": dict(_D, size=128, pool=1, seed=310),
    "default_init_128": dict(_D, size=128, pool=1, weights="conv2d", seed=311),
}
NET64 = tuple(n for n, s in REGIMES.items() if s["size"] == 64 and n != "overflow")
MASK_ZERO_IMAGE = 3
DIM = 0.01

# route -> kind of arithmetic ("fp32" | "tiled" | "large"), batch; per-layer routes also the block.  The batches are the
# smallest that select each kernel (tests/test_gpu_disc_regimes.py derives them from oi_conv4x4_fwd_arena's conditions).
ROUTES = {
    "small_b1": dict(kind="fp32", B=1), "small_b4": dict(kind="fp32", B=4), "arena_b5": dict(kind="fp32", B=5),
    "arena_b32": dict(kind="tiled", B=32), "large_b16": dict(kind="large", B=16),
    "pre_b2": dict(kind="fp32", B=2), "pre_b32": dict(kind="tiled", B=32),
    # per layer; `launch`: what oi_conv4x4_fwd_arena must choose there, (pixel tile, K splits) of the tiled kernel or None
    "L1_b8": dict(kind="tiled", B=8, layer=1, launch=(64, 2)), "L1_b32": dict(kind="tiled", B=32, layer=1, launch=(64, 1)),
    "L1_b64": dict(kind="tiled", B=64, layer=1, launch=(128, 1)), "L1_b2": dict(kind="fp32", B=2, layer=1, launch=None),
    "L1_b32_any": dict(kind="fp32", B=32, layer=1, any_scale=True, launch=None),
    "L2_b16": dict(kind="tiled", B=16, layer=2, launch=(64, 2)), "L3_b32": dict(kind="tiled", B=32, layer=3, launch=(64, 2)),
}
LAYER_ROUTES = tuple(r for r, v in ROUTES.items() if "layer" in v)
LAYER_KEYS = tuple(f"L{l}/{s}" for l in (1, 2, 3) for s in (1.0, SLOPE))

MUTATIONS = ("drop_xl_wh", "drop_xh_wl", "flush_lo", "trunc_hi", "lrelu_after_split", "slope1_on_load", "bf16_limbs")


def compare(B):
    """The images of a batch of B that a test compares with the reference."""
    return list(range(B)) if B <= 5 else [0, B // 2, B - 1]


def batch_of(t, B):
    """Image i of a batch of B is pool image i % POOL."""
    return t[torch.arange(B) % t.shape[0]].contiguous()


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def err(y, ref, scale):
    """max |y - ref| / scale; inf when y is not finite.  `scale`: the rms of the reference over the regime's pool."""
    y = y.detach().double().cpu()
    if not bool(torch.isfinite(y).all()):
        return math.inf
    return float((y - ref.double()).abs().max()) / scale


# ----------------------------------------------------------------------------------------------------------------------
# weights, images
# ----------------------------------------------------------------------------------------------------------------------
def shapes(spec):
    ch = (spec["in_dim"],) + CH[spec["size"]]
    sh = {f"blocks.{i}.weight": (ch[i + 1], ch[i], 4, 4) for i in range(len(ch) - 1)}
    sh["conv_out.weight"] = (spec["out_dim"], ch[-1], 4, 4)
    return sh


def weights(spec, gain=None):
    sh = shapes(spec)
    if spec["weights"] == "conv2d":   # oi_amd.discriminator._ConvParam / the reference's layers: nn.Conv2d's own initialisation
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(spec["seed"])
            return {k: torch.nn.Conv2d(s[1], s[0], 4, bias=False).weight.detach().clone() for k, s in sh.items()}
    g = spec["gain"] if gain is None else gain
    return {k: v * g for k, v in O.seeded_conv_weights(sh, spec["seed"]).items()}


def images(spec):
    g = torch.Generator().manual_seed(spec["seed"] * 7 + 1)
    P, C, R = spec["pool"], spec["in_dim"], spec["size"]
    x = torch.rand(P, C, R, R, generator=g)
    kind = spec["images"]
    if kind == "white_bg":
        x = torch.where(torch.rand(P, C, R, R, generator=g) < 0.8, torch.ones(()), x * 2 - 1)
    elif kind == "mask":
        x = (x < 0.25).float()
        x[MASK_ZERO_IMAGE] = 0.0
    elif kind == "dark":
        x = x * 0.05
    elif kind == "two_levels":
        x = x * torch.where(torch.arange(P) % 2 == 0, 1.0, DIM).view(P, 1, 1, 1)
    return x


# ----------------------------------------------------------------------------------------------------------------------
# the three chains
# ----------------------------------------------------------------------------------------------------------------------
def _layers(wsd):
    n = len(wsd) - 1
    return [(wsd[f"blocks.{i}.weight"], 2, 1) for i in range(n)] + [(wsd["conv_out.weight"], 1, 0)]


def conv32(a, w, stride, pad):
    """A float32 convolution whose every bit is defined: the 16 taps of one input channel are summed exactly (float64), rounded,
    and the channels added in a plain float32 loop, in order.  (F.conv2d's float32 result depends on the instruction set the
    machine's library picks -- its error moves by a factor of 5 between two of them -- so it cannot carry a committed table.)"""
    B, Cin, H, W = a.shape
    Cout = w.shape[0]
    Ho, Wo = (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1
    cols = F.unfold(a.double(), 4, padding=pad, stride=stride).view(B, Cin, 16, Ho * Wo)
    p = torch.einsum("bckl,ock->cbol", cols, w.double().reshape(Cout, Cin, 16)).float()
    acc = p[0].clone()
    for c in range(1, Cin):
        acc += p[c]
    return acc.view(B, Cout, Ho, Wo)


_T = {0: ((1, 0), (3, -1)), 1: ((0, 1), (2, 0))}   # stride 2, pad 1: output row 2 i + p takes kernel row k from input row i + d


def conv_t32(g, w):
    """The data gradient of a stride-2 block the same way: the <= 4 taps of one output channel exact, the channels in a loop."""
    B, Cout, h, wd_ = g.shape
    gp, wd = F.pad(g.double(), (1, 1, 1, 1)), w.double()
    out = torch.empty(B, w.shape[1], 2 * h, 2 * wd_)
    for py in (0, 1):
        for px in (0, 1):
            gs = torch.stack([gp[:, :, 1 + dy:1 + dy + h, 1 + dx:1 + dx + wd_] for _, dy in _T[py] for _, dx in _T[px]])
            ws = torch.stack([wd[:, :, ky, kx] for ky, _ in _T[py] for kx, _ in _T[px]])
            p = torch.einsum("sboij,soc->obcij", gs, ws).float()
            acc = p[0].clone()
            for o in range(1, Cout):
                acc += p[o]
            out[:, :, py::2, px::2] = acc
    return out


def chain(wsd, x, dtype):
    """Every layer's pre-activation (the last one: the logits as (B, out_dim, 1, 1)): O.dc_discriminator's own expressions in
    float64, `conv32` in their place in float32."""
    us, a = [], x.to(dtype)
    for i, (w, stride, pad) in enumerate(_layers(wsd)):
        u = F.conv2d(a, w.to(dtype), stride=stride, padding=pad) if dtype == torch.float64 else conv32(a, w, stride, pad)
        us.append(u)
        a = F.leaky_relu(u, SLOPE)
    return us


def ref64(wsd, x):
    return chain(wsd, x, torch.float64)


def ref32(wsd, x):
    return chain(wsd, x, torch.float32)


def head_t32(cot, w):
    """The data gradient of the head (4 x 4 window, stride 1, no padding) for a cotangent (B, out_dim) on the logits: every
    product rounded once, the logits added in a plain float32 loop, in order."""
    p = (cot.double()[:, :, None, None, None] * w.double()[None]).float()   # (B, out_dim, C, 4, 4)
    acc = p[:, 0].clone()
    for o in range(1, p.shape[1]):
        acc += p[:, o]
    return acc


def grad32(wsd, us32, cot=None, per_layer=False):
    """d (logit 0 summed over the images) / d image along the float32 chain, in float32 throughout.  `cot`: a cotangent
    (B, out_dim) on the logits in place of the selection of logit 0.  `per_layer`: the gradient with respect to every
    layer's pre-activation instead, [d / d u_0, ..., d / d logits] (tests/helpers/disc_bwd_regimes.py)."""
    L = _layers(wsd)
    B = us32[0].shape[0]
    if cot is None:
        g = L[-1][0][0][None].expand(B, -1, -1, -1)   # through the head: its weights of logit 0
    else:
        g = head_t32(cot, L[-1][0])
    gs = [None if cot is None else cot.float().reshape(B, -1, 1, 1)]
    for l in range(len(L) - 2, -1, -1):
        g = g * torch.where(us32[l] > 0, 1.0, SLOPE)
        gs.append(g)
        g = conv_t32(g, L[l][0])
    return gs[::-1] if per_layer else g


def _trunc16(t):
    """fp32 -> the fp16 value towards zero (normal range)."""
    return (t.contiguous().view(torch.int32) & -8192).view(torch.float32).half().float()


def split(t, mutate=None):
    """fp32 -> (hi, lo) as float64: split_half / split8 of the kernels.  |t| >= 65520: hi = +-inf, lo = -+inf, as there."""
    t = t.float()
    if mutate == "bf16_limbs":
        hi = t.bfloat16().float()
        lo = (t - hi).bfloat16().float()
    else:
        hi = _trunc16(t) if mutate == "trunc_hi" else t.half().float()
        lo = (t - hi).half().float()
        if mutate == "flush_lo":
            lo = torch.where(lo.abs() < 2.0 ** -14, torch.zeros(()), lo)
    return hi.double(), lo.double()


def limb_conv(u, w, x_slope, stride, pad, mutate=None):
    """One convolution on limbs -> fp32 sums.  `u` fp32: the predecessor's sums (x_slope 0.2: its LeakyReLU is applied in fp32
    before the split, as conv4x4_tiled_f16x3_kernel and disc_large.hip's epilogues do) or an image (x_slope 1)."""
    if x_slope != 1.0 and mutate == "lrelu_after_split":
        xh, xl = (F.leaky_relu(t, x_slope) for t in split(u, mutate))
    else:
        xh, xl = split(u if (x_slope == 1.0 or mutate == "slope1_on_load") else F.leaky_relu(u.float(), x_slope), mutate)
    wh, wl = split(w, mutate)
    c = lambda a, b: F.conv2d(a, b, stride=stride, padding=pad)
    y = c(xh, wh)
    if mutate != "drop_xh_wl":
        y = y + c(xh, wl)
    if mutate != "drop_xl_wh":
        y = y + c(xl, wh)
    return y.float()


def exact_conv(u, w, x_slope, stride, pad):
    """An fp32 kernel with fp64 accumulation: exact products of the fp32 operands, one rounding."""
    a = u.float() if x_slope == 1.0 else F.leaky_relu(u.float(), x_slope)
    return F.conv2d(a.double(), w.double(), stride=stride, padding=pad).float()


def limb_model(wsd, x, kind, mutate=None):
    """The whole network as the route `kind` computes it -> every layer's fp32 sums."""
    assert kind in ("tiled", "large") and (mutate is None or mutate in MUTATIONS)
    L = _layers(wsd)
    us, u = [], x.float()
    for i, (w, stride, pad) in enumerate(L):
        x_slope = 1.0 if i == 0 else SLOPE
        head = i == len(L) - 1
        if kind == "tiled" and (i == 0 or head):
            u = exact_conv(u, w, x_slope, stride, pad)
        elif kind == "large" and head:   # dl_head_kernel: fp32(hi) + fp32(lo) times fp32 weights
            if mutate == "lrelu_after_split":
                hi, lo = (F.leaky_relu(t, SLOPE) for t in split(u, mutate))
            else:
                hi, lo = split(u if mutate == "slope1_on_load" else F.leaky_relu(u, SLOPE), mutate)
            u = F.conv2d((hi.float() + lo.float()).double(), w.double()).float()
        else:
            u = limb_conv(u, w, x_slope, stride, pad, mutate)
        us.append(u)
    return us


def limb_carried(us32, x, kind):
    """(P,) largest |value| that route `kind` carries on limbs, per image, from the float32 chain's sums."""
    acts = [x.float()] + [F.leaky_relu(u, SLOPE) for u in us32[:-1]]
    sel = acts[1:-1] if kind == "tiled" else acts
    return torch.stack([a.abs().flatten(1).max(1).values for a in sel]).max(0).values


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
def find_overflow_gain(spec, x):
    """The smallest gain on a grid of 0.25 at which every bright (even) image carries an input of blocks 1-3 above 65504, no
    input of any layer of a dim (odd) image reaches it, and the float32 chain is finite."""
    us = ref32(weights(spec, 1.0), x)
    top = float(limb_carried(us, x, "tiled")[0::2].min())
    g = math.floor((F16_MAX / top) ** (1.0 / 3.0) / 0.25) * 0.25   # (the input of block 3 grows as gain^3)
    for _ in range(16):
        us = ref32(weights(spec, g), x)
        t, l = limb_carried(us, x, "tiled"), limb_carried(us, x, "large")
        if bool((t[0::2] > F16_MAX).all()):
            assert bool((l[1::2] < F16_MAX).all()) and all(bool(torch.isfinite(u).all()) for u in us), g
            return g
        g += 0.25
    raise AssertionError("no gain reaches the fp16 range")


def _kink_keep(us64, us32, floors):
    """(B, 1, H, W) bool: the input pixels whose gradient no kink-adjacent activation reaches.  Kink-adjacent: the float32
    and float64 chains disagree on the sign, or |u| is within 3x the layer's fp32 floor of zero.  A sum that is exactly zero
    in both (`mask`: a window of zeros) is ON the kink in any arithmetic and stays in: the derivative there is the slope."""
    m = None
    for l in range(len(us64) - 2, -1, -1):
        near = (torch.sign(us64[l]) != torch.sign(us32[l].double())) | ((us64[l].abs() < 3 * floors[l] * rms(us64[l])) & (us64[l] != 0))
        near = near.any(1, keepdim=True).double()
        m = near if m is None else torch.clamp(near + m, max=1.0)
        m = (F.conv_transpose2d(m, torch.ones(1, 1, 4, 4, dtype=torch.float64), stride=2, padding=1) > 0).double()
    return m == 0


def _grad_case(wsd, x2):
    """d (logit 0 summed over the images) / d image in float64 (autograd) and the pixels that keep away from the kinks."""
    xx = x2.double().requires_grad_(True)
    us64 = chain(wsd, xx, torch.float64)
    g64, = torch.autograd.grad(us64[-1][:, :1].sum(), xx)
    us64 = [u.detach() for u in us64]
    us32 = ref32(wsd, x2)
    floors = [err(a, b, rms(b)) for a, b in zip(us32, us64)]
    return g64, us32, _kink_keep(us64, us32, floors)


GRAD_CAP = 0.005   # of the input pixels may be left out of the gradient comparison


@functools.lru_cache(maxsize=None)
def case(name):
    """The regime, built once, shared, never modified: weights `wsd`, pool images `x`, the float64 / float32 chains `u64` /
    `u32`, `ref` {key: float64 reference over the pool}, `scale` {key: its rms}, `inp` {per-layer key: fp32 input}, and for the
    64 x 64 networks `dx64` / `dx32` / `dx_keep` of pool images 0 and 1.  The seed moves on (by 1000) until the gradient
    comparison keeps GRAD_CAP."""
    spec0 = REGIMES[name]
    for attempt in range(20):
        spec = dict(spec0, seed=spec0["seed"] + 1000 * attempt)
        x = images(spec)
        gain = find_overflow_gain(spec, x) if name == "overflow" else None
        wsd = weights(spec, gain)
        c = {"name": name, "spec": spec, "gain": gain if gain is not None else spec["gain"], "wsd": wsd, "x": x}
        if spec["size"] == 64 and name != "overflow":
            c["dx64"], us32, c["dx_keep"] = _grad_case(wsd, x[:2])
            if 1.0 - float(c["dx_keep"].double().mean()) > GRAD_CAP:
                continue
            c["dx32"] = grad32(wsd, us32)
        break
    else:
        raise AssertionError(f"{name}: no seed keeps the gradient comparison's cap")
    c["u64"], c["u32"] = ref64(wsd, x), ref32(wsd, x)
    P = x.shape[0]
    c["ref"] = {"logits": c["u64"][-1].reshape(P, -1)}
    c["inp"] = {}
    if spec["size"] == 64 and name != "overflow":
        for key in LAYER_KEYS:
            l, s = int(key[1]), float(key[3:])
            w, stride, pad = _layers(wsd)[l]
            u = c["u32"][l - 1]
            c["inp"][key] = u
            c["ref"][key] = F.conv2d(u.double() if s == 1.0 else F.leaky_relu(u.double(), s), w.double(), stride=stride, padding=pad)
        keep = c["dx_keep"].expand_as(c["dx64"])
        c["ref"]["dx"] = c["dx64"]
        c["scale"] = {k: rms(v) for k, v in c["ref"].items()}
        c["scale"]["dx"] = rms(c["dx64"][keep])
    elif name == "overflow":
        c["over"] = {k: limb_carried(c["u32"], x, k) > F16_MAX for k in ("tiled", "large")}
        lg = c["ref"]["logits"]
        c["scale"] = {"logits_over": rms(lg[0::2]), "logits_under": rms(lg[1::2])}
    else:
        c["scale"] = {k: rms(v) for k, v in c["ref"].items()}
    return c


def layer_floor(c, key):
    l, s = int(key[1]), float(key[3:])
    w, stride, pad = _layers(c["wsd"])[l]
    u = c["inp"][key]
    return conv32(u if s == 1.0 else F.leaky_relu(u, s), w, stride, pad)


def layer_model(c, key, mutate=None):
    l, s = int(key[1]), float(key[3:])
    w, stride, pad = _layers(c["wsd"])[l]
    return limb_conv(c["inp"][key], w, s, stride, pad, mutate)


def _pop(key):
    """Pool images an overflow key is measured on."""
    return slice(0, None, 2) if key == "logits_over" else slice(1, None, 2)


def measure_floor(name):
    """{key: err(float32 chain, float64 chain)}."""
    c = case(name)
    P = c["x"].shape[0]
    lg = c["u32"][-1].reshape(P, -1)
    if name == "overflow":
        return {k: err(lg[_pop(k)], c["ref"]["logits"][_pop(k)], c["scale"][k]) for k in ("logits_over", "logits_under")}
    out = {"logits": err(lg, c["ref"]["logits"], c["scale"]["logits"])}
    if c["inp"]:
        for key in LAYER_KEYS:
            out[key] = err(layer_floor(c, key), c["ref"][key], c["scale"][key])
        keep = c["dx_keep"].expand_as(c["dx64"])
        out["dx"] = err(c["dx32"][keep], c["dx64"][keep], c["scale"]["dx"])
    return out


@functools.lru_cache(maxsize=None)
def model_outputs(name, kind, mutate=None):
    """{key: the limb model's fp32 output over the pool} of the route kind: "logits", and for "tiled" every per-layer key."""
    c = case(name)
    out = {"logits": limb_model(c["wsd"], c["x"], kind, mutate)[-1].reshape(c["x"].shape[0], -1)}
    if kind == "tiled" and c["inp"]:
        for key in LAYER_KEYS:
            out[key] = layer_model(c, key, mutate)
    return out


def measure_model(name, kind, mutate=None):
    """{key: err(limb model, float64 chain)} of the route kind; `mutate`: the same of a deliberately wrong model."""
    c = case(name)
    out = model_outputs(name, kind, mutate)
    if name == "overflow":
        return {"logits_under": err(out["logits"][1::2], c["ref"]["logits"][1::2], c["scale"]["logits_under"])}
    return {k: err(v, c["ref"][k], c["scale"][k]) for k, v in out.items()}


def bar(route, name, key):
    """3 x the committed fp32 floor (fp32 routes, the input gradient, an overflowing image), 3 x (model + floor) (limb routes)."""
    kind = ROUTES[route]["kind"]
    if kind == "fp32" or key in ("dx", "logits_over"):
        return 3.0 * FP32_FLOOR[name][key]
    return 3.0 * (LIMB_MODEL[kind][name][key] + FP32_FLOOR[name][key])


def judge(route, name, outputs):
    """-> list of messages, one per assertion of the GPU test that the candidate breaks.  `outputs`: {key: tensor over the
    images compare(B) of the route's batch}; keys "logits" (B', out_dim), "L<l>/<slope>" (B', C, H, W), "dx" (2, C, H, W)."""
    c = case(name)
    R = ROUTES[route]
    idx = torch.tensor(compare(R["B"])) % c["x"].shape[0]
    bad = []
    for key, y in outputs.items():
        y = y.detach().cpu()
        assert y.dtype == torch.float32, (key, y.dtype)
        if name == "overflow":
            assert key == "logits" and R["kind"] != "fp32"
            ref, over = c["ref"]["logits"][idx], c["over"][R["kind"]][idx]
            for j in range(len(idx)):
                k = "logits_over" if bool(over[j]) else "logits_under"
                assert bool(over[j]) == (int(idx[j]) % 2 == 0)
                b = bar(route, name, k)
                fin = torch.isfinite(y[j])
                e = float(((y[j].double() - ref[j]).abs() / c["scale"][k])[fin].max()) if bool(fin.any()) else 0.0
                if not bool(over[j]) and not bool(fin.all()):
                    bad.append(f"{key}: image {j} carries nothing above 65504, yet a logit is not finite")
                if e > b:
                    bad.append(f"{key}: image {j} ({'above' if bool(over[j]) else 'below'} 65504): a finite logit is off by {e:.3e}, bar {b:.3e}")
            continue
        if not bool(torch.isfinite(y).all()):
            bad.append(f"{key}: not finite")
            continue
        ref = c["ref"][key] if key == "dx" else c["ref"][key][idx]
        assert y.shape == ref.shape, (key, y.shape, ref.shape)
        if key == "dx":
            keep = c["dx_keep"].expand_as(ref)
            y, ref = y[keep], ref[keep]
        e, b = err(y, ref, c["scale"][key]), bar(route, name, key)
        if e > b:
            bad.append(f"{key}: error {e:.3e} above the bar {b:.3e}")
    return bad


# Mutations no regime can expose at the bar, with the arithmetic reason.
NOT_DETECTABLE = {
    "trunc_hi": "the lo limb takes up what a truncated hi limb leaves: the residual is at most 2^-10 |v| instead of 2^-11 |v| and lo "
                "holds it to 11 bits -- 2^-21 |v| instead of 2^-22 |v| where lo is normal, the same 2^-25 where it is subnormal "
                "(nine operands in ten): at most a factor of 2 on the model's error, inside the factor 3 of every bar",
}

# The envelope regimes in which the mutated model, judged as the GPU output is, fails on the whole-network routes of both limb
# kernels (tests/test_disc_regimes_cpu.py::test_mutation_is_caught demands every entry).  bf16 limbs (16 bits instead of 22) are
# 1-2x the bar where the lo limbs are subnormal anyway, and clearly above it from unit scale upwards.
_INSIDE = ("unit", "default_init", "white_bg", "mask", "grown3", "grown8")
CAUGHT_BY = {
    "drop_xl_wh": _INSIDE, "drop_xh_wl": _INSIDE, "flush_lo": _INSIDE, "lrelu_after_split": _INSIDE, "slope1_on_load": _INSIDE,
    "bf16_limbs": ("unit", "grown3", "grown8"),
}

# Measured by `measure_floor` / `measure_model` (every bit of both is defined: see conv32); tests/test_disc_regimes_cpu.py keeps
# a fresh computation within the last printed digit.  Keys: "logits" the whole chain, "L<block>/<x_slope>" one block fed from
# the float32 chain, "dx" the input gradient of pre_b2; `overflow`: the bright ("over") and the dim ("under") images.
FP32_FLOOR = {
    "unit": {"logits": 1.47e-06, "L1/1.0": 1.32e-06, "L1/0.2": 1.38e-06, "L2/1.0": 1.85e-06, "L2/0.2": 2.49e-06, "L3/1.0": 4.19e-06, "L3/0.2": 2.61e-06, "dx": 2.71e-06},
    "default_init": {"logits": 1.34e-06, "L1/1.0": 1.37e-06, "L1/0.2": 1.93e-06, "L2/1.0": 1.81e-06, "L2/0.2": 2.02e-06, "L3/1.0": 2.75e-06, "L3/0.2": 3.08e-06, "dx": 2.71e-06},
    "white_bg": {"logits": 2.21e-06, "L1/1.0": 1.77e-06, "L1/0.2": 1.59e-06, "L2/1.0": 1.99e-06, "L2/0.2": 1.81e-06, "L3/1.0": 2.78e-06, "L3/0.2": 3.65e-06, "dx": 2.86e-06},
    "mask": {"logits": 6.28e-07, "L1/1.0": 1.47e-06, "L1/0.2": 1.40e-06, "L2/1.0": 2.13e-06, "L2/0.2": 2.05e-06, "L3/1.0": 3.23e-06, "L3/0.2": 3.06e-06, "dx": 2.87e-06},
    "dark": {"logits": 1.61e-06, "L1/1.0": 1.42e-06, "L1/0.2": 1.75e-06, "L2/1.0": 2.45e-06, "L2/0.2": 2.15e-06, "L3/1.0": 2.51e-06, "L3/0.2": 2.86e-06, "dx": 3.04e-06},
    "shrunk": {"logits": 1.47e-06, "L1/1.0": 1.42e-06, "L1/0.2": 1.24e-06, "L2/1.0": 2.43e-06, "L2/0.2": 2.01e-06, "L3/1.0": 2.69e-06, "L3/0.2": 3.15e-06, "dx": 2.87e-06},
    "grown3": {"logits": 1.32e-06, "L1/1.0": 2.09e-06, "L1/0.2": 1.54e-06, "L2/1.0": 2.24e-06, "L2/0.2": 2.27e-06, "L3/1.0": 3.22e-06, "L3/0.2": 3.02e-06, "dx": 2.86e-06},
    "grown8": {"logits": 1.74e-06, "L1/1.0": 1.64e-06, "L1/0.2": 1.26e-06, "L2/1.0": 1.70e-06, "L2/0.2": 1.99e-06, "L3/1.0": 2.71e-06, "L3/0.2": 2.51e-06, "dx": 3.06e-06},
    "overflow": {"logits_over": 1.52e-06, "logits_under": 1.64e-06},
    "unit_128": {"logits": 9.16e-07},
    "default_init_128": {"logits": 1.54e-06},
}
LIMB_MODEL = {
    "tiled": {
        "unit": {"logits": 2.56e-06, "L1/1.0": 1.55e-06, "L1/0.2": 1.49e-06, "L2/1.0": 2.23e-06, "L2/0.2": 2.34e-06, "L3/1.0": 4.30e-06, "L3/0.2": 3.78e-06},
        "default_init": {"logits": 5.77e-06, "L1/1.0": 4.22e-06, "L1/0.2": 4.27e-06, "L2/1.0": 5.99e-06, "L2/0.2": 7.13e-06, "L3/1.0": 8.80e-06, "L3/0.2": 9.03e-06},
        "white_bg": {"logits": 6.27e-06, "L1/1.0": 3.57e-06, "L1/0.2": 4.11e-06, "L2/1.0": 5.75e-06, "L2/0.2": 5.93e-06, "L3/1.0": 9.48e-06, "L3/0.2": 8.76e-06},
        "mask": {"logits": 2.16e-06, "L1/1.0": 4.90e-06, "L1/0.2": 4.67e-06, "L2/1.0": 7.76e-06, "L2/0.2": 7.95e-06, "L3/1.0": 9.38e-06, "L3/0.2": 1.09e-05},
        "dark": {"logits": 4.13e-05, "L1/1.0": 6.48e-06, "L1/0.2": 9.55e-06, "L2/1.0": 1.50e-05, "L2/0.2": 2.01e-05, "L3/1.0": 3.51e-05, "L3/0.2": 4.89e-05},
        "shrunk": {"logits": 1.35e-05, "L1/1.0": 8.37e-06, "L1/0.2": 8.55e-06, "L2/1.0": 1.25e-05, "L2/0.2": 1.35e-05, "L3/1.0": 2.76e-05, "L3/0.2": 2.86e-05},
        "grown3": {"logits": 7.84e-07, "L1/1.0": 8.05e-07, "L1/0.2": 7.76e-07, "L2/1.0": 1.00e-06, "L2/0.2": 1.01e-06, "L3/1.0": 1.24e-06, "L3/0.2": 1.45e-06},
        "grown8": {"logits": 4.67e-07, "L1/1.0": 4.73e-07, "L1/0.2": 3.95e-07, "L2/1.0": 4.80e-07, "L2/0.2": 4.87e-07, "L3/1.0": 6.14e-07, "L3/0.2": 6.59e-07},
        "overflow": {"logits_under": 4.05e-07},
    },
    "large": {
        "unit": {"logits": 2.38e-06},
        "default_init": {"logits": 8.57e-06},
        "white_bg": {"logits": 7.15e-06},
        "mask": {"logits": 3.69e-06},
        "dark": {"logits": 9.20e-05},
        "shrunk": {"logits": 7.22e-05},
        "grown3": {"logits": 9.05e-07},
        "grown8": {"logits": 4.67e-07},
        "overflow": {"logits_under": 5.43e-06},
    },
}


def stats(name):
    """What the regime is: the range of the head's input, the share of limb operands (weights of blocks 1-3 and their inputs
    after the LeakyReLU) below 2^-3 (an fp16 lo limb is subnormal there and keeps fewer than 11 bits) and below 3e-4, the share
    of zero pixels."""
    c = case(name)
    acts = [F.leaky_relu(u, SLOPE) for u in c["u32"][:-1]]
    ops = torch.cat([t.abs().flatten() for t in acts[:-1]] + [w.abs().flatten() for w, _, _ in _layers(c["wsd"])[1:-1]])
    return {"head_in_max": float(acts[-1].abs().max()), "logit_rms": c["scale"].get("logits", 0.0),
            "below_2^-3": float((ops < 0.125).double().mean()), "below_3e-4": float((ops < 3e-4).double().mean()),
            "zero_pixels": float((c["x"] == 0).double().mean()), "one_pixels": float((c["x"] == 1).double().mean())}


def errors(route, name, outputs):
    """{key: measured err} of a candidate, as `judge` measures it (what the GPU test records and prints).  `overflow`: the
    worst FINITE logit of the bright ("logits_over"; 0.0 when none is finite) and of the dim images ("logits_under")."""
    c = case(name)
    idx = torch.tensor(compare(ROUTES[route]["B"])) % c["x"].shape[0]
    out = {}
    for key, y in outputs.items():
        y = y.detach().cpu()
        if name == "overflow":
            ref, over = c["ref"]["logits"][idx], c["over"][ROUTES[route]["kind"]][idx]
            for k, sel in (("logits_over", over), ("logits_under", ~over)):
                d = ((y[sel].double() - ref[sel]).abs() / c["scale"][k])
                fin = torch.isfinite(y[sel])
                out[k] = float(d[fin].max()) if bool(fin.any()) else 0.0
        elif key == "dx":
            keep = c["dx_keep"].expand_as(c["dx64"])
            out[key] = err(y[keep], c["dx64"][keep], c["scale"][key])
        else:
            out[key] = err(y, c["ref"][key][idx], c["scale"][key])
    return out


def block_shape(in_dim, layer):
    """(Cin, H, Cout) of block `layer` of the 64 x 64 network."""
    ch = (in_dim,) + CH[64]
    return ch[layer], 64 >> layer, ch[layer + 1]


def tiled_launch(B, Cin, H, Cout, stride=2, pad=1, any_scale=False):
    """oi_conv4x4_fwd_arena's choice (csrc/disc.hip), restated: (pixel tile, K splits) of conv4x4_tiled_f16x3_kernel, or None
    for the fp32 split-K kernel."""
    cdiv = lambda a, b: -(-a // b)
    Ho = (H + 2 * pad - 4) // stride + 1
    M, K = B * Ho * Ho, Cin * 16
    small = cdiv(M, 128) * (Cout // 64) < 256
    splits = 2 if (small and cdiv(M, 64) * (Cout // 64) < 192 and K >= 1024) else 1
    enough = cdiv(M, 64 if small else 128) * (Cout // 64) * splits >= 128
    if not any_scale and M >= 512 and enough and Cout % 64 == 0 and K % 64 == 0:
        return (64 if small else 128), splits
    return None
