"""The scalar tail of a training step -- csrc/loss.hip (oi_gan_losses_fwd / _bwd, oi_weighted_sum_*, oi_render_scalars_*,
oi_scalar_glue) and csrc/optim.hip with oi_amd/optim.py (FusedAdam, FusedRMSprop, ema_update) -- in the regimes a training
run reaches.  All plain torch on the CPU, nothing of oi_amd:

* restatements: `gan_losses`, `weighted_sum`, `render_scalars`, `scalar_glue`, `adam_step`, `rmsprop_step`, `ema_lerp`, each
  spelled out from the reference formulas (src/loss/gan.py:5-22,39-49, src/loss/position.py:4-18, renderer.py:404,430-448,
  lighting.py:50-60, torch's single-tensor adam.py / rmsprop.py, Tensor.lerp) so that a branch can be mutated.  Unmutated
  they are bit-identical, in float64 and float32, to F.binary_cross_entropy_with_logits / compute_grad2 / F.mse_loss and
  autograd, and to torch.optim.Adam / RMSprop(foreach=False) on CPU tensors (tests/test_step_tail_regimes_cpu.py).
  float64 is the reference, float32 the reference's own arithmetic noise (the "fp32 floor").
* `cells()` / `case(cell)`: every named, seeded cell with its inputs and both restatements; `judge`, `margins`, `bar`,
  `FP32_FLOOR`, `measure_floor`: what the GPU test asserts on a candidate's outputs, and the bars that follow from the floors.
* `MUTATIONS`, `CAUGHT_BY`, `NOT_DETECTABLE`: the plausible kernel / host errors and the cells that expose them.

What the arithmetic allows, and what the regimes do about it
------------------------------------------------------------
Saturated logits.  BCE against 1 is softplus(-x).  The naive log(1 + exp(x)) overflows float32 at x > 88.72 (exp) and
float64 never here; the kernel's form m + log(exp(-m) + exp(-x - m)), m = max(-x, 0), and its gradient 1 / (1 + exp(-x))
meet three thresholds: |x| ~ 16.6 (exp(-|x|) < 2^-24: 1 + exp rounds to 1, the loss of the "right" side is exactly 0 and its
gradient exactly 0 or -1), 88.72 (expf overflows: 1 / (1 + inf) must be 0, not NaN) and 103.97 (expf underflows to 0 even as a
denormal).  `saturated` places +-15, +-17, +-30, +-88, +-90, +-104 in column 0, the real logit and its negative as the fake
one, so every value meets both targets.  A batch smaller than 12 cannot hold them at once: `saturated@j` is the j-th window
of B of them, and the windows of one shape visit all twelve (ceil(12 / B) cells; only window 0 runs every term set, the others
the fullest one the shape allows).  Against max(1, |ref|) -- the project's measure -- the float32 loss is exact to ~4e-8
there and the gradient to 5e-8 (x = 15: 1 + exp(-15) rounds by 0.43 ulp of 1), half of the 1e-7 bar: B = 1, where no 1 / B
shrinks it, is the sharpest cell.
Tiny logits (|x| <= 1e-6): softplus = ln 2 + x / 2, sigmoid = 1 / 2 + x / 4: a form that loses x (e.g. log(2) exactly) is 5e-7
off in the loss, below its 2e-6 bar, but 2.5e-7 in the gradient, above 1e-7.
R1.  reg = mean_b sum_i gx^2: at N = 3 x 128 x 128 and B = 8 each of the 1,024 threads accumulates 384 products before the tree;
the gx regimes 1e-6 / 1 / 1e3 put reg_w x reg at 1e-7, 1e6 and 1e12 against BCE terms of ~1: the total is measured relative to
itself, the parts each on their own.  g_gx = (2 reg_w g / B) gx has no existing bar; its own chain is four roundings
(2.4e-7), the float32 restatement shows ~1e-7, so it is judged at the logit gradients' 1e-7 (or 3x floor) relative to its
largest element.
K = 1 shapes cannot carry a pose term and N = 0 no gx: the term sets that need them are not cells of those shapes.

Glue.  inv_s = clamp(exp(10 v), 1e-6, 1e6): ln(1e6) = 13.81551, so v = +-1.3815 is just inside and +-1.3816 just outside.
Every glue output and render-scalar gradient is its own "tensor", measured relative to |ref| (the existing test's
rtol = 2e-6, atol = 0) -- except `1 - ambient colour`, a difference of two O(1) numbers, measured relative to 1: at
ambient = 30 its float64 value is 9e-14 and every float32 evaluation is 0.  A reference of exactly 0 admits exactly 0.
render scalars: r4[1] = 0 leaves the bare 1e-5 (the float32 constant is 1e-8 relative from the double's), and the gradient
-g r4[0] / den^2 reaches 1e10 x r4[0].

Optimisers.  Gradients are fixed by seed and never depend on the parameters, so a trajectory cannot diverge: the error after
n steps is the sum of n roundings, not their amplification.  Distance is the project's: max |x - ref| / max(1, max |ref|) per
tensor, the worst tensor of the cell.  For that measure to see a RELATIVE error in a moment the moment must reach 1:
`ordinary`, `long` draw 8 x randn (exp_avg_sq ~ 3 at step 50 with beta2 = 0.999), `spike` reaches 1e5.
The complement of beta: torch hands lerp_ / addcmul_ the double 1 - beta, rounded once; 1.0f - (float)beta is 0.00099998713
for 0.999 (1.3e-5 relative), 0.100000024 for 0.9 (2.2e-7), 0.00999999 for 0.99 (1e-6).  exp_avg_sq inherits the factor
whole: that is mutation `complement_rounded`, visible at torch's defaults only.
`vanishing`: |g| in [1e-12, 1e-8], g^2 (1 - beta2) >= 1e-27 stays a normal float32; sqrt(v) is below eps = 1e-8 nearly
everywhere, so the step is lr x g / eps-like: `eps_inside_sqrt` moves the step by orders of magnitude there and by nothing
measurable in `ordinary`.
`zeros`: tensor 1 never sees a gradient other than 0 and every fifth element of the others neither; with a zero first moment
the update is 0 / (0 + eps) = 0 and p must keep its bits (Adam at any beta1 -- exp_avg stays 0 -- and RMSprop).
`late`: state loaded at step 999: bias_correction2 = 1 - 0.999^1000 = 0.632 still moves, 1 - 0.9^1000 is 1.  `skips`: one
parameter has no gradient on steps 2 and 5 of 8, so two bias-correction groups exist at once and its count lags by two.
"""
import functools
import math
import zlib

import numpy as np
import torch

# ----------------------------------------------------------------------------------------------------------------------
# the project's existing bars (tests/test_gpu_modules.py, tests/test_gpu_kernels.py) per kind of quantity
# ----------------------------------------------------------------------------------------------------------------------
PROJECT_BAR = {"param": 2e-7, "state": 1e-6, "loss": 2e-6, "logit_grad": 1e-7, "glue": 2e-6}
KIND = {"parts": "loss", "g_real": "logit_grad", "g_fake": "logit_grad", "g_gx": "logit_grad", "p": "param", "p_ema": "param",
        "exp_avg": "state", "exp_avg_sq": "state", "square_avg": "state", "total": "loss", "g_terms": "loss"}
GLUE_OUT = ("inv_s", "s_val", "ambient", "diffuse", "specular")
RS_OUT = ("gradient_error", "surface_loss", "g_r4_0", "g_r4_1", "g_r4_2", "g_r4_3")
for _n in GLUE_OUT + RS_OUT:
    KIND[_n] = "glue"
ABSOLUTE_GLUE = ("diffuse",)   # measured relative to 1 (module docstring)

LOSS_SHAPES = ((1, 1, 0), (1, 7, 3 * 64 * 64), (3, 1, 16 * 16), (5, 7, 1031), (64, 7, 48), (8, 1, 3 * 128 * 128))
LOGIT_REGIMES = ("balanced", "saturated", "tiny")
SATURATED = (15.0, -15.0, 17.0, -17.0, 30.0, -30.0, 88.0, -88.0, 90.0, -90.0, 104.0, -104.0)
GX_REGIMES = {"1e-6": 1e-6, "1": 1.0, "1e3": 1e3}
REG_W, AUX_W = 10.0, 0.37
TERM_SETS = ("real", "fake", "real+fake", "real+fake+pose", "real+fake+gx", "real+fake+pose+gx")
CAT_SHAPES = ((1, 7, 3 * 64 * 64), (3, 1, 256))

GLUE_VARIANCE = (-2.0, -1.3816, -1.3815, 0.0, 0.3, 1.3815, 1.3816, 2.0)
GLUE_AMBIENT = (-30.0, 0.0, 30.0)
GLUE_SPECULAR = (-0.2, 0.0, 0.7)
RS_R1 = (0.0, 1.0, 340.0)
RS_R0 = (0.0, 12.5)
WSUM_CASES = {"n=1": ((0.73,), (2.5,)), "n=1,w=0": ((0.73,), (0.0,)),
              "n=8": ((1e-8, 3.5e-5, 0.012, 0.9, 41.0, 2.7e3, 8.1e4, 1e6), (1.0, 0.1, 10.0, 0.0, -2.5, 1e-3, 0.5, 1.0))}

OPT_SIZES = (1, 7, 4095, 4096, 4097, 3 * 4096 + 5)   # plus one zero-element parameter (not in `long`)
HYPER = {"adam": {"config": dict(lr=2e-5, betas=(0.0, 0.9), eps=1e-8), "default": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)},
         "rmsprop": {"config": dict(lr=1e-4, alpha=0.99, eps=1e-8), "default": dict(lr=1e-2, alpha=0.99, eps=1e-8)}}
GRAD_REGIMES = {"ordinary": 50, "mixed": 10, "vanishing": 10, "spike": 30, "zeros": 10, "long": 200, "late": 3, "skips": 8}
LATE_STEP = 999
SKIP_TENSOR, SKIP_STEPS = 2, (2, 5)      # (1-based steps)
ZERO_TENSOR, ZERO_EVERY = 1, 5
EMA_BETAS = (0.0, 0.5, 0.999, 1.0)
EMA_UPDATES = 3

MUTATIONS = ("naive_softplus", "mean_BK", "pose_mean_B", "r1_no_div_B", "real_grad_no_minus1", "pose_grad_col0",
             "eps_inside_sqrt", "no_bc2", "bc_frozen", "skipped_step_advanced", "stale_grad", "complement_rounded",
             "lerp_swapped", "lerp_one_form", "glue_no_clamp", "rs_no_eps")


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


class _one_thread:
    """torch's sums must not depend on the machine's thread count (the float32 floors are committed)."""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *a):
        torch.set_num_threads(self.n)


# ----------------------------------------------------------------------------------------------------------------------
# restatements: losses
# ----------------------------------------------------------------------------------------------------------------------
def _softplus_neg_logsigmoid(x, mutate):
    """-log sigmoid(x) = softplus(-x).  torch evaluates log sigmoid as min(x, 0) - log1p(exp(-|x|)) with its own vectorised
    log1p, so the stable form is taken from F.logsigmoid itself (bit identity); the naive form is the mutation."""
    if mutate == "naive_softplus":
        return torch.log(1.0 + torch.exp(-x))
    return -torch.nn.functional.logsigmoid(x)


def _bce(x, target, B, K, mutate):
    """F.binary_cross_entropy_with_logits(x[:, :1], target): (1 - t) x - log sigmoid(x), mean over the B logits."""
    x0 = x[:, :1]
    loss = (1.0 - target) * x0 + _softplus_neg_logsigmoid(x0, mutate)
    return loss.sum() / (B * K if mutate == "mean_BK" else B)


def gan_losses(d_real, d_fake, pose, gx, aux_w, reg_w, dtype, mutate=None, g_total=1.0):
    """-> {"parts": [6] = (total, real + fake, reg, fake, real, aux), "g_real", "g_fake", "g_gx"} (absent terms: 0.0 in
    parts, None as gradient) in `dtype`.  total = BCE(d_real[:, :1], 1) + BCE(d_fake[:, :1], 0) + reg_w mean_b sum gx^2 +
    aux_w MSE(d_fake[:, 1:], pose); the gradients are those of g_total x total."""
    assert mutate is None or mutate in MUTATIONS, mutate
    c = lambda t: None if t is None else t.to(dtype)
    d_real, d_fake, pose, gx = c(d_real), c(d_fake), c(pose), c(gx)
    ref = d_real if d_real is not None else d_fake
    B, K = ref.shape
    zero = torch.zeros((), dtype=dtype)
    go = torch.tensor(g_total, dtype=dtype)
    real = _bce(d_real, 1.0, B, K, mutate) if d_real is not None else zero
    fake = _bce(d_fake, 0.0, B, K, mutate) if d_fake is not None else zero
    reg = zero
    if gx is not None and gx.numel():
        s = gx.pow(2).reshape(B, -1).sum(1)
        reg = s.sum() if mutate == "r1_no_div_B" else s.mean()
    aux = zero
    if pose is not None:
        diff = d_fake[:, 1:] - pose
        aux = (diff * diff).sum() / (B if mutate == "pose_mean_B" else B * (K - 1))
    total = real + fake
    if gx is not None and gx.numel():
        total = total + reg_w * reg
    if pose is not None:
        total = total + aux_w * aux
    out = {"parts": torch.stack([total, real + fake, reg, fake, real, aux]), "g_real": None, "g_fake": None, "g_gx": None}
    nb = B * K if mutate == "mean_BK" else B
    if d_real is not None:
        g = torch.zeros_like(d_real)
        sg = torch.sigmoid(d_real[:, 0])
        g[:, 0] = (sg if mutate == "real_grad_no_minus1" else sg - 1.0) * go / nb
        out["g_real"] = g
    if d_fake is not None:
        g = torch.zeros_like(d_fake)
        g[:, 0] = (torch.sigmoid(d_fake[:, 0]) - 0.0) * go / nb
        if pose is not None:
            n_aux = B if mutate == "pose_mean_B" else B * (K - 1)
            gp = (2.0 / n_aux) * (d_fake[:, 1:] - pose) * (go * aux_w)
            if mutate == "pose_grad_col0":
                g[:, :-1] += gp
            else:
                g[:, 1:] = gp
        out["g_fake"] = g
    if gx is not None and gx.numel():
        cg = go * reg_w if mutate == "r1_no_div_B" else go * reg_w / B
        out["g_gx"] = cg * (gx * 2.0)
    elif gx is not None:
        out["g_gx"] = torch.zeros_like(gx)
    return out


def weighted_sum(terms, weights, dtype, g_out=3.0):
    """-> {"total": sum_i w_i term_i, "g_terms": [n] = w_i g_out} (gan_pose_trainer.py:122-137)."""
    t = torch.tensor(terms, dtype=torch.float32).to(dtype)
    total = torch.zeros((), dtype=dtype)
    for v, w in zip(t, weights):
        total = total + v * w
    return {"total": total, "g_terms": torch.tensor(weights, dtype=torch.float32).to(dtype) * g_out}


def render_scalars(r4, inv_nt, dtype, g_err=2.0, g_surf=5.0, mutate=None):
    """gradient_error = r4[0] / (r4[1] + 1e-5), surface_loss = r4[2] inv_nt (renderer.py:430-446) and the gradient of
    g_err x gradient_error + g_surf x surface_loss with respect to r4."""
    r = r4.to(dtype)
    den = r[1] if mutate == "rs_no_eps" else r[1] + 1e-5
    return {"gradient_error": r[0] / den, "surface_loss": r[2] * inv_nt, "g_r4_0": g_err / den,
            "g_r4_1": -g_err * r[0] / (den * den), "g_r4_2": torch.tensor(g_surf * inv_nt, dtype=dtype),
            "g_r4_3": torch.zeros((), dtype=dtype)}


def scalar_glue(variance, ambient, specular, shininess, dtype, mutate=None):
    """inv_s = exp(10 variance).clamp(1e-6, 1e6) (renderer.py:404), its reciprocal, the ambient / diffuse colours sigmoid(a),
    1 - sigmoid(a) and the specular colour relu(s) (lighting.py:50-60); packed3 = the three light parameters as they are."""
    v, a, s = (torch.tensor(x, dtype=torch.float32).to(dtype) for x in (variance, ambient, specular))
    inv_s = torch.exp(v * 10.0)
    if mutate != "glue_no_clamp":
        inv_s = inv_s.clamp(1e-6, 1e6)
    amb = torch.sigmoid(a)
    return {"inv_s": inv_s, "s_val": 1.0 / inv_s, "ambient": amb, "diffuse": 1.0 - amb, "specular": s.clamp(min=0.0),
            "packed3": torch.tensor([ambient, specular, shininess], dtype=torch.float32)}


# ----------------------------------------------------------------------------------------------------------------------
# restatements: optimisers, EMA
# ----------------------------------------------------------------------------------------------------------------------
def _w(beta, mutate):
    """The complement handed to lerp_ / addcmul_: torch forms 1 - beta in double."""
    if mutate == "complement_rounded":
        return float(np.float32(1.0) - np.float32(beta))
    return 1 - beta


def adam_step(p, g, m, v, step, lr, betas, eps, mutate=None):
    """One step of torch's _single_tensor_adam (no weight decay / amsgrad), in place; `step` is the count AFTER this step."""
    b1, b2 = betas
    m.lerp_(g, _w(b1, mutate))
    v.mul_(b2).addcmul_(g, g, value=_w(b2, mutate))
    k = 1 if mutate == "bc_frozen" else step
    bias_correction1 = 1 - b1 ** k
    bias_correction2 = 1 - b2 ** k
    step_size = lr / bias_correction1
    bias_correction2_sqrt = 1.0 if mutate == "no_bc2" else bias_correction2 ** 0.5
    if mutate == "eps_inside_sqrt":
        denom = (v + eps).sqrt() / bias_correction2_sqrt
    else:
        denom = (v.sqrt() / bias_correction2_sqrt).add_(eps)
    p.addcdiv_(m, denom, value=-step_size)


def rmsprop_step(p, g, sq, lr, alpha, eps, mutate=None):
    """One step of torch's _single_tensor_rmsprop (no weight decay / momentum / centering), in place."""
    sq.mul_(alpha).addcmul_(g, g, value=_w(alpha, mutate))
    avg = (sq + eps).sqrt() if mutate == "eps_inside_sqrt" else sq.sqrt().add_(eps)
    p.addcdiv_(g, avg, value=-lr)


def ema_lerp(p_ema, p, beta, mutate=None):
    """p_ema <- p.lerp(p_ema, beta) (src/utils/ema.py:26-30); Tensor.lerp is a + w (b - a) below w = 0.5 and
    b - (b - a) (1 - w) from there on: exact at both ends."""
    if mutate == "lerp_swapped":
        return p_ema.lerp(p, beta)
    if mutate == "lerp_one_form":
        return p + beta * (p_ema - p)
    return p.lerp(p_ema, beta)


def opt_sizes(regime):
    return OPT_SIZES if regime == "long" else OPT_SIZES + (0,)


def opt_params(kind, hyper, regime):
    """Initial parameters (float32) of the cell."""
    g = torch.Generator().manual_seed(_seed(f"{kind}/{hyper}/{regime}/p"))
    return [torch.randn(n, generator=g) for n in opt_sizes(regime)]


def opt_initial_state(kind, hyper, regime):
    """None, or the state `late` is loaded with: (step, [s0], [s1 or None])."""
    if regime != "late":
        return None
    g = torch.Generator().manual_seed(_seed(f"{kind}/{hyper}/{regime}/state"))
    s0 = [torch.randn(n, generator=g) for n in opt_sizes(regime)]
    s1 = [torch.randn(n, generator=g) ** 2 for n in opt_sizes(regime)]
    if kind == "rmsprop":
        return LATE_STEP, s1, None
    return LATE_STEP, s0, s1


def opt_grads(kind, hyper, regime, t):
    """The float32 gradients of step t (1-based): a list with None for a parameter that has none."""
    g = torch.Generator().manual_seed(_seed(f"{kind}/{hyper}/{regime}/g") + 7919 * t)
    out = []
    for i, n in enumerate(opt_sizes(regime)):
        x = torch.randn(n, generator=g)
        u = torch.rand(n, generator=g)
        if regime in ("ordinary", "long"):
            x = 8.0 * x
        elif regime == "mixed":
            mag = torch.rand(n, generator=torch.Generator().manual_seed(_seed(f"mag{i}")))   # fixed per element
            x = x * 10.0 ** (-6.0 + 9.0 * mag)
        elif regime == "vanishing":
            x = torch.where(x >= 0, 1.0, -1.0) * 10.0 ** (-12.0 + 4.0 * u)
        elif regime == "spike":
            x = torch.where(x >= 0, 1e4, -1e4) if t == 21 else 1e-3 * x
        elif regime == "zeros":
            if i == ZERO_TENSOR:
                x = torch.zeros(n)
            else:
                x[::ZERO_EVERY] = 0.0
        if regime == "skips" and i == SKIP_TENSOR and t in SKIP_STEPS:
            x = None
        out.append(x)
    return out


def run_optimizer(kind, hyper, regime, dtype, mutate=None):
    """The whole trajectory of one cell in `dtype` -> {"p": [...], state tensors, "step": [...]}."""
    assert mutate is None or mutate in MUTATIONS, mutate
    h = HYPER[kind][hyper]
    p = [t.to(dtype) for t in opt_params(kind, hyper, regime)]
    init = opt_initial_state(kind, hyper, regime)
    if init is None:
        steps = [0] * len(p)
        s0 = [torch.zeros_like(t) for t in p]
        s1 = [torch.zeros_like(t) for t in p]
    else:
        steps = [init[0]] * len(p)
        s0 = [t.to(dtype) for t in init[1]]
        s1 = [torch.zeros_like(t) for t in p] if init[2] is None else [t.to(dtype) for t in init[2]]
    prev = None
    for t in range(1, GRAD_REGIMES[regime] + 1):
        grads = opt_grads(kind, hyper, regime, t)
        used = grads
        if mutate == "stale_grad" and prev is not None:   # the descriptor table still points at the previous gradients
            used = [a if (a is None or b is None) else b for a, b in zip(grads, prev)]
        for i, g in enumerate(used):
            if g is None:
                if mutate == "skipped_step_advanced":
                    steps[i] += 1
                continue
            steps[i] += 1
            g = g.to(dtype)
            if kind == "adam":
                adam_step(p[i], g, s0[i], s1[i], steps[i], h["lr"], h["betas"], h["eps"], mutate)
            else:
                rmsprop_step(p[i], g, s0[i], h["lr"], h["alpha"], h["eps"], mutate)
        prev = grads
    if kind == "adam":
        return {"p": p, "exp_avg": s0, "exp_avg_sq": s1, "step": steps}
    return {"p": p, "square_avg": s0, "step": steps}


def ema_sequence(beta):
    """(initial p_ema, [p of update 1..3]) as float32 lists."""
    g = torch.Generator().manual_seed(_seed(f"ema/{beta}"))
    sizes = OPT_SIZES + (0,)
    return [torch.randn(n, generator=g) for n in sizes], [[torch.randn(n, generator=g) for n in sizes] for _ in range(EMA_UPDATES)]


def run_ema(beta, dtype, mutate=None):
    pe, seq = ema_sequence(beta)
    pe = [t.to(dtype) for t in pe]
    for ps in seq:
        pe = [ema_lerp(a, b.to(dtype), beta, mutate) for a, b in zip(pe, ps)]
    return {"p_ema": pe}


# ----------------------------------------------------------------------------------------------------------------------
# cells
# ----------------------------------------------------------------------------------------------------------------------
def shape_name(s):
    return "x".join(str(v) for v in s)


def n_windows(B):
    return 1 if B >= len(SATURATED) else -(-len(SATURATED) // B)


def term_sets(shape):
    B, K, N = shape
    return tuple(t for t in TERM_SETS if ("pose" not in t or K > 1) and ("gx" not in t or N > 0))


def loss_cells():
    out = []
    for shape in LOSS_SHAPES:
        sets = term_sets(shape)
        for logit in LOGIT_REGIMES:
            for j in range(n_windows(shape[0]) if logit == "saturated" else 1):
                lname = f"{logit}@{j}" if logit == "saturated" else logit
                for ts in (sets if j == 0 else sets[-1:]):
                    for gxr in (GX_REGIMES if "gx" in ts else ("-",)):
                        if j > 0 and gxr not in ("-", "1"):
                            continue
                        out.append(f"loss/{shape_name(shape)}/{lname}/{ts}/{gxr}")
    return out


def cat_cells():
    out = []
    for shape in CAT_SHAPES:
        ts = term_sets(shape)[-1]
        for logit in ("balanced", "saturated@0", "tiny"):
            out.append(f"cat/{shape_name(shape)}/{logit}/{ts}/1")
    return out


def glue_cells():
    return [f"glue/{v}/{GLUE_AMBIENT[i % 3]}/{GLUE_SPECULAR[i % 3]}" for i, v in enumerate(GLUE_VARIANCE)]


def rs_cells():
    return [f"rs/{r0}/{r1}" for r1 in RS_R1 for r0 in RS_R0]


def wsum_cells():
    return [f"wsum/{k}" for k in WSUM_CASES]


def opt_cells():
    return [f"{kind}/{hyper}/{regime}" for kind in ("adam", "rmsprop") for hyper in ("config", "default") for regime in GRAD_REGIMES]


def ema_cells():
    return [f"ema/{b}" for b in EMA_BETAS]


def cells():
    return loss_cells() + cat_cells() + glue_cells() + rs_cells() + wsum_cells() + opt_cells() + ema_cells()


def _logits(shape, lname, g):
    """(d_real, d_fake) [B, K] float32 of one logit regime."""
    B, K, _ = shape
    dr, df = torch.rand(B, K, generator=g) * 6 - 3, torch.rand(B, K, generator=g) * 6 - 3
    if lname == "tiny":
        dr, df = dr * (1e-6 / 3), df * (1e-6 / 3)
    elif lname.startswith("saturated"):
        j = int(lname.split("@")[1])
        for b in range(min(B, len(SATURATED))):
            v = SATURATED[(j * B + b) % len(SATURATED)]
            dr[b, 0], df[b, 0] = v, -v
    return dr, df


def loss_inputs(cell):
    """The float32 inputs of a loss / cat cell: dict(d_real, d_fake, pose, gx, shape) with None for absent terms."""
    fam, sname, lname, ts, gxr = cell.split("/")
    shape = tuple(int(v) for v in sname.split("x"))
    B, K, N = shape
    g = torch.Generator().manual_seed(_seed(cell))
    dr, df = _logits(shape, lname, g)
    terms = ts.split("+")
    pose = torch.randn(B, K - 1, generator=g) if "pose" in terms else None
    gx = torch.randn(B, N, generator=g) * GX_REGIMES[gxr] if "gx" in terms else None
    return {"d_real": dr if "real" in terms else None, "d_fake": df if "fake" in terms else None, "pose": pose, "gx": gx,
            "shape": shape}


def restate(cell, dtype, mutate=None):
    """The restatement's outputs of a cell in `dtype` (with one error built in: `mutate`)."""
    fam = cell.split("/")[0]
    with _one_thread():
        if fam in ("loss", "cat"):
            i = loss_inputs(cell)
            return gan_losses(i["d_real"], i["d_fake"], i["pose"], i["gx"], AUX_W, REG_W, dtype, mutate)
        if fam == "glue":
            v, a, s = (float(x) for x in cell.split("/")[1:])
            return scalar_glue(v, a, s, 10.0, dtype, mutate)
        if fam == "rs":
            r0, r1 = (float(x) for x in cell.split("/")[1:])
            return render_scalars(torch.tensor([r0, r1, 7.25, 0.0]), 1.0 / 4096.0, dtype, mutate=mutate)
        if fam == "wsum":
            return weighted_sum(*WSUM_CASES[cell.split("/")[1]], dtype)
        if fam in ("adam", "rmsprop"):
            _, hyper, regime = cell.split("/")
            return run_optimizer(fam, hyper, regime, dtype, mutate)
        if fam == "ema":
            return run_ema(float(cell.split("/")[1]), dtype, mutate)
    raise KeyError(cell)


@functools.lru_cache(maxsize=16)
def case(cell):
    """{"r64", "r32"}: both restatements of the cell, computed once, never modified."""
    return {"r64": restate(cell, torch.float64), "r32": restate(cell, torch.float32)}


# ----------------------------------------------------------------------------------------------------------------------
# the judgement of a candidate (the kernels' outputs on the GPU, a mutated float32 restatement on the CPU)
# ----------------------------------------------------------------------------------------------------------------------
def _as_list(x):
    return x if isinstance(x, (list, tuple)) else [x]


def distance(name, got, ref):
    """The project's measure: the worst, over the tensors of `got`, of max |x - ref| / max(1, max |ref|).  Glue outputs:
    relative to |ref| (ABSOLUTE_GLUE: to 1; a reference of exactly 0: absolute).  inf for a non-finite or missing output."""
    worst = 0.0
    for x, r in zip(_as_list(got), _as_list(ref)):
        if r is None or r.numel() == 0:
            continue
        if x is None:
            return math.inf
        x, r = x.detach().double().cpu().reshape(-1), r.detach().double().reshape(-1)
        if x.shape != r.shape or not bool(torch.isfinite(x).all()):
            return math.inf
        scale = max(1.0, float(r.abs().max()))
        if KIND[name] == "glue":
            scale = 1.0 if (name in ABSOLUTE_GLUE or float(r.abs().max()) == 0.0) else float(r.abs().max())
        worst = max(worst, float((x - r).abs().max()) / scale)
    return worst


def tensors_of(cell):
    """The judged tensors of a cell (those its float64 restatement holds)."""
    r = case(cell)["r64"]
    return [k for k, v in r.items() if k in KIND and v is not None]


def bar(cell, name):
    """The larger of the project's existing bar for that kind of quantity and 3x the committed float32 floor
    (tests/conftest.py: "<= 3x the native-fp32 error")."""
    return max(PROJECT_BAR[KIND[name]], 3.0 * FP32_FLOOR[cell][name])


def margins(cell, got):
    """{tensor: distance / bar} of a candidate's outputs."""
    r = case(cell)["r64"]
    return {k: distance(k, got.get(k), r[k]) / bar(cell, k) for k in tensors_of(cell)}


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                      b.view(torch.int32) if b.dtype == torch.float32 else b)


def structural(cell, got):
    """The exact assertions -> list of messages."""
    bad = []
    fam = cell.split("/")[0]
    r64 = case(cell)["r64"]
    if fam in ("loss", "cat"):
        i = loss_inputs(cell)
        parts = got["parts"].detach().cpu()
        absent = {"real": (4,), "fake": (3,), "pose": (5,), "gx": (2,)}
        for term, key in (("real", "d_real"), ("fake", "d_fake"), ("pose", "pose"), ("gx", "gx")):
            if i[key] is None:
                for s in absent[term]:
                    if float(parts[s]) != 0.0:
                        bad.append(f"parts[{s}] = {float(parts[s])} although the {term} term is absent")
        for gname, key in (("g_real", "d_real"), ("g_fake", "d_fake"), ("g_gx", "gx")):
            if i[key] is None and got.get(gname) is not None:
                bad.append(f"{gname} exists although {key} is absent")
    elif fam == "glue":
        if not _bits_equal(got["packed3"], r64["packed3"]):
            bad.append("packed3 is not its inputs, bit for bit")
    elif fam in ("adam", "rmsprop"):
        _, hyper, regime = cell.split("/")
        if [int(s) for s in got["step"]] != list(r64["step"]):
            bad.append(f"step counts {[int(s) for s in got['step']]} against {list(r64['step'])}")
        sq = "exp_avg_sq" if fam == "adam" else "square_avg"
        if any(bool((t.detach().cpu() < 0).any()) for t in got[sq]):
            bad.append(f"{sq} < 0")
        if regime == "zeros":
            p0 = opt_params(fam, hyper, regime)
            if not _bits_equal(got["p"][ZERO_TENSOR], p0[ZERO_TENSOR]):
                bad.append("the parameter whose gradient is always 0 moved")
            for k, (a, b) in enumerate(zip(got["p"], p0)):
                if k != ZERO_TENSOR and not _bits_equal(a.detach().cpu()[::ZERO_EVERY].contiguous(), b[::ZERO_EVERY].contiguous()):
                    bad.append(f"elements of parameter {k} whose gradient is always 0 moved")
    elif fam == "ema":
        beta = float(cell.split("/")[1])
        pe0, seq = ema_sequence(beta)
        if beta == 1.0 and not all(_bits_equal(a, b) for a, b in zip(got["p_ema"], pe0)):
            bad.append("beta = 1 changed p_ema")
        if beta == 0.0 and not all(_bits_equal(a, b) for a, b in zip(got["p_ema"], seq[-1])):
            bad.append("beta = 0 did not leave p_ema bit-equal to p")
    return bad


def judge(cell, got, factor=1.0):
    """-> list of (kind, message) of every assertion of the GPU test that the candidate breaks: "structural" (exact) and
    "value" (distance from the float64 restatement above `factor` x bar; a non-finite output has distance inf).  The CPU
    rehearsal demands that a mutation misses the bar by a factor of 3."""
    bad = [("structural", m) for m in structural(cell, got)]
    for k, m in margins(cell, got).items():
        if not m <= factor:
            bad.append(("value", f"{k}: {m:.3g} x bar ({bar(cell, k):.3e})"))
    return bad


def measure_floor(cell):
    """{tensor: distance of the float32 restatement from the float64 one}."""
    c = case(cell)
    return {k: distance(k, c["r32"][k], c["r64"][k]) for k in tensors_of(cell)}


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
# Which cells catch which mutation (a mutated float32 restatement judged as the GPU output is, bar x 3):
# tests/test_step_tail_regimes_cpu.py::test_mutation_is_caught demands every entry.
CAUGHT_BY = {
    "naive_softplus": ("loss/1x1x0/saturated@8/real+fake/-", "loss/1x7x12288/saturated@9/real+fake+pose+gx/1",
                       "loss/64x7x48/saturated@0/real/-", "loss/8x1x49152/saturated@1/real+fake+gx/1"),
    "mean_BK": ("loss/1x7x12288/balanced/real/-", "loss/5x7x1031/balanced/real+fake+pose+gx/1", "loss/64x7x48/tiny/fake/-"),
    "pose_mean_B": ("loss/1x7x12288/balanced/real+fake+pose/-", "loss/5x7x1031/tiny/real+fake+pose+gx/1e-6",
                    "loss/64x7x48/balanced/real+fake+pose/-"),
    "r1_no_div_B": ("loss/3x1x256/balanced/real+fake+gx/1", "loss/5x7x1031/balanced/real+fake+pose+gx/1e3",
                    "loss/8x1x49152/tiny/real+fake+gx/1", "cat/3x1x256/balanced/real+fake+gx/1"),
    "real_grad_no_minus1": ("loss/1x1x0/balanced/real/-", "loss/1x7x12288/tiny/real+fake/-", "loss/8x1x49152/balanced/real+fake+gx/1"),
    "pose_grad_col0": ("loss/1x7x12288/balanced/real+fake+pose/-", "loss/64x7x48/tiny/real+fake+pose+gx/1",
                       "cat/1x7x12288/balanced/real+fake+pose+gx/1"),
    "eps_inside_sqrt": ("adam/config/vanishing", "adam/default/vanishing", "rmsprop/config/vanishing", "rmsprop/default/vanishing"),
    "no_bc2": ("adam/config/ordinary", "adam/default/ordinary", "adam/default/late", "adam/config/skips"),
    "bc_frozen": ("adam/config/ordinary", "adam/default/long", "adam/default/late", "adam/default/spike"),
    "skipped_step_advanced": ("adam/config/skips", "adam/default/skips", "rmsprop/config/skips"),
    "stale_grad": ("adam/config/ordinary", "adam/default/mixed", "rmsprop/config/spike", "rmsprop/default/zeros"),
    "complement_rounded": ("adam/default/ordinary", "adam/default/mixed", "adam/default/spike"),
    "lerp_swapped": ("ema/0.0", "ema/0.999", "ema/1.0"),
    "lerp_one_form": ("ema/1.0",),
    "glue_no_clamp": ("glue/-2.0/-30.0/-0.2", "glue/-1.3816/0.0/0.0", "glue/1.3816/-30.0/-0.2", "glue/2.0/0.0/0.0"),
    "rs_no_eps": ("rs/0.0/0.0", "rs/12.5/0.0", "rs/12.5/1.0"),
}

# Mutations no cell can expose at the bar, with the reason.
NOT_DETECTABLE = {}

# Measured by `measure_floor` (torch CPU, one thread); tests/test_step_tail_regimes_cpu.py keeps a fresh measurement within
# 1.5x of these.  FP32_FLOOR[cell][tensor].
FP32_FLOOR = {
    "loss/1x1x0/balanced/real/-": {"parts": 1.082e-08, "g_real": 1.730e-08},
    "loss/1x1x0/balanced/fake/-": {"parts": 3.787e-10, "g_fake": 4.958e-08},
    "loss/1x1x0/balanced/real+fake/-": {"parts": 1.021e-08, "g_real": 9.879e-09, "g_fake": 1.382e-08},
    "loss/1x1x0/saturated@0/real/-": {"parts": 1.197e-14, "g_real": 5.173e-08},
    "loss/1x1x0/saturated@0/fake/-": {"parts": 3.059e-07, "g_fake": 6.396e-15},
    "loss/1x1x0/saturated@0/real+fake/-": {"parts": 3.059e-07, "g_real": 5.173e-08, "g_fake": 6.396e-15},
    "loss/1x1x0/saturated@1/real+fake/-": {"parts": 2.039e-08, "g_real": 7.879e-09, "g_fake": 5.173e-08},
    "loss/1x1x0/saturated@2/real+fake/-": {"parts": 4.140e-08, "g_real": 4.140e-08, "g_fake": 2.674e-15},
    "loss/1x1x0/saturated@3/real+fake/-": {"parts": 2.435e-09, "g_real": 1.821e-08, "g_fake": 4.140e-08},
    "loss/1x1x0/saturated@4/real+fake/-": {"parts": 9.237e-14, "g_real": 9.348e-14, "g_fake": 6.210e-21},
    "loss/1x1x0/saturated@5/real+fake/-": {"parts": 3.079e-15, "g_real": 9.359e-14, "g_fake": 9.348e-14},
    "loss/1x1x0/saturated@6/real+fake/-": {"parts": 4.102e-46, "g_real": 0.000e+00, "g_fake": 4.102e-46},
    "loss/1x1x0/saturated@7/real+fake/-": {"parts": 0.000e+00, "g_real": 0.000e+00, "g_fake": 0.000e+00},
    "loss/1x1x0/saturated@8/real+fake/-": {"parts": 3.932e-46, "g_real": 0.000e+00, "g_fake": 8.194e-40},
    "loss/1x1x0/saturated@9/real+fake/-": {"parts": 0.000e+00, "g_real": 0.000e+00, "g_fake": 0.000e+00},
    "loss/1x1x0/saturated@10/real+fake/-": {"parts": 6.814e-46, "g_real": 0.000e+00, "g_fake": 6.814e-46},
    "loss/1x1x0/saturated@11/real+fake/-": {"parts": 0.000e+00, "g_real": 0.000e+00, "g_fake": 0.000e+00},
    "loss/1x1x0/tiny/real/-": {"parts": 9.110e-09, "g_real": 2.620e-08},
    "loss/1x1x0/tiny/fake/-": {"parts": 3.559e-08, "g_fake": 4.086e-08},
    "loss/1x1x0/tiny/real+fake/-": {"parts": 4.237e-08, "g_real": 2.175e-10, "g_fake": 3.236e-08},
    "loss/1x7x12288/balanced/real/-": {"parts": 5.756e-10, "g_real": 3.404e-08},
    "loss/1x7x12288/balanced/fake/-": {"parts": 4.554e-08, "g_fake": 1.572e-08},
    "loss/1x7x12288/balanced/real+fake/-": {"parts": 1.603e-08, "g_real": 1.431e-08, "g_fake": 9.667e-09},
    "loss/1x7x12288/balanced/real+fake+pose/-": {"parts": 3.410e-08, "g_real": 8.878e-09, "g_fake": 2.186e-08},
    "loss/1x7x12288/balanced/real+fake+gx/1e-6": {"parts": 4.501e-08, "g_real": 4.816e-09, "g_fake": 1.887e-08, "g_gx": 3.638e-12},
    "loss/1x7x12288/balanced/real+fake+gx/1": {"parts": 1.060e-07, "g_real": 1.338e-08, "g_fake": 6.774e-09, "g_gx": 4.888e-08},
    "loss/1x7x12288/balanced/real+fake+gx/1e3": {"parts": 1.170e-08, "g_real": 2.501e-08, "g_fake": 2.248e-08, "g_gx": 4.219e-08},
    "loss/1x7x12288/balanced/real+fake+pose+gx/1e-6": {"parts": 2.096e-08, "g_real": 4.363e-08, "g_fake": 2.960e-08, "g_gx": 3.638e-12},
    "loss/1x7x12288/balanced/real+fake+pose+gx/1": {"parts": 3.249e-08, "g_real": 3.685e-08, "g_fake": 3.576e-08, "g_gx": 4.372e-08},
    "loss/1x7x12288/balanced/real+fake+pose+gx/1e3": {"parts": 3.866e-08, "g_real": 2.306e-08, "g_fake": 2.186e-08, "g_gx": 4.756e-08},
    "loss/1x7x12288/saturated@0/real/-": {"parts": 1.197e-14, "g_real": 5.173e-08},
    "loss/1x7x12288/saturated@0/fake/-": {"parts": 3.059e-07, "g_fake": 6.396e-15},
    "loss/1x7x12288/saturated@0/real+fake/-": {"parts": 3.059e-07, "g_real": 5.173e-08, "g_fake": 6.396e-15},
    "loss/1x7x12288/saturated@0/real+fake+pose/-": {"parts": 8.597e-08, "g_real": 5.173e-08, "g_fake": 1.011e-08},
    "loss/1x7x12288/saturated@0/real+fake+gx/1e-6": {"parts": 3.059e-07, "g_real": 5.173e-08, "g_fake": 6.396e-15, "g_gx": 3.638e-12},
    "loss/1x7x12288/saturated@0/real+fake+gx/1": {"parts": 3.815e-08, "g_real": 5.173e-08, "g_fake": 6.396e-15, "g_gx": 4.535e-08},
    "loss/1x7x12288/saturated@0/real+fake+gx/1e3": {"parts": 7.085e-08, "g_real": 5.173e-08, "g_fake": 6.396e-15, "g_gx": 4.650e-08},
    "loss/1x7x12288/saturated@0/real+fake+pose+gx/1e-6": {"parts": 3.059e-07, "g_real": 5.173e-08, "g_fake": 1.291e-08, "g_gx": 3.638e-12},
    "loss/1x7x12288/saturated@0/real+fake+pose+gx/1": {"parts": 3.958e-08, "g_real": 5.173e-08, "g_fake": 1.828e-08, "g_gx": 4.526e-08},
    "loss/1x7x12288/saturated@0/real+fake+pose+gx/1e3": {"parts": 9.332e-08, "g_real": 5.173e-08, "g_fake": 7.947e-09, "g_gx": 4.527e-08},
    "loss/1x7x12288/saturated@1/real+fake+pose+gx/1": {"parts": 3.596e-08, "g_real": 7.879e-09, "g_fake": 5.173e-08, "g_gx": 5.222e-08},
    "loss/1x7x12288/saturated@2/real+fake+pose+gx/1": {"parts": 2.430e-08, "g_real": 4.140e-08, "g_fake": 3.691e-08, "g_gx": 5.289e-08},
    "loss/1x7x12288/saturated@3/real+fake+pose+gx/1": {"parts": 3.007e-08, "g_real": 1.821e-08, "g_fake": 4.140e-08, "g_gx": 5.038e-08},
    "loss/1x7x12288/saturated@4/real+fake+pose+gx/1": {"parts": 4.843e-08, "g_real": 9.348e-14, "g_fake": 3.646e-08, "g_gx": 4.728e-08},
    "loss/1x7x12288/saturated@5/real+fake+pose+gx/1": {"parts": 4.149e-08, "g_real": 9.359e-14, "g_fake": 2.075e-08, "g_gx": 4.902e-08},
    "loss/1x7x12288/saturated@6/real+fake+pose+gx/1": {"parts": 2.017e-08, "g_real": 0.000e+00, "g_fake": 1.878e-08, "g_gx": 5.084e-08},
    "loss/1x7x12288/saturated@7/real+fake+pose+gx/1": {"parts": 4.401e-08, "g_real": 0.000e+00, "g_fake": 2.126e-08, "g_gx": 3.523e-08},
    "loss/1x7x12288/saturated@8/real+fake+pose+gx/1": {"parts": 1.082e-09, "g_real": 0.000e+00, "g_fake": 4.768e-09, "g_gx": 4.580e-08},
    "loss/1x7x12288/saturated@9/real+fake+pose+gx/1": {"parts": 6.533e-08, "g_real": 0.000e+00, "g_fake": 2.801e-08, "g_gx": 4.717e-08},
    "loss/1x7x12288/saturated@10/real+fake+pose+gx/1": {"parts": 5.417e-08, "g_real": 0.000e+00, "g_fake": 3.194e-08, "g_gx": 5.283e-08},
    "loss/1x7x12288/saturated@11/real+fake+pose+gx/1": {"parts": 5.396e-08, "g_real": 0.000e+00, "g_fake": 1.495e-08, "g_gx": 3.758e-08},
    "loss/1x7x12288/tiny/real/-": {"parts": 2.522e-09, "g_real": 2.949e-08},
    "loss/1x7x12288/tiny/fake/-": {"parts": 4.253e-08, "g_fake": 7.583e-09},
    "loss/1x7x12288/tiny/real+fake/-": {"parts": 1.161e-08, "g_real": 7.092e-09, "g_fake": 7.813e-09},
    "loss/1x7x12288/tiny/real+fake+pose/-": {"parts": 2.621e-08, "g_real": 6.470e-09, "g_fake": 1.424e-08},
    "loss/1x7x12288/tiny/real+fake+gx/1e-6": {"parts": 4.309e-08, "g_real": 1.903e-08, "g_fake": 1.117e-08, "g_gx": 3.638e-12},
    "loss/1x7x12288/tiny/real+fake+gx/1": {"parts": 7.687e-08, "g_real": 1.738e-08, "g_fake": 1.679e-08, "g_gx": 5.039e-08},
    "loss/1x7x12288/tiny/real+fake+gx/1e3": {"parts": 6.829e-08, "g_real": 2.232e-08, "g_fake": 1.370e-08, "g_gx": 5.128e-08},
    "loss/1x7x12288/tiny/real+fake+pose+gx/1e-6": {"parts": 4.327e-08, "g_real": 2.823e-09, "g_fake": 3.455e-08, "g_gx": 3.638e-12},
    "loss/1x7x12288/tiny/real+fake+pose+gx/1": {"parts": 3.795e-08, "g_real": 4.226e-09, "g_fake": 5.106e-09, "g_gx": 5.080e-08},
    "loss/1x7x12288/tiny/real+fake+pose+gx/1e3": {"parts": 6.848e-09, "g_real": 3.187e-09, "g_fake": 8.362e-09, "g_gx": 3.947e-08},
    "loss/3x1x256/balanced/real/-": {"parts": 1.104e-09, "g_real": 1.617e-08},
    "loss/3x1x256/balanced/fake/-": {"parts": 1.557e-08, "g_fake": 3.707e-09},
    "loss/3x1x256/balanced/real+fake/-": {"parts": 6.393e-08, "g_real": 9.194e-09, "g_fake": 7.602e-09},
    "loss/3x1x256/balanced/real+fake+gx/1e-6": {"parts": 1.236e-08, "g_real": 1.734e-08, "g_fake": 1.774e-08, "g_gx": 1.213e-12},
    "loss/3x1x256/balanced/real+fake+gx/1": {"parts": 9.133e-08, "g_real": 8.029e-09, "g_fake": 5.068e-09, "g_gx": 5.591e-08},
    "loss/3x1x256/balanced/real+fake+gx/1e3": {"parts": 5.999e-08, "g_real": 1.504e-08, "g_fake": 7.965e-09, "g_gx": 5.947e-08},
    "loss/3x1x256/saturated@0/real/-": {"parts": 4.355e-08, "g_real": 1.724e-08},
    "loss/3x1x256/saturated@0/fake/-": {"parts": 4.355e-08, "g_fake": 7.308e-09},
    "loss/3x1x256/saturated@0/real+fake/-": {"parts": 4.355e-08, "g_real": 1.724e-08, "g_fake": 7.308e-09},
    "loss/3x1x256/saturated@0/real+fake+gx/1e-6": {"parts": 4.379e-08, "g_real": 1.724e-08, "g_fake": 7.308e-09, "g_gx": 1.213e-12},
    "loss/3x1x256/saturated@0/real+fake+gx/1": {"parts": 6.653e-08, "g_real": 1.724e-08, "g_fake": 7.308e-09, "g_gx": 5.760e-08},
    "loss/3x1x256/saturated@0/real+fake+gx/1e3": {"parts": 8.604e-08, "g_real": 1.724e-08, "g_fake": 7.308e-09, "g_gx": 5.374e-08},
    "loss/3x1x256/saturated@1/real+fake+gx/1": {"parts": 4.598e-08, "g_real": 9.934e-09, "g_fake": 2.373e-08, "g_gx": 4.934e-08},
    "loss/3x1x256/saturated@2/real+fake+gx/1": {"parts": 3.753e-08, "g_real": 9.934e-09, "g_fake": 9.934e-09, "g_gx": 5.052e-08},
    "loss/3x1x256/saturated@3/real+fake+gx/1": {"parts": 2.032e-08, "g_real": 9.934e-09, "g_fake": 9.934e-09, "g_gx": 5.035e-08},
    "loss/3x1x256/tiny/real/-": {"parts": 3.103e-08, "g_real": 1.154e-08},
    "loss/3x1x256/tiny/fake/-": {"parts": 4.766e-08, "g_fake": 1.576e-08},
    "loss/3x1x256/tiny/real+fake/-": {"parts": 3.247e-08, "g_real": 1.951e-08, "g_fake": 6.783e-09},
    "loss/3x1x256/tiny/real+fake+gx/1e-6": {"parts": 9.783e-08, "g_real": 7.245e-09, "g_fake": 7.186e-09, "g_gx": 1.213e-12},
    "loss/3x1x256/tiny/real+fake+gx/1": {"parts": 4.292e-08, "g_real": 1.162e-08, "g_fake": 6.209e-09, "g_gx": 5.861e-08},
    "loss/3x1x256/tiny/real+fake+gx/1e3": {"parts": 2.000e-08, "g_real": 9.348e-09, "g_fake": 4.811e-09, "g_gx": 5.764e-08},
    "loss/5x7x1031/balanced/real/-": {"parts": 6.619e-08, "g_real": 8.590e-09},
    "loss/5x7x1031/balanced/fake/-": {"parts": 1.054e-07, "g_fake": 9.004e-09},
    "loss/5x7x1031/balanced/real+fake/-": {"parts": 2.128e-08, "g_real": 1.007e-08, "g_fake": 8.235e-09},
    "loss/5x7x1031/balanced/real+fake+pose/-": {"parts": 8.164e-08, "g_real": 1.077e-08, "g_fake": 1.306e-08},
    "loss/5x7x1031/balanced/real+fake+gx/1e-6": {"parts": 6.837e-08, "g_real": 9.744e-09, "g_fake": 2.418e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/balanced/real+fake+gx/1": {"parts": 7.461e-08, "g_real": 1.313e-08, "g_fake": 5.951e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/balanced/real+fake+gx/1e3": {"parts": 1.172e-08, "g_real": 7.179e-09, "g_fake": 1.844e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/balanced/real+fake+pose+gx/1e-6": {"parts": 8.794e-08, "g_real": 9.219e-09, "g_fake": 1.550e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/balanced/real+fake+pose+gx/1": {"parts": 1.195e-07, "g_real": 9.032e-09, "g_fake": 1.174e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/balanced/real+fake+pose+gx/1e3": {"parts": 2.332e-08, "g_real": 8.169e-09, "g_fake": 1.359e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@0/real/-": {"parts": 6.805e-09, "g_real": 1.035e-08},
    "loss/5x7x1031/saturated@0/fake/-": {"parts": 6.805e-09, "g_fake": 1.126e-08},
    "loss/5x7x1031/saturated@0/real+fake/-": {"parts": 6.805e-09, "g_real": 1.035e-08, "g_fake": 1.126e-08},
    "loss/5x7x1031/saturated@0/real+fake+pose/-": {"parts": 2.708e-08, "g_real": 1.035e-08, "g_fake": 1.915e-08},
    "loss/5x7x1031/saturated@0/real+fake+gx/1e-6": {"parts": 7.595e-09, "g_real": 1.035e-08, "g_fake": 1.126e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@0/real+fake+gx/1": {"parts": 1.166e-07, "g_real": 1.035e-08, "g_fake": 1.126e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@0/real+fake+gx/1e3": {"parts": 1.307e-08, "g_real": 1.035e-08, "g_fake": 1.126e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@0/real+fake+pose+gx/1e-6": {"parts": 7.693e-09, "g_real": 1.035e-08, "g_fake": 1.126e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@0/real+fake+pose+gx/1": {"parts": 1.621e-07, "g_real": 1.035e-08, "g_fake": 1.126e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@0/real+fake+pose+gx/1e3": {"parts": 7.617e-08, "g_real": 1.035e-08, "g_fake": 1.589e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@1/real+fake+pose+gx/1": {"parts": 1.403e-07, "g_real": 2.980e-09, "g_fake": 9.954e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/saturated@2/real+fake+pose+gx/1": {"parts": 4.750e-08, "g_real": 1.035e-08, "g_fake": 1.268e-08, "g_gx": 0.000e+00},
    "loss/5x7x1031/tiny/real/-": {"parts": 2.893e-08, "g_real": 8.317e-09},
    "loss/5x7x1031/tiny/fake/-": {"parts": 8.573e-09, "g_fake": 9.784e-09},
    "loss/5x7x1031/tiny/real+fake/-": {"parts": 9.194e-08, "g_real": 5.565e-09, "g_fake": 6.789e-09},
    "loss/5x7x1031/tiny/real+fake+pose/-": {"parts": 3.862e-08, "g_real": 8.750e-09, "g_fake": 1.139e-08},
    "loss/5x7x1031/tiny/real+fake+gx/1e-6": {"parts": 6.151e-08, "g_real": 6.778e-09, "g_fake": 5.155e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/tiny/real+fake+gx/1": {"parts": 2.207e-08, "g_real": 8.545e-09, "g_fake": 6.717e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/tiny/real+fake+gx/1e3": {"parts": 1.387e-08, "g_real": 9.489e-09, "g_fake": 8.528e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/tiny/real+fake+pose+gx/1e-6": {"parts": 2.006e-08, "g_real": 5.148e-09, "g_fake": 6.896e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/tiny/real+fake+pose+gx/1": {"parts": 5.601e-09, "g_real": 8.888e-09, "g_fake": 8.825e-09, "g_gx": 0.000e+00},
    "loss/5x7x1031/tiny/real+fake+pose+gx/1e3": {"parts": 1.178e-08, "g_real": 5.855e-09, "g_fake": 9.371e-09, "g_gx": 0.000e+00},
    "loss/64x7x48/balanced/real/-": {"parts": 1.097e-07, "g_real": 1.083e-09},
    "loss/64x7x48/balanced/fake/-": {"parts": 3.162e-08, "g_fake": 9.364e-10},
    "loss/64x7x48/balanced/real+fake/-": {"parts": 5.574e-08, "g_real": 1.112e-09, "g_fake": 9.879e-10},
    "loss/64x7x48/balanced/real+fake+pose/-": {"parts": 2.709e-08, "g_real": 8.764e-10, "g_fake": 1.217e-09},
    "loss/64x7x48/balanced/real+fake+gx/1e-6": {"parts": 4.062e-08, "g_real": 1.083e-09, "g_fake": 1.179e-09, "g_gx": 5.684e-14},
    "loss/64x7x48/balanced/real+fake+gx/1": {"parts": 1.230e-07, "g_real": 8.171e-10, "g_fake": 1.181e-09, "g_gx": 2.262e-08},
    "loss/64x7x48/balanced/real+fake+gx/1e3": {"parts": 1.264e-08, "g_real": 1.051e-09, "g_fake": 1.129e-09, "g_gx": 4.035e-08},
    "loss/64x7x48/balanced/real+fake+pose+gx/1e-6": {"parts": 5.204e-08, "g_real": 8.776e-10, "g_fake": 1.142e-09, "g_gx": 4.263e-14},
    "loss/64x7x48/balanced/real+fake+pose+gx/1": {"parts": 2.805e-08, "g_real": 8.656e-10, "g_fake": 1.002e-09, "g_gx": 4.711e-08},
    "loss/64x7x48/balanced/real+fake+pose+gx/1e3": {"parts": 5.067e-08, "g_real": 9.647e-10, "g_fake": 1.017e-09, "g_gx": 2.544e-08},
    "loss/64x7x48/saturated@0/real/-": {"parts": 4.588e-09, "g_real": 8.082e-10},
    "loss/64x7x48/saturated@0/fake/-": {"parts": 2.884e-08, "g_fake": 9.760e-10},
    "loss/64x7x48/saturated@0/real+fake/-": {"parts": 5.614e-08, "g_real": 8.082e-10, "g_fake": 1.044e-09},
    "loss/64x7x48/saturated@0/real+fake+pose/-": {"parts": 3.798e-08, "g_real": 1.079e-09, "g_fake": 1.140e-09},
    "loss/64x7x48/saturated@0/real+fake+gx/1e-6": {"parts": 5.577e-08, "g_real": 9.860e-10, "g_fake": 1.048e-09, "g_gx": 4.263e-14},
    "loss/64x7x48/saturated@0/real+fake+gx/1": {"parts": 7.633e-09, "g_real": 8.876e-10, "g_fake": 1.039e-09, "g_gx": 2.535e-08},
    "loss/64x7x48/saturated@0/real+fake+gx/1e3": {"parts": 3.825e-08, "g_real": 8.082e-10, "g_fake": 1.071e-09, "g_gx": 2.747e-08},
    "loss/64x7x48/saturated@0/real+fake+pose+gx/1e-6": {"parts": 2.139e-08, "g_real": 8.082e-10, "g_fake": 1.105e-09, "g_gx": 5.684e-14},
    "loss/64x7x48/saturated@0/real+fake+pose+gx/1": {"parts": 8.461e-08, "g_real": 1.098e-09, "g_fake": 1.023e-09, "g_gx": 2.504e-08},
    "loss/64x7x48/saturated@0/real+fake+pose+gx/1e3": {"parts": 1.041e-07, "g_real": 1.136e-09, "g_fake": 9.727e-10, "g_gx": 4.932e-08},
    "loss/64x7x48/tiny/real/-": {"parts": 4.272e-08, "g_real": 5.910e-10},
    "loss/64x7x48/tiny/fake/-": {"parts": 2.747e-08, "g_fake": 6.959e-10},
    "loss/64x7x48/tiny/real+fake/-": {"parts": 3.792e-08, "g_real": 6.739e-10, "g_fake": 6.621e-10},
    "loss/64x7x48/tiny/real+fake+pose/-": {"parts": 6.643e-08, "g_real": 6.577e-10, "g_fake": 6.598e-10},
    "loss/64x7x48/tiny/real+fake+gx/1e-6": {"parts": 2.384e-08, "g_real": 6.927e-10, "g_fake": 6.402e-10, "g_gx": 5.684e-14},
    "loss/64x7x48/tiny/real+fake+gx/1": {"parts": 6.219e-09, "g_real": 6.945e-10, "g_fake": 6.736e-10, "g_gx": 5.033e-08},
    "loss/64x7x48/tiny/real+fake+gx/1e3": {"parts": 1.736e-08, "g_real": 6.774e-10, "g_fake": 6.919e-10, "g_gx": 4.812e-08},
    "loss/64x7x48/tiny/real+fake+pose+gx/1e-6": {"parts": 8.477e-08, "g_real": 6.842e-10, "g_fake": 6.461e-10, "g_gx": 5.684e-14},
    "loss/64x7x48/tiny/real+fake+pose+gx/1": {"parts": 7.819e-08, "g_real": 6.668e-10, "g_fake": 9.494e-10, "g_gx": 5.762e-08},
    "loss/64x7x48/tiny/real+fake+pose+gx/1e3": {"parts": 9.968e-08, "g_real": 6.884e-10, "g_fake": 6.505e-10, "g_gx": 2.840e-08},
    "loss/8x1x49152/balanced/real/-": {"parts": 2.547e-08, "g_real": 6.005e-09},
    "loss/8x1x49152/balanced/fake/-": {"parts": 1.759e-08, "g_fake": 3.198e-09},
    "loss/8x1x49152/balanced/real+fake/-": {"parts": 2.376e-08, "g_real": 6.511e-09, "g_fake": 6.255e-09},
    "loss/8x1x49152/balanced/real+fake+gx/1e-6": {"parts": 6.605e-08, "g_real": 7.149e-09, "g_fake": 6.091e-09, "g_gx": 4.547e-13},
    "loss/8x1x49152/balanced/real+fake+gx/1": {"parts": 1.062e-07, "g_real": 5.094e-09, "g_fake": 3.657e-09, "g_gx": 3.865e-08},
    "loss/8x1x49152/balanced/real+fake+gx/1e3": {"parts": 9.407e-08, "g_real": 7.366e-09, "g_fake": 5.543e-09, "g_gx": 4.141e-08},
    "loss/8x1x49152/saturated@0/real/-": {"parts": 4.631e-09, "g_real": 6.466e-09},
    "loss/8x1x49152/saturated@0/fake/-": {"parts": 4.631e-09, "g_fake": 6.466e-09},
    "loss/8x1x49152/saturated@0/real+fake/-": {"parts": 4.631e-09, "g_real": 6.466e-09, "g_fake": 6.466e-09},
    "loss/8x1x49152/saturated@0/real+fake+gx/1e-6": {"parts": 1.770e-08, "g_real": 6.466e-09, "g_fake": 6.466e-09, "g_gx": 4.547e-13},
    "loss/8x1x49152/saturated@0/real+fake+gx/1": {"parts": 7.720e-08, "g_real": 6.466e-09, "g_fake": 6.466e-09, "g_gx": 4.113e-08},
    "loss/8x1x49152/saturated@0/real+fake+gx/1e3": {"parts": 9.888e-08, "g_real": 6.466e-09, "g_fake": 6.466e-09, "g_gx": 4.082e-08},
    "loss/8x1x49152/saturated@1/real+fake+gx/1": {"parts": 9.575e-08, "g_real": 6.466e-09, "g_fake": 6.466e-09, "g_gx": 4.215e-08},
    "loss/8x1x49152/tiny/real/-": {"parts": 1.648e-08, "g_real": 4.059e-09},
    "loss/8x1x49152/tiny/fake/-": {"parts": 1.635e-08, "g_fake": 4.404e-09},
    "loss/8x1x49152/tiny/real+fake/-": {"parts": 7.841e-08, "g_real": 4.778e-09, "g_fake": 5.391e-09},
    "loss/8x1x49152/tiny/real+fake+gx/1e-6": {"parts": 4.666e-08, "g_real": 4.444e-09, "g_fake": 4.476e-09, "g_gx": 4.547e-13},
    "loss/8x1x49152/tiny/real+fake+gx/1": {"parts": 3.554e-08, "g_real": 5.017e-09, "g_fake": 3.919e-09, "g_gx": 3.740e-08},
    "loss/8x1x49152/tiny/real+fake+gx/1e3": {"parts": 1.987e-08, "g_real": 5.254e-09, "g_fake": 5.140e-09, "g_gx": 4.434e-08},
    "cat/1x7x12288/balanced/real+fake+pose+gx/1": {"parts": 1.544e-08, "g_real": 1.611e-08, "g_fake": 1.152e-08, "g_gx": 4.841e-08},
    "cat/1x7x12288/saturated@0/real+fake+pose+gx/1": {"parts": 5.667e-08, "g_real": 5.173e-08, "g_fake": 2.583e-08, "g_gx": 4.277e-08},
    "cat/1x7x12288/tiny/real+fake+pose+gx/1": {"parts": 3.826e-08, "g_real": 4.208e-08, "g_fake": 1.031e-08, "g_gx": 4.540e-08},
    "cat/3x1x256/balanced/real+fake+gx/1": {"parts": 8.963e-10, "g_real": 6.780e-09, "g_fake": 2.885e-09, "g_gx": 5.156e-08},
    "cat/3x1x256/saturated@0/real+fake+gx/1": {"parts": 2.047e-08, "g_real": 1.724e-08, "g_fake": 7.308e-09, "g_gx": 4.283e-08},
    "cat/3x1x256/tiny/real+fake+gx/1": {"parts": 8.424e-08, "g_real": 1.056e-08, "g_fake": 1.648e-08, "g_gx": 6.139e-08},
    "glue/-2.0/-30.0/-0.2": {"inv_s": 2.525e-09, "s_val": 0.000e+00, "ambient": 6.636e-08, "diffuse": 9.359e-14, "specular": 0.000e+00},
    "glue/-1.3816/0.0/0.0": {"inv_s": 2.525e-09, "s_val": 0.000e+00, "ambient": 0.000e+00, "diffuse": 0.000e+00, "specular": 0.000e+00},
    "glue/-1.3815/30.0/0.7": {"inv_s": 5.205e-07, "s_val": 4.957e-07, "ambient": 9.348e-14, "diffuse": 9.348e-14, "specular": 0.000e+00},
    "glue/0.0/-30.0/-0.2": {"inv_s": 0.000e+00, "s_val": 0.000e+00, "ambient": 6.636e-08, "diffuse": 9.359e-14, "specular": 0.000e+00},
    "glue/0.3/0.0/0.0": {"inv_s": 1.175e-07, "s_val": 8.926e-08, "ambient": 0.000e+00, "diffuse": 0.000e+00, "specular": 0.000e+00},
    "glue/1.3815/30.0/0.7": {"inv_s": 4.957e-07, "s_val": 5.205e-07, "ambient": 9.348e-14, "diffuse": 9.348e-14, "specular": 0.000e+00},
    "glue/1.3816/-30.0/-0.2": {"inv_s": 0.000e+00, "s_val": 2.525e-09, "ambient": 6.636e-08, "diffuse": 9.359e-14, "specular": 0.000e+00},
    "glue/2.0/0.0/0.0": {"inv_s": 0.000e+00, "s_val": 2.525e-09, "ambient": 0.000e+00, "diffuse": 0.000e+00, "specular": 0.000e+00},
    "rs/0.0/0.0": {"gradient_error": 0.000e+00, "surface_loss": 0.000e+00, "g_r4_0": 1.455e-16, "g_r4_1": 0.000e+00, "g_r4_2": 0.000e+00, "g_r4_3": 0.000e+00},
    "rs/12.5/0.0": {"gradient_error": 0.000e+00, "surface_loss": 0.000e+00, "g_r4_0": 1.455e-16, "g_r4_1": 6.144e-08, "g_r4_2": 0.000e+00, "g_r4_3": 0.000e+00},
    "rs/0.0/1.0": {"gradient_error": 0.000e+00, "surface_loss": 0.000e+00, "g_r4_0": 1.368e-08, "g_r4_1": 0.000e+00, "g_r4_2": 0.000e+00, "g_r4_3": 0.000e+00},
    "rs/12.5/1.0": {"gradient_error": 5.393e-09, "surface_loss": 0.000e+00, "g_r4_0": 1.368e-08, "g_r4_1": 1.069e-08, "g_r4_2": 0.000e+00, "g_r4_3": 0.000e+00},
    "rs/0.0/340.0": {"gradient_error": 0.000e+00, "surface_loss": 0.000e+00, "g_r4_0": 4.897e-08, "g_r4_1": 0.000e+00, "g_r4_2": 0.000e+00, "g_r4_3": 0.000e+00},
    "rs/12.5/340.0": {"gradient_error": 7.114e-08, "surface_loss": 0.000e+00, "g_r4_0": 4.897e-08, "g_r4_1": 9.026e-08, "g_r4_2": 0.000e+00, "g_r4_3": 0.000e+00},
    "wsum/n=1": {"total": 0.000e+00, "g_terms": 0.000e+00},
    "wsum/n=1,w=0": {"total": 0.000e+00, "g_terms": 0.000e+00},
    "wsum/n=8": {"total": 7.212e-09, "g_terms": 2.484e-10},
    "adam/config/ordinary": {"p": 5.309e-07, "exp_avg": 0.000e+00, "exp_avg_sq": 3.397e-07},
    "adam/config/mixed": {"p": 1.552e-07, "exp_avg": 0.000e+00, "exp_avg_sq": 2.050e-07},
    "adam/config/vanishing": {"p": 1.773e-07, "exp_avg": 0.000e+00, "exp_avg_sq": 4.787e-24},
    "adam/config/spike": {"p": 2.923e-07, "exp_avg": 0.000e+00, "exp_avg_sq": 3.614e-08},
    "adam/config/zeros": {"p": 1.889e-07, "exp_avg": 0.000e+00, "exp_avg_sq": 1.732e-07},
    "adam/config/long": {"p": 8.818e-07, "exp_avg": 0.000e+00, "exp_avg_sq": 3.016e-07},
    "adam/config/late": {"p": 8.470e-08, "exp_avg": 0.000e+00, "exp_avg_sq": 1.464e-07},
    "adam/config/skips": {"p": 1.706e-07, "exp_avg": 0.000e+00, "exp_avg_sq": 1.867e-07},
    "adam/default/ordinary": {"p": 4.260e-07, "exp_avg": 1.033e-07, "exp_avg_sq": 7.239e-07},
    "adam/default/mixed": {"p": 1.787e-07, "exp_avg": 8.638e-08, "exp_avg_sq": 1.744e-07},
    "adam/default/vanishing": {"p": 2.080e-07, "exp_avg": 1.948e-16, "exp_avg_sq": 9.443e-26},
    "adam/default/spike": {"p": 4.303e-07, "exp_avg": 3.070e-07, "exp_avg_sq": 1.004e-07},
    "adam/default/zeros": {"p": 2.454e-07, "exp_avg": 7.268e-08, "exp_avg_sq": 8.690e-09},
    "adam/default/long": {"p": 9.888e-07, "exp_avg": 1.501e-07, "exp_avg_sq": 2.074e-06},
    "adam/default/late": {"p": 8.323e-08, "exp_avg": 9.383e-08, "exp_avg_sq": 1.785e-07},
    "adam/default/skips": {"p": 1.641e-07, "exp_avg": 8.746e-08, "exp_avg_sq": 6.371e-09},
    "rmsprop/config/ordinary": {"p": 4.361e-07, "square_avg": 5.330e-07},
    "rmsprop/config/mixed": {"p": 1.922e-07, "square_avg": 1.620e-07},
    "rmsprop/config/vanishing": {"p": 1.772e-07, "square_avg": 6.126e-25},
    "rmsprop/config/spike": {"p": 2.654e-07, "square_avg": 7.117e-08},
    "rmsprop/config/zeros": {"p": 1.832e-07, "square_avg": 5.188e-08},
    "rmsprop/config/long": {"p": 8.771e-07, "square_avg": 1.431e-06},
    "rmsprop/config/late": {"p": 8.121e-08, "square_avg": 1.558e-07},
    "rmsprop/config/skips": {"p": 1.901e-07, "square_avg": 4.347e-08},
    "rmsprop/default/ordinary": {"p": 3.415e-07, "square_avg": 5.913e-07},
    "rmsprop/default/mixed": {"p": 1.978e-07, "square_avg": 1.471e-07},
    "rmsprop/default/vanishing": {"p": 2.146e-07, "square_avg": 5.627e-25},
    "rmsprop/default/spike": {"p": 3.257e-07, "square_avg": 7.117e-08},
    "rmsprop/default/zeros": {"p": 1.847e-07, "square_avg": 5.359e-08},
    "rmsprop/default/long": {"p": 1.323e-06, "square_avg": 1.167e-06},
    "rmsprop/default/late": {"p": 9.084e-08, "square_avg": 1.588e-07},
    "rmsprop/default/skips": {"p": 1.845e-07, "square_avg": 4.657e-08},
    "ema/0.0": {"p_ema": 0.000e+00},
    "ema/0.5": {"p_ema": 8.268e-08},
    "ema/0.999": {"p_ema": 1.472e-07},
    "ema/1.0": {"p_ema": 0.000e+00},
}
