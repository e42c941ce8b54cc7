"""DC discriminators -- drop-ins for src.models.discriminator.DCDiscriminator / ADADiscriminator /
ADADiscriminatorView (discriminator.py:49-108): same constructor kwargs, `forward(x, **kwargs)`,
`get_resolution()`, `.aug`, and state_dict keys `blocks.{i}.weight`, `conv_out.weight[/bias]`,
`aug.p`, `aug.Hz_geom`, `aug.Hz_fbank`.  Convolutions are the implicit-GEMM MFMA kernels of
csrc/disc.hip with the LeakyReLU fused.  `route()` names the way a forward call takes."""
import os
import weakref
from math import log2

import torch
import torch.nn as nn

from . import autograd_conv as AC
from . import ops
from .autograd_disc import conv4x4_lrelu
from .config import build_from_config

_SMALL_PLANS = weakref.WeakKeyDictionary()   # (not in __dict__: plans hold library handles; copy.deepcopy(module) must work)
_LARGE_PACKS = weakref.WeakKeyDictionary()
_FAST_ADA = weakref.WeakKeyDictionary()   # module -> _FastSmallAda: skips a call's marshalling, never its route decision
LARGE_PATH = True   # batch >= 16 no-grad forwards take csrc/disc_large.hip when the network is covered (False: the general chain)
LARGE_MIN_BATCH = 16
FAST_ADA = True     # ADADiscriminator.forward, shipped augmentation, batch <= 4: parameters drawn inside the library (False: numpy)
SMALL_PATH = True   # batch <= 4 no-grad forwards of the 64 x 64 network take csrc/disc_small.hip (False: the general chain)
SMALL_PATH_128 = os.environ.get("OI_SMALL128", "1") != "0"   # ... and of the shipped 128 x 128 / five-block network (round 6)
# what csrc/disc_small.hip covers: BASELINE's 64 x 64 network or the shipped 128 x 128 one (configs/train.yaml:78-102)
_SMALL_WIDTHS = {(64, 64): (64, 128, 256, 512), (128, 128): (32, 64, 128, 256, 512)}


def route(shape, grad, cuda, capturing, widths, in_dim, out_dim, w_in, weights_ok, stock=None, theta=False, fast_draw=False):
    """The way a forward call takes -> (augmentation route, network route), from plain facts and the module switches as they stand
    at the call: no tensor, no library (DESIGN 4.8 has the table, tests/test_disc_route_cpu.py holds it).  `w_in`: the first block's
    input channels; `weights_ok`: all fp32 and contiguous; `stock`: AugmentPipe.is_stock(), None without a pipe (DCDiscriminator);
    `theta`: aug_theta was given; `fast_draw`: AugmentPipe.fast_draw_ok().
    Network: "small" (csrc/disc_small.hip, a library plan) | "large" (csrc/disc_large.hip; "arena" when the pack does not cover the
    network) | "arena" (the no-grad chain of csrc/disc.hip) | with gradient "pre" (pre-activation chain) | "lrelu".
    Augmentation, inside the small network's first launch: "theta" (the plain entry, the caller's device matrices: what captured
    graphs pass) | "lib" (draws inside the library) | "host" (numpy draws, matrices by value); ahead of the parent's forward: "sep"
    (the separable launch from host matrices; "pipe" when ops.ada_geom_sep_ok does not cover the batch) | "pipe" (AugmentPipe).
    Under somebody's capture no plan (its counters' zero fill would be recorded, not run: advisor, round 4) and no pack (an eager
    allocation keyed on parameter versions: round 5) is taken; "theta" refuses a FIRST call inside one (ops.disc_fwd_small)."""
    B, C = shape[0], shape[1]
    small = (SMALL_PATH and not grad and cuda and len(shape) == 4 and B <= 4 and C <= 4 and out_dim <= 8
             and _SMALL_WIDTHS.get(tuple(shape[2:])) == tuple(widths) and (len(widths) == 4 or SMALL_PATH_128)
             and C == in_dim == w_in and weights_ok)
    if grad:
        net = "pre" if AC.PRE_CHAIN and cuda else "lrelu"
    elif small and not capturing:
        net = "small"
    elif LARGE_PATH and B >= LARGE_MIN_BATCH and cuda and not capturing:
        net = "large"
    else:
        net = "arena"
    if stock is None:
        return None, net
    if small and stock:
        if theta:
            return "theta", "small"
        if capturing:
            return "pipe", net
        return ("lib" if FAST_ADA and fast_draw else "host"), "small"
    if not theta and FAST_ADA and not grad and cuda and B >= LARGE_MIN_BATCH and stock and fast_draw:
        return "sep", net
    return "pipe", net


def _weight_ptrs(disc, f12=None):
    """Addresses of `disc`'s live weights (+ head bias, + filter `f12`): what a plan was built on must be what the modules hold."""
    ws, wh, bh = disc.live_weights()
    return [t.data_ptr() for t in (*ws, wh, bh, f12) if t is not None]


class _ConvParam(nn.Module):
    """Holds `weight` (and optional `bias`) under the same names as nn.Conv2d(…, 4, s, p)."""

    def __init__(self, cin, cout, bias=False):
        super().__init__()
        conv = nn.Conv2d(cin, cout, 4, bias=bias)  # identical default initialisation to the reference's layers
        self.weight = nn.Parameter(conv.weight.detach().clone())
        if bias:
            self.bias = nn.Parameter(conv.bias.detach().clone())
        else:
            self.register_parameter("bias", None)


class DCDiscriminator(nn.Module):
    def __init__(self, in_dim=3, out_dim=1, n_feat=512, img_size=64, last_bias=False):
        super().__init__()
        self.in_dim, self.out_dim = in_dim, out_dim
        n_layers = int(log2(img_size) - 2)
        chans = [in_dim] + [int(n_feat / (2 ** (n_layers - 1 - i))) for i in range(n_layers)]
        self.blocks = nn.ModuleList([_ConvParam(chans[i], chans[i + 1]) for i in range(n_layers)])
        self.conv_out = _ConvParam(n_feat, out_dim, bias=last_bias)

    def live_weights(self):
        """(block weights, head weight, head bias or None) as the modules hold them NOW: a replaced Parameter or layer is seen.
        Through the modules' own dicts: 0.6 us, not the 5.5 of nn.Module.__getattr__ (route()'s facts are gathered on every call)."""
        head = self._modules["conv_out"]._parameters
        return [m._parameters["weight"] for m in self._modules["blocks"]._modules.values()], head["weight"], head["bias"]

    def _facts(self, x):
        """route()'s facts about this image and network."""
        ws, wh, bh = self.live_weights()
        return dict(shape=tuple(x.shape), grad=torch.is_grad_enabled(), cuda=x.is_cuda,
                    capturing=x.is_cuda and torch.cuda.is_current_stream_capturing(), widths=tuple([w.shape[0] for w in ws]),
                    in_dim=self.in_dim, out_dim=self.out_dim, w_in=ws[0].shape[1],
                    weights_ok=all(w.dtype == torch.float32 and w.is_contiguous() for w in (*ws, wh, bh) if w is not None))

    def _small_ok(self, x):
        """csrc/disc_small.hip covers this call: route()'s "small", bar its capture condition."""
        return route(**dict(self._facts(x), capturing=False))[1] == "small"

    def _forward_arena(self, x):
        """Forward-only chain: all layer outputs live in ONE zero-filled arena (a single fill launch instead of one per
        split-K layer) and every block hands over its pre-activation sums -- the LeakyReLU is applied by the next
        layer while it loads them, so the split-K layers need no activation pass: 6 launches instead of 13."""
        ws, wh, bh = self.live_weights()
        layers = [(w, None, 2, 1, 0.2) for w in ws] + [(wh, bh, 1, 0, 1.0)]
        shapes, shp = [], tuple(x.shape)
        for w, _, stride, pad, _ in layers:
            shp = ops.conv4x4_out_shape(shp, w.shape[0], stride, pad)
            shapes.append(shp)
        sizes = [(s[0] * s[1] * s[2] * s[3] + 3) // 4 * 4 for s in shapes]
        # no fill launch: the first layer (K = 16 in_dim taps: never split) clears the rest of the arena while it runs
        arena = torch.empty(sum(sizes), dtype=torch.float32, device=x.device)
        off, x_slope = 0, 1.0
        for i, ((w, b, stride, pad, slope), s, n) in enumerate(zip(layers, shapes, sizes)):
            x = ops.conv4x4_fwd(x, w, b, stride, pad, slope if i == len(layers) - 1 else 1.0, x_slope=x_slope,
                                out=arena[off:off + s[0] * s[1] * s[2] * s[3]].view(s),
                                zero_tail=sum(sizes) - sizes[0] if i == 0 else 0, out_is_zero=i > 0)
            x_slope = slope  # this block's activation, deferred to the next layer's loads
            off += n
        return x

    def _forward_large(self, x):
        """Batch >= 16: activations as NHWC fp16 limb planes, weights packed once per parameter version (ops.DiscLargePack), K split
        with a fixed-order reduction -- csrc/disc_large.hip.  None when the network / shape is not covered."""
        ws, wh, bh = self.live_weights()
        key = tuple((w.data_ptr(), w._version) for w in (*ws, wh))
        ent = _LARGE_PACKS.get(self)
        if ent is None or ent[0] != key:
            ent = _LARGE_PACKS[self] = (key, ops.DiscLargePack(ws, wh))
        return ops.disc_fwd_large(x, ent[1], ws[0], bh)

    def _forward_small(self, x, f12=None, theta_np=None, theta_dev=None, margins=None):
        """theta_dev (captured graphs): the plain entry.  Otherwise a plan held by the library (ops.DiscGraph, launch by launch):
        everything but the image pointer and the matrices is marshalled once per (shape, stream, weight addresses), not per
        call -- 50 us of host time per forward less."""
        if theta_dev is not None:
            return ops.disc_fwd_small(x.float(), *self.live_weights(), f12=f12, theta_dev=theta_dev, margins=margins)
        aug_on = theta_np is not None
        return self._small_plan(x, f12 if aug_on else None, margins if aug_on else None)(x.float(), theta_np, fresh=True)

    def _small_plan(self, x, f12, margins):
        """The library plan (ops.DiscGraph, launched launch by launch) for this image shape / stream / weight addresses; with the
        augmentation at static `margins` when they are given."""
        key = (tuple(x.shape), x.device.index, ops._stream().value or 0, None if margins is None else tuple(int(v) for v in margins),
               tuple(_weight_ptrs(self, f12)))
        plans = _SMALL_PLANS.setdefault(self, {})
        plan = plans.get(key)
        if plan is None:
            if len(plans) >= 8:
                plans.clear()   # (weights moved, many shapes: start over rather than grow)
                _FAST_ADA.pop(self, None)
            plan = plans[key] = ops.DiscGraph(tuple(x.shape), x.device, *self.live_weights(), f12=f12, margins=margins, launch="eager")
        return plan

    def forward(self, x, **kwargs):
        batch_size = x.shape[0]
        assert x.shape[1] == self.in_dim, x.shape
        net = route(**self._facts(x))[1]
        if net == "small":
            return self._forward_small(x)
        if net in ("large", "arena"):
            out = self._forward_large(x.float()) if net == "large" else None   # (None: the pack does not cover the network)
            return (self._forward_arena(x.float()) if out is None else out).reshape(batch_size, self.out_dim)
        ws, wh, bh = self.live_weights()
        if net == "pre":
            # (autograd_conv._ConvPre): every block hands over its sums, the next layer applies the LeakyReLU while it loads
            # them -- no activation pass forward, no mask pass backward
            slope_in = 1.0
            for w in ws:
                x = AC.conv4x4_pre(x, w, slope_in, 2, 1)
                slope_in = 0.2
            out = AC.conv4x4_pre(x, wh, slope_in, 1, 0)
            if bh is not None:
                out = AC._AddBias.apply(out, bh)
            return out.reshape(batch_size, self.out_dim)
        for w in ws:
            x = conv4x4_lrelu(x, w, None, stride=2, pad=1, slope=0.2)
        return conv4x4_lrelu(x, wh, bh, stride=1, pad=0, slope=1.0).reshape(batch_size, self.out_dim)


class _FastSmallAda:
    """The memo of ADADiscriminator.forward's "lib" route: the plan (ops.DiscGraph.call_ada answers with ONE library call: draws,
    sampling matrices, the four launches) and route()'s facts that follow from the image's shape / device and the weight TENSORS.
    It saves a call's marshalling (the plan's key, the margins, the fp32 copy), not its decision: every call checks the image's
    shape / dtype / layout, the stream and the LIVE addresses of the weights and the filter (live_weights(): no Parameter
    is kept, a replaced one is seen; in-place optimiser updates keep the addresses the plan holds), then asks route() again with
    the switches, capture state and pipe as they stand.  Not "lib" -> dropped, None -> the forward decides afresh.  Review, round 5:
    numpy draws (20 us), matrix algebra (4 us), marshalling (5 us) and ~15 us of per-call checks stood against 16 us of launches."""

    __slots__ = ("facts", "device", "stream", "ptrs", "plan")

    def __init__(self, disc, x, plan, facts):
        self.facts = {k: facts[k] for k in ("shape", "cuda", "widths", "w_in", "weights_ok")}
        self.device, self.stream, self.plan, self.ptrs = x.device, ops._stream().value, plan, _weight_ptrs(disc, disc.aug.Hz_geom)

    def __call__(self, disc, x):
        if (tuple(x.shape) != self.facts["shape"] or x.dtype is not torch.float32 or x.device != self.device or not x.is_contiguous()
                or torch.is_grad_enabled() or ops._stream().value != self.stream):
            return None   # (another kind of call: decided afresh, the memo stays for its own kind)
        aug = disc._modules["aug"]
        draw = aug.fast_draw_ok()   # (implies is_stock())
        if (_weight_ptrs(disc, aug._buffers["Hz_geom"]) != self.ptrs
                or route(grad=False, capturing=torch.cuda.is_current_stream_capturing(), in_dim=disc.in_dim, out_dim=disc.out_dim,
                         stock=draw or aug.is_stock(), fast_draw=draw, **self.facts)[0] != "lib"):
            del _FAST_ADA[disc]   # stale: other weights, switches or pipe
            return None
        return self.plan.call_ada(x, aug.draw_seed(), *aug.fast_params(), fresh=True)


class ADADiscriminator(DCDiscriminator):
    def __init__(self, aug, aug_p, **kwargs):
        super().__init__(**kwargs)
        self.aug = build_from_config(aug)
        self.aug.p.copy_(torch.tensor(aug_p, dtype=torch.float32))
        self.resolution = kwargs["img_size"]

    def get_resolution(self):
        return self.resolution

    def forward(self, x, aug_theta=None, **kwargs):
        """`aug_theta`: precomputed sampling grid for the shape-static augmentation (see AugmentPipe.forward)."""
        aug = self.aug
        fast = _FAST_ADA.get(self)
        if fast is not None and aug_theta is None:
            out = fast(self, x)
            if out is not None:
                return out
        facts = self._facts(x)
        how = route(**facts, stock=aug.is_stock(), theta=aug_theta is not None, fast_draw=aug.fast_draw_ok())[0]
        if how in ("theta", "lib", "host"):
            # augmentation + network in four launches, at the largest margins the transform's own clamp allows (static: one plan
            # serves every draw; the same pixels are sampled as with margins fitted to the draw, augment.py:272-282)
            H, W = x.shape[2:]
            margins = aug.static_margins(H, W)
            if how == "theta":
                return self._forward_small(x, f12=aug.Hz_geom, theta_dev=aug_theta, margins=margins)
            if how == "lib":   # the shipped configuration: parameters drawn inside the library from one seed of numpy's stream
                x = x.float().contiguous()
                fast = _FAST_ADA[self] = _FastSmallAda(self, x, self._small_plan(x, aug.Hz_geom, margins), facts)
                return fast(self, x)
            G_inv = aug.sample_G_inv(x, None)
            if G_inv is None:
                return self._forward_small(x)
            return self._forward_small(x, f12=aug.Hz_geom, theta_np=aug.theta_for(G_inv, margins, H, W), margins=margins)
        if how == "sep":
            # large batches: one seed of numpy's stream expanded inside the library (as "lib"), the matrices in the arguments of ONE
            # augmentation launch (numpy draws + matrix algebra + 64 uploads cost the host more than the forward costs the GPU)
            xf = x.float().contiguous()
            if ops.ada_geom_sep_ok(xf):
                B, _, H, W = xf.shape
                return super().forward(ops.ada_geom_sep_host(xf, aug.theta_fast(B, H, W), aug.Hz_geom, aug.static_margins(H, W)), **kwargs)
        return super().forward(aug(x) if aug_theta is None else aug(x, theta=aug_theta), **kwargs)


class ADADiscriminatorView(ADADiscriminator):
    def __init__(self, out_dim_position, out_dim_latent, **kwargs):
        self.out_dim_position = out_dim_position
        self.out_dim_latent = out_dim_latent
        super().__init__(**kwargs)
