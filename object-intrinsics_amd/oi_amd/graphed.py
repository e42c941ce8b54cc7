"""HIP-graph capture of the eval-mode `Generator.forward` ("HIP-graph the step").

One frame of the inference driver is ~90 small launches around the two MLP kernels; at low resolution the host cannot
issue them as fast as the GPU retires them.  `GraphedForward` records the whole forward once into a hipGraph
(`torch.cuda.CUDAGraph`; our ctypes launches go to torch's current stream, which is the capturing stream, so they are
recorded like any other kernel) and replays it with one `hipGraphLaunch` per frame.  Inputs (pose, latent, background
colour) are copied into fixed device buffers before each replay; outputs are views of the graph's own memory pool and
are overwritten by the next replay (clone what must survive).

Restrictions: eval mode only (no per-ray jitter: its RNG offset would be frozen), fixed batch size / resolution /
iteration counter (`cos_anneal_ratio` is a launch argument and therefore baked in), and parameters must not be
re-packed between capture and replay (call `recapture()` after an optimiser step or `load_state_dict`).
"""
import contextlib
import os

import torch

# captured discriminator step: real and fake branch on two streams (parallel branches of the graph).  Off by default: the
# step alone replays in 0.66 instead of 0.75 ms, but a training iteration got 0.05-0.1 ms SLOWER on the same box (four
# runs) -- a graph with branches costs more to launch than the shorter chain saves between the neighbouring renders
FORK = os.environ.get("OI_GRAPH_D_FORK", "0") == "1"
# captured discriminator step: real and fake batch through the discriminator in ONE pass of 2B images (OI_GRAPH_D_CAT=0: two)
CAT = os.environ.get("OI_GRAPH_D_CAT", "1") == "1"


class GraphedForward:
    def __init__(self, generator, bs=1, it=0, return_raw=True, keys=None):
        if generator.training:
            raise ValueError("GraphedForward captures the eval-mode forward (generator.eval())")
        self.gen, self.bs, self.it, self.return_raw, self.keys = generator, bs, int(it), return_raw, keys
        dev = generator.it.device
        if dev.type != "cuda":
            raise ValueError("GraphedForward needs the generator on a GPU")
        self.b2w = torch.eye(4, device=dev).repeat(bs, 1, 1)
        self.b2w[:, 2, 3] = 0.0
        self.z = torch.zeros(bs, generator.z_dim, device=dev)
        self.bg = torch.zeros(bs, 3, device=dev)
        self.graph, self.out = None, None

    def _run(self):
        with torch.no_grad():
            blob = self.gen(bs=self.bs, it=self.it, data={"b2w": self.b2w, "z": self.z, "bg_color": self.bg},
                            return_raw=self.return_raw)["box"]
        out = blob["render_out"]
        return out if self.keys is None else {k: out[k] for k in self.keys}

    def recapture(self):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):      # warm-up off the capture: packs the weights, sets kernel attributes
            for _ in range(2):
                self._run()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._run()
        return self

    def __call__(self, b2w, z, bg_color=None):
        if self.graph is None:
            self.recapture()
        self.b2w.copy_(b2w, non_blocking=True)
        self.z.copy_(z, non_blocking=True)
        if bg_color is not None:
            self.bg.copy_(bg_color, non_blocking=True)
        self.graph.replay()
        return self.out


def _has_geometric(aug):
    """True when AugmentPipe.sample_G_inv can return a transform at all (augment.py:191-268: one branch per strength)."""
    return any(float(getattr(aug, k, 0)) > 0 for k in ("xflip", "rotate90", "xint", "scale", "rotate", "aniso", "xfrac"))


class GraphedDStep:
    """hipGraph of one discriminator training step WITHOUT the optimiser step: zero the gradients, real forward + R1
    double backward, fake forward (+ auxiliary pose regression), backward (gan_pose_trainer.py:154-200).

    Eagerly that is ~230 launches of a few microseconds each behind Python `autograd.Function`s: 3.1 ms of host time
    for 0.8 ms of GPU work at batch 1 (bench `training.d_step`).  Captured, the step is one `hipGraphLaunch`.
    What makes it capturable:
      * shapes: the ADA augmentation runs with the largest padding margins its own clamp allows
        (`AugmentPipe.static_margins`), so no intermediate size depends on the sampled transform;
      * randomness: the augmentation parameters are still drawn by numpy on the host, in the eager order (real batch
        first, then fake), and reach the graph as two (B, 2, 3) sampling grids in fixed device buffers;
      * scalars that change per iteration (the pose-loss weight) are device scalars;
      * the optimiser step stays outside (its chunk table is re-uploaded when pointers change): the gradients come
        out of the graph at fixed addresses, `opt.step()` follows eagerly (one launch), and under FlatGradDDP the
        gradient exchange is issued right after the replay (before the caller enqueues anything else, so that on the
        communication stream it overlaps whatever follows), `sync()` before the optimiser step waits for it.
    A different input shape (or pose-regression presence) recaptures.  The returned loss scalars are views of ONE
    clone taken after the replay: they stay valid when the next replay overwrites the graph's own buffers.
    Recapture after anything that replaces parameter / gradient tensors (load_state_dict keeps them)."""

    def __init__(self, disc, gan, aux_pose=None, reg_weight=10.0, prior=None):
        self.disc, self.gan, self.aux_pose, self.reg_weight, self.prior = disc, gan, aux_pose, float(reg_weight), prior
        self.graph = None

    def _net(self):
        return self.disc.module if hasattr(self.disc, "flat_grad") else self.disc

    def _alloc(self, x_real, x_fake, c2b):
        dev = x_real.device
        B = x_real.shape[0]
        # real and fake batch side by side: ONE discriminator pass over 2B images when CAT (the step is a chain of launches
        # that wait for each other, ~6 us each whatever their size: half as many for the forward and the plain backward)
        self._cat = CAT and x_real.shape == x_fake.shape
        self.x_cat = torch.empty(2 * B, *x_real.shape[1:], device=dev) if self._cat else None
        self.x_real = self.x_cat[:B] if self._cat else torch.empty_like(x_real)
        self.x_fake = self.x_cat[B:] if self._cat else torch.empty_like(x_fake)
        # augmentation matrices and the pose-loss weight live in ONE flat buffer: up to 64 floats reach it inside the
        # arguments of the input-staging launch (ops.stage_inputs), together with the copies of the images
        self._imm = torch.zeros(12 * B + 1, device=dev)
        self.th_cat = self._imm[:12 * B].view(2 * B, 2, 3)
        self.th_real, self.th_fake = self.th_cat[:B], self.th_cat[B:]
        self._gsel = None
        self.c2b = None if c2b is None else torch.empty_like(c2b)
        self.aux_w = self._imm[12 * B]
        self._one = torch.ones((), device=dev)
        self._fork = torch.cuda.Stream(device=dev)
        # no geometric augmentation configured: the eager path returns the images untouched (AugmentPipe.forward), so the
        # captured step must not run the pad / resample chain on an identity transform either
        self._geom = _has_geometric(self._net().aug)
        # ring of pinned staging buffers: the host runs several steps ahead of the stream, and a pinned buffer may only be
        # rewritten once the copy that reads it has executed
        self._pins = [torch.empty(2, B, 2, 3, pin_memory=True) for _ in range(8)]
        self._pin_ev = [None] * 8
        self._pin_i = 0

    def _step(self):
        disc = self.disc
        wrapped = hasattr(disc, "flat_grad")
        if wrapped:
            disc._in_graph = True  # the wrapper's gradient hooks are Python: they would run at capture time only
        try:
            return self._step_body(disc, wrapped)
        finally:
            if wrapped:
                disc._in_graph = False  # an eager `loss.backward(); opt.step()` on the same wrapper exchanges as usual

    def _step_body(self, disc, wrapped):
        from . import ops
        if getattr(self, "_pool", None) is None:
            self._pool = ops.ZeroPool()
        self._pool.begin(self.x_real.device)   # ONE fill for every split-K / scatter output of the step
        with self._pool:
            return self._step_ops(disc, wrapped)

    def _step_ops(self, disc, wrapped):
        from .losses import gan_losses, grad_wrt_input
        if wrapped:
            disc.zero_grad()
        else:
            for p in disc.parameters():
                p.grad = None
        if self._cat:
            loss, parts = self._losses_cat(disc)
            return self._backward(loss, parts, wrapped)
        th_real, th_fake = (self.th_real, self.th_fake) if self._geom else (None, None)
        x_real = self.x_real.detach().requires_grad_()   # (a fresh leaf over the static buffer: nothing writes it in the step)
        # The fake branch (forward, and -- autograd runs a node's backward on its forward's stream -- its backward) goes to a
        # second stream: the step is a chain of ~110 launches of a few microseconds, each waiting for its predecessor; the
        # real branch (forward + R1 double backward) is two thirds of them, and the captured graph runs the two side by side.
        main = torch.cuda.current_stream()
        fork = self._fork if FORK else None
        if fork is not None:
            fork.wait_stream(main)
        with torch.cuda.stream(fork) if fork is not None else contextlib.nullcontext():
            d_fake = disc(self.x_fake, aug_theta=th_fake)    # (the reference marks x_fake requires_grad too: a gradient nothing reads)
            pose = self.prior.pose_to_vec_repr(self.c2b) if d_fake.size(1) > 1 else None
        d_real = disc(x_real, aug_theta=th_real)
        gx = grad_wrt_input(d_real[:, :1], x_real)        # R1: d sum(d_real[:, 0]) / d x_real, graph kept
        if fork is not None:
            main.wait_stream(fork)
        # BCE(real, 1) + BCE(fake, 0) + reg_weight R1 + aux_w MSE(pose): one launch forward, one backward (losses.gan_losses)
        loss, parts = gan_losses(d_real, d_fake, pose, gx, self.aux_w if pose is not None else None, self.reg_weight)
        return self._backward(loss, parts, wrapped)

    def _losses_cat(self, disc):
        """One pass over [real; fake]: D is per-sample (no batch statistics), so row b of the output depends on image b only.
        R1's inner gradient is d sum(d[:B, 0]) / d x_all -- its fake half is exactly zero and contributes nothing."""
        from .losses import gan_losses_cat, grad_wrt_input
        B = self.x_real.shape[0]
        x = self.x_cat.detach().requires_grad_()
        d = disc(x, aug_theta=self.th_cat if self._geom else None)
        if self._gsel is None or self._gsel.shape != d.shape:
            self._gsel = torch.zeros_like(d)
            self._gsel[:B, 0] = 1.0
        gx = grad_wrt_input(d, x, self._gsel)
        pose = self.prior.pose_to_vec_repr(self.c2b) if d.size(1) > 1 else None
        return gan_losses_cat(d, B, pose, gx, self.aux_w if pose is not None else None, self.reg_weight)

    def _backward(self, loss, parts, wrapped):
        # only the parameters' gradients: not the images' (see oi_amd.trainer._backward_to).  The convolution weights collect
        # their four contributions (real, R1 x2, fake) in place: the flat gradient buffer under FlatGradDDP (just zeroed),
        # pre-zeroed pool memory otherwise
        from . import ops
        params = [p for p in self._net().parameters() if p.requires_grad]
        from .autograd_conv import FUSED_BWD
        convw = [p for p in params if p.dim() == 4 and tuple(p.shape[2:]) == (4, 4)] if FUSED_BWD else []
        sink = {p.data_ptr(): (p.grad if wrapped else ops._new_acc(p, *p.shape)) for p in convw}
        with ops.GradSink(sink):
            torch.autograd.backward(loss, grad_tensors=self._one, inputs=params)
        if not wrapped:
            for p in convw:
                assert p.grad is None, "a convolution weight received a gradient outside the sink"
                p.grad = sink[p.data_ptr()]
        return parts   # [fake + real, reg, fake, real, aux]

    @staticmethod
    def _named(vec):
        return {"loss": vec[0], "reg": vec[1], "fake": vec[2], "real": vec[3], "aux_pose": vec[4]}

    def _thetas(self, shape):
        """Host-side augmentation parameters in the eager draw order: real batch, then fake batch."""
        aug = self._net().aug
        B, C, H, W = shape
        dummy = torch.empty(B, C, H, W, device="meta")
        m = aug.static_margins(H, W)
        out = []
        for _ in range(2):
            G = aug.sample_G_inv(dummy)
            if G is None:
                import numpy as np
                G = np.tile(np.eye(3, dtype=np.float32), (B, 1, 1))
            out.append(aug.theta_for(G, m, H, W))
        return out

    def _upload(self, x_real, x_fake, c2b, aux_w):
        from . import ops
        copies = [(x_real, self.x_real), (x_fake, self.x_fake), (c2b, self.c2b)]
        if self._imm.numel() <= 64:  # (batches of up to 5 images: everything in one launch)
            import numpy as np
            th = self._thetas(tuple(x_real.shape)) if self._geom else None
            flat = np.zeros(self._imm.numel(), np.float32)
            if th is not None:
                flat[:-1] = np.concatenate([np.asarray(th[0], np.float32).ravel(), np.asarray(th[1], np.float32).ravel()])
            flat[-1] = float(aux_w)
            ops.stage_inputs(copies, flat, self._imm)
            return
        if self._geom:
            th = self._thetas(tuple(x_real.shape))
            i = self._pin_i = (self._pin_i + 1) % len(self._pins)
            if self._pin_ev[i] is not None:
                self._pin_ev[i].synchronize()
            pin = self._pins[i]
            pin[0].numpy()[:] = th[0]
            pin[1].numpy()[:] = th[1]
            self.th_cat.copy_(pin.view(-1, 2, 3), non_blocking=True)   # (th_real | th_fake are its halves)
            self._pin_ev[i] = torch.cuda.Event()
            self._pin_ev[i].record()
        ops.stage_inputs(copies)
        self.aux_w.fill_(float(aux_w))

    def capture(self, x_real, x_fake, c2b, aux_w):
        import numpy as np
        self._alloc(x_real, x_fake, c2b)
        state = np.random.get_state()       # warm-up / capture must not consume the trainer's random stream
        self._upload(x_real, x_fake, c2b, aux_w)
        # warm-up and capture on ONE stream: autograd pins every AccumulateGrad node to the stream its parameter was first
        # used on, and a capture that meets nodes of another stream warns ("may break CUDA graph capture")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.out = self._step()
        self.stream = side  # an EAGER step on the same parameters should run under it too (their AccumulateGrad nodes live here)
        np.random.set_state(state)
        self._sig = (tuple(x_real.shape), tuple(x_fake.shape), None if c2b is None else tuple(c2b.shape))
        return self

    def __call__(self, x_real, x_fake, c2b=None, aux_w=0.0):
        self.prepare(x_real, x_fake, c2b, aux_w)
        return self.run()

    def prepare(self, x_real, x_fake, c2b=None, aux_w=0.0):
        """First half of a call: (re)capture if the shapes changed, draw the augmentation parameters on the host (numpy, the eager
        order: this is where the step consumes the random stream) and stage the inputs -- one launch on the current stream."""
        sig = (tuple(x_real.shape), tuple(x_fake.shape), None if c2b is None else tuple(c2b.shape))
        if self.graph is None or sig != self._sig:
            self.capture(x_real, x_fake, c2b, aux_w)
        self._upload(x_real, x_fake, c2b, aux_w)

    def run(self):
        """Second half: replay on the current stream (after `prepare` on the same stream, or on one that waits for it)."""
        if os.environ.get("OI_GRAPH_D_EAGER") == "1":   # debugging aid: the same shape-static step, launch by launch
            vec = self._step()
        else:
            self.graph.replay()
            vec = self.out.clone()
        if hasattr(self.disc, "flat_grad"):
            self.disc._exchange()  # the replayed backward filled the flat buffer: the collective starts now
        return self._named(vec)


class GraphedDForward:
    """hipGraph of the no-grad ADA-discriminator forward (augmentation chain + convolution chain: ~20 launches of ~5 us,
    i.e. host-bound at batch 1).  Same recipe as GraphedDStep: static padding margins, augmentation parameters drawn by
    numpy on the host in the eager order and uploaded through a ring of pinned buffers, the input copied into a fixed
    buffer.  The returned tensor is the graph's output buffer: read it (or clone it) before the next call."""

    def __init__(self, disc):
        self.disc, self.graph = disc, None

    def _thetas(self, shape):
        import numpy as np
        aug = self.disc.aug
        B, C, H, W = shape
        G = aug.sample_G_inv(torch.empty(B, C, H, W, device="meta"))
        if G is None:
            G = np.tile(np.eye(3, dtype=np.float32), (B, 1, 1))
        return aug.theta_for(G, aug.static_margins(H, W), H, W)

    def _upload(self, x):
        from . import ops
        if self.theta.numel() <= 64:  # (up to 10 images: the matrices travel in the arguments of the copy launch)
            th = self._thetas(tuple(x.shape)) if self._geom else None
            ops.stage_inputs([(x, self.x)], None if th is None else th.ravel(), self.theta)
            return
        if self._geom:
            th = self._thetas(tuple(x.shape))
            i = self._pin_i = (self._pin_i + 1) % len(self._pins)
            if self._pin_ev[i] is not None:
                self._pin_ev[i].synchronize()
            self._pins[i].numpy()[:] = th
            self.theta.copy_(self._pins[i], non_blocking=True)
            self._pin_ev[i] = torch.cuda.Event()
            self._pin_ev[i].record()
        self.x.copy_(x, non_blocking=True)

    def _library_graph(self, x):
        """Batch <= 4 of the 64 x 64 network: the library's own graph (ops.DiscGraph) -- image pointer and sampling matrices are
        node parameters, so a call is the host-side draw + ONE graph launch (no staging launch)."""
        from . import ops
        d = self.disc
        aug = getattr(d, "aug", None)
        with torch.no_grad():
            ok = d._small_ok(x)
        if not ok or os.environ.get("OI_GRAPH_D_LIBRARY", "1") == "0" or (aug is not None and not aug.is_stock()):
            return None
        geom = aug is not None and _has_geometric(aug)
        H, W = x.shape[2:]
        return ops.DiscGraph(tuple(x.shape), x.device, *d.live_weights(), f12=aug.Hz_geom if geom else None,
                             margins=aug.static_margins(H, W) if geom else None,
                             launch="eager" if len(d.blocks) == 5 else None), geom   # (the 128 x 128 plan: launch by launch only)

    def capture(self, x):
        import numpy as np
        B = x.shape[0]
        lib = self._library_graph(x)
        if lib is not None:
            self._lib, self._geom = lib
            self.x, self.graph = torch.empty(x.shape, device="meta"), "library"   # (shape bookkeeping only)
            return self
        self._lib = None
        self.x = torch.empty_like(x)
        self.theta = torch.empty(B, 2, 3, device=x.device)
        self._pins = [torch.empty(B, 2, 3, pin_memory=True) for _ in range(8)]
        self._pin_ev = [None] * 8
        self._pin_i = 0
        self._geom = _has_geometric(self.disc.aug)  # nothing to do -> nothing captured (the eager path returns x)
        theta = self.theta if self._geom else None
        state = np.random.get_state()   # warm-up / capture must not consume the caller's random stream
        self._upload(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(2):
                self.disc(self.x, aug_theta=theta)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side), torch.no_grad():
            self.out = self.disc(self.x, aug_theta=theta)
        np.random.set_state(state)
        return self

    def __call__(self, x):
        if self.graph is None or tuple(x.shape) != tuple(self.x.shape):
            self.capture(x)
        if self._lib is not None:
            aug = getattr(self.disc, "aug", None)
            if self._geom and aug.fast_draw_ok():   # the shipped configuration: one seed from numpy's stream, draws in the library
                return self._lib.call_ada(x.float().contiguous(), aug.draw_seed(), *aug.fast_params())
            return self._lib(x.float(), self._thetas(tuple(x.shape)) if self._geom else None)
        self._upload(x)
        self.graph.replay()
        return self.out
