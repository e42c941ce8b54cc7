"""Thin functional wrappers: torch tensors in/out, HIP kernels underneath (no autograd here).

Every function allocates its outputs with the torch caching allocator, passes raw device
pointers + the *current* HIP stream to liboi_hip.so, and returns immediately (stream ordered).
Autograd structure lives in `oi_amd.autograd`."""
import ctypes
import os

import numpy as np
import torch

from . import lib as _l

_vp = ctypes.c_void_p


def _stream():
    """Raw hipStream_t of torch's current stream on the current device.  torch.cuda.current_stream() builds a Python
    Stream object (~8 us); the two C accessors below cost ~0.3 us and this runs once per kernel launch."""
    return _vp(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _l.OiHipError("oi_amd ops need CUDA/HIP tensors (there is no CPU path)")
    if t.dtype not in (torch.float32, torch.uint8):
        raise _l.OiHipError(f"expected float32 tensor, got {t.dtype}")
    if not t.is_contiguous():
        raise _l.OiHipError("expected a contiguous tensor")
    return _vp(t.data_ptr())


def _c(t):
    return t.contiguous().float() if t is not None else None


def _new(ref, *shape):
    return torch.empty(shape, dtype=torch.float32, device=ref.device)


class ZeroPool:
    """Pre-zeroed memory for the accumulate-outputs (split-K sums, scatter-adds) of ONE captured step: a single fill at
    the start of the step instead of a fill launch in front of every such op (93 of 631 launches of a training iteration
    were fills).  Bump allocation in call order; while active, the library is told not to clear those outputs itself
    (oi_outputs_prezeroed_stream, for this stream only).  The first pass only measures (every request is served by its own torch.zeros); the buffer is
    allocated at the next `begin()`.  Slices stay valid until the next `begin()` -- the owner (oi_amd.graphed.GraphedDStep)
    guarantees that nothing outlives its step except what the optimiser reads before the next one starts."""

    _active = {}   # raw stream handle -> the pool that is active for launches on that stream

    def __init__(self):
        self.buf, self.off, self.need = None, 0, 0

    def begin(self, device, must_not_alias=()):
        """Start of a step: (re)allocate if the last pass asked for more, then ONE fill of what the step will hand out.
        `must_not_alias`: parameters whose `.grad` must not live in the pool any more (a gradient kept across steps --
        gradient accumulation, zero_grad(set_to_none=False) -- would be zeroed under its owner: fail loudly instead)."""
        if self.buf is not None and must_not_alias:
            lo, hi = self.buf.data_ptr(), self.buf.data_ptr() + self.buf.numel() * 4
            for p_ in must_not_alias:
                g_ = p_.grad
                if g_ is not None and lo <= g_.data_ptr() < hi:
                    raise RuntimeError("ZeroPool.begin: a parameter's .grad still points into the pool of the previous step; call "
                                       "zero_grad(set_to_none=True) before the step (or clone gradients that must outlive it)")
        if self.buf is None or self.buf.numel() < self.need:
            self.buf = torch.empty(self.need, dtype=torch.float32, device=device) if self.need else None
        self.off, self.need = 0, 0
        if self.buf is not None:
            _l.check(_l.load().oi_zero_fill(_p(self.buf), self.buf.numel(), _stream()), "oi_zero_fill")

    def take(self, ref, shape):
        n = int(torch.Size(shape).numel())
        n4 = (n + 63) // 64 * 64       # 256-byte granules
        self.need += n4
        if self.buf is None or self.off + n4 > self.buf.numel():
            dev = ref if isinstance(ref, torch.device) else ref.device
            return torch.zeros(shape, dtype=torch.float32, device=dev)   # measuring pass / overflow: its own fill
        out = self.buf[self.off:self.off + n].view(shape)
        self.off += n4
        return out

    def __enter__(self):
        # The declaration belongs to the CURRENT STREAM (oi_outputs_prezeroed_stream): the ops of this step -- forward here,
        # backward on the autograd thread but on the same stream -- take pool memory and skip their fills; any other thread /
        # stream keeps plain torch.empty outputs that the library clears itself.
        self._key = _stream().value or 0
        assert self._key not in ZeroPool._active, "nested ZeroPool on one stream"
        was = _l.load().oi_outputs_prezeroed_stream(_vp(self._key), 1)
        if was < 0:
            _l.check(was, "oi_outputs_prezeroed_stream")
        self._was = was
        ZeroPool._active[self._key] = self
        return self

    def __exit__(self, *exc):
        _l.load().oi_outputs_prezeroed_stream(_vp(self._key), self._was)
        del ZeroPool._active[self._key]
        return False


def _active_pool():
    if not ZeroPool._active:
        return None
    return ZeroPool._active.get(_stream().value or 0)


def _new_acc(ref, *shape):
    """Output buffer of an op that ACCUMULATES into it: plain memory (the launcher clears it) unless a ZeroPool is active."""
    pool = _active_pool()
    return torch.empty(shape, dtype=torch.float32, device=ref.device) if pool is None else pool.take(ref, shape)


def _zeros_split(dev, *shapes):
    """Several zero-initialised fp32 tensors from ONE fill launch (views of one flat buffer, each 16-byte aligned) -- or
    from the step's ZeroPool when one is active (no launch)."""
    pool = _active_pool()
    if pool is not None:
        return [pool.take(dev, sh) for sh in shapes]
    sizes = [int(torch.Size(sh).numel()) for sh in shapes]
    offs, tot = [], 0
    for n in sizes:
        offs.append(tot)
        tot += (n + 3) // 4 * 4
    flat = torch.zeros(tot, dtype=torch.float32, device=dev)
    return [flat[o:o + n].view(sh) for o, n, sh in zip(offs, sizes, shapes)]


# ------------------------------------------------------------------------------------------
# a6 stand-alone: the albedo head on caller-supplied features (csrc/color_head.hip)
# ------------------------------------------------------------------------------------------

def color_head_fwd(feat, normals, gamma, beta, wv, bv, wrgb, brgb, B):
    """feat (n,128), normals (n,3), gamma / beta (B,128) -> rgb (n,3); n = B * points per element (element-major rows)."""
    n = feat.shape[0]
    assert n % B == 0 and feat.shape[1] == 128 and normals.shape == (n, 3) and gamma.shape == (B, 128) == beta.shape
    rgb = _new(feat, n, 3)
    _l.check(_l.load().oi_color_head_fwd(_p(feat), _p(normals), _p(gamma), _p(beta), 128, _p(wv), _p(bv), _p(wrgb), _p(brgb),
                                         _p(rgb), B, n // B, _stream()), "oi_color_head_fwd")
    return rgb


def color_head_bwd(feat, normals, gamma, beta, wv, bv, wrgb, brgb, g_rgb, B):
    """-> d_feat, d_normals, d_gamma, d_beta, d_wv, d_bv, d_wrgb, d_brgb (all assigned; fixed summation order)."""
    L = _l.load()
    n = feat.shape[0]
    ws_bytes = int(L.oi_color_head_bwd_workspace_bytes(B, n // B))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=feat.device)
    d_feat, d_normals = _new(feat, n, 128), _new(feat, n, 3)
    d_gamma, d_beta = _new(feat, B, 128), _new(feat, B, 128)
    d_wv, d_bv, d_wrgb, d_brgb = _new(feat, 128, 131), _new(feat, 128), _new(feat, 3, 128), _new(feat, 3)
    _l.check(L.oi_color_head_bwd(_p(feat), _p(normals), _p(gamma), _p(beta), 128, _p(wv), _p(bv), _p(wrgb), _p(brgb), _p(g_rgb),
                                 _p(d_feat), _p(d_normals), _p(d_gamma), _p(d_beta), 128, _p(d_wv), _p(d_bv), _p(d_wrgb),
                                 _p(d_brgb), _p(ws), ws_bytes, B, n // B, _stream()), "oi_color_head_bwd")
    return d_feat, d_normals, d_gamma, d_beta, d_wv, d_bv, d_wrgb, d_brgb


# ------------------------------------------------------------------------------------------
# MLP
# ------------------------------------------------------------------------------------------

def film_params(style_w, style_b, gw, gb, bw, bb, z=None, w=None):
    """(w, gamma[B,NL,128], beta[B,NL,128]); give z (style MLP runs) or w.  Without FiLM heads (gw None: the style MLP
    alone) gamma and beta are None -- the kernel writes none."""
    L = _l.load()
    assert (z is None) != (w is None)
    src = z if z is not None else w
    B, NL = src.shape[0], (gw.shape[0] if gw is not None else 0)
    w_out = _new(src, B, 64) if w is None else _c(w)
    gamma, beta = (_new(src, B, NL, 128), _new(src, B, NL, 128)) if NL else (None, None)
    z_ = _c(z)
    args = [_c(style_w), _c(style_b), z_, w_out, _c(gw), _c(gb), _c(bw), _c(bb)]
    _l.check(L.oi_film_params(*[_p(a) for a in args], _p(gamma), _p(beta), B, NL, _stream()), "oi_film_params")
    return w_out, gamma, beta


def prep_render(b2w, w2b, c2b, offs, bg, kinv, R, S, jitter, light_direction, film_P, z, jitter_normal=False, f3_packed=None,
                f3_blob=None):
    """ONE launch for everything a render needs before its first MLP pass (oi_prep_render): the pose block (numpy, host) goes
    BY VALUE in the kernel arguments; rays, near / far, light direction, coarse samples + points and the style MLP + FiLM
    parameters come back.  -> dict(pose (53 B: b2w | w2b | c2b | offs | bg blocks), rays_o, rays_d, near, far, light_dir, z_coarse, pts_coarse, w, gamma, beta)."""
    L = _l.load()
    B = b2w.shape[0]
    assert B <= _l.PREP_MAX_B and z is not None
    dev = z.device
    P = _l.PrepParams()
    for name, arr, n in (("b2w", b2w, 16), ("w2b", w2b, 16), ("c2b", c2b, 16), ("offs", offs, 2), ("bg", bg, 3)):
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(B, n)
        dst = np.frombuffer(getattr(P, name), dtype=np.float32).reshape(_l.PREP_MAX_B, n)
        dst[:B] = a
    NL = film_P["gw"].shape[0]
    N = B * R * R
    f = lambda *sh: _new(z, *sh)
    out = {"pose": f(B * 53), "rays_o": f(B, R, R, 3), "rays_d": f(B, R, R, 3), "near": f(N, 1), "far": f(N, 1),
           "light_dir": f(B, 3), "z_coarse": f(N, S), "pts_coarse": f(N, S, 3), "w": f(B, 64), "gamma": f(B, NL, 128),
           "beta": f(B, NL, 128)}
    P.B, P.R, P.S, P.NL = B, int(R), int(S), NL
    keep = [_c(kinv), _c(light_direction), _c(jitter), _c(z)] + [_c(film_P[k]) for k in ("style_w", "style_b", "gw", "gb", "bw", "bb")]
    P.kinv, P.light_direction, P.jitter, P.z = (_p(t) for t in keep[:4])
    P.style_w, P.style_b, P.gw, P.gb, P.bw, P.bb = (_p(t) for t in keep[4:])
    P.pose_out, P.rays_o, P.rays_d, P.near_, P.far_ = (_p(out[k]) for k in ("pose", "rays_o", "rays_d", "near", "far"))
    P.light_dir, P.z_coarse, P.pts_coarse = _p(out["light_dir"]), _p(out["z_coarse"]), _p(out["pts_coarse"])
    P.w_out, P.gamma, P.beta = _p(out["w"]), _p(out["gamma"]), _p(out["beta"])
    P.jitter_normal = int(bool(jitter_normal))
    if f3_blob is not None:   # the f16x3 kernel's per-element blobs, formed by the FiLM workgroups (oi_sdf_mlp_fwd_ex / OI_MLP_BLOB_READY)
        P.f3_packed, P.f3_blob = _p(f3_packed), _p(f3_blob)
    _l.check(L.oi_prep_render(ctypes.byref(P), _stream()), "oi_prep_render")
    return out


def film_params_bwd(d_gamma, d_beta, w, gw, bw, style_w=None, style_b=None, z=None, d_w_in=None, want_dz=False):
    """Backward of film_params -> dict(d_gw, d_gb, d_bw, d_bb, d_w [, d_style_w, d_style_b, d_z])."""
    L = _l.load()
    B, NL = d_gamma.shape[0], d_gamma.shape[1]
    d_gamma, d_beta, w = _c(d_gamma), _c(d_beta), _c(w)
    out = {"d_gw": _new(w, *gw.shape), "d_gb": _new(w, NL, 128), "d_bw": _new(w, *bw.shape), "d_bb": _new(w, NL, 128),
           "d_w": _zeros_split(w.device, w.shape)[0] if d_w_in is None else d_w_in.contiguous().clone()}
    if z is not None:
        out["d_style_w"], out["d_style_b"] = _zeros_split(w.device, style_w.shape, style_b.shape)
        if want_dz:
            out["d_z"] = _new(z, *z.shape)
    _l.check(L.oi_film_params_bwd(_p(d_gamma), _p(d_beta), _p(w), _p(_c(gw)), _p(_c(bw)), _p(out["d_gw"]), _p(out["d_gb"]),
                                  _p(out["d_bw"]), _p(out["d_bb"]), _p(out["d_w"]), _p(_c(style_w)), _p(_c(style_b)),
                                  _p(_c(z)), _p(out.get("d_style_w")), _p(out.get("d_style_b")), _p(out.get("d_z")), B, NL,
                                  _stream()), "oi_film_params_bwd")
    return out


def style_bwd(d_w, style_w, style_b, z, want_dz=False):
    """Backward of the style MLP alone (oi_film_params_bwd with no FiLM layer) -> dict(d_style_w, d_style_b [, d_z])."""
    L = _l.load()
    B = z.shape[0]
    out = dict(zip(("d_style_w", "d_style_b"), _zeros_split(z.device, style_w.shape, style_b.shape)))
    if want_dz:
        out["d_z"] = torch.empty_like(z)
    d_w = d_w.contiguous().clone()
    _l.check(L.oi_film_params_bwd(None, None, None, None, None, None, None, None, None, _p(d_w), _p(_c(style_w)),
                                  _p(_c(style_b)), _p(_c(z)), _p(out["d_style_w"]), _p(out["d_style_b"]), _p(out.get("d_z")),
                                  B, 0, _stream()), "oi_film_params_bwd")
    return out


def mlp_pack_weights(w0, b0, wh, bh, wsig, bsig, wv, bv, wrgb, brgb, prec):
    L = _l.load()
    packed = torch.empty(L.oi_mlp_packed_bytes(prec), dtype=torch.uint8, device=w0.device)
    args = [_c(t) for t in (w0, b0, wh, bh, wsig.reshape(-1), bsig.reshape(-1), wv, bv, wrgb, brgb)]
    _l.check(L.oi_mlp_pack_weights(*[_p(a) for a in args], _p(packed), prec, _stream()), "oi_mlp_pack_weights")
    return packed


def mlp_pack_status(packed):
    """Raises (OI_ERR_UNSUPPORTED) if the packed image was built from an inf / NaN weight; synchronises the stream."""
    _l.check(_l.load().oi_mlp_pack_status(_p(packed), _stream()), "oi_mlp_pack_status")


def mlp_scratch_bytes(B, n_per_elem, prec=None):
    L = _l.load()
    return L.oi_mlp_scratch_bytes(B, n_per_elem) if prec is None else L.oi_mlp_scratch_bytes_prec(B, n_per_elem, prec)


def sdf_mlp_fwd(pts, packed, gamma, beta, B, prec, fast_trig=False, want_grad=False, want_rgb=False,
                want_feat=False, scratch=None, blob_ready=False):
    """pts (B*n, 3) -> sdf (B*n,), grad (B*n,3)|None, rgb (B*n,3)|None, feat (B*n,128)|None, scratch.
    blob_ready: `scratch` (from f3_scratch_for) already holds the per-element blobs of the f16x3 kernel, written by
    prep_render for these gamma / beta (oi_sdf_mlp_fwd_ex, OI_MLP_BLOB_READY)."""
    L = _l.load()
    pts = _c(pts)
    n_tot = pts.shape[0]
    assert n_tot % B == 0
    n = n_tot // B
    sdf = _new(pts, n_tot)
    grad = _new(pts, n_tot, 3) if want_grad else None
    rgb = _new(pts, n_tot, 3) if want_rgb else None
    feat = _new(pts, n_tot, 128) if want_feat else None
    if want_grad and scratch is None:
        scratch = torch.empty(L.oi_mlp_scratch_bytes_prec(B, n, prec), dtype=torch.uint8, device=pts.device)
    assert not want_rgb or want_grad
    if blob_ready:
        # (== : the blob's offset inside the scratch depends on the point count the scratch was sized for -- f3_scratch_for(B, n))
        assert want_grad and prec == _l.OI_PREC_F16X3 and scratch.numel() == L.oi_mlp_scratch_bytes_prec(B, n, prec), \
            "blob_ready: the scratch was not made by f3_scratch_for for this (B, n)"
        _l.check(L.oi_sdf_mlp_fwd_ex(_p(pts), _p(packed), _p(gamma), _p(beta), _p(sdf), _p(grad), _p(rgb), _p(feat), _p(scratch), B, n,
                                     prec, int(bool(fast_trig)), _l.OI_MLP_BLOB_READY, _stream()), "oi_sdf_mlp_fwd_ex")
        return sdf, grad, rgb, feat, scratch
    _l.check(L.oi_sdf_mlp_fwd(_p(pts), _p(packed), _p(gamma), _p(beta), _p(sdf), _p(grad), _p(rgb), _p(feat),
                              _p(scratch) if want_grad else None, B, n, prec, int(bool(fast_trig)), _stream()),
             "oi_sdf_mlp_fwd")
    return sdf, grad, rgb, feat, scratch


def f3_scratch_for(B, n, device):
    """(scratch, blob view) of the f16x3 gradient pass over n points per element: the blob view is where oi_prep_render writes the
    per-element blobs (its f3_blob field) that OI_MLP_BLOB_READY then promises."""
    L = _l.load()
    scratch = torch.empty(L.oi_mlp_scratch_bytes_prec(B, n, _l.OI_PREC_F16X3), dtype=torch.uint8, device=device)
    off = L.oi_mlp_f3_blob_offset(B, n)
    return scratch, scratch[off:off + B * L.oi_mlp_f3_blob_bytes()]


def bwd_scratch_cap_bytes():
    """Upper bound of the MLP backward's working memory (OI_BWD_SCRATCH_MB, default 9216: the C2 training render fits one chunk): larger problems run in chunks."""
    return int(float(os.environ.get("OI_BWD_SCRATCH_MB", "9216")) * (1 << 20))


def sdf_mlp_bwd(pts, packed, gamma, beta, grad_fwd, rgb_fwd, feat_fwd, g_sdf, g_grad, g_rgb, B, prec, fast_trig=False,
                scratch_cap=None, g_feat=None):
    """-> d_small (flat), d_wmat (8,128,128), d_gamma (B,9,128), d_beta (B,9,128).  Working memory is bounded by
    `scratch_cap` bytes (default bwd_scratch_cap_bytes()); the library processes the points in chunks that fit.
    `g_feat` (n,128): upstream gradient of the feature output (oi_sdf_mlp_bwd_feat; None = the fused-path kernel)."""
    L = _l.load()
    pts = _c(pts)
    n = pts.shape[0] // B
    dev = pts.device
    d_small, d_wmat, d_gamma, d_beta = _zeros_split(dev, (L.oi_mlp_bwd_small_floats(),), (8, 128, 128), (B, 9, 128),
                                                    (B, 9, 128))
    nbytes = L.oi_mlp_bwd_scratch_bytes_capped(B, n, bwd_scratch_cap_bytes() if scratch_cap is None else int(scratch_cap))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = [_c(t) for t in (grad_fwd, rgb_fwd, feat_fwd, g_sdf, g_grad, g_rgb)]
    if g_feat is None:
        _l.check(L.oi_sdf_mlp_bwd(_p(pts), _p(packed), _p(_c(gamma)), _p(_c(beta)), *[_p(a) for a in args], _p(d_small),
                                  _p(d_wmat), _p(d_gamma), _p(d_beta), _p(scratch), nbytes, B, n, prec, int(bool(fast_trig)),
                                  _stream()), "oi_sdf_mlp_bwd")
    else:
        _l.check(L.oi_sdf_mlp_bwd_feat(_p(pts), _p(packed), _p(_c(gamma)), _p(_c(beta)), *[_p(a) for a in args], _p(_c(g_feat)),
                                       _p(d_small), _p(d_wmat), _p(d_gamma), _p(d_beta), _p(scratch), nbytes, B, n, prec,
                                       int(bool(fast_trig)), _stream()), "oi_sdf_mlp_bwd_feat")
    return d_small, d_wmat, d_gamma, d_beta


# ------------------------------------------------------------------------------------------
# rays / sampling / compositing
# ------------------------------------------------------------------------------------------

def gen_rays(c2b, kinv3, offs, R, w2b=None, light_direction=None):
    """-> rays_o, rays_d, near, far [, light_dir (B, 3) when `w2b` and the raw `light_direction` parameter are given]"""
    L = _l.load()
    B = c2b.shape[0]
    ro, rd = _new(c2b, B, R, R, 3), _new(c2b, B, R, R, 3)
    near, far = _new(c2b, B * R * R, 1), _new(c2b, B * R * R, 1)
    if w2b is None:
        _l.check(L.oi_gen_rays(_p(_c(c2b)), _p(_c(kinv3)), _p(_c(offs)), B, R, _p(ro), _p(rd), _p(near), _p(far),
                               _stream()), "oi_gen_rays")
        return ro, rd, near, far
    ldir = _new(c2b, B, 3)
    _l.check(L.oi_gen_rays_light(_p(_c(c2b)), _p(_c(kinv3)), _p(_c(offs)), B, R, _p(ro), _p(rd), _p(near), _p(far),
                                 _p(_c(w2b)), _p(_c(light_direction.detach())), _p(ldir), _stream()), "oi_gen_rays_light")
    return ro, rd, near, far, ldir


def coarse_samples(rays_o, rays_d, near, far, S, jitter=None):
    L = _l.load()
    N = rays_o.shape[0]
    z, pts = _new(rays_o, N, S), _new(rays_o, N, S, 3)
    _l.check(L.oi_coarse_samples(_p(_c(rays_o)), _p(_c(rays_d)), _p(_c(near)), _p(_c(far)), _p(_c(jitter)), N, S,
                                 _p(z), _p(pts), _stream()), "oi_coarse_samples")
    return z, pts


def upsample(rays_o, rays_d, z, sdf, n_new, inv_s, merge=True, mid_last_dist=None):
    """-> z_new, pts_new, z_merged [, (dists, mid_z, pts_mid) when `mid_last_dist` is given: the section mid-points of the
    merged list from the same launch (oi_upsample_mid = oi_upsample + oi_midpoints, bit-identical)]."""
    L = _l.load()
    N, Sc = z.shape
    z_new, pts_new = _new(z, N, n_new), _new(z, N, n_new, 3)
    if mid_last_dist is not None:
        T = Sc + n_new
        z_merged, dists, mid_z, pts = _new(z, N, T), _new(z, N, T), _new(z, N, T), _new(z, N, T, 3)
        _l.check(L.oi_upsample_mid(_p(_c(rays_o)), _p(_c(rays_d)), _p(_c(z)), _p(_c(sdf)), N, Sc, n_new, float(inv_s),
                                   _p(z_new), _p(pts_new), _p(z_merged), float(mid_last_dist), _p(dists), _p(mid_z), _p(pts),
                                   _stream()), "oi_upsample_mid")
        return z_new, pts_new, z_merged, (dists, mid_z, pts)
    z_merged = _new(z, N, Sc + n_new) if merge else None
    _l.check(L.oi_upsample(_p(_c(rays_o)), _p(_c(rays_d)), _p(_c(z)), _p(_c(sdf)), N, Sc, n_new, float(inv_s),
                           _p(z_new), _p(pts_new), _p(z_merged), _stream()), "oi_upsample")
    return z_new, pts_new, z_merged


def merge_sorted(z, sdf, z_new, sdf_new):
    L = _l.load()
    N, Sc = z.shape
    n_new = z_new.shape[1]
    zo, so = _new(z, N, Sc + n_new), _new(z, N, Sc + n_new)
    _l.check(L.oi_merge_sorted(_p(_c(z)), _p(_c(sdf)), _p(_c(z_new)), _p(_c(sdf_new)), N, Sc, n_new, _p(zo), _p(so),
                               _stream()), "oi_merge_sorted")
    return zo, so


def midpoints(rays_o, rays_d, z, last_dist):
    L = _l.load()
    N, T = z.shape
    dists, mid_z, pts = _new(z, N, T), _new(z, N, T), _new(z, N, T, 3)
    _l.check(L.oi_midpoints(_p(_c(rays_o)), _p(_c(rays_d)), _p(_c(z)), N, T, float(last_dist), _p(dists), _p(mid_z),
                            _p(pts), _stream()), "oi_midpoints")
    return dists, mid_z, pts


PER_SAMPLE_OUT = ("weights", "cdf", "alpha", "inside_sphere", "pts_norm")
PER_RAY_OUT = {"weight_sum": 1, "weight_max": 1, "color_fine": 3, "image_no_bg": 3, "image": 3, "shading": 1,
               "normal": 3, "mask": 1, "z_map": 1, "specular_map": 1, "diffuse_map": 1}


_STATS_TICKETS = {}
# oi_composite_fwd can do oi_render_stats' work itself (its last workgroup sums the partials: stats16 / stats_ticket).  Measured
# at C2 (1024 workgroups, rocprofv3): 25.7 us for the one launch against 14.4 + 4.7 us for the two -- the reduction then sits
# behind the slowest workgroup as a chain of round trips (store acknowledgement, two arrival counters, the loads) that costs
# more than the launch boundary it replaces.  Default: two launches; the one-launch form stays tested (bit-identical).
FUSED_STATS = False


def _stats_ticket(dev):
    """One zero-initialised device word per (device, stream): the arrival counter of the compositing launch's last-block
    reduction (the kernel leaves it at zero; launches that may overlap must not share one)."""
    key = (dev, _stream().value or 0)
    t = _STATS_TICKETS.get(key)
    if t is None:
        t = _STATS_TICKETS[key] = torch.zeros(_l.TICKET_WORDS, dtype=torch.int32, device=dev)
    return t


def composite_fwd(sdf, grad, rgb, dists, mid_z, rays_o, rays_d, light_dir, bg, variance, light, cos_anneal_ratio,
                  B, outputs=None, image_planar=False):
    """Returns dict of requested outputs (default: all) + 'reduce4' = [sum m*(|g|-1)^2, sum m, sum exp(-100|sdf|), 0].
    With 'reduce4' come two forward-only extras from the SAME launch (its last workgroup does oi_render_stats' sums):
    'ray_sums' = [sum cdf[:,0], sum weight_max, sum weight_sum, 0] and 'finals' = [gradient_error, surface_loss, the three
    means].  `image_planar`: 'image' comes back as (B, 3, N / B) -- the (B, 3, H, W) map itself -- instead of (N, 3)."""
    L = _l.load()
    N, T = dists.shape
    P = _l.CompositeParams()
    keep = []
    for name, t in (("sdf", sdf), ("grad", grad), ("rgb", rgb), ("dists", dists), ("mid_z", mid_z), ("rays_o", rays_o),
                    ("rays_d", rays_d), ("light_dir", light_dir), ("bg", bg), ("variance", variance.reshape(1)),
                    ("light", light)):
        t = _c(t)
        keep.append(t)
        setattr(P, name, _p(t))
    P.cos_anneal_ratio = float(cos_anneal_ratio)
    P.N, P.T, P.B = N, T, B
    want = set(outputs) if outputs is not None else set(PER_SAMPLE_OUT) | set(PER_RAY_OUT) | {"reduce4"}
    out = {}
    for name in PER_SAMPLE_OUT:
        if name in want:
            out[name] = _new(dists, N, T)
        setattr(P, name, _p(out.get(name)))
    for name, c in PER_RAY_OUT.items():
        if name in want:
            out[name] = _new(dists, B, 3, N // B) if (name == "image" and image_planar) else _new(dists, N, c)
        setattr(P, name, _p(out.get(name)))
    P.image_planar = int(bool(image_planar))
    partials = out16 = None
    if "reduce4" in want:  # per-block partial sums (no atomics), reduced by the launch's last workgroup in a fixed order
        partials = _new(dists, L.oi_composite_num_blocks(N), 8)
        out16 = _new(dists, 16)
        if FUSED_STATS:
            ticket = _stats_ticket(dists.device)
            P.stats16, P.stats_ticket = _p(out16), _vp(ticket.data_ptr())
    P.reduce4 = None
    P.block_partials = _p(partials)
    _l.check(L.oi_composite_fwd(ctypes.byref(P), _stream()), "oi_composite_fwd")
    if partials is not None:
        if not FUSED_STATS:  # the two-launch form (kept as the yardstick of tests/test_gpu_kernels.py)
            _l.check(L.oi_render_stats(_p(partials), partials.shape[0], N, T, _p(out16), _stream()), "oi_render_stats")
        out["reduce4"], out["ray_sums"], out["finals"] = out16[0:4], out16[4:8], out16[8:13]
    return out


GRAD_IN = ("weights", "weight_sum", "color_fine", "image_no_bg", "image", "shading", "normal", "mask", "z_map",
           "specular_map", "diffuse_map", "reduce4")


def composite_bwd(sdf, grad, rgb, dists, mid_z, rays_o, rays_d, light_dir, bg, variance, light, cos_anneal_ratio, B,
                  gouts, image_planar=False):
    """gouts: dict name -> upstream gradient (missing / None = zero).  -> d_sdf, d_grad, d_rgb, d_variance (1,),
    d_light (3,), d_light_dir (B,3).  `image_planar`: gouts["image"] is (B, 3, N / B), the layout the forward wrote."""
    L = _l.load()
    N, T = dists.shape
    P = _l.CompositeParams()
    keep = []
    for name, t in (("sdf", sdf), ("grad", grad), ("rgb", rgb), ("dists", dists), ("mid_z", mid_z), ("rays_o", rays_o),
                    ("rays_d", rays_d), ("light_dir", light_dir), ("bg", bg), ("variance", variance.reshape(1)),
                    ("light", light)):
        t = _c(t)
        keep.append(t)
        setattr(P, name, _p(t))
    P.cos_anneal_ratio = float(cos_anneal_ratio)
    P.N, P.T, P.B = N, T, B
    P.image_planar = int(bool(image_planar))
    G = _l.CompositeGrads()
    for name in GRAD_IN:
        t = _c(gouts.get(name))
        keep.append(t)
        setattr(G, "g_" + name, _p(t))
    dev = dists.device
    d_sdf, d_grad, d_rgb = _new(dists, N, T), _new(dists, N, T, 3), _new(dists, N, T, 3)
    d_var, d_light, d_ldir = _zeros_split(dev, (1,), (3,), (B, 3))
    G.d_sdf, G.d_grad, G.d_rgb = _p(d_sdf), _p(d_grad), _p(d_rgb)
    G.d_variance, G.d_light, G.d_light_dir = _p(d_var), _p(d_light), _p(d_ldir)
    partials = _new(dists, N, 8)  # per-ray partial sums of the global gradients, reduced by a second small kernel
    G.ray_partials = _p(partials)
    _l.check(L.oi_composite_bwd(ctypes.byref(P), ctypes.byref(G), _stream()), "oi_composite_bwd")
    return d_sdf, d_grad, d_rgb, d_var, d_light, d_ldir


RELIGHT_OUT = ("image", "image_no_bg", "shading", "diffuse", "specular")


def relight_fwd(weights, grad, rgb, mid_z, rays_o, rays_d, w2b, lights, bg, B, outputs=("image",), out=None):
    """Shades and composites a captured render under L lights in one launch (oi_relight_fwd, include/oi_relight.h).
    weights / mid_z (N, T), grad / rgb (N, T, 3), rays_o / rays_d (N, 3), w2b (B, 4, 4), lights (L, 16) (oi_amd.relight.
    stack_lights), bg (B, 3) or None.  -> {name: (L, B, 3, N / B)} for each name of `outputs` (RELIGHT_OUT).
    `out`: {name: (L, B, 3, N / B) contiguous tensor} to write into instead of new buffers."""
    L_ = _l.load()
    N, T = weights.shape
    nl = lights.shape[0]
    for name in outputs:
        if name not in RELIGHT_OUT:
            raise ValueError(f"relight_fwd: unknown output {name!r} (one of {RELIGHT_OUT})")
    if nl < 1 or nl > _l.RELIGHT_MAX_LIGHTS or tuple(lights.shape[1:]) != (_l.RELIGHT_LIGHT_FLOATS,):
        raise ValueError(f"relight_fwd: lights {tuple(lights.shape)}, expected (L, {_l.RELIGHT_LIGHT_FLOATS}) with 1 <= L <= "
                         f"{_l.RELIGHT_MAX_LIGHTS}")
    if B < 1 or N % B != 0:
        raise ValueError(f"relight_fwd: {N} rays cannot be split over {B} elements")
    P = _l.RelightParams()
    keep = []
    for name, t in (("weights", weights), ("grad", grad), ("rgb", rgb), ("mid_z", mid_z), ("rays_o", rays_o),
                    ("rays_d", rays_d), ("w2b", w2b), ("lights", lights), ("bg", bg)):
        t = _c(t)
        keep.append(t)
        setattr(P, name, _p(t))
    P.N, P.T, P.B, P.L = N, T, B, nl
    res = {}
    for name in RELIGHT_OUT:
        if name in outputs:
            t = out.get(name) if out is not None else None
            if t is None:
                t = _new(weights, nl, B, 3, N // B)
            elif tuple(t.shape) != (nl, B, 3, N // B) or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError(f"relight_fwd: out[{name!r}] must be a contiguous float32 {(nl, B, 3, N // B)} tensor")
            res[name] = t
        setattr(P, name, _p(res.get(name)))
    _l.check(L_.oi_relight_fwd(ctypes.byref(P), _stream()), "oi_relight_fwd")
    return res


# ------------------------------------------------------------------------------------------
# intrinsic mesh export (include/oi_mesh_attr.h); oi_amd.mesh.vertex_attributes sequences these around sdf_mlp_fwd
# ------------------------------------------------------------------------------------------

def _bytes(ref, n):
    return torch.empty(int(n), dtype=torch.uint8, device=ref.device)


def mesh_vertex_world(verts_index, xs, ys, zs):
    """Index-space vertices (V, 3) -> world positions (V, 3) through the lattice's axis arrays, and cleared flags (V,) uint8."""
    V = verts_index.shape[0]
    pos, flags = _new(verts_index, V, 3), _bytes(verts_index, V)
    _l.check(_l.load().oi_mesh_vertex_world(_p(verts_index), V, _p(xs), _p(ys), _p(zs), len(xs), len(ys), len(zs), _p(pos),
                                            _p(flags), _stream()), "oi_mesh_vertex_world")
    return pos, flags


def mesh_newton(pos, pos0, sdf, grad, threshold, limits, residual, flags):
    """One projection step of `pos` (in place) towards sdf = -threshold; residual (V,) and flags (V,) are written / OR-ed."""
    _l.check(_l.load().oi_mesh_newton(_p(pos), _p(pos0), _p(sdf), _p(grad), pos.shape[0], float(threshold),
                                      *(float(v) for v in limits), _p(residual), _p(flags), _stream()), "oi_mesh_newton")


def mesh_attr_finalize(pos, sdf, grad, rgb, threshold, residual=None, want_record=False):
    """-> unit normals (V, 3), albedo (V, 3), the interleaved record (V, 27) uint8 or None; residual (V,) is written."""
    V = pos.shape[0]
    normals, albedo = _new(pos, V, 3), _new(pos, V, 3)
    record = _bytes(pos, V * _l.MESH_RECORD_BYTES).view(V, _l.MESH_RECORD_BYTES) if want_record else None
    _l.check(_l.load().oi_mesh_attr_finalize(_p(pos), _p(sdf), _p(grad), _p(rgb), V, float(threshold), _p(normals),
                                             _p(albedo), _p(residual), _p(record), _stream()), "oi_mesh_attr_finalize")
    return normals, albedo, record


def mesh_vertex_record(pos, normals, rgb):
    """The interleaved record (V, 27) uint8 of positions, normals and colours (V, 3) each."""
    V = pos.shape[0]
    if normals.shape != pos.shape or rgb.shape != pos.shape:
        raise ValueError(f"mesh_vertex_record: positions {tuple(pos.shape)}, normals {tuple(normals.shape)}, colours "
                         f"{tuple(rgb.shape)}")
    record = _bytes(pos, V * _l.MESH_RECORD_BYTES).view(V, _l.MESH_RECORD_BYTES)
    _l.check(_l.load().oi_mesh_vertex_record(_p(_c(pos)), _p(_c(normals)), _p(_c(rgb)), V, _p(record), _stream()),
             "oi_mesh_vertex_record")
    return record


# ------------------------------------------------------------------------------------------
# textured mesh export (include/oi_mesh_tex.h); oi_amd.mesh.bake_textures sequences these around the vertex pass's chain
# ------------------------------------------------------------------------------------------

def tex_layout(F, T):
    """The atlas of F triangles at texel size T -> (W, H, cols): oi_tex_layout, a host-only query (no device is touched).
    ValueError for a texel size outside its range or an atlas above lib.TEX_MAX_SIZE."""
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or not _l.TEX_MIN_TEXEL <= int(T) <= _l.TEX_MAX_TEXEL:
        raise ValueError(f"texel={T!r} (an integer, {_l.TEX_MIN_TEXEL} <= texel <= {_l.TEX_MAX_TEXEL})")
    W, H, cols = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    L = _l.load()
    if L.oi_tex_layout(int(F), int(T), ctypes.byref(W), ctypes.byref(H), ctypes.byref(cols)) != 0:
        raise ValueError(L.oi_last_error().decode())
    return W.value, H.value, cols.value


def _tris(triangles):
    if triangles.dtype != torch.int32 or not triangles.is_cuda or not triangles.is_contiguous():
        raise _l.OiHipError("expected a contiguous int32 CUDA tensor of triangles (there is no CPU path)")
    return _vp(triangles.data_ptr())


def tex_uv(F, T, ref):
    """Texture coordinates (F, 3, 2) of every corner of the atlas of F triangles at texel size T (on ref's device)."""
    uv = _new(ref, F, 3, 2)
    _l.check(_l.load().oi_tex_uv(F, int(T), _p(uv), _stream()), "oi_tex_uv")
    return uv


def tex_points(pos, triangles, f0, nf, T, out=None, flags=None):
    """The planar texel points (nf * n_T, 3) of triangles f0 .. f0 + nf - 1 and their cleared flags (nf * n_T,) uint8; `out`
    and `flags`: caller-provided buffers of at least that many rows, whose leading rows are written and returned."""
    n = nf * (T * (T + 1) // 2)
    out = _new(pos, n, 3) if out is None else out[:n]
    flags = _bytes(pos, n) if flags is None else flags[:n]
    _l.check(_l.load().oi_tex_points(_p(pos), _tris(triangles), f0, nf, int(T), _p(out), _p(flags), _stream()), "oi_tex_points")
    return out, flags


def tex_store(normals, rgb, f0, nf, T, F, albedo_f32=None, normal_f32=None, albedo_u8=None, normal_u8=None):
    """Scatter the normals and colours (nf * n_T, 3) of a chunk into the atlases given (H, W, 3), float32 or uint8."""
    _l.check(_l.load().oi_tex_store(_p(normals), _p(rgb), f0, nf, int(T), F, _p(albedo_f32), _p(normal_f32), _p(albedo_u8),
                                    _p(normal_u8), _stream()), "oi_tex_store")


# ------------------------------------------------------------------------------------------
# sphere-traced surface rendering (include/oi_trace.h); oi_amd.trace sequences these around sdf_mlp_fwd
# ------------------------------------------------------------------------------------------

def _ip(t):
    """Raw pointer of a contiguous device tensor of any dtype (int32 lists, uint8 states)."""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise _l.OiHipError("oi_amd ops need contiguous CUDA/HIP tensors (there is no CPU path)")
    return _vp(t.data_ptr())


def _ray_state(st, S, lead, N, ref, rays_o, rays_d, near, far):
    """The arrays of an oi_trace_state of N rays under the leading shape `lead` (() for TraceState, (E,) for
    TraceBatchState) as attributes of `st`, and their pointers in the struct S.  t is an output (ops._new); status (uint8)
    and steps (int16: the header's uint16, at most 1024) are outputs too; the rest is working memory.  rays_o, rays_d, near,
    far: the caller's, or None to allocate them (ref: any tensor on the device)."""
    e = lambda *sh, dt=torch.float32: torch.empty(lead + sh, dtype=dt, device=ref.device)
    own = lambda x, *sh: _c(x).reshape(lead + sh) if x is not None else e(*sh)
    st.N = int(N)
    st.rays_o, st.rays_d, st.near, st.far = own(rays_o, N, 3), own(rays_d, N, 3), own(near, N), own(far, N)
    st.t = _new(ref, *lead, N)
    st.status, st.steps = e(N, dt=torch.uint8), e(N, dt=torch.int16)
    st.bracket, st.side = e(N, 4), e(N, dt=torch.uint8)
    st.active, st.points = e(2, N, dt=torch.int32), e(N, 3)
    st.counts = e(_l.TRACE_COUNT_WORDS, dt=torch.int32)
    S.N = st.N
    S.rays_o, S.rays_d, S.near_, S.far_ = _p(st.rays_o), _p(st.rays_d), _p(st.near), _p(st.far)
    S.t, S.status, S.steps, S.bracket, S.side = _p(st.t), _p(st.status), _ip(st.steps), _p(st.bracket), _p(st.side)
    S.active, S.points, S.counts = _ip(st.active), _p(st.points), _ip(st.counts)


class TraceState:
    """The arrays of one oi_trace_state for N rays (_ray_state).  rays_o / rays_d (N, 3), near / far (N,): the caller's for a
    primary trace, allocated here for a shadow trace (ref: any tensor on the device)."""

    def __init__(self, N, rays_o=None, rays_d=None, near=None, far=None, ref=None):
        self.c = _l.TraceState()
        _ray_state(self, self.c, (), N, rays_o if rays_o is not None else ref, rays_o, rays_d, near, far)


def trace_begin(st):
    _l.check(_l.load().oi_trace_begin(ctypes.byref(st.c), _stream()), "oi_trace_begin")


def trace_step(st, sdf, bound, k, tol, omega):
    _l.check(_l.load().oi_trace_step(ctypes.byref(st.c), _p(sdf), int(bound), int(k), float(tol), float(omega), _stream()),
             "oi_trace_step")


def trace_finish(st):
    """-> hit_index (N,) int32 (its first n_hit entries are written), hit_points (N, 3), hit_slot (N,) int32."""
    dev = st.t.device
    hit_index = torch.empty(st.N, dtype=torch.int32, device=dev)
    hit_points = torch.empty(st.N, 3, dtype=torch.float32, device=dev)
    hit_slot = torch.empty(st.N, dtype=torch.int32, device=dev)
    _l.check(_l.load().oi_trace_finish(ctypes.byref(st.c), _ip(hit_index), _p(hit_points), _ip(hit_slot), _stream()),
             "oi_trace_finish")
    return hit_index, hit_points, hit_slot


def trace_shadow_begin(st, hit_points, grad, n_hit, lights, w2b, bias):
    _l.check(_l.load().oi_trace_shadow_begin(ctypes.byref(st.c), _p(hit_points), _p(grad), int(n_hit), _p(lights),
                                             lights.shape[0], _p(w2b), float(bias), _stream()), "oi_trace_shadow_begin")


def trace_visibility(shadow_status, hit_slot, N, n_hit, L):
    """-> visibility (L, N) float32."""
    vis = _new(hit_slot, L, N)
    _l.check(_l.load().oi_trace_visibility(_p(shadow_status), _ip(hit_slot), int(N), int(n_hit), int(L), _p(vis), _stream()),
             "oi_trace_visibility")
    return vis


SURFACE_OUT = {"depth": (1,), "position": (3,), "normal": (3,), "normal_world": (3,), "albedo": (3,), "mask": (1,)}


def _surface_shade(what, P, rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_hit, w2b, lights, bg, visibility,
                   outputs, image_out, floats=_l.RELIGHT_LIGHT_FLOATS):
    """The arguments surface_shade, surface_shade_ao and surface_shade_local share, filled into the struct P.  -> (outputs,
    tensors to keep)."""
    N = t.shape[0]
    res = _shade_planes(what, SURFACE_OUT, P, N, t, outputs, lights, visibility, image_out, floats)
    P.N, P.n_hit = N, int(n_hit)
    keep = [_c(x) for x in (rays_o, rays_d, t, hit_points, grad, rgb, w2b, lights, bg, visibility)]
    (P.rays_o, P.rays_d, P.t, P.hit_points, P.grad, P.rgb, P.w2b, P.lights, P.bg, P.visibility) = (_p(x) for x in keep)
    P.status, P.hit_slot = _p(status), _ip(hit_slot)
    return res, keep


def _shade_planes(what, table, P, M, ref, outputs, lights, visibility, image_out, floats=_l.RELIGHT_LIGHT_FLOATS):
    """What the shade entries share, for M pixels and the output table `table` (SURFACE_OUT or SCENE_OUT): the checks of
    `outputs`, the lights, the visibility's shape and `image_out`, and the output planes, whose pointers and L go into the
    struct P.  -> {name: plane} of (M,) or (M, 3) for the names of `table` in `outputs` ("instance": int32) and "image"
    (L, 3, M) (`image_out` when given).  floats: the floats of one light record (LOCAL_LIGHT_FLOATS for local lights)."""
    for name in outputs:
        if name not in table and name != "image":
            raise ValueError(f"{what}: unknown output {name!r} (one of {tuple(table) + ('image',)})")
    nl = 0 if lights is None else lights.shape[0]
    if "image" in outputs and (nl < 1 or nl > _l.RELIGHT_MAX_LIGHTS or tuple(lights.shape[1:]) != (floats,)):
        raise ValueError(f"{what}: lights {None if lights is None else tuple(lights.shape)}, expected (L, "
                         f"{floats}) with 1 <= L <= {_l.RELIGHT_MAX_LIGHTS}")
    if visibility is not None and tuple(visibility.shape) != (nl, M):
        raise ValueError(f"{what}: visibility {tuple(visibility.shape)}, expected {(nl, M)}")
    P.L, res = nl, {}
    for name, sh in table.items():
        if name in outputs:
            res[name] = _new(ref, M) if sh == (1,) else _new(ref, M, 3)
            if name == "instance":
                res[name] = res[name].view(torch.int32)
        setattr(P, name, _ip(res.get(name)))
    if "image" in outputs:
        if image_out is None:
            image_out = _new(ref, nl, 3, M)
        elif tuple(image_out.shape) != (nl, 3, M) or not image_out.is_contiguous() or image_out.dtype != torch.float32:
            raise ValueError(f"{what}: image_out must be a contiguous float32 {(nl, 3, M)} tensor")
        res["image"] = image_out
    P.image = _p(res.get("image"))
    return res


def surface_shade(rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_hit, w2b, lights=None, bg=None,
                  visibility=None, outputs=tuple(SURFACE_OUT) + ("image",), image_out=None):
    """The G-buffer and the Phong image of a traced view (oi_surface_shade).  -> {name: (N,) or (N, 3)} for the names of
    SURFACE_OUT in `outputs`, and "image" (L, 3, N) (written into `image_out` when given)."""
    P = _l.SurfaceParams()
    res, _keep = _surface_shade("surface_shade", P, rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_hit, w2b, lights,
                                bg, visibility, outputs, image_out)
    _l.check(_l.load().oi_surface_shade(ctypes.byref(P), _stream()), "oi_surface_shade")
    return res


# ------------------------------------------------------------------------------------------
# batched sphere tracing (include/oi_trace_batch.h); oi_amd.trace.sphere_trace_batch sequences these
# ------------------------------------------------------------------------------------------

def sdf_mlp_fwd_segments(pts, packed, gamma, beta, sdf, B, n_per_elem, prec, fast_trig=False):
    """The sdf-only pass on the first n_per_elem points of each of B segments: pts (B, stride, 3) -> sdf (B, stride), the
    caller's, of which [:, :n_per_elem] is written and the rest left as it is."""
    if pts.dim() != 3 or pts.shape[0] != B or pts.shape[2] != 3 or tuple(sdf.shape) != tuple(pts.shape[:2]):
        raise ValueError(f"sdf_mlp_fwd_segments: pts {tuple(pts.shape)}, sdf {tuple(sdf.shape)}, expected ({B}, stride, 3) and ({B}, stride)")
    _l.check(_l.load().oi_sdf_mlp_fwd_segments(_p(pts), _p(packed), _p(gamma), _p(beta), _p(sdf), int(B), int(n_per_elem),
                                               pts.shape[1], prec, int(bool(fast_trig)), _stream()), "oi_sdf_mlp_fwd_segments")
    return sdf


class TraceBatchState:
    """The arrays of one oi_trace_batch: E elements of N rays each, every array of TraceState with a leading element
    dimension (_ray_state), so counts (E, TRACE_COUNT_WORDS), and live (TRACE_COUNT_WORDS,) int32.  rays_o / rays_d (E, N, 3),
    near / far (E, N) are the caller's."""

    def __init__(self, E, N, rays_o, rays_d, near, far):
        self.E, self.c = int(E), _l.TraceBatch()
        _ray_state(self, self.c.s, (self.E,), N, rays_o, rays_o, rays_d, near, far)
        self.live = torch.empty(_l.TRACE_COUNT_WORDS, dtype=torch.int32, device=rays_o.device)
        self.c.E, self.c.live = self.E, _ip(self.live)


def trace_batch_begin(st):
    _l.check(_l.load().oi_trace_batch_begin(ctypes.byref(st.c), _stream()), "oi_trace_batch_begin")


def trace_batch_step(st, sdf, bound, k, tol, omega):
    _l.check(_l.load().oi_trace_batch_step(ctypes.byref(st.c), _p(sdf), int(bound), int(k), float(tol), float(omega), _stream()),
             "oi_trace_batch_step")


def trace_batch_finish(st):
    """-> hit_index (E, N) int32 (the first n_hit_e entries of row e are written), hit_slot (E, N) int32."""
    dev = st.t.device
    hit_index = torch.empty(st.E, st.N, dtype=torch.int32, device=dev)
    hit_slot = torch.empty(st.E, st.N, dtype=torch.int32, device=dev)
    _l.check(_l.load().oi_trace_batch_finish(ctypes.byref(st.c), _ip(hit_index), _ip(hit_slot), _stream()), "oi_trace_batch_finish")
    return hit_index, hit_slot


def trace_batch_gather(st, hit_index, n_pad):
    """-> hit_points_padded (E, n_pad, 3): row e holds its n_hit_e hit points, then the coordinate origin."""
    out = _new(st.t, st.E, int(n_pad), 3)
    if n_pad:
        _l.check(_l.load().oi_trace_batch_gather(ctypes.byref(st.c), _ip(hit_index), int(n_pad), _p(out), _stream()),
                 "oi_trace_batch_gather")
    return out


# ------------------------------------------------------------------------------------------
# many instances in one scene image (include/oi_scene.h); oi_amd.scene sequences these around the batched march
# ------------------------------------------------------------------------------------------

def trace_batch_state_empty(E, N, ref):
    """A TraceBatchState whose rays, near and far the begin kernel writes (oi_scene_begin, oi_scene_shadow_begin)."""
    return TraceBatchState(E, N, _new(ref, E, N, 3), _new(ref, E, N, 3), _new(ref, E, N), _new(ref, E, N))


def scene_begin(st, c2b, kinv, window, W, S):
    """st: TraceBatchState of E elements x W * W rays; c2b (E, 4, 4), kinv (3, 3), window (E, 2) int32."""
    _l.check(_l.load().oi_scene_begin(ctypes.byref(st.c), _p(c2b), _p(kinv), _ip(window), int(W), int(S), _stream()),
             "oi_scene_begin")


def scene_resolve(st, window, W, S):
    """-> owner, owner_ray (S * S,) int32."""
    # (int32 outputs through _new, the same width: the tests' guarded arenas see them)
    owner, owner_ray = _new(st.t, S * S).view(torch.int32), _new(st.t, S * S).view(torch.int32)
    _l.check(_l.load().oi_scene_resolve(ctypes.byref(st.c), _ip(window), int(W), int(S), _ip(owner), _ip(owner_ray), _stream()),
             "oi_scene_resolve")
    return owner, owner_ray


def scene_visible(st, owner, window, W, S):
    """-> vis_index (E, N) int32 (the first n_vis_e entries of row e are written), vis_slot (E, N) int32.  Overwrites the hit
    words of st.counts and st.live with the visible counts."""
    vis_index = torch.empty(st.E, st.N, dtype=torch.int32, device=st.t.device)
    vis_slot = _new(st.t, st.E, st.N).view(torch.int32)
    _l.check(_l.load().oi_scene_visible(ctypes.byref(st.c), _ip(owner), _ip(window), int(W), int(S), _ip(vis_index), _ip(vis_slot),
                                        _stream()), "oi_scene_visible")
    return vis_index, vis_slot


SCENE_OUT = {"depth": (1,), "position": (3,), "normal": (3,), "normal_world": (3,), "albedo": (3,), "mask": (1,), "instance": (1,)}


def scene_shade(st, W, S, owner, owner_ray, vis_slot, hit_points, grad, rgb, n_pad, w2b, b2w, lights=None, bg=None,
                visibility=None, outputs=tuple(SCENE_OUT) + ("image",), image_out=None):
    """The G-buffer and the Phong image of a scene (oi_scene_shade).  hit_points, grad, rgb (E, n_pad, 3) (None with n_pad ==
    0).  -> {name: (S * S,) or (S * S, 3)} for the names of SCENE_OUT in `outputs` ("instance": int32), and "image" (L, 3,
    S * S) (written into `image_out` when given)."""
    P = _l.SceneShadeParams()
    res, _keep = _scene_shade("scene_shade", P, st, W, S, owner, owner_ray, vis_slot, hit_points, grad, rgb, n_pad, w2b, b2w, lights,
                              bg, visibility, outputs, image_out)
    _l.check(_l.load().oi_scene_shade(ctypes.byref(P), _stream()), "oi_scene_shade")
    return res


def _scene_shade(what, P, st, W, S, owner, owner_ray, vis_slot, hit_points, grad, rgb, n_pad, w2b, b2w, lights, bg, visibility,
                 outputs, image_out, floats=_l.RELIGHT_LIGHT_FLOATS):
    """The arguments scene_shade, scene_shade_ao and scene_shade_local share, filled into the struct P.  -> (outputs, tensors to
    keep)."""
    res = _shade_planes(what, SCENE_OUT, P, S * S, st.t, outputs, lights, visibility, image_out, floats)
    P.E, P.W, P.S, P.n_pad = st.E, int(W), int(S), int(n_pad)
    keep = [_c(x) for x in (hit_points, grad, rgb, w2b, b2w, lights, bg, visibility)]
    P.hit_points, P.grad, P.rgb, P.w2b, P.b2w, P.lights, P.bg, P.visibility = (_p(x) for x in keep)
    P.rays_o, P.rays_d, P.t = _p(st.rays_o), _p(st.rays_d), _p(st.t)
    P.owner, P.owner_ray, P.vis_slot = _ip(owner), _ip(owner_ray), _ip(vis_slot)
    return res, keep


def scene_points(st, hit_points, grad, n_pad, offset, n_vis, b2w, w2b):
    """-> position, normal (n_vis, 3) in the world frame, elem (n_vis,) int32: the visible points of all elements, point
    offset[e] + slot."""
    pos, nrm, elem = _new(st.t, n_vis, 3), _new(st.t, n_vis, 3), _new(st.t, n_vis).view(torch.int32)
    _l.check(_l.load().oi_scene_points(ctypes.byref(st.c), _p(hit_points), _p(grad), int(n_pad), _ip(offset), int(n_vis), _p(_c(b2w)),
                                       _p(_c(w2b)), _p(pos), _p(nrm), _ip(elem), _stream()), "oi_scene_points")
    return pos, nrm, elem


def scene_shadow_begin(sb, hit_points, grad, n_pad, offset, elem, position, normal, n_vis, lights, w2b, bias):
    """sb: TraceBatchState of E occluder elements x L * n_vis rays (trace_batch_state_empty)."""
    _l.check(_l.load().oi_scene_shadow_begin(ctypes.byref(sb.c), _p(hit_points), _p(grad), int(n_pad), _ip(offset), _ip(elem),
                                             _p(position), _p(normal), int(n_vis), _p(lights), lights.shape[0], _p(_c(w2b)),
                                             float(bias), _stream()), "oi_scene_shadow_begin")


def scene_visibility(shadow_status, owner, owner_ray, vis_slot, offset, E, N, L, n_vis, S):
    """-> visibility (L, S * S) float32."""
    vis = _new(owner, L, S * S)
    _l.check(_l.load().oi_scene_visibility(_p(shadow_status), _ip(owner), _ip(owner_ray), _ip(vis_slot), _ip(offset), int(E), int(N),
                                           int(L), int(n_vis), int(S), _p(vis), _stream()), "oi_scene_visibility")
    return vis


# ------------------------------------------------------------------------------------------
# sampled secondary rays between the instances of a scene (include/oi_scene_light.h); oi_amd.scene sequences these
# ------------------------------------------------------------------------------------------

def scene_point_pixels(st, vis_index, window, W, S, offset, n_vis):
    """-> pixel (n_vis,) int32: the scene pixel Y * S + X of visible point offset[e] + slot."""
    pixel = _new(st.t, n_vis).view(torch.int32)
    _l.check(_l.load().oi_scene_point_pixels(ctypes.byref(st.c), _ip(vis_index), _ip(window), int(W), int(S), _ip(offset), int(n_vis),
                                             _ip(pixel), _stream()), "oi_scene_point_pixels")
    return pixel


def scene_occlusion_begin(sb, hit_points, grad, n_pad, offset, elem, pixel, position, normal, n_vis, w2b, bias, samples, j0, chunk,
                          seed=0, lights=None, radius=None, distance=None):
    """sb: TraceBatchState of E occluder elements x L * chunk * n_vis rays (trace_batch_state_empty): the samples [j0, j0 +
    chunk) of `samples` strata.  lights (L, 16) and radius (L,) float32: caps about the lights; distance (a float, inf
    allowed) instead: the hemisphere about the normal."""
    ambient = lights is None
    if ambient == (distance is None) or (not ambient and radius is None):
        raise ValueError("scene_occlusion_begin: give lights and radius, or distance (the ambient form)")
    if not ambient and (not torch.is_tensor(radius) or radius.dtype != torch.float32 or tuple(radius.shape) != (lights.shape[0],)):
        raise ValueError(f"scene_occlusion_begin: radius must be a float32 tensor of shape ({lights.shape[0]},), one per light")
    P = _l.SceneOcclusionParams()
    P.L, P.S, P.j0, P.Sc, P.ambient = 1 if ambient else lights.shape[0], int(samples), int(j0), int(chunk), int(ambient)
    P.seed, P.bias, P.distance, P.n_pad, P.n_vis = int(seed), float(bias), float(distance) if ambient else 0.0, int(n_pad), int(n_vis)
    keep = [_c(x) for x in (hit_points, grad, position, normal, lights, radius, w2b)]
    P.hit_points, P.grad, P.position, P.normal, P.lights, P.radius, P.w2b = (_p(x) for x in keep)
    P.offset, P.elem, P.pixel = _ip(offset), _ip(elem), _ip(pixel)
    _l.check(_l.load().oi_scene_occlusion_begin(ctypes.byref(sb.c), ctypes.byref(P), _stream()), "oi_scene_occlusion_begin")


def trace_batch_step_anyhit(st, sdf, bound, k, tol, omega):
    _l.check(_l.load().oi_trace_batch_step_anyhit(ctypes.byref(st.c), _p(sdf), int(bound), int(k), float(tol), float(omega),
                                                  _stream()), "oi_trace_batch_step_anyhit")


def scene_occlusion_resolve(status, owner, owner_ray, vis_slot, offset, E, N, L, samples, j0, chunk, n_vis, S, count, out, last):
    """Adds the chunk's escaped samples to count (L, S * S) int32 (overwritten at j0 == 0); last: out (L, S * S) = count /
    samples on the mask, 1 off it."""
    _l.check(_l.load().oi_scene_occlusion_resolve(_p(status), _ip(owner), _ip(owner_ray), _ip(vis_slot), _ip(offset), int(E), int(N),
                                                  int(L), int(samples), int(j0), int(chunk), int(n_vis), int(S), int(bool(last)),
                                                  _ip(count), _p(out), _stream()), "oi_scene_occlusion_resolve")


def scene_transfer_resolve(status, rays_d, owner, owner_ray, vis_slot, offset, w2b, E, N, samples, j0, chunk, n_vis, S, transfer,
                           last):
    """Adds the chunk's escaped samples' SH basis (world frame) to transfer (9, S * S) (overwritten at j0 == 0); last:
    divided by samples."""
    _l.check(_l.load().oi_scene_transfer_resolve(_p(status), _p(rays_d), _ip(owner), _ip(owner_ray), _ip(vis_slot), _ip(offset),
                                                 _p(_c(w2b)), int(E), int(N), int(samples), int(j0), int(chunk), int(n_vis), int(S),
                                                 int(bool(last)), _p(transfer), _stream()), "oi_scene_transfer_resolve")


def scene_transfer_normal(grad, n_pad, owner, owner_ray, vis_slot, w2b, E, N, S):
    """-> the unshadowed transfer map (9, S * S): A_band y_c(world normal) on the mask, zeros off it."""
    out = _new(grad, _l.ENV_COEFFS, S * S)
    _l.check(_l.load().oi_scene_transfer_normal(_p(grad), int(n_pad), _ip(owner), _ip(owner_ray), _ip(vis_slot), _p(_c(w2b)), int(E),
                                                int(N), int(S), _p(out), _stream()), "oi_scene_transfer_normal")
    return out


def scene_shade_ao(st, W, S, owner, owner_ray, vis_slot, hit_points, grad, rgb, n_pad, w2b, b2w, lights=None, bg=None,
                   visibility=None, ambient_occlusion=None, outputs=tuple(SCENE_OUT) + ("image",), image_out=None):
    """scene_shade with an occlusion factor (S * S,) in [0, 1] on the ambient term (oi_scene_shade_ao); None: scene_shade's
    bytes."""
    if ambient_occlusion is not None and tuple(ambient_occlusion.shape) != (S * S,):
        raise ValueError(f"scene_shade_ao: ambient_occlusion {tuple(ambient_occlusion.shape)}, expected {(S * S,)}")
    A = _l.SceneShadeAoParams()
    res, _keep = _scene_shade("scene_shade_ao", A.s, st, W, S, owner, owner_ray, vis_slot, hit_points, grad, rgb, n_pad, w2b, b2w,
                              lights, bg, visibility, outputs, image_out)
    ao = _c(ambient_occlusion)
    A.ambient_occlusion = _p(ao)
    _l.check(_l.load().oi_scene_shade_ao(ctypes.byref(A), _stream()), "oi_scene_shade_ao")
    return res


# ------------------------------------------------------------------------------------------
# soft shadows and ambient occlusion on the traced surface (include/oi_occlusion.h)
# ------------------------------------------------------------------------------------------

def occlusion_light_begin(st, hit_points, grad, hit_index, n_hit, lights, radius, samples, w2b, bias, seed=0):
    """S = samples rays per (light, hit) into the TraceState st of L * S * n_hit rays; radius (L,) float32 on the device."""
    if not torch.is_tensor(radius) or radius.dtype != torch.float32 or tuple(radius.shape) != (lights.shape[0],):
        raise ValueError(f"occlusion_light_begin: radius must be a float32 tensor of shape ({lights.shape[0]},), one per light")
    _l.check(_l.load().oi_occlusion_light_begin(ctypes.byref(st.c), _p(hit_points), _p(grad), _ip(hit_index), int(n_hit), _p(lights),
                                                _p(radius), lights.shape[0], int(samples), _p(w2b), float(bias), int(seed),
                                                _stream()), "oi_occlusion_light_begin")


def occlusion_ambient_begin(st, hit_points, grad, hit_index, n_hit, samples, bias, distance, seed=0):
    """S = samples hemisphere rays per hit into the TraceState st of S * n_hit rays."""
    _l.check(_l.load().oi_occlusion_ambient_begin(ctypes.byref(st.c), _p(hit_points), _p(grad), _ip(hit_index), int(n_hit),
                                                  int(samples), float(bias), float(distance), int(seed), _stream()),
             "oi_occlusion_ambient_begin")


def occlusion_step(st, sdf, bound, k, tol, omega):
    _l.check(_l.load().oi_occlusion_step(ctypes.byref(st.c), _p(sdf), int(bound), int(k), float(tol), float(omega), _stream()),
             "oi_occlusion_step")


def occlusion_resolve(status, hit_slot, N, n_hit, L, samples):
    """-> (L, N) float32: the share of each pixel's `samples` rays per light that ended TRACE_MISS (1 off the mask)."""
    out = _new(hit_slot, L, N)
    _l.check(_l.load().oi_occlusion_resolve(_p(status), _ip(hit_slot), int(N), int(n_hit), int(L), int(samples), _p(out),
                                            _stream()), "oi_occlusion_resolve")
    return out


def surface_shade_ao(rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_hit, w2b, lights=None, bg=None,
                     visibility=None, ambient_occlusion=None, outputs=tuple(SURFACE_OUT) + ("image",), image_out=None):
    """surface_shade with an occlusion factor (N,) in [0, 1] on the ambient term (oi_surface_shade_ao)."""
    if ambient_occlusion is not None and tuple(ambient_occlusion.shape) != (t.shape[0],):
        raise ValueError(f"surface_shade_ao: ambient_occlusion {tuple(ambient_occlusion.shape)}, expected {(t.shape[0],)}")
    P = _l.SurfaceAoParams()
    res, _keep = _surface_shade("surface_shade_ao", P, rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_hit, w2b,
                                lights, bg, visibility, outputs, image_out)
    ao = _c(ambient_occlusion)
    P.ambient_occlusion = _p(ao)
    _l.check(_l.load().oi_surface_shade_ao(ctypes.byref(P), _stream()), "oi_surface_shade_ao")
    return res


# ------------------------------------------------------------------------------------------
# local lights: point, spot and sphere lights in the world (include/oi_local_light.h); oi_amd.trace and oi_amd.scene sequence these
# ------------------------------------------------------------------------------------------

def _check_local(what, lights):
    if not torch.is_tensor(lights) or lights.dtype != torch.float32 or lights.dim() != 2 or lights.shape[1] != _l.LOCAL_LIGHT_FLOATS:
        raise ValueError(f"{what}: lights must be a float32 tensor of shape (L, {_l.LOCAL_LIGHT_FLOATS}) (oi_amd.relight."
                         "stack_local_lights)")


def local_light_begin(st, hit_points, grad, hit_index, n_hit, lights, samples, w2b, bias, seed=0):
    """S = samples rays per (local light, hit), aimed at the light and ending there, into the TraceState st of L * S * n_hit
    rays; lights (L, 20) float32 on the device."""
    _check_local("local_light_begin", lights)
    _l.check(_l.load().oi_local_light_begin(ctypes.byref(st.c), _p(hit_points), _p(grad), _ip(hit_index), int(n_hit), _p(lights),
                                            lights.shape[0], int(samples), _p(w2b), float(bias), int(seed), _stream()),
             "oi_local_light_begin")


def surface_shade_local(rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_hit, w2b, lights=None, bg=None,
                        visibility=None, ambient_occlusion=None, outputs=tuple(SURFACE_OUT) + ("image",), image_out=None):
    """surface_shade_ao under local lights (L, 20) (oi_surface_shade_local): the G-buffer is surface_shade's."""
    if ambient_occlusion is not None and tuple(ambient_occlusion.shape) != (t.shape[0],):
        raise ValueError(f"surface_shade_local: ambient_occlusion {tuple(ambient_occlusion.shape)}, expected {(t.shape[0],)}")
    P = _l.SurfaceAoParams()
    res, _keep = _surface_shade("surface_shade_local", P, rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_hit, w2b,
                                lights, bg, visibility, outputs, image_out, _l.LOCAL_LIGHT_FLOATS)
    ao = _c(ambient_occlusion)
    P.ambient_occlusion = _p(ao)
    _l.check(_l.load().oi_surface_shade_local(ctypes.byref(P), _stream()), "oi_surface_shade_local")
    return res


# ------------------------------------------------------------------------------------------
# the mesh rasteriser (include/oi_raster.h); oi_amd.raster.render_mesh sequences these in front of the shade above
# ------------------------------------------------------------------------------------------

def _ints(ref, *shape):
    """int32 output through _new, the same width: the tests' guarded arenas see it."""
    return _new(ref, *shape).view(torch.int32)


def _raster_views(what, cams, R):
    """cams: (c2b or b2c (E, 4, 4), kinv or K (3, 3), offs (E, 2) or None), float32 on the device.  -> E and the pointers."""
    m, k, offs = cams
    E = m.shape[0]
    if tuple(m.shape) != (E, 4, 4) or tuple(k.shape) != (3, 3) or (offs is not None and tuple(offs.shape) != (E, 2)):
        raise ValueError(f"{what}: camera matrices {tuple(m.shape)}, intrinsics {tuple(k.shape)}, offsets "
                         f"{None if offs is None else tuple(offs.shape)}, expected (E, 4, 4), (3, 3) and (E, 2)")
    return E, (_p(m), _p(k), _p(offs), int(R), E)


def raster_setup(b2c, K, offs, R, pos, triangles, near, small_max):
    """The setup stage for E views of R x R pixels (oi_raster_setup).  b2c (E, 4, 4), K (3, 3), offs (E, 2) or None; pos (V, 3)
    float32, triangles (F, 3) int32.  -> dict of corners (E, F, 3, 2), bbox (E, F, 4) int32, cls (E, F) uint8, small_list,
    large_list (E, F) int32 (their first counts[e] entries are written), counts (E, 2) int32.  F == 0 launches nothing."""
    E, views = _raster_views("raster_setup", (b2c, K, offs), R)
    V, F = pos.shape[0], triangles.shape[0]
    out = {"corners": _ints(pos, E, F, 3, 2), "bbox": _ints(pos, E, F, 4),
           "cls": torch.empty(E, F, dtype=torch.uint8, device=pos.device),
           "small_list": torch.empty(E, F, dtype=torch.int32, device=pos.device),
           "large_list": torch.empty(E, F, dtype=torch.int32, device=pos.device),
           "counts": torch.zeros(E, 2, dtype=torch.int32, device=pos.device)}
    _l.check(_l.load().oi_raster_setup(*views, _p(pos), _tris(triangles), V, F, float(near), int(small_max), _ip(out["corners"]),
                                       _ip(out["bbox"]), _ip(out["cls"]), _ip(out["small_list"]), _ip(out["large_list"]),
                                       _ip(out["counts"]), _stream()), "oi_raster_setup")
    return out


def raster_fill(c2b, kinv, offs, R, pos, triangles, setup):
    """The visible triangle per pixel (oi_raster_fill) from raster_setup's dict.  -> zbuf (E, R * R) int64: the keys
    (float_as_uint(t) << 32) | f as signed words, -1 where no triangle covers the centre."""
    E, views = _raster_views("raster_fill", (c2b, kinv, offs), R)
    zbuf = _new(pos, E, R * R, 2).view(torch.int64).view(E, R * R)
    zbuf.fill_(-1)
    _l.check(_l.load().oi_raster_fill(*views, _p(pos), _tris(triangles), pos.shape[0], triangles.shape[0], _ip(setup["corners"]),
                                      _ip(setup["bbox"]), _ip(setup["small_list"]), _ip(setup["large_list"]), _ip(setup["counts"]),
                                      _ip(zbuf), _stream()), "oi_raster_fill")
    return zbuf


RASTER_OUT = {"rays_o": (3,), "rays_d": (3,), "t": (), "status": (), "hit_slot": (), "hit_points": (3,), "grad": (3,),
              "rgb": (3,), "triangle": (), "barycentric": (3,)}


def raster_resolve(c2b, kinv, offs, R, pos, triangles, zbuf, vertex=None, texture=None, outputs=tuple(RASTER_OUT)):
    """The ray state and the G-buffer of E rasterised views (oi_raster_resolve).  vertex: (normals, albedo) (V, 3) float32;
    texture: (uv (F, 3, 2), albedo atlas, normal atlas), the atlases (H, W, 3) uint8 or float32; exactly one of the two.
    -> {name: (E, N) or (E, N, 3)} for the names of RASTER_OUT in `outputs` (status uint8; hit_slot, triangle int32)."""
    what = "raster_resolve"
    E, views = _raster_views(what, (c2b, kinv, offs), R)
    V, F, N = pos.shape[0], triangles.shape[0], R * R
    if (vertex is None) == (texture is None):
        raise ValueError(f"{what}: give exactly one of vertex=(normals, albedo) and texture=(uv, albedo atlas, normal atlas)")
    for name in outputs:
        if name not in RASTER_OUT:
            raise ValueError(f"{what}: unknown output {name!r} (one of {tuple(RASTER_OUT)})")
    if tuple(zbuf.shape) != (E, N) or zbuf.dtype != torch.int64:
        raise ValueError(f"{what}: zbuf {tuple(zbuf.shape)} {zbuf.dtype}, expected {(E, N)} int64")
    src = [None] * 9   # vnormal, valbedo, uv, W, H, albedo_u8, albedo_f32, normal_u8, normal_f32
    src[3] = src[4] = 0
    if vertex is not None:
        vn, va = vertex
        if tuple(vn.shape) != (V, 3) or tuple(va.shape) != (V, 3):
            raise ValueError(f"{what}: vertex normals {tuple(vn.shape)}, albedo {tuple(va.shape)}, expected {(V, 3)}")
        src[0], src[1], mode = _p(vn), _p(va), _l.RASTER_VERTEX
    else:
        uv, am, nm = texture
        if tuple(uv.shape) != (F, 3, 2) or am.dim() != 3 or am.shape[2] != 3 or am.shape != nm.shape:
            raise ValueError(f"{what}: uv {tuple(uv.shape)}, atlases {tuple(am.shape)} and {tuple(nm.shape)}, expected "
                             f"{(F, 3, 2)} and two (H, W, 3)")
        src[2], src[3], src[4], mode = _p(uv), am.shape[1], am.shape[0], _l.RASTER_TEXTURE
        src[5 if am.dtype == torch.uint8 else 6] = _p(am)
        src[7 if nm.dtype == torch.uint8 else 8] = _p(nm)
    res = {}
    for name, sh in RASTER_OUT.items():
        if name not in outputs:
            continue
        if name == "status":
            res[name] = torch.empty(E, N, dtype=torch.uint8, device=pos.device)
        elif name in ("hit_slot", "triangle"):
            res[name] = _ints(pos, E, N)
        else:
            res[name] = _new(pos, E, N, *sh)
    _l.check(_l.load().oi_raster_resolve(*views, _p(pos), _tris(triangles), V, F, _ip(zbuf), mode, *src,
                                         *(_ip(res.get(name)) for name in RASTER_OUT), _stream()), "oi_raster_resolve")
    return res


# ------------------------------------------------------------------------------------------
# the secondary rays and the shade of E views in one chain (include/oi_occlusion_batch.h); oi_amd.trace sequences these
# ------------------------------------------------------------------------------------------

def occlusion_batch_begin(sb, mode, hit_points, grad, hit_index, counts, n_pad, samples, j0, chunk, bias, seed=0, lights=None,
                          radius=None, w2b=None, distance=None):
    """sb: TraceBatchState of E views x L * chunk * n_pad rays (trace_batch_state_empty): the samples [j0, j0 + chunk) of
    `samples` strata at every view's own hits.  mode: lib.OCCLUSION_BATCH_*.  hit_points, grad (E, n_pad, 3), hit_index (E, N)
    int32 and counts (E, TRACE_COUNT_WORDS) int32 of the primary batch; lights (L, 16) -- LOCAL: (L, 20) --, radius (L,)
    float32 for CAP, w2b (E, 4, 4); HEMISPHERE: distance instead, one set of rays."""
    what = "occlusion_batch_begin"
    ambient = mode == _l.OCCLUSION_BATCH_HEMISPHERE
    if ambient == (distance is None) or ambient != (lights is None):
        raise ValueError(f"{what}: give distance for the hemisphere, lights for every other mode")
    if mode == _l.OCCLUSION_BATCH_LOCAL:
        _check_local(what, lights)
    if mode == _l.OCCLUSION_BATCH_CAP and (not torch.is_tensor(radius) or radius.dtype != torch.float32
                                           or tuple(radius.shape) != (lights.shape[0],)):
        raise ValueError(f"{what}: radius must be a float32 tensor of shape ({lights.shape[0]},), one per light")
    if hit_index.dim() != 2 or hit_index.shape[0] != sb.E or tuple(counts.shape) != (sb.E, _l.TRACE_COUNT_WORDS):
        raise ValueError(f"{what}: hit_index {tuple(hit_index.shape)}, counts {tuple(counts.shape)} for {sb.E} views")
    if tuple(hit_points.shape) != (sb.E, int(n_pad), 3) or tuple(grad.shape) != (sb.E, int(n_pad), 3):
        raise ValueError(f"{what}: hit_points {tuple(hit_points.shape)}, grad {tuple(grad.shape)}, expected {(sb.E, int(n_pad), 3)}")
    if w2b is not None and w2b.numel() != sb.E * 16:
        raise ValueError(f"{what}: w2b {tuple(w2b.shape)}, expected ({sb.E}, 4, 4)")
    keep = [_c(x) for x in (lights, w2b)]
    _l.check(_l.load().oi_occlusion_batch_begin(ctypes.byref(sb.c), int(mode), _p(hit_points), _p(grad), _ip(hit_index), _ip(counts),
                                                hit_index.shape[1], int(n_pad), 1 if ambient else lights.shape[0], int(samples),
                                                int(j0), int(chunk), _p(keep[0]), _p(radius), _p(keep[1]), float(bias),
                                                float(distance) if ambient else 0.0, int(seed), _stream()), what)


def occlusion_batch_maps(ref, E, L, N, n_pad):
    """-> count (E, L, n_pad) int32 and out (E, L, N) float32 for occlusion_batch_resolve."""
    # (int32 through _new, the same width: the tests' guarded arenas see it)
    return _new(ref, E, L, n_pad).view(torch.int32), _new(ref, E, L, N)


def occlusion_batch_resolve(status, hit_slot, counts, n_pad, L, samples, j0, chunk, count, out, last):
    """Adds the chunk's rays that ended TRACE_MISS to count (E, L, n_pad) int32 (overwritten at j0 == 0); last: out (E, L, N) =
    count / samples on the mask, 1 off it.  status (E, L * chunk * n_pad) uint8, hit_slot (E, N) int32."""
    E, N = hit_slot.shape
    if (tuple(status.shape) != (E, L * chunk * n_pad) or tuple(count.shape) != (E, L, n_pad) or tuple(out.shape) != (E, L, N)
            or tuple(counts.shape) != (E, _l.TRACE_COUNT_WORDS)):
        raise ValueError(f"occlusion_batch_resolve: status {tuple(status.shape)}, count {tuple(count.shape)}, out {tuple(out.shape)}, "
                         f"counts {tuple(counts.shape)} for E={E}, N={N}, n_pad={n_pad}, L={L}, chunk={chunk}")
    _l.check(_l.load().oi_occlusion_batch_resolve(_p(status), _ip(hit_slot), _ip(counts), int(E), int(N), int(n_pad), int(L),
                                                  int(samples), int(j0), int(chunk), int(bool(last)), _ip(count), _p(out),
                                                  _stream()), "oi_occlusion_batch_resolve")


def surface_shade_batch(rays_o, rays_d, t, status, hit_slot, hit_points, grad, rgb, n_pad, w2b, lights=None, bg=None,
                        visibility=None, ambient_occlusion=None, outputs=tuple(SURFACE_OUT) + ("image",)):
    """surface_shade_ao -- under local lights (L, 20): surface_shade_local -- for E views in ONE launch
    (oi_surface_shade_batch).  rays_o, rays_d (E, N, 3), t, status, hit_slot (E, N); hit_points, grad, rgb (E, n_pad, 3) (None
    with n_pad == 0); w2b (E, 4, 4); visibility (E, L, N), ambient_occlusion (E, N) or None.  -> {name: (E, N) or (E, N, 3)}
    for the names of SURFACE_OUT in `outputs`, and "image" (E, L, 3, N)."""
    what = "surface_shade_batch"
    E, N = t.shape
    for name in outputs:
        if name not in SURFACE_OUT and name != "image":
            raise ValueError(f"{what}: unknown output {name!r} (one of {tuple(SURFACE_OUT) + ('image',)})")
    nl = 0 if lights is None else lights.shape[0]
    local = lights is not None and lights.shape[-1] == _l.LOCAL_LIGHT_FLOATS
    floats = _l.LOCAL_LIGHT_FLOATS if local else _l.RELIGHT_LIGHT_FLOATS
    if "image" in outputs and (nl < 1 or nl > _l.RELIGHT_MAX_LIGHTS or tuple(lights.shape[1:]) != (floats,)):
        raise ValueError(f"{what}: lights {None if lights is None else tuple(lights.shape)}, expected (L, {floats}) with "
                         f"1 <= L <= {_l.RELIGHT_MAX_LIGHTS}")
    if visibility is not None and tuple(visibility.shape) != (E, nl, N):
        raise ValueError(f"{what}: visibility {tuple(visibility.shape)}, expected {(E, nl, N)}")
    if ambient_occlusion is not None and tuple(ambient_occlusion.shape) != (E, N):
        raise ValueError(f"{what}: ambient_occlusion {tuple(ambient_occlusion.shape)}, expected {(E, N)}")
    if w2b.numel() != E * 16 or (n_pad and any(tuple(x.shape) != (E, int(n_pad), 3) for x in (hit_points, grad, rgb))):
        raise ValueError(f"{what}: w2b {tuple(w2b.shape)} or the hit arrays do not hold {E} views of n_pad={n_pad} points")
    P = _l.SurfaceAoParams()
    P.N, P.n_hit, P.L, res = N, int(n_pad), nl, {}
    for name, sh in SURFACE_OUT.items():
        if name in outputs:
            res[name] = _new(t, E, N) if sh == (1,) else _new(t, E, N, 3)
        setattr(P, name, _p(res.get(name)))
    if "image" in outputs:
        res["image"] = _new(t, E, nl, 3, N)
    P.image = _p(res.get("image"))
    keep = [_c(x) for x in (rays_o, rays_d, t, hit_points, grad, rgb, w2b, lights, bg, visibility, ambient_occlusion)]
    (P.rays_o, P.rays_d, P.t, P.hit_points, P.grad, P.rgb, P.w2b, P.lights, P.bg, P.visibility,
     P.ambient_occlusion) = (_p(x) for x in keep)
    P.status, P.hit_slot = _p(status), _ip(hit_slot)
    _l.check(_l.load().oi_surface_shade_batch(ctypes.byref(P), int(E), int(n_pad), int(local), _stream()), "oi_surface_shade_batch")
    return res


# ------------------------------------------------------------------------------------------
# adaptive anti-aliasing of the traced surface (include/oi_aa.h); oi_amd.trace sequences these
# ------------------------------------------------------------------------------------------

def aa_classify(status, hit_slot, hit_points, grad, n_hit, H, W, plane_threshold=_l.AA_DEFAULT_PLANE,
                cos_threshold=_l.AA_DEFAULT_COS):
    """The pixels of an H x W primary trace that need more samples (oi_aa_classify).  -> edge_index (N,) int32 (its first
    `count` entries are written: the flagged pixels, in no fixed order), edge_slot (N,) int32 (the pixel's position in
    edge_index, or -1), count (1,) int32 on the device."""
    N = int(H) * int(W)
    if status.shape[0] != N or hit_slot.shape[0] != N:
        raise ValueError(f"aa_classify: status {tuple(status.shape)}, hit_slot {tuple(hit_slot.shape)} for {H} x {W} pixels")
    edge_index = torch.empty(N, dtype=torch.int32, device=status.device)   # (partly written by contract, as trace_finish's hit_index)
    edge_slot = _new(status, N).view(torch.int32)
    count = _new(status, 1).view(torch.int32)
    _l.check(_l.load().oi_aa_classify(_p(status), _ip(hit_slot), _p(hit_points) if n_hit else None, _p(grad) if n_hit else None,
                                      int(n_hit), int(H), int(W), float(plane_threshold), float(cos_threshold), _ip(edge_index),
                                      _ip(edge_slot), _ip(count), _stream()), "oi_aa_classify")
    return edge_index, edge_slot, count


def aa_begin(st, c2b, kinv, offs, R, edge_index, n_edge, offsets):
    """The sub-pixel rays of the first n_edge pixels of edge_index into the TraceState st of (S - 1) * n_edge rays, started as
    trace_begin starts rays (oi_aa_begin).  c2b (16 floats), kinv (3, 3), offs (2 floats): gen_rays' at B = 1; offsets (S, 2)
    float32 on the device, in units of the pixel pitch (row 0, the centre, is not read)."""
    if offsets.dim() != 2 or offsets.shape[1] != 2 or offsets.dtype != torch.float32:
        raise ValueError(f"aa_begin: offsets {tuple(offsets.shape)} {offsets.dtype}, expected float32 (S, 2)")
    if c2b.numel() != 16 or kinv.numel() != 9 or offs.numel() != 2:
        raise ValueError("aa_begin: c2b, kinv and offs must hold 16, 9 and 2 floats (one view)")
    keep = [_c(c2b), _c(kinv), _c(offs), _c(offsets)]
    _l.check(_l.load().oi_aa_begin(ctypes.byref(st.c), _p(keep[0]), _p(keep[1]), _p(keep[2]), int(R), _ip(edge_index), int(n_edge),
                                   _p(keep[3]), offsets.shape[0], _stream()), "oi_aa_begin")


def aa_resolve(centre, sub, edge_slot, n_edge, S, out=None):
    """centre (P, N) and the sub-samples sub (P, (S - 1) * n_edge) (None with n_edge == 0) -> (P, N): centre off the flagged
    pixels, the mean of the S samples on them (oi_aa_resolve), written into `out` when given."""
    P, N = centre.shape
    if n_edge and (sub is None or tuple(sub.shape) != (P, (int(S) - 1) * int(n_edge))):
        raise ValueError(f"aa_resolve: sub {None if sub is None else tuple(sub.shape)}, expected {(P, (int(S) - 1) * int(n_edge))}")
    if edge_slot.shape[0] != N or edge_slot.dtype != torch.int32:
        raise ValueError(f"aa_resolve: edge_slot {tuple(edge_slot.shape)} {edge_slot.dtype}, expected int32 ({N},)")
    if out is None:
        out = _new(centre, P, N)
    elif tuple(out.shape) != (P, N) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError(f"aa_resolve: out must be a contiguous float32 {(P, N)} tensor")
    _l.check(_l.load().oi_aa_resolve(_p(centre), _p(sub) if n_edge else None, _ip(edge_slot), N, int(n_edge), int(S), P, _p(out),
                                     _stream()), "oi_aa_resolve")
    return out


# ------------------------------------------------------------------------------------------
# adaptive anti-aliasing of a scene of many instances (include/oi_scene_aa.h); oi_amd.scene sequences these
# ------------------------------------------------------------------------------------------

def scene_aa_classify(owner, owner_ray, vis_slot, hit_points, grad, n_pad, S, plane_threshold=_l.AA_DEFAULT_PLANE,
                      cos_threshold=_l.AA_DEFAULT_COS):
    """The scene pixels of a traced scene that need more samples (oi_scene_aa_classify).  owner, owner_ray (S * S,) int32,
    vis_slot (E, N) int32, hit_points and grad (E, n_pad, 3) (None with n_pad == 0).  -> edge_index (S * S,) int32 (its first
    `count` entries are written: the flagged pixels, in no fixed order), edge_slot (S * S,) int32 (the pixel's position in
    edge_index, or -1), count (1,) int32 on the device."""
    M = int(S) * int(S)
    E, N = vis_slot.shape
    if owner.shape[0] != M or owner_ray.shape[0] != M:
        raise ValueError(f"scene_aa_classify: owner {tuple(owner.shape)}, owner_ray {tuple(owner_ray.shape)} for {S} x {S} pixels")
    edge_index = torch.empty(M, dtype=torch.int32, device=owner.device)   # (partly written by contract, as aa_classify's)
    edge_slot = _new(owner, M).view(torch.int32)
    count = _new(owner, 1).view(torch.int32)
    _l.check(_l.load().oi_scene_aa_classify(_ip(owner), _ip(owner_ray), _ip(vis_slot), _p(hit_points) if n_pad else None,
                                            _p(grad) if n_pad else None, int(E), int(N), int(n_pad), int(S), float(plane_threshold),
                                            float(cos_threshold), _ip(edge_index), _ip(edge_slot), _ip(count), _stream()),
             "oi_scene_aa_classify")
    return edge_index, edge_slot, count


def scene_aa_begin(st, c2b, kinv, window, W, S, edge_index, n_edge, offsets):
    """The sub-pixel rays of the first n_edge pixels of edge_index in every instance's box frame, into the TraceBatchState st
    of E elements x at least (Sa - 1) * n_edge rays (oi_scene_aa_begin).  c2b (E, 4, 4), kinv (3, 3), window (E, 2) int32, W, S:
    scene_begin's; offsets (Sa, 2) float32 on the device, in units of the pixel pitch (row 0, the centre, is not read)."""
    if offsets.dim() != 2 or offsets.shape[1] != 2 or offsets.dtype != torch.float32:
        raise ValueError(f"scene_aa_begin: offsets {tuple(offsets.shape)} {offsets.dtype}, expected float32 (Sa, 2)")
    if c2b.numel() != st.E * 16 or kinv.numel() != 9 or window.numel() != st.E * 2:
        raise ValueError(f"scene_aa_begin: c2b, kinv and window must hold {st.E} x 16, 9 and {st.E} x 2 values")
    keep = [_c(c2b), _c(kinv), _c(offsets)]
    _l.check(_l.load().oi_scene_aa_begin(ctypes.byref(st.c), _p(keep[0]), _p(keep[1]), _ip(window), int(W), int(S), _ip(edge_index),
                                         int(n_edge), _p(keep[2]), offsets.shape[0], _stream()), "oi_scene_aa_begin")


def aa_resolve_strided(centre, sub, edge_slot, n_edge, S, out=None):
    """aa_resolve with the sub-samples' planes at a stride of their own (oi_aa_resolve_strided): sub (P, stride), stride >=
    (S - 1) * n_edge, of which the first (S - 1) * n_edge of every plane are read (None with n_edge == 0)."""
    P, N = centre.shape
    if n_edge and (sub is None or sub.dim() != 2 or sub.shape[0] != P or sub.shape[1] < (int(S) - 1) * int(n_edge)):
        raise ValueError(f"aa_resolve_strided: sub {None if sub is None else tuple(sub.shape)}, expected ({P}, at least "
                         f"{(int(S) - 1) * int(n_edge)})")
    if edge_slot.shape[0] != N or edge_slot.dtype != torch.int32:
        raise ValueError(f"aa_resolve_strided: edge_slot {tuple(edge_slot.shape)} {edge_slot.dtype}, expected int32 ({N},)")
    if out is None:
        out = _new(centre, P, N)
    elif tuple(out.shape) != (P, N) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError(f"aa_resolve_strided: out must be a contiguous float32 {(P, N)} tensor")
    stride = sub.shape[1] if n_edge else 0
    _l.check(_l.load().oi_aa_resolve_strided(_p(centre), _p(sub) if n_edge else None, stride, _ip(edge_slot), N, int(n_edge), int(S),
                                             P, _p(out), _stream()), "oi_aa_resolve_strided")
    return out


def scene_local_light_begin(sb, hit_points, grad, n_pad, offset, elem, pixel, position, normal, n_vis, w2b, bias, samples, j0, chunk,
                            lights, seed=0):
    """scene_occlusion_begin's chunk of rays aimed at local lights (L, 20) in the world frame: sb holds E occluder elements x
    L * chunk * n_vis rays."""
    _check_local("scene_local_light_begin", lights)
    P = _l.SceneOcclusionParams()
    P.L, P.S, P.j0, P.Sc, P.ambient = lights.shape[0], int(samples), int(j0), int(chunk), 0
    P.seed, P.bias, P.distance, P.n_pad, P.n_vis = int(seed), float(bias), 0.0, int(n_pad), int(n_vis)
    keep = [_c(x) for x in (hit_points, grad, position, normal, lights, w2b)]
    P.hit_points, P.grad, P.position, P.normal, P.lights, P.w2b = (_p(x) for x in keep)
    P.radius = None
    P.offset, P.elem, P.pixel = _ip(offset), _ip(elem), _ip(pixel)
    _l.check(_l.load().oi_scene_local_light_begin(ctypes.byref(sb.c), ctypes.byref(P), _stream()), "oi_scene_local_light_begin")


def scene_shade_local(st, W, S, owner, owner_ray, vis_slot, hit_points, grad, rgb, n_pad, w2b, b2w, lights=None, bg=None,
                      visibility=None, ambient_occlusion=None, outputs=tuple(SCENE_OUT) + ("image",), image_out=None):
    """scene_shade_ao under local lights (L, 20) in the world frame (oi_scene_shade_local)."""
    if ambient_occlusion is not None and tuple(ambient_occlusion.shape) != (S * S,):
        raise ValueError(f"scene_shade_local: ambient_occlusion {tuple(ambient_occlusion.shape)}, expected {(S * S,)}")
    A = _l.SceneShadeAoParams()
    res, _keep = _scene_shade("scene_shade_local", A.s, st, W, S, owner, owner_ray, vis_slot, hit_points, grad, rgb, n_pad, w2b, b2w,
                              lights, bg, visibility, outputs, image_out, _l.LOCAL_LIGHT_FLOATS)
    ao = _c(ambient_occlusion)
    A.ambient_occlusion = _p(ao)
    _l.check(_l.load().oi_scene_shade_local(ctypes.byref(A), _stream()), "oi_scene_shade_local")
    return res


# ------------------------------------------------------------------------------------------
# a ground plane that catches the instances' shadows (include/oi_ground.h); oi_amd.scene sequences these
# ------------------------------------------------------------------------------------------

def _check_ground_record(what, record):
    if not torch.is_tensor(record) or record.dtype != torch.float32 or tuple(record.shape) != (_l.GROUND_FLOATS,):
        raise ValueError(f"{what}: the ground record must be a float32 tensor of shape ({_l.GROUND_FLOATS},)")


def ground_begin(c2w, kinv, S, record, owner, owner_ray, t, window, W, E):
    """The ground pixels of a scene (oi_ground_begin).  c2w (4, 4), kinv (3, 3), record (12,) float32; owner, owner_ray (S * S,)
    int32, t (E, W * W), window (E, 2) int32 -- or owner None: no pixel is owned.  -> ground_t (S * S,) (NaN off the ground),
    ground_index (S * S,) int32 (its first `count` entries are written, in no fixed order), count (1,) int32 on the device."""
    _check_ground_record("ground_begin", record)
    M = int(S) * int(S)
    if c2w.numel() != 16 or kinv.numel() != 9:
        raise ValueError("ground_begin: c2w and kinv must hold 16 and 9 values")
    if owner is not None and (owner.shape[0] != M or owner_ray.shape[0] != M or t.numel() != int(E) * int(W) * int(W)):
        raise ValueError(f"ground_begin: owner {tuple(owner.shape)}, owner_ray {tuple(owner_ray.shape)}, t {tuple(t.shape)} for "
                         f"{S} x {S} pixels and {E} x {W} x {W} rays")
    keep = [_c(c2w), _c(kinv)]
    ground_t = _new(record, M)
    ground_index = torch.empty(M, dtype=torch.int32, device=record.device)   # (partly written by contract, as aa_classify's)
    count = _new(record, 1).view(torch.int32)
    _l.check(_l.load().oi_ground_begin(_p(keep[0]), _p(keep[1]), int(S), _p(record), _ip(owner), _ip(owner_ray), _p(t), _ip(window),
                                       int(W), int(E), _p(ground_t), _ip(ground_index), _ip(count), _stream()), "oi_ground_begin")
    return ground_t, ground_index, count


def ground_rays_begin(sb, c2w, kinv, S, record, ground_t, ground_index, n_g, w2b, bias, samples, j0, chunk, seed=0, lights=None,
                      radius=None, distance=None):
    """sb: TraceBatchState of E occluder elements x L * chunk * n_g rays: the samples [j0, j0 + chunk) of the secondary rays of
    the n_g ground points against every instance (oi_ground_rays_begin).  lights (L, 16) and radius (L,) float32: caps about
    directional lights; lights (L, 20): rays aimed at local lights; distance (a float, inf allowed) instead: the cosine
    hemisphere about the plane's normal."""
    _check_ground_record("ground_rays_begin", record)
    hemi = lights is None
    if hemi == (distance is None):
        raise ValueError("ground_rays_begin: give lights, or distance (the hemisphere)")
    local = not hemi and lights.shape[-1] == _l.LOCAL_LIGHT_FLOATS
    if not hemi and not local and (not torch.is_tensor(radius) or radius.dtype != torch.float32
                                   or tuple(radius.shape) != (lights.shape[0],)):
        raise ValueError(f"ground_rays_begin: radius must be a float32 tensor of shape ({lights.shape[0]},), one per light")
    if ground_index.dtype != torch.int32 or ground_index.numel() < int(n_g) or ground_t.numel() != int(S) * int(S):
        raise ValueError(f"ground_rays_begin: ground_index {tuple(ground_index.shape)} {ground_index.dtype}, ground_t "
                         f"{tuple(ground_t.shape)} for {n_g} ground points of {S} x {S} pixels")
    P = _l.SceneOcclusionParams()   # oi_scene_occlusion_begin's parameters: n_vis = n_g, pixel = the ground pixels
    P.L, P.S, P.j0, P.Sc, P.ambient = 1 if hemi else lights.shape[0], int(samples), int(j0), int(chunk), int(hemi)
    P.seed, P.bias, P.distance, P.n_pad, P.n_vis = int(seed), float(bias), float(distance) if hemi else 0.0, 0, int(n_g)
    keep = [_c(x) for x in (lights, None if local else radius, w2b, c2w, kinv)]
    P.lights, P.radius, P.w2b = (_p(x) for x in keep[:3])
    P.pixel = _ip(ground_index)
    mode = _l.GROUND_RAYS_HEMISPHERE if hemi else _l.GROUND_RAYS_LOCAL if local else _l.GROUND_RAYS_CAP
    _l.check(_l.load().oi_ground_rays_begin(ctypes.byref(sb.c), ctypes.byref(P), mode, _p(keep[3]), _p(keep[4]), int(S), _p(record),
                                            _p(ground_t), _stream()), "oi_ground_rays_begin")


def ground_resolve(status, E, n_g, L, samples, j0, chunk, count, out, last):
    """Adds the chunk's escaped samples to count (L, n_g) int32 (overwritten at j0 == 0); last: out (L, n_g) = count / samples."""
    _l.check(_l.load().oi_ground_resolve(_p(status), int(E), int(n_g), int(L), int(samples), int(j0), int(chunk), int(bool(last)),
                                         _ip(count), _p(out), _stream()), "oi_ground_resolve")


GROUND_OUT = ("image", "depth", "position", "normal_world", "albedo", "mask", "instance")


def ground_shade(c2w, kinv, S, record, ground_t, ground_index, n_g, lights, maps, visibility=None, ambient_occlusion=None):
    """The ground into the scene's maps, IN PLACE at the ground pixels (oi_ground_shade).  maps: {name: tensor} for names of
    GROUND_OUT -- image (L, 3, S * S), depth, mask (S * S,), position, normal_world, albedo (S * S, 3), instance (S * S,) int32 --
    as scene_shade returns them.  lights (L, 16) directional or (L, 20) local records; visibility (L, n_g), ambient_occlusion
    (n_g,) or None.  -> ground_mask (S * S,): 1 on the ground, 0 off it; shadow_matte (L, 3, S * S): 1 off the ground."""
    _check_ground_record("ground_shade", record)
    M, L = int(S) * int(S), lights.shape[0]
    shapes = {"image": (L, 3, M), "depth": (M,), "mask": (M,), "instance": (M,), "position": (M, 3), "normal_world": (M, 3),
              "albedo": (M, 3)}
    for k, v in maps.items():
        if k not in shapes or tuple(v.shape) != shapes[k] or not v.is_contiguous():
            raise ValueError(f"ground_shade: {k} {tuple(v.shape)}, expected a contiguous {shapes.get(k)} of {GROUND_OUT}")
    if visibility is not None and tuple(visibility.shape) != (L, int(n_g)):
        raise ValueError(f"ground_shade: visibility {tuple(visibility.shape)}, expected {(L, int(n_g))}")
    if ambient_occlusion is not None and tuple(ambient_occlusion.shape) != (int(n_g),):
        raise ValueError(f"ground_shade: ambient_occlusion {tuple(ambient_occlusion.shape)}, expected {(int(n_g),)}")
    ground_mask, matte = _new(record, M), _new(record, L, 3, M)
    ground_mask.zero_()
    matte.fill_(1.0)
    if int(n_g) == 0:
        return ground_mask, matte
    keep = [_c(x) for x in (c2w, kinv, lights, visibility, ambient_occlusion)]
    outs = [(_ip if k == "instance" else _p)(maps.get(k)) for k in GROUND_OUT]
    _l.check(_l.load().oi_ground_shade(_p(keep[0]), _p(keep[1]), int(S), _p(record), _p(ground_t), _ip(ground_index), int(n_g),
                                       _p(keep[2]), L, int(lights.shape[-1] == _l.LOCAL_LIGHT_FLOATS), _p(keep[3]), _p(keep[4]), *outs,
                                       _p(ground_mask), _p(matte), _stream()), "oi_ground_shade")
    return ground_mask, matte


def ground_occlude(sb, record, elem, b2w, n_vis, limit):
    """The ground as occluder of the instances' rays (oi_ground_occlude): in the finished chunk sb of scene_occlusion_begin or
    scene_shadow_begin, the owner's ray of every visible point turns from MISS to HIT where it meets the plane before `limit`
    (inf for directional rays)."""
    _check_ground_record("ground_occlude", record)
    keep = _c(b2w)
    _l.check(_l.load().oi_ground_occlude(ctypes.byref(sb.c), _p(record), _ip(elem), _p(keep), int(n_vis), float(limit), _stream()),
             "oi_ground_occlude")


# ------------------------------------------------------------------------------------------
# environment lighting on the traced surface (include/oi_envlight.h)
# ------------------------------------------------------------------------------------------

def env_project(radiance):
    """Equirectangular maps (E, 3, He, We) float32 on the device -> SH coefficients (E, 9, 3) (oi_env_project)."""
    if not torch.is_tensor(radiance) or radiance.dim() != 4 or radiance.shape[1] != 3:
        raise ValueError(f"env_project: radiance {tuple(getattr(radiance, 'shape', ()))}, expected (E, 3, He, We)")
    E, _, He, We = radiance.shape
    if not (1 <= E <= _l.ENV_MAX_ENVS and He >= 1 and We >= 1 and E * He * We < 1 << 31):
        raise ValueError(f"env_project: E={E}, He={He}, We={We} (1 <= E <= {_l.ENV_MAX_ENVS}, He, We >= 1, E * He * We < 2^31)")
    radiance = _c(radiance)
    L = _l.load()
    partial = _new(radiance, L.oi_env_project_partial_floats(E, He, We))
    coeffs = _new(radiance, E, _l.ENV_COEFFS, 3)
    _l.check(L.oi_env_project(_p(radiance), E, He, We, _p(partial), _p(coeffs), _stream()), "oi_env_project")
    return coeffs


def transfer_resolve(status, rays_d, hit_slot, N, n_hit, samples, w2b):
    """The finished states (S * n_hit,) uint8 and directions (S * n_hit, 3) of an ambient-occlusion trace -> the transfer map
    (9, N) float32: per pixel the mean over its `samples` rays of [escaped] y_c(world direction); zeros off the mask."""
    out = _new(hit_slot, _l.ENV_COEFFS, N)
    _l.check(_l.load().oi_transfer_resolve(_p(status), _p(rays_d), _ip(hit_slot), int(N), int(n_hit), int(samples), _p(w2b),
                                           _p(out), _stream()), "oi_transfer_resolve")
    return out


def transfer_normal(grad, hit_slot, N, n_hit, w2b):
    """The unshadowed transfer map (9, N) of the normals grad (n_hit, 3): A_band y_c(world normal); zeros off the mask."""
    out = _new(hit_slot, _l.ENV_COEFFS, N)
    _l.check(_l.load().oi_transfer_normal(_p(grad), _ip(hit_slot), int(N), int(n_hit), _p(w2b), _p(out), _stream()),
             "oi_transfer_normal")
    return out


ENV_SHADE_OUT = ("shading", "image")


def _env_shade(what, table, P, status, hit_slot, rgb, n_hit, transfer, envs, bg, outputs, out, own=None):
    """What env_shade, env_shade_bounce and env_shade_glossy share, for the output table `table`: the checks of envs, transfer
    and `outputs`, then the caller's own checks own(N, F), the output planes (F, 3, N) (out[name] when given) and the fields
    of EnvShadeParams in the struct P.  -> ({name: plane}, tensors to keep, what own returned)."""
    N = transfer.shape[1]
    F = envs.shape[0] if torch.is_tensor(envs) and envs.dim() == 3 else 0
    if not 1 <= F <= _l.ENV_MAX_ENVS or tuple(envs.shape[1:]) != (_l.ENV_COEFFS, 3):
        raise ValueError(f"{what}: envs {tuple(getattr(envs, 'shape', ()))}, expected (F, {_l.ENV_COEFFS}, 3) with "
                         f"1 <= F <= {_l.ENV_MAX_ENVS}")
    if tuple(transfer.shape) != (_l.ENV_COEFFS, N) or not outputs:
        raise ValueError(f"{what}: transfer {tuple(transfer.shape)}, expected ({_l.ENV_COEFFS}, N); outputs {outputs!r}")
    extra = own(N, F) if own else None
    res = {}
    for name in outputs:
        if name not in table:
            raise ValueError(f"{what}: unknown output {name!r} (one of {table})")
        t = None if out is None else out.get(name)
        if t is None:
            t = _new(transfer, F, 3, N)
        elif tuple(t.shape) != (F, 3, N) or not t.is_contiguous() or t.dtype != torch.float32:
            raise ValueError(f"{what}: out[{name!r}] must be a contiguous float32 {(F, 3, N)} tensor")
        res[name] = t
    P.N, P.n_hit, P.F = N, int(n_hit), F
    keep = [_c(x) for x in (rgb if n_hit else None, transfer, envs, bg)]
    P.rgb, P.transfer, P.envs, P.bg = (_p(x) for x in keep)
    P.status, P.hit_slot = _p(status), _ip(hit_slot)
    P.shading, P.image = _p(res.get("shading")), _p(res.get("image"))
    return res, keep, extra


def env_shade(status, hit_slot, rgb, n_hit, transfer, envs, bg=None, outputs=ENV_SHADE_OUT, out=None):
    """One captured view under the environments envs (F, 9, 3) (oi_env_shade).  -> {name: (F, 3, N)} for the names of
    ENV_SHADE_OUT in `outputs` (written into out[name] when given)."""
    P = _l.EnvShadeParams()
    res, _keep, _ = _env_shade("env_shade", ENV_SHADE_OUT, P, status, hit_slot, rgb, n_hit, transfer, envs, bg, outputs, out)
    _l.check(_l.load().oi_env_shade(ctypes.byref(P), _stream()), "oi_env_shade")
    return res


# ------------------------------------------------------------------------------------------
# one diffuse interreflection bounce under environment lighting (include/oi_envbounce.h)
# ------------------------------------------------------------------------------------------

def bounce_resolve(status, rays_d, hit_slot2, grad2, rgb2, n_hit2, hit_slot, N, n_hit, samples, w2b):
    """The finished states (S * n_hit,) uint8, directions (S * n_hit, 3) and secondary hit slots (S * n_hit,) int32 of a
    closest-hit trace of the transfer rays, the gradients and albedo (n_hit2, 3) at its hits (None when n_hit2 == 0) -> the
    bounce transfer (3, 9, N) float32: per pixel and channel the mean over its `samples` rays of [front-facing hit] albedo
    A_band y_c(world normal at the hit); zeros off the mask."""
    out = _new(hit_slot, 3, _l.ENV_COEFFS, N)
    g2, c2 = (_c(grad2), _c(rgb2)) if n_hit2 else (None, None)
    _l.check(_l.load().oi_bounce_resolve(_p(status), _p(rays_d), _ip(hit_slot2), _p(g2), _p(c2), _ip(hit_slot), int(N),
                                         int(n_hit), int(n_hit2), int(samples), _p(w2b), _p(out), _stream()), "oi_bounce_resolve")
    return out


ENV_BOUNCE_OUT = ENV_SHADE_OUT + ("indirect",)


def env_shade_bounce(status, hit_slot, rgb, n_hit, transfer, bounce, envs, bg=None, outputs=ENV_BOUNCE_OUT, out=None):
    """env_shade with the bounce transfer (3, 9, N) of bounce_resolve (oi_env_shade_bounce).  -> {name: (F, 3, N)} for the names
    of ENV_BOUNCE_OUT in `outputs` (written into out[name] when given): shading = direct + indirect."""
    def own(N, F):
        if not torch.is_tensor(bounce) or tuple(bounce.shape) != (3, _l.ENV_COEFFS, N):
            raise ValueError(f"env_shade_bounce: bounce {tuple(getattr(bounce, 'shape', ()))}, expected (3, {_l.ENV_COEFFS}, {N})")

    P = _l.EnvShadeBounceParams()
    res, _keep, _ = _env_shade("env_shade_bounce", ENV_BOUNCE_OUT, P, status, hit_slot, rgb, n_hit, transfer, envs, bg, outputs, out,
                               own)
    bounce = _c(bounce)
    P.bounce, P.indirect = _p(bounce), _p(res.get("indirect"))
    _l.check(_l.load().oi_env_shade_bounce(ctypes.byref(P), _stream()), "oi_env_shade_bounce")
    return res


# ------------------------------------------------------------------------------------------
# glossy environment lighting on the traced surface (include/oi_envgloss.h)
# ------------------------------------------------------------------------------------------

def check_shininess(shininess, what):
    """include/oi_envgloss.h's range of a shininess -> float."""
    try:
        s = float(shininess)
    except (TypeError, ValueError):
        s = float("nan")
    if isinstance(shininess, bool) or not _l.ENVGLOSS_MIN_SHININESS <= s <= _l.ENVGLOSS_MAX_SHININESS:
        raise ValueError(f"{what}: shininess={shininess!r} ({_l.ENVGLOSS_MIN_SHININESS} <= shininess <= "
                         f"{_l.ENVGLOSS_MAX_SHININESS}, finite)")
    return s


def env_prefilter(radiance, shininess, size):
    """Equirectangular maps (E, 3, He, We) float32 on the device -> their Phong-lobe convolutions (E, 3, Hp, Wp) at one
    shininess, size = (Hp, Wp) (oi_env_prefilter)."""
    if not torch.is_tensor(radiance) or radiance.dim() != 4 or radiance.shape[1] != 3:
        raise ValueError(f"env_prefilter: radiance {tuple(getattr(radiance, 'shape', ()))}, expected (E, 3, He, We)")
    s = check_shininess(shininess, "env_prefilter")
    E, _, He, We = radiance.shape
    Hp, Wp = (int(v) for v in size)
    L = _l.load()
    nf = L.oi_env_prefilter_partial_floats(E, He, We, Hp, Wp) if min(E, He, We, Hp, Wp) >= 1 else 0
    if nf == 0:
        raise ValueError(f"env_prefilter: E={E}, He={He}, We={We}, size={(Hp, Wp)} (1 <= E <= {_l.ENV_MAX_ENVS}, sizes >= 1, "
                         f"E * He * We and E * 3 * Hp * Wp below 2^31, E * ceil(He * We / {_l.ENVGLOSS_CHUNK}) * "
                         "ceil(Hp * Wp / 256) workgroups at most 2^23)")
    radiance = _c(radiance)
    partial = _new(radiance, nf)
    glossy = _new(radiance, E, 3, Hp, Wp)
    _l.check(L.oi_env_prefilter(_p(radiance), E, He, We, s, Hp, Wp, _p(partial), _p(glossy), _stream()), "oi_env_prefilter")
    return glossy


def occlusion_lobe_begin(st, rays_o, hit_points, grad, hit_index, n_hit, samples, shininess, bias, seed=0):
    """S = samples reflection-lobe rays per hit into the TraceState st of S * n_hit rays; rays_o (N, 3): the primary eyes."""
    _l.check(_l.load().oi_occlusion_lobe_begin(ctypes.byref(st.c), _p(rays_o), _p(hit_points), _p(grad), _ip(hit_index), int(n_hit),
                                               int(samples), float(shininess), float(bias), int(seed), _stream()),
             "oi_occlusion_lobe_begin")


ENV_GLOSSY_OUT = ENV_SHADE_OUT + ("specular",)


def _gloss_own(what, glossy, map_index, rot, k_s, spec_vis, dirs=None):
    """env_shade_glossy's and env_shade_glossy_dirs' own checks for _env_shade: -> own(N, F), which returns the map indices as a
    host array of F C integers."""
    def own(N, F):
        if not torch.is_tensor(glossy) or glossy.dim() != 4 or glossy.shape[1] != 3 or not 1 <= glossy.shape[0] <= _l.ENV_MAX_ENVS:
            raise ValueError(f"{what}: glossy {tuple(getattr(glossy, 'shape', ()))}, expected (M, 3, Hp, Wp) with "
                             f"1 <= M <= {_l.ENV_MAX_ENVS}")
        M = glossy.shape[0]
        idx = [int(v) for v in map_index]
        if len(idx) != F or any(not 0 <= v < M for v in idx):
            raise ValueError(f"{what}: map_index {idx} (F = {F} integers, 0 <= map_index < M = {M})")
        if tuple(rot.shape) != (F, 3, 3) or tuple(k_s.shape) != (3,) or (spec_vis is not None and tuple(spec_vis.shape) != (N,)):
            raise ValueError(f"{what}: rot {tuple(rot.shape)}, k_s {tuple(k_s.shape)}, expected {(F, 3, 3)} and (3,); "
                             f"spec_vis (N,) = {(N,)} or None")
        if dirs is not None and tuple(dirs.shape) != (N, 3):
            raise ValueError(f"{what}: dirs {tuple(dirs.shape)}, expected {(N, 3)}")
        return (ctypes.c_int * F)(*idx)
    return own


def env_shade_glossy(status, hit_slot, rgb, n_hit, transfer, envs, rays_o, hit_points, grad, w2b, spec_vis, glossy, map_index,
                     rot, k_s, bg=None, outputs=ENV_GLOSSY_OUT, out=None):
    """env_shade plus the glossy term (oi_env_shade_glossy): envs (F, 9, 3) the SH halves, glossy (M, 3, Hp, Wp) the
    prefiltered maps, map_index F host integers in [0, M) (checked here, before anything is uploaded), rot (F, 3, 3) world
    rotations, k_s (3,), spec_vis (N,) or None (= 1).  -> {name: (F, 3, N)} for the names of ENV_GLOSSY_OUT in `outputs`."""
    P = _l.EnvShadeParams()
    res, _keep, index = _env_shade("env_shade_glossy", ENV_GLOSSY_OUT, P, status, hit_slot, rgb, n_hit, transfer, envs, bg, outputs,
                                   out, _gloss_own("env_shade_glossy", glossy, map_index, rot, k_s, spec_vis))
    M, _, Hp, Wp = glossy.shape
    more = [_c(x) for x in (rays_o, hit_points if n_hit else None, grad if n_hit else None, w2b, spec_vis, glossy, rot, k_s)]
    ro, hp, g, wb, sv, gl, rt, ks = (_p(x) for x in more)
    _l.check(_l.load().oi_env_shade_glossy(ctypes.byref(P), ro, hp, g, wb, sv, gl, M, Hp, Wp, index, rt, ks,
                                           _p(res.get("specular")), _stream()), "oi_env_shade_glossy")
    return res


# ------------------------------------------------------------------------------------------
# glossy environment lighting in a scene of many instances (include/oi_scene_gloss.h); oi_amd.scene sequences these
# ------------------------------------------------------------------------------------------

def scene_lobe_begin(sb, rays_o, vis_index, N, hit_points, grad, n_pad, offset, elem, pixel, position, normal, n_vis, w2b, bias,
                     samples, j0, chunk, shininess, seed=0):
    """sb: TraceBatchState of E occluder elements x chunk * n_vis rays (trace_batch_state_empty): the samples [j0, j0 + chunk)
    of `samples` reflection-lobe rays per visible point, distributed as cos^shininess about the reflected view vector.  rays_o
    (E, N, 3): the primary batch's origins; vis_index (E, N) int32."""
    P = _l.SceneOcclusionParams()
    P.L, P.S, P.j0, P.Sc, P.ambient = 1, int(samples), int(j0), int(chunk), 1
    P.seed, P.bias, P.distance, P.n_pad, P.n_vis = int(seed), float(bias), float("inf"), int(n_pad), int(n_vis)
    keep = [_c(x) for x in (hit_points, grad, position, normal, w2b, rays_o)]
    P.hit_points, P.grad, P.position, P.normal, P.w2b, eyes = (_p(x) for x in keep)
    P.offset, P.elem, P.pixel = _ip(offset), _ip(elem), _ip(pixel)
    _l.check(_l.load().oi_scene_lobe_begin(ctypes.byref(sb.c), ctypes.byref(P), eyes, _ip(vis_index), int(N), float(shininess),
                                           _stream()), "oi_scene_lobe_begin")


def scene_reflect(rays_o, hit_points, grad, n_pad, owner, owner_ray, vis_slot, w2b, E, N, S):
    """-> the reflected view vector of every scene pixel (S * S, 3), world frame; zeros off the mask."""
    out = _new(grad, S * S, 3)
    _l.check(_l.load().oi_scene_reflect(_p(_c(rays_o)), _p(_c(hit_points)), _p(_c(grad)), int(n_pad), _ip(owner), _ip(owner_ray),
                                        _ip(vis_slot), _p(_c(w2b)), int(E), int(N), int(S), _p(out), _stream()), "oi_scene_reflect")
    return out


def env_shade_glossy_dirs(status, hit_slot, rgb, n_hit, transfer, envs, dirs, spec_vis, glossy, map_index, rot, k_s, bg=None,
                          outputs=ENV_GLOSSY_OUT, out=None):
    """env_shade_glossy with the world-frame lookup direction given per pixel, dirs (N, 3), in place of the eyes, the hits and
    the pose (oi_env_shade_glossy_dirs): a scene's planes.  -> {name: (F, 3, N)} for the names of ENV_GLOSSY_OUT in `outputs`."""
    what = "env_shade_glossy_dirs"
    if not torch.is_tensor(dirs) or dirs.dim() != 2:
        raise ValueError(f"{what}: dirs {tuple(getattr(dirs, 'shape', ()))}, expected (N, 3)")
    P = _l.EnvShadeParams()
    res, _keep, index = _env_shade(what, ENV_GLOSSY_OUT, P, status, hit_slot, rgb, n_hit, transfer, envs, bg, outputs, out,
                                   _gloss_own(what, glossy, map_index, rot, k_s, spec_vis, dirs))
    M, _, Hp, Wp = glossy.shape
    more = [_c(x) for x in (dirs, spec_vis, glossy, rot, k_s)]
    dr, sv, gl, rt, ks = (_p(x) for x in more)
    _l.check(_l.load().oi_env_shade_glossy_dirs(ctypes.byref(P), dr, sv, gl, M, Hp, Wp, index, rt, ks, _p(res.get("specular")),
                                                _stream()), "oi_env_shade_glossy_dirs")
    return res


# ------------------------------------------------------------------------------------------
# one diffuse interreflection bounce between the instances of a scene (include/oi_scene_bounce.h); oi_amd.scene sequences these
# ------------------------------------------------------------------------------------------

def scene_bounce_nearest(status, t, E, rays):
    """The finished states status (E, rays) uint8 and ray parameters t (E, rays) of a closest-hit batch -> winner (rays,) int32:
    the element whose HIT is nearest (the lowest index on equal t), -1 without one or when the ray ended in any element in a
    status other than MISS or HIT."""
    winner = _new(t, int(rays)).view(torch.int32)
    _l.check(_l.load().oi_scene_bounce_nearest(_p(status), _p(t), int(E), int(rays), _ip(winner), _stream()),
             "oi_scene_bounce_nearest")
    return winner


def scene_bounce_visible(sb, winner):
    """-> sel_index (E, N) int32 (the first n_sel_e entries of row e are written: the rays element e wins), sel_slot (E, N)
    int32 (-1 where the ray is not won).  Overwrites the hit words of sb.counts and sb.live with the selected counts."""
    sel_index = torch.empty(sb.E, sb.N, dtype=torch.int32, device=sb.t.device)
    sel_slot = _new(sb.t, sb.E, sb.N).view(torch.int32)
    _l.check(_l.load().oi_scene_bounce_visible(ctypes.byref(sb.c), _ip(winner), _ip(sel_index), _ip(sel_slot), _stream()),
             "oi_scene_bounce_visible")
    return sel_index, sel_slot


def scene_bounce_resolve(winner, sel_slot, rays_d, grad2, rgb2, n_pad2, owner, owner_ray, vis_slot, offset, w2b, E, N, samples, j0,
                         chunk, n_vis, S, bounce, last):
    """Adds the chunk's front-face winners' albedo A_band y_c(world normal) to bounce (3, 9, S * S) (overwritten at j0 == 0);
    last: divided by samples.  grad2, rgb2 (E, n_pad2, 3): the full pass at the gathered points (None with n_pad2 == 0)."""
    g2, c2 = (_c(grad2), _c(rgb2)) if n_pad2 else (None, None)
    _l.check(_l.load().oi_scene_bounce_resolve(_ip(winner), _ip(sel_slot), _p(rays_d), _p(g2), _p(c2), int(n_pad2), _ip(owner),
                                               _ip(owner_ray), _ip(vis_slot), _ip(offset), _p(_c(w2b)), int(E), int(N), int(samples),
                                               int(j0), int(chunk), int(n_vis), int(S), int(bool(last)), _p(bounce), _stream()),
             "oi_scene_bounce_resolve")


# ------------------------------------------------------------------------------------------
# discriminator side
# ------------------------------------------------------------------------------------------

def conv4x4_out_shape(x_shape, Cout, stride, pad):
    B, _, H, W = x_shape
    return B, Cout, (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1


def conv4x4_fwd(x, w, bias=None, stride=2, pad=1, slope=0.2, out=None, x_slope=1.0, any_scale=False, zero_tail=0,
                out_is_zero=None):
    """y = lrelu_slope(conv(lrelu_x_slope(x)) + bias).  `out`: optional ZERO-FILLED contiguous output (e.g. a view of an
    arena shared by a chain of layers): the split-K path then needs no fill launch of its own.  `x_slope`: LeakyReLU
    applied to x while it is loaded (the producing layer handed over pre-activations).  `any_scale`: an operand may be a
    gradient (OI_CONV_ANY_SCALE: fp32 matrix cores only)."""
    L = _l.load()
    x, w = _c(x), _c(w)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    assert w.shape[1:] == (Cin, 4, 4)
    shape = conv4x4_out_shape(x.shape, Cout, stride, pad)
    if out is None:
        y = _new_acc(x, *shape)
    else:
        assert tuple(out.shape) == shape and out.is_contiguous() and out.dtype == torch.float32, (out.shape, shape)
        y = out
    # `zero_tail`: floats of the arena behind `out` that this launch also clears (oi_conv4x4_fwd_arena);
    # `out_is_zero`: whether `out` already holds zeros (default: it does when given)
    zero = (out is not None) if out_is_zero is None else bool(out_is_zero)
    if out is not None and not zero and _active_pool() is not None:
        out.zero_()  # under a ZeroPool the library clears nothing: a caller-owned output that is not yet zero is cleared here
        zero = True
    _l.check(L.oi_conv4x4_fwd_arena(_p(x), _p(w), _p(_c(bias)), _p(y), B, Cin, H, W, Cout, stride, pad, float(slope),
                                    float(x_slope), int(zero) | (2 if any_scale else 0), int(zero_tail), _stream()),
             "oi_conv4x4_fwd")
    return y


def conv4x4_dgrad(g, w, H, W, stride=2, pad=1, mask_ref=None, slope=1.0):
    """mask_ref: the producing layer's forward output -- its LeakyReLU is applied to `g` on load (oi_conv4x4_dgrad_masked)."""
    L = _l.load()
    g, w = _c(g), _c(w)
    B, Cout = g.shape[:2]
    Cin = w.shape[1]
    gx = _new_acc(g, B, Cin, H, W)
    _l.check(L.oi_conv4x4_dgrad_masked(_p(g), _p(_c(mask_ref)), float(slope), _p(w), _p(gx), B, Cin, H, W, Cout, stride, pad,
                                       _stream()), "oi_conv4x4_dgrad")
    return gx


def conv4x4_wgrad(g, x, stride=2, pad=1, mask_ref=None, slope=1.0, acc=None):
    """acc: a [Cout, Cin, 4, 4] buffer that already holds a gradient (or zeros) -- this one is added to it and `acc` returned."""
    L = _l.load()
    g, x = _c(g), _c(x)
    B, Cin, H, W = x.shape
    Cout = g.shape[1]
    if acc is not None and (tuple(acc.shape) != (Cout, Cin, 4, 4) or not acc.is_contiguous()):
        raise _l.OiHipError(f"conv4x4_wgrad: accumulator of shape {tuple(acc.shape)} for a {(Cout, Cin, 4, 4)} gradient")
    gw = _new_acc(g, Cout, Cin, 4, 4) if acc is None else acc
    _l.check(L.oi_conv4x4_wgrad_masked(_p(g), _p(_c(mask_ref)), float(slope), _p(x), _p(gw), int(acc is not None), B, Cin, H, W,
                                       Cout, stride, pad, _stream()), "oi_conv4x4_wgrad")
    return gw


def conv4x4_dgrad_pre(g, w, x, x_slope, stride=2, pad=1):
    """Data gradient of y = conv(lrelu_{x_slope}(x), w) with respect to the pre-activation x (oi_conv4x4_dgrad_pre)."""
    L = _l.load()
    g, w, x = _c(g), _c(w), _c(x)
    B, Cin, H, W = x.shape
    gx = _new_acc(g, B, Cin, H, W)
    _l.check(L.oi_conv4x4_dgrad_pre(_p(g), _p(w), _p(x), float(x_slope), _p(gx), B, Cin, H, W, g.shape[1], stride, pad,
                                    _stream()), "oi_conv4x4_dgrad_pre")
    return gx


def conv4x4_bwd(g, w, x, stride=2, pad=1, mask_ref=None, slope=1.0, acc=None, x_slope=1.0):
    """Data and weight gradient of one layer in one launch (oi_conv4x4_bwd_pre) -> gx, gw (gw is `acc` when given).
    x_slope != 1: x is a pre-activation (the layer computed conv(lrelu(x), w)); gx is the gradient with respect to it."""
    L = _l.load()
    g, w, x = _c(g), _c(w), _c(x)
    B, Cin, H, W = x.shape
    Cout = g.shape[1]
    if acc is not None and (tuple(acc.shape) != (Cout, Cin, 4, 4) or not acc.is_contiguous()):
        raise _l.OiHipError(f"conv4x4_bwd: accumulator of shape {tuple(acc.shape)} for a {(Cout, Cin, 4, 4)} gradient")
    gx = _new_acc(g, B, Cin, H, W)
    gw = _new_acc(g, Cout, Cin, 4, 4) if acc is None else acc
    _l.check(L.oi_conv4x4_bwd_pre(_p(g), _p(_c(mask_ref)), float(slope), _p(w), _p(x), float(x_slope), _p(gx), _p(gw),
                                  int(acc is not None), B, Cin, H, W, Cout, stride, pad, _stream()), "oi_conv4x4_bwd")
    return gx, gw


class GradSink:
    """Weight-gradient accumulators for ONE plain backward pass (not create_graph): while active, the convolution Functions
    of oi_amd.autograd_conv add every weight-gradient contribution of a registered weight straight into its buffer
    (oi_conv4x4_wgrad_masked, accumulate) and hand autograd nothing for it -- instead of one fresh tensor per contribution
    that autograd then sums with one `+=` launch each (a discriminator step has four contributions per weight).  The owner
    zeroes the buffers beforehand and installs them as `.grad` afterwards (oi_amd.graphed.GraphedDStep)."""

    _active = None

    def __init__(self, buffers):
        self.buffers = {int(k): v for k, v in buffers.items()}   # weight.data_ptr() -> accumulator

    def __enter__(self):
        assert GradSink._active is None, "nested GradSink"
        GradSink._active = self
        return self

    def __exit__(self, *exc):
        GradSink._active = None

    @staticmethod
    def lookup(w):
        s = GradSink._active
        return None if s is None else s.buffers.get(w.data_ptr())


def lrelu_mask_mul(v, ref, slope):
    L = _l.load()
    v, ref = _c(v), _c(ref)
    out = _new(v, *v.shape)
    _l.check(L.oi_lrelu_mask_mul(_p(v), _p(ref), _p(out), v.numel(), float(slope), _stream()), "oi_lrelu_mask_mul")
    return out


def light_dir_fwd(d, w2b):
    L = _l.load()
    d, w2b = _c(d), _c(w2b)
    n = _new(w2b, w2b.shape[0], 3)
    _l.check(L.oi_light_dir_fwd(_p(d), _p(w2b), _p(n), w2b.shape[0], _stream()), "oi_light_dir_fwd")
    return n


def light_dir_bwd(d, w2b, g_n):
    L = _l.load()
    d, w2b, g_n = _c(d), _c(w2b), _c(g_n)
    g_d = _new(d, 3)
    _l.check(L.oi_light_dir_bwd(_p(d), _p(w2b), _p(g_n), _p(g_d), w2b.shape[0], _stream()), "oi_light_dir_bwd")
    return g_d


def _gan_shapes(d_real, d_fake, pose, gx, aux_w):
    """(B, K, N) of the fused GAN-loss launches, with the shape checks the ATen composition they replace performed on its
    own (torch.split / mse_loss raise on a mismatch; the kernels index raw pointers)."""
    ref = d_real if d_real is not None else d_fake
    if ref is None or ref.dim() != 2:
        raise ValueError("gan_losses: logits must be [B, K]")
    B, K = ref.shape
    for name, t in (("d_real", d_real), ("d_fake", d_fake)):
        if t is not None and tuple(t.shape) != (B, K):
            raise ValueError(f"gan_losses: {name} is {tuple(t.shape)}, expected {(B, K)}")
    if pose is not None:
        if d_fake is None:
            raise ValueError("gan_losses: a pose target needs the fake logits")
        if tuple(pose.shape) != (B, K - 1):
            raise ValueError(f"gan_losses: pose is {tuple(pose.shape)}, expected {(B, K - 1)} (logits [:, 1:], position.py:4-12)")
        if aux_w is None or aux_w.numel() != 1:
            raise ValueError("gan_losses: a pose target needs its weight (one device scalar)")
    if gx is not None and (gx.dim() < 1 or gx.shape[0] != B):
        raise ValueError(f"gan_losses: the R1 gradient has leading dimension {tuple(gx.shape)[:1]}, expected {B}")
    return B, K, (0 if gx is None else gx.numel() // B)


def gan_losses_fwd(d_real, d_fake, pose, gx, aux_w, reg_w):
    """-> out6 = (total, real + fake, reg, fake, real, aux): see oi_gan_losses_fwd.  d_real / d_fake [B, K] (or None),
    pose [B, K-1] (or None), gx [B, ...] (or None), aux_w a device scalar tensor (or None)."""
    L = _l.load()
    B, K, N = _gan_shapes(d_real, d_fake, pose, gx, aux_w)
    out = _new(d_real if d_real is not None else d_fake, 6)
    _l.check(L.oi_gan_losses_fwd(_p(d_real), _p(d_fake), _p(pose), _p(gx), _p(aux_w), float(reg_w), _p(out), B, K, N, _stream()),
             "oi_gan_losses_fwd")
    return out


def stage_inputs(copies, imm=None, imm_dst=None):
    """One launch for the inputs of a captured step: `copies` = up to 4 (src, dst) pairs of equally sized contiguous float32
    device tensors; `imm` = up to 64 Python / numpy floats written to the device tensor `imm_dst` (oi_stage_inputs)."""
    L = _l.load()
    copies = [(s_, d_) for s_, d_ in copies if s_ is not None]
    n = len(copies)
    for s_, d_ in copies:
        assert s_.numel() == d_.numel(), (tuple(s_.shape), tuple(d_.shape))
    srcs = (ctypes.c_void_p * max(n, 1))(*[_p(_c(s_.detach())).value for s_, _ in copies])
    dsts = (ctypes.c_void_p * max(n, 1))(*[_p(d_).value for _, d_ in copies])
    cnts = (ctypes.c_longlong * max(n, 1))(*[s_.numel() for s_, _ in copies])
    vals = [] if imm is None else [float(v) for v in imm]
    assert len(vals) <= 64 and (not vals or imm_dst.numel() >= len(vals))
    immv = (ctypes.c_float * max(len(vals), 1))(*vals)
    _l.check(L.oi_stage_inputs(srcs, dsts, cnts, n, immv, len(vals), _p(imm_dst) if vals else None, _stream()), "oi_stage_inputs")


def scalar_glue(variance, ambient, specular, shininess):
    """-> (out5 = [inv_s, 1 / inv_s, ambient colour, diffuse colour, specular colour], packed3 = the compositing kernel's light
    block) from the four 0-dim parameters: one launch (oi_scalar_glue)."""
    L = _l.load()
    out5, packed = _new(variance, 5), _new(variance, 3)
    ps = [_p(t.detach().reshape(1)) for t in (variance, ambient, specular, shininess)]
    _l.check(L.oi_scalar_glue(*ps, _p(out5), _p(packed), _stream()), "oi_scalar_glue")
    return out5, packed


def upload_small(values, device):
    """numpy / Python floats (<= 64 of them) -> a new float32 device tensor of the same shape, through the ARGUMENTS of one launch
    (oi_stage_inputs): no pageable host-to-device copy -- which makes the host wait for everything queued on the stream -- and
    no pinned staging ring."""
    import numpy as np
    arr = np.ascontiguousarray(values, dtype=np.float32)
    out = torch.empty(arr.shape, dtype=torch.float32, device=device)
    stage_inputs([], arr.ravel(), out)
    return out


def render_scalars_fwd(r4, inv_nt):
    """(gradient_error, surface_loss) = (r4[0] / (r4[1] + 1e-5), r4[2] * inv_nt) as a [2] tensor."""
    L = _l.load()
    out = _new(r4, 2)
    _l.check(L.oi_render_scalars_fwd(_p(r4), float(inv_nt), _p(out), _stream()), "oi_render_scalars_fwd")
    return out


def render_scalars_bwd(r4, g_err, g_surf, inv_nt):
    L = _l.load()
    g = _new(r4, 4)
    _l.check(L.oi_render_scalars_bwd(_p(r4), _p(g_err), _p(g_surf), float(inv_nt), _p(g), _stream()), "oi_render_scalars_bwd")
    return g


def weighted_sum_fwd(terms, weights):
    """sum_i weights[i] * terms[i] over up to 8 device scalars (0-dim or 1-element float32 tensors) -> 0-dim tensor."""
    L = _l.load()
    n = len(terms)
    ptrs = (ctypes.c_void_p * n)(*[_p(t).value for t in terms])
    ws = (ctypes.c_float * n)(*[float(w) for w in weights])
    out = _new(terms[0])
    _l.check(L.oi_weighted_sum_fwd(ptrs, ws, n, _p(out), _stream()), "oi_weighted_sum_fwd")
    return out


def weighted_sum_bwd(g_out, weights, device):
    """-> [n] tensor of weights[i] * g_out (g_out: a device scalar)."""
    L = _l.load()
    n = len(weights)
    ws = (ctypes.c_float * n)(*[float(w) for w in weights])
    g = _new(g_out, n)
    _l.check(L.oi_weighted_sum_bwd(_p(g_out), ws, n, _p(g), _stream()), "oi_weighted_sum_bwd")
    return g


def gan_losses_bwd(g_total, d_real, d_fake, pose, gx, aux_w, reg_w, want_real, want_fake, want_gx, out=None):
    """out: optional (g_real, g_fake, g_gx) destinations (contiguous; e.g. slices of one tensor)."""
    L = _l.load()
    B, K, N = _gan_shapes(d_real, d_fake, pose, gx, aux_w)
    if out is not None:
        g_real, g_fake, g_gx = out
    else:
        g_real = _new(d_real, *d_real.shape) if want_real else None
        g_fake = _new(d_fake, *d_fake.shape) if want_fake else None
        g_gx = _new(gx, *gx.shape) if want_gx else None
    _l.check(L.oi_gan_losses_bwd(_p(g_total), _p(d_real), _p(d_fake), _p(pose), _p(gx), _p(aux_w), float(reg_w), _p(g_real),
                                 _p(g_fake), _p(g_gx), B, K, N, _stream()), "oi_gan_losses_bwd")
    return g_real, g_fake, g_gx


def channel_sum(g):
    L = _l.load()
    g = _c(g)
    B, C = g.shape[:2]
    gb = _new(g, C)
    _l.check(L.oi_channel_sum(_p(g), _p(gb), B, C, g[0, 0].numel(), _stream()), "oi_channel_sum")
    return gb


def upfirdn2d(x, f, upx=1, upy=1, downx=1, downy=1, padx0=0, padx1=0, pady0=0, pady1=0, flip=False, gain=1.0):
    """Same contract as the reference plugin op (f is 2-D [fh, fw])."""
    L = _l.load()
    x, f = _c(x), _c(f)
    B, C, H, W = x.shape
    fh, fw = f.shape
    Wo = (W * upx + padx0 + padx1 - fw + downx) // downx
    Ho = (H * upy + pady0 + pady1 - fh + downy) // downy
    y = _new(x, B, C, Ho, Wo)
    _l.check(L.oi_upfirdn2d(_p(x), _p(f), _p(y), B * C, H, W, fh, fw, upx, upy, downx, downy, padx0, padx1, pady0,
                            pady1, int(bool(flip)), float(gain), _stream()), "oi_upfirdn2d")
    return y


_DISC_TICKETS = {}
# the batch <= 4 forward's C entries by the number of blocks (4: the 64 x 64 network | 5: the shipped 128 x 128 one, whose entries
# fix the image size): (forward, workspace floats, plan creation, H and W passed)
_DISC_SMALL = {4: ("oi_disc_fwd_small", "oi_disc_fwd_small_workspace_floats", "oi_disc_graph_create", True),
               5: ("oi_disc_fwd_small128", "oi_disc_fwd_small128_workspace_floats", "oi_disc_graph_create128", False)}


def disc_fwd_small(x, weights, whead, bhead, f12=None, theta_np=None, theta_dev=None, margins=(0, 0, 0, 0), slope=0.2):
    """DCDiscriminator(img_size 64, n_feat 512) forward at batch <= 4 in four / five launches (oi_disc_fwd_small): optional ADA
    geometry (theta_np: (B, 2, 3) numpy, passed by value | theta_dev: device tensor; margins (mx0, my0, mx1, my1) as
    AugmentPipe.margins_for returns them) + four conv blocks + head.  -> logits (B, out_dim)."""
    L = _l.load()
    x = _c(x)
    B, C, H, W = x.shape
    mx0, my0, mx1, my1 = (int(v) for v in margins)
    fwd, wsf, _, hw = _DISC_SMALL[len(weights)]
    assert hw or (H, W) == (128, 128)
    ws = torch.empty(getattr(L, wsf)(B, C, mx0, mx1, my0, my1), dtype=torch.float32, device=x.device)
    key = (x.device, _stream().value or 0)
    ticket = _DISC_TICKETS.get(key)
    if ticket is None:
        if torch.cuda.is_current_stream_capturing():
            # the zero fill would become a node of the caller's graph (and the memory part of its private pool): eager calls on
            # this stream would then reuse counters that were never cleared.  Warm the entry point up before capturing.
            raise _l.OiHipError("oi_disc_fwd_small: first call on this stream is inside a stream capture; call it once eagerly "
                                "(warm-up) before capturing")
        ticket = _DISC_TICKETS[key] = torch.zeros(_l.TICKET_WORDS, dtype=torch.int32, device=x.device)
    out_dim = whead.shape[0]
    logits = _new(x, B, out_dim)
    th_host = th_arr = None
    if theta_np is not None:
        th_arr = np.ascontiguousarray(theta_np, dtype=np.float32).reshape(-1)   # alive during the call: the C side copies the
        assert th_arr.size == 6 * B                                             # values into the kernel arguments
        th_host = th_arr.ctypes.data_as(ctypes.c_void_p)
    ws_ = [_c(w) for w in weights]
    _l.check(getattr(L, fwd)(_p(x), th_host, _p(_c(theta_dev)), _p(_c(f12)) if f12 is not None else _p(x), mx0, mx1, my0, my1,
                             *[_p(w) for w in ws_], _p(_c(whead)), _p(_c(bhead)), _p(ws), _vp(ticket.data_ptr()), _p(logits),
                             B, C, *((H, W) if hw else ()), int(ws_[-1].shape[0]), int(out_dim), float(slope), _stream()), fwd)
    return logits


class DiscLargePack:
    """Packed weights of the batch >= 16 no-grad discriminator forward (oi_disc_large_*, csrc/disc_large.hip).  `ok` is False when
    the network is not covered (the caller keeps the general chain)."""

    def __init__(self, weights, whead):
        L = _l.load()
        self.chans = [int(weights[0].shape[1])] + [int(w.shape[0]) for w in weights]
        self.nb, self.out_dim = len(weights), int(whead.shape[0])
        self.c_chans = (ctypes.c_int * len(self.chans))(*self.chans)
        n = int(L.oi_disc_large_packed_bytes(self.c_chans, self.nb, self.out_dim))
        self.ok = n > 0 and all(w.dtype == torch.float32 and w.is_contiguous() and w.is_cuda for w in list(weights) + [whead])
        if not self.ok:
            return
        self.packed = torch.empty(n, dtype=torch.uint8, device=weights[0].device)
        ptrs = (ctypes.c_void_p * self.nb)(*[w.data_ptr() for w in weights])
        _l.check(L.oi_disc_large_pack(ptrs, _p(whead), self.c_chans, self.nb, self.out_dim, _p(self.packed), _stream()),
                 "oi_disc_large_pack")
        self._ws = {}

    def workspace(self, B, H, device):
        key = (B, H, _stream().value or 0)
        ws = self._ws.get(key)
        if ws is None:
            n = int(_l.load().oi_disc_large_workspace_bytes(self.c_chans, self.nb, self.out_dim, B, H))
            if n == 0:
                return None
            if len(self._ws) >= 4:
                self._ws.clear()
            ws = self._ws[key] = torch.empty(n, dtype=torch.uint8, device=device)
        return ws


def disc_fwd_large(x, pack, w1, bhead, slope=0.2):
    """-> logits (B, out_dim), or None when the (shape, network) pair is not covered."""
    x = _c(x)
    B, C, H, W = x.shape
    if not pack.ok or H != W or C != pack.chans[0]:
        return None
    ws = pack.workspace(B, H, x.device)
    if ws is None:
        return None
    logits = _new(x, B, pack.out_dim)
    _l.check(_l.load().oi_disc_fwd_large(_p(x), _p(w1), _p(pack.packed), _p(_c(bhead)), _p(ws), ws.numel(), _p(logits), pack.c_chans,
                                         pack.nb, pack.out_dim, B, H, float(slope), _stream()), "oi_disc_fwd_large")
    return logits


class DiscGraph:
    """oi_disc_graph_*: the batch <= 4 discriminator forward as a plan owned by the library -- every argument but the image pointer
    and the sampling matrices is fixed at creation; a call passes those two and costs one short ctypes call.  `launch`:
    "eager" (default; OI_DISC_LAUNCH): the four launches issued one by one from the stored arguments | "graph": a hipGraph
    replay whose first nodes get the image pointer and the matrices as updated kernel-node parameters (no staging launch
    either way).  Measured at batch 1: 31.7 us per image eager, 36.6 us replayed -- a graph launch costs ~5 us of GPU time
    between two replays on this runtime, back-to-back eager launches have no gap, and the host needs ~16 us for them.
    `margins`: the STATIC ones (AugmentPipe.static_margins) or None for no augmentation.  The returned logits tensor is
    overwritten by the next call."""

    def __init__(self, shape, device, weights, whead, bhead, f12=None, margins=None, slope=0.2, launch=None):
        L = _l.load()
        B, C, H, W = shape
        if torch.cuda.is_current_stream_capturing():
            raise _l.OiHipError("ops.DiscGraph: created inside a stream capture (its arrival counters are zeroed at creation: the "
                                "fill must run, not be recorded); create the plan before capturing")
        self.shape, self.aug = (B, C, H, W), margins is not None
        launch = launch or os.environ.get("OI_DISC_LAUNCH", "eager")
        assert launch in ("eager", "graph"), launch
        self.eager = launch == "eager"
        mx0, my0, mx1, my1 = (int(v) for v in margins) if self.aug else (0, 0, 0, 0)
        nb = len(weights)
        _, wsf, create, hw = _DISC_SMALL[nb]
        self.big = not hw   # the shipped 128 x 128 / five-block network: launch by launch only
        if self.big and launch != "eager":
            raise _l.OiHipError("ops.DiscGraph: the 128 x 128 plan is launched launch by launch (launch='eager')")
        assert hw or (H, W) == (128, 128)
        self.ws = torch.empty(getattr(L, wsf)(B, C, mx0, mx1, my0, my1), dtype=torch.float32, device=device)
        self.ticket = torch.zeros(_l.TICKET_WORDS, dtype=torch.int32, device=device)   # this graph's own
        self.logits = torch.empty(B, whead.shape[0], dtype=torch.float32, device=device)
        # (the graph holds raw pointers: keep the tensors it was built from alive)
        self.keep = [_c(w) for w in weights] + [_c(whead), _c(bhead), _c(f12) if f12 is not None else None]
        self.handle = ctypes.c_void_p()
        _l.check(getattr(L, create)(ctypes.byref(self.handle), int(self.aug), _p(self.keep[nb + 2]), mx0, mx1, my0, my1,
                                    *[_p(w) for w in self.keep[:nb + 2]], _p(self.ws), _vp(self.ticket.data_ptr()), _p(self.logits),
                                    B, C, *((H, W) if hw else ()), int(self.keep[nb - 1].shape[0]), int(whead.shape[0]),
                                    float(slope)), create)

    def __call__(self, x, theta_np=None, fresh=False):
        """`fresh` (eager launches only): the result goes to a new tensor instead of the plan's own buffer."""
        assert tuple(x.shape) == self.shape and (theta_np is not None) == self.aug
        x = _c(x)
        th = None
        if self.aug:
            th_arr = np.ascontiguousarray(theta_np, dtype=np.float32).reshape(-1)   # (alive during the call: copied by value)
            assert th_arr.size == 6 * self.shape[0]
            th = th_arr.ctypes.data_as(ctypes.c_void_p)
        L = _l.load()
        if self.eager:
            out = torch.empty_like(self.logits) if fresh else self.logits
            _l.check(L.oi_disc_graph_launch_eager(self.handle, _p(x), th, _p(out), _stream()), "oi_disc_graph_launch_eager")
            return out
        assert not fresh, "a graph replay writes the buffer it was captured with"
        _l.check(L.oi_disc_graph_launch(self.handle, _p(x), th, _stream()), "oi_disc_graph_launch")
        return self.logits

    def call_ada(self, x, seed, p_xint, xint_max, p_scale, scale_std, fresh=False):
        """The forward with AugmentPipe's xint + scale draws made INSIDE the library from one 64-bit seed
        (oi_disc_graph_launch_ada): no numpy, no matrix algebra and no array marshalling on the way.  `x` must already be a
        contiguous fp32 CUDA tensor of the plan's shape (the caller's guard)."""
        L = _l.load()
        if self.eager:
            out = torch.empty_like(self.logits) if fresh else self.logits
            rc = L.oi_disc_graph_launch_ada(self.handle, x.data_ptr(), seed, p_xint, xint_max, p_scale, scale_std, out.data_ptr(), 1,
                                            _stream())
        else:
            out = self.logits
            rc = L.oi_disc_graph_launch_ada(self.handle, x.data_ptr(), seed, p_xint, xint_max, p_scale, scale_std, None, 0, _stream())
        if rc != 0:
            _l.check(rc, "oi_disc_graph_launch_ada")
        return out

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                _l.load().oi_disc_graph_destroy(h)
            except Exception:
                pass


def ada_theta_xint_scale(seed, B, H, W, margins, p_xint, xint_max, p_scale, scale_std, with_draws=False):
    """(B, 2, 3) float32 numpy: the sampling matrices the library forms from `seed` (oi_ada_theta_xint_scale; host only, no HIP
    call) -- what DiscGraph.call_ada uses for the same seed.  with_draws: also (B, 3) = (t_x, t_y, s) as drawn."""
    th = np.empty((B, 2, 3), np.float32)
    ts = np.empty((B, 3), np.float32) if with_draws else None
    mx0, my0, mx1, my1 = (int(v) for v in margins)
    _l.check(_l.load().oi_ada_theta_xint_scale(int(seed), B, H, W, mx0, mx1, my0, my1, p_xint, xint_max, p_scale, scale_std,
                                               th.ctypes.data_as(_vp), None if ts is None else ts.ctypes.data_as(_vp)),
             "oi_ada_theta_xint_scale")
    return (th, ts) if with_draws else th


ADA_SEPARABLE = os.environ.get("OI_ADA_SEP", "1") != "0"   # axis-aligned matrices: the one-launch form (oi_ada_geom_sep_fwd)


def ada_geom_sep_ok(x):
    """The one-launch separable augmentation covers this image batch (1..3 channels of 64 x 64, fp32, on the GPU)."""
    return (ADA_SEPARABLE and x.is_cuda and x.dim() == 4 and x.dtype is torch.float32 and x.shape[0] <= 65535
            and bool(_l.load().oi_ada_geom_sep_supported(x.shape[1], x.shape[2], x.shape[3])))


def ada_geom_sep_host(x, theta_np, f12, margins):
    """oi_ada_geom_sep_fwd with AXIS-ALIGNED sampling matrices that live on the host ((B, 2, 3) float32 numpy: they travel in the
    kernel arguments, nothing is uploaded).  No gradient."""
    x, f12 = _c(x), _c(f12)
    B, C, H, W = x.shape
    mx0, my0, mx1, my1 = margins
    th = np.ascontiguousarray(theta_np, np.float32)
    assert th.shape == (B, 2, 3) and f12.numel() == 12
    if np.any(th[:, 0, 1] != 0) or np.any(th[:, 1, 0] != 0):   # (the kernel does not read them: it would silently drop a rotation)
        raise ValueError("ada_geom_sep_host: a sampling matrix with off-diagonal entries (rotation) -- use ada_geom_fwd")
    y = _new(x, *x.shape)
    _l.check(_l.load().oi_ada_geom_sep_fwd(_p(x), None, th.ctypes.data_as(_vp), _p(f12), _p(y), B, C, H, W, mx0, mx1, my0, my1,
                                           _stream()), "oi_ada_geom_sep_fwd")
    return y


def ada_geom_adj_sep(gy, theta, f12, margins):
    """A^T gy for AXIS-ALIGNED device matrices in one launch (oi_ada_geom_sep_adj); the caller checked ada_geom_sep_ok(gy)."""
    gy, theta, f12 = _c(gy), _c(theta), _c(f12)
    B, C, H, W = gy.shape
    mx0, my0, mx1, my1 = margins
    gx = _new(gy, *gy.shape)
    _l.check(_l.load().oi_ada_geom_sep_adj(_p(gy), _p(theta), None, _p(f12), _p(gx), B, C, H, W, mx0, mx1, my0, my1, _stream()),
             "oi_ada_geom_sep_adj")
    return gx


def ada_geom_fwd(x, theta, f12, margins, axis_aligned=False):
    """reflect pad + x2 up-FIR + affine resample + /2 down-FIR (AugmentPipe geometry); see oi_ada_geom_fwd (two launches) and
    oi_ada_geom_sep_fwd (one: `axis_aligned` is the caller's promise that no theta carries a rotation)."""
    L = _l.load()
    x, theta, f12 = _c(x), _c(theta), _c(f12)
    B, C, H, W = x.shape
    mx0, my0, mx1, my1 = margins
    assert f12.numel() == 12 and theta.shape == (B, 2, 3)
    y = _new(x, *x.shape)
    if axis_aligned and ADA_SEPARABLE and B <= 65535 and L.oi_ada_geom_sep_supported(C, H, W):
        _l.check(L.oi_ada_geom_sep_fwd(_p(x), _p(theta), None, _p(f12), _p(y), B, C, H, W, mx0, mx1, my0, my1, _stream()),
                 "oi_ada_geom_sep_fwd")
        return y
    canvas = _new(x, B * C * 2 * (H + my0 + my1) * 2 * (W + mx0 + mx1))
    _l.check(L.oi_ada_geom_fwd(_p(x), _p(theta), _p(f12), _p(y), _p(canvas), B, C, H, W, mx0, mx1, my0, my1, _stream()),
             "oi_ada_geom_fwd")
    return y


def affine_grid_sample_fwd(x, theta, Ho, Wo):
    L = _l.load()
    x, theta = _c(x), _c(theta)
    B, C, Hi, Wi = x.shape
    y = _new(x, B, C, Ho, Wo)
    _l.check(L.oi_affine_grid_sample_fwd(_p(x), _p(theta), _p(y), B, C, Hi, Wi, Ho, Wo, _stream()),
             "oi_affine_grid_sample_fwd")
    return y


def affine_grid_sample_bwd(gy, theta, Hi, Wi):
    L = _l.load()
    gy, theta = _c(gy), _c(theta)
    B, C, Ho, Wo = gy.shape
    gx = _new_acc(gy, B, C, Hi, Wi)
    _l.check(L.oi_affine_grid_sample_bwd(_p(gy), _p(theta), _p(gx), B, C, Hi, Wi, Ho, Wo, _stream()),
             "oi_affine_grid_sample_bwd")
    return gx


def reflect_pad_fwd(x, px0, px1, py0, py1):
    L = _l.load()
    x = _c(x)
    B, C, H, W = x.shape
    y = _new(x, B, C, H + py0 + py1, W + px0 + px1)
    _l.check(L.oi_reflect_pad_fwd(_p(x), _p(y), B * C, H, W, px0, px1, py0, py1, _stream()), "oi_reflect_pad_fwd")
    return y


def reflect_pad_bwd(gy, H, W, px0, px1, py0, py1):
    L = _l.load()
    gy = _c(gy)
    B, C = gy.shape[:2]
    gx = _new_acc(gy, B, C, H, W)
    _l.check(L.oi_reflect_pad_bwd(_p(gy), _p(gx), B * C, H, W, px0, px1, py0, py1, _stream()), "oi_reflect_pad_bwd")
    return gx
