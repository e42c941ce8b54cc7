"""fp64 torch restatement of oi_relight_fwd (include/oi_relight.h): the Phong shading and compositing of
oi_oracle.render_maps (generator.py:80-174; lighting.py:126-225) with the ambient, diffuse and specular colours widened to
RGB, evaluated for L lights on captured per-sample tensors."""
import torch


def _normalize(v, eps=1e-6):
    """F.normalize(v, dim=-1, eps): v / max(|v|, eps)."""
    return v / v.norm(dim=-1, keepdim=True).clamp(min=eps)


def relight_ref(weights, grad, rgb, mid_z, rays_o, rays_d, w2b, lights, bg, B):
    """weights / mid_z (N, T), grad / rgb (N, T, 3), rays_o / rays_d (N, 3), w2b (B, 4, 4), lights (L, 16) packed as
    oi_amd.relight.Light.packed, bg (B, 3) or None.  -> {image, image_no_bg, shading, diffuse, specular}: (L, B, 3, N / B)
    float64 on the inputs' device."""
    f = lambda t: t.detach().double()
    w, g, alb, mz, ro, rd, w2b, lt = (f(t) for t in (weights, grad, rgb, mid_z, rays_o, rays_d, w2b, lights))
    N, T = w.shape
    hw = N // B
    d = lt[:, 0:3] / lt[:, 0:3].norm(dim=-1, keepdim=True)                      # (L, 3) world frame
    ldir = _normalize(torch.einsum("bij,lj->lbi", w2b[:, :3, :3], d))           # (L, B, 3) box frame of each element
    l = ldir.repeat_interleave(hw, dim=1)[:, :, None, :]                        # (L, N, 1, 3)
    ca, cd, cs, sh = lt[:, 4:7], lt[:, 8:11], lt[:, 12:15], lt[:, 15]
    n = _normalize(g)[None]                                                     # (1, N, T, 3)
    pts = ro[:, None, :] + rd[:, None, :] * mz[..., None]
    v = _normalize(ro[:, None, :] - pts)[None]
    ndl = (n * l).sum(-1, keepdim=True)                                         # (L, N, T, 1)
    diff = cd[:, None, None, :] * torch.relu(ndl)                               # (L, N, T, 3)
    refl = -l + 2.0 * ndl * n
    al = torch.relu((v * refl).sum(-1, keepdim=True)) * (ndl > 0).double()
    spec = cs[:, None, None, :] * torch.pow(al, sh[:, None, None, None])
    shade = ca[:, None, None, :] + diff
    wt = w[None, :, :, None]

    def wsum(x):   # (L, N, T, 3) -> (L, B, 3, N / B)
        return (x * wt).sum(2).view(-1, B, hw, 3).permute(0, 1, 3, 2)

    image_no_bg = wsum(shade * alb[None] + spec)
    wsm = w.sum(1).view(B, 1, hw)
    image = image_no_bg if bg is None else image_no_bg + f(bg)[:, :, None] * (1.0 - wsm)
    return {"image": image, "image_no_bg": image_no_bg, "shading": wsum(shade), "diffuse": wsum(diff),
            "specular": wsum(spec)}
