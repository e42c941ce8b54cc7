"""Importance resampling (csrc/render.hip upsample_kernel / oi_upsample_mid / merge_sorted_kernel) in the regimes a trained
field reaches.  All plain torch on the CPU:

* `restate`: one up-sampling step (section weights, inverse CDF, merge) as ONE function of (rays, z, sdf, n_new, inv_s),
  spelled out from the oracle's O.up_sample_weights / O.sample_pdf_det / O.merge_sorted so that every deciding quantity is
  returned and every branch can be mutated.  Unmutated it is bit-identical to those three calls in float64 and float32
  (tests/test_upsample_regimes_cpu.py::test_restatement_is_the_oracle).  float64 is the reference, float32 the reference's
  own arithmetic noise (the "fp32 floor").
* `REGIMES` / `case`: named, seeded chains on an analytic field that is positive outside with the gradient outwards (the
  sphere of radius 0.6 of tests/helpers/composite_regimes.py; `unit_sphere` moves the body to radius 0.985, `uniform` has no
  surface).  A chain is coarse z (O.coarse_z with training jitter) and K steps at inv_s = 64 * 2**i.  Every step's inputs
  are the FLOAT32 reference chain's (z, sdf): a step is tested on its own and cannot drift.
* `decided`, `judge`, `FP32_FLOOR`, `bar`: which samples have a defined value, the assertions the GPU test makes on a
  candidate (z_new, z_merged), the committed floors and the bar that follows from them.

What the arithmetic allows, and what the regimes do about it
------------------------------------------------------------
The flat branch (`den < 1e-5`).  pdf_i = (w_i + 1e-5) / (W + nsec 1e-5) < 1e-5 needs w_i < 1e-5 (W - 1 + nsec 1e-5): the ray
must be opaque to within nsec 1e-5 and the section must carry w_i < ~1e-8.  In front of a surface alpha >= 1e-5 / (1 + 1e-5)
and T = 1, so w_i ~ 1e-5: never flat.  Flat sections therefore lie BEHIND an (almost) opaque surface, each holds just under
1e-5 of the CDF, and the last sample sits at u = 1 - 0.5 / n_new: a sample lands in one only if n_flat x 1e-5 > 0.5 / n_new,
i.e. n_flat x n_new > 5e4.  At the shapes the renderer ships (n_new <= 32, Sc <= 224) the branch is unreachable, which is
why 5,000 random samples never met it.  Between two surfaces the sections are flat only if the transmittance left by the
first one is below nsec 1e-5 - (1 - W); with T > 1e-3 in front that needs nsec > 100 AND the first surface's CDF mass tuned
into a window 1e-3 wide that also has to contain a u: no sorted input at the suite's sizes does both.  `flat` is the
nearest input that reaches the branch: one opaque body, Sc = 400, n_new = 256 (n_flat ~ 250-330 behind the surface, one
sample per hitting ray ~60 sections deep in the flat stretch).  The transmittance in front of those sections is ~0; nothing
with T > 1e-3 can be flat at this size.  This is a stated deviation from the regime table.
And float32 cannot DECIDE the branch there: a flat section's den is 1e-5 / (W + nsec 1e-5), 4e-8 below the threshold at
nsec = 399 (1e-7 at the kernel's limit of 1,024 samples), while the CDF entries it is the difference of are ~0.998 and
live on a grid of 6e-8.  The float32 restatement's own increments are 167 or 168 grid steps (1e-5 = 167.8): about one
flat section in ten is NOT flat in float32.  No den margin derived from that error leaves a flat sample decided, so the
population `flat` is exempt from the cap (it loses every member), the mutation `no_den` is NOT_DETECTABLE, and what the GPU
test asserts on those samples is the union of both outcomes: inside [z_below, z_above] (`judge`, kind "bracket").
A float32 flat sample is z_below + (u - c_below) (z_above - z_below) with the second term < 1e-5 x 5e-3, below half an ulp
of z: it EQUALS z_below, so `flat` is also where the chain produces ties between z_new and z.

The clamp at -1e3.  |cos| = |d sdf| / (d z + 1e-5) <= |d sdf| x 1e5: the clamp needs |d sdf| > 1e-2 across a gap that is
small against 1e-5.  Neither forward noise level (below) reaches that on a smooth field; it takes a tie in z with two
different sdf values, or noise of 1e-2.  `ties` has the former (placed on purpose: the section BEHIND a zero-length section
inherits prev_cos = d sdf / 1e-5 ~ -3e3), `steep` the latter: 3e-2 on samples closer than 1e-4 to their neighbour, which is
no forward's noise and is the nearest input that makes the clamp active where transmittance remains.

The searchsorted side only matters when u is bit-equal to a CDF knot, and then only if the lower bracket is flat (otherwise
t = 1 of one bracket and t = 0 of the next are the same z).  The running maximum only matters when float32 rounding makes
the raw inverse CDF descend (t rounds above 1 at the end of a bracket).  Both depend on the last bit of the kernel's own
CDF, whose summation order (a 64-lane tree scan) differs from torch's: no input can place them.  They are listed in
NOT_DETECTABLE; the structural assertions (monotone z_new, z_new inside [z[0], z[-1]]) hold the kernel to the contract
whenever such an event does occur.  The + 1e-7 in the transmittance, expected to be invisible, is not: see CAUGHT_BY.

Noise levels: the fp32-class f16x3 forward is 1e-5 from the oracle, the bf16 forward 1e-3
(worst 1.08e-3, median 2e-4).  `noisy` gives even rays the first and odd rays the second; every other regime uses 1e-5.
"""
import functools
import math

import torch

import oi_oracle as O
from helpers.composite_regimes import IMPACT

RAYS_PER_WORKGROUP = 4
NOISE_F16X3, NOISE_BF16 = 1e-5, 1e-3
CLASSES = ("head_on", "grazing", "body_miss", "unit_miss")
MUTATIONS = ("ss_left", "no_den", "no_prev_cos", "inside_r0", "no_clamp", "no_w_floor", "T_reset_64", "cdf_reset_64",
             "max_reset_64", "no_T_eps")

# Impacts beyond IMPACT: rays that cross the unit sphere without meeting the body, rays that straddle radius 1, rays whose
# every point is outside radius 1 (inside == 0 throughout).
BEYOND = (0.9, 0.97, 0.995, 0.9995, 1.0005, 1.02, 1.2, 1.6)
_DEFAULT_IMPACTS = IMPACT + IMPACT[3:10] + BEYOND            # 27 rays
_HITS = (0.0, 0.1, 0.2, 0.3, 0.4, 0.45, 0.5, 0.52, 0.55, 0.57)

_D = dict(impacts=_DEFAULT_IMPACTS, body=0.6, noise="f16x3", ties=0, jitter_extremes=False)
REGIMES = {
    "chain_small": dict(_D, S=16, n_new=9, K=4, seed=201),
    "chain_64": dict(_D, S=64, n_new=16, K=4, seed=202),                     # 64 -> 80 -> 96 -> 112
    "wide": dict(_D, S=66, n_new=140, K=2, seed=203),                        # Sc - 1 = 65, then 205
    "noisy": dict(_D, S=65, n_new=65, K=2, noise="mixed", seed=204),         # Sc - 1 = 64: exactly one scan chunk
    "steep": dict(_D, S=32, n_new=16, K=6, noise="steep", seed=205),         # the last step runs at inv_s = 2048
    "ties": dict(_D, S=40, n_new=64, K=2, ties=3, seed=206),
    "flat": dict(_D, S=400, n_new=256, K=1, impacts=_HITS + IMPACT + BEYOND[2:6], seed=207),   # 26 rays
    "unit_sphere": dict(_D, S=65, n_new=16, K=2, body=0.985, jitter_extremes=True,
                        impacts=tuple(b for b in (0.0, 0.1, 0.2, 0.3, 0.4, 0.5) for _ in range(3))
                        + (0.9, 0.97, 0.98, 0.99, 0.995, 0.999) + BEYOND[3:], seed=208),   # 29 rays
    "uniform": dict(_D, S=30, n_new=16, K=2, body=None, seed=209),
}

# Floors of the margins a sample keeps from the reference's discrete choices.  A float32 evaluation is off by ~1.5e-7 in a
# radius (|p| <= 1.7; tests/helpers/composite_regimes.py measures 1.4e-7 for pts_norm), so 1e-6 is > 3x that.  In the CDF the
# float32 error is 1e-7 on head-on and missing rays and up to ~1e-4 on grazing ones (the weights are ill-conditioned there),
# so no constant fits: a sample's knot margin is 3x the float32 restatement's worst CDF error ON ITS OWN RAY (the worst of
# its (regime, step, ray class) cell would be steadier, but one ill-conditioned grazing ray then removes a third of the
# samples of every grazing ray and no seed of `chain_small` keeps the 2 % cap), floored at
# 5e-7 (3x the 1.5e-7 a well-conditioned ray shows); den = c_above - c_below is a difference of two CDF entries, each rounded
# to the float32 grid (6e-8 near 1): its margin is 3x the ray's worst float32 error in such a difference, floored at 2e-7 (three grid steps).  cos / prev_cos / the clamp are CONTINUOUS kinks (min and clamp): a float32
# evaluation that takes the other side of one moves c by no more than its own rounding error, which the fp32 floor already
# contains -- swapping them can never move alpha by more than the bar, so they keep no margin (cos = 0 and cos = prev_cos
# exactly are plentiful).  `inside` is the one discontinuous choice in alpha: a ray whose section has a radius within the
# margin of 1 leaves as a whole where the other choice moves a weight by more than ALPHA_SWAP = 1e-7 (the float32 floor of a
# weight).  tests/test_upsample_regimes_cpu.py::test_margins_cover_the_fp32_error checks the measured errors against these.
MARGIN = {"knot": 5e-7, "den": 2e-7, "radius": 1e-6}
ALPHA_SWAP = 1e-7
CAP_UNDECIDED, CAP_POPULATION = 0.02, 0.25
T_FELT = 1e-3    # "not opaque before the branch"


def ulp32(x):
    """Spacing of float32 at |x| (x: any float tensor)."""
    _, e = torch.frexp(x.detach().double().abs().clamp(min=1e-30))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 24)


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _excl_cumprod(om):
    return torch.cumprod(torch.cat([torch.ones_like(om[:, :1]), om], -1), -1)[:, :-1]   # as O.transmittance_weights


def running_max(z_raw, reset_at=None):
    """The kernel's contract for z_new: the running maximum of the raw inverse CDF (the reference sorts afterwards; in exact
    arithmetic the raw values ascend already).  reset_at=64: a maximum that forgets what the first 64 samples reached."""
    if reset_at is None or z_raw.shape[1] <= reset_at:
        return torch.cummax(z_raw, -1).values
    return torch.cat([torch.cummax(z_raw[:, :reset_at], -1).values, torch.cummax(z_raw[:, reset_at:], -1).values], -1)


def restate(ro, rd, z, sdf, n_new, inv_s, dtype, mutate=None):
    """One up-sampling step in `dtype` -> dict.  Per section (N, Sc - 1): r0, r1, inside, cos, prev_cos, c (what enters
    alpha), alpha, T (transmittance in front), w5 (= w + 1e-5), pdf; cdf (N, Sc); per new sample (N, n_new): u, below, above
    (indices into z), z_below, z_above, den (before the 1e-5 escape), z_raw (O.sample_pdf_det's value), z_new (its running
    maximum); z_merged (N, Sc + n_new); W (N,) = sum of w.  `mutate`: one name of MUTATIONS, a deliberately WRONG step."""
    assert mutate is None or mutate in MUTATIONS, mutate
    ro, rd, z, sdf = (t.to(dtype) for t in (ro, rd, z, sdf))
    N, Sc = z.shape
    nsec = Sc - 1
    pts = ro[:, None, :] + rd[:, None, :] * z[..., None]
    radius = torch.linalg.norm(pts, dim=-1)
    r0, r1 = radius[:, :-1], radius[:, 1:]
    inside = (r0 < 1.0) if mutate == "inside_r0" else ((r0 < 1.0) | (r1 < 1.0))
    ps, ns = sdf[:, :-1], sdf[:, 1:]
    pz, nz = z[:, :-1], z[:, 1:]
    cos = (ns - ps) / (nz - pz + 1e-5)
    prev_cos = torch.cat([torch.zeros_like(cos[:, :1]), cos[:, :-1]], -1)
    c = cos if mutate == "no_prev_cos" else torch.minimum(prev_cos, cos)
    c_raw = c.clamp(max=0.0) if mutate == "no_clamp" else c.clamp(-1e3, 0.0)
    c = c_raw * inside
    alpha = O.section_alpha(ps, ns, c, nz - pz, inv_s)
    om = 1.0 - alpha if mutate == "no_T_eps" else 1.0 - alpha + 1e-7
    T = _excl_cumprod(om)
    if mutate == "T_reset_64" and nsec > 64:
        T = torch.cat([T[:, :64], _excl_cumprod(om[:, 64:])], -1)
    w = alpha * T
    w5 = w if mutate == "no_w_floor" else w + 1e-5
    pdf = w5 / w5.sum(-1, keepdim=True)
    cs = torch.cumsum(pdf, -1)
    if mutate == "cdf_reset_64" and nsec > 64:
        cs = torch.cat([cs[:, :64], torch.cumsum(pdf[:, 64:], -1)], -1)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), cs], -1)
    u = torch.linspace(0.5 / n_new, 1.0 - 0.5 / n_new, n_new, dtype=dtype).expand(N, n_new).contiguous()
    ind = torch.searchsorted(cdf, u, right=mutate != "ss_left")
    below = (ind - 1).clamp(min=0)
    above = ind.clamp(max=Sc - 1)
    c0, c1 = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(z, 1, below), torch.gather(z, 1, above)
    den = c1 - c0
    den_used = den if mutate == "no_den" else torch.where(den < 1e-5, torch.ones_like(den), den)
    z_raw = b0 + (u - c0) / den_used * (b1 - b0)
    z_new = running_max(z_raw, 64 if mutate == "max_reset_64" else None)
    z_merged, _ = O.merge_sorted(z, z_new)
    return {"r0": r0, "r1": r1, "inside": inside, "cos": cos, "prev_cos": prev_cos, "c": c, "c_raw": c_raw, "alpha": alpha, "T": T, "w5": w5,
            "pdf": pdf, "cdf": cdf, "u": u, "below": below, "above": above, "z_below": b0, "z_above": b1, "c_below": c0,
            "c_above": c1, "den": den, "z_raw": z_raw, "z_new": z_new, "z_merged": z_merged, "W": w.sum(-1)}


# ----------------------------------------------------------------------------------------------------------------------
# the chains
# ----------------------------------------------------------------------------------------------------------------------
def _rays(impacts, g):
    n = len(impacts)
    b = torch.tensor(impacts, dtype=torch.float64)
    phi = 2 * math.pi * torch.rand(n, generator=g, dtype=torch.float64)
    Q = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64)).Q
    o_loc = torch.stack([b * torch.cos(phi), b * torch.sin(phi), torch.full_like(b, -3.0)], -1)
    return torch.einsum("nij,nj->ni", Q, o_loc).float(), Q[:, :, 2].float()


def _field(spec, ro, rd, z, g, z_old=None):
    """sdf (float32) of the regime's analytic field at ro + rd z, plus its noise."""
    r = torch.linalg.norm(ro.double()[:, None] + rd.double()[:, None] * z.double()[..., None], dim=-1)
    f = r + 0.5 if spec["body"] is None else r - spec["body"]
    e = torch.randn(z.shape, generator=g, dtype=torch.float64)
    if spec["noise"] == "mixed":
        amp = torch.where(torch.arange(z.shape[0]) % 2 == 0, NOISE_F16X3, NOISE_BF16)[:, None].double()
    elif spec["noise"] == "steep":
        # 3e-2 on samples closer than 1e-4 to a neighbour (of the list they join, or of their own)
        zz = z.double()
        gap = torch.full_like(zz, 1.0)
        if zz.shape[1] > 1:
            d = zz[:, 1:] - zz[:, :-1]
            gap[:, 1:] = torch.minimum(gap[:, 1:], d.abs())
            gap[:, :-1] = torch.minimum(gap[:, :-1], d.abs())
        if z_old is not None:
            gap = torch.minimum(gap, (zz[:, :, None] - z_old.double()[:, None, :]).abs().min(-1).values)
        amp = torch.where(gap < 1e-4, 3e-2, NOISE_F16X3)
    else:
        amp = NOISE_F16X3
    return (f + amp * e).float()


def ray_classes(impacts, W):
    """(N,) long index into CLASSES, from the impact and the float64 reference's weight sum of this step."""
    b = torch.tensor(impacts, dtype=torch.float64)
    cls = torch.full((len(impacts),), CLASSES.index("grazing"))
    cls[W > 1 - 1e-2] = CLASSES.index("head_on")
    cls[W < 1e-2] = CLASSES.index("body_miss")
    cls[b >= 1.0] = CLASSES.index("unit_miss")
    return cls


def decided(r64, r32):
    """-> (decided, knot_ok), (N, n_new) bool each: the samples whose value is defined, i.e. where the float64 reference's
    discrete choices are stable under float32 noise (see MARGIN), and those that keep the knot margin alone."""
    e_cdf = (r32["cdf"].double() - r64["cdf"]).abs().max(-1).values            # (N,)
    inc = lambda r: (r["cdf"][:, 1:] - r["cdf"][:, :-1]).double()
    e_den = (inc(r32) - inc(r64)).abs().max(-1).values
    knot = torch.maximum(torch.full_like(e_cdf, MARGIN["knot"]), 3 * e_cdf)[:, None]
    denm = torch.maximum(torch.full_like(e_den, MARGIN["den"]), 3 * e_den)[:, None]
    knot_ok = (r64["u"] - r64["c_below"] >= knot) & (r64["c_above"] - r64["u"] >= knot)
    ok = knot_ok.clone()
    ok &= (r64["den"] - 1e-5).abs() >= denm
    # the radius of the sample's own section
    near1 = ((r64["r0"] - 1.0).abs() < MARGIN["radius"]) | ((r64["r1"] - 1.0).abs() < MARGIN["radius"])
    sec = r64["below"].clamp(max=near1.shape[1] - 1)
    ok &= ~torch.gather(near1, 1, sec)
    # swap test, per ray: a section whose radius is within its margin of 1 AND whose other choice of `inside` moves a weight
    if bool(near1.any()):
        a_alt = r64["_alpha_of"](torch.where(near1, r64["c_raw"] * (~r64["inside"]), r64["c"]))
        moved = (a_alt - r64["alpha"]).abs() * r64["T"] > ALPHA_SWAP
        ok &= ~(near1 & moved).any(-1)[:, None]
    return ok, knot_ok


def _with_alpha_fn(r, z, sdf, inv_s):
    z, sdf = z.to(r["alpha"].dtype), sdf.to(r["alpha"].dtype)
    r["_alpha_of"] = lambda c: O.section_alpha(sdf[:, :-1], sdf[:, 1:], c, z[:, 1:] - z[:, :-1], inv_s)
    return r


def _place_ties(z, sdf, k, g):
    """k zero-length sections per ray: z[j + 1] := z[j], the two sdf values stay different."""
    N, Sc = z.shape
    z, sdf = z.clone(), sdf.clone()
    for r in range(N):
        for j in torch.randperm(Sc - 3, generator=g)[:k].tolist():
            z[r, j + 2] = z[r, j + 1]
    return z, sdf


def build_chain(name, seed):
    spec = REGIMES[name]
    g = torch.Generator().manual_seed(seed)
    impacts = spec["impacts"]
    N, S, n_new, K = len(impacts), spec["S"], spec["n_new"], spec["K"]
    ro, rd = _rays(impacts, g)
    near, far = O.near_far_from_sphere(ro, rd)
    jitter = torch.rand(N, 1, generator=g)
    if spec["jitter_extremes"]:
        jitter[0::3] = 0.0                       # z[0] = near - 1 / S: outside [near, far]
        jitter[1::3] = 1.0 - 2.0 ** -24          # z[-1] = far + 1 / S
    z = O.coarse_z(near, far, S, jitter).contiguous()
    sdf = _field(spec, ro, rd, z, g)
    steps = []
    nt = torch.get_num_threads()
    torch.set_num_threads(1)   # the order of torch's sums, and with it the float32 chain, must not depend on the machine
    try:
        for i in range(K):
            inv_s = 64.0 * 2 ** i
            if spec["ties"]:
                z, sdf = _place_ties(z, sdf, spec["ties"], g)
            r32 = _with_alpha_fn(restate(ro, rd, z, sdf, n_new, inv_s, torch.float32), z, sdf, inv_s)
            r64 = _with_alpha_fn(restate(ro, rd, z, sdf, n_new, inv_s, torch.float64), z, sdf, inv_s)
            z_new = r32["z_new"]
            sdf_new = _field(spec, ro, rd, z_new, g, z_old=z)
            cls = ray_classes(impacts, r64["W"])
            dec, knot_ok = decided(r64, r32)
            steps.append({"i": i, "inv_s": inv_s, "n_new": n_new, "z": z, "sdf": sdf, "sdf_new": sdf_new, "r64": r64, "r32": r32,
                          "decided": dec, "knot_ok": knot_ok, "cls": cls})
            z, sdf = O.merge_sorted(z, z_new, sdf, sdf_new)
            z, sdf = z.contiguous(), sdf.contiguous()
    finally:
        torch.set_num_threads(nt)
    return {"name": name, "seed": seed, "ro": ro, "rd": rd, "near": near, "far": far, "jitter": jitter, "impacts": impacts,
            "steps": steps, "last_dist": 2.0 / S}


# ----------------------------------------------------------------------------------------------------------------------
# populations
# ----------------------------------------------------------------------------------------------------------------------
def populations(chain, st):
    """Numbers of sections / samples / rays of one step in the branches the regimes are named for (float64 restatement).
    `_felt`: with transmittance above T_FELT in front.  Sets of member samples for the cap are in `population_members`."""
    r, z = st["r64"], st["z"].double()
    felt = r["T"] > T_FELT
    raw = torch.minimum(r["prev_cos"], r["cos"])
    ins = r["inside"]
    nsec = z.shape[1] - 1
    near, far = chain["near"].double(), chain["far"].double()
    cnt = lambda m: int(m.sum())
    p = {"nsec": nsec, "n_new": st["n_new"], "inv_s": st["inv_s"],
         "clamp_felt": cnt((raw < -1e3) & ins & felt), "outside": cnt(~ins),
         "rays_all_outside": cnt((~ins).all(-1)),
         "straddle_enter_felt": cnt((r["r0"] >= 1) & (r["r1"] < 1) & felt & (r["alpha"] > 1e-3)),
         "straddle_leave": cnt((r["r0"] < 1) & (r["r1"] >= 1)),
         "straddle_first": cnt((r["r0"][:, 0] >= 1) & (r["r1"][:, 0] < 1)), "straddle_last": cnt((r["r0"][:, -1] < 1) & (r["r1"][:, -1] >= 1)),
         "z0_before_near": cnt(z[:, 0] < near[:, 0]), "zlast_beyond_far": cnt(z[:, -1] > far[:, 0]),
         "prev_decides_felt": cnt((r["prev_cos"] < r["cos"]) & (raw < 0) & ins & felt),
         "cos_decides_felt": cnt((r["cos"] < r["prev_cos"]) & (raw < 0) & ins & felt),
         "cos_positive_felt": cnt((raw > 0) & ins & felt),
         "ties_in_z": cnt(z[:, 1:] == z[:, :-1]),
         "ties_new_vs_z": cnt((st["r32"]["z_new"][:, :, None] == st["z"][:, None, :]).any(-1)),
         "gaps_below_1e-4": cnt((z[:, 1:] - z[:, :-1]) < 1e-4),
         "flat_samples": cnt(r["den"] < 1e-5), "flat_samples_decided": cnt((r["den"] < 1e-5) & st["decided"]),
         "alpha_floor_everywhere": cnt((r["alpha"] < 1.1e-5).all(-1)),
         "T64_window": cnt((r["T"][:, 64] > 0.1) & (r["T"][:, 64] < 0.9)) if nsec > 64 else 0,
         "undecided": 1.0 - float(st["decided"].double().mean())}
    for k, name in enumerate(CLASSES):
        p[name] = cnt(st["cls"] == k)
    # grazing rays on both sides of the body's surface
    b = torch.tensor(chain["impacts"])
    body = REGIMES[chain["name"]]["body"]
    if body is not None:
        g_ = st["cls"] == CLASSES.index("grazing")
        p["grazing_inside"], p["grazing_outside"] = cnt(g_ & (b < body)), cnt(g_ & (b >= body))
    return p


def population_members(st):
    """{population: (N, n_new) bool}: the new samples that belong to a branch population, for the cap (a population may not
    lose more than CAP_POPULATION of its members to `undecided`)."""
    r = st["r64"]
    raw = torch.minimum(r["prev_cos"], r["cos"])
    sec = r["below"].clamp(max=raw.shape[1] - 1)
    at = lambda m: torch.gather(m, 1, sec)
    felt = r["T"] > T_FELT
    return {"flat": r["den"] < 1e-5, "clamp": at((raw < -1e3) & r["inside"] & felt), "outside": at(~r["inside"]),
            "prev_decides": at((r["prev_cos"] < r["cos"]) & (raw < 0) & r["inside"] & felt),
            "cos_positive": at((raw > 0) & r["inside"] & felt),
            "zero_length": r["z_above"] == r["z_below"]}


CAP_EXEMPT = ("flat",)   # populations that may lose more than CAP_POPULATION of their members (module docstring)

# what each regime must contain: checked on EVERY step (p = populations of that step) unless the entry names steps
POPULATION = {
    "chain_small": lambda p, i: min(p["head_on"], p["body_miss"], p["unit_miss"]) >= 3 and p["grazing_inside"] >= 1 and p["grazing_outside"] >= 1,
    "chain_64": lambda p, i: min(p["head_on"], p["body_miss"], p["unit_miss"]) >= 3 and p["grazing_inside"] >= 1 and p["grazing_outside"] >= 1,
    "wide": lambda p, i: p["nsec"] > 64 and p["n_new"] > 64 and p["T64_window"] >= 2,
    "noisy": lambda p, i: p["nsec"] == 64 + 64 * i + i and min(p["cos_positive_felt"], p["prev_decides_felt"], p["cos_decides_felt"]) >= 20,
    "steep": lambda p, i: i < 3 or (p["gaps_below_1e-4"] >= 20 and p["clamp_felt"] >= 5),
    "ties": lambda p, i: p["ties_in_z"] >= 50 and p["clamp_felt"] >= 5,
    "flat": lambda p, i: p["flat_samples"] >= 8 and p["ties_new_vs_z"] >= 8,
    "unit_sphere": lambda p, i: (p["rays_all_outside"] >= 3 and (i > 0 or (p["straddle_first"] >= 1 and p["straddle_last"] >= 1))
                                 and p["straddle_enter_felt"] >= 5 and p["straddle_leave"] >= 5
                                 and p["z0_before_near"] >= 5 and p["zlast_beyond_far"] >= 5),
    "uniform": lambda p, i: p["alpha_floor_everywhere"] == len(_DEFAULT_IMPACTS) and p["head_on"] + p["grazing"] == 0,
}


@functools.lru_cache(maxsize=None)
def case(name):
    """The regime's chain, built once, shared, never modified.  The seed moves on (by 1000) until every step holds the
    regime's population and keeps the cap on undecided samples: offenders are redrawn here, nothing is masked later."""
    for attempt in range(20):
        chain = build_chain(name, REGIMES[name]["seed"] + 1000 * attempt)
        pops = [populations(chain, st) for st in chain["steps"]]
        if all(POPULATION[name](p, st["i"]) and p["undecided"] <= CAP_UNDECIDED for p, st in zip(pops, chain["steps"])):
            return chain
    raise AssertionError(f"{name}: no seed reaches the regime's population")


def cases():
    """[(regime, step)] of every step of every regime."""
    return [(n, i) for n, s in REGIMES.items() for i in range(s["K"])]


# ----------------------------------------------------------------------------------------------------------------------
# the judgement of a candidate (the kernel's output on the GPU, a mutated float32 restatement on the CPU)
# ----------------------------------------------------------------------------------------------------------------------
def cell_errors(st, z_new):
    """{class: (worst |z_new - float64 reference| over the class's decided samples, their number)}."""
    err = (z_new.double().cpu() - st["r64"]["z_raw"]).abs()
    out = {}
    for k, name in enumerate(CLASSES):
        m = st["decided"] & (st["cls"] == k)[:, None]
        out[name] = (float(err[m].max()) if bool(m.any()) else 0.0, int(m.sum()))
    return out


def bar(name, i, cls):
    """The bar of one (regime, step, ray class): 3x the committed float32 floor (tests/conftest.py: "<= 3x the native-fp32
    error"); `judge` floors it per sample at 4 ulp of z."""
    return 3.0 * FP32_FLOOR[name][i][cls]


def judge(name, i, z_new, z_merged, value_factor=1.0):
    """-> list of (kind, message) of every assertion of the GPU test that the candidate (float32 z_new (N, n_new), z_merged
    (N, Sc + n_new)) breaks: kind = "structural" / "bracket" / "value".  value_factor: the value bar is multiplied by it
    (the CPU rehearsal demands that a mutation misses the bar by a factor of 3)."""
    st = case(name)["steps"][i]
    z, r = st["z"], st["r64"]
    z_new, z_merged = z_new.detach().cpu(), z_merged.detach().cpu()
    assert z_new.dtype == torch.float32 and z_merged.dtype == torch.float32
    bad = []
    if not bool(torch.isfinite(z_new).all()):
        bad.append(("structural", "z_new is not finite"))
        return bad
    if not bool((z_new[:, 1:] >= z_new[:, :-1]).all()):
        bad.append(("structural", f"z_new descends at {int((z_new[:, 1:] < z_new[:, :-1]).sum())} places"))
    zd, z0, z1 = z_new.double(), z[:, :1].double(), z[:, -1:].double()
    out = (zd < z0 - ulp32(z0)) | (zd > z1 + ulp32(z1))
    if bool(out.any()):
        bad.append(("structural", f"{int(out.sum())} z_new outside [z[0], z[-1]] by more than an ulp"))
    if not torch.equal(z_merged, torch.sort(torch.cat([z, z_new], -1), -1).values):
        bad.append(("structural", "z_merged is not the sorted concatenation of z and z_new"))
    d = st["decided"]
    lo, hi = r["z_below"], r["z_above"]    # (float64 copies of float32 values: exact)
    off = d & ((zd < lo) | (zd > hi))
    if bool(off.any()):
        bad.append(("bracket", f"{int(off.sum())} decided samples outside the reference's section"))
    flat = d & (r["den"] < 1e-5)
    off = flat & ((zd - lo).abs() > 1e-5 * (hi - lo) + ulp32(lo))
    if bool(off.any()):
        bad.append(("bracket", f"{int(off.sum())} decided flat-branch samples further than 1e-5 of the section from z_below"))
    either = (r["den"] < 1e-5) & st["knot_ok"] & ((zd < lo) | (zd > hi))   # float32 may or may not take the flat branch
    if bool(either.any()):
        bad.append(("bracket", f"{int(either.sum())} flat-branch samples outside the reference's section"))
    err = (zd - r["z_raw"]).abs()
    for k, cls in enumerate(CLASSES):
        m = d & (st["cls"] == k)[:, None]
        if not bool(m.any()):
            continue
        b = torch.maximum(torch.full_like(err, bar(name, i, cls)), 4 * ulp32(r["z_raw"]))
        ratio = (err / b)[m]
        if float(ratio.max()) > value_factor:
            j = int(ratio.argmax())
            bad.append(("value", f"{cls}: |z_new - ref| = {float(err[m][j]):.3e} against a bar of {float(b[m][j]):.3e}"))
    return bad


def measure_floor(name):
    """{step: {class: worst |float32 restatement - float64 restatement| of z over the cell's decided samples}}."""
    return {st["i"]: {c: e for c, (e, _) in cell_errors(st, st["r32"]["z_new"]).items()} for st in case(name)["steps"]}


# Mutations no regime can expose at the bar, with the reason (see the module docstring).
NOT_DETECTABLE = {
    "no_den": "float32 cannot decide the branch: den of a flat section is 4e-8 below 1e-5, the CDF grid near 1 is 6e-8 "
              "(module docstring); every flat sample is undecided and the correct kernel may leave the branch too",
    "ss_left": "differs only where u is bit-equal to a CDF knot of the kernel's own CDF AND the bracket below is flat",
    "max_reset_64": "the running maximum only acts where float32 rounding makes the raw inverse CDF descend (<= 1 ulp), and "
                    "only a descent across new samples 63|64 would show; the kernel's rounding is not the restatement's",
}

# Which regimes catch which mutation (a mutated float32 restatement judged as the GPU output is, value bar x 3):
# tests/test_upsample_regimes_cpu.py::test_mutation_is_caught demands every entry.  no_T_eps IS caught: without the + 1e-7 the
# transmittance behind a section with alpha == 1 is exactly 0 instead of ~1e-7, which is 1 % of the 1e-5 floor of a weight.
CAUGHT_BY = {
    "no_prev_cos": ("chain_small", "chain_64", "wide", "noisy", "steep", "ties"),
    "inside_r0": ("unit_sphere",),
    "no_clamp": ("steep", "ties"),
    "no_w_floor": ("chain_small", "chain_64", "wide", "noisy", "steep", "ties", "flat"),
    "T_reset_64": ("chain_64", "wide"),
    "cdf_reset_64": ("chain_64", "wide", "noisy"),
    "no_T_eps": ("wide", "steep", "ties"),
}

# Measured by `measure_floor` (torch CPU, one thread); tests/test_upsample_regimes_cpu.py keeps a fresh measurement within
# 1.5x of these.  FP32_FLOOR[regime][step][ray class]; 0.0: the cell has no decided sample (or no ray of that class).
FP32_FLOOR = {
    "chain_small": {
        0: {"head_on": 1.951e-07, "grazing": 2.387e-07, "body_miss": 3.264e-04, "unit_miss": 2.424e-07},
        1: {"head_on": 1.181e-07, "grazing": 1.832e-07, "body_miss": 3.387e-04, "unit_miss": 1.542e-07},
        2: {"head_on": 1.211e-07, "grazing": 3.895e-07, "body_miss": 1.664e-07, "unit_miss": 1.143e-07},
        3: {"head_on": 1.148e-07, "grazing": 6.845e-07, "body_miss": 1.173e-07, "unit_miss": 5.070e-08},
    },
    "chain_64": {
        0: {"head_on": 3.730e-07, "grazing": 5.609e-07, "body_miss": 4.604e-05, "unit_miss": 3.452e-07},
        1: {"head_on": 1.241e-07, "grazing": 5.325e-07, "body_miss": 1.454e-04, "unit_miss": 1.140e-07},
        2: {"head_on": 1.499e-07, "grazing": 6.760e-07, "body_miss": 1.697e-07, "unit_miss": 1.115e-07},
        3: {"head_on": 1.189e-07, "grazing": 4.132e-06, "body_miss": 1.133e-07, "unit_miss": 1.133e-07},
    },
    "wide": {
        0: {"head_on": 1.824e-06, "grazing": 5.591e-06, "body_miss": 1.707e-04, "unit_miss": 2.102e-07},
        1: {"head_on": 1.031e-06, "grazing": 1.340e-05, "body_miss": 8.772e-05, "unit_miss": 3.562e-07},
    },
    "noisy": {
        0: {"head_on": 4.433e-07, "grazing": 2.005e-06, "body_miss": 2.592e-04, "unit_miss": 2.727e-07},
        1: {"head_on": 8.337e-07, "grazing": 2.292e-06, "body_miss": 4.375e-05, "unit_miss": 2.860e-07},
    },
    "steep": {
        0: {"head_on": 1.444e-07, "grazing": 2.897e-07, "body_miss": 2.155e-04, "unit_miss": 1.695e-07},
        1: {"head_on": 1.656e-07, "grazing": 4.486e-07, "body_miss": 1.219e-04, "unit_miss": 1.085e-07},
        2: {"head_on": 1.179e-07, "grazing": 3.600e-07, "body_miss": 1.120e-07, "unit_miss": 1.070e-07},
        3: {"head_on": 1.897e-07, "grazing": 8.298e-07, "body_miss": 1.975e-07, "unit_miss": 1.129e-07},
        4: {"head_on": 1.389e-07, "grazing": 8.820e-07, "body_miss": 2.743e-07, "unit_miss": 1.185e-07},
        5: {"head_on": 1.189e-07, "grazing": 0.000e+00, "body_miss": 1.563e-07, "unit_miss": 1.112e-07},
    },
    "ties": {
        0: {"head_on": 1.041e-06, "grazing": 0.000e+00, "body_miss": 4.783e-07, "unit_miss": 2.539e-07},
        1: {"head_on": 6.176e-07, "grazing": 1.167e-07, "body_miss": 2.646e-07, "unit_miss": 2.585e-07},
    },
    "flat": {
        0: {"head_on": 1.073e-05, "grazing": 4.606e-05, "body_miss": 4.088e-05, "unit_miss": 3.708e-07},
    },
    "unit_sphere": {
        0: {"head_on": 1.625e-07, "grazing": 3.176e-07, "body_miss": 0.000e+00, "unit_miss": 2.505e-07},
        1: {"head_on": 1.212e-07, "grazing": 4.887e-07, "body_miss": 0.000e+00, "unit_miss": 1.550e-07},
    },
    "uniform": {
        0: {"head_on": 0.000e+00, "grazing": 0.000e+00, "body_miss": 2.958e-07, "unit_miss": 2.958e-07},
        1: {"head_on": 0.000e+00, "grazing": 0.000e+00, "body_miss": 1.740e-07, "unit_miss": 1.740e-07},
    },
}
