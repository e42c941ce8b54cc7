"""The scalar tail of a training step on the GPU -- oi_amd.losses.gan_losses / gan_losses_cat / weighted_sum,
oi_amd.renderer.render_scalars, oi_amd.ops.scalar_glue (csrc/loss.hip) and FusedAdam / FusedRMSprop / EMA (csrc/optim.hip,
oi_amd/optim.py) -- against the float64 restatements of tests/helpers/step_tail_regimes.py, on every cell: saturated and
tiny logits, batch 1, K = 1, the R1 sum at 393,216 elements and the backward's stride loop, every optional-term combination,
both clamp ends of exp(10 v), r4[1] = 0, eight terms; torch's default hyper-parameters beside the config's, 50 and 200
steps, vanishing / mixed / spiking / zero gradients, a late step count, skipped parameters; beta in {0, 1} for the EMA.

Inputs, reference, floors and bars are rehearsed on the CPU by tests/test_step_tail_regimes_cpu.py, which also shows that each
plausible kernel / host error fails the assertions made here (`R.judge`).  Bar per (cell, tensor) = the larger of the
project's existing bar and 3x the committed fp32 floor; every cell's margin is printed and reported through record_margin
under step_tail[<cell>] (profiles/step_tail_regimes_margins.txt).

The host-logic cases at the end feed FusedAdam / FusedRMSprop and torch.optim on CPU float64 the same gradients; their bar is
the larger of the project's and 3x the distance of torch.optim on CPU float32 from the same float64 run."""
import pytest
import torch

from conftest import record_margin
from helpers import step_tail_regimes as R
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]


def _report_and_judge(cell, got):
    m = R.margins(cell, got)
    r64 = R.case(cell)["r64"]
    for k, v in m.items():
        d = R.distance(k, got.get(k), r64[k])
        record_margin(f"step_tail[{cell}]", k, d)
        print(f"  step_tail {cell} {k:14s} error {d:.3e}  floor {R.FP32_FLOOR[cell][k]:.3e}  bar {R.bar(cell, k):.3e}  margin {v:.3f}")
    bad = R.judge(cell, got)
    assert not bad, (cell, bad)


def _dev(t, grad=False):
    return None if t is None else t.cuda().requires_grad_(grad)


# ----------------------------------------------------------------------------------------------------------------------
# losses and glue
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=R.shape_name)
def test_gan_losses(shape):
    from oi_amd.losses import gan_losses
    print()
    for cell in R.loss_cells():
        if cell.split("/")[1] != R.shape_name(shape):
            continue
        i = R.loss_inputs(cell)
        dr, df, gx = _dev(i["d_real"], True), _dev(i["d_fake"], True), _dev(i["gx"], True)
        aux_w = torch.full((), R.AUX_W, device="cuda") if i["pose"] is not None else None
        total, parts = gan_losses(dr, df, _dev(i["pose"]), gx, aux_w, R.REG_W)
        total.backward()
        got = {"parts": torch.cat([total.detach().reshape(1), parts.detach()]), "g_real": None if dr is None else dr.grad,
               "g_fake": None if df is None else df.grad, "g_gx": None if gx is None else gx.grad}
        _report_and_judge(cell, got)


@pytest.mark.parametrize("cell", R.cat_cells())
def test_gan_losses_cat(cell):
    """One discriminator pass over [real; fake]: d_all [2B, K], gx_all [2B, N] with an exactly zero fake half."""
    from oi_amd.losses import gan_losses_cat
    i = R.loss_inputs(cell)
    B, K, N = i["shape"]
    d_all = torch.cat([i["d_real"], i["d_fake"]]).cuda().requires_grad_()
    gx_all = torch.cat([i["gx"], torch.zeros(B, N)]).cuda().requires_grad_()
    aux_w = torch.full((), R.AUX_W, device="cuda") if i["pose"] is not None else None
    total, parts = gan_losses_cat(d_all, B, _dev(i["pose"]), gx_all, aux_w, R.REG_W)
    total.backward()
    print()
    _report_and_judge(cell, {"parts": torch.cat([total.detach().reshape(1), parts.detach()]), "g_real": d_all.grad[:B],
                             "g_fake": d_all.grad[B:], "g_gx": gx_all.grad[:B]})
    assert float(gx_all.grad[B:].abs().max()) == 0.0


def test_scalar_glue():
    from oi_amd import ops
    print()
    for cell in R.glue_cells():
        v, a, s = (torch.tensor(float(x), device="cuda") for x in cell.split("/")[1:])
        out5, packed3 = ops.scalar_glue(v, a, s, torch.tensor(10.0, device="cuda"))
        got = {k: out5[j] for j, k in enumerate(R.GLUE_OUT)}
        got["packed3"] = packed3
        _report_and_judge(cell, got)


def test_render_scalars():
    from oi_amd.renderer import render_scalars
    print()
    for cell in R.rs_cells():
        r0, r1 = (float(x) for x in cell.split("/")[1:])
        r4 = torch.tensor([r0, r1, 7.25, 0.0], device="cuda", requires_grad=True)
        err, surf = render_scalars(r4, 4096)
        (2.0 * err + 5.0 * surf).backward()
        got = {"gradient_error": err.detach(), "surface_loss": surf.detach()}
        got.update({f"g_r4_{k}": r4.grad[k] for k in range(4)})
        _report_and_judge(cell, got)


def test_weighted_sum():
    from oi_amd.losses import weighted_sum
    print()
    for cell in R.wsum_cells():
        terms, weights = R.WSUM_CASES[cell.split("/")[1]]
        ts = [torch.tensor(t, device="cuda", requires_grad=True) for t in terms]
        total = weighted_sum(ts, weights)
        (total * 3.0).backward()
        _report_and_judge(cell, {"total": total.detach(), "g_terms": torch.stack([t.grad for t in ts])})


# ----------------------------------------------------------------------------------------------------------------------
# optimisers, EMA: the regimes
# ----------------------------------------------------------------------------------------------------------------------
def _fused(kind, params, **kw):
    from oi_amd.optim import FusedAdam, FusedRMSprop
    return (FusedAdam if kind == "adam" else FusedRMSprop)(params, **kw)


def _state_names(kind):
    return ("exp_avg", "exp_avg_sq") if kind == "adam" else ("square_avg",)


def _collect(kind, opt, ps):
    """{"p", state lists, "step"} of a fused optimiser, through state_dict() (the step counts are written there)."""
    sd = opt.state_dict()["state"]
    got = {"p": [p.detach() for p in ps], "step": [int(sd[k]["step"]) if k in sd else 0 for k in range(len(ps))]}
    for n in _state_names(kind):
        got[n] = [sd[k][n] if k in sd else torch.zeros_like(ps[k]) for k in range(len(ps))]
    return got


@pytest.mark.parametrize("cell", R.opt_cells())
def test_optimizer_regime(cell):
    kind, hyper, regime = cell.split("/")
    ps = [t.cuda().requires_grad_() for t in R.opt_params(kind, hyper, regime)]
    opt = _fused(kind, ps, **R.HYPER[kind][hyper])
    init = R.opt_initial_state(kind, hyper, regime)
    if init is not None:
        sd = opt.state_dict()
        sd["state"] = {k: dict(step=torch.tensor(float(init[0])), **{n: v[k].clone() for n, v in zip(_state_names(kind), init[1:])})
                       for k in range(len(ps))}
        opt.load_state_dict(sd)
    for t in range(1, R.GRAD_REGIMES[regime] + 1):
        for p, g in zip(ps, R.opt_grads(kind, hyper, regime, t)):
            p.grad = None if g is None else g.cuda()
        opt.step()
    print()
    _report_and_judge(cell, _collect(kind, opt, ps))


@pytest.mark.parametrize("cell", R.ema_cells())
def test_ema(cell):
    from oi_amd.ema import EMA
    beta = float(cell.split("/")[1])
    pe0, seq = R.ema_sequence(beta)
    m = torch.nn.Module()
    m.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in pe0])
    m = m.cuda()
    ema = EMA(m, beta)
    for ps in seq:
        with torch.no_grad():
            for p, new in zip(m.ps, ps):
                p.copy_(new)
        ema.update(0)
    print()
    _report_and_judge(cell, {"p_ema": [p.detach() for p in ema.module.ps]})


# ----------------------------------------------------------------------------------------------------------------------
# optimisers: host logic, against torch.optim on CPU float64 fed the same gradients
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(1,), (7,), (33, 65), (4097,), (0,), (3 * 4096 + 5,)]


def _torch_opt(kind, params, **kw):
    return (torch.optim.Adam if kind == "adam" else torch.optim.RMSprop)(params, foreach=False, **kw)


def _groups(ps, lrs):
    """Parameter groups: one, or two halves with their own lr."""
    if lrs is None:
        return ps
    h = len(ps) // 2
    return [dict(params=ps[:h], lr=lrs[0]), dict(params=ps[h:], lr=lrs[1])]


def _grad(seed, t, k, shape):
    g = torch.Generator().manual_seed(1000 * seed + 37 * t + k)
    return 8.0 * torch.randn(shape, generator=g)


def _compare(case, kind, fused_ps, fused_sd, ref):
    """fused (GPU float32) against ref[float64], at the larger of the project's bar and 3x the distance of ref[float32]."""
    (o64, p64), (o32, p32) = ref[torch.float64], ref[torch.float32]
    print()
    for name in ("p",) + _state_names(kind):
        if name == "p":
            got, r64, r32 = [p.detach() for p in fused_ps], [p.detach() for p in p64], [p.detach() for p in p32]
        else:
            has = [k for k, p in enumerate(p64) if p in o64.state]
            got = [fused_sd[k][name] for k in has]
            r64, r32 = [o64.state[p64[k]][name] for k in has], [o32.state[p32[k]][name] for k in has]
        floor, d = R.distance(name, r32, r64), R.distance(name, got, r64)
        bar = max(R.PROJECT_BAR[R.KIND[name]], 3 * floor)
        record_margin(f"step_tail[host/{case}]", name, d)
        print(f"  step_tail host/{case} {name:14s} error {d:.3e}  floor {floor:.3e}  bar {bar:.3e}  margin {d / bar:.3f}")
        assert d <= bar, (case, name, d, bar)
    for k, p in enumerate(p64):
        want = int(o64.state[p]["step"]) if p in o64.state else None
        have = int(fused_sd[k]["step"]) if k in fused_sd else None
        assert want == have, (case, "step", k, want, have)


def _drive(case, kind, hyper, n_steps, lrs=None, halve_lr_after=None, skip=None, realloc=False, transposed=False, seed=1):
    h = R.HYPER[kind][hyper]
    init = [torch.randn(s, generator=torch.Generator().manual_seed(50 + k)) for k, s in enumerate(SHAPES)]
    fp = [t.cuda().requires_grad_() for t in init]
    fo = _fused(kind, _groups(fp, lrs), **h)
    ref = {}
    for dt in (torch.float64, torch.float32):
        ps = [t.to(dt).clone().requires_grad_() for t in init]
        ref[dt] = (_torch_opt(kind, _groups(ps, lrs), **h), ps)
    alive, addresses = [], [set() for _ in SHAPES]
    for t in range(1, n_steps + 1):
        for k, s in enumerate(SHAPES):
            g = None if (skip is not None and k == skip[0] and t in skip[1]) else _grad(seed, t, k, s)
            for dt, (_, ps) in ref.items():
                ps[k].grad = None if g is None else g.to(dt)
            if g is None:
                fp[k].grad = None
            elif transposed and len(s) == 2:
                fp[k].grad = g.t().contiguous().cuda().t()            # a transposed view: same values, strides (1, 33)
                assert not fp[k].grad.is_contiguous() and torch.equal(fp[k].grad.cpu(), g)
            else:
                fp[k].grad = g.cuda()
            if realloc and g is not None:
                alive.append(fp[k].grad)                               # kept alive: the next one cannot reuse the address
                addresses[k].add(fp[k].grad.data_ptr())
        fo.step()
        for o, _ in ref.values():
            o.step()
        if t == halve_lr_after:
            for o in [fo] + [o for o, _ in ref.values()]:
                for grp in o.param_groups:
                    grp["lr"] *= 0.5
    if realloc:
        from oi_amd.optim import _ChunkTable
        assert n_steps > _ChunkTable.RING and all(len(a) == n_steps for k, a in enumerate(addresses) if init[k].numel())
    _compare(case, kind, fp, fo.state_dict()["state"], ref)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("hyper", ["config", "default"])
def test_gradients_at_new_addresses_for_more_steps_than_the_ring(kind, hyper):
    _drive(f"realloc/{kind}/{hyper}", kind, hyper, 7, realloc=True)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_non_contiguous_gradient(kind):
    _drive(f"transposed/{kind}", kind, "default", 3, transposed=True)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_two_groups_with_their_own_lr(kind):
    lr = R.HYPER[kind]["default"]["lr"]
    _drive(f"two_groups/{kind}", kind, "default", 4, lrs=(lr, 0.1 * lr))


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_lr_halved_between_steps(kind):
    _drive(f"lr_halved/{kind}", kind, "default", 4, halve_lr_after=2)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("hyper", ["config", "default"])
def test_parameter_without_gradient_on_two_steps(kind, hyper):
    """Steps 2 and 5 of 8: from step 2 on Adam runs two bias-correction groups per step."""
    _drive(f"skips/{kind}/{hyper}", kind, hyper, 8, skip=(3, (2, 5)))


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("direction", ["fused_into_torch", "torch_into_fused"])
def test_state_dict_interchanges_at_torch_defaults(kind, direction):
    """5 steps in one implementation, state_dict() into the other, 3 more steps there: against 8 steps of torch.optim on CPU
    float64 (nothing is compared with itself; the bar's floor is torch.optim on CPU float32 over the same 8 steps)."""
    h = R.HYPER[kind]["default"]
    init = [torch.randn(s, generator=torch.Generator().manual_seed(50 + k)) for k, s in enumerate(SHAPES)]
    ref = {}
    for dt in (torch.float64, torch.float32):
        ps = [t.to(dt).clone().requires_grad_() for t in init]
        o = _torch_opt(kind, ps, **h)
        for t in range(1, 9):
            for k, s in enumerate(SHAPES):
                ps[k].grad = _grad(2, t, k, s).to(dt)
            o.step()
        ref[dt] = (o, ps)
    fp = [t.cuda().requires_grad_() for t in init]
    fo = _fused(kind, fp, **h)
    tp = [t.clone().requires_grad_() for t in init]         # torch.optim on CPU float32: the other side of the interchange
    to = _torch_opt(kind, tp, **h)
    first, second = ((fo, fp), (to, tp)) if direction == "fused_into_torch" else ((to, tp), (fo, fp))
    for t in range(1, 6):
        for k, s in enumerate(SHAPES):
            first[1][k].grad = _grad(2, t, k, s).to(first[1][k].device)
        first[0].step()
    second[0].load_state_dict(first[0].state_dict())
    with torch.no_grad():
        for a, b in zip(second[1], first[1]):
            a.copy_(b)
    for t in range(6, 9):
        for k, s in enumerate(SHAPES):
            second[1][k].grad = _grad(2, t, k, s).to(second[1][k].device)
        second[0].step()
    sd = second[0].state_dict()["state"]
    assert all(float(v["step"]) == 8.0 for v in sd.values()) and set(sd) == set(range(len(SHAPES)))
    _compare(f"state_dict/{direction}/{kind}", kind, second[1], sd, ref)
