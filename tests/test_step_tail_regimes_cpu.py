"""The rehearsal of tests/test_gpu_step_tail_regimes.py on the CPU alone: the restatements of
tests/helpers/step_tail_regimes.py are what they restate bit for bit (F.binary_cross_entropy_with_logits, compute_grad2,
F.mse_loss and autograd; torch.optim.Adam / RMSprop(foreach=False); Tensor.lerp), every regime reaches what it is named for,
the committed fp32 floors -- from which the GPU test's bars follow -- are what this torch build measures, and every mutation
of a restatement is caught by the cells CAUGHT_BY names when it is judged exactly as the GPU output is."""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import step_tail_regimes as R


def test_tables_are_the_issue_s():
    assert R.LOSS_SHAPES == ((1, 1, 0), (1, 7, 12288), (3, 1, 256), (5, 7, 1031), (64, 7, 48), (8, 1, 49152))
    assert 64 * 7 > 256 and 8 * 49152 == 393216 > 1024 * 256 and 1031 % 64 != 0
    assert R.LOGIT_REGIMES == ("balanced", "saturated", "tiny") and set(abs(v) for v in R.SATURATED) == {15, 17, 30, 88, 90, 104}
    assert sorted(R.SATURATED) == sorted(-v for v in R.SATURATED)
    assert R.GX_REGIMES == {"1e-6": 1e-6, "1": 1.0, "1e3": 1e3} and R.REG_W == 10.0
    assert R.TERM_SETS == ("real", "fake", "real+fake", "real+fake+pose", "real+fake+gx", "real+fake+pose+gx")
    assert R.CAT_SHAPES == ((1, 7, 12288), (3, 1, 256))
    assert R.GLUE_VARIANCE == (-2.0, -1.3816, -1.3815, 0.0, 0.3, 1.3815, 1.3816, 2.0)
    assert R.GLUE_AMBIENT == (-30.0, 0.0, 30.0) and R.GLUE_SPECULAR == (-0.2, 0.0, 0.7)
    assert R.RS_R1 == (0.0, 1.0, 340.0) and 0.0 in R.RS_R0 and len(R.RS_R0) == 2
    assert {len(t) for t, _ in R.WSUM_CASES.values()} == {1, 8}
    t8, w8 = R.WSUM_CASES["n=8"]
    assert 0.0 in w8 and min(t8) == 1e-8 and max(t8) == 1e6
    assert R.OPT_SIZES == (1, 7, 4095, 4096, 4097, 3 * 4096 + 5) and R.opt_sizes("ordinary")[-1] == 0
    assert R.opt_sizes("long") == R.OPT_SIZES and R.GRAD_REGIMES["long"] == 200 and R.GRAD_REGIMES["ordinary"] == 50
    assert R.HYPER["adam"] == {"config": dict(lr=2e-5, betas=(0.0, 0.9), eps=1e-8), "default": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)}
    assert R.HYPER["rmsprop"] == {"config": dict(lr=1e-4, alpha=0.99, eps=1e-8), "default": dict(lr=1e-2, alpha=0.99, eps=1e-8)}
    assert {"ordinary", "mixed", "vanishing", "spike", "zeros", "long", "late"} <= set(R.GRAD_REGIMES) and R.LATE_STEP == 999
    assert R.EMA_BETAS == (0.0, 0.5, 0.999, 1.0) and R.EMA_UPDATES == 3
    assert R.PROJECT_BAR == {"param": 2e-7, "state": 1e-6, "loss": 2e-6, "logit_grad": 1e-7, "glue": 2e-6}
    cells = R.cells()
    assert len(cells) == len(set(cells)) and set(cells) == set(R.FP32_FLOOR)
    for c in cells:
        assert set(R.FP32_FLOOR[c]) == set(R.tensors_of(c)), c
    assert set(R.CAUGHT_BY) | set(R.NOT_DETECTABLE) == set(R.MUTATIONS) and not set(R.CAUGHT_BY) & set(R.NOT_DETECTABLE)
    assert all(c in cells for cs in R.CAUGHT_BY.values() for c in cs)
    # every shape meets every logit regime and every term set it can carry; every term set is met
    for shape in R.LOSS_SHAPES:
        mine = [c.split("/") for c in R.loss_cells() if c.split("/")[1] == R.shape_name(shape)]
        assert {c[2].split("@")[0] for c in mine} == set(R.LOGIT_REGIMES)
        for logit in ("balanced", "saturated@0", "tiny"):
            assert {c[3] for c in mine if c[2] == logit} == set(R.term_sets(shape)), (shape, logit)
        if shape[2]:
            assert {c[4] for c in mine if "gx" in c[3]} == set(R.GX_REGIMES)
    assert set(R.term_sets((5, 7, 1031))) == set(R.TERM_SETS)


def _reference_losses(i, dtype):
    """The composition the kernels replace: BCE with logits on column 0, compute_grad2 (src/loss/gan.py:5-14) through a
    discriminator that is linear in its input (so that its input gradient IS gx), MSE on the remaining columns, summed as
    the trainer sums them; gradients by autograd."""
    B, K, N = i["shape"]
    c = lambda t: None if t is None else t.to(dtype).clone().requires_grad_()
    dr, df, gx = c(i["d_real"]), c(i["d_fake"]), c(i["gx"])
    pose = None if i["pose"] is None else i["pose"].to(dtype)
    zero = torch.zeros((), dtype=dtype)
    real = F.binary_cross_entropy_with_logits(dr[:, :1], torch.ones(B, 1, dtype=dtype)) if dr is not None else zero
    fake = F.binary_cross_entropy_with_logits(df[:, :1], torch.zeros(B, 1, dtype=dtype)) if df is not None else zero
    reg = zero
    if gx is not None:
        x_in = torch.zeros(B, N, dtype=dtype, requires_grad=True)
        d_out = (x_in * gx).sum(1, keepdim=True)
        (grad_dout,) = torch.autograd.grad(outputs=d_out.sum(), inputs=x_in, create_graph=True, retain_graph=True, only_inputs=True)
        reg = grad_dout.pow(2).reshape(B, -1).sum(1).mean()
    aux = F.mse_loss(df[:, 1:], pose) if pose is not None else zero
    total = real + fake
    if gx is not None:
        total = total + R.REG_W * reg
    if pose is not None:
        total = total + R.AUX_W * aux
    named = [(n, t) for n, t in (("g_real", dr), ("g_fake", df), ("g_gx", gx)) if t is not None]
    grads = torch.autograd.grad(total, [t for _, t in named])
    return torch.stack([total, real + fake, reg, fake, real, aux]).detach(), {n: g for (n, _), g in zip(named, grads)}


@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=R.shape_name)
def test_loss_restatement_is_what_it_restates(shape):
    for cell in R.loss_cells():
        if cell.split("/")[1] != R.shape_name(shape):
            continue
        i = R.loss_inputs(cell)
        for dt in (torch.float64, torch.float32):
            with R._one_thread():
                parts, grads = _reference_losses(i, dt)
            r = R.restate(cell, dt)
            assert torch.equal(parts, r["parts"]), (cell, dt)
            for k in ("g_real", "g_fake", "g_gx"):
                assert (r[k] is None) == (k not in grads), (cell, k)
                if k in grads:
                    assert torch.equal(grads[k], r[k]), (cell, dt, k)


@pytest.mark.parametrize("cell", R.opt_cells())
def test_optimizer_restatement_is_torch_optim(cell):
    kind, hyper, regime = cell.split("/")
    h = R.HYPER[kind][hyper]
    for dt in (torch.float64, torch.float32):
        ps = [t.to(dt).clone().requires_grad_() for t in R.opt_params(kind, hyper, regime)]
        opt = (torch.optim.Adam if kind == "adam" else torch.optim.RMSprop)(ps, foreach=False, **h)
        init = R.opt_initial_state(kind, hyper, regime)
        names = ("exp_avg", "exp_avg_sq") if kind == "adam" else ("square_avg",)
        if init is not None:
            sd = opt.state_dict()
            sd["state"] = {k: dict(step=torch.tensor(float(init[0])), **{n: v[k].to(dt).clone() for n, v in zip(names, init[1:])})
                           for k in range(len(ps))}
            opt.load_state_dict(sd)
        with R._one_thread():
            for t in range(1, R.GRAD_REGIMES[regime] + 1):
                for p, g in zip(ps, R.opt_grads(kind, hyper, regime, t)):
                    p.grad = None if g is None else g.to(dt)
                opt.step()
        r = R.restate(cell, dt)
        for k, p in enumerate(ps):
            st = opt.state[p]
            assert torch.equal(p.detach(), r["p"][k]) and int(st["step"]) == r["step"][k], (cell, dt, k)
            for n in names:
                assert torch.equal(st[n], r[n][k]), (cell, dt, k, n)


@pytest.mark.parametrize("beta", R.EMA_BETAS)
def test_ema_restatement_is_tensor_lerp(beta):
    for dt in (torch.float64, torch.float32):
        pe, seq = R.ema_sequence(beta)
        pe = [t.to(dt) for t in pe]
        for ps in seq:
            pe = [p.to(dt).lerp(a, beta) for a, p in zip(pe, ps)]     # p_ema.copy_(p.lerp(p_ema, beta))
        for a, b in zip(pe, R.restate(f"ema/{beta}", dt)["p_ema"]):
            assert torch.equal(a, b)
    # a + w (b - a) below one half, b - (b - a)(1 - w) from there on
    a, b = torch.randn(64, generator=torch.Generator().manual_seed(1)), torch.randn(64, generator=torch.Generator().manual_seed(2))
    assert torch.equal(a.lerp(b, 0.25), a + 0.25 * (b - a)) and torch.equal(a.lerp(b, 0.75), b - (b - a) * (1 - 0.75))


def test_glue_restatements_are_the_tensor_expressions():
    for cell in R.glue_cells():
        v, a, s = (torch.tensor(float(x)) for x in cell.split("/")[1:])
        r = R.restate(cell, torch.float32)
        inv_s = torch.exp(v * 10.0).clamp(1e-6, 1e6)
        ref = [inv_s, 1.0 / inv_s, torch.sigmoid(a), 1 - torch.sigmoid(a), s.clamp(min=0)]
        assert all(torch.equal(r[k], x) for k, x in zip(R.GLUE_OUT, ref)), cell
        assert torch.equal(r["packed3"], torch.stack([a, s, torch.tensor(10.0)]))
    for cell in R.rs_cells():
        for dt in (torch.float64, torch.float32):
            r0, r1 = (float(x) for x in cell.split("/")[1:])
            r4 = torch.tensor([r0, r1, 7.25, 0.0], dtype=dt, requires_grad=True)
            err, surf = r4[0] / (r4[1] + 1e-5), r4[2] * (1.0 / 4096.0)
            (2.0 * err + 5.0 * surf).backward()
            r = R.restate(cell, dt)
            assert torch.equal(err.detach(), r["gradient_error"]) and torch.equal(surf.detach(), r["surface_loss"])
            got = torch.stack([r[f"g_r4_{k}"] for k in range(4)])
            assert torch.allclose(got, r4.grad, rtol=1e-14 if dt == torch.float64 else 3e-7, atol=0), cell
    for cell in R.wsum_cells():
        terms, weights = R.WSUM_CASES[cell.split("/")[1]]
        r = R.restate(cell, torch.float64)
        assert float(r["total"]) == pytest.approx(sum(float(torch.tensor(t)) * w for t, w in zip(terms, weights)), rel=1e-12)


def test_regimes_reach_what_they_are_named_for():
    x887, x1039 = math.log(torch.finfo(torch.float32).max), -math.log(2.0 ** -150)     # 88.72, 103.97
    for shape in R.LOSS_SHAPES:
        B, K, N = shape
        sat = [c for c in R.loss_cells() if c.split("/")[1] == R.shape_name(shape) and "saturated" in c and "real+fake" in c]
        vals = torch.cat([torch.cat([R.loss_inputs(c)["d_real"][:, 0], R.loss_inputs(c)["d_fake"][:, 0]]) for c in sat])
        for lim in (16.64, x887, x1039):   # both sides of every threshold, both signs
            assert bool(((vals > 0) & (vals < lim) & (vals >= 15)).any()) and bool((vals > lim).any()), (shape, lim)
            assert bool(((vals < 0) & (vals > -lim) & (vals <= -15)).any()) and bool((vals < -lim).any()), (shape, lim)
        real0 = torch.cat([R.loss_inputs(c)["d_real"][:, 0] for c in sat])
        assert {float(v) for v in real0 if abs(float(v)) >= 15} == set(R.SATURATED), shape    # real meets all twelve, fake their negatives
        if B >= 12:
            assert bool((real0.abs() <= 3).any())                                               # ... among ordinary ones
        tiny = R.loss_inputs(f"loss/{R.shape_name(shape)}/tiny/real+fake/-")
        assert 0 < float(tiny["d_real"].abs().max()) <= 1e-6 and float(tiny["d_fake"].abs().max()) <= 1e-6
        bal = R.loss_inputs(f"loss/{R.shape_name(shape)}/balanced/real+fake/-")
        assert float(bal["d_real"].abs().max()) <= 3
    assert R.loss_inputs("loss/1x1x0/balanced/real/-")["gx"] is None and R.loss_inputs("loss/1x1x0/balanced/real/-")["d_fake"] is None
    big = R.loss_inputs("loss/8x1x49152/balanced/real+fake+gx/1")["gx"]
    assert big.numel() > 1024 * 256
    for gxr, scale in R.GX_REGIMES.items():
        gx = R.loss_inputs(f"loss/5x7x1031/balanced/real+fake+gx/{gxr}")["gx"]
        assert 0.5 * scale < float(gx.std()) < 2 * scale
    for c in R.cat_cells():
        assert R.loss_inputs(c)["gx"] is not None
    # glue: both sides of both clamp ends
    inv = {v: float(torch.exp(torch.tensor(v, dtype=torch.float64) * 10)) for v in R.GLUE_VARIANCE}
    assert inv[-1.3816] < 1e-6 < inv[-1.3815] < 1.001e-6 and 0.999e6 < inv[1.3815] < 1e6 < inv[1.3816]
    # optimisers
    for kind in ("adam", "rmsprop"):
        for hyper, h in R.HYPER[kind].items():
            sq = "exp_avg_sq" if kind == "adam" else "square_avg"
            r = R.case(f"{kind}/{hyper}/vanishing")["r64"]
            v = torch.cat(r[sq])
            if kind == "adam":
                v = v / (1 - h["betas"][1] ** R.GRAD_REGIMES["vanishing"])
            assert float((v.sqrt() < 10 * h["eps"]).double().mean()) >= 0.25, (kind, hyper)
            gs = [g for t in range(1, 11) for g in R.opt_grads(kind, hyper, "vanishing", t)]
            g2 = torch.cat(gs) ** 2 * (1 - (h["betas"][1] if kind == "adam" else h["alpha"]))
            assert float(g2.min()) >= float(torch.finfo(torch.float32).tiny)                   # every square a normal float32
            assert 1e-12 <= float(torch.cat(gs).abs().min()) and float(torch.cat(gs).abs().max()) <= 1.0001e-8
            m = torch.cat(R.opt_grads(kind, hyper, "mixed", 3)).abs()
            assert float(m[m > 0].min()) < 1e-5 and float(m.max()) > 1e2
            sp = [float(torch.cat(R.opt_grads(kind, hyper, "spike", t)).abs().max()) for t in range(1, 31)]
            assert sp[20] == 1e4 and max(sp[:20] + sp[21:]) < 1e-2
            z = R.opt_grads(kind, hyper, "zeros", 4)
            assert float(z[R.ZERO_TENSOR].abs().max()) == 0.0 and float(z[3][::R.ZERO_EVERY].abs().max()) == 0.0 and float(z[3].abs().max()) > 0
            assert R.case(f"{kind}/{hyper}/late")["r64"]["step"] == [R.LATE_STEP + 3] * 7
            steps = R.case(f"{kind}/{hyper}/skips")["r64"]["step"]
            assert steps[R.SKIP_TENSOR] == 6 and steps[0] == 8
            assert float(torch.cat(R.case(f"{kind}/{hyper}/ordinary")["r64"][sq]).max()) > 1.0    # a relative error shows


@pytest.mark.parametrize("family", ("loss", "cat", "glue", "rs", "wsum", "adam", "rmsprop", "ema"))
def test_fp32_floor_is_the_committed_one(family):
    """A fresh measurement within 1.5x of the committed table (a torch build whose float32 arithmetic is noisier must fail
    here, not move the GPU test's bars silently); the float32 restatement itself passes every assertion of the GPU test."""
    for cell in R.cells():
        if cell.split("/")[0] != family:
            continue
        fresh = R.measure_floor(cell)
        for k, v in fresh.items():
            assert v <= 1.5 * R.FP32_FLOOR[cell][k] + 1e-300, (cell, k, v, R.FP32_FLOOR[cell][k])
            assert R.bar(cell, k) >= R.PROJECT_BAR[R.KIND[k]]
        assert R.judge(cell, R.case(cell)["r32"]) == [], cell


@pytest.mark.parametrize("mutation", tuple(R.CAUGHT_BY))
def test_mutation_is_caught(mutation):
    """The float32 restatement with one plausible kernel / host error, judged exactly as the GPU output is (structural,
    value bar x 3), fails in every cell CAUGHT_BY names."""
    print()
    for cell in R.CAUGHT_BY[mutation]:
        bad = R.judge(cell, R.restate(cell, torch.float32, mutation), factor=3.0)
        print(f"  {mutation} in {cell}: {bad}")
        assert bad, (mutation, cell)


def test_complement_of_beta_is_the_predicted_deviation():
    """1.0f - (float)beta against torch's (float)(1.0 - beta): exp_avg_sq of 50 default-beta steps moves by 1.3e-5 (relative)
    from float64, ten times the float32 restatement's own distance, and misses bar() by more than 3x."""
    cell = "adam/default/ordinary"
    r64 = R.case(cell)["r64"]
    mut = R.restate(cell, torch.float32, "complement_rounded")
    rel = lambda a, b: max(float((x.double() - y).abs().max()) / float(y.abs().max()) for x, y in zip(a, b) if y.numel())
    d_mut, d_f32 = rel(mut["exp_avg_sq"], r64["exp_avg_sq"]), rel(R.case(cell)["r32"]["exp_avg_sq"], r64["exp_avg_sq"])
    print(f"\nexp_avg_sq after 50 steps: complement from the rounded float {d_mut:.2e}, torch float32 {d_f32:.2e} (relative)")
    assert 1.0e-5 < d_mut < 1.6e-5 and d_f32 < 3e-6
    assert R.margins(cell, mut)["exp_avg_sq"] > 3.0
    assert R.bar(cell, "exp_avg_sq") <= 3 * max(R.FP32_FLOOR[cell]["exp_avg_sq"], R.PROJECT_BAR["state"] / 3)


def test_mutations_listed_as_not_detectable_are_caught_nowhere():
    """(If one of these starts to be caught, it belongs in CAUGHT_BY.)  Every entry carries its written reason."""
    for mutation, reason in R.NOT_DETECTABLE.items():
        assert len(reason) > 40, mutation
        assert all(not R.judge(c, R.restate(c, torch.float32, mutation), factor=3.0) for c in R.cells()), mutation
