"""The FiLM-SIREN MLP kernels (csrc/mlp.hip, mlp_fwd3.hip, mlp_bwd.hip) against the float64 restatement of
tests/helpers/mlp_regimes.py in the regimes a trained field reaches: distinct image scales per layer, grown weights, FiLM
scales through zero, an a-priori adjoint bound that is met and one that is 2^7 loose, scale-setting weight outliers, a dead
layer, far points and phases of +-41 revolutions.  Every bar is 3 x the committed float32 floor of its (cell, tensor) and never
above the project's existing bar (tests/test_mlp_regimes_cpu.py); the measured errors go to
mlp_regimes[<mode>] / mlp_regimes_backward[f16x3] (profiles/mlp_regimes_margins.txt)."""
import functools
import os

import pytest
import torch

from conftest import GOLDEN, record_margin
from helpers import mlp_regimes as M
from helpers.guarded import guarded_ops  # noqa: F401  (fixture)

# every output of oi_amd.ops is a guarded, poisoned arena view (tests/helpers/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_ops")]
PREC = {"f32": 0, "f16x3": 4}
NET_KW = dict(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
CALLS = ("sdf_only", "grad_rgb", "grad_rgb_feat")


@functools.lru_cache(maxsize=None)
def forward(name, mode):
    """The three calls of one (cell, mode) -> {call: {tensor: CPU tensor}}; run once, shared (distinct_scales reads init's)."""
    from oi_amd import ops
    c = M.cell(name)
    d = {k: c[k].cuda() for k in M.LEAVES + ("pts",)}
    prec = PREC[mode]
    packed = ops.mlp_pack_weights(*[d[k] for k in M.PARAMS], prec)
    ops.mlp_pack_status(packed)          # raises unless every image was built from finite weights
    out = {}
    for call, (wg, wr, wf) in zip(CALLS, ((False, False, False), (True, True, False), (True, True, True))):
        sdf, grad, rgb, feat, _ = ops.sdf_mlp_fwd(d["pts"], packed, d["gamma"], d["beta"], M.B, prec, want_grad=wg, want_rgb=wr,
                                                  want_feat=wf)
        torch.cuda.synchronize()
        out[call] = {k: v.detach().cpu().clone() for k, v in (("sdf", sdf), ("grad", grad), ("rgb", rgb), ("feat", feat))
                     if v is not None}
    return out


def _report(name, tensor, err, floor_key=None):
    fk = floor_key or tensor
    return f"{name}/{tensor}: error {err:.3e}, bar {M.bar(name, fk):.3e}, float32 floor {M.FP32_FLOOR[name][fk]:.3e}"


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("name", M.CELLS)
def test_forward_regime(name, mode):
    """sdf only (sdf_mlp_kernel), grad + rgb, grad + rgb + feat (f16x3: the register-resident kernel): every output finite and
    within 3 x the float32 floor of the float64 restatement, the three sdf within the bar of each other, the pack status clean.
    dead_layer: d sdf/dx of element 0 is exactly 0.  distinct_scales: every output word is init's, in both modes -- the
    power-of-two rescaling leaves the scaled fp16 image, G, A and B (f16x3) and every float32 product and sum (f32) unchanged."""
    out = forward(name, mode)
    bad = []
    for call in CALLS:
        for k, v in out[call].items():
            assert bool(torch.isfinite(v).all()), f"{name}[{mode}] {call}: {k} is not finite " \
                                                  f"({int((~torch.isfinite(v)).sum())} of {v.numel()} values)"
        for tensor, err in M.errors(name, out[call]).items():
            record_margin(f"mlp_regimes[{mode}]", f"{name}/{tensor}", err)
            print(f"[{mode}] {call} {_report(name, tensor, err)}")
            if err > M.bar(name, tensor):
                bad.append(f"{call} {_report(name, tensor, err)}")
    for call in CALLS[1:]:
        e = float((out[call]["sdf"].double() - out["sdf_only"]["sdf"].double()).abs().max())
        record_margin(f"mlp_regimes[{mode}]", f"{name}/sdf({call} - sdf_only)", e)
        if e > M.bar(name, "sdf"):
            bad.append(f"sdf of {call} against sdf_only: {_report(name, 'sdf', e)}")
    assert not bad, f"[{mode}] " + "; ".join(bad)
    if name == "dead_layer":
        for call in CALLS[1:]:
            g0 = out[call]["grad"][:M.N_PER]
            assert int((g0 != 0).sum()) == 0, f"{call}: d sdf/dx behind the dead layer is not exactly 0: {g0.abs().max():.3e}"
    if name == "distinct_scales":
        ref = forward("init", mode)
        for call in CALLS:
            for k, v in out[call].items():
                diff = v.view(torch.int32) != ref[call][k].view(torch.int32)
                assert not bool(diff.any()), f"[{mode}] {call}: {int(diff.sum())} words of {k} differ from init's, worst " \
                                             f"{float((v.double() - ref[call][k].double()).abs().max()):.3e}"


def _state_dicts(c):
    """The cell's weights under the reference's state_dict names (the FiLM heads keep the golden values: gamma and beta are
    leaves of the test, not outputs of the heads)."""
    sd, csd = ({k: v.clone() for k, v in s.items()} for s in M.golden_sds())
    for l in range(8):
        sd[f"pts_linears.{l}.weight"] = M._weight(c, l).clone()
        sd[f"pts_linears.{l}.bias"] = M._bias(c, l).clone()
    sd["sigma_linear.weight"], sd["sigma_linear.bias"] = c["wsig"].view(1, M.C).clone(), c["bsig"].clone()
    csd["views_linears.weight"], csd["views_linears.bias"] = c["wv"].clone(), c["bv"].clone()
    csd["rgb_linear.weight"], csd["rgb_linear.bias"] = c["wrgb"].clone(), c["brgb"].clone()
    return sd, csd


@functools.lru_cache(maxsize=None)
def backward(name):
    """{tensor of M.backward_names(): CPU gradient} of <cs, sdf> + <cg, grad> + <cr, rgb> through FieldPack / autograd.sdf_mlp
    in f16x3, gamma and beta as leaves; run once per cell, shared (distinct_scales reads init's)."""
    from oi_amd.fields import ShapeNetwork, ColorNetwork, FieldPack
    from oi_amd.autograd import sdf_mlp
    c = M.cell(name)
    sd, csd = _state_dicts(c)
    sdf_net = ShapeNetwork(os.path.join(GOLDEN, "weights_sdf.npz"), **NET_KW)
    sdf_net.load_state_dict(sd)
    col_net = ColorNetwork(**NET_KW)
    col_net.load_state_dict(csd)
    sdf_net, col_net = sdf_net.cuda(), col_net.cuda()
    pack = FieldPack(sdf_net, col_net, "f16x3")
    gamma, beta = c["gamma"].cuda().requires_grad_(True), c["beta"].cuda().requires_grad_(True)
    sdf, grad, rgb, _ = sdf_mlp(pack, c["pts"].cuda(), gamma, beta, M.B, True, True, False)
    cs, cg, cr = (x.cuda() for x in M.cotangents(name))
    loss = (sdf * cs).sum() + (grad * cg).sum() + (rgb * cr).sum()
    sp, cp = dict(sdf_net.named_parameters()), dict(col_net.named_parameters())
    leaves = {"w0": sp["pts_linears.0.weight"], "b0": sp["pts_linears.0.bias"], "wsig": sp["sigma_linear.weight"],
              "bsig": sp["sigma_linear.bias"], "wv": cp["views_linears.weight"], "bv": cp["views_linears.bias"],
              "wrgb": cp["rgb_linear.weight"], "brgb": cp["rgb_linear.bias"]}
    for l in range(1, 8):
        leaves[f"wh.{l}"], leaves[f"bh.{l}"] = sp[f"pts_linears.{l}.weight"], sp[f"pts_linears.{l}.bias"]
    names = list(leaves)
    gr = torch.autograd.grad(loss, [leaves[k] for k in names] + [gamma, beta])
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().clone() for k, v in zip(names, gr)}
    out["wsig"] = out["wsig"].reshape(-1)
    g_gamma, g_beta = gr[-2].detach().cpu(), gr[-1].detach().cpu()
    for l in range(9):
        out[f"gamma.{l}"], out[f"beta.{l}"] = g_gamma[:, l].clone(), g_beta[:, l].clone()
    return out


@pytest.mark.parametrize("name", M.BWD_CELLS)
def test_backward_regime(name):
    """Every parameter gradient, d_gamma and d_beta (per layer) of the f16x3 backward against float64 autograd through the
    restatement, rel_err against 3 x the float32 floor of float32 autograd.  dead_layer: the FiLM layers below the dead layer
    receive exactly 0 from element 0.  distinct_scales: dW_l 2^j, db_l 2^j and d gamma_l 2^-j are init's within the bar."""
    got = backward(name)
    bad = []
    for k in M.backward_names():
        assert bool(torch.isfinite(got[k]).all()), f"{name}: d {k} is not finite"
    for k, err in M.backward_errors(name, got).items():
        record_margin("mlp_regimes_backward[f16x3]", f"{name}/d.{k}", err)
        print(f"[f16x3] backward {_report(name, 'd.' + k, err)}")
        if err > M.bar(name, "d." + k):
            bad.append(_report(name, "d." + k, err))
    assert not bad, "; ".join(bad)
    if name == "dead_layer":
        for l in range(M.DEAD_LAYER):
            for k in (f"gamma.{l}", f"beta.{l}"):
                assert int((got[k][0] != 0).sum()) == 0, f"d {k} of element 0 (below the dead layer): {got[k][0].abs().max():.3e}"
    if name == "distinct_scales":
        ref = backward("init")
        js = dict(zip(range(1, 8), M.J_SCALES))
        pairs = [(f"wh.{l}", 2.0 ** j) for l, j in js.items()] + [(f"bh.{l}", 2.0 ** j) for l, j in js.items()] + \
                [(f"gamma.{l}", 2.0 ** -j) for l, j in js.items()] + \
                [("wv", 2.0 ** M.J_COLOUR), ("bv", 2.0 ** M.J_COLOUR), ("gamma.8", 2.0 ** -M.J_COLOUR)]
        scaled = dict(pairs)
        for k in scaled:
            e = M.rel_err(got[k] * scaled[k], ref[k])
            record_margin("mlp_regimes_backward[f16x3]", f"distinct_scales/d.{k} (rescaled - init)", e)
            if e > M.bar("init", "d." + k):
                bad.append(f"d {k} rescaled against init's: {_report('init', 'd.' + k, e)}")
        assert not bad, "; ".join(bad)
