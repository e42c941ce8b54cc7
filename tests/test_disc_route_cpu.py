"""CPU checks of the discriminator's host layer (oi_amd.discriminator): `route()` as a truth table -- the
expected column is written from the list of conditions, and every row is also held against a transcription of the nest of
conditions the forwards had before there was a route function --, the live-weight accessor after a parameter is replaced, and
lib.TICKET_WORDS against the header."""
import re

import pytest
import torch
import torch.nn as nn

import oi_amd.discriminator as DM
from helpers import cabi

SWITCHES = dict(SMALL_PATH=True, SMALL_PATH_128=True, LARGE_PATH=True, FAST_ADA=True, PRE_CHAIN=True)
W64, W128 = (64, 128, 256, 512), (32, 64, 128, 256, 512)
# a batch-1 no-grad call of the 64 x 64 / n_feat 512 network on the GPU, nobody capturing; no pipe (DCDiscriminator.forward)
BASE = dict(shape=(1, 3, 64, 64), grad=False, cuda=True, capturing=False, widths=W64, in_dim=3, out_dim=7, w_in=3, weights_ok=True)
NET128 = dict(shape=(1, 3, 128, 128), widths=W128)
ADA = dict(stock=True, theta=False, fast_draw=True)   # the shipped pipe in front of it (ADADiscriminator.forward)

ROWS = [
    # ---- network route (no pipe): one row per route
    ("small 64", {}, {}, (None, "small")),
    ("small 128", NET128, {}, (None, "small")),
    ("small B4 C1 out1", dict(shape=(4, 1, 64, 64), in_dim=1, w_in=1, out_dim=1), {}, (None, "small")),
    ("large B16", dict(shape=(16, 3, 64, 64)), {}, (None, "large")),
    ("arena B15", dict(shape=(15, 3, 64, 64)), {}, (None, "arena")),
    ("pre-activation chain", dict(grad=True), {}, (None, "pre")),
    ("lrelu chain: switch", dict(grad=True), dict(PRE_CHAIN=False), (None, "lrelu")),
    ("lrelu chain: CPU", dict(grad=True, cuda=False), {}, (None, "lrelu")),
    # ---- each single condition that knocks a call off the small route
    ("SMALL_PATH off", {}, dict(SMALL_PATH=False), (None, "arena")),
    ("SMALL_PATH_128 off at 128", NET128, dict(SMALL_PATH_128=False), (None, "arena")),
    ("SMALL_PATH_128 off at 64", {}, dict(SMALL_PATH_128=False), (None, "small")),
    ("grad", dict(grad=True), {}, (None, "pre")),
    ("CPU", dict(cuda=False), {}, (None, "arena")),
    ("B5", dict(shape=(5, 3, 64, 64)), {}, (None, "arena")),
    ("C5", dict(shape=(1, 5, 64, 64), in_dim=5, w_in=5), {}, (None, "arena")),
    ("out_dim 9", dict(out_dim=9), {}, (None, "arena")),
    ("wrong widths", dict(widths=(8, 16, 32, 64)), {}, (None, "arena")),
    ("128 with four blocks", dict(shape=(1, 3, 128, 128)), {}, (None, "arena")),
    ("64 with five blocks", dict(widths=W128), {}, (None, "arena")),
    ("32 x 32", dict(shape=(1, 3, 32, 32)), {}, (None, "arena")),
    ("C != in_dim", dict(in_dim=1), {}, (None, "arena")),
    ("C != weight's channels", dict(w_in=1), {}, (None, "arena")),
    ("non-contiguous / non-fp32 weight", dict(weights_ok=False), {}, (None, "arena")),
    ("capturing", dict(capturing=True), {}, (None, "arena")),
    # ---- the large route's conditions
    ("large: switch", dict(shape=(16, 3, 64, 64)), dict(LARGE_PATH=False), (None, "arena")),
    ("large: capturing", dict(shape=(16, 3, 64, 64), capturing=True), {}, (None, "arena")),
    ("large: CPU", dict(shape=(16, 3, 64, 64), cuda=False), {}, (None, "arena")),
    ("large: grad", dict(shape=(16, 3, 64, 64), grad=True), {}, (None, "pre")),
    ("large: any network (the pack decides)", dict(shape=(64, 3, 16, 16), widths=(32, 64)), {}, (None, "large")),
    # ---- augmentation routes in front of the small network
    ("lib", ADA, {}, ("lib", "small")),
    ("lib 128 B4", dict(ADA, widths=W128, shape=(4, 3, 128, 128)), {}, ("lib", "small")),
    ("theta", dict(ADA, theta=True), {}, ("theta", "small")),
    ("theta under capture", dict(ADA, theta=True, capturing=True), {}, ("theta", "small")),
    ("theta, FAST_ADA off", dict(ADA, theta=True), dict(FAST_ADA=False), ("theta", "small")),
    ("capturing: the pipe", dict(ADA, capturing=True), {}, ("pipe", "arena")),
    ("host: FAST_ADA off", ADA, dict(FAST_ADA=False), ("host", "small")),
    ("host: pinned percentile / other branches", dict(ADA, fast_draw=False), {}, ("host", "small")),
    # ---- off the small route: the pipe (or the separable launch) ahead of the parent's forward
    ("pipe: not stock", dict(ADA, stock=False, fast_draw=False), {}, ("pipe", "small")),
    ("pipe: not stock, theta", dict(ADA, stock=False, fast_draw=False, theta=True), {}, ("pipe", "small")),
    ("pipe: SMALL_PATH off", ADA, dict(SMALL_PATH=False), ("pipe", "arena")),
    ("pipe: SMALL_PATH_128 off", dict(ADA, **NET128), dict(SMALL_PATH_128=False), ("pipe", "arena")),
    ("pipe: B5", dict(ADA, shape=(5, 3, 64, 64)), {}, ("pipe", "arena")),
    ("pipe: B15", dict(ADA, shape=(15, 3, 64, 64)), {}, ("pipe", "arena")),
    ("pipe: grad", dict(ADA, grad=True), {}, ("pipe", "pre")),
    ("sep: B16", dict(ADA, shape=(16, 3, 64, 64)), {}, ("sep", "large")),
    ("sep: B64 at 128", dict(ADA, widths=W128, shape=(64, 3, 128, 128)), {}, ("sep", "large")),
    ("sep: LARGE_PATH off", dict(ADA, shape=(16, 3, 64, 64)), dict(LARGE_PATH=False), ("sep", "arena")),
    ("sep: capturing", dict(ADA, shape=(16, 3, 64, 64), capturing=True), {}, ("sep", "arena")),
    ("no sep: theta", dict(ADA, shape=(16, 3, 64, 64), theta=True), {}, ("pipe", "large")),
    ("no sep: FAST_ADA off", dict(ADA, shape=(16, 3, 64, 64)), dict(FAST_ADA=False), ("pipe", "large")),
    ("no sep: grad", dict(ADA, shape=(16, 3, 64, 64), grad=True), {}, ("pipe", "pre")),
    ("no sep: CPU", dict(ADA, shape=(16, 3, 64, 64), cuda=False), {}, ("pipe", "arena")),
    ("no sep: not stock", dict(ADA, shape=(16, 3, 64, 64), stock=False, fast_draw=False), {}, ("pipe", "large")),
    ("no sep: pinned percentile", dict(ADA, shape=(16, 3, 64, 64), fast_draw=False), {}, ("pipe", "large")),
]


def former_route(f, sw):
    """The conditions as DCDiscriminator.forward / ADADiscriminator.forward nested them before route() existed (`_small_ok`,
    `_plan_ok`, `_forward_nograd`), on the same facts."""
    B, C = f["shape"][0], f["shape"][1]

    def small_ok():
        if not (sw["SMALL_PATH"] and not f["grad"] and f["cuda"] and len(f["shape"]) == 4 and B <= 4 and C <= 4 and f["out_dim"] <= 8):
            return False
        hw, nb = tuple(f["shape"][2:]), len(f["widths"])
        if not ((hw == (64, 64) and nb == 4) or (hw == (128, 128) and nb == 5 and sw["SMALL_PATH_128"])):
            return False
        if list(f["widths"]) != ([64, 128, 256, 512] if nb == 4 else [32, 64, 128, 256, 512]):
            return False
        return C == f["in_dim"] == f["w_in"] and f["weights_ok"]

    def dc_forward():
        if small_ok() and not f["capturing"]:
            return "small"
        if not f["grad"]:
            if sw["LARGE_PATH"] and B >= DM.LARGE_MIN_BATCH and f["cuda"] and not f["capturing"]:
                return "large"
            return "arena"
        return "pre" if sw["PRE_CHAIN"] and f["cuda"] else "lrelu"

    if f.get("stock") is None:
        return None, dc_forward()
    if small_ok() and f["stock"]:
        if f["theta"]:
            return "theta", "small"
        if f["capturing"]:
            return "pipe", dc_forward()
        return ("lib" if sw["FAST_ADA"] and f["fast_draw"] else "host"), "small"
    if (not f["theta"] and sw["FAST_ADA"] and not f["grad"] and f["cuda"] and B >= DM.LARGE_MIN_BATCH and f["stock"] and f["fast_draw"]):
        return "sep", dc_forward()
    return "pipe", dc_forward()


@pytest.mark.parametrize("name,facts,switches,want", ROWS, ids=[r[0] for r in ROWS])
def test_route_truth_table(monkeypatch, name, facts, switches, want):
    f, sw = dict(BASE, **facts), dict(SWITCHES, **switches)
    for k, v in sw.items():
        monkeypatch.setattr(DM.AC if k == "PRE_CHAIN" else DM, k, v)
    assert DM.LARGE_MIN_BATCH == 16
    assert former_route(f, sw) == want
    assert DM.route(**f) == want


def test_route_equals_the_former_conditions_on_every_combination(monkeypatch):
    """Beyond the rows: every combination of the facts' interesting values and of the switches, against the transcription."""
    import itertools
    shapes = [(1, 3, 64, 64), (4, 3, 128, 128), (5, 3, 64, 64), (15, 3, 64, 64), (16, 3, 64, 64), (64, 3, 128, 128), (2, 3, 32, 32)]
    pipes = [dict(stock=None)] + [dict(stock=s, theta=t, fast_draw=s and d) for s, t, d in itertools.product((True, False), repeat=3)]
    n = 0
    for values in itertools.product((True, False), repeat=len(SWITCHES)):
        sw = dict(zip(SWITCHES, values))
        for k, v in sw.items():
            monkeypatch.setattr(DM.AC if k == "PRE_CHAIN" else DM, k, v)
        for shape, widths, grad, cuda, capturing, ok, pipe in itertools.product(shapes, (W64, W128, (8, 16)), (False, True), (True, False),
                                                                                (False, True), (True, False), pipes):
            f = dict(BASE, shape=shape, widths=widths, grad=grad, cuda=cuda, capturing=capturing and cuda, weights_ok=ok, **pipe)
            assert DM.route(**f) == former_route(f, sw), (f, sw)
            n += 1
    assert n == 32 * 7 * 3 * 16 * 9


def test_route_reads_the_facts_of_a_module():
    """`_facts` on CPU modules: the shipped shapes' widths, the channel counts, a non-contiguous weight."""
    D = DM.DCDiscriminator(in_dim=3, out_dim=7, n_feat=512, img_size=128)
    x = torch.zeros(2, 3, 128, 128)
    with torch.no_grad():
        f = D._facts(x)
    assert f == dict(BASE, shape=(2, 3, 128, 128), widths=W128, cuda=False)
    assert D._facts(x)["grad"]
    D.blocks[1].weight = nn.Parameter(D.blocks[1].weight.detach().transpose(2, 3))
    assert not D._facts(x)["weights_ok"]
    D = DM.DCDiscriminator(in_dim=1, out_dim=1, n_feat=512, img_size=64, last_bias=True)
    D.conv_out.bias = nn.Parameter(D.conv_out.bias.detach().double())
    f = D._facts(torch.zeros(1, 1, 64, 64))
    assert (f["widths"], f["in_dim"], f["w_in"], f["out_dim"], f["weights_ok"]) == (W64, 1, 1, 1, False)


def test_live_weights_follow_replaced_parameters():
    """The accessor returns the Parameter objects the modules hold NOW: after an assignment and after
    load_state_dict(assign=True); so do the addresses the plan memo compares."""
    D = DM.DCDiscriminator(in_dim=3, out_dim=1, n_feat=64, img_size=16, last_bias=True)
    ws, wh, bh = D.live_weights()
    assert [w is l.weight for w, l in zip(ws, D.blocks)] == [True, True] and wh is D.conv_out.weight and bh is D.conv_out.bias
    ptrs = DM._weight_ptrs(D)
    assert ptrs == [w.data_ptr() for w in (*ws, wh, bh)]
    new = nn.Parameter(0.5 * ws[0].detach())
    D.blocks[0].weight = new
    assert D.live_weights()[0][0] is new and D.live_weights()[0][1] is ws[1]
    assert DM._weight_ptrs(D) == [new.data_ptr()] + ptrs[1:]
    sd2 = {k: 2.0 * v.detach().clone() for k, v in D.state_dict().items()}
    D.load_state_dict(sd2, assign=True)
    ws2, wh2, bh2 = D.live_weights()
    got = dict(zip(["blocks.0.weight", "blocks.1.weight", "conv_out.weight", "conv_out.bias"], (*ws2, wh2, bh2)))
    for k, v in got.items():
        assert v.data_ptr() == sd2[k].data_ptr() and torch.equal(v, sd2[k]), k
    assert all(a is not b for a, b in zip((*ws2, wh2, bh2), (new, ws[1], wh, bh)))
    assert DM._weight_ptrs(D) == [sd2[k].data_ptr() for k in got]
    # no bias: the slot is skipped, not None
    D0 = DM.DCDiscriminator(in_dim=3, out_dim=1, n_feat=64, img_size=16)
    assert D0.live_weights()[2] is None and len(DM._weight_ptrs(D0)) == 3


def test_stock_pipe_predicate():
    """AugmentPipe.is_stock: the class's own forward, no instance override, 12 taps; fast_draw_ok builds on it."""
    from oi_amd.augment import AugmentPipe
    aug = AugmentPipe(xint=1, scale=1)
    assert aug.is_stock() and aug.fast_draw_ok()
    aug.forward = lambda im: im
    assert not aug.is_stock() and not aug.fast_draw_ok()
    del aug.forward
    aug.Hz_geom = aug.Hz_geom[:10]
    assert not aug.is_stock() and not aug.fast_draw_ok()

    class Other(AugmentPipe):
        def forward(self, images, debug_percentile=None, theta=None):
            return images
    assert not Other(xint=1, scale=1).is_stock()
    rot = AugmentPipe(xint=1, scale=1, rotate=1)
    assert rot.is_stock() and not rot.fast_draw_ok()


def test_ticket_words_match_the_header():
    from oi_amd import lib
    assert int(re.search(r"#define OI_TICKET_WORDS (\d+)", cabi.read("oi_hip.h")).group(1)) == lib.TICKET_WORDS == 4097
