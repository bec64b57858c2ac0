"""CPU: the restatements of tests/vote_grad_restatement.py are what the GPU file holds the kernels to, so they are checked here first.

* every hand-written reverse pass equals fp64 torch autograd through the guarded formula, and every planted-mistake switch moves a result
  by far more than any tolerance;
* the reason for the r == 0 convention: the literal formula of oracle/torch_ref.kpconv gives NaN point gradients when a cloud is convolved
  with itself, the guarded one is finite and agrees with central differences;
* the seeded inputs of the GPU file keep every decision (|r - sigma|, every non-planted r, ||o| - R|, LeakyReLU / ReLU inputs, max-pool ties,
  KPConv count rows) at least MARGIN away from its edge in fp64, and satisfy the floor of the vote-encoder input;
* the Python wrappers refuse host tensors, and a C_in = 1 KPConv refuses points that require grad."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vote_grad_restatement as V
from oracle import torch_ref

POINT_CASES = {p.name: p for p in V.points_cases()}


def points_autograd(p, dtype, literal=False):
    """(d_q, d_s) of <A, dA> by autograd; q and s the same tensor: both are the one gradient"""
    f = p.f.to(dtype)
    q = p.q.detach().clone().to(dtype).requires_grad_(True)
    s = q if p.same else p.s.detach().clone().to(dtype).requires_grad_(True)
    A = V.aggregate(f, q, s, p.idx, p.kp, p.sigma, literal)
    (A * p.dA.to(dtype)).sum().backward()
    return q.grad, s.grad


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_points_grad_restatement_equals_autograd(name):
    p = POINT_CASES[name]
    dq, ds = V.kpconv_points_grad(p.dA.double(), p.f.double(), p.q.double(), p.s.double(), p.idx, p.kp, p.sigma)
    aq, as_ = points_autograd(p, torch.float64)
    scale = max(1.0, float(aq.abs().max()))
    if p.same:
        assert float((dq + ds - aq).abs().max()) <= 1e-12 * scale
    else:
        assert float((dq - aq).abs().max()) <= 1e-12 * scale and float((ds - as_).abs().max()) <= 1e-12 * scale
    assert torch.isfinite(dq).all() and torch.isfinite(ds).all()


@pytest.mark.parametrize("switch", ["flip_ds", "drop_inv_r", "transpose_kc"])
def test_points_grad_switches_move_the_result(switch):
    p = POINT_CASES["diff-19x23x17-c256"]
    args = (p.dA.double(), p.f.double(), p.q.double(), p.s.double(), p.idx, p.kp, p.sigma)
    dq, ds = V.kpconv_points_grad(*args)
    bq, bs = V.kpconv_points_grad(*args, **{switch: True})
    moved = max(float((bq - dq).abs().max() / dq.abs().max()), float((bs - ds).abs().max() / ds.abs().max()))
    assert moved > 0.1, (switch, moved)


def test_points_grad_exact_zeros_of_the_cases():
    """an edge beyond the hinge of all 15 kernel points and an unlisted support send exactly nothing"""
    p = POINT_CASES["diff-19x23x17-c256"]
    dq, ds = V.kpconv_points_grad(p.dA.double(), p.f.double(), p.q.double(), p.s.double(), p.idx, p.kp, p.sigma)
    assert bool((dq[0] == 0).all()) and bool((ds[20:] == 0).all()) and float(dq[1:].abs().min()) > 0


def test_literal_formula_is_nan_where_the_guarded_one_is_right():
    """q is s with self edges: sqrt(0) at kernel point 0.  oracle/torch_ref.kpconv (the reference's formula) -> NaN for every point; the
    guarded formula -> finite, and equal to central differences of the (continuous) function"""
    p = POINT_CASES["same-30x30x12-c64"]
    gen = torch.Generator().manual_seed(11)
    sd = {"weights": torch.randn(15, p.C, 8, generator=gen).double(), "kernel_points": p.kp.double()}
    cot = torch.randn(p.M, 8, generator=gen).double()
    idx = V.E.to_ref_idx(p.idx, p.Ns)
    f = p.f.double().abs()                                        # positive rows: the neighbour count is the same constant in both formulas

    x = p.q.double().clone().requires_grad_(True)
    (torch_ref.kpconv(sd, "", f, x, x, idx, p.sigma) * cot).sum().backward()
    assert bool(torch.isnan(x.grad).all()), "the literal formula was expected to give NaN for every point"

    def loss(pts):
        return (V.kpconv(sd, "", f, pts, pts, p.idx, p.sigma) * cot).sum()

    y = p.q.double().clone().requires_grad_(True)
    loss(y).backward()
    assert torch.isfinite(y.grad).all()
    with torch.no_grad():
        assert float((loss(y) - (torch_ref.kpconv(sd, "", f, y, y, idx, p.sigma) * cot).sum()).abs()) <= 1e-12 * float(loss(y).abs())
        h, worst = 1e-6, 0.0
        for m in (0, 7, 29):
            for d in range(3):
                e = torch.zeros_like(y)
                e[m, d] = h
                fd = (loss(y + e) - loss(y - e)) / (2 * h)
                worst = max(worst, float((fd - y.grad[m, d]).abs()))
        assert worst <= 1e-7 * max(1.0, float(y.grad.abs().max())), worst


def test_vote_shift_restatement():
    off, xyz, g = (t.double() for t in V.shift_problem())
    o = off.clone().requires_grad_(True)
    x = xyz.clone().requires_grad_(True)
    (V.vote_shift(x, o, V.SHIFT_RANGE) * g).sum().backward()
    got = V.vote_shift_grad(off, g, V.SHIFT_RANGE)
    assert float((got - o.grad).abs().max()) <= 1e-13 and torch.equal(x.grad, g)
    assert torch.equal(got[8], g[8]) and torch.equal(got[:4], g[:4]), "inside the range and exactly at it: the identity"
    assert float(off.float().norm(dim=1)[8]) == V.SHIFT_RANGE
    bad = V.vote_shift_grad(off, g, V.SHIFT_RANGE, ignore_clip=True)
    assert float((bad - got).abs().max() / got.abs().max()) > 0.1
    assert V.clip_margin(off[:8], V.SHIFT_RANGE) >= V.MARGIN


def test_neighbor_mean_restatement():
    pts, idx, pad, g = V.mean_problem()
    x = pts.double().clone().requires_grad_(True)
    (V.neighbor_mean(x, idx, pad) * g.double()).sum().backward()
    got = V.neighbor_mean_grad(g.double(), idx, pad)
    assert float((got - x.grad).abs().max()) <= 1e-14
    assert bool((got[9:] == 0).all()) and bool((got[5] == g[2].double()).all())          # unlisted votes; the node with one vote
    bad = V.neighbor_mean_grad(g.double(), idx, pad, divide_by_h=True)
    assert float((bad - got).abs().max() / got.abs().max()) > 0.1


@pytest.mark.parametrize("C1,C2", [(256, 512), (512, 256)])
def test_upsample_concat_restatement(C1, C2):
    x, idx, skip, g = (t.double() if t.is_floating_point() else t for t in V.upsample_problem(C1, C2))
    a = x.clone().requires_grad_(True)
    b = skip.clone().requires_grad_(True)
    (V.upsample_concat(a, idx, b) * g).sum().backward()
    dx, dskip = V.upsample_concat_grad(g, idx, x.shape[0], C1)
    assert float((dx - a.grad).abs().max()) <= 1e-13 and torch.equal(dskip, b.grad)
    fan = torch.bincount(idx[:, 0][idx[:, 0] < 6], minlength=6).tolist()
    assert fan[1] == 0 and fan[2] == 1 and fan[0] > 5 and int((idx[:, 0] == 6).sum()) >= 3
    assert bool((dx[1] == 0).all())


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_point_case_margins(name):
    hinge, rmin = POINT_CASES[name].margins()
    assert hinge >= V.MARGIN and rmin >= V.MARGIN, (name, hinge, rmin)


@pytest.mark.parametrize("name", list(V.BLOCKS))
def test_block_problem_margins(name):
    tr = V.BlockPointsProblem(name).margin()
    assert tr.margin() >= V.MARGIN, tr.report()


@pytest.mark.parametrize("pairs", [1, 2])
def test_vote_problem_floor_and_margins(pairs):
    p = V.VoteProblem(pairs)
    lists = p.host_lists()
    with torch.no_grad():
        _, off = V.vote_layer(p.sd, "vote.", p.points_c, p.feats, V.MAX_RANGE)
    assert V.vote_floor(lists, p.lens_c, off), (lists["length"].tolist(), off.norm(dim=1).tolist())
    tr = p.margin(lists)
    print("pairs %d: nodes %s  %s" % (pairs, lists["length"].tolist(), tr.report()))
    assert tr.margin() >= V.MARGIN, tr.report()


def test_vote_encoder_restatement_is_oracle_vote_encoder():
    """the guarded vote encoder is oracle/torch_ref.vote_encoder's function (same values from the same lists)"""
    p = V.VoteProblem(1)
    lists = p.host_lists()
    sd = {k: v.double() for k, v in p.sd.items()}
    with torch.no_grad():
        mine = V.vote_encoder(sd, p.feats.double(), p.points_c.double(), p.lens_c, lists, V.MAX_RANGE)
        pad = p.points_c.shape[0]
        centers = V.neighbor_mean(mine["shifted_points_c"], lists["knn"], pad)
        f = p.feats.double()
        for name, q, s, idx, mult, strided in (("encoder6_1.", centers, p.points_c.double(), lists["sub"], 8, True),
                                               ("encoder6_2.", centers, centers, lists["nb"], 16, False),
                                               ("encoder6_3.", centers, centers, lists["nb"], 16, False)):
            f = torch_ref.residual_block(sd, name, f, q, s, idx, V.SIGMA * mult, V.GROUPS, strided)
        shifted = torch_ref.vote_layer(sd, "vote.", p.points_c.double(), p.feats.double(), V.MAX_RANGE)
    assert float((mine["shifted_points_c"] - shifted).abs().max()) <= 1e-12
    assert float((mine["feats_c"] - f).abs().max()) <= 1e-10 * float(f.abs().max())


@pytest.mark.parametrize("pairs", [1, 2])
def test_decoder_problem_margins(pairs):
    m = V.DecoderProblem(pairs).margin()
    assert m >= V.MARGIN, m


def test_wrappers_refuse_host_tensors():
    from lcrnet_amd import functional as F
    x3, i2 = torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int64)
    calls = [lambda: F.vote_shift(x3, x3, 4.2), lambda: F.vote_shift_grad(x3, x3, 4.2), lambda: F.neighbor_mean(x3, i2, 4),
             lambda: F.neighbor_mean_grad(x3, i2, 4, None), lambda: F.upsample_concat(torch.zeros(4, 8), i2, torch.zeros(4, 8)),
             lambda: F.upsample_concat_grad(torch.zeros(4, 16), i2, 4, 8),
             lambda: F.kpconv_points_grad(torch.zeros(4, 15 * 32), torch.zeros(4, 32), x3, x3, i2, V.kernel_points().numpy(), 0.6)]
    for c in calls:
        with pytest.raises(RuntimeError, match="GPU only"):
            c()
    with pytest.raises(RuntimeError, match="GPU only"):
        F.vote_shift(x3.clone().requires_grad_(True), x3, 4.2)


def test_cin1_kpconv_refuses_points_that_require_grad():
    from lcrnet_amd.modules.kpconv import KPConv
    m = KPConv(1, 8, 15, V.RADIUS, V.SIGMA).train()
    q = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(NotImplementedError, match="in_channels == 1"):
        m.forward_raw(torch.ones(4, 1), q, torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int64))
