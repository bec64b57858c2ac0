"""CPU: the fp64 restatements of tests/encoder_grad_restatement.py against fp64 torch autograd through oracle/torch_ref (kpconv, group_norm,
maxpool, conv_block, residual_block), the planted mistakes, the inverted-list restatement, the decision margins of every seeded input of
tests/test_encoder_grad_gpu.py, and the new C ABI entries: declared in the header, exported by the library, refused on CPU tensors by the
Python wrappers.  The last three fail on the parent commit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_grad_restatement as R
from oracle import torch_ref

ROOT = R.ROOT
NEW_ENTRIES = ["lcr_neighbor_transpose_ws_bytes", "lcr_neighbor_transpose", "lcr_kpconv_aggregate_grad", "lcr_kpconv_cin1_grad_ws_bytes",
               "lcr_kpconv_cin1_grad", "lcr_maxpool_grad", "lcr_groupnorm_apply_grad_ws_bytes", "lcr_groupnorm_apply_grad"]
TOL = 1e-12
MOVED = 1e-3          # a planted mistake must move its result by at least this much of max|g|: 1000 x the widest GPU tolerance seen


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def kp_sd(Cin, Cout, gen, dtype=torch.float64):
    return {"KPConv.weights": (torch.randn(15, Cin, Cout, generator=gen) / (15 * Cin) ** 0.5).to(dtype), "KPConv.bias": (0.1 * torch.randn(Cout, generator=gen)).to(dtype),
            "KPConv.kernel_points": R.kernel_points().to(dtype)}


def kp_inputs(p, Cin, dtype=torch.float64):
    gen = torch.Generator().manual_seed(5)
    s_feats = torch.randn(p.Ns, Cin, generator=gen).to(dtype)
    return s_feats, p.q.to(dtype), p.s.to(dtype), gen


@pytest.mark.parametrize("Cin,Cout", [(1, 64), (32, 32), (64, 16)])
def test_kpconv_restatement_equals_autograd(Cin, Cout):
    p = R.KPProblem("cpu", 23, 17, 9, Cin, seed=11)
    s_feats, q, s, gen = kp_inputs(p, Cin)
    sd = kp_sd(Cin, Cout, gen)
    d_out = torch.randn(p.M, Cout, generator=gen).double()
    sf = s_feats.clone().requires_grad_(True)
    W, b = sd["KPConv.weights"].clone().requires_grad_(True), sd["KPConv.bias"].clone().requires_grad_(True)
    out = torch_ref.kpconv({"KPConv.weights": W, "KPConv.bias": b, "KPConv.kernel_points": sd["KPConv.kernel_points"]}, "KPConv.", sf, q, s,
                           R.to_ref_idx(p.idx, p.Ns), p.sigma)
    (out * d_out).sum().backward()
    df, dW, db = R.kpconv_grad(d_out, s_feats, q, s, p.idx, sd["KPConv.kernel_points"], p.sigma, sd["KPConv.weights"])
    assert rel(df, sf.grad) <= TOL and rel(dW, W.grad) <= TOL and rel(db, b.grad) <= TOL
    # planted mistakes
    for kw in (dict(drop_count=True), dict(count_padding=True)):
        df2, dW2, _ = R.kpconv_grad(d_out, s_feats, q, s, p.idx, sd["KPConv.kernel_points"], p.sigma, sd["KPConv.weights"], **kw)
        assert rel(dW2, W.grad) > MOVED, kw
    if Cin > 1:
        df3, _, _ = R.kpconv_grad(d_out, s_feats, q, s, p.idx, sd["KPConv.kernel_points"], p.sigma, sd["KPConv.weights"], transpose_kc=True)
        assert rel(df3, sf.grad) > MOVED


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("res_mode", ["none", "plain", "norm"])
def test_groupnorm_restatement_equals_autograd(act, res_mode):
    p = R.GNProblem(130, 128, 32, [1, 63, 64, 2], seed=3)
    t = {k: getattr(p, k).double().requires_grad_(True) for k in ("x", "res", "gamma", "beta", "rgamma", "rbeta")}
    z = torch_ref.group_norm({"norm.weight": t["gamma"], "norm.bias": t["beta"]}, "", t["x"], p.groups, p.seg)
    if res_mode == "plain":
        z = z + t["res"]
    elif res_mode == "norm":
        z = z + torch_ref.group_norm({"norm.weight": t["rgamma"], "norm.bias": t["rbeta"]}, "", t["res"], p.groups, p.seg)
    y = torch.nn.functional.leaky_relu(z, 0.1) if act else z
    (y * p.dy.double()).sum().backward()
    d = {k: v.detach() for k, v in t.items()}
    y2, z2 = R.groupnorm_apply(d["x"], d["gamma"], d["beta"], p.groups, p.seg, None if res_mode == "none" else d["res"],
                               (d["rgamma"], d["rbeta"]) if res_mode == "norm" else None, 0.1, act)
    assert rel(y2, y.detach()) <= TOL
    kw = dict(res=None if res_mode == "none" else d["res"], res_gamma=d["rgamma"] if res_mode == "norm" else None)
    g = R.groupnorm_apply_grad(d["x"], d["gamma"], y2, p.dy.double(), p.groups, p.seg, 0.1, act, **kw)
    assert rel(g["dx"], t["x"].grad) <= TOL and rel(g["dgamma"], t["gamma"].grad) <= TOL and rel(g["dbeta"], t["beta"].grad) <= TOL
    if res_mode != "none":
        assert rel(g["dres"], t["res"].grad) <= TOL
    if res_mode == "norm":
        assert rel(g["drgamma"], t["rgamma"].grad) <= TOL and rel(g["drbeta"], t["rbeta"].grad) <= TOL
    for m in ("drop_xhat_term", "const_stats") + (("no_slope",) if act else ()):
        bad = R.groupnorm_apply_grad(d["x"], d["gamma"], y2, p.dy.double(), p.groups, p.seg, 0.1, act, **kw, **{m: True})
        assert rel(bad["dx"], t["x"].grad) > MOVED, m


def test_groupnorm_zero_output_takes_the_slope():
    """torch's leaky_relu backward uses x > 0: an element that is exactly zero takes the slope; so does the restatement"""
    z = torch.tensor([[0.0, 1.0, -1.0, 0.0]], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.leaky_relu(z, 0.1).sum().backward()
    assert z.grad.tolist() == [[0.1, 1.0, 0.1, 0.1]]
    y = torch.tensor([[0.0, 1.0, -0.1, 0.0]], dtype=torch.float64)
    x = torch.tensor([[0.3, 1.0, -2.0, 0.7]], dtype=torch.float64)
    g = R.groupnorm_apply_grad(x, torch.ones(4, dtype=torch.float64), y, torch.ones(1, 4, dtype=torch.float64), 1, None, 0.1, True)
    assert g["dz"].tolist() == [[0.1, 1.0, 0.1, 0.1]]


def test_maxpool_restatement_equals_autograd():
    p = R.KPProblem("cpu", 31, 40, 66, 64, seed=12)
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(p.Ns, 64, generator=gen).double()
    assert R.maxpool_margin(x, p.idx) > R.MARGIN
    d_out = torch.randn(p.M, 64, generator=gen).double()
    xr = x.clone().requires_grad_(True)
    out = torch_ref.maxpool(xr, R.to_ref_idx(p.idx, p.Ns))
    (out * d_out).sum().backward()
    first, pooled, _, _ = R.maxpool_winners(x, p.idx)
    assert torch.equal(pooled, out.detach())
    assert rel(R.maxpool_grad(d_out, x, p.idx), xr.grad) <= TOL
    # a support listed twice in one row: torch sends the gradient to one of the two, the planted mistake to both
    idx = torch.tensor([[2, 2, 0], [1, -1, -1]], dtype=torch.int32)
    xs = torch.tensor([[1.0, -1.0], [-3.0, -2.0], [5.0, 4.0]], dtype=torch.float64)
    g = R.maxpool_grad(torch.ones(2, 2, dtype=torch.float64), xs, idx)
    assert g.tolist() == [[0.0, 0.0], [0.0, 0.0], [1.0, 1.0]]            # row 1: the shadow zero owns both maxima -> nowhere
    assert R.maxpool_grad(torch.ones(2, 2, dtype=torch.float64), xs, idx, all_ties=True).tolist() == [[0.0, 0.0], [0.0, 0.0], [2.0, 2.0]]


def test_neighbor_transpose_restatement():
    for p in R.kp_cases():
        row_start, edges = R.neighbor_transpose(p.idx, p.Ns)
        flat = p.idx.reshape(-1).numpy().astype(np.int64)
        ok = (flat >= 0) & (flat < p.Ns)
        assert row_start[0] == 0 and row_start[-1] == ok.sum() == len(edges)
        assert sorted(edges.tolist()) == np.nonzero(ok)[0].tolist()                      # a permutation of the valid entries
        for n in range(p.Ns):
            e = edges[row_start[n]:row_start[n + 1]]
            assert (flat[e] == n).all() and (np.diff(e) > 0).all()                        # the row's own entries, ascending


def block_sd(kind, Cin, Cout, gen, dtype=torch.float64):
    """seeded weights of ConvBlock(Cin, Cout) / ResidualBlock(Cin, Cout) in the checkpoint layout"""
    sd = {}

    def norm(pfx, C):
        sd[pfx + "norm.norm.weight"] = (1 + 0.3 * torch.randn(C, generator=gen)).to(dtype)
        sd[pfx + "norm.norm.bias"] = (0.2 * torch.randn(C, generator=gen)).to(dtype)

    def unary(pfx, i, o):
        sd[pfx + "mlp.weight"] = (torch.randn(o, i, generator=gen) / i ** 0.5).to(dtype)
        sd[pfx + "mlp.bias"] = (0.1 * torch.randn(o, generator=gen)).to(dtype)
        norm(pfx, o)

    def kpconv(pfx, i, o):
        sd[pfx + "weights"] = (torch.randn(15, i, o, generator=gen) / (15 * i) ** 0.5 * 4).to(dtype)
        sd[pfx + "bias"] = (0.1 * torch.randn(o, generator=gen)).to(dtype)
        sd[pfx + "kernel_points"] = R.kernel_points().to(dtype)

    if kind == "conv":
        kpconv("KPConv.", Cin, Cout)
        norm("", Cout)
    else:
        mid = Cout // 4
        if Cin != mid:
            unary("unary1.", Cin, mid)
        kpconv("KPConv.", mid, mid)
        sd["norm_conv.norm.weight"] = (1 + 0.3 * torch.randn(mid, generator=gen)).to(dtype)
        sd["norm_conv.norm.bias"] = (0.2 * torch.randn(mid, generator=gen)).to(dtype)
        unary("unary2.", mid, Cout)
        if Cin != Cout:
            unary("unary_shortcut.", Cin, Cout)
    return sd


def test_block_restatements_compose_to_autograd():
    """conv_block and a strided residual_block written as a chain of the restatements equal fp64 autograd through torch_ref: the pieces fit"""
    p = R.KPProblem("cpu", 29, 41, 12, 32, seed=13)
    gen = torch.Generator().manual_seed(21)
    q, s, idxr = p.q.double(), p.s.double(), R.to_ref_idx(p.idx, p.Ns)
    # ConvBlock(1, 32)
    sd = block_sd("conv", 1, 32, gen)
    f = torch.rand(p.Ns, 1, generator=gen).double() + 0.5
    leaf = {k: v.clone().requires_grad_(k != "KPConv.kernel_points") for k, v in sd.items()}
    d_out = torch.randn(p.M, 32, generator=gen).double()
    (torch_ref.conv_block(leaf, "", f, q, s, idxr, p.sigma, 32) * d_out).sum().backward()
    x = torch_ref.kpconv(sd, "KPConv.", f, q, s, idxr, p.sigma)
    y, _ = R.groupnorm_apply(x, sd["norm.norm.weight"], sd["norm.norm.bias"], 32, None, slope=0.1, act=True)
    g = R.groupnorm_apply_grad(x, sd["norm.norm.weight"], y, d_out, 32, None, 0.1, True)
    _, dW, db = R.kpconv_grad(g["dx"], f, q, s, p.idx, sd["KPConv.kernel_points"], p.sigma, sd["KPConv.weights"])
    assert rel(dW, leaf["KPConv.weights"].grad) <= TOL
    # a bias in front of a GroupNorm has no gradient: both sides are rounding noise, held to the weights' scale
    assert float((db - leaf["KPConv.bias"].grad).abs().max()) <= TOL * float(dW.abs().max())
    assert rel(g["dgamma"], leaf["norm.norm.weight"].grad) <= TOL and rel(g["dbeta"], leaf["norm.norm.bias"].grad) <= TOL
    # strided ResidualBlock(32, 64): unary1 (32 -> 16), KPConv(16), unary2 (16 -> 64), max-pool + shortcut (32 -> 64)
    sd = block_sd("res", 32, 64, gen)
    f = torch.randn(p.Ns, 32, generator=gen).double()
    assert R.maxpool_margin(f, p.idx) > 0                    # no exact tie: fp64 on both sides, nothing else matters here
    leaf = {k: v.clone().requires_grad_(not k.endswith("kernel_points")) for k, v in sd.items()}
    fl = f.clone().requires_grad_(True)
    d_out = torch.randn(p.M, 64, generator=gen).double()
    (torch_ref.residual_block(leaf, "", fl, q, s, idxr, p.sigma, 8, True) * d_out).sum().backward()
    G = 8
    lin = lambda pfx, v: v @ sd[pfx + "mlp.weight"].t() + sd[pfx + "mlp.bias"]
    gn = lambda pfx: (sd[pfx + "norm.weight"], sd[pfx + "norm.bias"])
    u1 = lin("unary1.", f)
    a1, _ = R.groupnorm_apply(u1, *gn("unary1.norm."), G)
    k = torch_ref.kpconv(sd, "KPConv.", a1, q, s, idxr, p.sigma)
    a2, _ = R.groupnorm_apply(k, *gn("norm_conv."), G)
    u2 = lin("unary2.", a2)
    _, pooled, _, _ = R.maxpool_winners(f, p.idx)
    sc = lin("unary_shortcut.", pooled)
    yb, _ = R.groupnorm_apply(u2, *gn("unary2.norm."), G, None, sc, gn("unary_shortcut.norm."), 0.1, True)
    gb = R.groupnorm_apply_grad(u2, gn("unary2.norm.")[0], yb, d_out, G, None, 0.1, True, res=sc, res_gamma=gn("unary_shortcut.norm.")[0])
    assert rel(gb["drgamma"], leaf["unary_shortcut.norm.norm.weight"].grad) <= TOL
    assert rel(gb["dres"].t() @ pooled, leaf["unary_shortcut.mlp.weight"].grad) <= TOL
    d_f = R.maxpool_grad(gb["dres"] @ sd["unary_shortcut.mlp.weight"], f, p.idx)
    assert rel(gb["dx"].t() @ a2, leaf["unary2.mlp.weight"].grad) <= TOL
    gc = R.groupnorm_apply_grad(k, gn("norm_conv.")[0], a2, gb["dx"] @ sd["unary2.mlp.weight"], G, None, 0.1, True)
    assert rel(gc["dgamma"], leaf["norm_conv.norm.weight"].grad) <= TOL
    da1, dW, db = R.kpconv_grad(gc["dx"], a1, q, s, p.idx, sd["KPConv.kernel_points"], p.sigma, sd["KPConv.weights"])
    assert rel(dW, leaf["KPConv.weights"].grad) <= TOL and float((db - leaf["KPConv.bias"].grad).abs().max()) <= TOL * float(dW.abs().max())
    g1 = R.groupnorm_apply_grad(u1, gn("unary1.norm.")[0], a1, da1, G, None, 0.1, True)
    assert rel(g1["dx"].t() @ f, leaf["unary1.mlp.weight"].grad) <= TOL
    d_f = d_f + g1["dx"] @ sd["unary1.mlp.weight"]
    assert rel(d_f, fl.grad) <= TOL


def test_gpu_inputs_keep_their_decision_margins():
    """every seeded input of tests/test_encoder_grad_gpu.py keeps its discontinuous decisions (LeakyReLU zero, max-pool tie, KPConv row sum zero)
    at least MARGIN of the tensor's magnitude away from the edge in fp64"""
    import test_encoder_grad_gpu as G
    report = G.decision_margins()
    assert report, "no margins reported"
    for name, margin in report.items():
        print("margin %-40s %.3e" % (name, margin))
        assert margin >= R.MARGIN, (name, margin)


def test_header_declares_and_library_exports_the_entries():
    from lcrnet_amd import _lib
    with open(os.path.join(ROOT, "include", "lcr_hip.h")) as f:
        sigs = _lib.parse_header(f.read())
    for name in NEW_ENTRIES:
        assert name in sigs, name + " is not declared in include/lcr_hip.h"
    assert os.path.exists(_lib.LIB_PATH), "the library has not been built"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(lcr_\w+)", out))
    for name in NEW_ENTRIES:
        assert name in exported, name + " is not exported by the library"


def test_wrappers_refuse_cpu_tensors():
    from lcrnet_amd import functional as F
    p = R.KPProblem("cpu", 4, 5, 3, 32, seed=1)
    x = torch.randn(5, 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.neighbor_transpose(p.idx, p.Ns)
    inv = (torch.zeros(6, dtype=torch.int32), torch.zeros(12, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        F.kpconv_aggregate_grad(p.dA, p.q, p.s, inv, p.H, p.kp.numpy(), p.sigma)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.kpconv_cin1_grad(torch.randn(4, 64), torch.rand(5), p.q, p.s, p.idx, p.kp.numpy(), p.sigma, torch.randn(15, 1, 64))
    with pytest.raises(RuntimeError, match="GPU only"):
        F.maxpool_grad(torch.randn(4, 32), x, torch.randn(4, 32), p.idx, inv)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.groupnorm_apply_grad(x, torch.zeros(8, 1, 32, 2, dtype=torch.float64), torch.ones(32), x, x, 32)
