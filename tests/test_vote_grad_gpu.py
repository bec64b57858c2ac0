"""GPU: the reverse passes behind the vote encoder and the decoder — lcr_kpconv_points_grad (csrc/kpconv_grad.hip), lcr_vote_shift_grad,
lcr_neighbor_mean_grad, lcr_upsample_concat_grad (csrc/pose_tail.hip) — and the Python layer over them (functional, modules/kpconv,
model_family/LCRNet.Vote_Encoder / KPDecoder) against the fp64 restatements of tests/vote_grad_restatement.py and fp64 autograd through the
guarded-sqrt formula (the r == 0 convention of DESIGN §8) and oracle/torch_ref.kp_decoder.

Tolerance: encoder_grad_restatement.bound, per output tensor: max|got - g64| <= max(4 e_ref, 2^-20 max|g64|), e_ref being the error of fp32
torch autograd of the same formula on the same input (computed here, on the CPU).  A bias in front of a GroupNorm has a gradient of exactly
zero and is held to the scale of its layer's weight gradient, as in tests/test_encoder_grad_gpu.py.  Exact: rows of unlisted supports /
votes / x rows, an edge beyond the hinge, the identity branch of the clip, power-of-two counts, d_skip, run-to-run and alone-versus-stack
bytes.  Outputs and workspaces are NaN-filled before every call and sit between canaries.

The seeded inputs keep every decision at least MARGIN away from its edge in fp64 (tests/test_vote_grad_cpu.py asserts that without a GPU;
the module tests assert it again with the index lists the device computed).  The vote-encoder clouds hold 8 + 6 points (6 + 5 + 5 + 6 for
two pairs): no seed keeps the ReLU margin at 20 + 16 (vote_grad_restatement.VOTE).

On the parent commit the kernel tests fail for want of the entry points, the Python-layer tests because node centres and upsampled
features carry no graph."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_grad_restatement as R
import vote_grad_restatement as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
CANARY = 12345.0


# ------------------------------------------------------------------------------------------------ helpers
def guarded(shape, dtype=torch.float32):
    """(whole buffer, NaN-filled view of `shape` between two canary bands)"""
    n = int(math.prod(shape))
    t = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
    t[PAD:PAD + n].fill_(float("nan"))
    v = t[PAD:PAD + n]
    return t, (v.view(dtype) if dtype != torch.float32 else v).view(*shape)


def intact(*ts):
    return all(bool((t[:PAD] == CANARY).all()) and bool((t[-PAD:] == CANARY).all()) for t in ts)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(label, got, g64, g32, scale=None):
    """print err / tol and err / e_ref, then hold `got` to R.bound"""
    g64 = g64.double()
    err = float((got.double().cpu() - g64).abs().max())
    e_ref = float((g32.double() - g64).abs().max())
    scale = float(g64.abs().max()) if scale is None else scale
    tol = R.bound(e_ref, scale)
    print("%-52s err %.3e  tol %.3e  err/tol %6.3f  err/e_ref %8.3f" % (label, err, tol, err / tol if tol > 0 else 0.0,
                                                                         err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))))
    assert torch.isfinite(got).all(), label + ": not finite"
    assert err <= tol, (label, err, tol)


def gn_bias_scale(key, g64):
    """a bias in front of a GroupNorm of one channel per group has a zero gradient: where the fp64 gradient is zero up to rounding the bias
    is held to the scale of its layer's weight gradient (tests/test_encoder_grad_gpu.py); None = the tensor's own scale"""
    for tail, weight in (("KPConv.bias", "KPConv.weights"), ("mlp.bias", "mlp.weight")):
        if key.endswith(tail):
            w = float(g64[key[:-len(tail)] + weight].abs().max())
            if float(g64[key].abs().max()) < 1e-9 * w:
                return w
    return None


def lib():
    from lcrnet_amd import _lib
    return _lib


def stream():
    return lib().stream_ptr(torch.device(DEV, 0))


def transpose_dev(idx, Ns):
    from lcrnet_amd import functional as F
    return F.neighbor_transpose(idx.to(DEV).contiguous(), Ns)


# ------------------------------------------------------------------------------------------------ lcr_kpconv_points_grad
def points_grad_dev(p, want_q=True, want_s=True):
    L = lib()
    idx = p.idx.to(DEV).contiguous()
    row_start, edges = transpose_dev(p.idx, p.Ns) if want_s else (None, None)
    dA, f, q, s = (t.to(DEV).contiguous() for t in (p.dA, p.f, p.q, p.s))
    if p.same:
        s = q
    t_q, dq = guarded((p.M, 3))
    t_s, ds = guarded((p.Ns, 3))
    nws = L.ws_size("lcr_kpconv_points_grad_ws_bytes", p.M, p.H)
    t_w, ws = guarded(((nws + 3) // 4,))
    kp = np.ascontiguousarray(p.kp.numpy(), dtype=np.float32)
    L.call.lcr_kpconv_points_grad(L.ptr(dA), L.ptr(f), L.ptr(q), L.ptr(s), L.ptr(idx), 1 if idx.dtype == torch.int64 else 0, L.ptr(row_start),
                                  L.ptr(edges), p.M, p.Ns, p.H, p.C, ctypes.c_void_p(kp.ctypes.data), float(p.sigma), L.ptr(dq if want_q else None),
                                  L.ptr(ds if want_s else None), L.ptr(ws if want_s else None), nws if want_s else 0, stream())
    torch.cuda.synchronize()
    assert intact(t_q, t_s, t_w), "a canary was overwritten"
    if not want_q:
        assert bool(torch.isnan(dq).all()), "d_q was written although it was not asked for"
    if not want_s:
        assert bool(torch.isnan(ds).all()) and bool(torch.isnan(ws).all()), "d_s or the workspace was written although d_s was not asked for"
    return dq.cpu(), ds.cpu()


def points_autograd(p, dtype):
    """(d_q, d_s) of <A, dA> by autograd through the guarded formula, q and s as separate leaves (equal values where they are one tensor)"""
    q = p.q.detach().clone().to(dtype).requires_grad_(True)
    s = p.s.detach().clone().to(dtype).requires_grad_(True)
    (V.aggregate(p.f.to(dtype), q, s, p.idx, p.kp, p.sigma) * p.dA.to(dtype)).sum().backward()
    return q.grad, s.grad


POINT_CASES = {p.name: p for p in V.points_cases()}


@pytest.mark.parametrize("name", list(POINT_CASES))
def test_points_grad_matches_fp64(name):
    p = POINT_CASES[name]
    hinge, rmin = p.margins()
    assert hinge >= V.MARGIN and rmin >= V.MARGIN
    dq, ds = points_grad_dev(p)
    q64, s64 = V.kpconv_points_grad(p.dA.double(), p.f.double(), p.q.double(), p.s.double(), p.idx, p.kp, p.sigma)
    a64 = points_autograd(p, torch.float64)
    assert float((q64 - a64[0]).abs().max()) <= 1e-12 * max(1.0, float(q64.abs().max()))
    a32 = points_autograd(p, torch.float32)
    check(name + " d_q", dq, q64, a32[0])
    check(name + " d_s", ds, s64, a32[1])
    again = points_grad_dev(p)
    assert same_bytes(dq, again[0]) and same_bytes(ds, again[1]), "a second run gave other bytes"
    # one output at a time: the same bytes
    assert same_bytes(points_grad_dev(p, want_s=False)[0], dq) and same_bytes(points_grad_dev(p, want_q=False)[1], ds)
    # a support nobody lists, a row of padding only: exact zeros
    ok = R.valid_mask(p.idx, p.Ns)
    listed = torch.zeros(p.Ns, dtype=torch.bool)
    listed[p.idx[ok].long()] = True
    assert bool((ds[~listed] == 0).all()) and bool((dq[~ok.any(1)] == 0).all())
    if name == "diff-19x23x17-c256":                     # the edge beyond the hinge of all 15 kernel points: exact zeros at both ends
        assert int((~listed).sum()) == 2 and bool((dq[0] == 0).all()) and bool((ds[22] == 0).all()) and float(dq[1:].abs().min()) > 0
    if name == "pad-7x5x3-c32":
        assert int((~ok.any(1)).sum()) == 1
    if p.same:                                           # self edges: r == 0 at kernel point 0 contributes exactly nothing, nothing is NaN
        assert bool((p.idx[:, 0].long() == torch.arange(p.M)).all()) and bool((p.kp[0] == 0).all())
        assert torch.isfinite(dq).all() and torch.isfinite(ds).all()
        lone = V.PointsProblem("self-only", p.M, p.Ns, 1, p.C, 3, same=True)
        lone.kp = p.kp.clone()
        lone.kp[1:] += 100.0                             # only kernel point 0 reaches the self edge, at r == 0
        z = points_grad_dev(lone)
        assert bool((z[0] == 0).all()) and bool((z[1] == 0).all())


def test_points_grad_alone_equals_stack():
    """a cloud's rows have the same bytes alone and as the second of a stack of two"""
    a, b = V.PointsProblem("a", 21, 17, 19, 64, 31), V.PointsProblem("b", 40, 33, 19, 64, 32)
    total = a.Ns + b.Ns
    idx = torch.cat([torch.where(R.valid_mask(a.idx, a.Ns), a.idx, torch.full_like(a.idx, total)),
                     torch.where(R.valid_mask(b.idx, b.Ns), b.idx + a.Ns, torch.full_like(b.idx, total))])
    st = V.PointsProblem("stack", a.M + b.M, total, 19, 64, 33, idx=idx)
    st.q, st.s, st.dA, st.f = torch.cat([a.q, b.q]), torch.cat([a.s, b.s]), torch.cat([a.dA, b.dA]), torch.cat([a.f, b.f])
    got, alone = points_grad_dev(st), points_grad_dev(b)
    assert same_bytes(got[0][a.M:], alone[0]) and same_bytes(got[1][a.Ns:], alone[1])


def test_points_grad_domain_and_empty_calls():
    L = lib()
    x = torch.zeros(256, device=DEV)
    kp = np.zeros((15, 3), np.float32)
    n = ctypes.c_size_t(0)
    for M, Ns, H, C in [(4, 4, 129, 32), (4, 4, 4, 48), (4, 4, 0, 32), (1 << 24, 4, 64, 32)]:
        rc = L.lib().lcr_kpconv_points_grad(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), 0, L.ptr(x), L.ptr(x), M, Ns, H, C,
                                            ctypes.c_void_p(kp.ctypes.data), 0.6, L.ptr(x), L.ptr(x), L.ptr(x), 1 << 40, stream())
        assert rc == -1 and L.lib().lcr_last_error().startswith(b"lcr_kpconv_points_grad:")
    assert L.lib().lcr_kpconv_points_grad_ws_bytes(4, 129, ctypes.byref(n)) != 0
    # d_s without the list or with a short workspace, sigma <= 0
    args = lambda rs, ws, nws, sigma: (L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), 0, rs, rs, 2, 2, 2, 32, ctypes.c_void_p(kp.ctypes.data), sigma,
                                       L.ptr(x), L.ptr(x), ws, nws, stream())
    assert L.lib().lcr_kpconv_points_grad(*args(None, L.ptr(x), 1024, 0.6)) != 0
    assert L.lib().lcr_kpconv_points_grad(*args(L.ptr(x), L.ptr(x), 8, 0.6)) != 0
    assert L.lib().lcr_kpconv_points_grad(*args(L.ptr(x), L.ptr(x), 1024, 0.0)) != 0
    torch.cuda.synchronize()
    assert bool((x == 0).all()), "a refused call launched something"
    # M == 0 / Ns == 0: clean calls; the output that has rows is zero
    from lcrnet_amd import functional as F
    e3, ef = torch.zeros(0, 3, device=DEV), torch.zeros(0, 64, device=DEV)
    q, f = torch.randn(5, 3, device=DEV), torch.randn(5, 64, device=DEV)
    kpp = V.kernel_points().numpy()
    empty_list = lambda Ns, E: (torch.zeros(Ns + 1, dtype=torch.int32, device=DEV), torch.zeros(max(E, 1), dtype=torch.int32, device=DEV))
    dq, ds = F.kpconv_points_grad(torch.zeros(0, 15 * 64, device=DEV), f, e3, q, torch.zeros(0, 4, dtype=torch.int32, device=DEV), kpp, 0.6,
                                  empty_list(5, 0))
    assert dq.shape == (0, 3) and bool((ds == 0).all())
    idx = torch.zeros(5, 4, dtype=torch.int32, device=DEV)
    dq, ds = F.kpconv_points_grad(torch.randn(5, 15 * 64, device=DEV), ef, q, e3, idx, kpp, 0.6, empty_list(0, 20))
    assert ds.shape == (0, 3) and bool((dq == 0).all())


# ------------------------------------------------------------------------------------------------ lcr_vote_shift_grad
def test_vote_shift_grad_matches_fp64():
    from lcrnet_amd import functional as F
    L = lib()
    off, xyz, g = V.shift_problem()
    t_o, d_off = guarded(tuple(off.shape))
    off_d, g_d = off.to(DEV), g.to(DEV)
    L.call.lcr_vote_shift_grad(L.ptr(off_d), L.ptr(g_d), off.shape[0], V.SHIFT_RANGE, L.ptr(d_off), stream())
    torch.cuda.synchronize()
    assert intact(t_o)
    got = d_off.cpu()
    g64 = V.vote_shift_grad(off.double(), g.double(), V.SHIFT_RANGE)
    o32 = off.clone().requires_grad_(True)
    (V.vote_shift(xyz, o32, V.SHIFT_RANGE) * g).sum().backward()
    check("vote_shift d_off", got, g64, o32.grad)
    assert same_bytes(got[:4], g[:4]) and same_bytes(got[8:], g[8:]), "inside the range and exactly at it the gradient passes unchanged"
    assert float((got[4:8] - g[4:8]).abs().min()) > 0
    # the forward took the same branches
    fwd = F.vote_shift(xyz.to(DEV), off.to(DEV), V.SHIFT_RANGE).cpu()
    assert same_bytes(fwd[8], xyz[8] + off[8]) and float((fwd[:4] - (xyz[:4] + off[:4])).abs().max()) == 0
    # through the wrapper: d_xyz is the cotangent itself
    x, o = xyz.to(DEV).requires_grad_(True), off.to(DEV).requires_grad_(True)
    (F.vote_shift(x, o, V.SHIFT_RANGE) * g.to(DEV)).sum().backward()
    assert same_bytes(x.grad.cpu(), g) and same_bytes(o.grad.cpu(), got)
    # N = 1 and N = 0
    t_1, d1 = guarded((1, 3))
    off_1, g_1 = off[5:6].to(DEV), g[5:6].to(DEV)
    L.call.lcr_vote_shift_grad(L.ptr(off_1), L.ptr(g_1), 1, V.SHIFT_RANGE, L.ptr(d1), stream())
    torch.cuda.synchronize()
    assert intact(t_1) and same_bytes(d1.cpu(), got[5:6])
    assert L.lib().lcr_vote_shift_grad(None, None, 0, V.SHIFT_RANGE, None, stream()) == 0
    assert L.lib().lcr_vote_shift_grad(None, L.ptr(d1), 1, V.SHIFT_RANGE, L.ptr(d1), stream()) == -1
    assert L.lib().lcr_last_error().startswith(b"lcr_vote_shift_grad:")
    assert F.vote_shift_grad(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV), 4.2).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ lcr_neighbor_mean_grad
def test_neighbor_mean_grad_matches_fp64():
    from lcrnet_amd import functional as F
    L = lib()
    pts, idx, pad, g = V.mean_problem()
    row_start, edges = transpose_dev(idx, pad)
    t_o, d = guarded((pad, 3))
    g_d, idx_d = g.to(DEV), idx.to(DEV)
    L.call.lcr_neighbor_mean_grad(L.ptr(g_d), L.ptr(idx_d), 0, L.ptr(row_start), L.ptr(edges), idx.shape[0], idx.shape[1], pad, L.ptr(d), stream())
    torch.cuda.synchronize()
    assert intact(t_o)
    got = d.cpu()
    g64 = V.neighbor_mean_grad(g.double(), idx, pad)
    x32 = pts.clone().requires_grad_(True)
    (V.neighbor_mean(x32, idx, pad) * g).sum().backward()
    check("neighbor_mean d_pts", got, g64, x32.grad)
    assert bool((got[9:] == 0).all()), "a vote nobody lists gets zeros"
    # one edge and a count that is a power of two: exact (votes 2, 4, 5, 8 of nodes with 4, 2, 1 and 4 votes)
    for vote, node, cnt in ((2, 0, 4.0), (4, 1, 2.0), (5, 2, 1.0), (8, 4, 4.0)):
        assert same_bytes(got[vote], g[node] / cnt), (vote, node)
    # through the wrapper, with the forward
    x = pts.to(DEV).requires_grad_(True)
    out = F.neighbor_mean(x, idx.to(DEV), pad)
    assert same_bytes(out.detach(), F.neighbor_mean(pts.to(DEV), idx.to(DEV), pad))
    (out * g.to(DEV)).sum().backward()
    assert same_bytes(x.grad.cpu(), got)
    bad = torch.zeros(64, device=DEV)
    assert L.lib().lcr_neighbor_mean_grad(L.ptr(bad), L.ptr(bad), 0, L.ptr(bad), L.ptr(bad), 4, 129, 4, L.ptr(bad), stream()) != 0
    assert L.lib().lcr_neighbor_mean_grad(None, None, 0, None, None, 0, 4, 0, None, stream()) == 0


# ------------------------------------------------------------------------------------------------ lcr_upsample_concat_grad
@pytest.mark.parametrize("C1,C2", [(256, 512), (512, 256), (6, 3)])
def test_upsample_concat_grad_matches_fp64(C1, C2):
    from lcrnet_amd import functional as F
    L = lib()
    x, idx, skip, g = V.upsample_problem(C1, C2)
    N, Nx = idx.shape[0], x.shape[0]
    row_start, edges = transpose_dev(idx[:, :1], Nx)
    t_x, dx = guarded((Nx, C1))
    t_s, ds = guarded((N, C2))
    g_d = g.to(DEV)
    L.call.lcr_upsample_concat_grad(L.ptr(g_d), L.ptr(row_start), L.ptr(edges), N, Nx, C1, C2, L.ptr(dx), L.ptr(ds), stream())
    torch.cuda.synchronize()
    assert intact(t_x, t_s)
    got_x, got_s = dx.cpu(), ds.cpu()
    x64, _ = V.upsample_concat_grad(g.double(), idx, Nx, C1)
    a = x.clone().requires_grad_(True)
    (V.upsample_concat(a, idx, skip) * g).sum().backward()
    check("upsample_concat d_x %d+%d" % (C1, C2), got_x, x64, a.grad)
    assert same_bytes(got_s, g[:, C1:].contiguous()), "d_skip is an exact copy"
    assert bool((got_x[1] == 0).all()), "an x row nobody lists gets zeros"
    assert same_bytes(got_x[2], g[8, :C1]), "fan-in 1: an exact copy (row 8 is the only one that lists x row 2)"
    # through the wrapper, with the forward; one output at a time
    xa, sa = x.to(DEV).requires_grad_(True), skip.to(DEV).requires_grad_(True)
    out = F.upsample_concat(xa, idx.to(DEV), sa)
    assert same_bytes(out.detach(), F.upsample_concat(x.to(DEV), idx.to(DEV), skip.to(DEV)))
    (out * g.to(DEV)).sum().backward()
    assert same_bytes(xa.grad.cpu(), got_x) and same_bytes(sa.grad.cpu(), got_s)
    only_x, none_s = F.upsample_concat_grad(g.to(DEV), idx.to(DEV), Nx, C1, want_skip=False)
    assert none_s is None and same_bytes(only_x.cpu(), got_x)
    assert L.lib().lcr_upsample_concat_grad(L.ptr(g_d), None, None, N, Nx, C1, C2, L.ptr(dx), None, stream()) == -1
    assert L.lib().lcr_last_error().startswith(b"lcr_upsample_concat_grad:")
    assert L.lib().lcr_upsample_concat_grad(None, None, None, 0, 0, C1, C2, None, None, stream()) == 0


# ------------------------------------------------------------------------------------------------ KPConv / ResidualBlock: gradients to the points
def block_module(b):
    from lcrnet_amd.modules.kpconv import KPConv, ResidualBlock
    if b.kind == "kpconv":
        m = KPConv(b.Cin, b.Cout, 15, V.RADIUS, V.SIGMA, bias=True)
    else:
        m = ResidualBlock(b.Cin, b.Cout, 15, V.RADIUS, V.SIGMA, V.GROUPS, strided=b.strided)
    m.load_state_dict(b.sd, strict=True)
    return m.to(DEV).train()


@pytest.mark.parametrize("name", list(V.BLOCKS))
def test_block_point_gradients_match_fp64_autograd(name):
    b = V.BlockPointsProblem(name)
    tr = b.margin()
    assert tr.margin() >= V.MARGIN, tr.report()
    out64, g64, df64, dq64, ds64 = b.reference(torch.float64)
    out32, g32, df32, dq32, ds32 = b.reference(torch.float32)
    m, p = block_module(b), b.p
    feats = b.feats.to(DEV).requires_grad_(True)
    q = p.q.to(DEV).requires_grad_(True)
    s = q if p.same else p.s.to(DEV).requires_grad_(True)
    out = m(feats, q, s, p.idx.to(DEV))
    assert out.grad_fn is not None
    ferr = float((out.detach().cpu().double() - out64).abs().max() / out64.abs().max())
    assert ferr <= 1e-4, ("forward", ferr)
    (out * b.d_out.to(DEV)).sum().backward()
    check(name + " d_q_points", q.grad, dq64, dq32)
    if not p.same:
        check(name + " d_s_points", s.grad, ds64, ds32)
    check(name + " d_feats", feats.grad, df64, df32)
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k + " has no gradient"
        check(name + " " + k, prm.grad, g64[k], g32[k], scale=gn_bias_scale(k, g64))
    # points alone requiring grad: the same point gradient bytes, nothing else gets one
    m2 = block_module(b).requires_grad_(False)
    q2 = p.q.to(DEV).requires_grad_(True)
    s2 = q2 if p.same else p.s.to(DEV).requires_grad_(True)
    out2 = m2(b.feats.to(DEV), q2, s2, p.idx.to(DEV))
    assert same_bytes(out2.detach(), out.detach())
    (out2 * b.d_out.to(DEV)).sum().backward()
    assert same_bytes(q2.grad, q.grad)
    # eval mode: plain tensors whatever requires grad
    quiet = m.eval()(feats, q, s, p.idx.to(DEV))
    assert quiet.grad_fn is None and not quiet.requires_grad


# ------------------------------------------------------------------------------------------------ Vote_Encoder
def vote_module(p):
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family.LCRNet import Vote_Encoder
    cfg = make_cfg()
    assert cfg["Vote"]["MAX_TRANSLATE_RANGE"] == V.MAX_RANGE and cfg["Vote"]["NMS_radius"] == 2.4
    m = Vote_Encoder(64, 15, V.RADIUS, V.SIGMA, V.GROUPS, cfg["Vote"], V.VOTE_LIMITS)
    m.load_state_dict(p.sd, strict=True)
    return m.to(DEV)


def device_lists(m, p, dd):
    """the index computations of Vote_Encoder.forward, made once with the module's own operators: dict(mask, length, knn, sub, nb) on the host"""
    from lcrnet_amd import functional as F
    from lcrnet_amd.modules.ops import radius_search
    with torch.no_grad():
        pts, lens = dd["points"][-1], dd["lengths"][-1]
        shifted = m.vote(pts, p.feats.to(DEV))
        keep, length = F.greedy_nms(shifted, lens, m.NMS_radius)
        knn = radius_search(shifted[keep.bool()].contiguous(), shifted, length, lens, 2.4, V.VOTE_LIMITS[-1], check=False)
        centers = F.neighbor_mean(shifted, knn, shifted.shape[0])
        sub = radius_search(centers, pts, length, lens, V.RADIUS * 8, V.VOTE_LIMITS[-2], check=False)
        nb = radius_search(centers, centers, length, length, V.RADIUS * 16, V.VOTE_LIMITS[-1], check=False)
    return dict(mask=keep.bool().cpu(), length=length.cpu(), knn=knn.cpu(), sub=sub.cpu(), nb=nb.cpu())


@pytest.mark.parametrize("pairs", [1, 2])
def test_vote_encoder_gradients_match_fp64_autograd(pairs):
    from lcrnet_amd.modules.kpconv import modules as kp_modules
    p = V.VoteProblem(pairs)
    m = vote_module(p).train()
    dd = {"points": [p.points_c.to(DEV)], "lengths": [p.lens_c.to(DEV)]}
    lists = device_lists(m, p, dd)
    with torch.no_grad():
        _, off = V.vote_layer(p.sd, "vote.", p.points_c, p.feats, V.MAX_RANGE)
    assert V.vote_floor(lists, p.lens_c, off), lists["length"].tolist()
    tr = p.margin(lists)
    print("pairs %d: nodes %s  %s" % (pairs, lists["length"].tolist(), tr.report()))
    assert tr.margin() >= V.MARGIN, tr.report()
    out64, g64, df64 = p.reference(torch.float64, lists)
    out32, g32, df32 = p.reference(torch.float32, lists)

    feats = p.feats.to(DEV).requires_grad_(True)
    out = m(feats, dd, pairs=pairs)
    assert torch.equal(out["nms_mask"].bool().cpu(), lists["mask"]) and torch.equal(out["length"].cpu(), lists["length"])
    cot = p.cotangents(out["feats_c"].shape[0])
    for k in cot:
        assert out[k].grad_fn is not None, k + " carries no graph"
        err = float((out[k].detach().cpu().double() - out64[k]).abs().max() / out64[k].abs().max())
        assert err <= 1e-4, ("forward", k, err)
    # ctr_reg gets a gradient from feats_c ALONE: through the node centres and KPConv's influence weights
    (g_ctr,) = torch.autograd.grad((out["feats_c"] * cot["feats_c"].to(DEV)).sum(), m.vote.ctr_reg.weight, retain_graph=True, allow_unused=True)
    assert g_ctr is not None and float(g_ctr.abs().max()) > 0
    sum((out[k] * cot[k].to(DEV)).sum() for k in cot).backward()
    check("vote_encoder[%d] d_feats" % pairs, feats.grad, df64, df32)
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k + " has no gradient"
        check("vote_encoder[%d] %s" % (pairs, k), prm.grad, g64[k], g32[k], scale=gn_bias_scale(k, g64))

    # eval mode with grad mode on: plain tensors; its values are the training forward's to the bit once normalise-on-load is off
    m.eval()
    saved = kp_modules._NO_NORM_ON_LOAD
    kp_modules._NO_NORM_ON_LOAD = True
    try:
        quiet = m(feats, dd, pairs=pairs)
    finally:
        kp_modules._NO_NORM_ON_LOAD = saved
    for k in ("feats_c", "points_c", "shifted_points_c"):
        assert quiet[k].grad_fn is None and not quiet[k].requires_grad, k
        assert same_bytes(quiet[k], out[k].detach()), k + ": the training forward differs from the eval forward"


# ------------------------------------------------------------------------------------------------ KPDecoder
@pytest.mark.parametrize("pairs", [1, 2])
def test_decoder_gradients_match_fp64_autograd(pairs):
    from lcrnet_amd.model_family.LCRNet import KPDecoder
    p = V.DecoderProblem(pairs)
    assert p.margin() >= V.MARGIN
    l64, g64, df64 = p.reference(torch.float64)
    l32, g32, df32 = p.reference(torch.float32)
    m = KPDecoder(64, V.GROUPS)
    m.load_state_dict(p.sd, strict=True)
    m = m.to(DEV).train()
    feats = [f.to(DEV).requires_grad_(True) for f in p.feats]
    dd = {"upsampling": [u.to(DEV) for u in p.up], "lengths": [l.to(DEV) for l in p.lengths]}
    l1, l2, l3 = m(feats, dd, pairs=pairs)
    assert l1.grad_fn is not None and l2.grad_fn is not None and l3.grad_fn is not None
    err = float((l1.detach().cpu().double() - l64).abs().max() / l64.abs().max())
    assert err <= 1e-4, ("forward", err)
    (l1 * p.cot.to(DEV)).sum().backward()
    for i, f in enumerate(feats):
        check("decoder[%d] d_f%d" % (pairs, i + 1), f.grad, df64[i], df32[i])
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k + " has no gradient"
        check("decoder[%d] %s" % (pairs, k), prm.grad, g64[k], g32[k], scale=gn_bias_scale(k, g64))
    quiet = m.eval()(feats, dd, pairs=pairs)
    assert all(t.grad_fn is None and not t.requires_grad for t in quiet)
    assert same_bytes(quiet[0], l1.detach()) and same_bytes(quiet[2], l3.detach())
