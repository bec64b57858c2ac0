"""GPU: the reverse passes of the KPConv encoder (csrc/kpconv_grad.hip, csrc/groupnorm_grad.hip behind lcrnet_amd.functional, modules/kpconv and
backbone4.KPEncoder) against the fp64 restatements of tests/encoder_grad_restatement.py and fp64 autograd through oracle/torch_ref.

Tolerance rule (R.bound), per output tensor: max|got - g64| <= max(4 e_ref, 2^-20 max|g64|), e_ref being the error of fp32 torch autograd of the
same formula on the same input (computed here, on the CPU).  A bias in front of a GroupNorm has a gradient of exactly zero; both sides are then
rounding noise of a sum whose terms have the size of the layer's weight gradient, so such a bias is held to the scale of that weight gradient.
Exact: the inverted list, rows of unlisted supports, zero dOut rows, run-to-run and alone-versus-stack bytes, a 1 x 1 GroupNorm, y == 0.
Outputs and workspaces are NaN-filled before every call and sit between canaries.

Gradients are discontinuous at a LeakyReLU zero, a max-pool tie and a KPConv row sum of zero.  Every seeded input below keeps each of those
decisions at least R.MARGIN (1e-5) of the tensor's magnitude away from its edge in fp64; the seeds were searched for that (decision_margins()
reports the margins found, tests/test_encoder_grad_cpu.py asserts them without a GPU, the tests here assert them again before comparing).
An encoder of a few hundred points per cloud holds ~3e5 pre-activations, of which ~10 fall inside 1e-5 of the largest whatever the seed: the
clouds of the whole-encoder tests were shrunk until a seed keeps the margin (ENC below).

On the parent commit every test of this file fails: the kernel tests for want of the entry points, the Python-layer tests because the
modules return tensors without a graph."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_grad_restatement as R
from oracle import torch_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
CANARY = 12345.0


# ------------------------------------------------------------------------------------------------ helpers
def guarded(shape, dtype=torch.float32):
    """(whole buffer, NaN-filled view of `shape` between two canary bands); integer views share the float buffer's bytes"""
    n = int(math.prod(shape))
    words = n if dtype in (torch.float32, torch.int32) else (n + 3) // 4
    t = torch.full((words + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
    t[PAD:PAD + words].fill_(float("nan"))
    v = t[PAD:PAD + words]
    if dtype != torch.float32:
        v = v.view(dtype)[:n]
    return t, v.view(*shape)


def intact(*ts):
    return all(bool((t[:PAD] == CANARY).all()) and bool((t[-PAD:] == CANARY).all()) for t in ts)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def leaf(t, dtype):
    """a fresh leaf in `dtype` (never the problem's own tensor: .to() of the same dtype returns its argument)"""
    return t.detach().clone().to(dtype).requires_grad_(True)


def _over(err, e_ref):
    return err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))


def check(label, got, g64, g32, scale=None):
    """print err / tol and err / e_ref, then hold `got` to R.bound"""
    g64 = g64.double()
    err = float((got.double().cpu() - g64).abs().max())
    e_ref = float((g32.double() - g64).abs().max())
    scale = float(g64.abs().max()) if scale is None else scale
    tol = R.bound(e_ref, scale)
    print("%-46s err %.3e  tol %.3e  err/tol %6.3f  err/e_ref %8.3f" % (label, err, tol, err / tol if tol > 0 else 0.0, _over(err, e_ref)))
    assert torch.isfinite(got).all(), label + ": not finite"
    assert err <= tol, (label, err, tol)


def lib():
    from lcrnet_amd import _lib
    return _lib


def fn():
    from lcrnet_amd import functional as F
    return F


def transpose_dev(idx, Ns):
    """lcr_neighbor_transpose into guarded buffers -> (row_start, edges) device int32 views, plus the buffers"""
    L = lib()
    M, H = idx.shape
    d_idx = idx.to(DEV).contiguous()
    t_r, row_start = guarded((Ns + 1,), torch.int32)
    t_e, edges = guarded((max(M * H, 1),), torch.int32)
    nws = L.ws_size("lcr_neighbor_transpose_ws_bytes", M, H)
    t_w, ws = guarded(((nws + 3) // 4,))
    L.call.lcr_neighbor_transpose(L.ptr(d_idx), 1 if idx.dtype == torch.int64 else 0, M, Ns, H, L.ptr(row_start), L.ptr(edges), L.ptr(ws), nws,
                                  L.stream_ptr(torch.device(DEV, 0)))
    torch.cuda.synchronize()
    assert intact(t_r, t_e, t_w), "a canary was overwritten"
    return row_start, edges, (t_r, t_e)


def aggregate_grad_dev(p, dA=None, inv=None):
    L = lib()
    inv = transpose_dev(p.idx, p.Ns) if inv is None else inv
    dA = (p.dA if dA is None else dA).to(DEV).contiguous()
    q, s = p.q.to(DEV), p.s.to(DEV)
    t_o, out = guarded((p.Ns, p.C))
    kp = np.ascontiguousarray(p.kp.numpy(), dtype=np.float32)
    L.call.lcr_kpconv_aggregate_grad(L.ptr(dA), L.ptr(q), L.ptr(s), L.ptr(inv[0]), L.ptr(inv[1]), p.M, p.Ns, p.H, p.C, ctypes.c_void_p(kp.ctypes.data),
                                     float(p.sigma), L.ptr(out), L.stream_ptr(torch.device(DEV, 0)))
    torch.cuda.synchronize()
    assert intact(t_o), "a canary was overwritten"
    return out.cpu()


def aggregate_autograd(p, dtype):
    """torch autograd of A = sum_h w f through the reference's formula (oracle/torch_ref.kpconv's first half), d/d s_feats of <A, dA>"""
    f = torch.zeros(p.Ns, p.C, dtype=dtype, requires_grad=True)
    w, ok, j = R.influences(p.q.to(dtype), p.s.to(dtype), p.idx, p.kp, p.sigma)
    A = torch.matmul(w.transpose(1, 2), f[j] * ok[:, :, None].to(dtype))
    (A.reshape(p.M, -1) * p.dA.to(dtype)).sum().backward()
    return f.grad


KP_CASES = {p.name: p for p in R.kp_cases()}


# ------------------------------------------------------------------------------------------------ the inverted list
@pytest.mark.parametrize("name", list(KP_CASES))
def test_neighbor_transpose_is_exact(name):
    p = KP_CASES[name]
    row_start, edges, _ = transpose_dev(p.idx, p.Ns)
    want_r, want_e = R.neighbor_transpose(p.idx, p.Ns)
    assert row_start.cpu().tolist() == want_r.tolist()
    E = len(want_e)
    assert edges[:E].cpu().tolist() == want_e.tolist()
    assert bool(torch.isnan(edges[E:].view(torch.float32)).all()), "padding entries were written"
    again = transpose_dev(p.idx, p.Ns)
    assert torch.equal(again[0], row_start) and torch.equal(again[1][:E], edges[:E])


# ------------------------------------------------------------------------------------------------ lcr_kpconv_aggregate_grad
@pytest.mark.parametrize("name", list(KP_CASES))
def test_aggregate_grad_matches_fp64(name):
    p = KP_CASES[name]
    got = aggregate_grad_dev(p)
    g64 = R.kpconv_aggregate_grad(p.dA.double(), p.q.double(), p.s.double(), p.idx, p.kp, p.sigma)
    assert (g64 - aggregate_autograd(p, torch.float64)).abs().max() <= 1e-12 * max(1.0, float(g64.abs().max()))
    w, _, _ = R.influences(p.q.double(), p.s.double(), p.idx, p.kp, p.sigma)
    print("%s: %.0f %% of the influences are non-zero" % (name, 100.0 * float((w > 0).double().mean())))
    check(name, got, g64, aggregate_autograd(p, torch.float32))
    assert same_bytes(got, aggregate_grad_dev(p)), "a second run gave other bytes"
    # a support nobody lists gets a row of exact zeros
    listed = torch.zeros(p.Ns, dtype=torch.bool)
    ok = R.valid_mask(p.idx, p.Ns)
    listed[p.idx[ok].long()] = True
    assert bool((got[~listed] == 0).all()) and (name != "hub-300x40x6-c64" or int((~listed).sum()) >= 20)


def test_aggregate_grad_zero_rows_add_nothing():
    """queries whose dA row is zero add exactly what queries that list nobody add: nothing"""
    p = KP_CASES["40x33x65-c64"]
    dA = p.dA.clone()
    dA[::2] = 0.0
    masked = R.KPProblem("masked", p.M, p.Ns, p.H, p.C, 3)
    assert torch.equal(masked.idx, p.idx) and torch.equal(masked.q, p.q)
    masked.idx = p.idx.clone()
    masked.idx[::2] = -1
    assert same_bytes(aggregate_grad_dev(p, dA=dA), aggregate_grad_dev(masked))


def test_aggregate_grad_alone_equals_stack():
    """a cloud's rows have the same bytes alone and as the middle one of a stack of three"""
    parts = [R.KPProblem("a", 21, 17, 19, 64, 31), R.KPProblem("b", 40, 33, 19, 64, 32), R.KPProblem("c", 9, 12, 19, 64, 33)]
    mo = no = 0
    qs, ss, idxs, dAs = [], [], [], []
    total = sum(p.Ns for p in parts)
    for p in parts:
        ok = R.valid_mask(p.idx, p.Ns)
        idxs.append(torch.where(ok, p.idx + no, torch.full_like(p.idx, total)))
        qs.append(p.q), ss.append(p.s), dAs.append(p.dA)
        mo, no = mo + p.M, no + p.Ns
    stack = R.KPProblem("stack", mo, no, 19, 64, 34, idx=torch.cat(idxs))
    stack.q, stack.s, stack.dA = torch.cat(qs), torch.cat(ss), torch.cat(dAs)
    got = aggregate_grad_dev(stack)
    lo = parts[0].Ns
    assert same_bytes(got[lo:lo + parts[1].Ns], aggregate_grad_dev(parts[1]))


def test_aggregate_grad_refuses_outside_its_domain():
    L = lib()
    x = torch.zeros(64, device=DEV)
    kp = np.zeros((15, 3), np.float32)
    for M, Ns, H, C in [(4, 4, 129, 32), (4, 4, 4, 48), (4, 4, 0, 32)]:
        rc = L.lib().lcr_kpconv_aggregate_grad(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), M, Ns, H, C, ctypes.c_void_p(kp.ctypes.data), 0.6, L.ptr(x),
                                               L.stream_ptr(torch.device(DEV, 0)))
        assert rc == -1 and L.lib().lcr_last_error().startswith(b"lcr_kpconv_aggregate_grad:")


# ------------------------------------------------------------------------------------------------ lcr_groupnorm_apply_grad
GN_CASES = {"1x32": (0, 0.0), "37x64": (1, 0.0), "130x128-seg4": (2, 0.0), "200x256-seg2": (3, 0.0), "5x1024": (4, 0.0), "37x64-mean9": (1, 9.0)}
# searched (lowest seed that keeps the margin in all three residual modes); margins found: 3.3e-3, 2.6e-5, 3.0e-5, 1.6e-5, 4.1e-5, 2.6e-5
GN_SEEDS = {"1x32": 0, "37x64": 1, "130x128-seg4": 190, "200x256-seg2": 134, "5x1024": 0, "37x64-mean9": 1}
RES_MODES = ["none", "plain", "norm"]


def gn_problem(name):
    i, mos = GN_CASES[name]
    return R.GNProblem(*R.GN_SHAPES[i], seed=GN_SEEDS[name], mean_over_sigma=mos)


def gn_forward64(p, res_mode, act):
    d = lambda t: t.double()
    return R.groupnorm_apply(d(p.x), d(p.gamma), d(p.beta), p.groups, p.seg, None if res_mode == "none" else d(p.res),
                             (d(p.rgamma), d(p.rbeta)) if res_mode == "norm" else None, 0.1, act)


def gn_margin(p):
    return min(R.relu_margin(gn_forward64(p, m, True)[1]) for m in RES_MODES)


def gn_autograd(p, res_mode, act, dtype):
    t = {k: leaf(getattr(p, k), dtype) for k in ("x", "res", "gamma", "beta", "rgamma", "rbeta")}

    def norm(x, w, b):
        if x.shape[0] * (p.C // p.groups) == 1:          # torch's group_norm refuses one value per group: the same formula, written out
            return R.groupnorm_apply(x, w, b, p.groups, p.seg, act=False)[1]
        return torch_ref.group_norm({"norm.weight": w, "norm.bias": b}, "", x, p.groups, p.seg)

    z = norm(t["x"], t["gamma"], t["beta"])
    if res_mode == "plain":
        z = z + t["res"]
    elif res_mode == "norm":
        z = z + norm(t["res"], t["rgamma"], t["rbeta"])
    y = torch.nn.functional.leaky_relu(z, 0.1) if act else z
    (y * p.dy.to(dtype)).sum().backward()
    zero = lambda k: t[k].grad if t[k].grad is not None else torch.zeros_like(t[k])
    return {"dx": zero("x"), "dgamma": zero("gamma"), "dbeta": zero("beta"), "dres": zero("res"), "drgamma": zero("rgamma"), "drbeta": zero("rbeta")}


def gn_grad_dev(x, stats, gamma, y, dy, groups, seg, act, want_dz):
    """lcr_groupnorm_apply_grad into guarded buffers; tensors on the device"""
    L = lib()
    N, C = x.shape
    seg_len = torch.tensor(seg, dtype=torch.int64).to(DEV)
    S = len(seg)
    nws = L.ws_size("lcr_groupnorm_apply_grad_ws_bytes", N, C, groups, S)
    t_w, ws = guarded(((nws + 3) // 4,))
    t_x, dx = guarded((N, C))
    t_g, dgamma = guarded((C,))
    t_b, dbeta = guarded((C,))
    t_z, dz = guarded((N, C))
    L.call.lcr_groupnorm_apply_grad(L.ptr(x), L.ptr(stats), L.ptr(gamma), L.ptr(y), L.ptr(dy), N, C, groups, L.ptr(seg_len), S, 1e-5, 0.1, int(act), L.ptr(dx),
                                    L.ptr(dgamma), L.ptr(dbeta), L.ptr(dz) if want_dz else None, L.ptr(ws), nws, L.stream_ptr(torch.device(DEV, 0)))
    torch.cuda.synchronize()
    assert intact(t_w, t_x, t_g, t_b, t_z), "a canary was overwritten"
    assert want_dz or bool(torch.isnan(dz).all())
    return dx, dgamma, dbeta, (dz if want_dz else None)


def gn_run_dev(p, res_mode, act, y_override=None):
    """forward through the project's kernels (statistics by lcr_groupnorm_stats), then the reverse pass -> dict of CPU tensors"""
    F = fn()
    dev = lambda t: t.to(DEV).contiguous()
    seg_len = torch.tensor(p.seg, dtype=torch.int64).to(DEV)
    x, res, dy = dev(p.x), dev(p.res), dev(p.dy)
    stats = F.groupnorm_stats(x, p.groups, seg_len)
    rstats = F.groupnorm_stats(res, p.groups, seg_len) if res_mode == "norm" else None
    y = F._groupnorm_apply(x, stats, dev(p.gamma), dev(p.beta), p.groups, seg_len, None if res_mode == "none" else res,
                           (rstats, dev(p.rgamma), dev(p.rbeta)) if res_mode == "norm" else None, 0.1, act)
    if y_override is not None:
        y = dev(y_override)
    dx, dgamma, dbeta, dz = gn_grad_dev(x, stats, dev(p.gamma), y if act else None, dy, p.groups, p.seg, act, res_mode != "none")
    out = {"dx": dx.cpu(), "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu(), "y": y.cpu()}
    if res_mode == "plain":
        out["dres"] = dz.cpu()
    elif res_mode == "norm":
        rx, rg, rb, _ = gn_grad_dev(res, rstats, dev(p.rgamma), None, dz, p.groups, p.seg, False, False)
        out.update(dres=rx.cpu(), drgamma=rg.cpu(), drbeta=rb.cpu())
    return out


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("res_mode", RES_MODES)
@pytest.mark.parametrize("name", list(GN_CASES))
def test_groupnorm_grad_matches_fp64(name, res_mode, act):
    p = gn_problem(name)
    if act:
        margin = R.relu_margin(gn_forward64(p, res_mode, True)[1])
        assert margin >= R.MARGIN, ("decision margin", name, res_mode, margin)
    got = gn_run_dev(p, res_mode, act)
    g64, g32 = gn_autograd(p, res_mode, act, torch.float64), gn_autograd(p, res_mode, act, torch.float32)
    keys = ["dx", "dgamma", "dbeta"] + (["dres"] if res_mode != "none" else []) + (["drgamma", "drbeta"] if res_mode == "norm" else [])
    for k in keys:
        check("%s %s act=%d %s" % (name, res_mode, act, k), got[k], g64[k], g32[k])
    again = gn_run_dev(p, res_mode, act)
    assert all(same_bytes(got[k], again[k]) for k in keys), "a second run gave other bytes"
    if name == "1x32":
        assert bool((got["dx"] == 0).all()), "one value per (segment, group): dx is exactly zero"


def test_groupnorm_grad_zero_output_takes_the_slope():
    p = gn_problem("37x64")
    y = gn_run_dev(p, "plain", True)["y"].clone()
    y[::3, ::5] = 0.0
    y[1::3, 1::5] = -0.0
    got = gn_run_dev(p, "plain", True, y_override=y)["dres"]                  # dres = dz
    want = torch.where(y > 0, p.dy, p.dy * torch.tensor(0.1, dtype=torch.float32))
    assert same_bytes(got, want)


def test_groupnorm_grad_segment_alone_equals_stack():
    p = gn_problem("130x128-seg4")
    whole = gn_run_dev(p, "norm", True)
    o = 0
    for n in p.seg:
        part = R.GNProblem(n, p.C, p.groups, [n])
        for k in ("x", "res", "dy"):
            setattr(part, k, getattr(p, k)[o:o + n].contiguous())
        for k in ("gamma", "beta", "rgamma", "rbeta"):
            setattr(part, k, getattr(p, k))
        alone = gn_run_dev(part, "norm", True)
        assert same_bytes(alone["dx"], whole["dx"][o:o + n]) and same_bytes(alone["dres"], whole["dres"][o:o + n]), n
        o += n


# ------------------------------------------------------------------------------------------------ max-pool, C_in = 1
MP_CASES = {"30x50x66-c64": (30, 50, 66, 64), "17x40x70-c256": (17, 40, 70, 256)}
MP_SEEDS = {"30x50x66-c64": 0, "17x40x70-c256": 2}                     # searched; margins found: 2.5e-4, 4.9e-5


def mp_problem(name):
    M, Ns, H, C = MP_CASES[name]
    p = R.KPProblem(name, M, Ns, H, C, seed=100 + MP_SEEDS[name], pad_frac=0.3)
    p.x = torch.randn(Ns, C, generator=p.gen)
    p.d_out = torch.randn(M, C, generator=p.gen)
    return p


def maxpool_grad_dev(p, x=None):
    L, F = lib(), fn()
    x = (p.x if x is None else x).to(DEV).contiguous()
    idx = p.idx.to(DEV)
    pooled = F._maxpool(x, idx)
    inv = transpose_dev(p.idx, p.Ns)
    t_w, win = guarded((p.M * p.C,), torch.uint8)
    t_x, dx = guarded((p.Ns, p.C))
    d_out = p.d_out.to(DEV)
    L.call.lcr_maxpool_grad(L.ptr(d_out), L.ptr(x), L.ptr(pooled), L.ptr(idx), 0, L.ptr(inv[0]), L.ptr(inv[1]), p.M, p.Ns, p.H, p.C, L.ptr(win), L.ptr(dx),
                            L.stream_ptr(torch.device(DEV, 0)))
    torch.cuda.synchronize()
    assert intact(t_w, t_x), "a canary was overwritten"
    return dx.cpu(), pooled.cpu()


@pytest.mark.parametrize("name", list(MP_CASES))
def test_maxpool_grad_matches_fp64(name):
    p = mp_problem(name)
    margin = R.maxpool_margin(p.x, p.idx)
    assert margin >= R.MARGIN, ("decision margin", name, margin)
    got, pooled = maxpool_grad_dev(p)
    assert torch.equal(pooled, R.maxpool_winners(p.x, p.idx)[1])
    g64 = R.maxpool_grad(p.d_out.double(), p.x.double(), p.idx)
    xr = p.x.clone().requires_grad_(True)
    (torch_ref.maxpool(xr, R.to_ref_idx(p.idx, p.Ns)) * p.d_out).sum().backward()
    check(name, got, g64, xr.grad)
    assert same_bytes(got, maxpool_grad_dev(p)[0]), "a second run gave other bytes"
    # all-negative features under rows that hold padding: the shadow zero owns every maximum of those rows, their gradient goes nowhere
    neg = -p.x.abs() - 0.5
    q = mp_problem(name)
    q.idx[:, -1] = -1
    got_neg, pooled_neg = maxpool_grad_dev(q, x=neg)
    assert bool((pooled_neg == 0).all()) and bool((got_neg == 0).all())


CIN1_CASES = {"40x33x66-o64": (40, 33, 66, 64), "21x30x70-o256": (21, 30, 70, 256)}


def cin1_problem(name):
    M, Ns, H, Cout = CIN1_CASES[name]
    p = R.KPProblem(name, M, Ns, H, 1, seed=200 + Cout)
    p.f = torch.randn(Ns, 1, generator=p.gen)                                   # about half of the supports count as neighbours (f > 0)
    p.W = torch.randn(15, 1, Cout, generator=p.gen) / 15 ** 0.5
    p.d_out = torch.randn(M, Cout, generator=p.gen)
    return p


def cin1_autograd(p, dtype):
    f, W = leaf(p.f, dtype), leaf(p.W, dtype)
    b = torch.zeros(p.W.shape[-1], dtype=dtype, requires_grad=True)
    sd = {"weights": W, "bias": b, "kernel_points": p.kp.to(dtype)}
    (torch_ref.kpconv(sd, "", f, p.q.to(dtype), p.s.to(dtype), R.to_ref_idx(p.idx, p.Ns), p.sigma) * p.d_out.to(dtype)).sum().backward()
    return f.grad, W.grad, b.grad


@pytest.mark.parametrize("name", list(CIN1_CASES))
def test_kpconv_cin1_grad_matches_fp64(name):
    L = lib()
    p = cin1_problem(name)
    margin = R.count_margin(p.f)
    assert margin >= R.MARGIN, ("decision margin", name, margin)
    Cout = p.W.shape[-1]
    inv = transpose_dev(p.idx, p.Ns)
    dev = lambda t: t.to(DEV).contiguous()
    d_out, f, q, s, idx, W = dev(p.d_out), dev(p.f.view(-1)), dev(p.q), dev(p.s), dev(p.idx), dev(p.W)
    kp = np.ascontiguousarray(p.kp.numpy(), dtype=np.float32)
    outs = []
    for want_feats in (True, False):
        nws = L.ws_size("lcr_kpconv_cin1_grad_ws_bytes", p.M, Cout, int(want_feats))
        t_w, ws = guarded(((nws + 3) // 4,))
        t_W, dW = guarded((15, 1, Cout))
        t_b, db = guarded((Cout,))
        t_f, df = guarded((p.Ns,))
        L.call.lcr_kpconv_cin1_grad(L.ptr(d_out), L.ptr(f), L.ptr(q), L.ptr(s), L.ptr(idx), 0, None, L.ptr(inv[0]) if want_feats else None,
                                    L.ptr(inv[1]) if want_feats else None, p.M, p.Ns, p.H, ctypes.c_void_p(kp.ctypes.data), float(p.sigma), L.ptr(W), Cout,
                                    L.ptr(dW), L.ptr(db), L.ptr(df) if want_feats else None, L.ptr(ws), nws, L.stream_ptr(torch.device(DEV, 0)))
        torch.cuda.synchronize()
        assert intact(t_w, t_W, t_b, t_f), "a canary was overwritten"
        assert want_feats or bool(torch.isnan(df).all())
        outs.append((dW.cpu(), db.cpu(), df.cpu()))
    (dW, db, df), (dW2, db2, _) = outs
    assert same_bytes(dW, dW2) and same_bytes(db, db2), "dW / dbias depend on whether d_s_feats was asked for"
    g64 = R.kpconv_grad(p.d_out.double(), p.f.double(), p.q.double(), p.s.double(), p.idx, p.kp, p.sigma, p.W.double())
    a64, a32 = cin1_autograd(p, torch.float64), cin1_autograd(p, torch.float32)
    assert (g64[1] - a64[1]).abs().max() <= 1e-12 * float(a64[1].abs().max())
    check(name + " dW", dW, a64[1], a32[1])
    check(name + " dbias", db, a64[2], a32[2])
    check(name + " d_s_feats", df.view(-1, 1), a64[0], a32[0])


# ------------------------------------------------------------------------------------------------ whole blocks through the Python layer
class Recorder:
    """While active, oracle/torch_ref records the decision margins of an fp64 run: every LeakyReLU input (its distance from zero), every
    LeakyReLU output as a KPConv input would see it (row sums), every max-pool (gap between the two largest distinct candidates)."""

    def __init__(self):
        self.relu, self.count, self.pool = math.inf, math.inf, math.inf

    def __enter__(self):
        rec = self
        self.saved = (torch_ref.F, torch_ref.maxpool)

        class Proxy:
            def __getattr__(self, k):
                return getattr(rec.saved[0], k)

            @staticmethod
            def leaky_relu(x, slope):
                y = rec.saved[0].leaky_relu(x, slope)
                rec.relu = min(rec.relu, R.relu_margin(x.detach()))
                rec.count = min(rec.count, R.count_margin(y.detach()))
                return y

        def maxpool(x, idx):
            xs = x.detach()
            i = torch.where(idx >= xs.shape[0], torch.full_like(idx, -1), idx)
            rec.pool = min(rec.pool, R.maxpool_margin(xs, i))
            return rec.saved[1](x, idx)

        torch_ref.F, torch_ref.maxpool = Proxy(), maxpool
        return self

    def __exit__(self, *exc):
        torch_ref.F, torch_ref.maxpool = self.saved
        return False

    def margin(self):
        return min(self.relu, self.count, self.pool)


BLOCKS = {  # kind, Cin, Cout, M, Ns, H, strided
    "ConvBlock(1,64)": ("conv", 1, 64, 60, 60, 20, False),
    "ResidualBlock(64,128)": ("res", 64, 128, 72, 72, 14, False),       # >= 64 rows: the no-grad forward takes the normalise-on-load GEMM
    "ResidualBlock(128,128,strided)": ("res", 128, 128, 30, 80, 16, True),
}
BLOCK_SEEDS = {"ConvBlock(1,64)": 4, "ResidualBlock(64,128)": 2, "ResidualBlock(128,128,strided)": 0}             # searched; margins found: 2.6e-5, 4.8e-5, 1.5e-4
GROUPS = 32


def block_sd(kind, Cin, Cout, gen):
    """seeded fp32 weights in the checkpoint layout of one block (prefix '')"""
    sd = {}

    def norm(pfx, C):
        sd[pfx + "norm.weight"] = 1 + 0.3 * torch.randn(C, generator=gen)
        sd[pfx + "norm.bias"] = 0.2 * torch.randn(C, generator=gen)

    def unary(pfx, i, o):
        sd[pfx + "mlp.weight"] = torch.randn(o, i, generator=gen) / i ** 0.5
        sd[pfx + "mlp.bias"] = 0.1 * torch.randn(o, generator=gen)
        norm(pfx + "norm.", o)

    def kpconv(i, o):
        sd["KPConv.weights"] = torch.randn(15, i, o, generator=gen) / (15 * i) ** 0.5 * 4
        sd["KPConv.bias"] = 0.1 * torch.randn(o, generator=gen)
        sd["KPConv.kernel_points"] = R.kernel_points()

    if kind == "conv":
        kpconv(Cin, Cout)
        norm("norm.", Cout)
    else:
        mid = Cout // 4
        if Cin != mid:
            unary("unary1.", Cin, mid)
        kpconv(mid, mid)
        norm("norm_conv.", mid)
        unary("unary2.", mid, Cout)
        if Cin != Cout:
            unary("unary_shortcut.", Cin, Cout)
    return sd


class BlockProblem:
    def __init__(self, name):
        self.name = name
        self.kind, self.Cin, self.Cout, M, Ns, H, self.strided = BLOCKS[name]
        p = R.KPProblem(name, M, Ns, H, 1, seed=300 + BLOCK_SEEDS[name], pad_frac=0.2)
        if not self.strided:
            p.q = p.s                                           # queries are the supports themselves
        self.p = p
        self.sd = block_sd(self.kind, self.Cin, self.Cout, p.gen)
        self.feats = torch.randn(Ns, self.Cin, generator=p.gen)
        self.d_out = torch.randn(M, self.Cout, generator=p.gen)

    def reference(self, dtype, record=None):
        """(output, {key: grad}, d_feats) by torch autograd through oracle/torch_ref in `dtype`"""
        p = self.p
        sd = {k: (v.to(dtype) if k.endswith("kernel_points") else leaf(v, dtype)) for k, v in self.sd.items()}
        f = leaf(self.feats, dtype)
        idx = R.to_ref_idx(p.idx, p.Ns)
        if self.kind == "conv":
            out = torch_ref.conv_block(sd, "", f, p.q.to(dtype), p.s.to(dtype), idx, p.sigma, GROUPS)
        else:
            out = torch_ref.residual_block(sd, "", f, p.q.to(dtype), p.s.to(dtype), idx, p.sigma, GROUPS, self.strided)
        (out * self.d_out.to(dtype)).sum().backward()
        return out.detach(), {k: v.grad for k, v in sd.items() if v.requires_grad}, f.grad

    def margin(self):
        with Recorder() as rec:
            self.reference(torch.float64)
        m = rec.margin()
        if self.kind == "conv":
            m = min(m, R.count_margin(self.feats))
        return m

    def module(self):
        from lcrnet_amd.modules.kpconv import ConvBlock, ResidualBlock
        if self.kind == "conv":
            m = ConvBlock(self.Cin, self.Cout, 15, R.RADIUS, R.SIGMA, GROUPS)
        else:
            m = ResidualBlock(self.Cin, self.Cout, 15, R.RADIUS, R.SIGMA, GROUPS, strided=self.strided)
        m.load_state_dict(self.sd, strict=True)
        return m.to(DEV)


def gn_bias_scale(key, g64):
    """a bias whose output feeds a GroupNorm of one channel per group has a zero gradient (the group's mean takes it away): where the fp64
    gradient is zero up to rounding (below 1e-9 of its layer's weight gradient) the bias is held to the scale of that weight gradient
    (module docstring); None = the tensor's own scale"""
    for tail, weight in (("KPConv.bias", "KPConv.weights"), ("mlp.bias", "mlp.weight")):
        if key.endswith(tail):
            w = float(torch.as_tensor(g64[key[:-len(tail)] + weight]).abs().max())
            if float(torch.as_tensor(g64[key]).abs().max()) < 1e-9 * w:
                return w
    return None


def run_block(b):
    """the block's module on the device: (module, output with its graph consumed, feats leaf with .grad)"""
    m = b.module()
    p = b.p
    feats = b.feats.detach().clone().to(DEV).requires_grad_(True)
    out = m(feats, p.q.to(DEV), p.s.to(DEV), p.idx.to(DEV))
    assert out.grad_fn is not None, "the block returned a tensor without a graph"
    (out * b.d_out.to(DEV)).sum().backward()
    return m, out.detach(), feats


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_gradients_match_reference_golden(name):
    """against torch autograd through the IMPORTED reference block (tests/golden/make_golden_encoder_grad.py): max(4 x the reference's own
    fp32-vs-fp64 error, 2^-20 of the scale)"""
    sys.path.insert(0, os.path.join(R.ROOT, "tests", "golden"))
    from make_golden_encoder_grad import load_golden
    gold = load_golden()
    b = BlockProblem(name)
    m, out, feats = run_block(b)
    want = torch.from_numpy(gold[name + "/out"])
    assert float((out.cpu() - want).abs().max() / want.abs().max()) <= 1e-4
    g = {k: torch.from_numpy(gold[name + "/grad/" + k]) for k, _ in m.named_parameters()}
    rows = [(k, prm.grad, g[k], float(gold[name + "/err/" + k]), gn_bias_scale(k, g)) for k, prm in m.named_parameters()]
    rows.append(("feats", feats.grad, torch.from_numpy(gold[name + "/grad_in/feats"]), float(gold[name + "/err/feats"]), None))
    for k, got, ref, e_ref, scale in rows:
        assert got is not None, k + " has no gradient"
        err = float((got.cpu() - ref).abs().max())
        tol = R.bound(e_ref, float(ref.abs().max()) if scale is None else scale)
        print("%-46s err %.3e  tol %.3e  err/tol %6.3f  err/e_ref %8.3f" % (name + " golden " + k, err, tol, err / tol, _over(err, e_ref)))
        assert err <= tol, (k, err, tol)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block_gradients_match_fp64_autograd(name):
    """in training mode (a fresh module's): every parameter and the input get a gradient; in eval mode the forward never carries a graph"""
    from lcrnet_amd.modules.kpconv import modules as kp_modules
    b = BlockProblem(name)
    margin = b.margin()
    assert margin >= R.MARGIN, ("decision margin", name, margin)
    out64, g64, df64 = b.reference(torch.float64)
    out32, g32, df32 = b.reference(torch.float32)
    m, out, feats = run_block(b)
    p = b.p
    q, s, idx = p.q.to(DEV), p.s.to(DEV), p.idx.to(DEV)
    ferr = float((out.detach().cpu().double() - out64).abs().max() / out64.abs().max())
    print("%-46s forward err %.3e (relative)" % (name, ferr))
    assert ferr <= 1e-4, ("forward", ferr)
    for k, prm in m.named_parameters():
        assert prm.grad is not None, k + " has no gradient"
        check(name + " " + k, prm.grad, g64[k], g32[k], scale=gn_bias_scale(k, g64))
    check(name + " d_feats", feats.grad, df64, df32)
    # eval mode builds no graph even with grad mode on and everything requiring grad (as before this module tree was differentiable)
    m.eval()
    quiet = m(feats, q, s, idx)
    assert quiet.grad_fn is None and not quiet.requires_grad
    m.train()
    # the no-grad forward: no graph, and the bytes of the training forward once the normalise-on-load GEMM is switched off as well
    with torch.no_grad():
        plain = m(feats, q, s, idx)
        assert plain.grad_fn is None and not plain.requires_grad
        saved = kp_modules._NO_NORM_ON_LOAD
        kp_modules._NO_NORM_ON_LOAD = True
        try:
            unfused = m(feats, q, s, idx)
        finally:
            kp_modules._NO_NORM_ON_LOAD = saved
    assert same_bytes(unfused, out.detach()), "the training forward differs from the unfused no-grad forward"
    assert same_bytes(quiet, plain), "the eval-mode forward differs from the no-grad forward"
    err = float((plain - out.detach()).abs().max() / out.detach().abs().max())
    assert err <= 1e-4, ("the no-grad forward left the forward tolerance", err)


# ------------------------------------------------------------------------------------------------ the whole KPEncoder
# searched: seed 34 is the first of 60 that keeps the margin (1.08e-5) at 20 + 16 points (stages of 36, 29, 14 and 7 rows, ~4e4 pre-activations);
# no seed below 60 does at 40 + 32 points
ENC = dict(seed=34, points=(20, 16), box=(3.0, 3.0, 1.2), weights_seed=7351)
LIMITS = [12, 12, 12, 12]


def encoder_clouds():
    gen = torch.Generator().manual_seed(400 + ENC["seed"])
    return [(torch.rand(n, 3, generator=gen) * torch.tensor(ENC["box"])).float().numpy() for n in ENC["points"]]


def encoder_inputs():
    """(data dict of CPU tensors from the oracle's collate, per-stage lengths)"""
    from oracle import ops as oracle_ops
    clouds = encoder_clouds()
    xyz = np.concatenate(clouds)
    lens = np.array([len(c) for c in clouds], dtype=np.int64)
    st = oracle_ops.precompute_data_stack_mode(xyz, lens, 4, 0.3, R.RADIUS, LIMITS)
    dd = {k: [torch.from_numpy(np.ascontiguousarray(t)) for t in v] for k, v in st.items()}
    return dd, [[int(v) for v in l] for l in dd["lengths"]]


def encoder_state():
    from lcrnet_amd.backbone4 import KPEncoder
    from lcrnet_amd.weights import seeded_state_dict
    enc = KPEncoder(1, 64, 15, R.RADIUS, R.SIGMA, GROUPS)
    enc.load_state_dict(seeded_state_dict(enc.state_dict(), ENC["weights_seed"]), strict=True)
    return enc


def encoder_target(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(401)) / shape[0]


def encoder_reference(sd, dd, lengths, dtype, record=False):
    sd = {"encoder." + k: v.detach().to(dtype).requires_grad_(v.dtype.is_floating_point and not k.endswith("kernel_points")) for k, v in sd.items()}
    d = {k: [t.to(dtype) if t.dtype.is_floating_point else t for t in v] for k, v in dd.items()}
    feats = torch.ones(d["points"][0].shape[0], 1, dtype=dtype)
    f = torch_ref.kp_encoder(sd, feats, d, init_sigma=R.SIGMA, groups=GROUPS, segment_lengths=lengths)
    loss = (f[-1] * encoder_target(f[-1].shape).to(dtype)).sum()
    loss.backward()
    return loss.detach(), [t.detach() for t in f], {k[len("encoder."):]: v.grad for k, v in sd.items() if v.requires_grad}


def encoder_margin():
    dd, lengths = encoder_inputs()
    with Recorder() as rec:
        encoder_reference(encoder_state().state_dict(), dd, lengths, torch.float64)
    return rec.margin()


def encoder_device_inputs():
    """the same clouds through the project's own collate (precompute_batch: per-cloud GroupNorm segments), checked against the oracle's lists"""
    from lcrnet_amd.data import precompute_batch
    clouds = encoder_clouds()
    pts = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    lens = torch.tensor([len(c) for c in clouds], device=DEV)
    d = precompute_batch(pts.contiguous(), lens, 4, 0.3, R.RADIUS, LIMITS)
    dd, lengths = encoder_inputs()
    for i in range(4):
        assert torch.equal(d["points"][i].cpu(), dd["points"][i]) and torch.equal(d["neighbors"][i].cpu().long(), dd["neighbors"][i].long())
    for i in range(3):
        assert torch.equal(d["subsampling"][i].cpu().long(), dd["subsampling"][i].long())
    assert d["lengths_host"] == lengths
    return d, dd, lengths


def test_encoder_gradients_match_fp64_autograd():
    from lcrnet_amd.modules.kpconv import modules as kp_modules
    margin = encoder_margin()
    assert margin >= R.MARGIN, ("decision margin", margin)
    d, dd, lengths = encoder_device_inputs()
    enc = encoder_state()
    sd = enc.state_dict()
    loss64, f64, g64 = encoder_reference(sd, dd, lengths, torch.float64)
    loss32, f32, g32 = encoder_reference(sd, dd, lengths, torch.float32)
    enc = enc.to(DEV)
    feats = torch.ones(d["points"][0].shape[0], 1, device=DEV)
    out = enc(feats, d)
    assert out[-1].grad_fn is not None
    (out[-1] * encoder_target(out[-1].shape).to(DEV)).sum().backward()
    for i in range(4):
        ferr = float((out[i].detach().cpu().double() - f64[i]).abs().max() / f64[i].abs().max())
        print("encoder forward stage %d: err %.3e (relative)" % (i, ferr))
        assert ferr <= 1e-4, ("forward", i, ferr)
    for k, prm in enc.named_parameters():
        assert prm.grad is not None, k + " has no gradient"
        if k in g64 and g64[k] is not None:
            check("encoder " + k, prm.grad, g64[k], g32[k], scale=gn_bias_scale(k, g64))
    # the training forward is the module tree with the normalise-on-load GEMM off, bit for bit; the native no-grad forward stays within 1e-4
    with torch.no_grad():
        native = enc(feats, d)
        saved, enc.native = (kp_modules._NO_NORM_ON_LOAD, enc.native), False
        kp_modules._NO_NORM_ON_LOAD = True
        try:
            tree = enc(feats, d)
        finally:
            kp_modules._NO_NORM_ON_LOAD, enc.native = saved
    for i in range(4):
        assert native[i].grad_fn is None
        assert same_bytes(tree[i], out[i].detach()), "stage %d: the training forward differs from the unfused module tree" % i
        err = float((native[i] - out[i].detach()).abs().max() / out[i].detach().abs().max())
        assert err <= 1e-4, (i, err)


def reference_training(sd, dd, lengths, steps):
    """the losses of `steps` steps of the same run through oracle/torch_ref and the torch form of Adan, fp32 on the CPU"""
    from lcrnet_amd.adan import Adan
    sd = {"encoder." + k: v.detach().clone().float() for k, v in sd.items()}
    params = [v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and not k.endswith("kernel_points")]
    opt = Adan(params, lr=2e-3, fused=False)
    feats = torch.ones(dd["points"][0].shape[0], 1)
    losses = []
    for _ in range(steps):
        f = torch_ref.kp_encoder(sd, feats, dd, init_sigma=R.SIGMA, groups=GROUPS, segment_lengths=lengths)
        loss = (f[-1] * encoder_target(f[-1].shape)).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_encoder_trains():
    """20 steps of a seeded scalar on the coarse features -> backward() -> fused Adan: the loss falls, and the first step's loss is the one
    oracle/torch_ref computes (1e-4 relative, the forward's tolerance).  The next four losses follow the same run through torch_ref and the
    torch form of the optimiser on the CPU within 1 %: the first Adan update is lr * sign(g), so a step taken on stale derived weights (the
    transposed / split forms cached per weight version) or with a wrong gradient sign moves the second loss by tens of percent (measured
    -42.05 against -185.11 while the fused step did not advance the parameters' version counters)."""
    from lcrnet_amd.adan import Adan
    d, dd, lengths = encoder_device_inputs()
    enc = encoder_state()
    loss_ref = float(encoder_reference(enc.state_dict(), dd, lengths, torch.float32)[0])
    ref_losses = reference_training(enc.state_dict(), dd, lengths, 5)
    enc = enc.to(DEV)
    opt = Adan(enc.parameters(), lr=2e-3, fused=True)
    feats = torch.ones(d["points"][0].shape[0], 1, device=DEV)
    target = None
    losses = []
    for step in range(20):
        out = enc(feats, d)[-1]
        target = encoder_target(out.shape).to(DEV) if target is None else target
        loss = (out * target).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print("training losses: " + " ".join("%.5f" % v for v in losses))
    assert all(math.isfinite(v) for v in losses)
    print("torch_ref losses: " + " ".join("%.5f" % v for v in ref_losses))
    assert abs(losses[0] - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref)), (losses[0], loss_ref)
    for k in range(1, 5):
        assert abs(losses[k] - ref_losses[k]) <= 1e-2 * abs(ref_losses[k]), (k, losses[k], ref_losses[k])
    assert losses[-1] < losses[0], "the loss did not fall"


# ------------------------------------------------------------------------------------------------ the margins of every seeded input (CPU)
def decision_margins():
    """{input: margin found} for every seeded input of this file whose gradient has a decision in it (no GPU needed)"""
    out = {}
    for name in GN_CASES:
        out["groupnorm " + name] = gn_margin(gn_problem(name))
    for name in MP_CASES:
        p = mp_problem(name)
        out["maxpool " + name] = R.maxpool_margin(p.x, p.idx)
    for name in CIN1_CASES:
        out["cin1 " + name] = R.count_margin(cin1_problem(name).f)
    for name in BLOCKS:
        out["block " + name] = BlockProblem(name).margin()
    out["encoder"] = encoder_margin()
    return out
