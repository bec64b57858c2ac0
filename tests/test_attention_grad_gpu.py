"""GPU: the reverse passes of the 3D-RoFormer (csrc/attention_grad.hip behind lcrnet_amd.functional and modules/thdroformer) against the fp64
restatements of tests/attention_grad_restatement.py, the reference's autograd golden of the whole transformer, and one short training run.

Tolerance rule (R.bound), per output tensor: max|got - g64| <= max(4 e_ref, 2^-20 max|g64|), e_ref being the error of fp32 torch autograd through
the reference's formula on the same input (computed here, on the CPU).  Exact: one key (dq = dk = 0, dv = d_out), zero d_out rows -> zero dq
rows, run-to-run and alone-versus-batch bytes.  Outputs and workspace are NaN-filled before every call and sit between canaries.

On the parent commit every test of this file fails: the kernel tests for want of the entry points, the Python-layer tests because the ops
return no graph (grad_fn is None / .grad is None)."""
import ctypes
import math
import os
import sys

import pytest
import torch

import attention_grad_restatement as R
from lcrnet_amd import _lib
from lcrnet_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
CANARY = 12345.0
HEADS = 4
W = HEADS * 32

# (Nq, Nk) or stacked problems; q scale
ATT_CASES = {
    "1x1": ([1], [1], 1.0), "5x7": ([5], [7], 1.0), "33x65": ([33], [65], 1.0), "32x128": ([32], [128], 1.0), "70x129": ([70], [129], 1.0),
    "300x277": ([300], [277], 1.0), "33x65-peaked": ([33], [65], 8.0), "ragged3": ([1, 40, 131], [3, 129, 64], 1.0),
    "p64": ([1 + i % 9 for i in range(64)], [1 + (i + 4) % 9 for i in range(64)], 1.0),
}


def guarded(shape, fill=float("nan")):
    n = int(math.prod(shape))
    t = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
    v = t[PAD:PAD + n]
    v.fill_(fill)
    return t, v.view(*shape)


def intact(t):
    return bool((t[:PAD] == CANARY).all()) and bool((t[-PAD:] == CANARY).all())


def _over(err, e_ref):
    """err / e_ref for the printed tables (the fp32 reference can be exact: one key, a single row)"""
    return err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))


def same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_attention_grad(q, k, v, d_out, q_lens, k_lens):
    """-> (dq, dk, dv) on the CPU from NaN-filled guarded buffers; `out` is the forward kernel's"""
    qd, kd, vd, gd = (t.cuda().contiguous() for t in (q, k, v, d_out))
    out = F._attention_forward(qd, kd, vd, HEADS, q_lens, k_lens)
    P = len(q_lens)
    nws = (_lib.ws_size("lcr_attention_grad_ws_bytes", q.shape[0], HEADS) + 3) // 4
    t_q, dq = guarded(q.shape)
    t_k, dk = guarded(k.shape)
    t_v, dv = guarded(v.shape)
    t_w, ws = guarded((nws,))
    ql, kl = (ctypes.c_int64 * P)(*q_lens), (ctypes.c_int64 * P)(*k_lens)
    _lib.call.lcr_attention_seg_grad_f32(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), _lib.ptr(out), _lib.ptr(gd), ctypes.cast(ql, ctypes.c_void_p),
                                         ctypes.cast(kl, ctypes.c_void_p), P, HEADS, 32, _lib.ptr(dq), _lib.ptr(dk), _lib.ptr(dv), _lib.ptr(ws), nws * 4,
                                         _lib.stream_ptr(qd.device))
    torch.cuda.synchronize()
    assert intact(t_q) and intact(t_k) and intact(t_v) and intact(t_w), "a canary was overwritten"
    return dq.cpu(), dk.cpu(), dv.cpu()


class AttCase:
    def __init__(self, name):
        self.q_lens, self.k_lens, q_scale = ATT_CASES[name]
        nq, nk = sum(self.q_lens), sum(self.k_lens)
        self.q, self.k, self.v, self.d_out = R.attention_problem(nq, nk, HEADS, seed=1000 + nq + nk, q_scale=q_scale)
        self.want = R.attention_restate(self.q, self.k, self.v, self.d_out, HEADS, self.q_lens, self.k_lens)[1:]
        w32 = R.autograd_attention(self.q, self.k, self.v, self.d_out, HEADS, self.q_lens, self.k_lens, torch.float32)
        self.e_ref = [(a - w).abs().max().item() for a, w in zip(w32, self.want)]
        self.tol = [R.bound(e, w.abs().max().item()) for e, w in zip(self.e_ref, self.want)]
        self.got = run_attention_grad(self.q, self.k, self.v, self.d_out, self.q_lens, self.k_lens)


_CACHE = {}


@pytest.fixture
def att(request):
    """One problem set, its references and the kernel's result per case, made once and shared by the tests (never modified)."""
    if request.param not in _CACHE:
        _CACHE[request.param] = AttCase(request.param)
    return _CACHE[request.param]


@pytest.mark.parametrize("att", list(ATT_CASES), indirect=True)
def test_attention_gradient_within_the_fp32_reference_error(att, request):
    errs = [(g.double() - w).abs().max().item() for g, w in zip(att.got, att.want)]
    print("attention grad %s: err / tol  dq %.3f dk %.3f dv %.3f   (err / e_ref %.2f %.2f %.2f)" % (
        request.node.callspec.id, *[e / t if t > 0 else 0.0 for e, t in zip(errs, att.tol)], *[_over(e, r) for e, r in zip(errs, att.e_ref)]))
    assert all(bool(torch.isfinite(g).all()) for g in att.got)
    for name, e, t in zip(("dq", "dk", "dv"), errs, att.tol):
        assert e <= t, (name, e, t)


def test_one_key_gives_exact_zero_dq_dk_and_dv_equal_to_d_out():
    q, k, v, d_out = R.attention_problem(1, 1, HEADS, seed=2)
    dq, dk, dv = run_attention_grad(q, k, v, d_out, [1], [1])
    assert bool((dq == 0).all()) and bool((dk == 0).all()) and same_bytes(dv, d_out)


@pytest.mark.parametrize("att", ["ragged3", "p64"], indirect=True)
def test_a_problem_alone_equals_its_rows_in_the_batch(att):
    qo = ko = 0
    for p, (nq, nk) in enumerate(zip(att.q_lens, att.k_lens)):
        qs, ks = slice(qo, qo + nq), slice(ko, ko + nk)
        dq, dk, dv = run_attention_grad(att.q[qs], att.k[ks], att.v[ks], att.d_out[qs], [nq], [nk])
        assert same_bytes(dq, att.got[0][qs]) and same_bytes(dk, att.got[1][ks]) and same_bytes(dv, att.got[2][ks]), p
        qo, ko = qo + nq, ko + nk


@pytest.mark.parametrize("att", ["300x277", "ragged3"], indirect=True)
def test_a_second_run_gives_the_same_bytes(att):
    again = run_attention_grad(att.q, att.k, att.v, att.d_out, att.q_lens, att.k_lens)
    assert all(same_bytes(a, b) for a, b in zip(again, att.got))


def test_zero_d_out_rows_give_exactly_zero_dq_rows():
    q, k, v, d_out = R.attention_problem(70, 129, HEADS, seed=5)
    rows = [0, 3, 31, 32, 69]
    d_out[rows] = 0.0
    dq, dk, dv = run_attention_grad(q, k, v, d_out, [70], [129])
    assert bool((dq[rows] == 0).all()) and bool(dq.abs().max() > 0) and bool(torch.isfinite(dk).all()) and bool(torch.isfinite(dv).all())


# ---- rotary ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 37, 300])
def test_rotary_gradient(n):
    g = torch.Generator().manual_seed(n)
    x, theta, dy = torch.randn(n, W, generator=g), torch.randn(n, W // 2, generator=g) * 3.0, torch.randn(n, W, generator=g)
    _, want_dx, want_dt = R.rotary_restate(x, theta, dy)
    a32 = R.autograd_rotary(x, theta, dy, HEADS, torch.float32)
    y = F.rotary_embed_(x.cuda().contiguous(), theta.cuda().contiguous(), HEADS)
    t_x, dx = guarded((n, W))
    t_t, dt = guarded((n, W // 2))
    dyd, thd = dy.cuda().contiguous(), theta.cuda().contiguous()
    _lib.call.lcr_rotary_embed_grad(_lib.ptr(y), _lib.ptr(dyd), _lib.ptr(thd), n, HEADS, _lib.ptr(dx), _lib.ptr(dt), _lib.stream_ptr(y.device))
    torch.cuda.synchronize()
    assert intact(t_x) and intact(t_t)
    for name, got, want, ref in (("dx", dx, want_dx, a32[0]), ("dtheta", dt, want_dt, a32[1])):
        e_ref, err = (ref - want).abs().max().item(), (got.cpu().double() - want).abs().max().item()
        tol = R.bound(e_ref, want.abs().max().item())
        print("rotary grad N=%d %s: err / tol %.3f (err / e_ref %.2f)" % (n, name, err / tol, err / max(e_ref, 1e-300)))
        assert err <= tol, (name, err, tol)


# ---- LayerNorm(a + b) -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1, 32), (37, 32), (1, 128), (37, 128), (1, 1024), (37, 1024), (1000, 128)])
@pytest.mark.parametrize("with_b", [False, True])
def test_add_layernorm_gradient(n, d, with_b):
    g = torch.Generator().manual_seed(n + d)
    a, b = torch.randn(n, d, generator=g), (torch.randn(n, d, generator=g) if with_b else None)
    gamma, beta, dy = 1.0 + 0.3 * torch.randn(d, generator=g), torch.randn(d, generator=g), torch.randn(n, d, generator=g)
    _, w_dx, w_dg, w_db = R.layernorm_restate(a, b, gamma, beta, dy)
    a32 = R.autograd_layernorm(a, b, gamma, beta, dy, 1e-5, torch.float32)
    nws = (_lib.ws_size("lcr_add_layernorm_grad_ws_bytes", n, d) + 3) // 4
    t_x, dx = guarded((n, d))
    t_g, dg = guarded((d,))
    t_b, db = guarded((d,))
    t_w, ws = guarded((nws,))
    ad, bd, gd, dyd = a.cuda(), (b.cuda() if with_b else None), gamma.cuda(), dy.cuda()
    _lib.call.lcr_add_layernorm_grad(_lib.ptr(ad), _lib.ptr(bd), _lib.ptr(gd), _lib.ptr(dyd), n, d, 1e-5, _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db),
                                     _lib.ptr(ws), nws * 4, _lib.stream_ptr(ad.device))
    torch.cuda.synchronize()
    assert intact(t_x) and intact(t_g) and intact(t_b) and intact(t_w)
    first = (dx.cpu().clone(), dg.cpu().clone(), db.cpu().clone())
    for name, got, want, ref in (("dx", dx, w_dx, a32[0]), ("dgamma", dg, w_dg, a32[2]), ("dbeta", db, w_db, a32[3])):
        e_ref, err = (ref - want).abs().max().item(), (got.cpu().double() - want).abs().max().item()
        tol = R.bound(e_ref, want.abs().max().item())
        print("layernorm grad N=%d D=%d b=%s %s: err / tol %.3f (err / e_ref %.2f)" % (n, d, with_b, name, err / tol, err / max(e_ref, 1e-300)))
        assert err <= tol, (name, err, tol)
    dx.fill_(float("nan")), dg.fill_(float("nan")), db.fill_(float("nan")), ws.fill_(float("nan"))
    _lib.call.lcr_add_layernorm_grad(_lib.ptr(ad), _lib.ptr(bd), _lib.ptr(gd), _lib.ptr(dyd), n, d, 1e-5, _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db),
                                     _lib.ptr(ws), nws * 4, _lib.stream_ptr(ad.device))
    assert all(same_bytes(x.cpu(), y) for x, y in zip((dx, dg, db), first)), "a second run gives the same bytes"


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------
def _check(name, got, want, ref32):
    e_ref, err = (ref32 - want).abs().max().item(), (got.detach().cpu().double() - want).abs().max().item()
    tol = R.bound(e_ref, want.abs().max().item())
    print("%s: err / tol %.3f (err / e_ref %.2f)" % (name, err / tol, err / max(e_ref, 1e-300)))
    assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("att", ["70x129", "ragged3"], indirect=True)
def test_functional_attention_is_differentiable(att):
    """Fails without the feature: the output of F.attention had no grad_fn."""
    q, k, v = (t.cuda().requires_grad_() for t in (att.q, att.k, att.v))
    lens = (att.q_lens, att.k_lens) if len(att.q_lens) > 1 else (None, None)
    out = F.attention(q, k, v, HEADS, *lens)
    assert out.grad_fn is not None
    (out * att.d_out.cuda()).sum().backward()
    for got, ref in zip((q.grad, k.grad, v.grad), att.got):
        assert same_bytes(got.cpu(), ref)
    with torch.no_grad():
        plain = F.attention(q, k, v, HEADS, *lens)
    plain2 = F.attention(q.detach(), k.detach(), v.detach(), HEADS, *lens)
    assert plain.grad_fn is None and plain2.grad_fn is None and same_bytes(plain, out.detach()) and same_bytes(plain2, plain)
    with pytest.raises(NotImplementedError, match="cfg.GAT.k"):
        F.attention_topk(q, k, v, HEADS, att.q_lens, att.k_lens, [1] * len(att.q_lens))


def test_functional_rotary_embed_sums_both_theta_contributions():
    n = 37
    g = torch.Generator().manual_seed(3)
    xq, xk, theta = torch.randn(n, W, generator=g), torch.randn(n, W, generator=g), torch.randn(n, W // 2, generator=g) * 3.0
    dyq, dyk = torch.randn(n, W, generator=g), torch.randn(n, W, generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        a, b, t = (z.to(dt).clone().requires_grad_() for z in (xq, xk, theta))
        ((R.rotary_formula(a, t, HEADS) * dyq.to(dt)).sum() + (R.rotary_formula(b, t, HEADS) * dyk.to(dt)).sum()).backward()
        ref[dt] = (a.grad.double(), b.grad.double(), t.grad.double())
    a, b, t = (z.cuda().requires_grad_() for z in (xq, xk, theta))
    ya, yb = F.rotary_embed(a, t, HEADS), F.rotary_embed(b, t, HEADS)
    assert ya.grad_fn is not None and same_bytes(a.detach(), xq.cuda()), "out of place"
    ((ya * dyq.cuda()).sum() + (yb * dyk.cuda()).sum()).backward()
    for name, got, w64, w32 in zip(("dxq", "dxk", "dtheta"), (a.grad, b.grad, t.grad), ref[torch.float64], ref[torch.float32]):
        _check("rotary_embed " + name, got, w64, w32)
    inplace = F.rotary_embed_(xq.cuda().contiguous(), theta.cuda().contiguous(), HEADS)
    with torch.no_grad():
        assert same_bytes(F.rotary_embed(a, t, HEADS), inplace)
    assert same_bytes(ya.detach(), inplace)


# rows below, at and above F.WEIGHT_GRAD_SPLIT_ROWS (dW summed over row chunks from there on; 2100 rows: an uneven last chunk; in = 3: padded)
@pytest.mark.parametrize("n,cin,cout,relu", [(37, 64, 128, False), (45, 3, 128, False), (300, 128, 256, True), (82, 256, 128, False),
                                             (511, 128, 64, False), (512, 128, 128, False), (1023, 128, 64, False), (2100, 64, 32, True),
                                             (1500, 3, 128, False)])
def test_functional_linear_is_differentiable(n, cin, cout, relu):
    g = torch.Generator().manual_seed(n + cin)
    x, w, b, dy = torch.randn(n, cin, generator=g), torch.randn(cout, cin, generator=g) * 0.2, torch.randn(cout, generator=g), torch.randn(n, cout, generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        xs, ws, bs = (z.to(dt).clone().requires_grad_() for z in (x, w, b))
        y = torch.nn.functional.linear(xs, ws, bs)
        ((torch.relu(y) if relu else y) * dy.to(dt)).sum().backward()
        ref[dt] = (xs.grad.double(), ws.grad.double(), bs.grad.double())
    xs, ws, bs = (z.cuda().requires_grad_() for z in (x, w, b))
    y = F.linear(xs, ws, bs, relu=relu)
    assert y.grad_fn is not None
    (y * dy.cuda()).sum().backward()
    for name, got, w64, w32 in zip(("dx", "dW", "db"), (xs.grad, ws.grad, bs.grad), ref[torch.float64], ref[torch.float32]):
        _check("linear %dx%d->%d relu=%s %s" % (n, cin, cout, relu, name), got, w64, w32)
    with torch.no_grad():
        assert same_bytes(F.linear(xs, ws, bs, relu=relu), y.detach())
    first = [t.grad.clone() for t in (xs, ws, bs)]
    xs.grad = ws.grad = bs.grad = None
    (F.linear(xs, ws, bs, relu=relu) * dy.cuda()).sum().backward()
    assert all(same_bytes(a, t.grad) for a, t in zip(first, (xs, ws, bs))), "a second run gives the same bytes"


def test_functional_add_layernorm_is_differentiable():
    n, d = 37, 128
    g = torch.Generator().manual_seed(9)
    a, b, gamma, beta, dy = (torch.randn(n, d, generator=g), torch.randn(n, d, generator=g), 1.0 + 0.3 * torch.randn(d, generator=g),
                             torch.randn(d, generator=g), torch.randn(n, d, generator=g))
    w64 = R.autograd_layernorm(a, b, gamma, beta, dy, 1e-5, torch.float64)
    w32 = R.autograd_layernorm(a, b, gamma, beta, dy, 1e-5, torch.float32)
    ts = [t.cuda().requires_grad_() for t in (a, b, gamma, beta)]
    y = F.add_layernorm(*ts)
    assert y.grad_fn is not None
    (y * dy.cuda()).sum().backward()
    for name, t, x64, x32 in zip(("da", "db", "dgamma", "dbeta"), ts, w64, w32):
        _check("add_layernorm " + name, t.grad, x64, x32)
    with torch.no_grad():
        assert same_bytes(F.add_layernorm(*ts), y.detach())


# ---- the whole transformer against the reference's autograd ---------------------------------------------------------------------------------
def _golden():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_roformer_grad as mg
    return mg, mg.load_golden()


def _golden_model(mg):
    from lcrnet_amd.modules.thdroformer.thdroformer_linear import ThDRoFormer
    from lcrnet_amd.weights import seeded_state_dict
    m = ThDRoFormer(*mg.CONFIG)
    m.load_state_dict(seeded_state_dict(m.state_dict(), mg.SEED), strict=True)
    return m.cuda()


def test_transformer_gradients_against_the_reference_golden():
    """Fails without the feature: every parameter's .grad stayed None."""
    import numpy as np
    mg, gold = _golden()
    arrays = mg.grad_inputs()
    assert np.allclose(gold["input_checksum"], [float(a.astype(np.float64).sum()) for a in arrays], rtol=0, atol=0)
    m = _golden_model(mg)
    p0, p1, f0, f1, c0, c1 = (torch.from_numpy(a).cuda() for a in arrays)
    f0.requires_grad_()
    f1.requires_grad_()
    e0, e1, t0, t1 = m(p0, p1, f0, f1, return_pos_emb=True)
    assert e0.grad_fn is not None and t0.grad_fn is not None and "_native_table" not in m.__dict__, "training takes the module tree"
    mg.scalar(e0, e1, t0, t1, c0, c1).backward()
    # the forward is test_transformer_gpu.py's subject; this only guards against a different model, seed or input (errors of order one)
    for name, got in (("out0", e0), ("out1", e1), ("theta0", t0), ("theta1", t1)):
        assert np.abs(got.detach().cpu().numpy() - gold[name]).max() <= 1e-3 * max(1.0, np.abs(gold[name]).max()), name
    worst = ("", 0.0)
    failed = []
    named = [("grad/" + k, p.grad) for k, p in m.named_parameters()] + [("grad_in/feats0", f0.grad), ("grad_in/feats1", f1.grad)]
    for key, grad in named:
        assert grad is not None, key + " has no .grad"
        want, e_ref = gold[key], float(gold["err/" + key.split("/", 1)[1]])
        tol = R.bound(e_ref, float(np.abs(want).max()))
        err = float(np.abs(grad.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max())
        print("roformer %-62s err / tol %.3f (err / e_ref %.2f)" % (key, err / tol, err / max(e_ref, 1e-300)))
        if err / tol > worst[1]:
            worst = (key, err / tol)
        if not err <= tol:
            failed.append((key, err, tol))
    print("roformer grad golden: worst err / tol %.3f at %s" % (worst[1], worst[0]))
    assert not failed, failed
    # the same forward under no_grad: the native one-call path, the same bytes
    with torch.no_grad():
        n0, n1, u0, u1 = m(p0, p1, f0, f1, return_pos_emb=True)
    assert "_native_table" in m.__dict__ and n0.grad_fn is None and not n0.requires_grad
    assert same_bytes(n0, e0.detach()) and same_bytes(n1, e1.detach()) and same_bytes(u0, t0.detach()) and same_bytes(u1, t1.detach())


def test_transformer_forward_and_backward_do_not_synchronise_with_the_host():
    """torch's sync debug mode raises on any synchronising torch call; that the new entry points only enqueue launches (no copy, no
    allocation, no stream or device wait) is established by reading csrc/attention_grad.hip."""
    mg, _ = _golden()
    m = _golden_model(mg)
    p0, p1, f0, f1, c0, c1 = (torch.from_numpy(a).cuda() for a in mg.grad_inputs())
    pi = torch.full((), math.pi, device=DEV)

    def step():
        e0, e1, t0, t1 = m(p0, p1, f0, f1, return_pos_emb=True)
        ((e0 * c0).sum() + (e1 * c1).sum() + torch.clamp(t0.abs() - pi, min=0).mean()).backward()

    step()                                        # first call: lazy set-up
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


# ---- end to end: transformer -> transport -> gap loss -> backward -> fused Adan -----------------------------------------------------------------
def test_gap_loss_trains_a_small_transformer():
    import lcrnet_amd.losses as L
    import sinkhorn_grad_restatement as RS
    from lcrnet_amd.adan import Adan
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.modules.thdroformer.thdroformer_linear import ThDRoFormer
    from lcrnet_amd.weights import seeded_state_dict
    from oracle import torch_ref
    K, C = 128, 32
    g = torch.Generator().manual_seed(12)
    pts = torch.rand(K, 3, generator=g) * 4.0
    perm = torch.randperm(K, generator=g)
    anc = pts[perm] + 0.01 * torch.randn(K, 3, generator=g)
    f0, f1 = torch.randn(K, 64, generator=g) * 0.5, torch.randn(K, 64, generator=g) * 0.5
    ma, mb = torch.ones(1, K, dtype=torch.bool), torch.ones(1, K, dtype=torch.bool)
    loss_fn = L.gap(make_cfg())
    data = {"transform": torch.eye(4)}
    pts_d, anc_d, f0_d, f1_d, ma_d, mb_d = (t.cuda() for t in (pts, anc, f0, f1, ma, mb))

    def train(dense):
        m = ThDRoFormer(64, C, 128, 4, 1)
        m.load_state_dict(seeded_state_dict(m.state_dict(), 77), strict=True)
        m = m.cuda()
        start = {k: p.detach().clone() for k, p in m.named_parameters()}
        alpha = torch.nn.Parameter(torch.tensor(1.0, device=DEV))
        opt = Adan(list(m.parameters()) + [alpha], lr=1e-3, fused=True)
        losses = []
        for _ in range(20):
            opt.zero_grad()
            if dense:                             # torch autograd through a torch restatement of the layer and of the transport
                e0, e1 = torch_ref.thd_roformer(dict(m.named_parameters()), pts_d, anc_d, f0_d, f1_d, pfx="", heads=4, num_layers=1)
                ms = RS.dense_transport((e0 @ e1.T)[None] / C ** 0.5, ma_d, mb_d, alpha)
            else:
                e0, e1 = m(pts_d, anc_d, f0_d, f1_d)
                ms = F.log_optimal_transport((e0 @ e1.T)[None], ma_d, mb_d, alpha, scale=1.0 / C ** 0.5, iters=100)
            out = {"matching_scores": ms, "pos_node_corr_knn_masks": ma_d, "anc_node_corr_knn_masks": mb_d,
                   "pos_node_corr_knn_points": pts_d[None], "anc_node_corr_knn_points": anc_d[None]}
            loss = loss_fn(out, data)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        # alpha alone would train without the feature (it hangs under _TransportFn, and Adan skips tensors without a .grad): what is shown
        # here is that the transformer's own parameters receive gradients and move.  A key bias of a cross layer shifts every score of a
        # row alike, so its gradient is rounding noise around zero and it need not move.
        for k, p in m.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k + " has no finite .grad"
            assert k.endswith("proj_k.bias") or not torch.equal(p.detach(), start[k]), k + " did not move"
        return losses

    losses, losses_d = train(False), train(True)
    F.check_transport_status()
    print("transformer gap training, native backward : " + " ".join("%.5f" % x for x in losses))
    print("transformer gap training, torch autograd  : " + " ".join("%.5f" % x for x in losses_d))
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
