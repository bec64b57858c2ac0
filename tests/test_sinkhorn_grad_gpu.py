"""GPU: the reverse pass of the transport (csrc/sinkhorn_grad.hip behind lcrnet_amd.functional) against the fp64 restatement of
tests/sinkhorn_grad_restatement.py.

Tolerance rule (R.bound): per problem, max|d_raw - g64| <= max(4 e_ref, 2^-20 max|g64|), e_ref being the error of fp32 torch autograd through
oracle/torch_ref.log_optimal_transport on the same input (computed here, on the CPU); d_alpha the same way with sum|dS| over the valid dustbin
entries as the scale.  Exact: zeros on masked lines, indifference to G on masked lines, zeros for a problem without a valid column, run-to-run
and alone-versus-batch bytes.  Workspace and outputs are NaN-filled before every call and sit between canaries."""
import ctypes

import pytest
import torch

import sinkhorn_grad_restatement as R
from lcrnet_amd import _lib
from lcrnet_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
CANARY = 12345.0
SCALE = 0.5

# (B, M, N), iterations, spread, form: the smallest and the patch shape, the last resident size, the first general size, a general one with
# several column blocks; T = 1 reads v_0; T = 150 at the last resident size records beyond LDS, into the workspace
CASES = {
    "tiny-T1": ((3, 5, 9), 1, 1.0, 0), "tiny-T2": ((3, 5, 9), 2, 1.0, 0), "tiny": ((3, 5, 9), 100, 1.0, 0),
    "patch": ((37, 128, 128), 100, 1.0, 0), "patch-spread8": ((2, 128, 128), 100, 8.0, 0),
    "last-resident": ((2, 131, 131), 100, 1.0, 0), "resident-ws-history": ((2, 131, 131), 150, 1.0, 0),
    "first-general": ((2, 132, 131), 100, 1.0, 1), "general": ((1, 193, 150), 100, 1.0, 1),
}


def guarded(n, fill=float("nan")):
    t = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
    v = t[PAD:PAD + n]
    v.fill_(fill)
    return t, v


def intact(t, n):
    return bool((t[:PAD] == CANARY).all()) and bool((t[PAD + n:] == CANARY).all())


def padded_scores(raw, rm, cm, alpha):
    B, M, N = raw.shape
    S0 = torch.empty((B, M + 1, N + 1), dtype=torch.float32, device=DEV)
    raw_d, alpha_d = raw.cuda().contiguous(), alpha.cuda().reshape(1)      # held until the launch is queued: a temporary's block is reused at once
    _lib.call.lcr_build_padded_scores(_lib.ptr(raw_d), _lib.ptr(rm), _lib.ptr(cm), B, M, N, SCALE, _lib.ptr(alpha_d), 1e12, _lib.ptr(S0),
                                      _lib.stream_ptr(S0.device))
    return S0


def run_native(raw, rm, cm, alpha, G, iters):
    """-> (dS, d_alpha_part) on the CPU, from NaN-filled guarded buffers."""
    B, M, N = raw.shape
    rm8, cm8 = rm.to(torch.uint8).cuda().contiguous(), cm.to(torch.uint8).cuda().contiguous()
    S0 = padded_scores(raw, rm8, cm8, alpha)
    n = B * (M + 1) * (N + 1)
    nws = (_lib.ws_size("lcr_log_sinkhorn_grad_ws_bytes", B, M, N, iters) + 3) // 4
    t_ds, dS = guarded(n)
    t_pa, part = guarded(B)
    t_ws, ws = guarded(nws)
    Gd = G.cuda().contiguous()
    _lib.call.lcr_log_sinkhorn_grad(_lib.ptr(S0), _lib.ptr(Gd), _lib.ptr(rm8), _lib.ptr(cm8), B, M, N, iters, 1e12, _lib.ptr(dS), _lib.ptr(part),
                                    _lib.ptr(ws), nws * 4, _lib.stream_ptr(S0.device))
    torch.cuda.synchronize()
    assert intact(t_ds, n) and intact(t_pa, B) and intact(t_ws, nws), "a canary was overwritten"
    return dS.view(B, M + 1, N + 1).cpu(), part.cpu()


class Case:
    def __init__(self, name):
        (B, M, N), self.iters, spread, self.form = CASES[name]
        self.shape = (B, M, N)
        self.raw, self.rm, self.cm, self.alpha, self.G_raw, self.G, self.V = R.problem(B, M, N, seed=100 + M + self.iters, spread=spread)
        self.d_raw, self.d_alpha, self.dS, self.part = R.restate(self.raw, self.rm, self.cm, self.alpha, SCALE, self.G, self.iters)
        g32, a32 = R.autograd_reference(self.raw, self.rm, self.cm, self.alpha, SCALE, self.G, self.iters, torch.float32)
        self.e_ref = (g32.double() - self.d_raw).abs().flatten(1).max(1)[0]                 # per problem
        self.e_ref_alpha = abs(a32.double().item() - self.d_alpha.item())
        dust = self.dS[:, M, :].abs().sum() + self.dS[:, :M, N].abs().sum()
        self.tol = torch.tensor([R.bound(e.item(), g.item()) for e, g in zip(self.e_ref, self.d_raw.abs().flatten(1).max(1)[0])])
        self.tol_alpha = R.bound(self.e_ref_alpha, dust.item())
        self.got_dS, self.got_part = run_native(self.raw, self.rm, self.cm, self.alpha, self.G, self.iters)


_CACHE = {}


@pytest.fixture
def case(request):
    """One problem set, its references and the kernel's result per case, made once and shared by the tests (never modified)."""
    if request.param not in _CACHE:
        _CACHE[request.param] = Case(request.param)
    return _CACHE[request.param]


@pytest.mark.parametrize("case", list(CASES), indirect=True)
def test_gradient_within_the_fp32_reference_error(case, request):
    B, M, N = case.shape
    form = ctypes.c_int(-1)
    _lib.call.lcr_log_sinkhorn_grad_form(B, M, N, ctypes.byref(form))
    assert form.value == case.form
    err = (case.got_dS[:, :M, :N].double() * SCALE - case.d_raw).abs().flatten(1).max(1)[0]
    err_alpha = abs(case.got_part.double().sum().item() - case.d_alpha.item())
    ratio = (err / case.e_ref.clamp(min=1e-300)).max().item()
    print("sinkhorn grad %s %s T=%d: max err / e_ref %.2f (max err / tol %.2f), d_alpha err / e_ref %.2f (/ tol %.2f)" % (
        request.node.callspec.id, case.shape, case.iters, ratio, (err / case.tol).max().item(), err_alpha / max(case.e_ref_alpha, 1e-300),
        err_alpha / case.tol_alpha))
    assert bool(torch.isfinite(case.got_dS).all()) and bool(torch.isfinite(case.got_part).all())
    assert bool((err <= case.tol).all()), (err / case.tol).max().item()
    assert err_alpha <= case.tol_alpha, (err_alpha, case.tol_alpha)
    assert bool((case.got_dS[~case.V] == 0).all()), "dS is exactly zero on masked lines"


@pytest.mark.parametrize("case", ["tiny-T2", "patch", "first-general"], indirect=True)
def test_planted_mistakes_are_far_outside_the_tolerance(case):
    B, M, N = case.shape
    got_raw, got_alpha = case.got_dS[:, :M, :N].double() * SCALE, case.got_part.double().sum().item()
    shown = 0
    for m in R.MISTAKES:
        if not R.mistake_shows(m, case.iters):
            continue
        Gin = case.G_raw if m == "g_unmasked" else case.G
        w_raw, w_alpha, _, _ = R.restate(case.raw, case.rm, case.cm, case.alpha, SCALE, Gin, case.iters, mistake=m)
        off = ((w_raw - got_raw).abs().flatten(1).max(1)[0] / case.tol).max().item()
        off_alpha = abs(w_alpha.item() - got_alpha) / case.tol_alpha
        print("planted %s: %.1f x tol (d_raw), %.1f x tol (d_alpha)" % (m, off, off_alpha))
        assert max(off, off_alpha) >= 8.0, (m, off, off_alpha)
        shown += 1
    assert shown == (len(R.MISTAKES) if case.iters == 2 else 3)


@pytest.mark.parametrize("case", ["patch", "first-general"], indirect=True)
def test_g_on_masked_lines_is_ignored_and_runs_repeat(case):
    again_dS, again_part = run_native(case.raw, case.rm, case.cm, case.alpha, case.G, case.iters)
    assert torch.equal(again_dS.view(torch.int32), case.got_dS.view(torch.int32)) and torch.equal(again_part.view(torch.int32), case.got_part.view(torch.int32))
    raw_dS, raw_part = run_native(case.raw, case.rm, case.cm, case.alpha, case.G_raw, case.iters)
    assert torch.equal(raw_dS.view(torch.int32), case.got_dS.view(torch.int32)) and torch.equal(raw_part.view(torch.int32), case.got_part.view(torch.int32))
    nan_G = torch.where(case.V, case.G, torch.full_like(case.G, float("nan")))
    nan_dS, _ = run_native(case.raw, case.rm, case.cm, case.alpha, nan_G, case.iters)
    assert torch.equal(nan_dS.view(torch.int32), case.got_dS.view(torch.int32))


@pytest.mark.parametrize("case", ["patch", "first-general"], indirect=True)
def test_a_problem_alone_equals_its_rows_in_the_batch(case):
    b = 5 if case.shape[0] > 5 else 1
    s = slice(b, b + 1)
    dS, part = run_native(case.raw[s], case.rm[s], case.cm[s], case.alpha, case.G[s], case.iters)
    assert torch.equal(dS.view(torch.int32), case.got_dS[s].view(torch.int32)) and torch.equal(part.view(torch.int32), case.got_part[s].view(torch.int32))


@pytest.mark.parametrize("shape", [(3, 5, 9), (2, 132, 131)])
def test_no_valid_column_or_row_gives_zeros(shape):
    B, M, N = shape
    raw, rm, cm, alpha, _, G, _ = R.problem(B, M, N, seed=9)
    cm[1] = False
    rm[0] = False
    dS, part = run_native(raw, rm, cm, alpha, G, 100)
    assert bool((dS[:2] == 0).all()) and bool((part[:2] == 0).all())
    if B > 2:                                            # the problem behind them is untouched by its neighbours
        alone, alone_part = run_native(raw[2:], rm[2:], cm[2:], alpha, G[2:], 100)
        assert torch.equal(alone.view(torch.int32), dS[2:].view(torch.int32)) and bool(alone.abs().max() > 0)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["patch", "first-general"], indirect=True)
def test_log_optimal_transport_is_differentiable(case):
    """Fails without the feature: the output of F.log_optimal_transport had no grad_fn."""
    B, M, N = case.shape
    raw = case.raw.cuda().requires_grad_()
    alpha = torch.nn.Parameter(case.alpha.clone().cuda())
    rm, cm = case.rm.cuda(), case.cm.cuda()
    out = F.log_optimal_transport(raw, rm, cm, alpha, scale=SCALE, iters=case.iters)
    assert out.grad_fn is not None
    (out * case.G.cuda()).sum().backward()
    err = (raw.grad.cpu().double() - case.d_raw).abs().flatten(1).max(1)[0]
    assert bool((err <= case.tol).all()), (err / case.tol).max().item()
    assert alpha.grad.shape == alpha.shape and abs(alpha.grad.item() - case.d_alpha.item()) <= case.tol_alpha
    with torch.no_grad():
        plain = F.log_optimal_transport(raw, rm, cm, alpha, scale=SCALE, iters=case.iters)
    plain2 = F.log_optimal_transport(raw.detach(), rm, cm, alpha.detach(), scale=SCALE, iters=case.iters)
    F.check_transport_status()
    assert plain.grad_fn is None and plain2.grad_fn is None and not plain2.requires_grad
    assert torch.equal(plain.view(torch.int32), out.detach().view(torch.int32)) and torch.equal(plain2.view(torch.int32), plain.view(torch.int32))


@pytest.mark.parametrize("case", ["patch", "first-general"], indirect=True)
def test_forward_and_backward_do_not_synchronise_with_the_host(case):
    """torch's sync debug mode raises on any synchronising torch call.  The ctypes calls are outside its view: that lcr_log_sinkhorn_grad only
    enqueues launches (no copy, no allocation, no stream or device wait) is established by reading csrc/sinkhorn_grad.hip."""
    raw, alpha = case.raw.cuda().requires_grad_(), torch.nn.Parameter(case.alpha.clone().cuda())
    rm, cm, G = case.rm.cuda(), case.cm.cuda(), case.G.cuda()
    (F.log_optimal_transport(raw, rm, cm, alpha, scale=SCALE, iters=case.iters) * G).sum().backward()      # first call: lazy set-up
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = F.log_optimal_transport(raw, rm, cm, alpha, scale=SCALE, iters=case.iters)
        (out * G).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    F.check_transport_status()
    assert bool(torch.isfinite(raw.grad).all())


def test_transport_module_trains_alone():
    from lcrnet_amd.model_family.LCRNet import LearnableLogOptimalTransport
    raw, rm, cm, _, _, G, _ = R.problem(3, 5, 9, seed=4)
    ot = LearnableLogOptimalTransport(100).cuda()
    out = ot(raw.cuda(), rm.cuda(), cm.cuda())
    (out * G.cuda()).sum().backward()
    want = R.restate(raw, rm, cm, torch.tensor(1.0), 1.0, G, 100)
    g32 = R.autograd_reference(raw, rm, cm, torch.tensor(1.0), 1.0, G, 100, torch.float32)[1]
    dust = want[2][:, 5, :].abs().sum() + want[2][:, :5, 9].abs().sum()
    assert abs(ot.alpha.grad.item() - want[1].item()) <= R.bound(abs(g32.item() - want[1].item()), dust.item())
    with torch.no_grad():
        assert ot(raw.cuda()).grad_fn is None


def dense_patch_scores(fa, ia, fb, ib, ma, mb, alpha, scale, dtype):
    """the dense form of patch_log_optimal_transport on the CPU: gather on the zero-row-padded features, product, oracle transport"""
    from oracle import torch_ref
    pa = torch.cat([fa, fa.new_zeros(1, fa.shape[1])])[ia]
    pb = torch.cat([fb, fb.new_zeros(1, fb.shape[1])])[ib]
    return torch_ref.log_optimal_transport(torch.bmm(pa, pb.transpose(1, 2)) * scale, ma, mb, alpha, iters=100)


def test_patch_transport_is_differentiable_in_the_features():
    P, K, C, n = 3, 128, 32, 500
    g = torch.Generator().manual_seed(6)
    fa, fb = torch.randn(n, C, generator=g), torch.randn(n + 7, C, generator=g)
    ia, ib = torch.randint(0, n, (P, K), generator=g), torch.randint(0, n + 7, (P, K), generator=g)
    ma, mb = torch.rand(P, K, generator=g) > 0.1, torch.rand(P, K, generator=g) > 0.1
    ma[:, 0] = mb[:, 0] = True
    ia[~ma], ib[~mb] = n, n + 7                          # shadow indices: the zero row
    G = torch.randn(P, K + 1, K + 1, generator=g)
    V = torch.ones(P, K + 1, K + 1, dtype=torch.bool)
    V[:, :K, :] &= ma[:, :, None]
    V[:, :, :K] &= mb[:, None, :]
    G = torch.where(V, G, torch.zeros_like(G))
    scale = 1.0 / C ** 0.5
    ref = {}
    for dt in (torch.float64, torch.float32):
        a, b, al = fa.to(dt).clone().requires_grad_(), fb.to(dt).clone().requires_grad_(), torch.tensor(0.7, dtype=dt).requires_grad_()
        (dense_patch_scores(a, ia, b, ib, ma, mb, al, scale, dt) * G.to(dt)).sum().backward()
        ref[dt] = (a.grad.double(), b.grad.double(), al.grad.double())
    a, b = fa.cuda().requires_grad_(), fb.cuda().requires_grad_()
    al = torch.nn.Parameter(torch.tensor(0.7, device=DEV))
    out = F.patch_log_optimal_transport(a, ia.cuda(), b, ib.cuda(), ma.cuda(), mb.cuda(), al, scale=scale, iters=100)
    assert out.grad_fn is not None
    (out * G.cuda()).sum().backward()
    # the scale of d_alpha is sum|dS| over the valid dustbin entries (it is a long sum with cancellation), from the fp64 restatement
    pa, pb = torch.cat([fa, fa.new_zeros(1, C)])[ia].double(), torch.cat([fb, fb.new_zeros(1, C)])[ib].double()
    dS64 = R.restate(torch.bmm(pa, pb.transpose(1, 2)), ma, mb, torch.tensor(0.7), scale, G, 100)[2]
    dust = (dS64[:, K, :].abs().sum() + dS64[:, :K, K].abs().sum()).item()
    for name, got, w64, w32 in zip(("feats_a", "feats_b", "alpha"), (a.grad, b.grad, al.grad), ref[torch.float64], ref[torch.float32]):
        e_ref, err = (w32 - w64).abs().max().item(), (got.cpu().double() - w64).abs().max().item()
        tol = R.bound(e_ref, dust if name == "alpha" else w64.abs().max().item())
        print("patch transport d %s: err / e_ref %.2f, err / tol %.2f" % (name, err / max(e_ref, 1e-300), err / tol))
        assert err <= tol, (name, err, e_ref)
    with torch.no_grad():
        fused = F.patch_log_optimal_transport(a, ia.cuda(), b, ib.cuda(), ma.cuda(), mb.cuda(), al, scale=scale, iters=100)
    assert fused.grad_fn is None
    # two forward forms of the same scores (fused product kernel / torch's product): test_pose_gpu's bound between fp32 forms of the transport
    assert (fused - out.detach())[V.cuda()].abs().max().item() < 1e-4


# ---- end to end: scores -> gap loss -> backward -> fused Adan ---------------------------------------------------------------------------------
def test_gap_loss_trains_patch_features_and_alpha():
    import lcrnet_amd.losses as L
    from lcrnet_amd.adan import Adan
    from lcrnet_amd.config import make_cfg
    P, K, C = 3, 128, 32
    g = torch.Generator().manual_seed(8)
    pts = torch.rand(P, K, 3, generator=g) * 4.0
    perm = torch.stack([torch.randperm(K, generator=g) for _ in range(P)])
    anc = torch.gather(pts, 1, perm[:, :, None].expand(P, K, 3)) + 0.01 * torch.randn(P, K, 3, generator=g)
    ma, mb = torch.rand(P, K, generator=g) > 0.1, torch.rand(P, K, generator=g) > 0.1
    ma[:, 0] = mb[:, 0] = True
    f0a, f0b = torch.randn(P * K, C, generator=g), torch.randn(P * K, C, generator=g)
    idx = torch.arange(P * K).view(P, K)
    loss_fn = L.gap(make_cfg())
    data = {"transform": torch.eye(4)}

    def train(dense):
        fa, fb = torch.nn.Parameter(f0a.clone().cuda()), torch.nn.Parameter(f0b.clone().cuda())
        alpha = torch.nn.Parameter(torch.tensor(1.0, device=DEV))
        opt = Adan([fa, fb, alpha], lr=1e-2, fused=True)
        losses = []
        for _ in range(20):
            opt.zero_grad()
            if dense:
                raw = torch.bmm(fa.view(P, K, C), fb.view(P, K, C).transpose(1, 2)) / C ** 0.5
                ms = R.dense_transport(raw, ma.cuda(), mb.cuda(), alpha)
            else:
                ms = F.patch_log_optimal_transport(fa, idx.cuda(), fb, idx.cuda(), ma.cuda(), mb.cuda(), alpha, scale=1.0 / C ** 0.5, iters=100)
            out = {"matching_scores": ms, "pos_node_corr_knn_masks": ma.cuda(), "anc_node_corr_knn_masks": mb.cuda(),
                   "pos_node_corr_knn_points": pts.cuda(), "anc_node_corr_knn_points": anc.cuda()}
            loss = loss_fn(out, data)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return losses, alpha.item()

    losses, a_native = train(False)
    losses_d, a_dense = train(True)
    print("gap training: loss %.6f -> %.6f (dense torch transport %.6f -> %.6f); alpha 1 -> %.8f (dense %.8f, difference %.2e)" % (
        losses[0], losses[-1], losses_d[0], losses_d[-1], a_native, a_dense, abs(a_native - a_dense)))
    assert losses[-1] < losses[0]
    assert a_native != 1.0 and a_dense != 1.0 and (a_native - 1.0) * (a_dense - 1.0) > 0
