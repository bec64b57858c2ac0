"""CPU: the fp64 restatement of the transport's reverse pass (tests/sinkhorn_grad_restatement.py) against fp64 torch autograd through
oracle/torch_ref.log_optimal_transport, its planted mistakes, and the host-only entries of csrc/sinkhorn_grad.hip (workspace size, form,
argument checks)."""
import ctypes

import pytest
import torch

import sinkhorn_grad_restatement as R

RESTATE_BOUND = 1e-12          # relative to max|g|; observed <= 3e-15
CASES = [((3, 5, 9), 1), ((3, 5, 9), 2), ((3, 5, 9), 100), ((1, 40, 33), 100), ((2, 128, 128), 100)]


@pytest.mark.parametrize("shape,iters", CASES)
def test_restatement_equals_fp64_autograd(shape, iters):
    B, M, N = shape
    raw, rm, cm, alpha, _, G, V = R.problem(B, M, N, seed=11 + M, spread=3.0)
    d_raw, d_alpha, dS, part = R.restate(raw, rm, cm, alpha, 0.5, G, iters)
    g_raw, g_alpha = R.autograd_reference(raw, rm, cm, alpha, 0.5, G, iters, torch.float64)
    scale = g_raw.abs().max().item()
    e_raw = (d_raw - g_raw).abs().max().item() / scale
    e_alpha = abs((d_alpha - g_alpha).item()) / max(part.abs().sum().item(), 1e-300)
    print("restatement %s T=%d: d_raw %.1e of max|g|, d_alpha %.1e" % (shape, iters, e_raw, e_alpha))
    assert e_raw <= RESTATE_BOUND and e_alpha <= RESTATE_BOUND
    assert bool((g_raw[~V[:, :M, :N]] == 0).all()), "autograd's gradient on masked entries is exactly zero"
    assert bool((dS[~V] == 0).all())
    for m in R.MISTAKES:
        if not R.mistake_shows(m, iters):
            continue
        Gin = R.problem(B, M, N, seed=11 + M, spread=3.0)[4] if m == "g_unmasked" else G
        w_raw, w_alpha, _, _ = R.restate(raw, rm, cm, alpha, 0.5, Gin, iters, mistake=m)
        moved = max((w_raw - g_raw).abs().max().item() / scale, abs((w_alpha - g_alpha).item()) / part.abs().sum().item())
        assert moved > 1e6 * RESTATE_BOUND, (m, moved)


def test_no_valid_column_gives_zeros():
    raw, rm, cm, alpha, _, G, _ = R.problem(2, 5, 9, seed=3)
    cm[1] = False
    d_raw, d_alpha, dS, part = R.restate(raw, rm, cm, alpha, 0.5, G, 10)
    assert bool((dS[1] == 0).all()) and part[1].item() == 0 and bool(torch.isfinite(dS).all())


def _lib():
    import lcrnet_amd._lib as L
    return L.lib()


def _ws(B, M, N, T):
    n = ctypes.c_size_t(0)
    rc = _lib().lcr_log_sinkhorn_grad_ws_bytes(B, M, N, T, ctypes.byref(n))
    return rc, n.value


def _form(B, M, N):
    f = ctypes.c_int(-1)
    rc = _lib().lcr_log_sinkhorn_grad_form(B, M, N, ctypes.byref(f))
    return rc, f.value


def test_workspace_and_form_answer_on_the_host():
    for M, N in [(5, 9), (128, 128), (131, 131), (132, 131), (131, 132), (350, 330)]:
        want = 0 if max(M, N) + 1 <= 132 else 1
        assert _form(1, M, N) == (0, want) and _form(3600, M, N) == (0, want)
        prev_b = 0
        for B in (1, 2, 16, 256, 3600):
            prev_t = 0
            for T in (1, 2, 100, 140, 141, 300):
                rc, n = _ws(B, M, N, T)
                assert rc == 0 and n >= 1 and n >= prev_t, (B, M, N, T, n)
                prev_t = n
            assert prev_t >= prev_b
            prev_b = prev_t
    # the resident form records into LDS while (2T + 1) * 136 floats fit 150 KiB, into the workspace beyond; the general form always
    assert _ws(3600, 128, 128, 100)[1] <= 256
    assert _ws(2, 131, 131, 150)[1] >= 2 * 301 * 136 * 4
    assert _ws(16, 350, 330, 100)[1] >= 16 * (100 * 351 + 101 * 331) * 4


def test_bad_arguments_are_refused():
    L = _lib()
    n = ctypes.c_size_t(0)
    f = ctypes.c_int(0)
    assert L.lcr_log_sinkhorn_grad_ws_bytes(1, 5, 9, 100, None) != 0
    assert L.lcr_log_sinkhorn_grad_ws_bytes(1, 0, 9, 100, ctypes.byref(n)) != 0
    assert L.lcr_log_sinkhorn_grad_ws_bytes(1, 5, 0, 100, ctypes.byref(n)) != 0
    assert L.lcr_log_sinkhorn_grad_ws_bytes(1, 5, 9, 0, ctypes.byref(n)) != 0
    assert L.lcr_log_sinkhorn_grad_ws_bytes(-1, 5, 9, 100, ctypes.byref(n)) != 0
    assert L.lcr_log_sinkhorn_grad_form(1, 5, 9, None) != 0
    assert L.lcr_log_sinkhorn_grad_form(1, 0, 9, ctypes.byref(f)) != 0
    # the launcher refuses before any launch (no GPU is touched): null pointers, iters < 1, a short workspace; B == 0 is a no-op
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.lcr_log_sinkhorn_grad(None, p, p, p, 1, 5, 9, 100, 1e12, p, p, p, 4096 * 4, None) != 0
    assert L.lcr_log_sinkhorn_grad(p, p, p, p, 1, 5, 9, 100, 1e12, None, p, p, 4096 * 4, None) != 0
    assert L.lcr_log_sinkhorn_grad(p, p, p, p, 1, 5, 9, 100, 1e12, p, p, None, 4096 * 4, None) != 0
    assert L.lcr_log_sinkhorn_grad(p, p, p, p, 1, 5, 9, 0, 1e12, p, p, p, 4096 * 4, None) != 0
    assert L.lcr_log_sinkhorn_grad(p, p, p, p, 1, 5, 9, 100, 1e12, p, p, p, 8, None) != 0
    assert L.lcr_log_sinkhorn_grad(p, p, p, p, 1, 200, 200, 100, 1e12, p, p, p, 4096 * 4, None) != 0
    assert L.lcr_log_sinkhorn_grad(None, None, None, None, 0, 5, 9, 100, 1e12, None, None, None, 0, None) == 0


def test_cpu_tensors_are_refused():
    from lcrnet_amd import functional as F
    raw, rm, cm, alpha, _, _, _ = R.problem(1, 5, 9, seed=1)
    with pytest.raises(RuntimeError):
        F.log_optimal_transport(raw, rm, cm, alpha, scale=0.5)
    with pytest.raises(RuntimeError):
        F.log_optimal_transport(raw.clone().requires_grad_(), rm, cm, alpha, scale=0.5)
