"""CPU: the fp64 restatements of the 3D-RoFormer reverse passes (tests/attention_grad_restatement.py) against fp64 torch autograd through the
reference's formulas (oracle/torch_ref), their planted mistakes against the tolerance the GPU tests use, and the host-only entries of
csrc/attention_grad.hip (workspace sizes, argument checks).

Observed agreement of the restatements with fp64 autograd, relative to max|g|: attention <= 2e-15, rotary <= 3e-16, LayerNorm <= 2e-15;
RESTATE_BOUND leaves more than two orders of magnitude over that (sums of up to 300 terms in a different order) and stays six orders below
the smallest planted mistake.

On the parent commit the three tests of the host-only entries and refusals fail (the library has no such symbols, `attention_topk` does not
look at grad mode); the restatement tests touch no product code and pass there."""
import ctypes

import pytest
import torch

import attention_grad_restatement as R

RESTATE_BOUND = 1e-12
HEADS = 4


def rel(got, want):
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


def gpu_tol(w32, w64):
    """the tolerance test_attention_grad_gpu.py applies to this tensor"""
    return R.bound((w32 - w64).abs().max().item(), w64.abs().max().item())


ATT_CASES = [((5, 7), None, None, 1.0), ((33, 65), None, None, 1.0), ((33, 65), None, None, 8.0), ((70, 129), None, None, 1.0),
             ((172, 196), [1, 40, 131], [3, 129, 64], 1.0)]


@pytest.mark.parametrize("shape,q_lens,k_lens,q_scale", ATT_CASES)
def test_attention_restatement_equals_fp64_autograd(shape, q_lens, k_lens, q_scale):
    q, k, v, d_out = R.attention_problem(shape[0], shape[1], HEADS, seed=shape[0] + shape[1], q_scale=q_scale)
    out, dq, dk, dv = R.attention_restate(q, k, v, d_out, HEADS, q_lens, k_lens)
    w64 = R.autograd_attention(q, k, v, d_out, HEADS, q_lens, k_lens, torch.float64)
    w32 = R.autograd_attention(q, k, v, d_out, HEADS, q_lens, k_lens, torch.float32)
    errs = [rel(g, w) for g, w in zip((dq, dk, dv), w64)]
    print("attention restatement %s x%g: dq %.1e dk %.1e dv %.1e of max|g|" % (shape, q_scale, *errs))
    assert rel(out, R.attention_formula(q.double(), k.double(), v.double(), HEADS, q_lens, k_lens)) <= RESTATE_BOUND
    assert max(errs) <= RESTATE_BOUND
    for m in R.ATTENTION_MISTAKES:
        wrong = R.attention_restate(q, k, v, d_out, HEADS, q_lens, k_lens, mistake=m)[1:]
        off = max((g - w).abs().max().item() / gpu_tol(a, w) for g, w, a in zip(wrong, w64, w32))
        print("planted %s: %.1f x the GPU tolerance" % (m, off))
        assert off >= 8.0, (m, off)


def test_single_key_gives_vanishing_dq_dk_and_dv_equal_to_d_out():
    """one key: P = 1, so dv = d_out; dP = D up to the order of two 32-term sums (the kernel forms both with one instruction sequence and
    gets exact zeros: test_attention_grad_gpu.py)"""
    q, k, v, d_out = R.attention_problem(1, 1, HEADS, seed=2)
    _, dq, dk, dv = R.attention_restate(q, k, v, d_out, HEADS)
    assert dq.abs().max().item() <= 1e-14 and dk.abs().max().item() <= 1e-14 and torch.equal(dv, d_out.double())


@pytest.mark.parametrize("n", [1, 37, 300])
def test_rotary_restatement_equals_fp64_autograd(n):
    g = torch.Generator().manual_seed(n)
    xq, xk = torch.randn(n, HEADS * 32, generator=g), torch.randn(n, HEADS * 32, generator=g)
    theta = torch.randn(n, HEADS * 16, generator=g) * 3.0
    dyq, dyk = torch.randn(n, HEADS * 32, generator=g), torch.randn(n, HEADS * 32, generator=g)
    y, dx, dth = R.rotary_restate(xq, theta, dyq)
    wx, wt = R.autograd_rotary(xq, theta, dyq, HEADS, torch.float64)
    print("rotary restatement N=%d: y %.1e dx %.1e dtheta %.1e" % (n, rel(y, R.rotary_formula(xq.double(), theta.double(), HEADS)), rel(dx, wx), rel(dth, wt)))
    assert rel(y, R.rotary_formula(xq.double(), theta.double(), HEADS)) <= RESTATE_BOUND and rel(dx, wx) <= RESTATE_BOUND and rel(dth, wt) <= RESTATE_BOUND
    # q and k rotated by the same theta: autograd sums the two contributions
    ref = {}
    for dt in (torch.float64, torch.float32):
        a, b, t = (z.to(dt).clone().requires_grad_() for z in (xq, xk, theta))
        ((R.rotary_formula(a, t, HEADS) * dyq.to(dt)).sum() + (R.rotary_formula(b, t, HEADS) * dyk.to(dt)).sum()).backward()
        ref[dt] = t.grad.double()
    both = R.rotary_qk_restate(xq, xk, theta, dyq, dyk)[2]
    assert rel(both, ref[torch.float64]) <= RESTATE_BOUND
    tol = gpu_tol(ref[torch.float32], ref[torch.float64])
    for m in R.ROTARY_MISTAKES:
        off = (R.rotary_qk_restate(xq, xk, theta, dyq, dyk, mistake=m)[2] - ref[torch.float64]).abs().max().item() / tol
        print("planted %s: %.1f x the GPU tolerance" % (m, off))
        assert off >= 8.0, (m, off)


@pytest.mark.parametrize("n,d", [(1, 32), (37, 32), (1, 128), (37, 128), (37, 1024), (1000, 128)])
@pytest.mark.parametrize("with_b", [False, True])
def test_layernorm_restatement_equals_fp64_autograd(n, d, with_b):
    g = torch.Generator().manual_seed(n + d)
    a, b = torch.randn(n, d, generator=g), (torch.randn(n, d, generator=g) if with_b else None)
    gamma, beta, dy = 1.0 + 0.3 * torch.randn(d, generator=g), torch.randn(d, generator=g), torch.randn(n, d, generator=g)
    y, dx, dg, db = R.layernorm_restate(a, b, gamma, beta, dy)
    w64 = R.autograd_layernorm(a, b, gamma, beta, dy, 1e-5, torch.float64)
    w32 = R.autograd_layernorm(a, b, gamma, beta, dy, 1e-5, torch.float32)
    errs = [rel(dx, w64[0]), rel(dg, w64[2]), rel(db, w64[3])]
    print("layernorm restatement N=%d D=%d b=%s: dx %.1e dgamma %.1e dbeta %.1e" % (n, d, with_b, *errs))
    assert max(errs) <= RESTATE_BOUND
    if with_b:
        assert torch.equal(w64[0], w64[1]), "both addends receive the same gradient"
    wrong = R.layernorm_restate(a, b, gamma, beta, dy, mistake="no_mean_dy_xhat")[1]
    off = (wrong - w64[0]).abs().max().item() / gpu_tol(w32[0], w64[0])
    print("planted no_mean_dy_xhat: %.1f x the GPU tolerance" % off)
    assert off >= 8.0, off


# ---- host-only entries ----------------------------------------------------------------------------------------------------------------------
def _lib():
    import lcrnet_amd._lib as L
    return L.lib()


def test_workspace_queries_answer_on_the_host():
    L = _lib()
    n = ctypes.c_size_t(0)
    prev = 0
    for nq in (0, 1, 33, 860, 27520):
        assert L.lcr_attention_grad_ws_bytes(nq, 4, ctypes.byref(n)) == 0 and n.value >= 2 * 4 * nq * 4 and n.value >= prev
        prev = n.value
    for N, D in [(0, 128), (1, 32), (37, 1024), (1000, 128)]:
        assert L.lcr_add_layernorm_grad_ws_bytes(N, D, ctypes.byref(n)) == 0 and n.value >= ((N + 15) // 16) * 2 * D * 4
    assert L.lcr_attention_grad_ws_bytes(1, 4, None) != 0 and L.lcr_attention_grad_ws_bytes(-1, 4, ctypes.byref(n)) != 0
    assert L.lcr_attention_grad_ws_bytes(1, 0, ctypes.byref(n)) != 0
    assert L.lcr_add_layernorm_grad_ws_bytes(1, 1025, ctypes.byref(n)) != 0 and L.lcr_add_layernorm_grad_ws_bytes(1, 0, ctypes.byref(n)) != 0
    assert L.lcr_add_layernorm_grad_ws_bytes(1, 128, None) != 0


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = ctypes.cast((ctypes.c_int64 * 1)(1), ctypes.c_void_p)
    zero = ctypes.cast((ctypes.c_int64 * 1)(0), ctypes.c_void_p)
    big = 4096 * 4
    assert L.lcr_attention_seg_grad_f32(None, p, p, p, p, one, one, 1, 4, 32, p, p, p, p, big, None) != 0
    assert L.lcr_attention_seg_grad_f32(p, p, p, p, p, one, one, 1, 4, 32, None, p, p, p, big, None) != 0
    assert L.lcr_attention_seg_grad_f32(p, p, p, p, p, one, one, 1, 4, 64, p, p, p, p, big, None) != 0          # head_dim
    assert L.lcr_attention_seg_grad_f32(p, p, p, p, p, one, one, 65, 4, 32, p, p, p, p, big, None) != 0         # P
    assert L.lcr_attention_seg_grad_f32(p, p, p, p, p, one, zero, 1, 4, 32, p, p, p, p, big, None) != 0         # a problem without keys
    assert L.lcr_attention_seg_grad_f32(p, p, p, p, p, one, one, 1, 4, 32, p, p, p, p, 8, None) != 0            # short workspace
    assert L.lcr_attention_seg_grad_f32(p, p, p, p, p, one, one, 1, 4, 32, p, p, p, None, big, None) != 0
    assert L.lcr_rotary_embed_grad(None, p, p, 1, 4, p, p, None) != 0 and L.lcr_rotary_embed_grad(p, p, p, 1, 0, p, p, None) != 0
    assert L.lcr_rotary_embed_grad(p, p, p, 0, 4, p, p, None) == 0
    assert L.lcr_add_layernorm_grad(None, p, p, p, 1, 128, 1e-5, p, p, p, p, big, None) != 0
    assert L.lcr_add_layernorm_grad(p, None, p, p, 1, 2048, 1e-5, p, p, p, p, big, None) != 0
    assert L.lcr_add_layernorm_grad(p, None, p, p, 37, 128, 1e-5, p, p, p, p, 8, None) != 0


def test_cpu_tensors_and_topk_are_refused():
    from lcrnet_amd import functional as F
    q, k, v, _ = R.attention_problem(5, 7, HEADS, seed=1)
    with pytest.raises(RuntimeError):
        F.attention(q.clone().requires_grad_(), k, v, HEADS)
    with pytest.raises(NotImplementedError, match="cfg.GAT.k"):
        F.attention_topk(q.clone().requires_grad_(), k, v, HEADS, [5], [7], [2])
