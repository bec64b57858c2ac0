"""fp64 restatements of the three reverse passes of csrc/attention_grad.hip, written from their formulas (no autograd), with planted mistakes;
beside each the differentiable torch formula of the reference (oracle/torch_ref: dynamic_attention with k = None, RotaryPositionalEmbedding.forward,
LayerNorm(a + b)) that autograd is run through.  Shared by test_attention_grad_cpu.py and test_attention_grad_gpu.py.

Layouts are the library's: q [Nq, heads*32], k / v [Nk, heads*32], theta [N, heads*16] (one angle per adjacent channel pair), stacked problems
given by q_lens / k_lens."""
import math

import torch

from oracle import torch_ref

HEAD_DIM = 32
ATTENTION_MISTAKES = ("no_D", "no_scale")
ROTARY_MISTAKES = ("dtheta_sign", "dtheta_q_only")
LAYERNORM_MISTAKES = ("no_mean_dy_xhat",)


def bound(e_ref, gmax):
    """the suite's rule: 4 x the error of fp32 torch autograd of the same formula against fp64, floored at 2^-20 max|g|"""
    return max(4.0 * e_ref, 2.0 ** -20 * gmax)


def _problems(nq, nk, q_lens, k_lens):
    ql = [nq] if q_lens is None else [int(x) for x in q_lens]
    kl = [nk] if k_lens is None else [int(x) for x in k_lens]
    assert len(ql) == len(kl) and sum(ql) == nq and sum(kl) == nk
    out, qo, ko = [], 0, 0
    for a, b in zip(ql, kl):
        out.append((slice(qo, qo + a), slice(ko, ko + b)))
        qo, ko = qo + a, ko + b
    return out


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
def attention_formula(q, k, v, heads, q_lens=None, k_lens=None):
    """the reference's dense attention per problem, differentiable, any dtype"""
    outs = []
    for qs, ks in _problems(q.shape[0], k.shape[0], q_lens, k_lens):
        qh, kh, vh = torch_ref._heads(q[qs], heads), torch_ref._heads(k[ks], heads), torch_ref._heads(v[ks], heads)
        s = torch.softmax(torch.einsum("hnd,hmd->hnm", qh, kh) / math.sqrt(qh.shape[-1]), dim=-1)
        outs.append(torch.einsum("hnm,hmd->hnd", s, vh).permute(1, 0, 2).reshape(qh.shape[1], -1))
    return torch.cat(outs)


def attention_restate(q, k, v, d_out, heads, q_lens=None, k_lens=None, mistake=None):
    """-> (out, dq, dk, dv) in fp64: P = softmax(scale Q K^T), O = P V, dV = P^T dO, dP = dO V^T, D = sum_d dO O, dS = P (dP - D),
    dQ = scale dS K, dK = scale dS^T Q, per problem and head."""
    q, k, v, d_out = (t.double() for t in (q, k, v, d_out))
    scale = 1.0 / math.sqrt(HEAD_DIM)
    out, dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for qs, ks in _problems(q.shape[0], k.shape[0], q_lens, k_lens):
        for h in range(heads):
            c = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            Q, K, V, dO = q[qs, c], k[ks, c], v[ks, c], d_out[qs, c]
            S = scale * Q @ K.T
            P = torch.exp(S - S.max(1, keepdim=True)[0])
            P = P / P.sum(1, keepdim=True)
            O = P @ V
            D = (dO * O).sum(1, keepdim=True)
            if mistake == "no_D":
                D = torch.zeros_like(D)
            dS = P * (dO @ V.T - D)
            g = 1.0 if mistake == "no_scale" else scale
            out[qs, c], dv[ks, c], dq[qs, c], dk[ks, c] = O, P.T @ dO, g * dS @ K, g * dS.T @ Q
    return out, dq, dk, dv


# ---- rotary ---------------------------------------------------------------------------------------------------------------------------------
def rotary_formula(x, theta, heads):
    """RotaryPositionalEmbedding.forward on the library's layout, differentiable, any dtype"""
    n = x.shape[0]
    return torch_ref.rotary(torch_ref._heads(x, heads), torch_ref._heads(theta, heads)).permute(1, 0, 2).reshape(n, -1)


def rotary_restate(x, theta, dy, mistake=None):
    """-> (y, dx, dtheta) in fp64: per channel pair y = R(theta) x, dx = R(-theta) dy, dtheta = dy0 (-y1) + dy1 y0 (from the rotated y)"""
    x, theta, dy = x.double(), theta.double(), dy.double()
    n = x.shape[0]
    xp, gp = x.reshape(n, -1, 2), dy.reshape(n, -1, 2)
    c, s = torch.cos(theta), torch.sin(theta)
    y0, y1 = xp[..., 0] * c - xp[..., 1] * s, xp[..., 1] * c + xp[..., 0] * s
    dx = torch.stack([gp[..., 0] * c + gp[..., 1] * s, gp[..., 1] * c - gp[..., 0] * s], -1).reshape(n, -1)
    dth = gp[..., 0] * (-y1) + gp[..., 1] * y0
    if mistake == "dtheta_sign":
        dth = -dth
    return torch.stack([y0, y1], -1).reshape(n, -1), dx, dth


def rotary_qk_restate(xq, xk, theta, dyq, dyk, mistake=None):
    """the self layers rotate q and k by the SAME theta: -> (dxq, dxk, dtheta) with dtheta the sum of both contributions"""
    _, dxq, tq = rotary_restate(xq, theta, dyq, mistake if mistake == "dtheta_sign" else None)
    _, dxk, tk = rotary_restate(xk, theta, dyk, mistake if mistake == "dtheta_sign" else None)
    return dxq, dxk, (tq if mistake == "dtheta_q_only" else tq + tk)


# ---- LayerNorm(a + b) -----------------------------------------------------------------------------------------------------------------------
def layernorm_formula(a, b, gamma, beta, eps=1e-5):
    x = a if b is None else a + b
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


def layernorm_restate(a, b, gamma, beta, dy, eps=1e-5, mistake=None):
    """-> (y, d(a + b), dgamma, dbeta) in fp64: xhat = (x - mean) rstd, g = dy gamma, dx = rstd (g - mean(g) - xhat mean(g xhat)),
    dgamma = sum_n dy xhat, dbeta = sum_n dy"""
    a, gamma, beta, dy = a.double(), gamma.double(), beta.double(), dy.double()
    x = a if b is None else a + b.double()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    g = dy * gamma
    m2 = (g * xh).mean(1, keepdim=True)
    if mistake == "no_mean_dy_xhat":
        m2 = torch.zeros_like(m2)
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * m2)
    return xh * gamma + beta, dx, (dy * xh).sum(0), dy.sum(0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def attention_problem(nq, nk, heads, seed, q_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nq, heads * HEAD_DIM, generator=g) * q_scale
    k, v = torch.randn(nk, heads * HEAD_DIM, generator=g), torch.randn(nk, heads * HEAD_DIM, generator=g)
    return q, k, v, torch.randn(nq, heads * HEAD_DIM, generator=g)


def autograd_attention(q, k, v, d_out, heads, q_lens, k_lens, dtype):
    """(dq, dk, dv) of torch autograd through attention_formula in `dtype`, returned in fp64"""
    a, b, c = (t.to(dtype).clone().requires_grad_() for t in (q, k, v))
    (attention_formula(a, b, c, heads, q_lens, k_lens) * d_out.to(dtype)).sum().backward()
    return a.grad.double(), b.grad.double(), c.grad.double()


def autograd_rotary(x, theta, dy, heads, dtype):
    a, t = x.to(dtype).clone().requires_grad_(), theta.to(dtype).clone().requires_grad_()
    (rotary_formula(a, t, heads) * dy.to(dtype)).sum().backward()
    return a.grad.double(), t.grad.double()


def autograd_layernorm(a, b, gamma, beta, dy, eps, dtype):
    ts = [None if t is None else t.to(dtype).clone().requires_grad_() for t in (a, b, gamma, beta)]
    (layernorm_formula(*ts, eps) * dy.to(dtype)).sum().backward()
    return tuple(None if t is None else t.grad.double() for t in ts)
