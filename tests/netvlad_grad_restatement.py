"""fp64 restatements of the global-descriptor head in TRAINING mode (lcr_netvlad_train_forward / lcr_netvlad_backward, csrc/netvlad_grad.hip):
the forward by row multiplicities, its hand-derived reverse pass, the running-statistics update, and a plain-torch form of the reference's
padded formula (GlobalDescritionHEAD's training branch around NetVLADLoupe2.forward with a mask) for autograd.  Shared by
tests/test_netvlad_grad_cpu.py and tests/test_netvlad_grad_gpu.py.  Weights come from tests/netvlad_restatement.py's seeded generators.

Row i of a cloud of L rows, padded cyclically to Lmax rows, appears c = (Lmax-1-i)//L + 1 times: once unmasked, p = c-1 times as padding.
    bn1 statistics: sums over the real rows weighted by c, divided by S Lmax
    assignment:     w = softmax(bn1(a)) + p/64          (a padding row is set to -1e12 in all 64 clusters: uniform)
`mutate=` plants ONE mistake (MUTATIONS); the CPU test demands that each moves some gradient (or buffer) by >= 1e-3 of its scale.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netvlad_restatement as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_DIM, K_DIM, D_DIM = NR.F_DIM, NR.K_DIM, NR.D_DIM
BN_EPS = 1e-5
PFX = "netvlad."
# the ten trainable tensors, in the order of lcrnet_amd.functional.NETVLAD_GRAD_NAMES
PARAMS = ("cluster_weights", "cluster_weights2", "hidden1_weights", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias",
          "context_gating.gating_weights", "context_gating.bn1.weight", "context_gating.bn1.bias")
C_NAMES = ("cluster_weights", "cluster_weights2", "hidden1_weights", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "gating_weights", "gbn_w", "gbn_b")
BNS = ("bn1.", "bn2.", "context_gating.bn1.")

FORWARD_MUTATIONS = ("pad_dropped", "pad_real_softmax", "bn1_unweighted")
BACKWARD_MUTATIONS = ("bn1_stats_const", "bn2_stats_const", "gxhat_mean_dropped", "asum_w2_grad_dropped", "second_norm_backward_skipped")
MUTATIONS = FORWARD_MUTATIONS + BACKWARD_MUTATIONS + ("running_var_biased",)

# ------------------------------------------------------------------------------------------------ the cases of the GPU file
WEIGHT_KIND = "seeded"


def _ragged(count, lo, hi, seed):
    return tuple(int(v) for v in np.random.default_rng(seed).integers(lo, hi + 1, size=count))


CASES = {                                   # name -> (seg_lens, feature seed)
    "no-padding": ((4, 4, 4), 1),
    "wraps": ((5, 9, 7, 2), 2),             # a partial wrap and a multiple wrap
    "one-row-x130": ((1, 130, 67), 3),      # one row repeated 130 times; crosses a 128-row chunk
    "nine-clouds": (_ragged(9, 3, 40, 9), 4),     # crosses the eval forward's 8-cloud group
    "batch78": (_ragged(78, 1, 12, 78), 5),       # the reference's batch; crosses the 64-cloud batched-GEMM group
}
GOLDEN_CASE = "wraps"


def bound(e_ref, scale):
    """the project's standing rule for a gradient tensor: max(4 x the error of fp32 torch autograd of the same formula, 2^-20 of max|g|)"""
    return max(4.0 * e_ref, 2.0 ** -20 * scale)


def features(seg_lens, seed, zero_row=None):
    x = NR.netvlad_features(seg_lens, 7000 + seed, zero_rows=None if zero_row is None else [zero_row])
    return x


def upstream(S, seed):
    return torch.randn(S, D_DIM, generator=torch.Generator().manual_seed(8000 + seed))


def weights(dtype=torch.float64, kind=WEIGHT_KIND):
    """fresh copies of the 16 netvlad.* tensors in `dtype` (the cached fp32 originals stay untouched)"""
    return {k: v.detach().clone().to(dtype) for k, v in NR.netvlad_weights(kind).items()}


def multiplicity(seg_lens):
    """c per stacked row: how often the row appears in its cloud's cyclic padding to max(seg_lens) rows"""
    Lmax = max(seg_lens)
    return torch.cat([(Lmax - 1 - torch.arange(L)) // L + 1 for L in seg_lens])


def row_segments(seg_lens):
    return torch.cat([torch.full((L,), s, dtype=torch.long) for s, L in enumerate(seg_lens)])


# ------------------------------------------------------------------------------------------------ the reference's formula, padded (plain torch)
def padded_reference(sd, x, seg_lens, want_stats=False):
    """GlobalDescritionHEAD's training branch in plain torch ops in the dtype of `sd` / `x` (differentiable): explicit cyclic padding, mask,
    F.batch_norm on batch statistics, masked -1e12, softmax, VLAD, both normalisations, hidden projection, bn2, gating, F.normalize."""
    Fn = torch.nn.functional
    P = lambda k: sd[PFX + k]
    S, Lmax = len(seg_lens), max(seg_lens)
    mask = torch.zeros(S, Lmax, dtype=torch.bool)
    rows = []
    for i, t in enumerate(torch.split(x, list(seg_lens))):
        rows.append(t[torch.arange(Lmax) % t.shape[0]])
        mask[i, :t.shape[0]] = True
    xp = Fn.normalize(torch.stack(rows), dim=2)
    act0 = torch.matmul(xp, P("cluster_weights")).view(-1, K_DIM)
    act = Fn.batch_norm(act0, None, None, P("bn1.weight"), P("bn1.bias"), True, 0.1, BN_EPS).view(S, Lmax, K_DIM)
    act = act.masked_fill(~mask[:, :, None], -1e12)
    act = torch.softmax(act, dim=-1)
    a = act.sum(-2, keepdim=True) * P("cluster_weights2")
    vlad = torch.matmul(act.transpose(2, 1), xp).transpose(2, 1) - a
    vlad = Fn.normalize(vlad, dim=1, p=2, eps=1e-6).reshape(S, -1)
    vlad = Fn.normalize(vlad, dim=1, p=2, eps=1e-6)
    h = torch.matmul(vlad, P("hidden1_weights"))
    hp = Fn.batch_norm(h, None, None, P("bn2.weight"), P("bn2.bias"), True, 0.1, BN_EPS)
    g0 = torch.matmul(hp, P("context_gating.gating_weights"))
    gates = torch.sigmoid(Fn.batch_norm(g0, None, None, P("context_gating.bn1.weight"), P("context_gating.bn1.bias"), True, 0.1, BN_EPS))
    out = Fn.normalize(hp * gates, dim=1)
    if want_stats:
        st = lambda t: (t.detach().mean(0), t.detach().var(0, unbiased=False), t.shape[0])
        return out, {"bn1.": st(act0), "bn2.": st(h), "context_gating.bn1.": st(g0)}
    return out


def autograd(sd, x, seg_lens, dout, dtype, form=None, mutate=None):
    """(out, {param: grad}, dx, stats) by torch autograd in `dtype` of padded_reference (form None) or of forward() below (form "rows")"""
    sd = {k: v.detach().clone().to(dtype).requires_grad_(k[len(PFX):] in PARAMS) for k, v in sd.items()}
    xl = x.detach().clone().to(dtype).requires_grad_(True)
    if form == "rows":
        out, c = forward(sd, xl, seg_lens, mutate=mutate)
        stats = c["stats"]
    else:
        out, stats = padded_reference(sd, xl, seg_lens, want_stats=True)
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), {k: sd[PFX + k].grad for k in PARAMS}, xl.grad, stats


# ------------------------------------------------------------------------------------------------ the restatement: forward by multiplicities
def forward(sd, x, seg_lens, mutate=None):
    """-> (out [S,256], cache).  Differentiable torch ops in the dtype of the inputs (fp64 in the tests)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    P = lambda k: sd[PFX + k]
    S, Lmax, N = len(seg_lens), max(seg_lens), x.shape[0]
    assert N == sum(seg_lens) and min(seg_lens) >= 1
    if S == 1:
        raise ValueError("Expected more than 1 value per channel when training")
    c = multiplicity(seg_lens).to(x.dtype)[:, None]
    rseg = row_segments(seg_lens)
    nrm = x.norm(dim=1, keepdim=True)
    xh = x / nrm.clamp(min=1e-12)
    a = xh @ P("cluster_weights")
    cs, count = (torch.ones_like(c), float(N)) if mutate == "bn1_unweighted" else (c, float(S * Lmax))
    mu = (cs * a).sum(0) / count
    var = (cs * (a - mu) ** 2).sum(0) / count
    r1 = 1.0 / torch.sqrt(var + BN_EPS)
    ah = (a - mu) * r1
    sm = torch.softmax(ah * P("bn1.weight") + P("bn1.bias"), dim=1)
    if mutate == "pad_dropped":
        w = sm
    elif mutate == "pad_real_softmax":
        w = c * sm
    else:
        w = sm + (c - 1.0) / 64.0
    offs = np.concatenate([[0], np.cumsum(seg_lens)])
    parts = [(xh[offs[s]:offs[s + 1]], w[offs[s]:offs[s + 1]]) for s in range(S)]
    A = torch.stack([ws.sum(0) for _, ws in parts])                                           # [S,64]
    V0 = torch.stack([xs.t() @ ws for xs, ws in parts]) - A[:, None, :] * P("cluster_weights2")  # [S,1024,64]
    n1raw = V0.norm(dim=1)
    V1 = V0 / n1raw.clamp(min=1e-6)[:, None, :]
    n2raw = V1.reshape(S, -1).norm(dim=1)
    v = (V1 / n2raw.clamp(min=1e-6)[:, None, None]).reshape(S, -1)
    h = v @ P("hidden1_weights")
    mu2, var2 = h.mean(0), h.var(0, unbiased=False)
    r2 = 1.0 / torch.sqrt(var2 + BN_EPS)
    hh = (h - mu2) * r2
    hp = hh * P("bn2.weight") + P("bn2.bias")
    g0 = hp @ P("context_gating.gating_weights")
    mug, varg = g0.mean(0), g0.var(0, unbiased=False)
    rg = 1.0 / torch.sqrt(varg + BN_EPS)
    gh = (g0 - mug) * rg
    g = torch.sigmoid(gh * P("context_gating.bn1.weight") + P("context_gating.bn1.bias"))
    t = hp * g
    tn = t.norm(dim=1, keepdim=True)
    out = t / tn.clamp(min=1e-12)
    det = lambda z: z.detach()
    cache = dict(x=det(x), c=c, rseg=rseg, nrm=det(nrm), xh=det(xh), a=det(a), r1=det(r1), ah=det(ah), sm=det(sm), w=det(w), A=det(A), n1raw=det(n1raw),
                 n2raw=det(n2raw), v=det(v), r2=det(r2), hh=det(hh), hp=det(hp), rg=det(rg), gh=det(gh), g=det(g), tn=det(tn), out=det(out), count=count,
                 seg_lens=tuple(seg_lens),
                 stats={"bn1.": (det(mu), det(var), S * Lmax), "bn2.": (det(mu2), det(var2), S), "context_gating.bn1.": (det(mug), det(varg), S)})
    return out, cache


# ------------------------------------------------------------------------------------------------ the hand-derived reverse pass
def backward(sd, cache, dout, mutate=None):
    """-> ({param: grad}, dx) from the cache of forward(): no autograd.  fp64 throughout."""
    assert mutate is None or mutate in MUTATIONS, mutate
    P = lambda k: sd[PFX + k].detach()
    c = cache
    S = dout.shape[0]
    zero = torch.zeros((), dtype=dout.dtype)

    def bn_back(dy, xh, gamma, r, const=False):
        dgamma, dbeta = (dy * xh).sum(0), dy.sum(0)
        if const:
            return gamma * r * dy, dgamma, dbeta
        m1 = zero if mutate == "gxhat_mean_dropped" else (dy * xh).mean(0)
        return gamma * r * (dy - dy.mean(0) - xh * m1), dgamma, dbeta

    out, tn, g, hp = c["out"], c["tn"], c["g"], c["hp"]
    dot = (dout * out).sum(1, keepdim=True)
    dt = dout / tn.clamp(min=1e-12) - torch.where(tn >= 1e-12, dot * out / tn, zero)
    dhp = dt * g
    dpre = dt * hp * g * (1 - g)
    dg0, d_gbn_w, d_gbn_b = bn_back(dpre, c["gh"], P("context_gating.bn1.weight"), c["rg"])
    d_gating = hp.t() @ dg0
    dhp = dhp + dg0 @ P("context_gating.gating_weights").t()
    dh, d_bn2_w, d_bn2_b = bn_back(dhp, c["hh"], P("bn2.weight"), c["r2"], const=mutate == "bn2_stats_const")
    v = c["v"]
    d_hidden = v.t() @ dh
    dv = dh @ P("hidden1_weights").t()
    n2raw, n1raw = c["n2raw"][:, None], c["n1raw"]
    n2 = n2raw.clamp(min=1e-6)
    if mutate == "second_norm_backward_skipped":          # the normalisation taken for the identity on the way back (its scale is 1/8)
        dV1 = dv
    else:
        dV1 = dv / n2 - torch.where(n2raw >= 1e-6, (dv * v).sum(1, keepdim=True) / n2raw, zero) * v
    dV1, V1 = dV1.view(S, F_DIM, K_DIM), (v * n2).view(S, F_DIM, K_DIM)
    dot1 = (dV1 * V1).sum(1)
    dV0 = dV1 / n1raw.clamp(min=1e-6)[:, None, :] - torch.where(n1raw >= 1e-6, dot1 / n1raw, zero)[:, None, :] * V1
    W2 = P("cluster_weights2")[0]
    dA = -(dV0 * W2[None]).sum(1)
    d_w2 = -(c["A"][:, None, :] * dV0).sum(0)[None]
    if mutate == "asum_w2_grad_dropped":
        dA, d_w2 = torch.zeros_like(dA), torch.zeros_like(d_w2)
    xh, w, sm, ah, rseg = c["xh"], c["w"], c["sm"], c["ah"], c["rseg"]
    dw, dxh = torch.empty_like(sm), torch.empty_like(xh)
    o = 0
    for s, L in enumerate(c["seg_lens"]):
        dw[o:o + L] = xh[o:o + L] @ dV0[s] + dA[s]
        dxh[o:o + L] = w[o:o + L] @ dV0[s].t()
        o += L
    da_hat = sm * (dw - (sm * dw).sum(1, keepdim=True))                     # real rows only: the padding copies are constants
    d_bn1_w, d_bn1_b = (da_hat * ah).sum(0), da_hat.sum(0)
    gd = da_hat * P("bn1.weight")
    if mutate == "bn1_stats_const":
        da = c["r1"] * gd
    else:
        m1 = zero if mutate == "gxhat_mean_dropped" else (gd * ah).sum(0)
        da = c["r1"] * (gd - c["c"] / c["count"] * (gd.sum(0) + ah * m1))
    d_wc = xh.t() @ da
    dxh = dxh + da @ P("cluster_weights").t()
    nrm = c["nrm"]
    dx = dxh / nrm.clamp(min=1e-12) - torch.where(nrm >= 1e-12, (dxh * xh).sum(1, keepdim=True) / nrm.clamp(min=1e-300), zero) * xh
    grads = {"cluster_weights": d_wc, "cluster_weights2": d_w2, "hidden1_weights": d_hidden, "bn1.weight": d_bn1_w, "bn1.bias": d_bn1_b,
             "bn2.weight": d_bn2_w, "bn2.bias": d_bn2_b, "context_gating.gating_weights": d_gating, "context_gating.bn1.weight": d_gbn_w,
             "context_gating.bn1.bias": d_gbn_b}
    return grads, dx


def gradients(sd, x, seg_lens, dout, mutate=None):
    """(out, grads, dx, stats) of the restatement with one planted mistake: a forward mistake by autograd through the mutated forward, a
    backward mistake by the hand-derived pass"""
    if mutate in FORWARD_MUTATIONS:
        return autograd(sd, x, seg_lens, dout, torch.float64, form="rows", mutate=mutate)
    with torch.no_grad():
        out, cache = forward(sd, x.double(), seg_lens)
        grads, dx = backward(sd, cache, dout.double(), mutate=mutate)
    return out, grads, dx, cache["stats"]


# ------------------------------------------------------------------------------------------------ running statistics
def running_update(sd, stats, mutate=None, momentum=0.1):
    """{buffer key: new value} as nn.BatchNorm1d leaves them after ONE training call: running <- (1-m) running + m new, the variance
    unbiased (n/(n-1)), num_batches_tracked + 1"""
    out = {}
    for bn in BNS:
        mean, var, n = stats[bn]
        unb = var if mutate == "running_var_biased" else var * (n / (n - 1.0))
        out[bn + "running_mean"] = (1 - momentum) * sd[PFX + bn + "running_mean"].to(mean.dtype) + momentum * mean
        out[bn + "running_var"] = (1 - momentum) * sd[PFX + bn + "running_var"].to(var.dtype) + momentum * unb
        out[bn + "num_batches_tracked"] = 1
    return out


@functools.lru_cache(maxsize=None)
def reference(case, zero_row=None):
    """the shared fp64 / fp32 references of a named case, computed once (treat as read-only):
    dict(x, dout, out64, g64, dx64, stats64, g32, dx32, out32, run64, run32)"""
    seg_lens, seed = CASES[case]
    x, dout = features(seg_lens, seed, zero_row), upstream(len(seg_lens), seed)
    sd = weights(torch.float64)
    out64, g64, dx64, st64 = gradients(sd, x, seg_lens, dout)
    out32, g32, dx32, st32 = autograd(weights(torch.float32), x, seg_lens, dout, torch.float32)
    return dict(seg_lens=seg_lens, x=x, dout=dout, out64=out64, g64=g64, dx64=dx64, stats64=st64, out32=out32, g32=g32, dx32=dx32,
                run64=running_update(sd, st64), run32=running_update(weights(torch.float32), st32))
