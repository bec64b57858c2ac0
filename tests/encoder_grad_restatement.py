"""Restatements of the encoder's reverse passes (csrc/kpconv_grad.hip, csrc/groupnorm_grad.hip) in plain torch, evaluated in the dtype of
their inputs (fp64 = the reference the kernels are held to), the problem generators the CPU and GPU files share, and the tolerance rule.

Every restatement is written out by hand (no autograd) and carries planted-mistake switches; tests/test_encoder_grad_cpu.py shows that
the clean form equals fp64 torch autograd through oracle/torch_ref and that every switch moves a result by far more than any tolerance.
Padding in an index list is any index outside [0, Ns); for oracle/torch_ref (one shadow row) `to_ref_idx` maps it to Ns.
"""
import math
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, SIGMA = 1.275, 0.6            # init_radius, init_sigma of the reference config
MARGIN = 1e-5                          # decision margin, relative to the tensor's magnitude


def bound(e_ref, scale):
    """The project's rule: four times the fp32 reference's own error, and never below 2^-20 of the result's magnitude."""
    return max(4.0 * e_ref, 2.0 ** -20 * scale)


def kernel_points(radius=RADIUS):
    kp = np.load(os.path.join(ROOT, "lcr-net_amd", "modules", "kpconv", "dispositions", "k_015_center_3D.npy"))
    return torch.from_numpy(np.ascontiguousarray(kp, dtype=np.float32).reshape(15, 3) * np.float32(radius))


def valid_mask(idx, Ns):
    return (idx >= 0) & (idx < Ns)


def to_ref_idx(idx, Ns):
    return torch.where(valid_mask(idx, Ns), idx, torch.full_like(idx, Ns)).long()


# ------------------------------------------------------------------------------------------------ restatements
def neighbor_transpose(idx, Ns):
    """(row_start [Ns + 1], edges [E]) as numpy int64: the flat positions of the valid entries, sorted by support index, ties by position."""
    flat = idx.reshape(-1).numpy().astype(np.int64)
    pos = np.nonzero((flat >= 0) & (flat < Ns))[0]
    order = np.argsort(flat[pos], kind="stable")
    edges = pos[order]
    row_start = np.searchsorted(flat[edges], np.arange(Ns + 1), side="left")
    return row_start.astype(np.int64), edges


def influences(q, s, idx, kp, sigma):
    """w [M, H, 15] = max(0, 1 - |s - q - kp| / sigma), zero at padding."""
    Ns = s.shape[0]
    ok = valid_mask(idx, Ns)
    j = torch.where(ok, idx, torch.zeros_like(idx)).long()
    rel = s[j] - q[:, None, :]
    d = ((rel[:, :, None, :] - kp[None, None].to(q.dtype)) ** 2).sum(-1).sqrt()
    return torch.clamp(1 - d / sigma, min=0.0) * ok[:, :, None].to(q.dtype), ok, j


def kpconv_aggregate_grad(dA, q, s, idx, kp, sigma, transpose_kc=False):
    """d_s_feats [Ns, C] from dA [M, 15 C].  transpose_kc: dA read as [M, C, 15] (planted mistake)."""
    M, C, Ns = q.shape[0], dA.shape[1] // 15, s.shape[0]
    w, ok, j = influences(q, s, idx, kp, sigma)
    g = dA.view(M, C, 15).transpose(1, 2) if transpose_kc else dA.view(M, 15, C)
    contrib = torch.einsum("mhk,mkc->mhc", w, g)
    out = torch.zeros(Ns, C, dtype=dA.dtype)
    out.index_add_(0, j[ok], contrib[ok])
    return out


def kpconv_grad(d_out, s_feats, q, s, idx, kp, sigma, W, drop_count=False, count_padding=False, transpose_kc=False):
    """(d_s_feats, dW [15, Cin, Cout], dbias) of the whole KPConv (any Cin; Cin = 1: s_feats [Ns, 1]).  The neighbour count (supports whose
    feature row sums to > 0, at least 1) is an integer without a gradient."""
    M, Ns, Cin = q.shape[0], s.shape[0], s_feats.shape[1]
    w, ok, j = influences(q, s, idx, kp, sigma)
    nf = s_feats[j] * ok[:, :, None].to(s_feats.dtype)
    if count_padding:
        cnt = ((nf.sum(-1) > 0) | ~ok).sum(-1).clamp(min=1)
    else:
        cnt = (nf.sum(-1) > 0).sum(-1).clamp(min=1)
    g = d_out if drop_count else d_out / cnt[:, None].to(d_out.dtype)
    A = torch.einsum("mhk,mhc->mkc", w, nf)                                  # [M, 15, Cin]
    dW = torch.einsum("mkc,mo->kco", A, g)
    dA = torch.einsum("mo,kco->mkc", g, W).reshape(M, 15 * Cin)
    return kpconv_aggregate_grad(dA, q, s, idx, kp, sigma, transpose_kc=transpose_kc), dW, d_out.sum(0)


def maxpool_winners(x, idx):
    """(winner column per (m, c) or -1, pooled [M, C]): the first real entry that holds the maximum; -1 when only the shadow row does."""
    Ns = x.shape[0]
    ok = valid_mask(idx, Ns)
    j = torch.where(ok, idx, torch.zeros_like(idx)).long()
    v = torch.where(ok[:, :, None], x[j], torch.full((), -math.inf, dtype=x.dtype))
    pooled = v.max(1)[0]
    if (~ok).any():
        pooled = torch.where((~ok).any(1)[:, None], pooled.clamp(min=0.0), pooled)
    hit = (v == pooled[:, None, :]) & ok[:, :, None]
    first = torch.where(hit.any(1), hit.to(torch.int64).argmax(1), torch.full((), -1, dtype=torch.int64))
    return first, pooled, hit, j


def maxpool_grad(d_out, x, idx, all_ties=False):
    """d_x [Ns, C].  all_ties: every neighbour that holds the maximum gets the gradient (planted mistake)."""
    first, _, hit, j = maxpool_winners(x, idx)
    M, H = idx.shape
    sel = hit if all_ties else (torch.arange(H)[None, :, None] == first[:, None, :])
    out = torch.zeros_like(x)
    out.index_add_(0, j.reshape(-1), (sel.to(x.dtype) * d_out[:, None, :]).reshape(M * H, -1))
    return out


def _segments(N, seg):
    seg = [N] if seg is None else [int(v) for v in seg]
    assert sum(seg) == N
    return seg


def group_stats(x, groups, seg):
    """(mean [N, C], rstd [N, C]) broadcast per (segment, group); biased variance, eps 1e-5."""
    N, C = x.shape
    gs = C // groups
    mean, rstd = torch.empty_like(x), torch.empty_like(x)
    o = 0
    for n in _segments(N, seg):
        v = x[o:o + n].reshape(n, groups, gs)
        m = v.mean((0, 2), keepdim=True)
        var = ((v - m) ** 2).mean((0, 2), keepdim=True)
        mean[o:o + n] = m.expand(n, groups, gs).reshape(n, C)
        rstd[o:o + n] = (1.0 / torch.sqrt(var + 1e-5)).expand(n, groups, gs).reshape(n, C)
        o += n
    return mean, rstd


def groupnorm_apply(x, gamma, beta, groups, seg=None, res=None, res_norm=None, slope=0.1, act=True):
    """y = act(GN(x) [+ res | + GN(res; rgamma, rbeta)]) -> (y, z)."""
    mean, rstd = group_stats(x, groups, seg)
    z = (x - mean) * rstd * gamma + beta
    if res is not None:
        if res_norm is not None:
            rm, rr = group_stats(res, groups, seg)
            z = z + (res - rm) * rr * res_norm[0] + res_norm[1]
        else:
            z = z + res
    return (torch.where(z > 0, z, z * slope) if act else z), z


def _gn_reverse(x, gamma, dz, groups, seg, drop_xhat_term=False, const_stats=False):
    N, C = x.shape
    gs = C // groups
    mean, rstd = group_stats(x, groups, seg)
    xh = (x - mean) * rstd
    g = dz * gamma
    dx = torch.empty_like(x)
    o = 0
    for n in _segments(N, seg):
        gg, hh = g[o:o + n].reshape(n, groups, gs), xh[o:o + n].reshape(n, groups, gs)
        m1 = gg.mean((0, 2), keepdim=True)
        m2 = (gg * hh).mean((0, 2), keepdim=True)
        if const_stats:
            d = gg
        elif drop_xhat_term:
            d = gg - m1
        else:
            d = gg - m1 - hh * m2
        dx[o:o + n] = d.reshape(n, C)
        o += n
    return dx * rstd, (dz * xh).sum(0), dz.sum(0)


def groupnorm_apply_grad(x, gamma, y, dy, groups, seg=None, slope=0.1, act=True, res=None, res_gamma=None, drop_xhat_term=False,
                         const_stats=False, no_slope=False):
    """dict(dx, dgamma, dbeta, dz [, dres, drgamma, drbeta]).  y: the forward's output (the LeakyReLU mask: y > 0, so y == 0 takes the slope).
    res given with res_gamma: a normalised residual; res given alone: a plain one (its gradient is dz)."""
    dz = dy * torch.where(y > 0, torch.ones_like(dy), torch.full_like(dy, 1.0 if no_slope else slope)) if act else dy.clone()
    dx, dgamma, dbeta = _gn_reverse(x, gamma, dz, groups, seg, drop_xhat_term, const_stats)
    out = dict(dx=dx, dgamma=dgamma, dbeta=dbeta, dz=dz)
    if res is not None:
        if res_gamma is None:
            out["dres"] = dz
        else:
            out["dres"], out["drgamma"], out["drbeta"] = _gn_reverse(res, res_gamma, dz, groups, seg, drop_xhat_term, const_stats)
    return out


# ------------------------------------------------------------------------------------------------ problems
def ball(gen, n, radius):
    v = torch.randn(n, 3, generator=gen)
    v = v / v.norm(dim=1, keepdim=True).clamp(min=1e-9)
    return (v * radius * torch.rand(n, 1, generator=gen) ** (1.0 / 3.0)).float()


class KPProblem:
    """q [M,3], s [Ns,3] in a ball of the block's radius, idx [M,H] int32 (padding: -1 or an index >= Ns), the module's kernel points and sigma."""

    def __init__(self, name, M, Ns, H, C, seed=0, pad_frac=0.15, idx=None, int64=False):
        gen = torch.Generator().manual_seed(1000 + seed)
        self.name, self.M, self.Ns, self.H, self.C = name, M, Ns, H, C
        self.q, self.s = ball(gen, M, RADIUS), ball(gen, Ns, RADIUS)
        if idx is None:
            idx = torch.randint(0, Ns, (M, H), generator=gen)
            pad = torch.rand(M, H, generator=gen) < pad_frac
            idx = torch.where(pad, torch.where(torch.rand(M, H, generator=gen) < 0.5, torch.full_like(idx, -1), torch.full_like(idx, Ns + 3)), idx)
        self.idx = idx.to(torch.int64 if int64 else torch.int32).contiguous()
        self.kp, self.sigma = kernel_points(), SIGMA
        self.dA = torch.randn(M, 15 * C, generator=gen)
        self.gen = gen


def kp_cases():
    """The aggregate-gradient cases of the GPU file, as (M, Ns, H, C) and what each is there for."""
    cases = [KPProblem("1x1x1-c32", 1, 1, 1, 32, 1, pad_frac=0.0)]
    cases[0].s = cases[0].q + torch.tensor([[0.05, -0.1, 0.2]])      # inside the centre kernel point's reach: one non-zero influence
    idx = torch.tensor([[0, 0, -1], [1, 2, 9], [4, 4, 4], [-1, -1, 3], [2, 0, 1], [3, 3, 0], [5, 7, 1]])   # padding, one support twice in a row
    cases.append(KPProblem("7x5x3-c32", 7, 5, 3, 32, 2, idx=idx))
    cases.append(KPProblem("40x33x65-c64", 40, 33, 65, 64, 3))
    cases.append(KPProblem("33x70x128-c128", 33, 70, 128, 128, 4))
    cases.append(KPProblem("19x23x17-c256", 19, 23, 17, 256, 5))
    cases.append(KPProblem("strided-12x90x40-c64", 12, 90, 40, 64, 6))
    gen = torch.Generator().manual_seed(77)
    hub = torch.randint(1, 20, (300, 6), generator=gen)          # supports 20 .. 39 are listed by nobody
    hub[:, 2] = 0                                                # every query lists support 0
    cases.append(KPProblem("hub-300x40x6-c64", 300, 40, 6, 64, 7, idx=hub))
    padrow = torch.randint(0, 11, (9, 5), generator=gen)
    padrow[4] = -1                                               # a row of padding only
    cases.append(KPProblem("padrow-9x11x5-c32", 9, 11, 5, 32, 8, idx=padrow))
    cases.append(KPProblem("int64-21x18x33-c128", 21, 18, 33, 128, 9, int64=True))
    return cases


# (N, C, groups, segments)
GN_SHAPES = [(1, 32, 32, [1]), (37, 64, 32, [37]), (130, 128, 32, [1, 63, 64, 2]), (200, 256, 32, [65, 135]), (5, 1024, 32, [5])]


class GNProblem:
    def __init__(self, N, C, groups, seg, seed=0, mean_over_sigma=0.0):
        gen = torch.Generator().manual_seed(2000 + seed)
        self.N, self.C, self.groups, self.seg = N, C, groups, seg
        self.x = (torch.randn(N, C, generator=gen) + mean_over_sigma).float()
        self.res = torch.randn(N, C, generator=gen).float()
        self.gamma, self.beta = (1 + 0.3 * torch.randn(C, generator=gen)).float(), (0.2 * torch.randn(C, generator=gen)).float()
        self.rgamma, self.rbeta = (1 + 0.3 * torch.randn(C, generator=gen)).float(), (0.2 * torch.randn(C, generator=gen)).float()
        self.dy = torch.randn(N, C, generator=gen).float()


def relu_margin(z):
    """min |z| / max |z| of a pre-activation tensor: the distance of the nearest LeakyReLU decision from its edge"""
    z = z.double()
    return float(z.abs().min() / z.abs().max().clamp(min=1e-300))


def maxpool_margin(x, idx):
    """the smallest gap between a column's maximum and its runner-up among DISTINCT supports (and the shadow zero), over max |x|"""
    x = x.double()
    Ns = x.shape[0]
    ok = valid_mask(idx, Ns)
    gap = math.inf
    for m in range(idx.shape[0]):
        rows = torch.unique(idx[m][ok[m]].long())
        v = x[rows]
        if (~ok[m]).any():
            v = torch.cat([v, torch.zeros(1, x.shape[1], dtype=x.dtype)], 0)
        if v.shape[0] > 1:
            top = v.topk(2, dim=0)[0]
            gap = min(gap, float((top[0] - top[1]).min()))
    return gap / float(x.abs().max())


def count_margin(s_feats, scale=None):
    """min |row sum| / max |s_feats|: how far every KPConv neighbour-count decision (row sum > 0) is from its edge"""
    s = s_feats.double()
    return float(s.sum(-1).abs().min() / (s.abs().max() if scale is None else scale))
