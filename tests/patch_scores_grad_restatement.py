"""Restatement of lcr_patch_scores_grad (csrc/patch_scores.hip, include/lcr_hip.h) in plain torch, evaluated in the dtype of its inputs (fp64 = the
reference, fp32 = the yardstick of the tolerance), and the dense formula it is the gradient of.

    G[p]    = scale * dS[p][:K,:K], an entry of a masked row or column taken as zero BY SELECT (dS may hold NaN there); the dustbin row and
              column are never read
    dA_g[p] = G[p] . gather(feats_b, idx_b[p]),   dB_g[p] = G[p]^T . gather(feats_a, idx_a[p])
    d_feats_a[n] = the sum of dA_g[p][i] over the slots with idx_a[p,i] == n (d_feats_b likewise); the shadow index (== N) and any index
                   outside [0, N) receive nothing; a row nobody lists is exactly zero

`mistake` plants one error, each of which tests/test_pair_train_cpu.py shows the tolerance catches:
    "no_transpose"   G not transposed for side b
    "no_mask"        the mask ignored (finite dS only: the select is what keeps NaN out)
    "dustbin"        the dustbin column read as column K - 1
    "no_scale"       the scale dropped
    "shadow"         shadow slots counted (onto the last row)"""
import torch

MISTAKES = ("no_transpose", "no_mask", "dustbin", "no_scale", "shadow")


def gather(feats, idx):
    """rows idx of feats with a zero row for every index outside [0, N) (index_select on the zero-padded tensor)"""
    N = feats.shape[0]
    ok = (idx >= 0) & (idx < N)
    return torch.where(ok[..., None], feats[idx.clamp(0, max(N - 1, 0))], torch.zeros((), dtype=feats.dtype))


def patch_scores_grad(dS, feats_a, feats_b, idx_a, idx_b, mask_a, mask_b, scale, mistake=None):
    """(d_feats_a [Na,C], d_feats_b [Nb,C]) in the dtype of feats_a"""
    assert mistake is None or mistake in MISTAKES
    dt = feats_a.dtype
    P, K = idx_a.shape
    Na, Nb = feats_a.shape[0], feats_b.shape[0]
    if mistake == "dustbin":
        inner = torch.cat([dS[:, :K, :K - 1], dS[:, :K, K:K + 1]], 2).to(dt)
    else:
        inner = dS[:, :K, :K].to(dt)
    live = mask_a.bool()[:, :, None] & mask_b.bool()[:, None, :]
    if mistake == "no_mask":
        live = torch.ones_like(live)
    G = torch.where(live, inner * (1.0 if mistake == "no_scale" else scale), torch.zeros((), dtype=dt))
    dA = torch.bmm(G, gather(feats_b, idx_b))
    dB = torch.bmm(G if mistake == "no_transpose" else G.transpose(1, 2), gather(feats_a, idx_a))

    def scatter(prod, idx, N):
        out = torch.zeros((N, prod.shape[2]), dtype=dt)
        flat, rows = idx.reshape(-1), prod.reshape(-1, prod.shape[2])
        ok = (flat >= 0) & (flat < N)
        if mistake == "shadow" and N > 0:
            ok, flat = torch.ones_like(ok), flat.clamp(0, N - 1)
        out.index_add_(0, flat[ok], rows[ok])
        return out
    return scatter(dA, idx_a, Na), scatter(dB, idx_b, Nb)


def dense_scores(feats_a, feats_b, idx_a, idx_b, mask_a, mask_b, scale):
    """The forward by the dense formula torch differentiates — cat a zero row, index, bmm, masked select: the scaled products [P,K,K] with
    zeros at masked entries (what reaches the transport from the features)."""
    fa = torch.cat([feats_a, feats_a.new_zeros(1, feats_a.shape[1])])[idx_a.clamp(0, feats_a.shape[0])]
    fb = torch.cat([feats_b, feats_b.new_zeros(1, feats_b.shape[1])])[idx_b.clamp(0, feats_b.shape[0])]
    raw = torch.bmm(fa, fb.transpose(1, 2)) * scale
    live = mask_a.bool()[:, :, None] & mask_b.bool()[:, None, :]
    return torch.where(live, raw, torch.zeros((), dtype=raw.dtype))


def autograd_grad(dS, feats_a, feats_b, idx_a, idx_b, mask_a, mask_b, scale, dtype):
    """(d_feats_a, d_feats_b) of <dense_scores, dS[:, :K, :K]> by torch autograd in `dtype`; dS must be finite on the live entries (masked and
    dustbin entries are replaced by zero first: they do not enter the formula)"""
    K = idx_a.shape[1]
    a = feats_a.detach().clone().to(dtype).requires_grad_(True)
    b = feats_b.detach().clone().to(dtype).requires_grad_(True)
    live = mask_a.bool()[:, :, None] & mask_b.bool()[:, None, :]
    g = torch.where(live, dS[:, :K, :K].to(dtype), torch.zeros((), dtype=dtype))
    (dense_scores(a, b, idx_a, idx_b, mask_a, mask_b, scale) * g).sum().backward()
    return a.grad, b.grad


class Case:
    """seeded inputs of the kernel tests: P patches of K = 128 slots over Na / Nb rows, ~10 % of the slots masked and carrying the shadow
    index (one masked slot per patch and side keeps a real index, one live slot carries the shadow index), patch `single` with one live row, NaN planted at every masked and every dustbin entry of dS"""

    def __init__(self, name, P, C, Na, Nb, seed, single=None, disjoint=False, nan=True):
        self.name, self.P, self.C, self.Na, self.Nb, self.K = name, P, C, Na, Nb, 128
        g = torch.Generator().manual_seed(seed)
        K = self.K
        self.fa = torch.randn(Na, C, generator=g)
        self.fb = torch.randn(Nb, C, generator=g)
        if disjoint:                                   # every row listed at most once: a patch's rows are its own
            assert P * K <= Na and P * K <= Nb
            self.ia = torch.randperm(Na, generator=g)[:P * K].reshape(P, K)
            self.ib = torch.randperm(Nb, generator=g)[:P * K].reshape(P, K)
        else:
            self.ia = torch.randint(0, Na, (P, K), generator=g)
            self.ib = torch.randint(0, Nb, (P, K), generator=g)
        self.ma = torch.rand(P, K, generator=g) >= 0.1
        self.mb = torch.rand(P, K, generator=g) >= 0.1
        if single is not None:
            self.ma[single] = False
            self.ma[single, 77] = True
        self.ia[~self.ma] = Na
        self.ib[~self.mb] = Nb
        if not disjoint:                               # live slots that carry the shadow index too: a zero row forward, nothing backward;
            self.ia[:, 5], self.ib[:, 9] = Na, Nb      # and masked slots that keep a real index: only the mask keeps them out
            self.ma[0, 5] = self.mb[0, 9] = True
            self.ia[:, 20], self.ib[:, 30] = 3, 4
            self.ma[:, 20] = self.mb[:, 30] = False
        self.scale = 1.0 / C ** 0.5
        self.dS = torch.randn(P, K + 1, K + 1, generator=g)
        if nan:
            live = torch.zeros(P, K + 1, K + 1, dtype=torch.bool)
            live[:, :K, :K] = self.ma[:, :, None] & self.mb[:, None, :]
            self.dS[~live] = float("nan")
        self.ma8, self.mb8 = self.ma.to(torch.uint8), self.mb.to(torch.uint8)

    def args(self, dtype=None):
        f = (lambda t: t) if dtype is None else (lambda t: t.to(dtype))
        return f(self.dS), f(self.fa), f(self.fb), self.ia, self.ib, self.ma, self.mb, self.scale

    def unlisted(self):
        """(rows of feats_a, rows of feats_b) that no live or masked slot lists"""
        ua = torch.ones(self.Na, dtype=torch.bool)
        ua[self.ia[self.ia < self.Na]] = False
        ub = torch.ones(self.Nb, dtype=torch.bool)
        ub[self.ib[self.ib < self.Nb]] = False
        return ua, ub


def cases():
    # P = 3, Na = 150, Nb = 157: 384 slots over ~150 rows, so rows repeat within and across patches; patch 1 has a single live row
    return [Case("C32", 3, 32, 150, 157, 11, single=1), Case("C96", 3, 96, 150, 157, 12, single=1)]
