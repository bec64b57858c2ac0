"""fp64 torch restatement of the KPConv encoder's operators (csrc/groupnorm.hip, csrc/kpconv.hip, lcr_gemm_f32_anorm of csrc/gemm_f32.hip), one
function per operator; the shared inputs and case tables of tests/test_encoder_ops_cpu.py and tests/test_encoder_ops_gpu.py; and the calibration
constants the GPU tolerances come from.

What each function restates (the reference locations are those cited at the top of oracle/torch_ref.py and in the kernels' headers):
    gn_stats, gn_apply   GroupNorm.forward, modules/kpconv/modules.py:33-50 (nn.GroupNorm(32, C): biased variance, eps 1e-5), restarted per
                         segment; UnaryBlock / ConvBlock :78-84, :140-145 and the tail of ResidualBlock :207-225 (LeakyReLU 0.1 after the sum);
                         the row flag is the `sum over channels > 0` of kpconv.py:113-114
    anorm_gemm           ResidualBlock norm_conv -> LeakyReLU -> unary2's Linear, modules.py:215-217
    kpconv_aggregate,    KPConv.forward, modules/kpconv/kpconv.py:79-122 (linear influence, shadow neighbour, neighbour-count normalisation)
    kpconv, kpconv_cin1
    maxpool              kpconv/functional.py:54-67 (the zero shadow row takes part)
    row_positive         kpconv.py:113-114
Every function computes in the dtype of its inputs and spells every sum as a torch.matmul, so the same code gives the fp64 reference and —
inside netvlad_restatement.pinned_fp32_matmul — the fp32 floor with its sums in plain index order.  GroupNorm is written by hand (two passes:
mean, then mean of squared deviations), not through F.group_norm, so that one-row segments work.

`mutate=` plants exactly ONE wrong step (MUTATIONS).  The CPU test measures how far each moves the fp64 result on the cases meant to catch it
(ASSIGNED) and demands SENSITIVITY x the GPU tolerance.
"""
import functools

import numpy as np
import torch

EPS, SLOPE = 1e-5, 0.1
NORTH_STAR = 1e-4        # the project's bound (relative to max(1, |want|max))
MARGIN = 4               # a kernel may order its sums differently from the floor run (as in netvlad_restatement)
SENSITIVITY = 20
AMBIGUOUS = 1e-5         # a row whose |sum_c| is below AMBIGUOUS * sum_c |.| may legitimately get either flag
AMBIGUOUS_CAP = 0.01     # ... and at most this share of a case's rows may be that
# |mean| / std of the tensors entering the encoder's GroupNorms: worst per-(segment, group) value 4.34 (tests/test_encoder_ops_cpu.py holds the
# table); the offset cases use twice that, rounded up
WORST_MEASURED_RATIO = 4.34
OFFSET = 9

# ------------------------------------------------------------------------------------------------ calibration (tests/test_encoder_ops_cpu.py)
# max |fp32 restatement - fp64 restatement| / max(1, |want|max) over every case of the GPU file, the fp32 sums in plain index order;
# "gn_var" is the error of the per-(segment, group) biased variance of the centred cases relative to variance + eps, the quantity the
# normalisation uses and the metric of the GPU file.  test_fp32_floor_matches_committed_constant
# recomputes them and fails when one leaves [FLOOR / 2, 2 FLOOR].
FLOOR = {"gn_mean": 1.8e-7, "gn_var": 1.4e-5, "gn_apply": 5.5e-6, "anorm_gemm": 5.8e-7, "kpconv_aggregate": 2.7e-7, "kpconv": 5.7e-7,
         "kpconv_cin1": 2.5e-7}
TOL = {k: min(NORTH_STAR, MARGIN * v) for k, v in FLOOR.items()}

MUTATIONS = {
    "gn_apply": ("unbiased_variance", "eps_dropped", "first_row_previous_stats", "last_row_next_stats", "wrong_group_size",
                 "residual_with_x_affine", "act_before_residual", "flag_from_x"),
    "kpconv": ("count_unclamped", "count_from_valid", "shadow_contributes", "influence_unclamped", "w_blocks_permuted", "bias_before_division"),
    "maxpool": ("ignore_shadow", "drop_last_ragged"),
}
_ALL_MUTATIONS = {m for v in MUTATIONS.values() for m in v}


def _ones(n, like):
    return torch.ones(n, 1, dtype=like.dtype)


def _bounds(seg_lens):
    o = np.concatenate([[0], np.cumsum(seg_lens)]).astype(np.int64)
    return [(int(o[s]), int(o[s + 1])) for s in range(len(seg_lens))]


# ------------------------------------------------------------------------------------------------ GroupNorm
def _group_sums(blk):
    """blk [n, G, gs] -> [G]: the sum over the rows and the channels of every group (one index-order chain per group)."""
    n, G, gs = blk.shape
    return torch.matmul(blk.permute(1, 0, 2).reshape(G, n * gs), _ones(n * gs, blk))[:, 0]


def gn_stats(x, seg_lens, groups):
    """[S, groups, 2]: (sum x, sum x^2) per (segment, group); zero rows for a zero-length segment."""
    n, C = x.shape
    out = torch.zeros(len(seg_lens), groups, 2, dtype=x.dtype)
    for s, (lo, hi) in enumerate(_bounds(seg_lens)):
        if hi > lo:
            blk = x[lo:hi].reshape(hi - lo, groups, C // groups)
            out[s, :, 0], out[s, :, 1] = _group_sums(blk), _group_sums(blk * blk)
    return out


def gn_moments(x, seg_lens, groups, unbiased=False):
    """(mean, variance) [S, groups] of every (segment, group), two passes; zeros for a zero-length segment."""
    n, C = x.shape
    gs = C // groups
    mean, var = torch.zeros(len(seg_lens), groups, dtype=x.dtype), torch.zeros(len(seg_lens), groups, dtype=x.dtype)
    for s, (lo, hi) in enumerate(_bounds(seg_lens)):
        if hi == lo:
            continue
        cnt = (hi - lo) * gs
        blk = x[lo:hi].reshape(hi - lo, groups, gs)
        mean[s] = _group_sums(blk) / cnt
        dev = blk - mean[s][None, :, None]
        var[s] = _group_sums(dev * dev) / (max(cnt - 1, 1) if unbiased else cnt)
    return mean, var


def moments_from_sums(sums, seg_lens, gs):
    """What the kernels derive from a statistics table [S, groups, 2] (replicas already folded): mean and biased variance, in fp64."""
    cnt = torch.tensor([max(int(n), 1) * gs for n in seg_lens], dtype=torch.float64)[:, None]
    mean = sums[..., 0].double() / cnt
    return mean, sums[..., 1].double() / cnt - mean * mean


def _normalise(x, seg_lens, groups, gamma, beta, mutate, eps):
    n, C = x.shape
    gs = C // groups
    mean, var = gn_moments(x, seg_lens, groups, unbiased=mutate == "unbiased_variance")
    rstd = 1.0 / torch.sqrt(var + (0.0 if mutate == "eps_dropped" else eps))
    seg = torch.zeros(n, dtype=torch.int64)                       # the segment whose statistics normalise each row
    live = [(s, lo, hi) for s, (lo, hi) in enumerate(_bounds(seg_lens)) if hi > lo]
    for i, (s, lo, hi) in enumerate(live):
        seg[lo:hi] = s
        if mutate == "first_row_previous_stats" and i > 0:
            seg[lo] = live[i - 1][0]
        if mutate == "last_row_next_stats" and i + 1 < len(live):
            seg[hi - 1] = live[i + 1][0]
    grp = torch.arange(C) // gs
    if mutate == "wrong_group_size":
        grp = (torch.arange(C) // (2 * gs)).clamp(max=groups - 1)
    m, r = mean[seg][:, grp], rstd[seg][:, grp]
    return (x - m) * r * gamma[None] + beta[None]


def leaky(x, slope=SLOPE):
    return torch.where(x > 0, x, x * slope)


def row_sums(x):
    """(sum_c x, sum_c |x|) per row."""
    return torch.matmul(x, _ones(x.shape[1], x))[:, 0], torch.matmul(x.abs(), _ones(x.shape[1], x))[:, 0]


def ambiguous_rows(x):
    s, a = row_sums(x)
    return s.abs() < AMBIGUOUS * a


def gn_apply(x, seg_lens, groups, gamma, beta, res=None, res_gamma=None, res_beta=None, act=True, slope=SLOPE, eps=EPS, mutate=None):
    """y = act(GN(x) [+ res | + GN_res(res)]) and the row flag sum_c y > 0.  res_gamma given: the residual is GroupNorm-ed with its own affine."""
    assert mutate is None or mutate in MUTATIONS["gn_apply"], mutate
    y = _normalise(x, seg_lens, groups, gamma, beta, mutate, eps)
    if mutate == "act_before_residual" and act:
        y = leaky(y, slope)
    if res is not None:
        if res_gamma is not None:
            rg, rb = (gamma, beta) if mutate == "residual_with_x_affine" else (res_gamma, res_beta)
            y = y + _normalise(res, seg_lens, groups, rg, rb, mutate, eps)
        else:
            y = y + res
    if act and mutate != "act_before_residual":
        y = leaky(y, slope)
    flag = row_sums(x if mutate == "flag_from_x" else y)[0] > 0
    return y, flag


def anorm_gemm(a, seg_lens, a_groups, gamma, beta, weight, bias, groups, slope=SLOPE, eps=EPS):
    """C = leaky(GN(a)) . weight^T (+ bias) and its (sum, sum of squares) per (segment, output group)."""
    h = leaky(_normalise(a, seg_lens, a_groups, gamma, beta, None, eps), slope)
    c = torch.matmul(h, weight.t().contiguous())
    if bias is not None:
        c = c + bias[None]
    return c, gn_stats(c, seg_lens, groups)


# ------------------------------------------------------------------------------------------------ KPConv
def kpconv_aggregate(s_feats, q_pts, s_pts, idx, kp, sigma, mutate=None):
    """A [M, 15, C] = sum over the valid neighbours of influence x feature row, and the count max(1, #{valid neighbours whose feature row sums
    to > 0}).  An index outside [0, Ns) is the shadow neighbour: no influence, no count."""
    assert mutate is None or mutate in MUTATIONS["kpconv"], mutate
    Ns = s_feats.shape[0]
    idx = idx.long()
    valid = (idx >= 0) & (idx < Ns)
    takes_part = torch.ones_like(valid) if mutate == "shadow_contributes" else valid       # the planted mistake: an index folded into range
    j = torch.where(valid, idx, (idx * 7 + 3) % Ns)
    nb = s_pts[j] - q_pts[:, None, :]                                                   # [M,H,3]
    e = nb[:, :, None, :] - kp[None, None]                                              # [M,H,15,3]
    d = torch.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2])
    w = 1 - d / sigma
    if mutate != "influence_unclamped":
        w = w.clamp(min=0.0)
    w = w * takes_part[:, :, None].to(w.dtype)
    A = torch.matmul(w.transpose(1, 2).contiguous(), s_feats[j])                        # [M,15,H] @ [M,H,C]
    positive = row_sums(s_feats)[0] > 0
    cnt = (valid if mutate == "count_from_valid" else (positive[j] & valid)).sum(1)
    if mutate != "count_unclamped":
        cnt = cnt.clamp(min=1)
    return A, cnt


def kpconv(s_feats, q_pts, s_pts, idx, kp, sigma, weights, bias=None, seg_lens=None, groups=0, mutate=None):
    """weights [15, C, O]: out = A . W / count (+ bias); with seg_lens and groups also the output's (sum, sum of squares) table."""
    A, cnt = kpconv_aggregate(s_feats, q_pts, s_pts, idx, kp, sigma, mutate)
    K, C, O = weights.shape
    W = weights.roll(1, dims=0) if mutate == "w_blocks_permuted" else weights
    out = torch.matmul(A.reshape(A.shape[0], K * C), W.reshape(K * C, O))
    div = cnt.to(out.dtype)[:, None]
    if bias is None:
        out = out / div
    elif mutate == "bias_before_division":
        out = (out + bias[None]) / div
    else:
        out = out / div + bias[None]
    sums = gn_stats(out, seg_lens, groups) if groups else None
    return out, sums, cnt


def kpconv_cin1(s_feats, q_pts, s_pts, idx, kp, sigma, weights, bias=None, mutate=None):
    """One input channel: s_feats [Ns], weights [15, 1, O]; a neighbour counts when its scalar feature is > 0."""
    out, _, cnt = kpconv(s_feats.reshape(-1, 1), q_pts, s_pts, idx, kp, sigma, weights, bias, mutate=mutate)
    return out, cnt


def maxpool(x, idx, mutate=None):
    assert mutate is None or mutate in MUTATIONS["maxpool"], mutate
    Ns, H = x.shape[0], idx.shape[1]
    idx = idx.long()
    valid = (idx >= 0) & (idx < Ns)
    g = torch.cat([x, torch.zeros_like(x[:1])], 0)[torch.where(valid, idx, torch.full_like(idx, Ns))]      # [M,H,C]
    if mutate == "ignore_shadow":
        g = g.masked_fill(~valid[:, :, None], float("-inf"))
    if mutate == "drop_last_ragged":
        n = valid.sum(1)
        last = (valid.long() * (torch.arange(H) + 1)[None]).argmax(1)
        rows = torch.nonzero((n % 8 != 0) & (n > 0))[:, 0]
        g[rows, last[rows]] = float("-inf")
    return g.max(1)[0]


def row_positive(x):
    return row_sums(x)[0] > 0


def shift_of(a, b):
    """max |a - b|, a non-finite difference counting as infinite."""
    d = (a.double() - b.double()).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
    return d.max().item() if d.numel() else 0.0


# ------------------------------------------------------------------------------------------------ cases: GroupNorm
# one- and two-row segments alone; 63 | 1 | 64 | 65; a long segment, three one-row ones (a workgroup's row range spans >= 3 segments) and another
# long one; zero-length segments inside the table; boundaries at rows 64k - 1, 64k and 64k + 1
SEG_TABLES = {"one": (1,), "two": (2,), "small": (63, 1, 64, 65), "mixed": (700, 1, 1, 1, 300), "empty": (70, 0, 130, 0, 1, 40),
              "edges64": (63, 1, 1, 62, 1, 1, 70)}
GN_SHAPES = ((32, 32), (64, 32), (128, 32), (256, 32), (1024, 32), (128, 2), (256, 2))      # (C, groups): 1 .. 32 channels per group, 64, 128
GN_ODD_SHAPES = ((24, 6), (40, 10), (96, 12))               # C / 4 does not divide 256: lcr_groupnorm_apply's general form without a fixed channel
GN_NON_POW2 = ((96, 32), (48, 16))                          # three channels per group: to be rejected (or computed right)
SHIFTS = (0, OFFSET)
RES_MODES = (0, 1, 2)                                       # none, plain residual, GroupNorm-ed residual


def _seed(*parts):
    import zlib
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def gn_case(C, groups, table, shift):
    """fp32 inputs of a GroupNorm case (cached: treat as read-only).  x = (N(0,1) + shift + a per-channel offset of at most 0.25) x a per-segment
    scale in {1, 1.5, 2}: neighbouring segments have different statistics, channels of one group different means, and |mean| / std is `shift`
    (up to the 0.25)."""
    seg_lens = SEG_TABLES[table]
    n = int(sum(seg_lens))
    g = torch.Generator().manual_seed(_seed("gn", C, groups, table, shift))
    x = torch.randn(n, C, generator=g) + float(shift) + 0.25 * torch.cos(torch.arange(C, dtype=torch.float32))[None]
    for s, (lo, hi) in enumerate(_bounds(seg_lens)):
        x[lo:hi] *= 1.0 + 0.5 * (s % 3)
    r = torch.randn(n, C, generator=g) * 1.5 + float(shift)
    return {"C": C, "groups": groups, "seg_lens": seg_lens, "shift": shift, "x": x, "res": r,
            "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g),
            "res_gamma": torch.rand(C, generator=g) + 0.5, "res_beta": torch.randn(C, generator=g)}


def gn_case_names(shapes=GN_SHAPES + GN_ODD_SHAPES):
    return [(C, G, t, sh) for (C, G) in shapes for t in SEG_TABLES for sh in SHIFTS]


def cast(case, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in case.items()}


def gn_apply_of(case, res_mode, act=True, mutate=None):
    c = case
    kw = {}
    if res_mode >= 1:
        kw["res"] = c["res"]
    if res_mode == 2:
        kw["res_gamma"], kw["res_beta"] = c["res_gamma"], c["res_beta"]
    return gn_apply(c["x"], c["seg_lens"], c["groups"], c["gamma"], c["beta"], act=act, mutate=mutate, **kw)


@functools.lru_cache(maxsize=None)
def gn_reference(C, groups, table, shift, res_mode, act=True, mutate=None):
    """(y, flag) in fp64 (cached; computed once and shared — do not modify)."""
    return gn_apply_of(cast(gn_case(C, groups, table, shift), torch.float64), res_mode, act, mutate)


@functools.lru_cache(maxsize=None)
def gn_moments_reference(C, groups, table, shift):
    c = cast(gn_case(C, groups, table, shift), torch.float64)
    return gn_moments(c["x"], c["seg_lens"], groups)


# ------------------------------------------------------------------------------------------------ cases: GEMM epilogue statistics
GEMM_STATS_K = 16


@functools.lru_cache(maxsize=None)
def gemm_stats_case(C, groups, table, shift):
    """a [n, 16], unit rows b [C, 16] and a bias so that c = a . b^T + bias has the statistics of gn_case: unit variance times the segment's
    scale, mean `shift` plus the per-channel offset."""
    seg_lens = SEG_TABLES[table]
    n = int(sum(seg_lens))
    g = torch.Generator().manual_seed(_seed("gemm_stats", C, groups, table, shift))
    a = torch.randn(n, GEMM_STATS_K, generator=g)
    for s, (lo, hi) in enumerate(_bounds(seg_lens)):
        a[lo:hi] *= 1.0 + 0.5 * (s % 3)
    b = torch.randn(C, GEMM_STATS_K, generator=g)
    b = b / b.norm(dim=1, keepdim=True)
    bias = float(shift) + 0.25 * torch.cos(torch.arange(C, dtype=torch.float32))
    return {"C": C, "groups": groups, "seg_lens": seg_lens, "a": a, "b": b, "bias": bias,
            "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g)}


@functools.lru_cache(maxsize=None)
def gemm_stats_reference(C, groups, table, shift):
    """fp64: (c, mean, var, y = GN(c) without activation)."""
    k = cast(gemm_stats_case(C, groups, table, shift), torch.float64)
    c = torch.matmul(k["a"], k["b"].t()) + k["bias"][None]
    mean, var = gn_moments(c, k["seg_lens"], groups)
    y, _ = gn_apply(c, k["seg_lens"], groups, k["gamma"], k["beta"], act=False)
    return c, mean, var, y


# ------------------------------------------------------------------------------------------------ cases: normalise-on-load GEMM
ANORM_K = (4, 32, 64, 128, 256)
ANORM_N = (36, 64, 100, 256)
# every segment holds >= 64 rows (the entry's contract): M = 64, 65, 130 (a boundary inside the second 64-row block), 777 (two segments of
# exactly 64 rows, then boundaries inside a block)
ANORM_SEGS = ((64,), (65,), (65, 65), (64, 64, 200, 449))
ANORM_A_GROUPS = {4: 2, 32: 32, 64: 32, 128: 32, 256: 32}
ANORM_GROUPS = {36: 9, 64: 32, 100: 25, 256: 32}


def anorm_case_names():
    """(K, N, segment table index, with bias): every K with every N; the four row counts and bias on / off cycle through them."""
    out = []
    for i, K in enumerate(ANORM_K):
        for j, N in enumerate(ANORM_N):
            out.append((K, N, (i + j) % len(ANORM_SEGS), (i + 2 * j) % 2 == 0))
    return out


@functools.lru_cache(maxsize=None)
def anorm_case(K, N, seg_i, with_bias):
    seg_lens = ANORM_SEGS[seg_i]
    M = int(sum(seg_lens))
    g = torch.Generator().manual_seed(_seed("anorm", K, N, seg_i, with_bias))
    a = torch.randn(M, K, generator=g) * 2.0 + 0.7
    for s, (lo, hi) in enumerate(_bounds(seg_lens)):
        a[lo:hi] *= 1.0 + 0.5 * (s % 3)
    return {"seg_lens": seg_lens, "a": a, "a_groups": ANORM_A_GROUPS[K], "groups": ANORM_GROUPS[N],
            "gamma": torch.rand(K, generator=g) + 0.5, "beta": torch.randn(K, generator=g),
            "weight": torch.randn(N, K, generator=g) / K ** 0.5, "bias": torch.randn(N, generator=g) if with_bias else None}


def anorm_of(c):
    return anorm_gemm(c["a"], c["seg_lens"], c["a_groups"], c["gamma"], c["beta"], c["weight"], c["bias"], c["groups"])


@functools.lru_cache(maxsize=None)
def anorm_reference(K, N, seg_i, with_bias):
    return anorm_of(cast(anorm_case(K, N, seg_i, with_bias), torch.float64))


# ------------------------------------------------------------------------------------------------ cases: KPConv, max-pool
KP_SIGMA, KP_EXTENT = 1.2, 3.0
AGG_C, AGG_H = (32, 64, 128, 256), (1, 9, 64, 65, 128)
CIN1_COUT, CIN1_H = (1, 32, 64, 65, 130, 256), (1, 40, 64, 65, 100)
POOL_C, POOL_H = (32, 96, 128, 384, 256, 512, 1024), (1, 7, 8, 9, 128)
KP_M, KP_NS = 150, 200


def kernel_points():
    from lcrnet_amd.weights import base_kernel_points
    return np.ascontiguousarray(base_kernel_points() * 1.5, dtype=np.float32)


def neighbour_lists(M, Ns, H, g):
    """int64 [M, H]: random supports, valid ones first up to a random fill, then the shadow index Ns — with holes: negative indices (also in
    front of valid ones) and indices beyond Ns.  Rows 0, 7, 14, ... have no neighbour at all, rows 1, 8, ... exactly one (in the LAST
    column), rows 2, 9, ... a full list."""
    idx = torch.randint(0, Ns, (M, H), generator=g, dtype=torch.int64)
    fill = torch.randint(0, H + 1, (M,), generator=g)
    fill[2::7] = H
    idx[torch.arange(H)[None, :] >= fill[:, None]] = Ns
    hole = torch.rand(M, H, generator=g) < 0.05
    hole[2::7] = False
    idx[hole] = torch.tensor([-1, -5, Ns + 3])[torch.randint(0, 3, (int(hole.sum()),), generator=g)]
    idx[0::7] = Ns
    idx[1::7] = Ns
    idx[1::7, H - 1] = torch.randint(0, Ns, (len(idx[1::7]),), generator=g)
    idx[3::14, 0] = -1
    return idx


def _points(M, Ns, g):
    s_pts = torch.rand(Ns, 3, generator=g) * KP_EXTENT
    q_pts = s_pts[torch.randint(0, Ns, (M,), generator=g)].contiguous() + 0.05 * torch.randn(M, 3, generator=g)
    return q_pts, s_pts


@functools.lru_cache(maxsize=None)
def kpconv_case(C, H, Cout=None, with_bias=True, seg_lens=None):
    """Supports whose feature rows are N(0,1), every fifth negated to a non-positive sum, every eleventh all zero (a valid neighbour that does
    not count).  Cout: also weights [15, C, Cout] and a bias."""
    M, Ns = (KP_M, KP_NS) if seg_lens is None else (int(sum(seg_lens)), KP_NS)
    g = torch.Generator().manual_seed(_seed("kpconv", C, H, Cout, with_bias, seg_lens))
    q_pts, s_pts = _points(M, Ns, g)
    feats = torch.randn(Ns, C, generator=g)
    feats[::5] = -feats[::5].abs()
    feats[::11] = 0.0
    out = {"q_pts": q_pts, "s_pts": s_pts, "idx": neighbour_lists(M, Ns, H, g), "feats": feats, "kp": torch.from_numpy(kernel_points()),
           "sigma": KP_SIGMA, "order": torch.randperm(M, generator=g).to(torch.int32), "seg_lens": seg_lens}
    if Cout is not None:
        out["weights"] = torch.randn(15, C, Cout, generator=g) / (15 * C) ** 0.5
        out["bias"] = torch.randn(Cout, generator=g) if with_bias else None
    return out


def aggregate_of(c, mutate=None):
    return kpconv_aggregate(c["feats"], c["q_pts"], c["s_pts"], c["idx"], c["kp"], c["sigma"], mutate)


def kpconv_of(c, groups=0, mutate=None):
    return kpconv(c["feats"], c["q_pts"], c["s_pts"], c["idx"], c["kp"], c["sigma"], c["weights"], c["bias"], c["seg_lens"], groups, mutate)


@functools.lru_cache(maxsize=None)
def aggregate_reference(C, H):
    return aggregate_of(cast(kpconv_case(C, H), torch.float64))


FUSED_TABLES = ("small", "mixed", "empty", "edges64", "one", "two")
FUSED_H = {"small": 9, "mixed": 65, "empty": 64, "edges64": 128, "one": 1, "two": 9}
FUSED_GROUPS = (32, 2)


@functools.lru_cache(maxsize=None)
def fused_case(table, shift):
    """C_in = C_out = 32 on the rows of a GroupNorm segment table; the bias is `shift` output standard deviations (of the fp64 output without
    bias) plus a per-channel offset, so that the output statistics have |mean| / std ~ shift."""
    c = dict(kpconv_case(32, FUSED_H[table], 32, True, SEG_TABLES[table]))
    c64 = cast(c, torch.float64)
    c64["bias"] = None
    out0 = kpconv_of(c64)[0]
    std = out0.std().item() if out0.numel() > 1 else 1.0
    c["bias"] = ((float(shift) + 0.25 * torch.cos(torch.arange(32, dtype=torch.float64))) * max(std, 1e-3)).float()
    return c


@functools.lru_cache(maxsize=None)
def fused_reference(table, shift, groups, mutate=None):
    return kpconv_of(cast(fused_case(table, shift), torch.float64), groups, mutate)


def cin1_case_names():
    return [(Cout, H, (i + j) % 2 == 0) for i, Cout in enumerate(CIN1_COUT) for j, H in enumerate(CIN1_H)]


@functools.lru_cache(maxsize=None)
def cin1_case(Cout, H, with_bias):
    """Scalar features drawn from {negative, 0, positive}."""
    g = torch.Generator().manual_seed(_seed("cin1", Cout, H, with_bias))
    q_pts, s_pts = _points(KP_M, KP_NS, g)
    f = torch.randn(KP_NS, generator=g)
    f[torch.rand(KP_NS, generator=g) < 0.25] = 0.0
    return {"q_pts": q_pts, "s_pts": s_pts, "idx": neighbour_lists(KP_M, KP_NS, H, g), "feats": f, "kp": torch.from_numpy(kernel_points()),
            "sigma": KP_SIGMA, "order": torch.randperm(KP_M, generator=g).to(torch.int32),
            "weights": torch.randn(15, 1, Cout, generator=g) / 15 ** 0.5, "bias": torch.randn(Cout, generator=g) if with_bias else None}


def cin1_of(c, mutate=None):
    return kpconv_cin1(c["feats"], c["q_pts"], c["s_pts"], c["idx"], c["kp"], c["sigma"], c["weights"], c["bias"], mutate)


@functools.lru_cache(maxsize=None)
def cin1_reference(Cout, H, with_bias, mutate=None):
    return cin1_of(cast(cin1_case(Cout, H, with_bias), torch.float64), mutate)


@functools.lru_cache(maxsize=None)
def pool_case(C, H, mixed=False):
    """All-negative features (a row without a shadow entry must give its negative maximum, one with a shadow entry 0); mixed: N(0,1) features,
    so that every neighbour of a partly filled list can be the maximum of some channel.  Rows 0, 7, ... are all shadow, rows 1, 8, ... hold
    one neighbour, rows 2, 9, ... no shadow entry; the other rows' neighbour counts are random (not multiples of 8)."""
    g = torch.Generator().manual_seed(_seed("pool", C, H, mixed))
    M, Ns = 100, 150
    x = torch.randn(Ns, C, generator=g) if mixed else -torch.rand(Ns, C, generator=g) - 0.01
    return {"x": x, "idx": neighbour_lists(M, Ns, H, g), "order": torch.randperm(M, generator=g).to(torch.int32)}


@functools.lru_cache(maxsize=None)
def pool_reference(C, H, mixed=False, mutate=None):
    c = pool_case(C, H, mixed)
    return maxpool(c["x"].double(), c["idx"], mutate)


# ------------------------------------------------------------------------------------------------ which cases must see which mutation
GN_MUTATION_MODE = {m: (2, True) for m in MUTATIONS["gn_apply"]}        # (residual mode, act) the mutation is judged in
_STACKED = lambda t: sum(n > 0 for n in SEG_TABLES[t]) >= 2
ASSIGNED = {
    # cnt / (cnt - 1) moves rstd by 1 / (2 cnt): seen where a group holds few values — the two-row segment, and the one-row segments with two
    # channels per group (with one channel per group cnt = 1 and the variance is 0 either way)
    "unbiased_variance": lambda C, G, t, sh: (C // G == 1 and t == "two") or (C // G in (2, 4) and t != "two"),
    # eps only matters where a variance is of its size: one-row segments with one channel per group (variance exactly 0: the mutation divides by 0)
    "eps_dropped": lambda C, G, t, sh: C // G == 1 and t != "two",
    "first_row_previous_stats": lambda C, G, t, sh: _STACKED(t),
    "last_row_next_stats": lambda C, G, t, sh: _STACKED(t),
    "wrong_group_size": lambda C, G, t, sh: G > 1 and t != "one",
    "residual_with_x_affine": lambda C, G, t, sh: True,
    "act_before_residual": lambda C, G, t, sh: True,
    "flag_from_x": lambda C, G, t, sh: sh == 0 and t not in ("one", "two"),
    # KPConv: per family of cases — "agg" (C, H): A or the count moves; "fused" (table, shift) and "cin1" (Cout, H, with bias): the output moves.
    # The one- and two-row tables hold only the all-shadow and the one-neighbour row of neighbour_lists; with H = 1 no count exceeds 1.
    "count_unclamped": {"agg": lambda C, H: True, "fused": lambda t, sh: True, "cin1": lambda O, H, b: True},
    "count_from_valid": {"agg": lambda C, H: H > 1, "fused": lambda t, sh: t not in ("one", "two"), "cin1": lambda O, H, b: H > 1},
    "shadow_contributes": {"agg": lambda C, H: True, "fused": lambda t, sh: t not in ("one", "two"), "cin1": lambda O, H, b: True},
    "influence_unclamped": {"agg": lambda C, H: True, "fused": lambda t, sh: t != "one", "cin1": lambda O, H, b: True},
    "w_blocks_permuted": {"agg": lambda C, H: False, "fused": lambda t, sh: t not in ("one", "two"), "cin1": lambda O, H, b: True},
    "bias_before_division": {"agg": lambda C, H: False, "fused": lambda t, sh: t not in ("one", "two"), "cin1": lambda O, H, b: b and H > 1},
    # max-pool (C, H, mixed): with all-negative features a row with a shadow entry gives 0 whatever is dropped, so a dropped neighbour shows in
    # the rows without one, whose count is H: H = 1, 7, 9.  With mixed signs it shows in every partly filled row: every H but 1.
    "ignore_shadow": lambda C, H, mixed: True,
    "drop_last_ragged": lambda C, H, mixed: H > 1 if mixed else H % 8 != 0,
}
