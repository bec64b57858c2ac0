"""The definitions of the registration loss terms (include/lcr_hip.h: lcr_gap_loss, lcr_min_dist) restated in torch, and the seeded
inputs the loss tests share.  Labels and nearest rows are decided in fp32 exactly as the header states (every operation rounded);
everything after them runs in fp64 on the fp32 inputs, and torch.autograd gives the gradients.  The drop test is done on the
fp32-rounded line mean.  `mistake=` plants one of the errors tests/test_losses_gpu.py must be able to see."""
import functools
import os

import numpy as np
import torch

F32 = torch.float32
MISTAKES = ("mask_negatives", "keep_dropped", "swap_dustbin", "ge_at_4r2", "mean_over_m")


# ---- labels -------------------------------------------------------------------------------------------------------------------------------
def moved(q, T):
    """q' = ((R0*x + R1*y) + R2*z) + t per component, fp32."""
    q, T = q.to(F32), T.to(F32)
    x, y, z = q[..., 0], q[..., 1], q[..., 2]
    return torch.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], -1)


def d2_by_differences(p, q):
    """(..., N, 3) x (..., M, 3) -> (..., N, M): ((dx*dx + dy*dy) + dz*dz) in fp32."""
    d = p.to(F32)[..., :, None, :] - q.to(F32)[..., None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def point_labels(p_pts, q_pts, pmask, qmask, T, radius, mistake=None):
    """-> (positive, negative) bool (B, N, M) and d2 fp32."""
    d2 = d2_by_differences(p_pts, moved(q_pts, T))
    r2 = torch.tensor(radius * radius, dtype=F32)
    r2n = torch.tensor((radius * 2) * (radius * 2), dtype=F32)
    both = pmask.bool()[:, :, None] & qmask.bool()[:, None, :]
    pos = (d2 < r2) & both
    neg = (d2 >= r2n) if mistake == "ge_at_4r2" else (d2 > r2n)
    if mistake == "mask_negatives":
        neg = neg & both
    return pos, neg, d2


def overlap_labels(n, m, corr, overlaps, pmask, qmask, thr, mistake=None):
    ov = torch.zeros(n, m, dtype=F32)
    ov[corr[:, 0].long(), corr[:, 1].long()] = overlaps.to(F32)
    both = pmask.bool()[:, None] & qmask.bool()[None, :]
    pos = (ov > torch.tensor(thr, dtype=F32)) & both
    neg = ov == 0
    if mistake == "mask_negatives":
        neg = neg & both
    return pos[None], neg[None], ov[None]


# ---- the gap core -------------------------------------------------------------------------------------------------------------------------
def _direction(S, pos, neg, gamma, mistake):
    """Lines = rows of S (B, n, m+1) with the dustbin in the last column; pos / neg (B, n, m) inner labels.  fp64."""
    inner = pos.sum(2)
    dust_pos = inner != 0 if mistake == "swap_dustbin" else inner == 0
    posf = torch.cat([pos, dust_pos[..., None]], 2)
    negf = torch.cat([neg, ~dust_pos[..., None]], 2)
    if mistake == "mean_over_m":                                   # the dustbin left out of the candidates
        posf = torch.cat([pos, torch.zeros_like(dust_pos)[..., None]], 2)
        negf = torch.cat([neg, torch.zeros_like(dust_pos)[..., None]], 2)
    cnt = posf.sum(2)
    line_pos = (-S * posf).sum(2) / cnt
    keep = line_pos.detach().to(F32) != torch.tensor(1e12, dtype=F32)
    if mistake == "keep_dropped":
        keep = torch.ones_like(keep)
    arg = line_pos[..., None] + S + gamma
    hinge = torch.clamp(arg, min=0) * negf
    s = hinge.sum(2)
    term = torch.log(s[keep] + 1).mean()
    return {"term": term, "keep": keep, "count": cnt, "active": (negf & (arg >= 0)).sum(2), "hinge": s, "pos": line_pos, "arg": arg,
            "posf": posf, "negf": negf}


def gap_core(scores, pos, neg, gamma, mistake=None):
    """One pair: scores (B, n+1, m+1) fp32 (a leaf with requires_grad for gradients), inner labels (B, n, m) -> dict with the row term,
    the column term, their mean (0-dim fp64 tensors), the kept counts and the per-line statistics of both directions."""
    S = scores.double()
    row = _direction(S[:, :-1, :], pos, neg, gamma, mistake)
    col = _direction(S[:, :, :-1].transpose(1, 2), pos.transpose(1, 2), neg.transpose(1, 2), gamma, mistake)
    B, n1, m1 = scores.shape
    plane = torch.zeros(B, n1, m1, dtype=torch.uint8)
    plane[:, :-1, :] = row["posf"].to(torch.uint8) + 2 * row["negf"].to(torch.uint8)
    plane[:, -1, :-1] = (col["posf"][:, :, -1].to(torch.uint8) + 2 * col["negf"][:, :, -1].to(torch.uint8))
    return {"row": row, "col": col, "row_term": row["term"], "col_term": col["term"], "mean": (row["term"] + col["term"]) / 2,
            "kept": (int(row["keep"].sum()), int(col["keep"].sum())), "labels": plane}


def constant_entries(core):
    """bool (B, n+1, m+1): the scores the loss does not depend on — entries that are neither positive nor negative in any kept line
    through them, and the corner."""
    r, c = core["row"], core["col"]
    use_r = (r["posf"] | r["negf"]) & r["keep"][..., None]
    use_c = ((c["posf"] | c["negf"]) & c["keep"][..., None]).transpose(1, 2)
    B, n, m1 = use_r.shape
    used = torch.zeros(B, n + 1, m1, dtype=torch.bool)
    used[:, :-1, :] |= use_r
    used[:, :, :-1] |= use_c
    return ~used


# ---- nearest distance -----------------------------------------------------------------------------------------------------------------------
def nearest_rows(A, D):
    """arg-min of the fp32 d2 by differences, the lower row on a tie; and the sorted two smallest d2 per query (for the margins)."""
    d2 = d2_by_differences(A, D).numpy()
    arg = d2.argmin(1)                                             # numpy: the first occurrence
    part = np.sort(d2, 1)[:, :2]
    return torch.from_numpy(arg), d2, part


def min_dist(A, D, valid=None):
    """One segment: A (na, 3), D (nd, 3) fp32 (leaves for gradients) -> dist fp64 (na), arg, mean over the valid queries (NaN without one)."""
    arg, _, _ = nearest_rows(A.detach(), D.detach())
    d = A.double() - D.double()[arg]
    dist = torch.sqrt(torch.clamp((d * d).sum(1), min=1e-12))
    v = torch.ones(A.shape[0], dtype=torch.bool) if valid is None else valid.bool()
    return dist, arg, dist[v].mean()


# ---- margins --------------------------------------------------------------------------------------------------------------------------------
def assert_margins(d2=None, radius=None, overlaps=None, thr=None, cores=(), nearest=None, margin=1e-9, tie_at_4r2=False, tie_rows=()):
    """Every threshold decision of a test input is at least `margin` away from a tie: d2 against r^2 and (2r)^2, overlap against
    positive_overlap, hinge arguments against 0, nearest against second-nearest distance.  tie_at_4r2 / tie_rows exempt the ties a test
    plants on purpose."""
    if d2 is not None:
        d = d2.double()
        assert ((d - float(np.float32(radius * radius))).abs() >= margin).all(), "d2 within the margin of r^2"
        at = (d - float(np.float32((2 * radius) * (2 * radius)))).abs() < margin
        assert tie_at_4r2 or not at.any(), "d2 within the margin of (2r)^2"
    if overlaps is not None:
        assert ((overlaps.double() - float(np.float32(thr))).abs() >= margin).all(), "overlap within the margin of positive_overlap"
    for core in cores:
        for side in ("row", "col"):
            s = core[side]
            a = s["arg"].detach()[s["negf"] & s["keep"][..., None]]
            assert (a.abs() >= margin).all(), "a hinge argument within the margin of 0"
    if nearest is not None:
        part = np.sqrt(nearest.astype(np.float64))
        gap_ = part[:, 1] - part[:, 0] if part.shape[1] > 1 else np.full(len(part), np.inf)
        ok = gap_ >= margin
        ok[list(tie_rows)] = True
        assert ok.all(), "nearest and second-nearest distance within the margin"


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------------
RADIUS, GAMMA, THR = 0.45, 0.5, 0.1
GAP_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 64, 64), (2, 65, 63), (4, 128, 128)]      # (B, N, M), point labels
NODE_SHAPE = (1, 200, 131)                                                       # overlap labels
MD_SIZES = [(q, d) for q in (1, 37, 300) for d in (1, 1000, 5000)]


def _rigid(rng, shift=60.0):
    a = rng.uniform(0, 2 * np.pi)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = rng.uniform(-shift, shift, 3) * [1, 1, 0.05]
    return T.astype(np.float32)


def _scores(rng, B, N, M, pmask, qmask):
    S = (rng.normal(size=(B, N + 1, M + 1)) * 3 - 8).astype(np.float32)
    for b in range(B):
        S[b, :N][~pmask[b]] = -1e12
        S[b, :, :M][:, ~qmask[b]] = -1e12
    return S


def gap_case(shape, seed=0):
    """(B, N, M) -> dict of numpy inputs with point labels: patches around a centre ~60 m out, the anc side given in its own frame;
    padded rows and columns (zero points, -1e12 scores); slice 1 (if any) without any positive; the LAST slice, when B > 2, fully padded
    on the pos side and a pair of its own (its row term is NaN); row 0 of slice 0 (N > 1) with the dustbin as its only positive.
    Pairs: seg_start.  Points are redrawn until every d2 is 1e-3 away from r^2 and (2r)^2."""
    B, N, M = shape
    rng = np.random.default_rng(1000 * seed + 100 * B + 10 * N + M)
    T = np.stack([_rigid(rng) for _ in range(2)])
    seg = [0, B] if B <= 2 else [0, B - 1, B]
    pair_of = np.searchsorted(seg, np.arange(B), side="right") - 1
    P_pts, Q_pts = np.zeros((B, N, 3), np.float32), np.zeros((B, M, 3), np.float32)
    pmask, qmask = np.ones((B, N), bool), np.ones((B, M), bool)
    for b in range(B):
        c = rng.uniform(-60, 60, 3) * [1, 1, 0.05]
        if N > 4:
            pmask[b, N - max(1, N // 8):] = False
        if M > 4:
            qmask[b, M - max(1, M // 10):] = False
        if B > 2 and b == B - 1:
            pmask[b] = False
        Tb = T[pair_of[b]].astype(np.float64)
        P_pts[b] = (c + rng.uniform(-1.5, 1.5, (N, 3))).astype(np.float32)
        if N > 1 and b == 0:
            P_pts[b, 0] += np.float32(25.0)                          # far from every anc point: only the dustbin is positive
        redo = np.ones(M, bool)
        for _ in range(200):
            src = P_pts[b][rng.integers(0, N, M)] + rng.normal(scale=0.4, size=(M, 3))
            if b == 1:
                src = src + 40.0                                     # a slice without any positive
            if N == 1 and M == 1:
                src = P_pts[b] + 0.1                                 # the smallest case: its one point pair is a positive
            Q_pts[b][redo] = ((src - Tb[:3, 3]) @ Tb[:3, :3]).astype(np.float32)[redo]
            Pz, Qz = P_pts[b] * pmask[b][:, None], Q_pts[b] * qmask[b][:, None]
            d2 = d2_by_differences(torch.from_numpy(Pz), moved(torch.from_numpy(Qz), torch.from_numpy(T[pair_of[b]]))).numpy()
            bad = (np.abs(d2 - RADIUS ** 2) < 1e-3) | (np.abs(d2 - 4 * RADIUS ** 2) < 1e-3)
            redo = bad.any(0) & qmask[b]
            if not bad.any():
                break
        else:
            raise RuntimeError("no margin found")
        P_pts[b], Q_pts[b] = Pz, Qz
    S = _scores(rng, B, N, M, pmask, qmask)
    if N == 1 and M == 1:
        S[0] = [[-9.0, -7.0], [-6.5, -8.0]]                          # both dustbin hinges active
    return {"scores": S, "p_pts": P_pts, "q_pts": Q_pts, "pmask": pmask, "qmask": qmask, "transforms": T[:len(seg) - 1], "seg": seg}


def node_case(shape=NODE_SHAPE, seed=0):
    _, N, M = shape
    rng = np.random.default_rng(7000 + seed)
    pmask, qmask = np.ones((1, N), bool), np.ones((1, M), bool)
    pmask[0, N - 9:] = False
    qmask[0, M - 5:] = False
    C = 3 * max(N, M)
    flat = rng.choice(N * M, size=C, replace=False)
    corr = np.stack([flat // M, flat % M], 1).astype(np.int64)
    corr = corr[corr[:, 0] != 3]                                     # node 3 has no correspondence: its dustbin is its only positive
    ov = rng.uniform(0.005, 1.0, len(corr)).astype(np.float32)
    ov[np.abs(ov - np.float32(THR)) < 1e-3] = 0.5
    return {"scores": _scores(rng, 1, N, M, pmask, qmask), "corr": corr, "overlaps": ov, "pmask": pmask, "qmask": qmask, "seg": [0, 1]}


def min_dist_case(nq, nd, seed=0):
    """Queries next to a data cloud ~60 m out.  With nd > 1 data rows 0 and 1 are the same point and query 0 sits next to it: an exact
    tie (tie_rows = [0]), to be resolved to row 0."""
    rng = np.random.default_rng(9000 + 100 * seed + nq + nd)
    c = np.array([60.0, -58.0, 3.0])
    D = (c + rng.uniform(-8, 8, (nd, 3))).astype(np.float32)
    A = (D[rng.integers(2 if nd > 2 else 0, nd, nq)] + rng.normal(scale=0.3, size=(nq, 3))).astype(np.float32)
    ties = []
    if nd > 1:
        D[1] = D[0]
        A[0] = D[0] + np.float32(0.01)
        ties = [0]
    valid = rng.uniform(size=nq) < 0.7
    valid[0] = True
    return {"A": A, "D": D, "valid": valid, "tie_rows": ties}


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def digest(case):
    """64 bits of a hash over a case's arrays: the golden file keeps one per input, so a generator that drifts is noticed."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(case):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return np.frombuffer(h.digest()[:8], dtype=np.uint64)[0]


# ---- the whole loss on one pair ---------------------------------------------------------------------------------------------------------------
WEIGHTS = {"weight_coarse_loss": 1.0, "weight_vote_loss": 0.25}
CORRES_RADIUS = 2.4


def overall_case(seed=0, n_pos=23, n_anc=19, B=6, N=12, M=10):
    """One pair's output dict (numpy) as LCRNet_Matching returns it, small: patches from gap_case-like geometry, a node score matrix with
    overlap labels, shifted nodes near the fine points of both clouds, overlap scores, rotary angles partly beyond pi."""
    rng = np.random.default_rng(4000 + seed)
    g = gap_case((B if B > 2 else 2, N, M), seed=seed + 1)
    keep = slice(0, g["seg"][1])                                     # the first pair of that case: no fully padded slice
    nd = node_case((1, n_pos, n_anc), seed=seed + 1)
    T = g["transforms"][0]
    pos_f = (np.array([55.0, -40.0, 1.0]) + rng.uniform(-10, 10, (400, 3)) * [1, 1, 0.1]).astype(np.float32)
    anc_world = (np.array([55.0, -40.0, 1.0]) + rng.uniform(-10, 10, (350, 3)) * [1, 1, 0.1])
    T64 = T.astype(np.float64)
    to_anc = lambda x: ((x - T64[:3, 3]) @ T64[:3, :3]).astype(np.float32)
    ori_pos = pos_f[rng.choice(400, n_pos, replace=False)]
    ori_anc_w = np.concatenate([ori_pos[:n_anc // 2] + rng.normal(scale=0.3, size=(n_anc // 2, 3)),
                                anc_world[rng.choice(350, n_anc - n_anc // 2, replace=False)]])
    sh_pos = (ori_pos + rng.normal(scale=0.8, size=ori_pos.shape)).astype(np.float32)
    sh_anc = to_anc(ori_anc_w + rng.normal(scale=0.8, size=ori_anc_w.shape))
    emb = lambda n: (rng.normal(size=(1, n, 8)) * 2.5).astype(np.float32)
    return {"matching_scores": g["scores"][keep], "pos_node_corr_knn_points": g["p_pts"][keep], "anc_node_corr_knn_points": g["q_pts"][keep],
            "pos_node_corr_knn_masks": g["pmask"][keep], "anc_node_corr_knn_masks": g["qmask"][keep], "transform": T,
            "node_matching_scores": nd["scores"][0], "gt_node_corr_indices": nd["corr"], "gt_node_corr_overlaps": nd["overlaps"],
            "pos_node_masks": nd["pmask"][0], "anc_node_masks": nd["qmask"][0],
            "shifted_pos_points_c": sh_pos, "shifted_anc_points_c": sh_anc, "pos_points_f": pos_f, "anc_points_f": to_anc(anc_world),
            "ori_pos_points_c": ori_pos, "ori_anc_points_c": to_anc(ori_anc_w), "pos_points_c": ori_pos, "anc_points_c": to_anc(ori_anc_w),
            "score": rng.uniform(0.02, 0.98, n_pos + n_anc).astype(np.float32), "pos_emb": emb(n_pos), "anc_emb": emb(n_anc)}


GRAD_KEYS = ("matching_scores", "node_matching_scores", "shifted_pos_points_c", "shifted_anc_points_c")


def as_tensors(case, device="cpu", grad=True):
    o = {k: t(v).to(device) for k, v in case.items()}
    if grad:
        for k in GRAD_KEYS:
            o[k].requires_grad_()
    return o


def vote_valid(o, corres_radius=CORRES_RADIUS):
    """mask.any(1), mask.any(0) of the reference's distance mask: a node is valid iff its nearest node of the other cloud is closer,
    in SQUARED distance, than corres_radius itself (matching.py:491-505 compares the squared distance with the radius)."""
    pos = o["ori_pos_points_c"].detach()
    anc = moved(o["ori_anc_points_c"].detach(), o["transform"])
    d2 = d2_by_differences(pos, anc).clamp(min=1e-12)
    return d2.min(1)[0] < corres_radius, d2.min(0)[0] < corres_radius


def overall(o, mask=None, mistake=None):
    """The seven entries of OverallLoss_new on tensors `o` (fp32 leaves), fp64 after the labels.  mask = (valid pos, valid anc)."""
    T = o["transform"]
    pos, neg, _ = point_labels(o["pos_node_corr_knn_points"], o["anc_node_corr_knn_points"], o["pos_node_corr_knn_masks"],
                               o["anc_node_corr_knn_masks"], T, RADIUS, mistake)
    g = gap_core(o["matching_scores"], pos, neg, GAMMA, mistake)["mean"]
    ns = o["node_matching_scores"]
    npos, nneg, _ = overlap_labels(ns.shape[0] - 1, ns.shape[1] - 1, o["gt_node_corr_indices"], o["gt_node_corr_overlaps"],
                                   o["pos_node_masks"], o["anc_node_masks"], THR, mistake)
    c = gap_core(ns[None], npos, nneg, GAMMA, mistake)["mean"]
    vp, va = vote_valid(o) if mask is None else mask
    sp, sa = o["shifted_pos_points_c"], o["shifted_anc_points_c"]
    T64 = T.double()
    sa_w = sa.double() @ T64[:3, :3].t() + T64[:3, 3]
    sa_w32 = moved(sa.detach(), T)                                   # the rows are chosen in fp32, on the points the kernel sees
    arg_f = torch.from_numpy(d2_by_differences(sp.detach(), sa_w32).numpy().argmin(1))
    arg_b = torch.from_numpy(d2_by_differences(sa_w32, sp.detach()).numpy().argmin(1))
    dist = lambda a, d, idx: torch.sqrt(torch.clamp(((a - d[idx]) ** 2).sum(1), min=1e-12))
    v = dist(sp.double(), sa_w, arg_f)[vp.bool()].mean() + dist(sa_w, sp.double(), arg_b)[va.bool()].mean()
    d = (min_dist(sp, o["pos_points_f"])[2] + min_dist(sa, o["anc_points_f"])[2]) / 2
    gt = torch.zeros(o["pos_points_c"].shape[0] + o["anc_points_c"].shape[0], dtype=torch.float64)
    gt[o["gt_node_corr_indices"][:, 0].long()] = 1.0
    gt[o["pos_points_c"].shape[0] + o["gt_node_corr_indices"][:, 1].long()] = 1.0
    w_neg = gt.sum() / gt.shape[0]
    w = torch.where(gt >= 0.5, 1 - w_neg, w_neg)
    n = (w * torch.nn.functional.binary_cross_entropy(o["score"].double(), gt, reduction="none")).mean()
    beyond = lambda e: torch.clamp(e.double().abs() - 3.1415926, min=0).mean()
    reg = (beyond(o["pos_emb"]) + beyond(o["anc_emb"])) / 2
    wv = WEIGHTS["weight_vote_loss"]
    out = {"c_loss": WEIGHTS["weight_coarse_loss"] * c, "g_loss": 5 * g, "reg_loss": reg, "v_loss": v * wv, "d_loss": d * wv, "n_loss": n}
    out["loss"] = out["c_loss"] + out["g_loss"] + reg + (v + d) * wv + n
    return out


# ---- what the tests share: the restated results of every seeded case, computed once ---------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses_golden.npz")


def bound(e_ref, want):
    """The tolerance rule: 4 x the error of the reference's own fp32 module against this restatement, with a floor of 2^-20 relative to the
    largest magnitude in the tensor."""
    w = np.asarray(want, dtype=np.float64)
    big = np.abs(w[np.isfinite(w)]).max() if np.isfinite(w).any() else 0.0
    return max(4.0 * float(e_ref), 2.0 ** -20 * big)


def err(got, want):
    """max |got - want| over the finite entries of want; NaN must sit where NaN is wanted."""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    assert np.array_equal(np.isnan(g), np.isnan(w)), "NaN pattern differs"
    f = ~np.isnan(w)
    return float(np.abs(g[f] - w[f]).max()) if f.any() else 0.0


def _gap_results(c, labels_of, mistake=None, check=True):
    """Per pair of a case: the restated terms, kept counts, label planes and line statistics, and the gradient of sum over pairs of
    (0.5 * row term + 0.5 * column term) with NaN terms left out — the gradient the reference's loss.backward() gives for the pairs
    whose loss is finite."""
    S = t(c["scores"]).clone().requires_grad_()
    seg, pairs, total = c["seg"], [], 0.0
    for p in range(len(seg) - 1):
        sl = slice(seg[p], seg[p + 1])
        pos, neg, dec = labels_of(p, sl, mistake)
        core = gap_core(S[sl], pos, neg, GAMMA, mistake)
        if check and mistake is None:
            core["decision"] = dec
        for k in ("row_term", "col_term"):
            if not torch.isnan(core[k]):
                total = total + 0.5 * core[k]
        pairs.append(core)
    if torch.is_tensor(total) and total.requires_grad:
        total.backward()
    grad = S.grad.numpy() if S.grad is not None else np.zeros(c["scores"].shape)
    return {"pairs": pairs, "grad": grad, "terms": np.array([[float(q[k].detach()) for k in ("row_term", "col_term", "mean")] for q in pairs]),
            "kept": np.array([q["kept"] for q in pairs])}


def gap_results(ci, mistake=None, case=None):
    c = gap_case(GAP_SHAPES[ci]) if case is None else case
    lab = lambda p, sl, mk: point_labels(t(c["p_pts"][sl]), t(c["q_pts"][sl]), t(c["pmask"][sl]), t(c["qmask"][sl]), t(c["transforms"][p]),
                                         RADIUS, mk)
    return c, _gap_results(c, lab, mistake)


def node_results(mistake=None):
    c = node_case()
    _, N, M = NODE_SHAPE
    lab = lambda p, sl, mk: overlap_labels(N, M, t(c["corr"]), t(c["overlaps"]), t(c["pmask"][0]), t(c["qmask"][0]), THR, mk)
    return c, _gap_results(c, lab, mistake)


def tie_case():
    """(1, 3, 3) with one point pair at d2 == (float)((2r)^2) exactly and scores that make that entry's hinge active: `>` and `>=`
    at (2r)^2 differ on it."""
    c = gap_case((1, 3, 3), seed=3)
    c["transforms"] = np.eye(4, dtype=np.float32)[None]
    c["pmask"][:], c["qmask"][:] = True, True
    r2n = np.float32((2 * RADIUS) * (2 * RADIUS))
    dx = np.float32(0.8999)
    for k in range(-64, 65):                                         # d = 0 - q is exact, so d2 = fl(fl(dx*dx) + fl(dy*dy))
        dy = np.float32(np.sqrt(np.float64(r2n) - np.float64(dx) ** 2)) + np.float32(k) * np.float32(1e-9)
        if np.float32(np.float32(dx * dx) + np.float32(dy * dy)) == r2n:
            break
    else:
        raise RuntimeError("no fp32 point gives d2 == (2r)^2 exactly")
    c["p_pts"][0] = [[0, 0, 0], [30, 0, 0], [0, 40, 0]]
    c["q_pts"][0] = [[0, 0, 0.1], [dx, dy, 0], [30.1, 0, 0]]         # (0, 0) and (1, 2) positive; (0, 1) sits at (2r)^2 exactly
    c["scores"][:] = np.float32(-1.0)
    return c


def masked_case():
    """(2, 6, 6) whose masked rows and columns carry ordinary finite scores: the only input on which masking the negatives by validity
    changes the value (under -1e12 scores a masked negative's hinge is zero either way)."""
    c = gap_case((2, 6, 6), seed=5)
    c["scores"] = (np.random.default_rng(77).normal(size=c["scores"].shape) * 3 - 8).astype(np.float32)
    return c


@functools.lru_cache(maxsize=None)
def cached(kind, key=None):
    if kind == "gap" and key == "masked":
        return gap_results(None, case=masked_case())
    if kind == "gap":
        return gap_results(key)
    if kind == "node":
        return node_results()
    if kind == "md":
        c = min_dist_case(*key)
        A = t(c["A"]).clone().requires_grad_()
        dist, arg, mean = min_dist(A, t(c["D"]), t(c["valid"]))
        mean.backward()
        return c, {"dist": dist.detach().numpy(), "arg": arg.numpy(), "mean": float(mean.detach()), "grad": A.grad.numpy()}
    if kind == "overall":
        c = overall_case()
        o = as_tensors(c)
        res = overall(o)
        res["loss"].backward()
        return c, {"losses": {k: float(v.detach()) for k, v in res.items()}, "grads": {k: o[k].grad.numpy() for k in GRAD_KEYS},
                   "valid": [v.numpy() for v in vote_valid(o)]}
    raise KeyError(kind)
