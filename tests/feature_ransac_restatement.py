"""NumPy restatement of feature-matching RANSAC as include/lcr_hip.h states it (lcr_feature_nn, lcr_feature_correspondences,
lcr_ransac_correspondences_ex): the exact float32 nearest neighbour in feature space, the correspondence list with the mutual filter and
its fall-back, the two correspondence checkers, and the checked RANSAC, which reuses the sampler, Kabsch, score and selection of
tests/ransac_restatement.py and only masks the rejected hypotheses.  Plus planted pairs with features."""
import numpy as np

import ransac_restatement as rr

REJECT_VALID, REJECT_DEGENERATE, REJECT_EDGE, REJECT_DISTANCE = 0, 1, 2, 3

# the planted pairs of the CPU and GPU tests (vetted in tests/test_feature_ransac_cpu.py) and the RANSAC settings they run with
PLANTED = (dict(n=2000, overlap=0.35, feat_noise=0.15, seed=11, ransac_n=3), dict(n=1500, overlap=0.4, feat_noise=0.15, seed=12, ransac_n=4))
PLANTED_THR, PLANTED_ITERS, PLANTED_SEED = 0.3, 4000, 3


def feature_nn(qf, df, chunk=256):
    """(nn int32 [nq], d2 float32 [nq]) of one pair by the exact chain: float32 arrays, one channel per step (acc = acc + t * t with
    t = q[c] - d[c], every operation rounded to float32), the minimum of (d2, row) with NaN distances never winning; -1 / NaN where the
    database is empty or every distance is NaN.  Chunked over query rows."""
    qf = np.ascontiguousarray(qf, dtype=np.float32)
    df = np.ascontiguousarray(df, dtype=np.float32)
    nq, C = qf.shape
    nd = df.shape[0]
    nn = np.full(nq, -1, np.int32)
    d2 = np.full(nq, np.nan, np.float32)
    if nd == 0:
        return nn, d2
    dT = np.ascontiguousarray(df.T)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, nq, chunk):
            b = min(nq, a + chunk)
            acc = np.zeros((b - a, nd), np.float32)
            for c in range(C):
                t = qf[a:b, c:c + 1] - dT[c][None, :]
                acc = acc + t * t
            assert acc.dtype == np.float32
            valid = ~np.isnan(acc)
            m = np.where(valid, acc, np.float32(np.inf)).min(axis=1)
            hit = valid & (acc == m[:, None])
            has = hit.any(axis=1)
            j = hit.argmax(axis=1)                          # the first (smallest) row that attains the minimum
            nn[a:b] = np.where(has, j, -1)
            d2[a:b] = np.where(has, m, np.float32(np.nan))
    return nn, d2


def feature_nn_f64(qf, df):
    """float64 brute force: (argmin, minimum, runner-up distance) per query row."""
    q, d = np.asarray(qf, np.float64), np.asarray(df, np.float64)
    D = ((q[:, None, :] - d[None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(D, axis=1, kind="stable")
    best = order[:, 0]
    m = D[np.arange(len(q)), best]
    second = D[np.arange(len(q)), order[:, 1]] if d.shape[0] > 1 else np.full(len(q), np.inf)
    return best, m, second


def correspondences(nn_sr, nn_rs=None, n_ref=None, min_rows=3):
    """One pair: (rows int32 [K,2] (i, nn_sr[i]) in ascending i, mutual_used).  Row i is kept iff 0 <= nn_sr[i] < n_ref and (no mutual
    filter or nn_rs[nn_sr[i]] == i); a mutual set of fewer than min_rows rows falls back to the unfiltered one."""
    nn_sr = np.asarray(nn_sr, np.int64)
    n_ref = (len(nn_rs) if nn_rs is not None else (int(nn_sr.max()) + 1 if len(nn_sr) else 0)) if n_ref is None else n_ref
    i = np.arange(len(nn_sr))
    any_ = (nn_sr >= 0) & (nn_sr < n_ref)
    keep, used = any_, False
    if nn_rs is not None:
        nn_rs = np.asarray(nn_rs, np.int64)
        mut = any_.copy()
        mut[any_] = nn_rs[nn_sr[any_]] == i[any_]
        if int(mut.sum()) >= min_rows:
            keep, used = mut, True
    return np.stack([i[keep], nn_sr[keep]], axis=1).astype(np.int32).reshape(-1, 2), used


def edge_check(ps, pr, edge_similarity):
    """ps, pr [H,k,3] float32 sampled rows -> bool [H]: for every two draws a < b, ls2 = |s_a - s_b|^2 and lr2 = |r_a - r_b|^2 in the
    float32 form (dx*dx + dy*dy) + dz*dz, k2 = edge_similarity * edge_similarity (float32); pass iff ls2 >= k2 * lr2 and lr2 >= k2 * ls2."""
    ps, pr = np.asarray(ps, np.float32), np.asarray(pr, np.float32)
    ok = np.ones(ps.shape[0], bool)
    if not edge_similarity > 0:
        return ok
    k2 = np.float32(edge_similarity) * np.float32(edge_similarity)
    k = ps.shape[1]

    def len2(p, a, b):
        d = p[:, a] - p[:, b]
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    for a in range(k):
        for b in range(a + 1, k):
            ls2, lr2 = len2(ps, a, b), len2(pr, a, b)
            assert ls2.dtype == np.float32
            ok &= (ls2 >= k2 * lr2) & (lr2 >= k2 * ls2)
    return ok


def _fma32(a, b, c):
    """fma in float32 for float32 inputs: the product is exact in float64; the sum is rounded to float64 and then to float32 (a double
    rounding that differs from a true fma only on float64 half-way cases)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def distance_check(ps, pr, R, t, checker_distance):
    """ps, pr [H,k,3] float32 sampled rows, R [H,3,3] / t [H,3] (fp64, stored as float32 here as on the device) -> (bool [H], fp64
    distances [H,k] of the sampled rows under the fp64 transform).  The scoring rule's float32 fma form: d2 < checker_distance^2."""
    ps, pr = np.asarray(ps, np.float32), np.asarray(pr, np.float32)
    dist = np.linalg.norm(np.einsum("hrc,hkc->hkr", R, ps.astype(np.float64)) + t[:, None, :] - pr, axis=2)
    if not checker_distance > 0:
        return np.ones(len(R), bool), dist
    m = np.concatenate([R, t[:, :, None]], axis=2).astype(np.float32)               # [H,3,4]
    d = []
    for r in range(3):
        v = _fma32(m[:, r, 0:1], ps[:, :, 0], m[:, r, 3:4] + np.zeros_like(ps[:, :, 0]))
        v = _fma32(m[:, r, 1:2], ps[:, :, 1], v)
        v = _fma32(m[:, r, 2:3], ps[:, :, 2], v)
        d.append(v - pr[:, :, r])
    d2 = _fma32(d[2], d[2], _fma32(d[1], d[1], d[0] * d[0]))
    c2 = np.float32(checker_distance) * np.float32(checker_distance)
    return (d2 < c2).all(axis=1), dist


def ransac_checked(src, ref, thr, ransac_n, iterations, seed=0, edge_similarity=0.9, checker_distance=None):
    """One pair of correspondence rows -> the dict of ransac_restatement.ransac plus reject [H] (0 valid, 1 degenerate, 2 edge,
    3 distance; the first check that fires in the order edge, degenerate, distance) and sample_dist [H,k] (fp64 distances of the sampled
    rows under the hypothesis).  checker_distance None: thr; <= 0 switches a check off."""
    checker_distance = thr if checker_distance is None else checker_distance
    src32, ref32 = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(ref, np.float32).reshape(-1, 3)
    H = iterations
    idx, R, t, valid = rr.hypotheses(src32, ref32, seed, ransac_n, iterations)
    reject = np.full(H, REJECT_DEGENERATE, np.int64)
    sample_dist = np.zeros((H, ransac_n))
    if len(src32) >= ransac_n:
        ps, pr = src32[idx], ref32[idx]
        e_ok = edge_check(ps, pr, edge_similarity)
        d_ok, sample_dist = distance_check(ps, pr, R, t, checker_distance)
        reject = np.where(~e_ok, REJECT_EDGE, np.where(~valid, REJECT_DEGENERATE, np.where(~d_ok, REJECT_DISTANCE, REJECT_VALID)))
    ok = reject == REJECT_VALID
    R, t = R.copy(), t.copy()
    R[~ok] = np.eye(3)
    t[~ok] = 0.0
    counts, sse = rr.score(src32, ref32, R, t, thr) if len(src32) else (np.zeros(H, np.int64), np.zeros(H))
    counts = np.where(ok, counts, -1)
    sse = np.where(ok, sse, 0.0)
    best = rr.select(counts, sse, ok)
    T = np.eye(4)
    inl, rmse = 0, 0.0
    if best >= 0:
        T[:3, :3], T[:3, 3] = R[best], t[best]
        inl, rmse = int(counts[best]), float(np.sqrt(sse[best] / counts[best]))
    return dict(T=T, inliers=inl, rmse=rmse, best_h=best, idx=idx, R=R, t=t, valid=ok, counts=counts, sse=sse, reject=reject,
                sample_dist=sample_dist)


def feature_ransac(src_points, ref_points, src_feats, ref_feats, thr, ransac_n, iterations, seed=0, mutual_filter=False, edge_similarity=0.9):
    """One pair end to end: nearest neighbours, correspondences, checked RANSAC; the dict of ransac_checked plus corr [K,2] and nn_sr."""
    nn_sr, _ = feature_nn(src_feats, ref_feats)
    nn_rs = feature_nn(ref_feats, src_feats)[0] if mutual_filter else None
    corr, used = correspondences(nn_sr, nn_rs, n_ref=len(ref_points), min_rows=ransac_n)
    out = ransac_checked(np.asarray(src_points, np.float32)[corr[:, 0]], np.asarray(ref_points, np.float32)[corr[:, 1]], thr, ransac_n,
                         iterations, seed, edge_similarity)
    out.update(corr=corr, nn_sr=nn_sr, mutual_used=used)
    return out


def planted_feature_pair(n, overlap, feat_noise, seed, C=32, extent=40.0, jitter=0.02):
    """A reference cloud of n points, a source cloud of n points of which round(overlap * n) are moved, jittered copies of reference points
    (the rest lie elsewhere in the scene), and C-dimensional unit features: physically matching points share a random unit vector up to
    Gaussian noise of feat_noise per channel (re-normalised), all other points have unrelated ones.  The source rows are shuffled.
    -> (src_points, ref_points, src_feats, ref_feats (float32), T (4,4) fp64 mapping src onto ref, match int64 [n]: the reference row of
    every source row or -1)."""
    rng = np.random.default_rng(seed)
    m = int(round(overlap * n))
    ref = rng.uniform(-extent, extent, size=(n, 3))
    ref[:, 2] *= 0.1
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.2, 1.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    t = rng.uniform(-5, 5, size=3)
    shared = rng.permutation(n)[:m]
    own = rng.uniform(-extent, extent, size=(n - m, 3))
    own[:, 2] *= 0.1
    src_in_ref = np.concatenate([ref[shared] + rng.normal(scale=jitter, size=(m, 3)), own])
    src = (src_in_ref - t) @ R                                  # R^T (x - t): T maps src back onto ref
    match = np.concatenate([shared, np.full(n - m, -1)])

    def unit(x):
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    base_ref = unit(rng.normal(size=(n, C)))
    base_src = np.concatenate([base_ref[shared], unit(rng.normal(size=(n - m, C)))])
    ref_f = unit(base_ref + rng.normal(scale=feat_noise, size=(n, C)))
    src_f = unit(base_src + rng.normal(scale=feat_noise, size=(n, C)))
    perm = rng.permutation(n)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return (src[perm].astype(np.float32), ref.astype(np.float32), src_f[perm].astype(np.float32), ref_f.astype(np.float32), T, match[perm])
