"""fp64 NumPy restatement of the deterministic correspondence RANSAC of include/lcr_hip.h (lcr_ransac_correspondences): sampler,
Kabsch hypotheses, scoring and selection.  The GPU tests hold the kernels against it, tools/ransac_bench.py times it as the CPU
baseline.  Scores are computed in fp64 here and in fp32 on the device, so inlier decisions may differ for rows whose distance lies
within rounding of the threshold."""
import numpy as np

GOLDEN_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def sample(seed, h, ransac_n, n):
    """int64 [len(h), ransac_n]: draw j of hypothesis h = (hi32(SplitMix64(seed + gamma * (1 + 8h + j))) * n) >> 32."""
    h = np.asarray(h, dtype=np.uint64).reshape(-1)
    j = np.arange(ransac_n, dtype=np.uint64)
    k = np.uint64(1) + np.uint64(8) * h[:, None] + j[None, :]
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + GOLDEN_GAMMA * k
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    return (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def kabsch(ps, pr):
    """Unit-weight Kabsch of batches ps, pr [H,k,3] (fp64) -> R [H,3,3], t [H,3], valid [H] (sigma_2 > 1e-9 sigma_1 and sigma_1 > 1e-30)."""
    cs, cr = ps.mean(axis=1), pr.mean(axis=1)
    Hm = np.einsum("hjr,hjc->hrc", ps - cs[:, None], pr - cr[:, None])
    U, S, Vt = np.linalg.svd(Hm)
    valid = ~((S[:, 0] <= 1e-30) | (S[:, 1] <= 1e-9 * S[:, 0]))
    V = np.transpose(Vt, (0, 2, 1))
    Ut = np.transpose(U, (0, 2, 1))
    sgn = np.where(np.linalg.det(V @ Ut) >= 0, 1.0, -1.0)
    D = np.zeros_like(Hm)
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = sgn
    R = V @ D @ Ut
    t = cr - np.einsum("hrc,hc->hr", R, cs)
    R[~valid] = np.eye(3)
    t[~valid] = 0.0
    return R, t, valid


def hypotheses(src, ref, seed, ransac_n, iterations):
    """All hypotheses of one pair: (idx [H,ransac_n], R [H,3,3], t [H,3], valid [H]); no valid one when the pair has < ransac_n rows."""
    src, ref = np.asarray(src, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    n = len(src)
    if n < ransac_n:
        H = iterations
        return np.zeros((H, ransac_n), np.int64), np.tile(np.eye(3), (H, 1, 1)), np.zeros((H, 3)), np.zeros(H, bool)
    idx = sample(seed, np.arange(iterations), ransac_n, n)
    R, t, valid = kabsch(src[idx], ref[idx])
    return idx, R, t, valid


def score(src, ref, R, t, thr, chunk=256):
    """Inlier count and inlier SSE of every hypothesis (fp64): row i is an inlier iff |R src_i + t - ref_i|^2 < thr^2."""
    src, ref = np.asarray(src, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    H = len(R)
    counts, sse = np.zeros(H, np.int64), np.zeros(H, np.float64)
    for a in range(0, H, chunk):
        b = min(H, a + chunk)
        d = np.matmul(src[None], np.transpose(R[a:b], (0, 2, 1))) + t[a:b, None, :] - ref[None]
        d2 = np.einsum("hnc,hnc->hn", d, d)
        m = d2 < thr * thr
        counts[a:b] = m.sum(axis=1)
        sse[a:b] = np.where(m, d2, 0.0).sum(axis=1)
    return counts, sse


def select(counts, sse, valid):
    """Index of the winner in the total order (count desc, SSE asc, h asc) over valid hypotheses with >= 1 inlier, or -1."""
    c = np.where(valid, counts, -1)
    ok = np.nonzero(c >= 1)[0]
    if len(ok) == 0:
        return -1
    order = np.lexsort((ok, sse[ok], -c[ok]))
    return int(ok[order[0]])


def ransac(src, ref, thr, ransac_n, iterations, seed=0):
    """One pair -> dict(T (4,4) fp64, inliers, rmse, best_h, and the per-hypothesis idx / R / t / valid / counts / sse)."""
    idx, R, t, valid = hypotheses(src, ref, seed, ransac_n, iterations)
    counts, sse = score(src, ref, R, t, thr) if len(src) else (np.zeros(iterations, np.int64), np.zeros(iterations))
    counts = np.where(valid, counts, -1)
    best = select(counts, sse, valid)
    T = np.eye(4)
    inl, rmse = 0, 0.0
    if best >= 0:
        T[:3, :3], T[:3, 3] = R[best], t[best]
        inl, rmse = int(counts[best]), float(np.sqrt(sse[best] / counts[best]))
    return dict(T=T, inliers=inl, rmse=rmse, best_h=best, idx=idx, R=R, t=t, valid=valid, counts=counts, sse=sse)


def planted_pair(n, outlier_frac, noise, seed, extent=40.0):
    """src [n,3], ref = T src + noise for the inliers, uniform ref for the outliers (f32); -> (src, ref, T (4,4) fp64, inlier mask)."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-extent, extent, size=(n, 3))
    src[:, 2] *= 0.1
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.2, 1.0)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    t = rng.uniform(-5, 5, size=3)
    ref = src @ R.T + t + rng.normal(scale=noise, size=(n, 3))
    out = rng.random(n) < outlier_frac
    ref[out] = rng.uniform(-extent, extent, size=(int(out.sum()), 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return src.astype(np.float32), ref.astype(np.float32), T, ~out


def save_golden_pair_files(out_dir, golden_path, copies=1, seq=0):
    """`{seq}_{anc}_{pos}.npz` pair files (io_formats.save_registration) built from a fixture holding the reference's correspondences:
    pos / anc correspondence points and scores, its LGR estimated_transform, and as ground truth the fixture's `transform_gt` (planted
    pairs: anchor onto positive) or else its estimated_transform.  Point clouds the fixture does not hold are stood in by the
    correspondence points (the evaluation never reads them)."""
    import torch
    from lcrnet_amd import io_formats as io
    g = np.load(golden_path)
    pos, anc = g["pos_corr_points"], g["anc_corr_points"]
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in (("pos_points_f", pos), ("anc_points_f", anc), ("pos_points_c", pos),
                                                                        ("anc_points_c", anc), ("pos_corr_points", pos), ("anc_corr_points", anc))}
    out.update(pos_node_corr_indices=torch.from_numpy(g["pos_node_corr_indices"].astype(np.int64)),
               anc_node_corr_indices=torch.from_numpy(g["anc_node_corr_indices"].astype(np.int64)),
               corr_scores=torch.from_numpy(g["corr_scores"]), estimated_transform=torch.from_numpy(g["estimated_transform"]),
               pos_feature_global=torch.zeros(1, 256), anc_feature_global=torch.zeros(1, 256))
    gt = g["transform_gt"] if "transform_gt" in g else g["estimated_transform"]
    return [io.save_registration(out_dir, seq, 100 + i, 200 + i, out, gt) for i in range(copies)]
