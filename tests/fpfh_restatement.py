"""fp64 NumPy restatement of the FPFH descriptors of include/lcr_hip.h (lcr_fpfh): the neighbourhood is the C++ oracle's exact radius
search with neighbor_limit = max_nn (oracle.ops, CPU) with the row itself removed wherever it stands; pair features, bins, SPFH and FPFH
follow the header line by line.  Besides the descriptors it returns a per-row MARGIN: how far the row's pair features stay from every
discrete decision (a bin boundary, the swap, the |v| == 0 test), so that a test can tell the rows whose integer votes do not depend on the
last bits of an fp64 chain.  The GPU tests hold the kernels against it, tools/fpfh_bench.py times it as the CPU baseline."""
import numpy as np

import normals_restatement as nr

SAFE_MARGIN = 1e-9          # many orders of magnitude above the fp64 rounding of the chain (~1e-15 relative)
BINS = 33


def neighbourhoods(points, radius, max_nn):
    """-> (idx int64 [n, max_nn] rows of the cloud without the row itself, padded with n at the end; d2 f32 [n, max_nn] the search's
    fp32 squared distances (0 in the padding); m int [n])"""
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    n = len(pts)
    idx, _ = nr.neighbourhoods(pts, radius, max_nn)
    if n == 0:
        return idx, np.zeros((0, max_nn), np.float32), np.zeros(0, np.int64)
    keep = (idx < n) & (idx != np.arange(n)[:, None])
    order = np.argsort(~keep, axis=1, kind="stable")                    # kept entries first, in list order
    idx = np.where(np.take_along_axis(keep, order, 1), np.take_along_axis(idx, order, 1), n)
    valid = idx < n
    d = pts[:, None, :] - pts[np.where(valid, idx, 0)]                   # fp32, every operation rounded: the search's own d2
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return idx, np.where(valid, d2, np.float32(0)).astype(np.float32), valid.sum(axis=1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _after_swap(n1, n2, dp, a1, a2, swap):
    """Features for a given swap decision -> (f [..,3], |v| [..]); pairs with d == 0 are overwritten by the caller."""
    s = swap[..., None]
    m1, m2, q = np.where(s, n2, n1), np.where(s, n1, n2), np.where(s, -dp, dp)
    f2 = np.where(swap, -a2, a1)
    v = _cross(q, m1)
    vn = np.sqrt(_dot(v, v))
    zero = vn == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        v = v / vn[..., None]
    w = _cross(m1, v)
    f1 = _dot(v, m2)
    f0 = np.arctan2(_dot(w, m2), _dot(m1, m2))
    f = np.stack([f0, f1, f2], axis=-1)
    return np.where(zero[..., None], 0.0, f), vn


def _scaled(f):
    return np.stack([11.0 * (f[..., 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[..., 1] + 1.0) / 2.0, 11.0 * (f[..., 2] + 1.0) / 2.0], axis=-1)


def _bins(scaled):
    with np.errstate(invalid="ignore"):
        b = np.floor(scaled)
    return np.where(b >= 0, np.minimum(b, 10), 0).astype(np.int64)        # NaN -> 0, as the kernel


def pair_features(p1, n1, p2, n2):
    """fp64 on the fp32 inputs promoted, broadcast over leading axes -> (bins int [..,3], margin [..])."""
    p1, n1, p2, n2 = (np.asarray(x, np.float32).astype(np.float64) for x in (p1, n1, p2, n2))
    n1, n2 = np.broadcast_arrays(n1, n2)
    dp = p2 - p1
    d = np.sqrt(_dot(dp, dp))
    coincident = d == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        a1, a2 = _dot(n1, dp) / d, _dot(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        f, vn = _after_swap(n1, n2, dp, a1, a2, swap)
        g, un = _after_swap(n1, n2, dp, a1, a2, ~swap)
        f = np.where(coincident[..., None], 0.0, f)
        sc = _scaled(f)
        bins = _bins(sc)
        # (1) distance of the three scaled values to an interior bin boundary 1..10, in bin units
        margin = np.abs(sc[..., None] - np.arange(1.0, 11.0)).min(axis=(-1, -2))
        # (2) the swap: only where the other decision would change a bin or a zero test, never where n1 == n2 bitwise
        other = _bins(_scaled(g))
        matters = ((other != bins).any(axis=-1) | ((vn == 0) != (un == 0))) & ~(n1 == n2).all(axis=-1)
        margin = np.where(matters, np.minimum(margin, np.abs(np.abs(a1) - np.abs(a2))), margin)
        # (3) the |v| == 0 test
        margin = np.minimum(margin, vn / d)
    margin = np.where(coincident, 0.5, margin)                         # d == 0 is decided on the inputs; its votes sit mid-bin
    return bins, np.nan_to_num(margin, nan=0.0)


def fpfh(points, normals, radius, max_nn):
    """One cloud -> dict(features f64 [n,33], spfh f64 [n,33], votes int [n,33], count int [n], margin f64 [n] (inf for m == 0),
    safe_spfh bool [n], safe_fpfh bool [n], idx, d2)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    n = len(pts)
    idx, d2, m = neighbourhoods(pts, radius, max_nn)
    votes = np.zeros((n, BINS), np.int64)
    margin = np.full(n, np.inf)
    out = dict(features=np.zeros((n, BINS)), spfh=np.zeros((n, BINS)), votes=votes, count=m, margin=margin, safe_spfh=np.ones(n, bool),
               safe_fpfh=np.ones(n, bool), idx=idx, d2=d2)
    if n == 0:
        return out
    valid = idx < n
    nb = np.where(valid, idx, 0)
    bins, pm = np.zeros(idx.shape + (3,), np.int64), np.zeros(idx.shape)
    for r0 in range(0, n, 1024):                                       # row chunks: the margins take [rows, max_nn, 3, 10] doubles
        r = slice(r0, r0 + 1024)
        bins[r], pm[r] = pair_features(pts[r, None, :], nrm[r, None, :], pts[nb[r]], nrm[nb[r]])
    rows = np.broadcast_to(np.arange(n)[:, None], idx.shape)[valid]
    for k in range(3):
        np.add.at(votes, (rows, 11 * k + bins[..., k][valid]), 1)
    margin[:] = np.where(valid, pm, np.inf).min(axis=1, initial=np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        spfh = np.where(m[:, None] > 0, (votes * 100).astype(np.float64) / m[:, None], 0.0)
    use = valid & (d2 != 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        wgt = np.where(use, 1.0, 0.0)[:, :, None] * spfh[nb] / np.where(use, d2.astype(np.float64), 1.0)[:, :, None]
    acc = wgt.sum(axis=1)                                                # fp64: the order of the sum is far below the test's bound
    s = acc.reshape(n, 3, 11).sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.where(s != 0, 100.0 / s, 0.0)
    feat = acc * np.repeat(scale, 11, axis=1) + spfh
    safe = margin >= SAFE_MARGIN
    safe_f = safe & np.where(valid, safe[nb], True).all(axis=1)
    out.update(features=feat, spfh=spfh, safe_spfh=safe, safe_fpfh=safe_f)
    return out


def nearest_rows(cloud, k=3000):
    """the k rows of a scan nearest the sensor (the origin), in their original order"""
    c = np.asarray(cloud, np.float32).reshape(-1, 3)
    d = (c.astype(np.float64) ** 2).sum(axis=1)
    return np.ascontiguousarray(c[np.sort(np.argsort(d, kind="stable")[:k])])


def scene_cloud(seed=0):
    """2 100 points seen from a sensor at the origin: ground (900, sigma 2 cm), a wall (600, sigma 1 cm) and a standing cylinder
    (600, sigma 1 cm) -> f32 [2100,3]"""
    rng = np.random.default_rng(seed)
    g = rng.uniform([2.0, -3.0], [8.0, 3.0], (900, 2))
    ground = np.stack([g[:, 0], g[:, 1], -1.7 + rng.normal(0, 0.02, 900)], 1)
    w = rng.uniform([-3.0, -1.7], [3.0, 1.3], (600, 2))
    wall = np.stack([8.0 + rng.normal(0, 0.01, 600), w[:, 0], w[:, 1]], 1)
    th, z = rng.uniform(0, 2 * np.pi, 600), rng.uniform(-1.7, 1.3, 600)
    r = 0.8 + rng.normal(0, 0.01, 600)
    cyl = np.stack([4.5 + r * np.cos(th), 1.0 + r * np.sin(th), z], 1)
    return np.concatenate([ground, wall, cyl]).astype(np.float32)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)
