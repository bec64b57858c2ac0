"""fp64 NumPy restatement of the surface normals of include/lcr_hip.h (lcr_estimate_normals): the neighbourhood is the C++ oracle's exact
radius search with neighbor_limit = max_nn (oracle.ops, CPU), which is the selection rule itself; the covariance is taken about the query
point in fp64, the eigenvectors come from numpy.linalg.eigh, and orientation and degeneracy follow the header.  The GPU tests hold the
kernels against it, tools/icp_bench.py times it as the CPU baseline."""
import numpy as np


def neighbourhoods(points, radius, max_nn):
    """-> (idx int64 [n, max_nn] cloud rows padded with n, count int [n]) of one cloud"""
    from oracle import ops
    pts = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    n = len(pts)
    if n == 0:
        return np.zeros((0, max_nn), np.int64), np.zeros(0, np.int64)
    idx = ops.radius_search(pts, pts, np.array([n]), np.array([n]), float(radius), int(max_nn))
    return idx, (idx < n).sum(axis=1)


def covariances(points, idx, count):
    """fp64 covariance about each query row: c_ab = s_ab / k - (s_a / k) (s_b / k), d = p_j - p_i -> [n,3,3]"""
    pts = np.asarray(points, np.float32).astype(np.float64)
    n, w = idx.shape
    valid = idx < n
    nb = pts[np.where(valid, idx, 0)]                                  # [n, w, 3]
    d = np.where(valid[:, :, None], nb - pts[:, None, :], 0.0)
    k = np.maximum(count, 1).astype(np.float64)
    s1 = d.sum(axis=1)
    s2 = np.einsum("nwa,nwb->nab", d, d)
    mu = s1 / k[:, None]
    return s2 / k[:, None, None] - mu[:, :, None] * mu[:, None, :]


def estimate_normals(points, radius, max_nn, viewpoint=(0.0, 0.0, 0.0)):
    """One cloud -> dict(normals f64 [n,3], curvature f64 [n], count int [n], degenerate bool [n], lam f64 [n,3] ascending,
    dot f64 [n] (n . (v - p) before orientation; |dot| tells how safe the sign is))."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    idx, count = neighbourhoods(pts, radius, max_nn)
    out = dict(normals=np.zeros((n, 3)), curvature=np.zeros(n), count=count, degenerate=np.ones(n, bool), lam=np.zeros((n, 3)),
               dot=np.zeros(n))
    if n == 0:
        return out
    C = covariances(pts, idx, count)
    lam, V = np.linalg.eigh(C)
    nrm = V[:, :, 0]
    deg = (count < 3) | (lam[:, 2] <= 1e-30) | (lam[:, 1] <= 1e-12 * lam[:, 2])
    w = np.asarray(viewpoint, np.float32).astype(np.float64)[None, :] - pts.astype(np.float64)
    dot = (nrm * w).sum(axis=1)
    first = np.where(nrm[:, 0] != 0, nrm[:, 0], np.where(nrm[:, 1] != 0, nrm[:, 1], nrm[:, 2]))
    flip = (dot < 0) | ((dot == 0) & (first < 0))
    nrm = np.where(flip[:, None], -nrm, nrm)
    with np.errstate(invalid="ignore", divide="ignore"):
        curv = lam[:, 0] / lam.sum(axis=1)
    out.update(normals=np.where(deg[:, None], 0.0, nrm), curvature=np.where(deg, 0.0, curv), degenerate=deg, lam=lam, dot=np.abs(dot))
    return out


def planes_cloud(n_per_plane=4000, seed=0):
    """Noise-free samples of three known planes (ground z = -1.7, a facade x = 8, a slanted wall) -> (points f32 [n,3], normal f64 [n,3]
    (unit, pointing toward the origin), plane id [n])"""
    rng = np.random.default_rng(seed)
    pts, nrm, pid = [], [], []
    a = rng.uniform(-6, 6, (n_per_plane, 2))
    pts.append(np.stack([a[:, 0], a[:, 1], np.full(n_per_plane, -1.7)], 1))
    nrm.append(np.tile([0.0, 0.0, 1.0], (n_per_plane, 1)))
    b = rng.uniform(-5, 5, (n_per_plane, 2))
    pts.append(np.stack([np.full(n_per_plane, 8.0), b[:, 0], b[:, 1] + 3.0], 1))
    nrm.append(np.tile([-1.0, 0.0, 0.0], (n_per_plane, 1)))
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    v = np.array([0.0, 0.0, 1.0])
    c = rng.uniform(-4, 4, (n_per_plane, 2))
    base = np.array([-10.0, 4.0, 2.0])
    pts.append(base + c[:, :1] * u + c[:, 1:] * v)
    nn = np.cross(u, v)
    nn = nn if np.dot(nn, -base) > 0 else -nn
    nrm.append(np.tile(nn, (n_per_plane, 1)))
    for i in range(3):
        pid.append(np.full(n_per_plane, i))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm), np.concatenate(pid)
