"""fp64 NumPy restatement of the point-to-plane ICP of include/lcr_hip.h (lcr_icp_point_to_plane): the correspondence step of
tests/icp_restatement.py, the plane update (A = sum J J^T, g = sum J r, A x = -g, T <- dT(x) T) and the loop.  The GPU tests hold the
kernels against it step by step, tools/icp_bench.py times it as the CPU baseline."""
import numpy as np

import icp_restatement as ir


def transform_vector6(x):
    """Open3D's TransformVector6dToMatrix4d: [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)]"""
    a, b, c = x[0], x[1], x[2]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    out = np.eye(4)
    out[:3, :3] = Rz @ Ry @ Rx
    out[:3, 3] = x[3:6]
    return out


def plane_update(src, tgt, tgt_normals, corr, T):
    """-> (T' f64 (4,4), applied).  Usable rows: partnered, partner normal non-zero.  T is kept when fewer than 6 are usable or an LDL^T
    pivot of A is <= 1e-12 times A's largest diagonal entry."""
    ok = corr >= 0
    nrm = np.asarray(tgt_normals, np.float32)
    use = np.zeros(len(corr), bool)
    use[ok] = np.any(nrm[corr[ok]] != 0, axis=1)
    if use.sum() < 6:
        return np.array(T, dtype=np.float64), False
    p = np.asarray(src, np.float32)[use].astype(np.float64)
    T = np.asarray(T, np.float64)
    s = ((T[None, :3, 0] * p[:, :1] + T[None, :3, 1] * p[:, 1:2]) + T[None, :3, 2] * p[:, 2:3]) + T[None, :3, 3]
    t = np.asarray(tgt, np.float32)[corr[use]].astype(np.float64)
    n = nrm[corr[use]].astype(np.float64)
    r = ((s - t) * n).sum(axis=1)
    J = np.concatenate([np.cross(s, n), n], axis=1)
    A = J.T @ J
    g = J.T @ r
    amax = np.diag(A).max()
    D = np.zeros(6)                                                # LDL^T pivots, as the kernel tests them
    L = np.eye(6)
    for j in range(6):
        D[j] = A[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
        if not D[j] > 1e-12 * amax:
            return np.array(T, dtype=np.float64), False
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / D[j]
    x = np.linalg.solve(A, -g)
    return transform_vector6(x) @ T, True


def icp(src, tgt, tgt_normals, r, init=np.eye(4), max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """One pair -> dict(T, fitness, rmse, iterations, corr, T_hist [iterations+1,4,4], fitness_hist, rmse_hist)."""
    T = np.array(init, dtype=np.float64)
    if len(src) == 0 or len(tgt) == 0:
        return dict(T=T, fitness=0.0, rmse=0.0, iterations=0, corr=np.full(len(src), -1, np.int64), T_hist=T[None], fitness_hist=np.zeros(1),
                    rmse_hist=np.zeros(1))
    res = ir.correspondence_step(src, tgt, T, r)
    Ts, fs, rs = [T], [res["fitness"]], [res["rmse"]]
    it = 0
    for _ in range(max_iteration):
        T, _ = plane_update(src, tgt, tgt_normals, res["corr"], T)
        it += 1
        new = ir.correspondence_step(src, tgt, T, r)
        Ts.append(T)
        fs.append(new["fitness"])
        rs.append(new["rmse"])
        stop = ir.converged(res, new, relative_fitness, relative_rmse)
        res = new
        if stop:
            break
    return dict(T=T, fitness=res["fitness"], rmse=res["rmse"], iterations=it, corr=res["corr"], T_hist=np.stack(Ts), fitness_hist=np.array(fs),
                rmse_hist=np.array(rs))
