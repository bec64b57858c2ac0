"""fp64 NumPy restatement of the generalized ICP of include/lcr_hip.h (lcr_icp_generalized): the correspondence step of
tests/icp_restatement.py, the plane-to-plane update (W = (C_t + R C_s R^T)^-1 per row, A = sum J^T W J, g = sum J^T W d, A x = -g,
T <- dT(x) T) and the loop.  It is the definition of the estimator: the GPU tests hold the kernels against it step by step,
tools/icp_bench.py times it as the CPU baseline."""
import numpy as np

import icp_plane_restatement as ipr
import icp_restatement as ir


def covariance(n, eps):
    """C(n) = I - (1 - eps) n n^T for one normal [3] or rows of normals [k,3] (promoted to fp64, not renormalised): eps along a unit
    normal, 1 across it; the zero normal gives I."""
    n = np.asarray(n, dtype=np.float64)
    return np.eye(3) - (1.0 - eps) * n[..., :, None] * n[..., None, :]


def normal_equations(src, src_normals, tgt, tgt_normals, corr, T, eps, reverse=False):
    """-> (A f64 (6,6), g f64 (6,), count) over the partnered rows at pose T; reverse sums the rows in the opposite order (for the
    spread that the order of an fp64 sum leaves in T')."""
    ok = np.nonzero(np.asarray(corr) >= 0)[0]
    if reverse:
        ok = ok[::-1]
    T = np.asarray(T, np.float64)
    p = np.asarray(src, np.float32)[ok].astype(np.float64)
    n = np.asarray(src_normals, np.float32)[ok].astype(np.float64)
    s = ((T[None, :3, 0] * p[:, :1] + T[None, :3, 1] * p[:, 1:2]) + T[None, :3, 2] * p[:, 2:3]) + T[None, :3, 3]
    a = (T[None, :3, 0] * n[:, :1] + T[None, :3, 1] * n[:, 1:2]) + T[None, :3, 2] * n[:, 2:3]
    t = np.asarray(tgt, np.float32)[corr[ok]].astype(np.float64)
    b = np.asarray(tgt_normals, np.float32)[corr[ok]].astype(np.float64)
    d = s - t
    M = 2.0 * np.eye(3)[None] - (1.0 - eps) * (a[:, :, None] * a[:, None, :] + b[:, :, None] * b[:, None, :])
    W = np.linalg.inv(M) if len(ok) else M
    J = np.zeros((len(ok), 3, 6))                                  # [-[s]x | I]
    J[:, 0, 1], J[:, 0, 2] = s[:, 2], -s[:, 1]
    J[:, 1, 0], J[:, 1, 2] = -s[:, 2], s[:, 0]
    J[:, 2, 0], J[:, 2, 1] = s[:, 1], -s[:, 0]
    J[:, :, 3:] = np.eye(3)
    WJ = W @ J
    A = (J.transpose(0, 2, 1) @ WJ).sum(axis=0)
    g = (WJ.transpose(0, 2, 1) @ d[:, :, None]).sum(axis=0)[:, 0]
    return A, g, len(ok)


def gicp_update(src, src_normals, tgt, tgt_normals, corr, T, eps, reverse=False):
    """-> (T' f64 (4,4), applied).  T is kept when fewer than 3 rows are partnered or an LDL^T pivot of A is <= 1e-12 times A's largest
    diagonal entry (the pivot rule of icp_plane_restatement.plane_update)."""
    A, g, count = normal_equations(src, src_normals, tgt, tgt_normals, np.asarray(corr), T, eps, reverse)
    if count < 3:
        return np.array(T, dtype=np.float64), False
    amax = np.diag(A).max()
    D = np.zeros(6)
    L = np.eye(6)
    for j in range(6):
        D[j] = A[j, j] - (L[j, :j] ** 2 * D[:j]).sum()
        if not D[j] > 1e-12 * amax:
            return np.array(T, dtype=np.float64), False
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / D[j]
    x = np.linalg.solve(A, -g)
    return ipr.transform_vector6(x) @ np.asarray(T, np.float64), True


def icp(src, src_normals, tgt, tgt_normals, r, init=np.eye(4), eps=1e-3, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """One pair -> dict(T, fitness, rmse, iterations, corr, T_hist [iterations+1,4,4], fitness_hist, rmse_hist)."""
    T = np.array(init, dtype=np.float64)
    if len(src) == 0 or len(tgt) == 0:
        return dict(T=T, fitness=0.0, rmse=0.0, iterations=0, corr=np.full(len(src), -1, np.int64), T_hist=T[None], fitness_hist=np.zeros(1),
                    rmse_hist=np.zeros(1))
    res = ir.correspondence_step(src, tgt, T, r)
    Ts, fs, rs = [T], [res["fitness"]], [res["rmse"]]
    it = 0
    for _ in range(max_iteration):
        T, _ = gicp_update(src, src_normals, tgt, tgt_normals, res["corr"], T, eps)
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
