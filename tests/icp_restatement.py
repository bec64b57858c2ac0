"""fp64 NumPy restatement of the point-to-point ICP of include/lcr_hip.h (lcr_icp_point_to_point): correspondence step, Kabsch update,
loop and stopping rule.  Nearest neighbours come from the C++ oracle's exact radius search with neighbor_limit = 1 (oracle.ops, CPU), on
the same fp32 transformed rows; Kabsch uses NumPy's SVD.  The GPU tests hold the kernels against it step by step, tools/icp_bench.py times
it as the CPU baseline."""
import numpy as np


def transform_f32(src, T):
    """q = fp32(((T00*x + T01*y) + T02*z) + T03) per row, in fp64 without contraction (NumPy never fuses)."""
    p = np.asarray(src, dtype=np.float32).astype(np.float64)
    T = np.asarray(T, dtype=np.float64)
    q = np.empty((len(p), 3), np.float32)
    for r in range(3):
        q[:, r] = (((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]).astype(np.float32)
    return q


def correspondence_step(src, tgt, T, r):
    """-> dict(corr int64 [n] (target row or -1), count, fitness, rmse, d2 f32 [n] (0 where unpartnered)) at pose T."""
    from oracle import ops
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    n = len(src)
    if n == 0 or len(tgt) == 0:
        return dict(corr=np.full(n, -1, np.int64), count=0, fitness=0.0, rmse=0.0, d2=np.zeros(n, np.float32))
    q = transform_f32(src, T)
    nn = ops.radius_search(q, tgt, np.array([n]), np.array([len(tgt)]), float(r), 1)[:, 0]
    corr = np.where(nn < len(tgt), nn, -1).astype(np.int64)
    ok = corr >= 0
    d = q[ok] - tgt[corr[ok]]                                    # fp32
    d2 = np.zeros(n, np.float32)
    d2[ok] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    count = int(ok.sum())
    rmse = float(np.sqrt(d2[ok].astype(np.float64).sum() / count)) if count else 0.0
    return dict(corr=corr, count=count, fitness=count / n, rmse=rmse, d2=d2)


def kabsch_update(src, tgt, corr, T):
    """Unit-weight Kabsch of the original source rows onto their partners -> (T' f64 (4,4), applied).  T is kept when fewer than 3 rows
    are partnered or H is degenerate (sigma_2 <= 1e-9 sigma_1 or sigma_1 <= 1e-30)."""
    ok = corr >= 0
    if ok.sum() < 3:
        return np.array(T, dtype=np.float64), False
    p = np.asarray(src, np.float32)[ok].astype(np.float64)
    r = np.asarray(tgt, np.float32)[corr[ok]].astype(np.float64)
    cp, cr = p.mean(axis=0), r.mean(axis=0)
    H = (p - cp).T @ (r - cr)
    U, S, Vt = np.linalg.svd(H)
    if S[0] <= 1e-30 or S[1] <= 1e-9 * S[0]:
        return np.array(T, dtype=np.float64), False
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0])
    R = Vt.T @ D @ U.T
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, cr - R @ cp
    return out, True


def converged(prev, cur, relative_fitness, relative_rmse):
    return abs(prev["fitness"] - cur["fitness"]) < relative_fitness and abs(prev["rmse"] - cur["rmse"]) < relative_rmse


def icp(src, tgt, r, init=np.eye(4), max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """One pair -> dict(T, fitness, rmse, iterations, corr, T_hist [iterations+1,4,4], fitness_hist, rmse_hist)."""
    T = np.array(init, dtype=np.float64)
    if len(src) == 0 or len(tgt) == 0:
        return dict(T=T, fitness=0.0, rmse=0.0, iterations=0, corr=np.full(len(src), -1, np.int64), T_hist=T[None], fitness_hist=np.zeros(1),
                    rmse_hist=np.zeros(1))
    res = correspondence_step(src, tgt, T, r)
    Ts, fs, rs = [T], [res["fitness"]], [res["rmse"]]
    it = 0
    for _ in range(max_iteration):
        T, _ = kabsch_update(src, tgt, res["corr"], T)
        it += 1
        new = correspondence_step(src, tgt, T, r)
        Ts.append(T)
        fs.append(new["fitness"])
        rs.append(new["rmse"])
        stop = converged(res, new, relative_fitness, relative_rmse)
        res = new
        if stop:
            break
    return dict(T=T, fitness=res["fitness"], rmse=res["rmse"], iterations=it, corr=res["corr"], T_hist=np.stack(Ts), fitness_hist=np.array(fs),
                rmse_hist=np.array(rs))


def rigid(axis, angle_deg, t):
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    a = np.deg2rad(angle_deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = t
    return T


def planted_scan_pair(target, motion, keep=0.7, noise=0.01, seed=0):
    """Source = a random `keep` share of the target's rows moved by motion^-1, plus Gaussian noise (m), so that `motion` maps the
    source onto the target.  -> source f32 [n,3]."""
    rng = np.random.default_rng(seed)
    tgt = np.asarray(target, np.float64)
    sub = tgt[rng.random(len(tgt)) < keep]
    R, t = motion[:3, :3], motion[:3, 3]
    src = (sub - t) @ R + rng.normal(scale=noise, size=sub.shape)
    return src.astype(np.float32)
