"""NumPy fp64 restatement of the TEASER-style registration of include/lcr_hip.h (lcr_teaser_registration), stage by stage, every stage
returning its intermediates; the oracle of tests/test_teaser_cpu.py and tests/test_teaser_gpu.py.  No TEASER++ binary is involved.

`mistake` plants one deviation from the definition (MISTAKES), so that the tests can show that the comparison with the GPU sees it."""
import numpy as np

MISTAKES = ("beta_without_2", "mu0_without_minus_1", "middle_weight_without_mu", "thresholds_swapped", "core_kmax_minus_1",
            "rho_term_dropped", "ties_reversed")
DEFAULTS = dict(noise_bound=0.01, cbar2=1.0, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12)


def pair_lengths(p):
    """|p_j - p_i| for all i, j as sqrt((dx dx + dy dy) + dz dz)"""
    p = np.asarray(p, np.float64)
    d = p[None, :, :] - p[:, None, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def graph(src, ref, noise_bound=0.01, cbar2=1.0, mistake=None):
    """-> (adjacency bool [N,N], | |a - b| - beta | per pair i < j (the edge margins), beta)"""
    beta = (1.0 if mistake == "beta_without_2" else 2.0) * noise_bound * np.sqrt(cbar2)
    n = len(src)
    diff = np.abs(pair_lengths(src) - pair_lengths(ref)) if n else np.zeros((0, 0))
    A = diff <= beta
    np.fill_diagonal(A, False)
    iu = np.triu_indices(n, 1)
    return A, np.abs(diff[iu] - beta), beta


def core_numbers(A):
    """Core number of every vertex by peeling: remove every vertex of degree <= k, k jumping to the smallest live degree."""
    n = len(A)
    deg = A.sum(1).astype(np.int64)
    live = np.ones(n, bool)
    core = np.zeros(n, np.int64)
    k = 0
    while live.any():
        k = max(k, int(deg[live].min()))
        rem = live & (deg <= k)
        core[rem] = k
        live[rem] = False
        deg = deg - A[:, rem].sum(1)
    return core


def core_numbers_brute(A):
    """The definition: the largest k such that the vertex lies in a subgraph of minimum degree k, over all vertex subsets."""
    n = len(A)
    core = np.zeros(n, np.int64)
    for bits in range(1, 1 << n):
        sub = np.array([(bits >> v) & 1 for v in range(n)], bool)
        k = int(A[np.ix_(sub, sub)].sum(1).min())
        core[sub] = np.maximum(core[sub], k)
    return core


def select(A, mistake=None):
    """-> (selected rows ascending, core numbers, k_max)"""
    core = core_numbers(A)
    kmax = int(core.max()) if len(core) else 0
    keep = core >= kmax - 1 if mistake == "core_kmax_minus_1" else core == kmax
    return np.nonzero(keep)[0], core, kmax


def rotation_from_H(H):
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    return V @ np.diag([1.0, 1.0, np.linalg.det(V @ U.T)]) @ U.T


def measurements(src, ref):
    """a_m = src_j - src_i, b_m = ref_j - ref_i over all pairs i < j, i-major"""
    src, ref = np.asarray(src, np.float64), np.asarray(ref, np.float64)
    i, j = np.triu_indices(len(src), 1)
    return src[j] - src[i], ref[j] - ref[i]


def gnc_tls(src, ref, noise_bound=0.01, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12, mistake=None, **_):
    """GNC-TLS rotation over all pairs of the given rows.  -> dict: R, iterations, cost (the last), weights (final), rot_inliers,
    residuals (under the final R), history [(R, mu, cost, d)] per iteration, stopped_on_mu."""
    a, b = measurements(src, ref)
    c2 = noise_bound * noise_bound
    w = np.ones(len(a))
    cost_prev, mu, hist = np.inf, 0.0, []
    out = dict(stopped_on_mu=False)
    for it in range(max_iterations):
        H = (a * w[:, None]).T @ b
        R = rotation_from_H(H)
        e = b - a @ R.T
        r = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        if it == 0:
            den = 2.0 * r.max() / c2 - (0.0 if mistake == "mu0_without_minus_1" else 1.0)
            with np.errstate(divide="ignore"):
                mu = 1.0 / den
            if not mu > 0:
                out.update(R=R, iterations=1, cost=float(r.sum()), stopped_on_mu=True)
                hist.append((R, mu, float(r.sum()), np.inf))
                break
        th1, th2 = (mu + 1.0) / mu * c2, mu / (mu + 1.0) * c2
        if mistake == "thresholds_swapped":
            th1, th2 = th2, th1
        cost = float((w * r).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            mid = np.sqrt(c2 * mu * (mu + 1.0) / r) - (0.0 if mistake == "middle_weight_without_mu" else mu)
        w = np.where(r >= th1, 0.0, np.where(r <= th2, 1.0, mid))
        d = abs(cost - cost_prev)
        hist.append((R, mu, cost, d))
        mu, cost_prev = mu * gnc_factor, cost
        out.update(R=R, iterations=it + 1, cost=cost)
        if d < cost_threshold:
            break
    out.update(weights=w, residuals=r, rot_inliers=int((w >= 0.5).sum()), history=hist)
    return out


def vote_axis(x, rho, mistake=None):
    """TLS voting on one axis.  -> dict: xhat, count, order (endpoint positions sorted), values (sorted endpoint values), costs [2K]
    (inf where C is empty), sets (|C|, first row of C in x order) per endpoint: the consensus set's identity."""
    x = np.asarray(x, np.float64)
    K = len(x)
    val = np.concatenate([x - rho, x + rho])
    pos = np.arange(2 * K)
    order = np.lexsort((-pos if mistake == "ties_reversed" else pos, val))
    inside = np.zeros(K, bool)
    costs, sets, means = np.full(2 * K, np.inf), [], np.zeros(2 * K)
    for e, p in enumerate(order):
        inside[p % K] = p < K
        if inside.any():
            xs = x[inside]
            m = xs.mean()
            costs[e] = ((xs - m) ** 2).sum() + (0.0 if mistake == "rho_term_dropped" else rho * rho * (K - len(xs)))
            means[e] = m
        sets.append(inside.tobytes())
    best = int(np.argmin(costs))                          # the first of equal minima
    last = np.zeros(K, bool)
    for p in order[:best + 1]:
        last[p % K] = p < K
    return dict(xhat=float(means[best]), count=int(last.sum()), order=order, values=val[order], costs=costs, sets=sets, best=best)


def vote_margin(v):
    """relative gap between the best cost and the best cost of any different consensus set"""
    c, best = v["costs"], v["best"]
    other = [c[e] for e in range(len(c)) if np.isfinite(c[e]) and v["sets"][e] != v["sets"][best]]
    return (min(other) - c[best]) / max(c[best], 1e-300) if other else np.inf


def teaser(src, ref, noise_bound=0.01, cbar2=1.0, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12, inlier_selection="kcore",
           mistake=None):
    """The whole definition on one problem.  -> dict with T (fp64 4x4), valid, n_selected, rot_inliers, t_count [3], iterations, cost,
    selected_mask [N], core [N], and the stages' intermediates (edge_margins, gnc, votes)."""
    src32, ref32 = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(ref, np.float32).reshape(-1, 3)
    N = len(src32)
    out = dict(T=np.eye(4), valid=0, n_selected=0, rot_inliers=0, t_count=np.zeros(3, np.int64), iterations=0, cost=0.0,
               selected_mask=np.zeros(N, np.uint8), core=np.zeros(N, np.int64), edge_margins=np.zeros(0), gnc=None, votes=None)
    if inlier_selection == "kcore":
        A, out["edge_margins"], _ = graph(src32, ref32, noise_bound, cbar2, mistake)
        sel, core, kmax = select(A, mistake)
        out.update(core=core, adjacency=A, kmax=kmax)
        if kmax < 1:
            return out
    else:
        sel = np.arange(N)
    if len(sel) < 3:
        return out
    s, r = src32[sel].astype(np.float64), ref32[sel].astype(np.float64)
    g = gnc_tls(s, r, noise_bound, gnc_factor, max_iterations, cost_threshold, mistake)
    R = g["R"]
    rho = noise_bound * np.sqrt(cbar2)
    x = r - s @ R.T
    votes = [vote_axis(x[:, k], rho, mistake) for k in range(3)]
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = [v["xhat"] for v in votes]
    mask = np.zeros(N, np.uint8)
    mask[sel] = 1
    out.update(T=T, valid=1, n_selected=len(sel), rot_inliers=g["rot_inliers"], t_count=np.array([v["count"] for v in votes]),
               iterations=g["iterations"], cost=g["cost"], selected_mask=mask, gnc=g, votes=votes, selected=sel)
    return out


def random_rotation(rng, max_angle=np.pi):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * (Kx @ Kx)


def planted(n_in, n_out, seed, noise_bound=0.01, box=40.0):
    """Planted problem: inliers ref = R src + t + uniform noise within +-0.2 noise_bound per axis, outliers uniform in the +-box cube,
    rows shuffled.  -> (src f32 [N,3], ref f32 [N,3], T fp64 4x4, inlier mask [N])"""
    rng = np.random.default_rng(1000 + seed)
    n = n_in + n_out
    R, t = random_rotation(rng), rng.uniform(-10, 10, 3)
    src = rng.uniform(-box, box, (n, 3))
    ref = src @ R.T + t + rng.uniform(-0.2 * noise_bound, 0.2 * noise_bound, (n, 3))
    ref[n_in:] = rng.uniform(-box, box, (n_out, 3))
    perm = rng.permutation(n)
    inl = np.zeros(n, bool)
    inl[:n_in] = True
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return src[perm].astype(np.float32), ref[perm].astype(np.float32), T, inl[perm]


def two_motions(seed=0, n_a=30, n_b=20, n_rand=15, noise_bound=0.01, box=40.0):
    """n_a rows of motion A, n_b of motion B, n_rand random, shuffled.  -> (src, ref, T_A, mask of the A rows)"""
    rng = np.random.default_rng(5000 + seed)
    n = n_a + n_b + n_rand
    src = rng.uniform(-box, box, (n, 3))
    ref = rng.uniform(-box, box, (n, 3))
    Ts = []
    for lo, hi in ((0, n_a), (n_a, n_a + n_b)):
        R, t = random_rotation(rng), rng.uniform(-10, 10, 3)
        ref[lo:hi] = src[lo:hi] @ R.T + t + rng.uniform(-0.2 * noise_bound, 0.2 * noise_bound, (hi - lo, 3))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        Ts.append(T)
    perm = rng.permutation(n)
    isa = np.zeros(n, bool)
    isa[:n_a] = True
    return src[perm].astype(np.float32), ref[perm].astype(np.float32), Ts[0], isa[perm]


def pendant(seed=0, noise_bound=0.01, box=40.0):
    """Three inlier rows (a triangle of the graph, core 2) and a fourth row whose length to row 0 alone is preserved (core 1 = k_max - 1):
    the input on which selecting core >= k_max - 1 shows.  -> (src, ref, T, inlier mask)"""
    src, ref, T, inl = planted(3, 0, seed, noise_bound, box)
    rng = np.random.default_rng(9000 + seed)
    s3 = rng.uniform(-box, box, 3)
    r3 = ref[0].astype(np.float64) + random_rotation(rng) @ (s3 - src[0].astype(np.float64))
    return (np.vstack([src, s3[None]]).astype(np.float32), np.vstack([ref, r3[None]]).astype(np.float32), T, np.append(inl, False))


def graded(seed=0, n_in=40, n_mid=12, n_out=8, noise_bound=0.01, box=40.0):
    """n_in inliers, n_mid rows whose noise is uniform within +-1.7 noise_bound per axis (their residuals pass through the middle band
    of the GNC weights), n_out outliers: the `none` input on which the middle weight shows.  -> (src, ref, T, mask of the n_in rows)"""
    src, ref, T, inl = planted(n_in + n_mid, n_out, seed, noise_bound, box)
    rng = np.random.default_rng(7000 + seed)
    idx = np.nonzero(inl)[0][:n_mid]
    ref = ref.astype(np.float64)
    ref[idx] += rng.uniform(-1.5 * noise_bound, 1.5 * noise_bound, (n_mid, 3))
    inl = inl.copy()
    inl[idx] = False
    return src, ref.astype(np.float32), T, inl


def observables(o):
    """what the GPU comparison holds equal"""
    return (int(o["valid"]), int(o["n_selected"]), int(o["iterations"]), int(o["rot_inliers"]), tuple(int(c) for c in o["t_count"]),
            tuple(int(c) for c in o["core"]), tuple(int(c) for c in o["selected_mask"]))


T_TOL = 4.0 * 2.0 ** -24             # per rotation entry; times max(1, |t|_inf) per translation entry
COST_TOL = 1e-9                      # relative


def seen(want, got, factor=100.0):
    """Does `got` (a dict with the output keys) differ from `want` in one of the equalities, or by factor x a tolerance in T or cost?"""
    if observables(want) != observables(got):
        return True
    Tw, Tg = np.asarray(want["T"], np.float64), np.asarray(got["T"], np.float64)
    if np.abs(Tw[:3, :3] - Tg[:3, :3]).max() > factor * T_TOL:
        return True
    if np.abs(Tw[:3, 3] - Tg[:3, 3]).max() > factor * T_TOL * max(1.0, np.abs(Tw[:3, 3]).max()):
        return True
    return abs(want["cost"] - got["cost"]) > factor * COST_TOL * abs(want["cost"])


# the planted inputs of the GPU test: (inliers, outliers, inlier_selection); N = 3, 7, 65, 130, 300 in kcore mode, 65 and 130 in none mode
CASES = [(3, 0, "kcore"), (5, 2, "kcore"), (40, 25, "kcore"), (30, 100, "kcore"), (30, 270, "kcore"), (52, 13, "none"), (100, 30, "none")]
SEEDS = (0, 1, 2)


def planted_inputs():
    """(name, (src, ref, T, inlier mask), inlier_selection) of every planted input of the CPU margin test and the GPU comparison"""
    for ni, no, mode in CASES:
        for seed in SEEDS:
            yield (ni, no, mode, seed), planted(ni, no, seed), mode
    yield ("two_motions",), two_motions(0), "kcore"
    yield ("pendant",), pendant(0), "kcore"
    yield ("graded",), graded(0), "none"
    # beyond one pass of the 1024-thread selection and voting workgroups (N > 1024, 2K > 1024) and of the 256 partials of a step
    yield ("n1100",), planted(600, 500, 0), "kcore"
    # more selected rows than the 256 threads of a sweep workgroup, in the mode that runs the GNC loop
    yield ("k270",), planted(230, 40, 0), "none"


# the input on which each planted mistake shows in what the GPU comparison holds equal (or at 100 x a tolerance); ties_reversed reaches
# no output (tests/test_teaser_cpu.py says why)
MISTAKE_INPUTS = {
    "beta_without_2": lambda: (planted(30, 270, 0), "kcore"),
    "mu0_without_minus_1": lambda: (planted(40, 25, 0), "kcore"),
    "middle_weight_without_mu": lambda: (graded(0), "none"),
    "thresholds_swapped": lambda: (planted(52, 13, 0), "none"),
    "core_kmax_minus_1": lambda: (pendant(0), "kcore"),
    "rho_term_dropped": lambda: (planted(5, 2, 0), "kcore"),
}
