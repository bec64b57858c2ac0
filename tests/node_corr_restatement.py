"""NumPy restatement of the ground-truth node correspondences of include/lcr_hip.h (lcr_node_correspondences), in fp32 mirroring the
definition's chain operation by operation (NumPy rounds every float32 operation and never fuses) and again in fp64, seeded case builders
in the layout `lcr_point_to_node_partition_stack` emits, and a handful of plantable mistakes.  Not a test module."""
import numpy as np

MISTAKES = ("le", "div_k", "no_knn_mask", "no_node_mask", "wrong_side", "row_for_col", "pad_other")


def transform_points(pts, T, dtype):
    """q' = ((R0*x + R1*y) + R2*z) + t per component, every operation rounded in `dtype`."""
    p, T = pts.astype(dtype), np.asarray(T).reshape(4, 4).astype(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1)


def _boxes(pts, knn, valid):
    """Axis-aligned boxes of the valid finite patch points, (M,3) lo / hi in fp64; empty boxes are (+inf, -inf)."""
    M, K = knn.shape
    g = pts[np.where(valid, knn, 0)].astype(np.float64)                     # (M,K,3)
    ok = valid & np.isfinite(g).all(-1)
    lo = np.where(ok[..., None], g, np.inf).min(1) if K else np.full((M, 3), np.inf)
    hi = np.where(ok[..., None], g, -np.inf).max(1) if K else np.full((M, 3), -np.inf)
    return lo, hi


def pair_labels(ref_pts, src_pts, ref_knn, src_knn, ref_km, src_km, ref_nm, src_nm, T, pos_radius, dtype=np.float32, mistake=None,
                r2_shift=0.0):
    """One pair.  -> dict(rows int64 (C,2) row-major, overlaps float32 (C,), cr / cs int32 (M,N) coverage counts, nr (M,), ns (N,)).
    dtype float32: the definition itself.  dtype float64: the same formulas in double on the float32 inputs, r2 = pos_radius**2 + r2_shift."""
    assert mistake is None or mistake in MISTAKES
    M, K = ref_knn.shape
    N = src_knn.shape[0]
    n_ref, n_src = len(ref_pts), len(src_pts)
    if dtype == np.float32:
        r2 = np.float32(pos_radius * pos_radius)
    else:
        r2 = np.float64(pos_radius) * np.float64(pos_radius) + r2_shift
    if mistake == "wrong_side":
        ref_t, src_t = transform_points(ref_pts, T, dtype), src_pts.astype(dtype)
    else:
        ref_t, src_t = ref_pts.astype(dtype), transform_points(src_pts, T, dtype)

    def valid(knn, km, nm, n_pts):
        v = (knn >= 0) & (knn < n_pts)
        if mistake != "no_knn_mask":
            v &= km.astype(bool)
        if mistake != "no_node_mask":
            v &= nm.astype(bool)[:, None]
        return v

    rv = valid(ref_knn, ref_km, ref_nm, n_ref)
    sv = valid(src_knn, src_km, src_nm, n_ref if mistake == "pad_other" else n_src)
    if mistake == "pad_other":
        sv &= src_knn < n_src                                              # (stay inside the array; the planted error is the smaller bound)
    nr, ns = rv.sum(1).astype(np.int32), sv.sum(1).astype(np.int32)
    cr, cs = np.zeros((M, N), np.int32), np.zeros((M, N), np.int32)
    if M and N and K:
        # candidates: boxes closer than the radius with a generous fp64 margin (the definition has no screen; this one is far from lossy)
        rlo, rhi = _boxes(ref_t, ref_knn, rv)
        slo, shi = _boxes(src_t, src_knn, sv)
        with np.errstate(invalid="ignore"):
            gap = np.maximum(slo[None] - rhi[:, None], rlo[:, None] - shi[None]).max(-1)      # (M,N); +inf where a box is empty
        cand = np.argwhere(gap <= 1.05 * pos_radius + 1e-2 * (1.0 + pos_radius))
        rp = np.where(rv[..., None], ref_t[np.where(rv, ref_knn, 0)], dtype(np.nan))          # invalid entries: NaN, never near
        sp = np.where(sv[..., None], src_t[np.where(sv, src_knn, 0)], dtype(np.nan))
        for a in range(0, len(cand), 256):
            ii, jj = cand[a:a + 256, 0], cand[a:a + 256, 1]
            with np.errstate(all="ignore"):
                d = rp[ii][:, :, None, :] - sp[jj][:, None, :, :]                              # (B,K,K,3) d = p - q'
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                near = (d2 <= r2) if mistake == "le" else (d2 < r2)
            cr[ii, jj] = near.any(2).sum(1)
            cs[ii, jj] = near.any(1).sum(1)
    if mistake == "row_for_col":
        cs = cr.copy()
    rows = np.argwhere(cr > 0).astype(np.int64)                                               # row-major
    i, j = rows[:, 0], rows[:, 1]
    f = np.float32
    dr = np.full(len(i), K, f) if mistake == "div_k" else nr[i].astype(f)
    ds = np.full(len(j), K, f) if mistake == "div_k" else ns[j].astype(f)
    overlaps = ((cr[i, j].astype(f) / dr + cs[i, j].astype(f) / ds) / f(2)).astype(f)
    return {"rows": rows, "overlaps": overlaps, "cr": cr, "cs": cs, "nr": nr, "ns": ns}


def batch_labels(case, dtype=np.float32, mistake=None, r2_shift=0.0):
    """Every pair of a stacked case (make_case's dict) -> list of pair_labels results."""
    po, mo = case["point_off"], case["node_off"]
    out = []
    for p in range(case["P"]):
        a, b = 2 * p, 2 * p + 1
        m0 = mo[0]
        sl = lambda c: slice(mo[c] - m0, mo[c + 1] - m0)
        out.append(pair_labels(case["points"][po[a]:po[a + 1]], case["points"][po[b]:po[b + 1]], case["knn"][sl(a)], case["knn"][sl(b)],
                               case["knn_mask"][sl(a)], case["knn_mask"][sl(b)], case["node_mask"][sl(a)], case["node_mask"][sl(b)],
                               case["transforms"][p], case["pos_radius"], dtype, mistake, r2_shift))
    return out


def stacked(labels):
    """(corr int32 (C,2), overlaps float32 (C,), start int32 (P+1,)) as the native call lays them out."""
    counts = [len(l["rows"]) for l in labels]
    corr = np.concatenate([l["rows"] for l in labels] or [np.zeros((0, 2), np.int64)]).astype(np.int32).reshape(-1, 2)
    ov = np.concatenate([l["overlaps"] for l in labels] or [np.zeros(0, np.float32)]).astype(np.float32)
    return corr, ov, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


# ---- case builders -----------------------------------------------------------------------------------------------------------------------
def rot90(ax, quarter_turns):
    """Rotation by quarter_turns * 90 degrees about axis ax: entries in {-1, 0, 1}, exact."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter_turns % 4]
    R = np.eye(3)
    a, b = [(1, 2), (0, 2), (0, 1)][ax]
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return R


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _patches(rng, pts, M, K, drop, spacing):
    """M nodes over a cloud: centre = a random point, patch = its K nearest points (patches of neighbouring nodes share points), entries
    beyond the cloud padded with len(pts), a share `drop` of the rest masked though they keep a real index (the reference's knn holds
    the K nearest points of the WHOLE cloud and masks those of other nodes)."""
    n = len(pts)
    knn = np.full((M, K), n, np.int64)
    km = np.zeros((M, K), np.uint8)
    nodes = np.zeros((M, 3), np.float32)
    for m in range(M):
        if n == 0:
            continue
        c = pts[rng.integers(n)]
        nodes[m] = c
        order = np.argsort(((pts.astype(np.float64) - c) ** 2).sum(1), kind="stable")[:K]
        knn[m, :len(order)] = order
        km[m, :len(order)] = rng.random(len(order)) >= drop
        if rng.random() < 0.3:                                              # a short patch: the tail holds the padding index
            cut = int(rng.integers(0, K + 1))
            knn[m, cut:], km[m, cut:] = n, 0
    return nodes, knn, km


def make_case(seed, sizes, K, mode="generic", pos_radius=0.45, bound=80.0, n_pts=600, drop=0.3, overlap_share=0.7, special=True):
    """A stacked case of P = len(sizes) pairs; sizes = [(ref nodes, src nodes), ...].
    mode "generic": coordinates up to `bound` m, random rotations.  mode "lattice": coordinates multiples of 1/16 m within +-32 m, rotations
    by multiples of 90 degrees about the axes and lattice translations, so that every product and sum of the direct AND of the expanded
    distance formula is exact in fp32; pairs at exactly d^2 = 0.25 are planted (0.5 m along an axis).
    special: plants a node with every knn entry masked and a node with node_mask = 0 on each side that has at least 3 nodes.
    Pair p with p % 4 == 3 (when P > 3) has no overlap at all: its two blocks of points lie tens of metres apart."""
    rng = np.random.default_rng(seed)
    lattice = mode == "lattice"
    pts_all, nodes_all, knn_all, km_all, nm_all, Ts = [], [], [], [], [], []
    point_off, node_off = [0], [0]
    for p, (M, N) in enumerate(sizes):
        n_ref = n_pts + int(rng.integers(0, 40))
        n_src = n_pts + 40 + int(rng.integers(0, 40))                       # the src cloud is the larger one (what "pad_other" trips over)
        apart = len(sizes) > 3 and p % 4 == 3                               # a pair with no overlap at all: the blocks end up far apart
        if lattice:
            ext = 4.0                                                       # a dense block somewhere inside +-32 m
            c0 = np.round(rng.uniform(-22, 22, 3) * 16) / 16
            c0[0] = 16.0 if apart else c0[0]
            ref = c0 + np.round(rng.uniform(-ext, ext, (n_ref, 3)) * 16) / 16
            R = rot90(int(rng.integers(3)), int(rng.integers(4))) @ rot90(int(rng.integers(3)), int(rng.integers(4)))
            t = np.round(rng.uniform(-4, 4, 3) * 16) / 16
        else:
            ext = 5.0
            az = rng.uniform(0, 2 * np.pi)                                  # |R^T (x - t)| <= |c0| + 17 stays below the bound
            c0 = rng.uniform(0.56 * bound, 0.78 * bound) * np.array([np.cos(az), np.sin(az), 0.0]) + np.array([0, 0, rng.uniform(-2, 2)])
            c0[0] = 30.0 if apart else c0[0]
            ref = c0 + rng.uniform(-ext, ext, (n_ref, 3))
            R = random_rotation(rng)
            t = rng.uniform(-4, 4, 3)
        # src = the ref points (a share of them) moved back by the inverse transform, jittered around the radius
        k_shared = int(overlap_share * n_src)
        base = ref[rng.integers(0, n_ref, k_shared)]
        if lattice:
            jit = rng.integers(-8, 9, (k_shared, 3)) / 16.0 * (rng.random((k_shared, 1)) < 0.7)
            jit[: k_shared // 8] = 0
            ax = rng.integers(0, 3, k_shared // 8)
            jit[np.arange(k_shared // 8), ax] = 0.5                         # exactly d^2 = 0.25 to the ref point it was copied from
            extra = c0 + np.round(rng.uniform(-ext, ext, (n_src - k_shared, 3)) * 16) / 16
        else:
            jit = rng.normal(size=(k_shared, 3)) * 0.3
            extra = c0 + rng.uniform(-ext, ext, (n_src - k_shared, 3))
        moved = np.concatenate([base + jit, extra])
        if apart:
            moved[:, 0] -= 32.0 if lattice else 60.0
        src = (moved - t) @ R                                               # R^T (x - t): exact on the lattice
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        ref, src = ref.astype(np.float32), src.astype(np.float32)
        for pts, m in ((ref, M), (src, N)):
            nodes, knn, km = _patches(rng, pts, m, K, drop, ext)
            nm = np.ones(m, np.uint8)
            if special and m >= 3:
                km[1] = 0                                                   # a node with every knn entry masked
                nm[2] = 0                                                   # a masked node (its knn masks stay set: node_mask must be honoured)
            pts_all.append(pts)
            nodes_all.append(nodes)
            knn_all.append(knn)
            km_all.append(km)
            nm_all.append(nm)
            point_off.append(point_off[-1] + len(pts))
            node_off.append(node_off[-1] + m)
        Ts.append(T.astype(np.float32))
    cat = lambda xs, shape, dt: (np.concatenate(xs) if xs else np.zeros(shape, dt)).astype(dt).reshape((-1,) + shape[1:])
    return {"P": len(sizes), "K": K, "pos_radius": pos_radius, "points": cat(pts_all, (0, 3), np.float32),
            "nodes": cat(nodes_all, (0, 3), np.float32), "knn": cat(knn_all, (0, K), np.int64), "knn_mask": cat(km_all, (0, K), np.uint8),
            "node_mask": cat(nm_all, (0,), np.uint8), "transforms": np.stack(Ts).astype(np.float32),
            "point_off": np.array(point_off, np.int64), "node_off": np.array(node_off, np.int64)}


def slice_pair(case, p):
    """Pair p of a case as a case of its own (P = 1)."""
    po, mo = case["point_off"], case["node_off"]
    a, b = po[2 * p], po[2 * p + 2]
    m0, m1 = mo[2 * p] - mo[0], mo[2 * p + 2] - mo[0]
    return {"P": 1, "K": case["K"], "pos_radius": case["pos_radius"], "points": case["points"][a:b].copy(),
            "nodes": case["nodes"][mo[2 * p]:mo[2 * p + 2]].copy(), "knn": case["knn"][m0:m1].copy(), "knn_mask": case["knn_mask"][m0:m1].copy(),
            "node_mask": case["node_mask"][m0:m1].copy(), "transforms": case["transforms"][p:p + 1].copy(),
            "point_off": po[2 * p:2 * p + 3] - a, "node_off": mo[2 * p:2 * p + 3] - mo[2 * p]}


def golden_case(gold, pos_scan, anc_scan, pos_radius=0.45):
    """The demo pair of tests/golden/matching_golden.npz (the reference's node centres, knn indices and masks) as a P = 1 case."""
    knn_p = gold["eval_pos_node_knn_indices"].astype(np.int64)
    knn_a = gold["eval_anc_node_knn_indices"].astype(np.int64)
    return {"P": 1, "K": knn_p.shape[1], "pos_radius": pos_radius,
            "points": np.concatenate([pos_scan, anc_scan]).astype(np.float32),
            "nodes": np.concatenate([gold["eval_pos_points_c"], gold["eval_anc_points_c"]]).astype(np.float32),
            "knn": np.concatenate([knn_p, knn_a]), "knn_mask": np.concatenate([knn_p != len(pos_scan), knn_a != len(anc_scan)]).astype(np.uint8),
            "node_mask": np.concatenate([gold["eval_pos_node_masks"], gold["eval_anc_node_masks"]]).astype(np.uint8),
            "transforms": gold["transform"].astype(np.float32).reshape(1, 4, 4),
            "point_off": np.array([0, len(pos_scan), len(pos_scan) + len(anc_scan)], np.int64),
            "node_off": np.array([0, len(knn_p), len(knn_p) + len(knn_a)], np.int64)}


def coordinate_margin(case):
    """m = 2 r delta + delta^2: how far the rounded d^2 of the definition can lie from the exact one at the radius, from the case's
    coordinate bound B.  One component of q' carries 3 products (each <= u B off, |R| <= 1) and 3 sums of partial results no larger than
    S = 3 B + |t| (each <= u S off); the difference p - q' is at most B + S in size and adds u (B + S).  delta = sqrt(3) times that."""
    u = 2.0 ** -24
    B = float(np.abs(case["points"][np.isfinite(case["points"]).all(1)]).max()) if len(case["points"]) else 0.0
    tmax = float(np.abs(case["transforms"][:, :3, 3]).max())
    S = 3 * B + tmax
    delta = np.sqrt(3.0) * u * (3 * B + 3 * S + (B + S))
    r = case["pos_radius"]
    return 2 * r * delta + delta * delta
