"""NumPy restatement of the range-image scan overlap of include/lcr_hip.h (lcr_range_images, lcr_scan_overlap), its plantable mistakes,
and the one builder of the inputs that tests/test_scan_overlap_gpu.py runs and tests/test_scan_overlap_cpu.py vets.

The definition, restated from the header:

  Parameters (defaults of a 64-beam sensor): H = 64, W = 900, fov_up = 3 degrees, fov_down = -25 degrees, max_range = 50, eps = 1.
  Derived angles: fu = fov_up*pi/180, fd = fov_down*pi/180, fov = |fu| + |fd|.
  Projection of one point: (x, y, z) is fp32 and promoted to fp64.  The rigid transform M is f64[3,4], applied in fp64 with every
  operation rounded, no FMA, in this order: x' = ((M00*x + M01*y) + M02*z) + M03, and likewise for y' and z'.
    d = sqrt((x'x' + y'y') + z'z');  the point is kept iff 0 < d < max_range;
    yaw = -atan2(y', x');  pitch = asin(clamp(z'/d, -1, 1));
    u = 0.5*(yaw/pi + 1)*W;  v = (1 - (pitch + |fd|)/fov)*H;
    column = floor(u) clamped to 0..W-1;  row = floor(v) clamped to 0..H-1 (points outside the vertical field of view land in the edge rows).
  Range image: a pixel holds the minimum over its points of d rounded to fp32; an empty pixel holds -1.
  lcr_range_images: M = identity (applied like any M); valid = the count of non-empty pixels.
  lcr_scan_overlap, pair (i, j) with rel = inv(T_i) T_j: cloud j is projected through rel into a scratch image, compared with images[i]:
    matches = pixels non-empty in both with |double(a) - double(b)| < eps;  valid_cur = valid[i];  valid_ref = non-empty pixels of the
    projected image.

Everything here is element-wise fp64 NumPy (transforms are never applied through `@`).  Beside images and counts every function reports
a *margin*: the smallest distance of any kept point's u or v to an integer, of any point's d to max_range, and of any compared
||a - b| - eps| to 0.  Above 1e-9 no difference of a few ulp between two libraries' atan2 / asin can move an integer."""
import functools

import numpy as np

DEFAULTS = dict(H=64, W=900, fov_up=3.0, fov_down=-25.0, max_range=50.0, eps=1.0)
IDENTITY = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])
MARGIN = 1e-9

# plantable mistakes: name -> what the wrong implementation does
MISTAKES = {
    "max_not_min": "a pixel keeps the largest depth",
    "le_not_lt": "0 <= d keeps a point at the sensor's origin (projected straight ahead at depth 0)",
    "no_clamp": "points outside the vertical field of view are dropped instead of landing in the edge rows",
    "swapped_roles": "cloud i is projected and compared with image j",
    "rel_inverted": "cloud j is projected through inv(rel)",
    "yaw_sign": "yaw = +atan2(y', x')",
    "empty_valid": "empty pixels count as valid (and as matching each other)",
    "fma_transform": "the transform's products are fused into the sums (one rounding per multiply-add)",
}


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def _two_prod(a, b):
    """a*b = p + e exactly (Dekker / Veltkamp; no overflow at these magnitudes)"""
    p = a * b
    c = 134217729.0
    t = c * a
    ah = t - (t - a)
    al = a - ah
    t = c * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _fma(a, b, c):
    """a*b + c with (all but) one rounding: the exact product's error is carried into the sum"""
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def transform(pts, M, mistake=None):
    """(x', y', z') fp64 of fp32 points through M f64[3,4], element-wise in the header's order"""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    M = np.asarray(M, dtype=np.float64)
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    out = []
    for r in range(3):
        if mistake == "fma_transform":
            out.append(_fma(M[r, 2], z, _fma(M[r, 1], y, M[r, 0] * x)) + M[r, 3])
        else:
            out.append(((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3])
    return out


def invert(M):
    """inverse of a rigid f64[3,4] as f64[3,4]"""
    T = np.eye(4)
    T[:3, :4] = M
    return np.linalg.inv(T)[:3, :4]


def project(pts, M=IDENTITY, mistake=None, **kw):
    """dict(keep bool[n], row, col int64[n], d32 f32[n], margin): the header's projection of every point"""
    p = params(**kw)
    H, W = int(p["H"]), int(p["W"])
    fu = p["fov_up"] * np.pi / 180.0
    fd = p["fov_down"] * np.pi / 180.0
    fov = abs(fu) + abs(fd)
    xt, yt, zt = transform(pts, M, mistake)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.sqrt((xt * xt + yt * yt) + zt * zt)
        keep = ((d >= 0.0) if mistake == "le_not_lt" else (d > 0.0)) & (d < p["max_range"])
        s = np.where(d > 0.0, zt / np.where(d > 0.0, d, 1.0), 0.0)
        pitch = np.arcsin(np.clip(s, -1.0, 1.0))
        yaw = np.arctan2(yt, xt)
        if mistake != "yaw_sign":
            yaw = -yaw
        u = 0.5 * (yaw / np.pi + 1.0) * W
        v = (1.0 - (pitch + abs(fd)) / fov) * H
    keep = keep & np.isfinite(u) & np.isfinite(v)
    fu_, fv_ = np.floor(np.where(keep, u, 0.0)), np.floor(np.where(keep, v, 0.0))
    if mistake == "no_clamp":
        keep = keep & (fv_ >= 0) & (fv_ <= H - 1)
    col = np.clip(fu_, 0, W - 1).astype(np.int64)
    row = np.clip(fv_, 0, H - 1).astype(np.int64)
    margin = np.inf
    if keep.any():
        margin = min(np.abs(u[keep] - np.rint(u[keep])).min(), np.abs(v[keep] - np.rint(v[keep])).min())
    fin = np.isfinite(d)
    if fin.any():
        margin = min(margin, np.abs(d[fin] - p["max_range"]).min())
    return dict(keep=keep, row=row, col=col, d32=d.astype(np.float32), margin=float(margin))


def range_image(pts, M=IDENTITY, mistake=None, **kw):
    """(image f32[H,W] with -1 in empty pixels, valid, margin)"""
    p = params(**kw)
    H, W = int(p["H"]), int(p["W"])
    pr = project(pts, M, mistake, **kw)
    k = pr["keep"]
    pix = pr["row"][k] * W + pr["col"][k]
    if mistake == "max_not_min":
        img = np.full(H * W, -np.inf, dtype=np.float32)
        np.maximum.at(img, pix, pr["d32"][k])
    else:
        img = np.full(H * W, np.inf, dtype=np.float32)
        np.minimum.at(img, pix, pr["d32"][k])
    img[~np.isfinite(img)] = -1.0
    valid = H * W if mistake == "empty_valid" else int((img != -1.0).sum())
    return img.reshape(H, W), valid, pr["margin"]


def range_images(clouds, mistake=None, **kw):
    """(images f32[B,H,W], valid i32[B], margin f64[B]) with M = identity"""
    p = params(**kw)
    out = [range_image(c, IDENTITY, mistake, **kw) for c in clouds]
    images = np.stack([o[0] for o in out]) if out else np.zeros((0, int(p["H"]), int(p["W"])), np.float32)
    return images, np.array([o[1] for o in out], dtype=np.int32), np.array([o[2] for o in out], dtype=np.float64)


def scan_overlap(clouds, pairs, rel, mistake=None, images=None, **kw):
    """dict(images, valid, image_margin f64[B], counts i32[P,3] = (matches, valid_cur, valid_ref), margin f64[P]) of the pairs (i, j) with rel f64[P,3,4]"""
    p = params(**kw)
    if images is None:
        images = range_images(clouds, mistake, **kw)
    img, valid, img_margin = images
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    rel = np.asarray(rel, dtype=np.float64).reshape(-1, 3, 4)
    counts = np.zeros((len(pairs), 3), dtype=np.int32)
    margin = np.zeros(len(pairs))
    for k, (i, j) in enumerate(pairs):
        if mistake == "swapped_roles":
            i, j = j, i
        M = invert(rel[k]) if mistake == "rel_inverted" else rel[k]
        b, vref, mb = range_image(clouds[j], M, mistake, **kw)
        a = img[i]
        both = np.ones(a.shape, bool) if mistake == "empty_valid" else (a != -1.0) & (b != -1.0)
        diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
        counts[k] = (int((both & (diff < p["eps"])).sum()), int(valid[i]), vref)
        mc = np.abs(diff[both] - p["eps"]).min() if both.any() else np.inf
        margin[k] = min(img_margin[i], mb, mc)
    return dict(images=img, valid=valid, counts=counts, margin=margin, image_margin=img_margin)


def overlap(counts, denom="current"):
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    den = c[:, 1] if denom == "current" else np.minimum(c[:, 1], c[:, 2])
    return np.where(den > 0, c[:, 0] / np.maximum(den, 1), 0.0)


# ---------------------------------------------------------------------------------------------------------------- shared GPU test inputs
def pose(x, y, yaw_deg, z=0.0, pitch_deg=0.0):
    """sensor-to-world f64[4,4]: yaw about z, then a small pitch about y"""
    a, b = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry
    T[:3, 3] = (x, y, z)
    return T


@functools.lru_cache(maxsize=None)
def world(seed=5, n_ground=14000, n_wall=7000, length=130.0):
    """A fixed world of surfaces, f64[n,3]: a ground plane 1.7 m below the sensors, two 8 m walls along a street (their tops above the
    field of view, the ground near a sensor below it) and a few pillars."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-20.0, length, n_ground), rng.uniform(-30.0, 30.0, n_ground), rng.normal(-1.7, 0.01, n_ground)], 1)
    walls = []
    for y0 in (-9.0, 11.0):
        walls.append(np.stack([rng.uniform(-20.0, length, n_wall), y0 + rng.normal(0.0, 0.02, n_wall), rng.uniform(-1.7, 6.3, n_wall)], 1))
    pillars = []
    for k in range(12):
        cx, cy = rng.uniform(-10.0, length - 10.0), rng.uniform(-7.0, 9.0)
        ang = rng.uniform(0, 2 * np.pi, 300)
        pillars.append(np.stack([cx + 0.4 * np.cos(ang), cy + 0.4 * np.sin(ang), rng.uniform(-1.7, 3.0, 300)], 1))
    return np.concatenate([g] + walls + pillars)


def view(T, max_range=50.0, keep_beyond=1.15, zbuffer=(64, 900), n=None, seed=0):
    """The world seen from pose T as an fp32 cloud in the sensor frame: cropped to keep_beyond * max_range around the sensor (so some
    points lie beyond max_range), z-buffered by the restatement itself at `zbuffer` (one point per pixel: a scan, not a transparent
    world), shuffled, and cut to n points."""
    w = world()
    Ti = np.linalg.inv(T)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    loc = np.stack([((Ti[r, 0] * x + Ti[r, 1] * y) + Ti[r, 2] * z) + Ti[r, 3] for r in range(3)], 1).astype(np.float32)
    d = np.sqrt((loc.astype(np.float64) ** 2).sum(axis=1))
    loc, d = loc[d < keep_beyond * max_range], d[d < keep_beyond * max_range]
    pr = project(loc, IDENTITY, H=zbuffer[0], W=zbuffer[1], max_range=max_range)
    pix = np.where(pr["keep"], pr["row"] * zbuffer[1] + pr["col"], -1)
    order = np.lexsort((pr["d32"], pix))
    first = np.ones(len(order), bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win = order[first & (pix[order] >= 0)]
    out = np.concatenate([loc[win], loc[~pr["keep"]]])          # the nearest point of every pixel, and the points beyond the range
    out = out[np.random.default_rng(seed).permutation(len(out))]
    return np.ascontiguousarray(out if n is None else out[:n])


def _specials(rng, max_range):
    """points at the sensor's origin, just inside / just outside / well beyond max_range"""
    dirs = rng.normal(size=(12, 3))
    dirs[:, 2] *= 0.2
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    scale = np.array([1 - 3e-6, 1 - 1e-5, 1 - 1e-4, 1 + 3e-6, 1 + 1e-5, 1 + 1e-4, 1.3, 2.0, 0.999, 1.001, 0.5, 0.9])
    return np.concatenate([np.zeros((3, 3)), dirs * (scale * max_range)[:, None]]).astype(np.float32)


def rel_of(poses, pairs):
    poses = np.asarray(poses, dtype=np.float64)
    return np.stack([(np.linalg.inv(poses[i]) @ poses[j])[:3, :4] for i, j in pairs]) if len(pairs) else np.zeros((0, 3, 4))


@functools.lru_cache(maxsize=None)
def base_clouds():
    """(clouds, poses): 10 clouds of 0, 1, 63, 64, 65, 1000 and about 5000 points seen from poses a step, a turn or a street apart"""
    rng = np.random.default_rng(21)
    poses = [pose(0, 0, 0), pose(1.5, 0.4, 10), pose(3.0, -0.5, -15, pitch_deg=1.0), pose(0.5, 0.2, 183), pose(4.0, 1.0, 5), pose(2.0, 0.0, 90),
             pose(1.0, 1.2, 45), pose(110.0, 0.0, 0), pose(0.3, -0.2, 2), pose(6.0, 0.5, -4)]
    sizes = [5000, 1000, 65, 64, 63, 1, 0, 1000, None, 2500]
    clouds = []
    for k, (T, n) in enumerate(zip(poses, sizes)):
        if n is None:                                       # only points behind the sensor, and some at its origin (le_not_lt)
            c = view(T, seed=k)
            c = np.concatenate([c[c[:, 0] < -1.0][:800], np.zeros((2, 3), np.float32)])
        else:
            c = view(T, n=n, seed=k)
            if n >= 1000:
                c = np.concatenate([c, _specials(rng, 50.0)])
                c = c[rng.permutation(len(c))]
        clouds.append(np.ascontiguousarray(c, dtype=np.float32))
    return clouds, np.stack(poses)


def _pairs70(B):
    allp = np.array([(i, j) for i in range(B) for j in range(B)], dtype=np.int64)
    rng = np.random.default_rng(3)
    must = np.array([(0, 0), (8, 8), (0, 1), (1, 0), (0, 8), (8, 0), (6, 6), (6, 0), (0, 6), (5, 5), (7, 0), (0, 7), (3, 0), (0, 9), (9, 0)])
    rest = np.array([p for p in allp[rng.permutation(len(allp))] if not (must == p).all(axis=1).any()])
    return np.concatenate([must, rest])[:70]


def _contention():
    """4096 points on one ray, in one pixel at every image size used, at depths that differ: one minimum fought over by every lane"""
    rng = np.random.default_rng(8)
    dirn = np.array([0.8, 0.55, -0.12])
    dirn /= np.linalg.norm(dirn)
    r = rng.uniform(2.0, 45.0, 4096)
    a = (dirn[None, :] * r[:, None]).astype(np.float32)
    b = (dirn[None, :] * rng.uniform(2.0, 45.0, 4096)[:, None]).astype(np.float32)
    poses = np.stack([pose(0, 0, 0), pose(0.05, 0.02, 0.3)])
    return [a, b], poses


@functools.lru_cache(maxsize=None)
def fma_case():
    """A pair on which a contracted transform changes `matches` although every margin is wide: rel is a rotation plus a translation whose
    x component is searched (to the last bit) so that the header's rounding order leaves d just below the midpoint of two neighbouring
    fp32 values and the fused order just above it; image i holds one depth a, and eps is the midpoint of (b_lo - a, b_hi - a)."""
    R = pose(0, 0, 17.0, pitch_deg=2.0)[:3, :3]
    ty, tz = 0.25, -0.1

    def d_both(q, tx):
        out = []
        for mistake in (None, "fma_transform"):
            M = np.zeros((len(tx), 3, 4))
            M[:, :, :3] = R
            M[:, 0, 3], M[:, 1, 3], M[:, 2, 3] = tx, ty, tz
            x, y, z = (np.float64(q[0, k]) for k in range(3))
            rows = []
            for r in range(3):
                if mistake:
                    rows.append(_fma(M[:, r, 2], z, _fma(M[:, r, 1], y, M[:, r, 0] * x)) + M[:, r, 3])
                else:
                    rows.append(((M[:, r, 0] * x + M[:, r, 1] * y) + M[:, r, 2] * z) + M[:, r, 3])
            out.append(np.sqrt((rows[0] * rows[0] + rows[1] * rows[1]) + rows[2] * rows[2]))
        return out

    for trial in range(400):
        q = np.array([[12.3 + 0.01 * trial, -4.5, 0.7]], np.float32)
        lo, hi = np.float64(1.0), np.float64(1.0 + 1e-4)
        f = lambda t: d_both(q, np.array([t]))[0].astype(np.float32)[0]
        flo, fhi = f(lo), f(hi)
        if flo == fhi:
            continue
        target = np.nextafter(flo, np.float32(np.inf))           # first flip above lo
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if f(mid) >= target:
                hi = mid
            else:
                lo = mid
        tx = (np.array([lo]).view(np.int64)[0] + np.arange(-300, 300)).view(np.float64)
        d0, d1 = d_both(q, tx)
        hit = np.flatnonzero(d0.astype(np.float32) != d1.astype(np.float32))
        if len(hit):
            t = tx[hit[0]]
            M = np.zeros((3, 4))
            M[:, :3] = R
            M[:, 3] = (t, ty, tz)
            b_true, b_fma = np.float32(d0[hit[0]]), np.float32(d1[hit[0]])
            xt, yt, zt = (v[0] for v in transform(q, M))
            a_pt = (np.array([[xt, yt, zt]]) * ((b_true - 0.7) / d0[hit[0]])).astype(np.float32)
            a = range_image(a_pt, H=8, W=32)[0].max()
            eps = 0.5 * ((np.float64(b_true) - np.float64(a)) + (np.float64(b_fma) - np.float64(a)))
            return dict(name="fma", clouds=[a_pt, q], pairs=np.array([[0, 1]]), rel=M[None], proj=dict(H=8, W=32, eps=float(eps)))
    raise AssertionError("no contraction-sensitive pair found")


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """Every input of tests/test_scan_overlap_gpu.py: dicts(name, clouds, pairs int64[P,2], rel f64[P,3,4], proj)"""
    clouds, poses = base_clouds()
    pairs = _pairs70(len(clouds))
    rel = rel_of(poses, pairs)
    cases = [dict(name="8x32", clouds=clouds, pairs=pairs, rel=rel, proj=dict(H=8, W=32)),
             dict(name="1x1", clouds=clouds, pairs=pairs[:24], rel=rel[:24], proj=dict(H=1, W=1)),
             dict(name="5x37", clouds=clouds, pairs=pairs, rel=rel, proj=dict(H=5, W=37)),
             dict(name="64x900", clouds=clouds, pairs=pairs[:16], rel=rel[:16], proj=dict(H=64, W=900))]
    cc, cp = _contention()
    cpairs = np.array([(0, 0), (0, 1), (1, 0), (1, 1)])
    cases.append(dict(name="contention", clouds=cc, pairs=cpairs, rel=rel_of(cp, cpairs), proj=dict(H=8, W=32)))
    cases.append(fma_case())
    return cases


@functools.lru_cache(maxsize=None)
def want(name):
    c = {c["name"]: c for c in gpu_cases()}[name]
    return scan_overlap(c["clouds"], c["pairs"], c["rel"], **c["proj"])


@functools.lru_cache(maxsize=None)
def trajectory_case():
    """A 40-frame planted trajectory at 16 x 128 with max_range = 20: frames 0..29 drive 3 m steps down the street, frames 30..39 revisit
    the places of frames 2..11 (0.3 m aside, 2 degrees off).  dict(clouds, poses, proj, exclude, revisits {i: j})"""
    proj = dict(H=16, W=128, max_range=20.0)
    poses = [pose(3.0 * k, 0.1 * np.sin(k), 1.5 * np.cos(k)) for k in range(30)]
    revisits = {}
    for m in range(10):
        poses.append(pose(3.0 * (m + 2) + 0.2, 0.1 * np.sin(m + 2) + 0.3, 1.5 * np.cos(m + 2) + 2.0))
        revisits[30 + m] = m + 2
    clouds = [view(T, max_range=20.0, zbuffer=(32, 256), n=3000, seed=100 + k) for k, T in enumerate(poses)]
    return dict(clouds=clouds, poses=np.stack(poses), proj=proj, exclude=15, revisits=revisits)
