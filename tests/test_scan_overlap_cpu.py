"""CPU: the range-image scan overlap without a GPU — the fp64 restatement (tests/scan_overlap_restatement.py) on hand-computable cases, its
planted mistakes, the condition the GPU tests rely on (every pair of every shared input has a margin of at least 1e-9, so the GPU test's
exclusion cap is never what makes it pass), the host-side pieces of lcrnet_amd.loop_gt (pair screen, labels, distance loop pairs), and the
host-only domain checks of lcr_range_images / lcr_scan_overlap (refused before anything is launched)."""
import ctypes
import os

import numpy as np
import pytest

import scan_overlap_restatement as R
from conftest import GOLDEN

EARG, ESPACE = -1, -2


# ------------------------------------------------------------------------------------------------------------------- hand-computable cases
def test_single_point_lands_in_a_known_pixel():
    # H = 4, W = 8, fov_up = 10, fov_down = -30: fov = 40 degrees, rows of 10 degrees from +10 down, columns of 45 degrees of yaw.
    kw = dict(H=4, W=8, fov_up=10.0, fov_down=-30.0, max_range=50.0)
    # (3, 4, 0): d = 5, pitch = 0 -> v = (1 - 30/40) * 4 = 1 up to rounding, so lift it a little: z = 0.5 -> pitch = 5.7 deg -> v = 0.43.
    # yaw = -atan2(4, 3) = -53.13 deg -> u = 0.5 * (1 - 0.2952) * 8 = 2.82 -> column 2.
    img, valid, _ = R.range_image(np.array([[3.0, 4.0, 0.5]], np.float32), **kw)
    d = np.float32(np.sqrt(25.25))
    assert valid == 1 and img[0, 2] == d and (img != -1).sum() == 1
    # the mirrored point (3, -4, 0.5): yaw = +53.13 deg -> u = 5.18 -> column 5; the yaw-sign mistake swaps the two
    img2, _, _ = R.range_image(np.array([[3.0, -4.0, 0.5]], np.float32), **kw)
    assert img2[0, 5] == d
    assert R.range_image(np.array([[3.0, 4.0, 0.5]], np.float32), mistake="yaw_sign", **kw)[0][0, 5] == d
    # straight down the -x axis with y = -0.0: the identity is applied like any M, so y' = +0, yaw = -pi, u = 0 -> column 0
    img3, _, _ = R.range_image(np.array([[-2.0, -0.0, -0.1]], np.float32), **kw)
    assert img3[1, 0] == np.float32(np.sqrt(4.01))
    # pitch -25 deg at d = 10: v = (1 - 5/40) * 4 = 3.5 -> row 3
    z = -10.0 * np.sin(np.deg2rad(25.0))
    x = 10.0 * np.cos(np.deg2rad(25.0))
    img4, _, _ = R.range_image(np.array([[x, 0.1, z]], np.float32), **kw)
    assert (img4[3] != -1).sum() == 1 and img4[3, 3] != -1          # yaw just below 0 -> u just below 4


def test_a_translation_moves_the_point_before_it_is_projected():
    kw = dict(H=4, W=8, fov_up=10.0, fov_down=-30.0)
    M = np.array([[0.0, -1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.0], [0.0, 0.0, 1.0, 0.5]])     # quarter turn, then (1, 2, 0.5)
    # (2, 1, 0) -> (-1 + 1, 2 + 2, 0.5) = (0, 4, 0.5): yaw = -90 deg -> u = 2 exactly on the edge, so use (2, 1.5, 0) -> (-0.5, 4, 0.5)
    img, valid, _ = R.range_image(np.array([[2.0, 1.5, 0.0]], np.float32), M, **kw)
    assert valid == 1 and img[0, 1] == np.float32(np.sqrt(0.25 + 16 + 0.25))       # yaw = -(97.1 deg) -> u = 1.84


def test_identical_clouds_with_the_identity_pose_match_everywhere():
    clouds, _ = R.base_clouds()
    for kw in (dict(H=8, W=32), dict(H=64, W=900)):
        o = R.scan_overlap([clouds[0]], [(0, 0)], R.IDENTITY[None], **kw)
        m, vc, vr = o["counts"][0]
        assert m == vc == vr == o["valid"][0] > 0.7 * min(kw["H"] * kw["W"], 5000)
        assert R.overlap(o["counts"])[0] == 1.0


def test_clouds_farther_apart_than_twice_the_range_overlap_in_nothing():
    clouds, poses = R.base_clouds()
    far = R.pose(100.001, 0.0, 30.0)                                     # 100.001 m from cloud 0's sensor: every point beyond 50 m
    crop = lambda c: c[np.sqrt((c.astype(np.float64) ** 2).sum(axis=1)) < 50.0]     # a scan's own points lie within its range
    o = R.scan_overlap([crop(clouds[0]), crop(clouds[1])], [(0, 1), (1, 0)], R.rel_of([poses[0], far], [(0, 1), (1, 0)]), H=8, W=32)
    assert o["counts"][:, 0].tolist() == [0, 0] and o["counts"][:, 2].tolist() == [0, 0] and (o["counts"][:, 1] > 0).all()
    assert R.overlap(o["counts"]).tolist() == [0.0, 0.0]


def test_points_outside_the_field_of_view_land_in_the_edge_rows():
    up = np.array([[5.0, 1.0, 5.0], [5.0, -1.0, 20.0]], np.float32)       # 44 and 76 degrees up
    down = np.array([[5.0, 1.0, -5.0], [0.5, -0.4, -1.7]], np.float32)    # 44 and 69 degrees down
    img, valid, _ = R.range_image(np.concatenate([up, down]), H=8, W=32)
    assert valid == 4 and (img[0] != -1).sum() == 2 and (img[7] != -1).sum() == 2
    assert R.range_image(np.concatenate([up, down]), mistake="no_clamp", H=8, W=32)[1] == 0


def test_the_origin_and_the_range_limit_are_excluded():
    pts = np.array([[0, 0, 0], [50, 0, 0], [30, 40, 0], [49.99, 0.3, 0.0], [50.0, 0.3, 0]], np.float32)
    pr = R.project(pts)
    assert pr["keep"].tolist() == [False, False, False, True, False]
    assert R.project(pts, mistake="le_not_lt")["keep"].tolist() == [True, False, False, True, False]


def test_overlap_ratio_and_denominators():
    from lcrnet_amd import loop_gt
    c = np.array([[30, 100, 60], [0, 0, 10], [5, 10, 0], [7, 7, 7]])
    assert loop_gt.overlap_from_counts(c).tolist() == [0.3, 0.0, 0.5, 1.0]
    assert loop_gt.overlap_from_counts(c, "min").tolist() == [0.5, 0.0, 0.0, 1.0]
    assert np.array_equal(loop_gt.overlap_from_counts(c), R.overlap(c)) and np.array_equal(loop_gt.overlap_from_counts(c, "min"), R.overlap(c, "min"))
    with pytest.raises(ValueError):
        loop_gt.overlap_from_counts(c, "max")


# ------------------------------------------------------------------------------------------------------------- the shared GPU test inputs
def _pixels(images):
    return images != -1.0


def test_every_planted_mistake_changes_an_integer_on_the_shared_inputs():
    """Integers: the counts, `valid`, and the pixel coordinates of the non-empty pixels.  The yaw sign mirrors every image about its
    middle column, current and projected alike, so by symmetry it can change no count: it shows in the pixel coordinates alone (which
    the GPU test compares with the images, bit for bit)."""
    cases = R.gpu_cases()
    for m in R.MISTAKES:
        by_count, by_pixel = [], []
        for c in cases:
            w, g = R.want(c["name"]), R.scan_overlap(c["clouds"], c["pairs"], c["rel"], mistake=m, **c["proj"])
            if not (np.array_equal(w["counts"], g["counts"]) and np.array_equal(w["valid"], g["valid"])):
                by_count.append(c["name"])
            if not np.array_equal(_pixels(w["images"]), _pixels(g["images"])):
                by_pixel.append(c["name"])
        print(m, "counts:", by_count, "pixel coordinates:", by_pixel)
        assert by_pixel if m == "yaw_sign" else by_count, m
    fma = {c["name"]: c for c in cases}["fma"]
    assert fma["proj"]["eps"] != 1.0 and R.want("fma")["margin"][0] > 1e-7           # wide margins, and still contraction shows


def test_every_pair_of_every_shared_input_has_a_margin():
    for c in R.gpu_cases():
        w = R.want(c["name"])
        print("%s: %d clouds, %d pairs, smallest margin %.3g" % (c["name"], len(c["clouds"]), len(c["pairs"]), w["margin"].min()))
        assert (w["margin"] >= R.MARGIN).all(), (c["name"], np.flatnonzero(w["margin"] < R.MARGIN))
    t = R.trajectory_case()
    pairs = _all_pairs(t)
    w = R.scan_overlap(t["clouds"], pairs, R.rel_of(t["poses"], pairs), **t["proj"])
    assert (w["margin"] >= R.MARGIN).all()


def test_shared_inputs_cover_what_the_gpu_test_is_meant_to_meet():
    clouds, _ = R.base_clouds()
    sizes = sorted(len(c) for c in clouds)
    assert sizes[:5] == [0, 1, 63, 64, 65] and 1000 <= sizes[6] <= 1100 and max(sizes) >= 5000
    big = clouds[0]
    d = np.sqrt((big.astype(np.float64) ** 2).sum(axis=1))
    assert (d == 0).sum() == 3 and ((d > 49.99) & (d < 50)).sum() >= 2 and ((d > 50) & (d < 50.01)).sum() >= 2 and (d > 55).sum() >= 2
    pairs = {tuple(p) for p in R.gpu_cases()[0]["pairs"].tolist()}
    assert len(pairs) == 70 and (0, 0) in pairs and (0, 1) in pairs and (1, 0) in pairs and any(6 in p for p in pairs)
    img = R.want("64x900")["images"]
    assert (img[0, 0] != -1).sum() > 50 and (img[0, 63] != -1).sum() > 5                  # both edge rows are used
    cont = {c["name"]: c for c in R.gpu_cases()}["contention"]
    assert len(cont["clouds"][0]) == 4096 and R.want("contention")["valid"].tolist() == [1, 1]
    assert R.want("contention")["images"][0].max() == R.project(cont["clouds"][0], H=8, W=32)["d32"].min()


# ------------------------------------------------------------------------------------------------------------------------- lcrnet_amd.loop_gt
def _all_pairs(t):
    n = len(t["clouds"])
    return np.array([(i, j) for i in range(n) for j in range(i - t["exclude"])], dtype=np.int64)


def test_candidate_pairs_drops_only_pairs_without_overlap():
    from lcrnet_amd import loop_gt
    t = R.trajectory_case()
    allp = _all_pairs(t)
    cand = loop_gt.candidate_pairs(t["poses"], exclude=t["exclude"], max_range=t["proj"]["max_range"])
    assert cand.dtype == np.int64 and cand.shape[1] == 2
    cs, as_ = {tuple(p) for p in cand.tolist()}, {tuple(p) for p in allp.tolist()}
    assert cs <= as_ and 0 < len(cs) < len(as_)
    assert [tuple(p) for p in cand.tolist()] == sorted(cs)                                   # ascending in (i, j)
    dropped = np.array(sorted(as_ - cs))
    o = R.scan_overlap(t["clouds"], dropped, R.rel_of(t["poses"], dropped), **t["proj"])
    assert not o["counts"][:, 0].any() and not o["counts"][:, 2].any()
    pos = t["poses"][:, :3, 3]
    assert all(np.linalg.norm(pos[i] - pos[j]) >= 2 * t["proj"]["max_range"] for i, j in dropped)
    assert len(loop_gt.candidate_pairs(t["poses"][:5], exclude=100)) == 0


def test_trajectory_labels_by_the_restatement_find_the_revisits():
    from lcrnet_amd import loop_gt
    t = R.trajectory_case()
    cand = loop_gt.candidate_pairs(t["poses"], exclude=t["exclude"], max_range=t["proj"]["max_range"])
    o = R.scan_overlap(t["clouds"], cand, R.rel_of(t["poses"], cand), **t["proj"])
    labels = loop_gt.loop_labels_from_overlap(len(t["clouds"]), cand, R.overlap(o["counts"]), 0.3)
    pos = t["poses"][:, :3, 3]
    for i, j in t["revisits"].items():
        assert float(j) in labels[i].tolist(), (i, j, labels[i])
    for i in range(len(labels)):
        assert all(np.linalg.norm(pos[i] - pos[int(j)]) < 2 * t["proj"]["max_range"] for j in labels[i]), i     # far frames are not labelled
    ov = dict(zip(map(tuple, cand.tolist()), R.overlap(o["counts"])))
    assert min(ov[(i, j)] for i, j in t["revisits"].items()) > 0.7        # a revisit 0.3 m aside sees the same street
    assert sum(len(l) for l in labels[:30]) == 0                          # the first pass down the street meets nothing again


def test_loop_labels_have_the_structure_of_the_committed_asset(tmp_path):
    from lcrnet_amd import evaluation, loop_gt
    asset = np.load(os.path.join(GOLDEN, "loop_gt_seq00_0.3overlap_inactive.npz"), allow_pickle=True)["arr_0"]
    pairs = np.array([(5, 1), (5, 0), (5, 3), (7, 2), (9, 4), (9, 4), (3, 0)])
    ov = np.array([0.31, 0.9, 0.3, 0.5, 0.2, 0.29, 0.30000001])
    lab = loop_gt.loop_labels_from_overlap(10, pairs, ov, 0.3)
    assert lab.dtype == asset.dtype == object and lab.shape == (10,) and asset.ndim == 1
    filled = next(a for a in asset if len(a))
    for k in range(10):
        assert isinstance(lab[k], np.ndarray) and lab[k].dtype == filled.dtype == np.float64 and lab[k].ndim == filled.ndim == 1
    assert [l.tolist() for l in lab] == [[], [], [], [0.0], [], [0.0, 1.0], [], [2.0], [], []]
    assert asset[0].dtype == lab[0].dtype and asset[0].shape == lab[0].shape == (0,)
    path = str(tmp_path / "labels.npz")
    loop_gt.save_loop_labels(path, lab)
    back = np.load(path, allow_pickle=True)["arr_0"]
    assert back.dtype == object and [b.tolist() for b in back] == [l.tolist() for l in lab]
    assert [b.tolist() for b in loop_gt.load_loop_labels(path)] == [l.tolist() for l in lab]
    # the evaluation consumes them like the asset: rows (query, candidate, distance)
    rows = np.array([[5.0, 1.0, 0.1], [7.0, 3.0, 0.2], [3.0, 0.0, 0.3]])
    assert evaluation.compute_topN(rows, back, 1) == evaluation.compute_topN(rows, lab, 1)


def figure_eight(n=400):
    s = np.linspace(0.0, 4.0 * np.pi, n, endpoint=False)
    poses = []
    for a in s:
        T = R.pose(30.0 * np.sin(a), 15.0 * np.sin(2.0 * a), np.rad2deg(np.arctan2(30.0 * np.cos(2 * a), 30.0 * np.cos(a))), z=0.01 * np.cos(3 * a))
        poses.append(T)
    return np.stack(poses)


def test_loop_pairs_by_distance_equal_a_brute_force_loop_and_round_trip(tmp_path):
    from lcrnet_amd import io_formats, loop_gt
    poses = figure_eight()
    data = loop_gt.loop_pairs_by_distance(poses, dis=4.0, start=100, gap=50, seq=7)
    t32 = poses[:, :3, 3].astype(np.float32)
    want = {}
    for i in range(100, len(poses)):
        for j in range(0, i - 50 + 1):
            dx, dy, dz = (np.float32(t32[j, k] - t32[i, k]) for k in range(3))
            if np.float32(np.float32(dx * dx + dy * dy) + dz * dz) < np.float32(16.0):
                want.setdefault(i, []).append(j)
    assert len(want) > 20 and [d["anc_idx"] for d in data] == sorted(want)
    for d in data:
        i = d["anc_idx"]
        assert d["seq_id"] == 7 and d["pos_idx"].tolist() == want[i] and d["pose"].shape == (len(want[i]), 4, 4)
        for k, j in enumerate(want[i]):
            assert np.array_equal(d["pose"][k], np.linalg.inv(poses[j]) @ poses[i])
    assert any(len(v) > 1 for v in want.values())
    assert min(i - max(v) for i, v in want.items()) >= 50
    path = str(tmp_path / "07.npz")
    loop_gt.save_loop_pairs(path, data)
    back = np.load(path, allow_pickle=True)["data"]
    assert len(back) == len(data) and back[0]["anc_idx"] == data[0]["anc_idx"] and np.array_equal(back[3]["pose"], data[3]["pose"])
    assert io_formats.load_loop_pairs(path) == [(j, i) for i in sorted(want) for j in want[i]]
    assert loop_gt.loop_pairs_by_distance(poses[:120], dis=0.01) == []


# ------------------------------------------------------------------------------------------------------------- host-only argument checks
def test_ws_bytes_helpers_and_their_domain():
    from lcrnet_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    assert L.lcr_range_images_ws_bytes(64, ctypes.byref(nb)) == 0 and nb.value >= 65 * 8
    assert L.lcr_scan_overlap_ws_bytes(64, 1 << 20, ctypes.byref(nb)) == 0 and nb.value >= 65 * 8
    assert L.lcr_scan_overlap_ws_bytes(1, 0, ctypes.byref(nb)) == 0
    for B in (0, 65, -1):
        assert L.lcr_range_images_ws_bytes(B, ctypes.byref(nb)) == EARG and b"lcr_range_images_ws_bytes" in L.lcr_last_error()
        assert L.lcr_scan_overlap_ws_bytes(B, 1, ctypes.byref(nb)) == EARG and b"lcr_scan_overlap_ws_bytes" in L.lcr_last_error()
    assert L.lcr_scan_overlap_ws_bytes(1, -1, ctypes.byref(nb)) == EARG and L.lcr_scan_overlap_ws_bytes(1, 2**31, ctypes.byref(nb)) == EARG
    assert L.lcr_range_images_ws_bytes(1, None) == EARG and L.lcr_scan_overlap_ws_bytes(1, 1, None) == EARG


PROJ_VIOLATIONS = (dict(B=0), dict(B=65), dict(H=0), dict(H=129), dict(W=0), dict(W=4097), dict(max_range=0.0), dict(max_range=-1.0),
                   dict(max_range=float("nan")), dict(fov_up=0.0, fov_down=0.0), dict(fov_up=float("nan")), dict(fov_down=float("inf")),
                   dict(lens=(-1,)), dict(lens=(2**31,)), dict(B=2, lens=(2**31 - 1, 1)), dict(pts=None), dict(ws=None))


def test_range_images_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)                                        # never dereferenced: the checks come first

    def call(B=1, lens=(10,), H=64, W=900, fov_up=3.0, fov_down=-25.0, max_range=50.0, pts=fake, images=fake, valid=fake, ws=fake,
             ws_bytes=1 << 20):
        ln = np.asarray(list(lens) + [0] * 64, np.int64)
        return L.lcr_range_images(pts, ln.ctypes.data, B, H, W, fov_up, fov_down, max_range, images, valid, ws, ws_bytes, None)

    for kw in PROJ_VIOLATIONS + (dict(images=None), dict(valid=None)):
        assert call(**kw) == EARG, kw
        assert b"lcr_range_images" in L.lcr_last_error()
    assert call(ws_bytes=8) == ESPACE


def test_scan_overlap_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)

    def call(B=1, lens=(10,), P=3, H=64, W=900, fov_up=3.0, fov_down=-25.0, max_range=50.0, eps=1.0, pts=fake, images=fake, valid=fake,
             pairs=fake, rel=fake, counts=fake, status=fake, ws=fake, ws_bytes=1 << 20):
        ln = np.asarray(list(lens) + [0] * 64, np.int64)
        return L.lcr_scan_overlap(pts, ln.ctypes.data, B, images, valid, pairs, rel, P, H, W, fov_up, fov_down, max_range, eps, counts, status,
                                  ws, ws_bytes, None)

    extra = (dict(P=-1), dict(P=2**31), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(images=None), dict(valid=None),
             dict(pairs=None), dict(rel=None), dict(counts=None), dict(status=None))
    for kw in PROJ_VIOLATIONS + extra:
        assert call(**kw) == EARG, kw
        assert b"lcr_scan_overlap" in L.lcr_last_error()
    assert call(ws_bytes=8) == ESPACE
    assert call(P=0, B=0, H=0, pts=None, ws=None) == 0                    # P == 0 returns first
