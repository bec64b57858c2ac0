"""GPU: range images and range-image scan overlaps (csrc/scan_overlap.hip, lcr_range_images / lcr_scan_overlap) against the fp64
restatement of tests/scan_overlap_restatement.py, bit for bit: images, `valid` and all three counts.

The definition both sides implement (include/lcr_hip.h): a point (x, y, z), fp32 promoted to fp64, goes through M f64[3,4] as
x' = ((M00*x + M01*y) + M02*z) + M03 (every operation rounded, no FMA); d = sqrt((x'x' + y'y') + z'z'); kept iff 0 < d < max_range;
yaw = -atan2(y', x'), pitch = asin(clamp(z'/d, -1, 1)); u = 0.5*(yaw/pi + 1)*W, v = (1 - (pitch + |fd|)/fov)*H; column / row = floor
clamped into the image; a pixel holds the minimum d rounded to fp32, an empty pixel -1; matches = pixels non-empty in both images with
|double(a) - double(b)| < eps, valid_cur = valid[i], valid_ref = non-empty pixels of the projected image.

A pair may be left out of a comparison only if its margin (the restatement's: distance of u, v to an integer, of d to max_range, of
||a - b| - eps| to 0) is below 1e-9, and at most 1 % of a case's pairs may be; tests/test_scan_overlap_cpu.py shows that the shared inputs
leave out none."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import scan_overlap_restatement as R

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in R.gpu_cases()]


def case(name):
    return {c["name"]: c for c in R.gpu_cases()}[name]


def stack(clouds):
    pts = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3), np.float32)
    return torch.from_numpy(np.ascontiguousarray(pts)).cuda(), [len(c) for c in clouds]


def split(proj):
    img = {k: v for k, v in proj.items() if k != "eps"}
    return img, proj.get("eps", 1.0)


def run(clouds, pairs, rel, proj):
    """one lcr_range_images and one lcr_scan_overlap call -> dict of numpy arrays (images, valid, counts, status)"""
    from lcrnet_amd import functional as F
    pts, ln = stack(clouds)
    ip, eps = split(proj)
    images, valid = F.range_images(pts, ln, **ip)
    pr = torch.from_numpy(np.asarray(pairs, np.int32).reshape(-1, 2)).cuda()
    rl = torch.from_numpy(np.ascontiguousarray(np.asarray(rel, np.float64).reshape(-1, 3, 4))).cuda()
    counts, status = F.scan_overlap(pts, ln, images, valid, pr, rl, eps=eps, **ip)
    torch.cuda.synchronize()
    return dict(images=images.cpu().numpy(), valid=valid.cpu().numpy(), counts=counts.cpu().numpy(), status=int(status.cpu()[0]))


@functools.lru_cache(maxsize=None)
def got(name):
    c = case(name)
    return run(c["clouds"], c["pairs"], c["rel"], c["proj"])


@pytest.mark.parametrize("name", CASES)
def test_images_valid_and_counts_equal_the_restatement_bit_for_bit(name):
    c, w, g = case(name), R.want(name), got(name)
    assert g["status"] == 0
    ok_img = w["image_margin"] >= R.MARGIN
    ok = w["margin"] >= R.MARGIN
    print("%s: %d clouds, %d pairs; left out for a margin below 1e-9: %d clouds, %d pairs" % (name, len(ok_img), len(ok), (~ok_img).sum(),
                                                                                           (~ok).sum()))
    assert (~ok).sum() <= 0.01 * len(ok) and (~ok_img).sum() <= 0.01 * len(ok_img)
    assert g["images"].dtype == np.float32 and g["images"].shape == w["images"].shape
    assert np.array_equal(g["images"][ok_img].view(np.uint32), w["images"][ok_img].view(np.uint32))
    assert np.array_equal(g["valid"][ok_img], w["valid"][ok_img])
    assert np.array_equal(g["counts"][ok], w["counts"][ok]), np.flatnonzero((g["counts"] != w["counts"]).any(axis=1) & ok)[:5]
    if name == "64x900":
        assert c["proj"]["H"] * c["proj"]["W"] * 4 > 160 * 1024           # more than one band of rows in LDS


def test_no_pair_one_pair_and_each_pair_alone_give_the_batch_bytes():
    """P = 0 and P = 1, and batch invariance: every pair of the 70, run alone, gives the bytes it has in the batch; so do a few at 64 x 900."""
    from lcrnet_amd import functional as F
    for name, take in (("8x32", range(70)), ("64x900", (0, 2, 7))):
        c, g = case(name), got(name)
        pts, ln = stack(c["clouds"])
        ip, eps = split(c["proj"])
        images, valid = F.range_images(pts, ln, **ip)
        pr = torch.from_numpy(c["pairs"].astype(np.int32)).cuda()
        rl = torch.from_numpy(np.ascontiguousarray(c["rel"])).cuda()
        outs = [F.scan_overlap(pts, ln, images, valid, pr[k:k + 1], rl[k:k + 1], eps=eps, **ip) for k in take]
        torch.cuda.synchronize()
        for k, (cnt, status) in zip(take, outs):
            assert int(status.cpu()[0]) == 0 and np.array_equal(cnt.cpu().numpy()[0], g["counts"][k]), (name, k)
        cnt, status = F.scan_overlap(pts, ln, images, valid, pr[:0], rl[:0], eps=eps, **ip)
        assert tuple(cnt.shape) == (0, 3) and int(status.cpu()[0]) == 0
        # the same pairs in another order and the clouds at other positions of the batch
        perm = np.random.default_rng(1).permutation(len(c["clouds"]))
        inv = np.argsort(perm)
        sub = np.asarray(list(take))[::-1]
        h = run([c["clouds"][j] for j in perm], inv[c["pairs"][sub]], c["rel"][sub], c["proj"])
        assert np.array_equal(h["counts"], g["counts"][sub]) and np.array_equal(h["images"][inv].view(np.uint32), g["images"].view(np.uint32))


def test_pair_index_out_of_range_is_reported_and_reads_nothing():
    c, g = case("8x32"), got("8x32")
    B = len(c["clouds"])
    pairs = c["pairs"][:6].copy()
    pairs[1] = (B, 0)
    pairs[3] = (0, -1)
    pairs[4] = (2**30, 2**30)
    h = run(c["clouds"], pairs, c["rel"][:6], c["proj"])
    assert h["status"] == 5                                             # the largest refused p, plus one
    assert (h["counts"][[1, 3, 4]] == -1).all() and np.array_equal(h["counts"][[0, 2, 5]], g["counts"][[0, 2, 5]])


def test_nan_workspace_and_canaries_around_every_output():
    from lcrnet_amd import _lib
    L = _lib.lib()
    for name in ("5x37", "64x900"):
        c, g = case(name), got(name)
        H, W = c["proj"]["H"], c["proj"]["W"]
        pts, ln = stack(c["clouds"])
        ln = np.asarray(ln, np.int64)
        B, P = len(ln), len(c["pairs"])
        nb = ctypes.c_size_t(0)
        assert L.lcr_range_images_ws_bytes(B, ctypes.byref(nb)) == 0 and nb.value % 4 == 0
        ws = torch.empty(nb.value + 4096, dtype=torch.uint8, device="cuda")
        ws[:nb.value].view(torch.float32).fill_(float("nan"))
        ws[nb.value:].fill_(0xA5)
        images = torch.full(((B + 2) * H * W,), -7.0, dtype=torch.float32, device="cuda")
        valid = torch.full((B + 66,), -7, dtype=torch.int32, device="cuda")
        sp = _lib.stream_ptr(pts.device)
        img_p, val_p = ctypes.c_void_p(images.data_ptr() + 4 * H * W), ctypes.c_void_p(valid.data_ptr() + 33 * 4)
        assert L.lcr_range_images(_lib.ptr(pts), ln.ctypes.data, B, H, W, 3.0, -25.0, 50.0, img_p, val_p, _lib.ptr(ws), nb.value, sp) == 0
        torch.cuda.synchronize()
        assert bool((ws[nb.value:] == 0xA5).all())
        assert bool((images[:H * W] == -7.0).all()) and bool((images[(B + 1) * H * W:] == -7.0).all())
        assert bool((valid[:33] == -7).all()) and bool((valid[33 + B:] == -7).all())
        assert np.array_equal(images[H * W:(B + 1) * H * W].cpu().numpy().view(np.uint32), g["images"].reshape(-1).view(np.uint32))
        assert np.array_equal(valid[33:33 + B].cpu().numpy(), g["valid"])
        assert L.lcr_range_images(_lib.ptr(pts), ln.ctypes.data, B, H, W, 3.0, -25.0, 50.0, img_p, val_p, _lib.ptr(ws), nb.value - 1, sp) == -2
        # the overlaps, on the images just written
        assert L.lcr_scan_overlap_ws_bytes(B, P, ctypes.byref(nb)) == 0 and nb.value % 4 == 0
        ws = torch.empty(nb.value + 4096, dtype=torch.uint8, device="cuda")
        ws[:nb.value].view(torch.float32).fill_(float("nan"))
        ws[nb.value:].fill_(0xA5)
        counts = torch.full((P + 2, 3), -7, dtype=torch.int32, device="cuda")
        status = torch.full((65,), -7, dtype=torch.int32, device="cuda")
        pr = torch.from_numpy(c["pairs"].astype(np.int32)).cuda()
        rl = torch.from_numpy(np.ascontiguousarray(c["rel"])).cuda()
        args = (_lib.ptr(pts), ln.ctypes.data, B, img_p, val_p, _lib.ptr(pr), _lib.ptr(rl), P, H, W, 3.0, -25.0, 50.0, c["proj"].get("eps", 1.0),
                ctypes.c_void_p(counts.data_ptr() + 12), ctypes.c_void_p(status.data_ptr() + 32 * 4), _lib.ptr(ws))
        assert L.lcr_scan_overlap(*args, nb.value, sp) == 0
        torch.cuda.synchronize()
        assert bool((ws[nb.value:] == 0xA5).all())
        assert bool((counts[0] == -7).all()) and bool((counts[-1] == -7).all())
        assert bool((status[:32] == -7).all()) and bool((status[33:] == -7).all()) and int(status[32]) == 0
        assert np.array_equal(counts[1:-1].cpu().numpy(), g["counts"])
        assert L.lcr_scan_overlap(*args, nb.value - 1, sp) == -2


def test_scan_overlaps_api_blocks_of_frames_and_denominators():
    """lcrnet_amd.loop_gt.scan_overlaps on 70 frames (three blocks of 32: a call holds the two blocks a pair touches), from host and from
    device points, against the restatement; both denominators."""
    from lcrnet_amd import loop_gt
    clouds, poses = R.base_clouds()
    small = [c for c in clouds if len(c) <= 1100]
    many = [small[k % len(small)] for k in range(70)]
    mposes = np.stack([poses[[i for i, c in enumerate(clouds) if len(c) <= 1100][k % len(small)]] for k in range(70)])
    rng = np.random.default_rng(4)
    pairs = np.concatenate([rng.integers(0, 70, (60, 2)), [(69, 0), (0, 69), (33, 33), (64, 31), (31, 64)]])
    proj = dict(H=8, W=32)
    w = R.scan_overlap(many, pairs, R.rel_of(mposes, pairs), **proj)
    assert (w["margin"] >= R.MARGIN).all()
    ov, counts = loop_gt.scan_overlaps(np.concatenate(many), [len(c) for c in many], mposes, pairs, **proj)
    assert ov.dtype == np.float64 and counts.dtype == np.int32 and np.array_equal(counts, w["counts"])
    assert np.array_equal(ov, R.overlap(w["counts"]))
    ov2, counts2 = loop_gt.scan_overlaps(torch.from_numpy(np.concatenate(many)).cuda(), [len(c) for c in many], mposes, pairs, denom="min", **proj)
    assert np.array_equal(counts2, counts) and np.array_equal(ov2, R.overlap(w["counts"], "min"))
    ov0, counts0 = loop_gt.scan_overlaps(np.concatenate(many), [len(c) for c in many], mposes, np.zeros((0, 2), np.int64), **proj)
    assert ov0.shape == (0,) and counts0.shape == (0, 3)
    with pytest.raises(ValueError):
        loop_gt.scan_overlaps(np.concatenate(many), [len(c) for c in many], mposes, [(0, 70)], **proj)
    with pytest.raises(TypeError):
        loop_gt.scan_overlaps(np.concatenate(many), [len(c) for c in many], mposes, pairs, rows=8)


def test_trajectory_labels_end_to_end_equal_the_restatement():
    """40 planted frames at 16 x 128: candidate_pairs -> scan_overlaps -> loop_labels_from_overlap on the GPU gives the restatement's labels;
    the revisits are labelled, frames farther than twice the range are not."""
    from lcrnet_amd import loop_gt
    t = R.trajectory_case()
    n = len(t["clouds"])
    cand = loop_gt.candidate_pairs(t["poses"], exclude=t["exclude"], max_range=t["proj"]["max_range"])
    w = R.scan_overlap(t["clouds"], cand, R.rel_of(t["poses"], cand), **t["proj"])
    want = loop_gt.loop_labels_from_overlap(n, cand, R.overlap(w["counts"]), 0.3)
    ov, counts = loop_gt.scan_overlaps(np.concatenate(t["clouds"]), [len(c) for c in t["clouds"]], t["poses"], cand, **t["proj"])
    assert np.array_equal(counts, w["counts"])
    labels = loop_gt.loop_labels_from_overlap(n, cand, ov, 0.3)
    assert [l.tolist() for l in labels] == [l.tolist() for l in want]
    pos = t["poses"][:, :3, 3]
    for i, j in t["revisits"].items():
        assert float(j) in labels[i].tolist()
    for i in range(n):
        assert all(np.linalg.norm(pos[i] - pos[int(j)]) < 2 * t["proj"]["max_range"] for j in labels[i])
    assert sum(len(l) for l in labels[:30]) == 0 and sum(len(l) for l in labels[30:]) >= 10


def test_loop_gt_tool_writes_labels_and_loop_pairs_of_a_sequence_on_disk(tmp_path, capsys):
    """tools/loop_gt_run.py --poses --calib --scans on the planted trajectory written as KITTI files (camera-frame pose lines, a calib Tr,
    velodyne .bin scans), run in this process: the labels equal the ones computed from the arrays, the loop pairs read back."""
    import importlib.util
    import json
    from lcrnet_amd import io_formats, loop_gt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("loop_gt_run_tool", os.path.join(root, "tools", "loop_gt_run.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    t = R.trajectory_case()
    Tr = np.eye(4)
    Tr[:3, :3] = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])          # velodyne axes to camera axes
    Tr[:3, 3] = (0.0, -0.1, -0.3)
    scans = tmp_path / "velodyne"
    scans.mkdir()
    with open(tmp_path / "poses.txt", "w") as f:
        for k, (c, T) in enumerate(zip(t["clouds"], t["poses"])):
            np.concatenate([c, np.zeros((len(c), 1), np.float32)], axis=1).astype(np.float32).tofile(str(scans / ("%06d.bin" % k)))
            f.write(" ".join(repr(float(v)) for v in (Tr @ T @ np.linalg.inv(Tr))[:3].reshape(-1)) + "\n")
    with open(tmp_path / "calib.txt", "w") as f:
        f.write("P0: 1 0 0 0 0 1 0 0 0 0 1 0\nTr: " + " ".join(repr(float(v)) for v in Tr[:3].reshape(-1)) + "\n")
    out = tool.main(["--poses", str(tmp_path / "poses.txt"), "--calib", str(tmp_path / "calib.txt"), "--scans", str(scans), "--out", str(tmp_path),
                     "--exclude", str(t["exclude"]), "--H", "16", "--W", "128", "--max-range", "20", "--loop-start", "30", "--loop-gap", "15",
                     "--loop-dis", "1.0"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == 40 and line["labelled_frames"] >= 10 and os.path.exists(line["labels_file"]) and os.path.exists(line["loop_pairs_file"])
    labels = loop_gt.load_loop_labels(line["labels_file"])
    assert labels.shape == (40,) and all(float(j) in labels[i].tolist() for i, j in t["revisits"].items())
    # the poses went through text and two changes of frame: the counts may differ from the array run by a pixel, the revisits may not
    pairs = io_formats.load_loop_pairs(line["loop_pairs_file"])
    assert sorted(pairs) == sorted((j, i) for i, j in t["revisits"].items()) and out["pairs"] == line["pairs"]
