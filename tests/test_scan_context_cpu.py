"""CPU: the Scan Context restatement (tests/scan_context_restatement.py) against cases whose answer is known in closed form, the margins of
every input the GPU tests share, the planted-revisit sequence of the end-to-end test, and the host-only argument checks of
lcr_scan_context / lcr_scan_context_distance / lcr_scan_context_topk (refused before anything is launched)."""
import ctypes
import inspect

import numpy as np
import pytest

import scan_context_restatement as R
from scan_context_restatement import mask_bits

EARG, ESPACE = -1, -2
FAKE = ctypes.c_void_p(256)
BIG = 1 << 40


def test_a_cloud_of_bin_centres_gives_the_expected_image():
    Rn, W, L, h = 4, 6, 12.0, 2.0
    rng = np.random.default_rng(0)
    z = rng.uniform(-1.0, 3.0, (Rn, W)).astype(np.float32)
    z[1, 2] = -5.0                                                   # below -lidar_height: stays negative
    pts, skip = [], {(0, 0), (3, 4)}
    for i in range(Rn):
        for j in range(W):
            if (i, j) in skip:
                continue
            r, th = (i + 0.5) * L / Rn, (j + 0.5) * 2 * np.pi / W
            pts.append((r * np.cos(th), r * np.sin(th), z[i, j]))
            pts.append((r * np.cos(th), r * np.sin(th), z[i, j] - 1.0))          # a lower point of the same bin loses
    pts.append((L * 1.01, 0.3, 50.0))                                # beyond max_length
    pts.append((0.0, 0.0, 7.0))                                      # the origin goes to (0, 0)
    d = R.descriptor(np.asarray(pts, np.float32), Rn, W, L, h)
    want = (z + np.float32(h)).astype(np.float32)
    want[0, 0], want[3, 4] = 9.0, 0.0
    assert d.dtype == np.float32 and np.array_equal(d, want) and d[1, 2] == -3.0
    key, unit, mask = R.derive(d)
    assert mask == (1 << W) - 1 and np.allclose((unit.astype(np.float64) ** 2).sum(0), 1.0, atol=1e-6)
    assert np.allclose(key, d.astype(np.float64).mean(1), atol=1e-6)
    # a rotation of the cloud by 2 sectors about +z moves the image by 2 columns: shift(a, b) = 2, and Rz(-shift * 2 pi / W) undoes it
    a = 2 * 2 * np.pi / W
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    p = np.asarray(pts[:-2], np.float64)
    db = R.derive(R.descriptor((p @ Rz.T).astype(np.float32), Rn, W, L, h))
    da = R.derive(R.descriptor(p.astype(np.float32), Rn, W, L, h))
    dist, shift, _ = R.distance(da[1], da[2], db[1], db[2])
    assert shift == 2 and abs(dist) < 1e-6


@pytest.mark.parametrize("shape", R.DISTANCE_SHAPES)
def test_rolled_copies_symmetry_and_exact_ties(shape):
    c = R.distance_case(*shape)
    W, u, m = shape[1], c["unit"], c["mask"]
    for (a, b), s in c["rolls"].items():
        assert abs(R.shift_distances(u[a], m[a], u[b], m[b])[s]) < 1e-6           # fp32 units: a column's self product is 1 within 1e-7
        d64 = c["desc"][a].astype(np.float64)
        exact = d64 / np.where(mask_bits(m[a], W), np.sqrt((d64 ** 2).sum(0)), 1.0)        # normalised in fp64
        dist, shift, _ = R.distance(exact, m[a], np.roll(exact, s, 1), m[b])
        assert abs(dist) < 1e-12 and (shift == s or W == 1)
    for a, b in c["pairs"][:30]:
        d_ab, d_ba = R.shift_distances(u[a], m[a], u[b], m[b]), R.shift_distances(u[b], m[b], u[a], m[a])
        assert np.abs(d_ab - d_ba[(W - np.arange(W)) % W]).max() < 1e-14   # d_s(a, b) = d_{(W - s) mod W}(b, a), up to the order of an fp64 sum
    # one-hot columns: integer sums, and the smallest of the tied shifts wins
    d = R.shift_distances(u[7], m[7], u[8], m[8])
    assert set(np.unique(d)) <= {0.0, 1.0}
    period = c["period"]
    assert R.distance(u[7], m[7], u[8], m[8])[:2] == (0.0, 1 % period) and R.distance(u[8], m[8], u[7], m[7])[:2] == (0.0, (period - 1) % period)
    assert R.distance(u[7], m[7], u[7], m[7])[:2] == (0.0, 0)
    assert np.array_equal(R.shift_distances32(u[7], m[7], u[8], m[8]).astype(np.float64), d)
    # the empty cloud: c(s) = 0 everywhere
    assert R.distance(u[0], m[0], u[3], m[3])[:2] == (1.0, 0) and R.distance(u[0], m[0], u[0], m[0])[:2] == (1.0, 0)
    # the fp32 form stays close to the fp64 form: R + W roundings of 2^-24 on terms <= 1, averaged over c(s) columns (measured <= 1.4e-7)
    assert max(R.e_ref(u[a], m[a], u[b], m[b]) for a, b in c["pairs"]) < (shape[0] + shape[1]) * 2.0 ** -24


def test_every_shared_cloud_has_its_margin():
    n = 0
    for c in R.gpu_cases():
        w = R.want(c["name"])
        assert (w["margin"] >= R.MARGIN).all(), (c["name"], w["margin"].min())
        n += len(c["clouds"])
    assert n >= 80
    w = R.want("below")
    assert (w["desc"][0] <= 0).all() and (w["desc"][0] < 0).sum() > 100          # negative bins are kept
    w = R.want("nonfinite")
    assert np.isfinite(w["desc"]).all() and (w["desc"][1] == 0).all() and w["mask"][1] == 0
    w = R.want("box200")
    assert all((np.hypot(c[:, 0], c[:, 1]) > 80.0).sum() > 10 for c in R.gpu_cases()[1]["clouds"])
    assert len(R.gpu_cases()[2]["clouds"][1]) > 2 * 4096                          # more than one workgroup's chunk of points
    assert (R.planted_want()["sc"]["margin"] >= R.MARGIN).all()


def test_planted_mistakes_are_seen():
    c = R.distance_case(20, 60)
    u, m = c["unit"], c["mask"]
    tol = 2.0 ** -20
    for mistake in ("shift_reversed", "divide_by_W", "mask_not_rotated"):
        worst = max(abs(R.distance(u[a], m[a], u[b], m[b], mistake)[0] - R.distance(u[a], m[a], u[b], m[b])[0]) +
                    (R.distance(u[a], m[a], u[b], m[b], mistake)[1] != R.distance(u[a], m[a], u[b], m[b])[1]) for a, b in c["pairs"])
        assert worst >= 100 * tol, mistake
    cl = R.gpu_cases()[1]
    for mistake in ("sector_xy", "empty_-1000"):
        d0, d1 = R.descriptor(cl["clouds"][0], **cl["params"]), R.descriptor(cl["clouds"][0], mistake=mistake, **cl["params"])
        assert np.abs(d0 - d1).max() >= 1.0, mistake                # against a bit-for-bit comparison


def test_the_planted_sequence_finds_every_twin_at_rank_one():
    w = R.planted_want()
    assert np.array_equal(w["top1"], np.arange(R.N_SCENES - 1))
    assert (w["gap"] >= 1e-5).all() and (w["second"] - w["dist"] > 0.05).all()
    # the twin of frame j is frame j + 12 turned by phi = 37 + 6 (j + 12) degrees; as query a against b = frame j, b is a turned by -phi
    phi = 37.0 + 6.0 * np.arange(R.N_SCENES, 2 * R.N_SCENES - 1)
    assert np.array_equal(w["shift"], np.round(-phi / 6.0).astype(int) % 60)


def test_topk_rows_sorts_by_distance_then_index():
    d = np.asarray([[0.5, 0.2, 0.2, 0.9, 0.1]])
    assert R.topk_rows(d, 4, 1, 5, 3, 0).tolist() == [[1, 2, 0]] and R.topk_rows(d, 2, 1, 5, 3, 1).tolist() == [[0, -1, -1]]


def test_argument_refusals_without_a_launch():
    from lcrnet_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    ln = np.asarray([5, 0, 7], np.int64)

    def sc(B=3, Rn=20, W=60, max_length=80.0, h=2.0, lengths=ln, ws_bytes=BIG, out=FAKE):
        return L.lcr_scan_context(FAKE, lengths.ctypes.data if lengths is not None else None, B, Rn, W, max_length, h, out, FAKE, FAKE, FAKE, FAKE,
                                  ws_bytes, None)

    bad = [dict(B=0), dict(B=65), dict(Rn=0), dict(Rn=33), dict(W=0), dict(W=65), dict(max_length=0.0), dict(max_length=float("inf")),
           dict(max_length=float("nan")), dict(h=float("nan")), dict(h=float("inf")), dict(lengths=None), dict(lengths=np.asarray([1, -1, 2], np.int64)),
           dict(lengths=np.asarray([2**31 - 1, 1, 0], np.int64)), dict(out=None)]
    for kw in bad:
        assert sc(**kw) == EARG and L.lcr_last_error().startswith(b"lcr_scan_context:"), kw
    assert L.lcr_scan_context_ws_bytes(3, 20, 60, ctypes.byref(nb)) == 0 and nb.value >= 3 * 20 * 60 * 4
    assert sc(ws_bytes=nb.value - 1) == ESPACE and L.lcr_last_error().startswith(b"lcr_scan_context:")
    for args in ((0, 20, 60), (65, 20, 60), (1, 0, 60), (1, 33, 60), (1, 20, 0), (1, 20, 65)):
        assert L.lcr_scan_context_ws_bytes(*args, ctypes.byref(nb)) == EARG and L.lcr_last_error().startswith(b"lcr_scan_context_ws_bytes:")
    assert L.lcr_scan_context_ws_bytes(1, 20, 60, None) == EARG

    def dist(B=12, Rn=20, W=60, P=5, out=FAKE):
        return L.lcr_scan_context_distance(FAKE, FAKE, B, Rn, W, FAKE, P, out, FAKE, FAKE, None, 0, None)

    for kw in (dict(B=0), dict(B=2**31), dict(Rn=0), dict(Rn=33), dict(W=0), dict(W=65), dict(P=-1), dict(P=2**31), dict(out=None)):
        assert dist(**kw) == EARG and L.lcr_last_error().startswith(b"lcr_scan_context_distance:"), kw
    assert dist(P=0) == 0 and dist(P=0, out=None) == 0                        # P == 0 is legal once B, R, W are in the domain
    assert dist(P=0, B=0) == EARG and dist(P=0, W=65) == EARG
    assert L.lcr_scan_context_distance_ws_bytes(12, 20, 60, 0, ctypes.byref(nb)) == 0 and nb.value == 0
    assert L.lcr_scan_context_distance_ws_bytes(0, 20, 60, 0, ctypes.byref(nb)) == EARG
    assert L.lcr_last_error().startswith(b"lcr_scan_context_distance_ws_bytes:")

    def topk(C=300, Rn=20, W=60, Q=70, q0=230, k=50, exclude=100, ws_bytes=BIG, out=FAKE):
        return L.lcr_scan_context_topk(FAKE, FAKE, C, Rn, W, Q, q0, k, exclude, out, FAKE, FAKE, FAKE, ws_bytes, None)

    for kw in (dict(C=0), dict(C=2**31), dict(Rn=0), dict(Rn=33), dict(W=0), dict(W=65), dict(Q=-1), dict(q0=-1), dict(q0=231), dict(Q=71), dict(k=0),
               dict(k=129), dict(exclude=-1), dict(out=None)):
        assert topk(**kw) == EARG and L.lcr_last_error().startswith(b"lcr_scan_context_topk:"), kw
    assert topk(Q=0) == 0 and topk(Q=0, C=0) == EARG
    assert L.lcr_scan_context_topk_ws_bytes(70, 230, 300, 100, ctypes.byref(nb)) == 0 and nb.value >= 8 * 70 * 199
    assert topk(ws_bytes=nb.value - 1) == ESPACE and L.lcr_last_error().startswith(b"lcr_scan_context_topk:")
    assert L.lcr_scan_context_topk_ws_bytes(70, 231, 300, 100, ctypes.byref(nb)) == EARG
    assert L.lcr_last_error().startswith(b"lcr_scan_context_topk_ws_bytes:")
    assert L.lcr_scan_context_topk_ws_bytes(70, 230, 300, 100, None) == EARG


def test_python_surface():
    from lcrnet_amd import functional as F, loop_closure, scan_context
    p = inspect.signature(loop_closure.run).parameters
    assert p["detector"].default == "descriptor" and list(p)[:5] == ["desc_model", "pair_model", "raw_frames", "thres", "out_dir"]
    assert list(inspect.signature(scan_context.detect_loops).parameters)[:5] == ["sc", "thres", "k", "exclude", "start"]
    assert list(inspect.signature(scan_context.scan_context_topk).parameters) == ["sc", "q0", "q1", "k", "exclude"]
    assert list(inspect.signature(scan_context.two_stage_topk).parameters)[:4] == ["sc", "n_candidates", "k", "exclude"]
    assert F.SCAN_CONTEXT_PARAMS == R.PARAMS
    import torch
    with pytest.raises(RuntimeError, match="GPU only"):
        F.scan_context(torch.zeros((4, 3)), [4])
    with pytest.raises(RuntimeError, match="GPU only"):
        F.scan_context_distance(torch.zeros((2, 20, 60)), torch.zeros(2, dtype=torch.int64), torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU only"):
        F.scan_context_topk(torch.zeros((2, 20, 60)), torch.zeros(2, dtype=torch.int64), 0, 2, 1, 0)
