"""GPU: Scan Context descriptors, pair distances and the causal top-k search (csrc/scan_context.hip: lcr_scan_context,
lcr_scan_context_distance, lcr_scan_context_topk) against the restatement of tests/scan_context_restatement.py.

  * desc, ring_key, unit and mask bit for bit.  A cloud may be left out only if its bin margin is below 1e-9, at most 1 % of a case's
    clouds; tests/test_scan_context_cpu.py shows that the shared inputs leave out none.
  * pair distances within max(4 e_ref, 2^-20) of the fp64 restatement fed the same fp32 unit columns (e_ref: the restatement's own fp32
    form against its fp64 form, the error of the arithmetic the kernel is allowed; 2^-20: four fp32 ulps of a distance near 1, for the
    pairs whose e_ref happens to be tiny); the shift must be a minimiser within that tolerance on every pair, and the restatement's own
    wherever its best two shifts are 1e-5 apart.
  * top-k bit for bit against a host sort by (dist, idx) of the pair entry's own distances over every admissible candidate, so no ranking
    margin is needed.
Every output and workspace of the raw calls is filled with NaN bytes between canaries."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import scan_context_restatement as R

pytestmark = pytest.mark.gpu

GAP = 256
TOL_FLOOR = 2.0 ** -20


class Guarded:
    """regions of the given byte sizes in one device buffer of 0xff bytes (NaN as floats, -1 as integers), GAP canary bytes around each"""

    def __init__(self, sizes):
        self.sizes, self.off, at = list(sizes), [], GAP
        for s in self.sizes:
            self.off.append(at)
            at += (s + 255) // 256 * 256 + GAP
        self.buf = torch.full((at,), 0xFF, dtype=torch.uint8, device="cuda")

    def ptr(self, i):
        return ctypes.c_void_p(self.buf.data_ptr() + self.off[i])

    def get(self, i, dtype, shape):
        raw = self.buf[self.off[i]:self.off[i] + self.sizes[i]].cpu().numpy()
        return raw.view(dtype).reshape(shape).copy()

    def canaries_intact(self):
        b = self.buf.cpu().numpy().copy()
        for o, s in zip(self.off, self.sizes):
            b[o:o + s] = 0xFF
        return bool((b == 0xFF).all())


def stack(clouds):
    pts = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3), np.float32)
    return torch.from_numpy(np.ascontiguousarray(pts)).cuda(), np.asarray([len(c) for c in clouds], np.int64)


def raw_descriptors(clouds, params):
    from lcrnet_amd import _lib
    L = _lib.lib()
    pts, ln = stack(clouds)
    B, Rn, W = len(clouds), params["R"], params["W"]
    nb = ctypes.c_size_t(0)
    assert L.lcr_scan_context_ws_bytes(B, Rn, W, ctypes.byref(nb)) == 0
    g = Guarded([B * Rn * W * 4, B * Rn * 4, B * Rn * W * 4, B * 8, nb.value])
    rc = L.lcr_scan_context(_lib.ptr(pts), ln.ctypes.data, B, Rn, W, params["max_length"], params["lidar_height"], g.ptr(0), g.ptr(1), g.ptr(2), g.ptr(3),
                            g.ptr(4), nb.value, _lib.stream_ptr(pts.device))
    assert rc == 0, L.lcr_last_error()
    torch.cuda.synchronize()
    assert g.canaries_intact()
    return dict(desc=g.get(0, np.float32, (B, Rn, W)), ring_key=g.get(1, np.float32, (B, Rn)), unit=g.get(2, np.float32, (B, Rn, W)),
                mask=g.get(3, np.uint64, (B,)))


def upload(case):
    return torch.from_numpy(case["unit"]).cuda(), torch.from_numpy(case["mask"].view(np.int64)).cuda()


def raw_distance(unit, mask, pairs):
    """-> (dist f32 [P], shift i32 [P], status)"""
    from lcrnet_amd import _lib
    L = _lib.lib()
    pr = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))).cuda()
    P, (B, Rn, W) = len(pr), unit.shape
    g = Guarded([max(P, 1) * 4, max(P, 1) * 4, 4])
    rc = L.lcr_scan_context_distance(_lib.ptr(unit), _lib.ptr(mask), B, Rn, W, _lib.ptr(pr), P, g.ptr(0), g.ptr(1), g.ptr(2), None, 0,
                                     _lib.stream_ptr(unit.device))
    assert rc == 0, L.lcr_last_error()
    torch.cuda.synchronize()
    assert g.canaries_intact()
    return g.get(0, np.float32, (-1,))[:P], g.get(1, np.int32, (-1,))[:P], int(g.get(2, np.int32, (1,))[0])


def raw_topk(unit, mask, Q, q0, k, exclude):
    from lcrnet_amd import _lib
    L = _lib.lib()
    C, Rn, W = unit.shape
    nb = ctypes.c_size_t(0)
    assert L.lcr_scan_context_topk_ws_bytes(Q, q0, C, exclude, ctypes.byref(nb)) == 0
    g = Guarded([Q * k * 4, Q * k * 4, Q * k * 4, nb.value])
    rc = L.lcr_scan_context_topk(_lib.ptr(unit), _lib.ptr(mask), C, Rn, W, Q, q0, k, exclude, g.ptr(0), g.ptr(1), g.ptr(2), g.ptr(3), nb.value,
                                 _lib.stream_ptr(unit.device))
    assert rc == 0, L.lcr_last_error()
    torch.cuda.synchronize()
    assert g.canaries_intact()
    return g.get(0, np.int32, (Q, k)), g.get(1, np.float32, (Q, k)), g.get(2, np.int32, (Q, k))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


# ------------------------------------------------------------------------------------------------------------------ descriptors
CASES = [c["name"] for c in R.gpu_cases()]


def case(name):
    return {c["name"]: c for c in R.gpu_cases()}[name]


@functools.lru_cache(maxsize=None)
def got(name):
    c = case(name)
    return raw_descriptors(c["clouds"], c["params"])


@pytest.mark.parametrize("name", CASES)
def test_descriptors_equal_the_restatement_bit_for_bit(name):
    w, g = R.want(name), got(name)
    ok = w["margin"] >= R.MARGIN
    print("%s: %d clouds, left out for a margin below 1e-9: %d" % (name, len(ok), (~ok).sum()))
    assert (~ok).sum() <= 0.01 * len(ok)
    for key in ("desc", "ring_key", "unit", "mask"):
        assert g[key].shape == w[key].shape and np.array_equal(bits(g[key][ok]), bits(w[key][ok])), key
    if name == "below":
        assert (g["desc"][0] < 0).sum() > 100
    if name == "nonfinite":
        assert np.isfinite(g["desc"]).all() and np.isfinite(g["unit"]).all()


def test_planted_descriptor_mistakes_are_seen():
    c, g = case("box200"), got("box200")
    for mistake in ("sector_xy", "empty_-1000"):
        bad = np.stack([R.descriptor(cl, mistake=mistake, **c["params"]) for cl in c["clouds"]])
        assert np.abs(bad - g["desc"]).max() >= 1.0, mistake            # a bit-for-bit comparison sees any difference; this one is whole metres


def test_a_cloud_alone_gives_its_stack_bytes_and_a_second_run_the_same():
    from lcrnet_amd import functional as F
    c, g = case("scan"), got("scan")
    again = raw_descriptors(c["clouds"], c["params"])
    for key in g:
        assert np.array_equal(bits(again[key]), bits(g[key])), key
    for b in (1, 2):
        pts, ln = stack([c["clouds"][b]])
        alone = [t.cpu().numpy() for t in F.scan_context(pts, ln, **c["params"])]
        for key, a in zip(("desc", "ring_key", "unit", "mask"), alone):
            assert a.tobytes() == g[key][b:b + 1].tobytes(), key


# ------------------------------------------------------------------------------------------------------------------ pair distances
@functools.lru_cache(maxsize=None)
def got_distance(shape):
    c = R.distance_case(*shape)
    unit, mask = upload(c)
    return raw_distance(unit, mask, c["pairs"])


@pytest.mark.parametrize("shape", R.DISTANCE_SHAPES)
def test_pair_distances_against_the_fp64_restatement(shape):
    c = R.distance_case(*shape)
    dist, shift, status = got_distance(shape)
    u, m = c["unit"], c["mask"]
    assert status == 0 and len(dist) == R.N_PAIRS
    worst = 0.0
    for p, (a, b) in enumerate(c["pairs"]):
        d64 = R.shift_distances(u[a], m[a], u[b], m[b])
        tol = max(4.0 * R.e_ref(u[a], m[a], u[b], m[b]), TOL_FLOOR)
        want_d, want_s, gap = R.distance(u[a], m[a], u[b], m[b])
        worst = max(worst, abs(float(dist[p]) - want_d) / tol)
        assert abs(float(dist[p]) - want_d) <= tol, (p, a, b, dist[p], want_d, tol)
        assert 0 <= shift[p] < shape[1] and d64[shift[p]] <= d64.min() + tol, (p, a, b, shift[p], want_s)
        if gap >= 1e-5:
            assert shift[p] == want_s, (p, a, b, shift[p], want_s)
    print("%s: worst |dist - fp64| / tol = %.3f" % (shape, worst))
    # exact cases: one-hot columns (integer sums, the smallest tied shift) and the empty cloud
    at = {tuple(pr): p for p, pr in enumerate(c["pairs"].tolist())}
    period = c["period"]
    assert (dist[at[(7, 8)]], shift[at[(7, 8)]]) == (0.0, 1 % period) and (dist[at[(8, 7)]], shift[at[(8, 7)]]) == (0.0, (period - 1) % period)
    assert (dist[at[(7, 7)]], shift[at[(7, 7)]]) == (0.0, 0)
    for pr in ((0, 3), (3, 0), (0, 0)):
        assert bits(dist[at[pr]:at[pr] + 1])[0] == 0x3f800000 and shift[at[pr]] == 0
    for (a, b), s in c["rolls"].items():
        if u[a].any():
            assert shift[at[(a, b)]] == s and abs(dist[at[(a, b)]]) < 1e-6


def test_planted_distance_mistakes_are_seen():
    c = R.distance_case(20, 60)
    dist, shift, _ = got_distance((20, 60))
    u, m = c["unit"], c["mask"]
    for mistake in ("shift_reversed", "divide_by_W", "mask_not_rotated"):
        seen = 0.0
        for p, (a, b) in enumerate(c["pairs"]):
            tol = max(4.0 * R.e_ref(u[a], m[a], u[b], m[b]), TOL_FLOOR)
            bad_d, bad_s, _ = R.distance(u[a], m[a], u[b], m[b], mistake)
            seen = max(seen, abs(float(dist[p]) - bad_d) / tol, 1e9 if bad_s != shift[p] and R.distance(u[a], m[a], u[b], m[b])[2] >= 1e-5 else 0.0)
        assert seen >= 100.0, mistake


@pytest.mark.parametrize("shape", R.DISTANCE_SHAPES)
def test_each_pair_alone_gives_its_batch_bytes(shape):
    from lcrnet_amd import functional as F
    c = R.distance_case(*shape)
    dist, shift, _ = got_distance(shape)
    unit, mask = upload(c)
    pr = torch.from_numpy(c["pairs"]).cuda()
    outs = [F.scan_context_distance(unit, mask, pr[p:p + 1]) for p in range(R.N_PAIRS)]          # P = 1
    rev = F.scan_context_distance(unit, mask, pr.flip(0))
    none = F.scan_context_distance(unit, mask, pr[:0])
    torch.cuda.synchronize()
    for p, (d, s, st) in enumerate(outs):
        assert int(st.cpu()[0]) == 0 and bits(d.cpu().numpy())[0] == bits(dist)[p] and int(s.cpu()[0]) == shift[p], p
    assert np.array_equal(bits(rev[0].cpu().numpy()[::-1]), bits(dist)) and np.array_equal(rev[1].cpu().numpy()[::-1], shift)
    assert tuple(none[0].shape) == (0,) and tuple(none[1].shape) == (0,)
    again = raw_distance(unit, mask, c["pairs"])
    assert np.array_equal(bits(again[0]), bits(dist)) and np.array_equal(again[1], shift)


def test_pair_index_out_of_range_is_reported_and_reads_nothing():
    c = R.distance_case(20, 60)
    dist, shift, _ = got_distance((20, 60))
    unit, mask = upload(c)
    pairs = c["pairs"][:6].copy()
    pairs[1] = (R.N_DESC, 0)
    pairs[3] = (0, -1)
    pairs[4] = (2**30, 2**30)
    d, s, status = raw_distance(unit, mask, pairs)
    assert status == 5                                                 # the largest refused p, plus one
    assert np.isnan(d[[1, 3, 4]]).all() and (s[[1, 3, 4]] == -1).all()
    assert np.array_equal(bits(d[[0, 2, 5]]), bits(dist[[0, 2, 5]])) and np.array_equal(s[[0, 2, 5]], shift[[0, 2, 5]])


# ------------------------------------------------------------------------------------------------------------------ top-k
@functools.lru_cache(maxsize=None)
def database():
    return upload(R.topk_database())


def host_topk(unit, mask, Q, q0, k, exclude):
    """a host sort by (dist, idx) of the pair entry's own distances over every admissible candidate"""
    C = unit.shape[0]
    lims = [max(0, min(C, q0 + r - exclude)) for r in range(Q)]
    pairs = np.asarray([(q0 + r, j) for r in range(Q) for j in range(lims[r])], np.int32).reshape(-1, 2)
    d, s, status = raw_distance(unit, mask, pairs) if len(pairs) else (np.zeros(0, np.float32), np.zeros(0, np.int32), 0)
    assert status == 0
    idx, dist, shift = np.full((Q, k), -1, np.int32), np.full((Q, k), np.inf, np.float32), np.full((Q, k), -1, np.int32)
    at = 0
    for r in range(Q):
        dr, sr = d[at:at + lims[r]], s[at:at + lims[r]]
        at += lims[r]
        o = np.lexsort((np.arange(lims[r]), dr))[:k]
        idx[r, :len(o)], dist[r, :len(o)], shift[r, :len(o)] = o, dr[o], sr[o]
    return idx, dist, shift


@pytest.mark.parametrize("C,Q,q0,exclude,k", R.TOPK_CASES)
def test_topk_equals_a_host_sort_of_the_pair_distances(C, Q, q0, exclude, k):
    unit, mask = database()
    unit, mask = unit[:C].contiguous(), mask[:C].contiguous()
    idx, dist, shift = raw_topk(unit, mask, Q, q0, k, exclude)
    w_idx, w_dist, w_shift = host_topk(unit, mask, Q, q0, k, exclude)
    assert np.array_equal(idx, w_idx) and np.array_equal(bits(dist), bits(w_dist)) and np.array_equal(shift, w_shift)
    short = [r for r in range(Q) if max(0, min(C, q0 + r - exclude)) < k]
    for r in short:
        n = max(0, min(C, q0 + r - exclude))
        assert (idx[r, n:] == -1).all() and np.isposinf(dist[r, n:]).all() and (shift[r, n:] == -1).all()
    if (C, Q, q0, exclude, k) == (1, 1, 0, 0, 1):
        assert idx[0, 0] == -1                                          # no candidate at all
    if (C, Q, q0, exclude, k) == (300, 70, 150, 0, 50):
        ties = sum(int((dist[r, 1:] == dist[r, :-1]).sum()) for r in range(Q))
        assert ties > 0                                                 # copies in the database: equal distances, ordered by index


def test_a_query_block_alone_gives_its_bytes_in_a_larger_call_and_a_second_run_the_same():
    from lcrnet_amd import functional as F
    unit, mask = database()
    big = raw_topk(unit, mask, 70, 230, 128, 100)
    part = [t.cpu().numpy() for t in F.scan_context_topk(unit, mask, 241, 5, 128, 100)]
    again = raw_topk(unit, mask, 70, 230, 128, 100)
    for a, b, c in zip(big, part, again):
        assert np.array_equal(bits(a[11:16]), bits(b)) and np.array_equal(bits(a), bits(c))


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_planted_revisits_end_to_end(tmp_path):
    from lcrnet_amd import evaluation, io_formats as io, scan_context
    frames = [torch.from_numpy(f).cuda() for f in R.planted_sequence()]
    w = R.planted_want()
    n = R.N_SCENES
    sc = scan_context.sequence_scan_contexts(frames, batch=7)
    ok = w["sc"]["margin"] >= R.MARGIN
    assert ok.all() and np.array_equal(bits(sc.unit.cpu().numpy()), bits(w["sc"]["unit"]))
    assert np.array_equal(sc.mask.cpu().numpy().view(np.uint64), w["sc"]["mask"])
    k = 5
    rows, kept, yaw = scan_context.detect_loops(sc, 0.4, k=k, exclude=R.E2E_EXCLUDE, start=n)
    assert rows.shape == ((n - 1) * k, 3) and rows.dtype == np.float64
    assert np.array_equal(rows[::k, 0], np.arange(n, 2 * n - 1)) and np.array_equal(rows[::k, 1], np.arange(n - 1))      # each twin at rank 1
    assert np.array_equal(yaw["shift"][:, 0], w["shift"]) and np.allclose(yaw["yaw"][:, 0], w["shift"] * 2 * np.pi / 60)
    assert np.abs(rows[::k, 2] - w["dist"]).max() < 1e-5
    top = kept[np.r_[True, kept[1:, 0] != kept[:-1, 0]]]
    assert np.array_equal(top[:, 1], top[:, 0] - n) and len(top) == n - 1
    idx2, dist2, shift2 = scan_context.two_stage_topk(sc, 8, k=1, exclude=R.E2E_EXCLUDE, q0=n, q1=2 * n - 1)
    assert np.array_equal(idx2.cpu().numpy()[:, 0], np.arange(n - 1)) and np.array_equal(shift2.cpu().numpy()[:, 0], w["shift"])
    assert np.array_equal(bits(dist2.cpu().numpy()[:, 0]), bits(rows[::k, 2].astype(np.float32)))
    io.save_pair_dist(str(tmp_path), rows)
    back = np.load(os.path.join(str(tmp_path), "predicted_des_L2_dis.npz"))["arr_0"].reshape(-1, 3)
    gt = [np.asarray([i - n] if i >= n else [], np.int64) for i in range(2 * n)]
    assert evaluation.compute_topN(back, gt, 1) == 1.0


def test_loop_closure_run_with_the_scan_context_detector_needs_no_model(tmp_path):
    """the plumbing of loop_closure.run(detector="scan_context"): no desc_model, no per-frame descriptor files, the same pair-distance and top-1
    files; 24 frames are fewer than the search's first query frame (101), so no pair is listed and the pair model is never called"""
    from lcrnet_amd import loop_closure
    frames = [torch.from_numpy(f).cuda() for f in R.planted_sequence()]
    out = loop_closure.run(None, None, frames, 0.3, str(tmp_path), detector="scan_context")
    assert out["descriptors"] is None and out["pairs"] == [] and out["rows"].shape == (0, 3)
    assert np.array_equal(bits(out["scan_contexts"].unit.cpu().numpy()), bits(R.planted_want()["sc"]["unit"]))
    assert sorted(os.listdir(os.path.join(str(tmp_path), "features"))) == ["predicted_des_L2_dis.npz"]
    assert os.path.exists(out["top1_file"]) and os.path.exists(out["pose_file"])
    with pytest.raises(ValueError, match="detector"):
        loop_closure.run(None, None, frames, 0.3, str(tmp_path), detector="other")
