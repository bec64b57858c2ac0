"""GPU: lcr_augment_clouds bit for bit against the fp32 restatement (tests/augment_restatement.py) — points, order and out_len, with the
outputs and the workspace NaN-filled between canaries — on the edge shapes of the kernels (one point, odd lengths, [N,4] rows, a cloud
of two sort tiles plus a wavefront tail cut at every limit around its length, masked selection words whose ties fall to the original
index, 128 clouds); the contract properties (repeatable bytes, stack invariance, values independent of the limit, streams keyed by
sample_id and seed); planted mistakes in the restatement, each seen above the fp32 bound; and the augmenters feeding the collates."""
import ctypes

import numpy as np
import pytest
import torch

import augment_restatement as R

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
GUARD = 64
BIG = 2049 + 70             # two sort tiles plus a wavefront tail


def _cloud(seed, n, cols=3):
    g = np.random.default_rng(100 + seed)
    xyz = g.uniform(-80.0, 80.0, size=(n, 3)).astype(np.float32)
    if cols == 3:
        return xyz
    extra = (1000.0 + g.uniform(1.0, 2.0, size=(n, cols - 3))).astype(np.float32)     # would be seen at once if it leaked
    return np.ascontiguousarray(np.concatenate([xyz, extra], axis=1))


def _params(B, seed=0, identity=False):
    from lcrnet_amd.augment import draw_params
    if identity:
        return {"rotation": np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)), "scale": np.ones(B, np.float32), "shift": np.zeros((B, 3), np.float32),
                "noise": np.zeros(B, np.float32), "sample_id": np.arange(B, dtype=np.uint32)}
    g = np.random.default_rng(seed)
    per = [draw_params(g, 1, 0.01, 0.8, 1.2, 2.0, 1.0, "euler" if b % 2 else "yaw") for b in range(B)]
    q = {k: np.concatenate([p[k] for p in per]).astype(np.float32) for k in per[0]}
    q["sample_id"] = (np.arange(B, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(seed)).astype(np.uint32)
    return q


def _guarded(n, dtype, device):
    """n elements of NaN / all-ones between two canaries"""
    t = torch.empty(n + 2 * GUARD, dtype=dtype, device=device)
    if dtype == torch.uint8:
        t.fill_(0xFF)
        t[:GUARD], t[-GUARD:] = 0xA5, 0xA5
    elif dtype == torch.float32:
        t.fill_(float("nan"))
        t[:GUARD], t[-GUARD:] = 1234.5, 1234.5
    else:
        t.fill_(-(2 ** 62))
        t[:GUARD], t[-GUARD:] = 777, 777
    return t


def _intact(t):
    want = {torch.uint8: 0xA5, torch.float32: 1234.5, torch.int64: 777}[t.dtype]
    return bool((t[:GUARD] == want).all()) and bool((t[-GUARD:] == want).all())


def _device(clouds, q, limit=0, seed=SEED):
    """The raw entry on canaried buffers -> (points [M,3], out_len list)."""
    import lcrnet_amd._lib as L
    dev = torch.device("cuda")
    lens = np.array([len(c) for c in clouds], dtype=np.int64)
    B, n, cols = len(clouds), int(lens.sum()), clouds[0].shape[1]
    out_lens = np.minimum(lens, limit) if limit > 0 else lens
    m = int(out_lens.sum())
    rows = torch.from_numpy(np.concatenate(clouds)).to(dev)
    up = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in q.items()}
    d_len = torch.from_numpy(lens).to(dev)
    out, out_len = _guarded(3 * m, torch.float32, dev), _guarded(B, torch.int64, dev)
    need = L.ws_size("lcr_augment_clouds_ws_bytes", n, B, limit)
    ws = _guarded((need + 3) // 4 * 4, torch.uint8, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call.lcr_augment_clouds(L.ptr(rows), cols, L.ptr(d_len), B, n, L.ptr(up["sample_id"]), L.ptr(up["rotation"]), L.ptr(up["scale"]),
                              L.ptr(up["shift"]), L.ptr(up["noise"]), seed, limit, out.data_ptr() + 4 * GUARD, m,
                              out_len.data_ptr() + 8 * GUARD, L.ptr(status), ws.data_ptr() + GUARD, need, L.stream_ptr(dev))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert _intact(out) and _intact(out_len) and _intact(ws)
    pts = out[GUARD:GUARD + 3 * m].cpu().numpy().reshape(m, 3)
    assert not np.isnan(pts).any()                                  # every promised row was written
    got_len = out_len[GUARD:GUARD + B].cpu().tolist()
    assert got_len == out_lens.tolist()
    return pts, got_len


def _restated(clouds, q, limit=0, seed=SEED, mask=0xFFFFFFFF, plant=None):
    return R.augment_stack(clouds, q["sample_id"], q["rotation"], q["scale"], q["shift"], q["noise"], seed, limit, mask, plant)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(clouds, q, limit=0, mask=0xFFFFFFFF):
    got, got_len = _device(clouds, q, limit)
    want, want_len = _restated(clouds, q, limit, mask=mask)
    assert got_len == want_len
    assert _same(got, want), "max |device - restatement| = %g" % np.abs(got - want).max()
    return got


def _between():
    """one long cloud between two short ones: only the middle one is ever cut"""
    return [_cloud(1, 1), _cloud(2, BIG), _cloud(3, 1)]


def test_one_point():
    _check([_cloud(0, 1)], _params(1))
    _check([_cloud(0, 1)], _params(1), limit=1)


@pytest.mark.parametrize("cols", [3, 4])
def test_odd_lengths_and_trailing_columns(cols):
    clouds = [_cloud(s, n, cols) for s, n in enumerate([1, 65, 300])]
    got = _check(clouds, _params(3))
    assert np.abs(got).max() < 500.0                                # nothing of the 1000+ columns arrived
    if cols == 4:
        assert _same(got, _device([c[:, :3].copy() for c in clouds], _params(3))[0])
        wide = [np.ascontiguousarray(np.concatenate([c, c[:, 3:], c[:, 3:]], axis=1)) for c in clouds]      # [N,6]: the strided load
        assert _same(got, _device(wide, _params(3))[0])


@pytest.mark.parametrize("limit", [1, BIG - 1, BIG, BIG + 1])
def test_limits_around_the_length(limit):
    clouds, q = _between(), _params(3, 4)
    got = _check(clouds, q, limit)
    assert len(got) == min(BIG, limit) + 2


@pytest.mark.parametrize("limit", [1, BIG - 1, BIG, BIG + 1, 700])
def test_ties_fall_to_the_original_index(limit):
    import lcrnet_amd._lib as L
    clouds, q = _between(), _params(3, 4)
    L.lib().lcr_augment_debug_select_mask(0xF)
    try:
        _check(clouds, q, limit, mask=0xF)
    finally:
        L.lib().lcr_augment_debug_select_mask(0xFFFFFFFF)
    if limit == 700:                                                # the mask changes the choice: the hook does reach the kernel
        assert not np.array_equal(R.select(BIG, 700, q["sample_id"][1], SEED), R.select(BIG, 700, q["sample_id"][1], SEED, mask=0xF))
        _check(clouds, q, limit)


@pytest.mark.parametrize("limit", [0, 5])
def test_128_clouds(limit):
    clouds = [_cloud(s, 1 + s % 9) for s in range(128)]
    _check(clouds, _params(128, 9), limit)


def test_identity_parameters_return_the_input():
    clouds = [_cloud(s, n, 4) for s, n in enumerate([7, 130])]
    assert not np.signbit(np.concatenate(clouds)[np.concatenate(clouds) == 0]).any()
    got, _ = _device(clouds, _params(2, identity=True))
    assert _same(got, np.concatenate(clouds)[:, :3].copy())


def test_contract_properties():
    clouds, q, limit = [_cloud(1, 40), _cloud(2, BIG), _cloud(3, 33)], _params(3, 4), 700
    a, _ = _device(clouds, q, limit)
    b, _ = _device(clouds, q, limit)
    assert _same(a, b)                                              # the same bytes run to run
    mid = {k: v[1:2] for k, v in q.items()}
    alone, _ = _device([clouds[1]], mid, limit)
    assert _same(alone, a[40:40 + limit])                            # a cloud alone gives the bytes it gives inside the stack
    full, _ = _device(clouds, q, 0)
    keep = R.select(BIG, limit, q["sample_id"][1], SEED)
    assert _same(a[40:40 + limit], full[40:40 + BIG][keep])          # a kept point's value does not depend on the limit
    assert _same(a[:40], full[:40]) and _same(a[40 + limit:], full[40 + BIG:])
    other_id = dict(q, sample_id=q["sample_id"] + np.uint32(1))
    c, _ = _device(clouds, other_id, 0)
    d, _ = _device(clouds, q, 0, seed=SEED + 1)
    e, _ = _device(clouds, q, 0, seed=SEED + (1 << 32))              # both halves of the seed are the key
    for x in (c, d, e):
        assert (x != full).any(axis=1).mean() > 0.99
    assert not _same(c, d) and not _same(d, e)


@pytest.mark.parametrize("plant", ["transposed", "uncentred", "scaled_shift", "output_counter", "unstable"])
def test_planted_mistakes_are_seen(plant):
    import lcrnet_amd._lib as L
    clouds, q, limit = _between(), _params(3, 4), 700
    mask = 0xF if plant == "unstable" else 0xFFFFFFFF
    L.lib().lcr_augment_debug_select_mask(mask)
    try:
        got, _ = _device(clouds, q, limit)
    finally:
        L.lib().lcr_augment_debug_select_mask(0xFFFFFFFF)
    assert _same(got, _restated(clouds, q, limit, mask=mask)[0])
    wrong, _ = _restated(clouds, q, limit, mask=mask, plant=plant)
    bnd = max(R.bound(c, s, t, nz) for c, s, t, nz in zip(clouds, q["scale"], q["shift"], q["noise"]))
    diff = float(np.abs(wrong.astype(np.float64) - got).max())
    print("%s: max difference %.3e, fp32 bound %.3e" % (plant, diff, bnd))
    assert diff > bnd


def test_functional_wrapper():
    from lcrnet_amd import functional as F
    clouds, q = [_cloud(1, 40, 4), _cloud(2, BIG, 4), _cloud(3, 33, 4)], _params(3, 4)
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    for limit in (0, 700, 5000):
        pts, lens = F.augment_clouds(rows, [len(c) for c in clouds], q["sample_id"], q["rotation"].astype(np.float64), q["scale"], q["shift"],
                                     q["noise"], SEED, limit)
        want, want_len = _restated(clouds, q, limit)
        assert pts.is_cuda and lens.is_cuda and lens.dtype == torch.int64 and lens.cpu().tolist() == want_len
        assert _same(pts.cpu().numpy(), want)
    with pytest.raises(ValueError):
        F.augment_clouds(rows, [1, 2], q["sample_id"][:2], q["rotation"][:2], q["scale"][:2], q["shift"][:2], q["noise"][:2], SEED)


def test_call_path_does_not_synchronise_with_the_host():
    """torch's sync debug mode raises on any synchronising torch call: the wrapper and both augmenters, on device clouds and on host clouds
    (whose upload is a pinned asynchronous copy), with and without a limit that bites.  The ctypes call is outside its view: that
    lcr_augment_clouds only enqueues launches is established by reading csrc/augment.hip."""
    from lcrnet_amd import functional as F
    from lcrnet_amd.augment import LoopAugmenter, RegistrationAugmenter
    clouds, q = [_cloud(1, 40, 4), _cloud(2, 300, 4), _cloud(3, 33, 4)], _params(3, 4)
    dev_clouds = [torch.from_numpy(c).cuda() for c in clouds]
    rows = torch.cat(dev_clouds)
    reg, loop = RegistrationAugmenter(dict(TRAIN, point_limit=100), seed=1), LoopAugmenter(dict(TRAIN, point_limit=100), seed=1)
    reg(clouds[0], clouds[1], np.eye(4))                                                     # first use: pinned pool, library load
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for limit in (0, 100):
            F.augment_clouds(rows, [40, 300, 33], q["sample_id"], q["rotation"], q["scale"], q["shift"], q["noise"], SEED, limit)
        for src in (clouds, dev_clouds):
            a = reg(src[0], src[1], np.eye(4))
            b = loop(src[0], src[1:2], src[2:3])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert a["src_points"].shape == (100, 3) and b["pos_points"].shape == (100, 3) and b["neg_lengths"].tolist() == [33]


TRAIN = {"point_limit": 30000, "use_augmentation": True, "augmentation_noise": 0.01, "augmentation_min_scale": 0.8,
         "augmentation_max_scale": 1.2, "augmentation_shift": 2.0, "augmentation_rotation": 1.0, "pos_num": 2, "neg_num": 2}


def _pair(g):
    """40 ref and 36 src points, the first 36 ref points the src points moved by T, every value exact in fp32 (a quarter-turn yaw,
    coordinates and translation on a 2^-8 grid)"""
    src = np.round(g.uniform(-3.0, 3.0, size=(36, 3)) * 256.0) / 256.0
    T = np.eye(4)
    T[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [0.5, -0.25, 0.125]
    ref = np.concatenate([src @ T[:3, :3].T + T[:3, 3], np.round(g.uniform(-3.0, 3.0, size=(4, 3)) * 256.0) / 256.0])
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    return ref.astype(np.float32), src.astype(np.float32), T


def test_registration_augmenter_feeds_the_pair_collate():
    from lcrnet_amd.augment import RegistrationAugmenter
    from lcrnet_amd.data import registration_collate_fn_stack_mode
    ref, src, T = _pair(np.random.default_rng(3))
    aug = RegistrationAugmenter(TRAIN, seed=7351)
    xyzi = [np.concatenate([c, np.full((len(c), 1), 1000.0, np.float32)], axis=1) for c in (ref, src)]
    sample = aug(xyzi[0], torch.from_numpy(xyzi[1]), T)                                      # [N,4] as loaded: a host array and a tensor
    assert set(sample) == {"ref_points", "src_points", "ref_feats", "src_feats", "transform", "pos_aug_rotation", "anc_aug_rotation"}
    assert sample["ref_points"].is_cuda and sample["ref_points"].shape == (40, 3) and sample["src_points"].shape == (36, 3)
    assert sample["transform"].dtype == np.float32 and (sample["pos_aug_rotation"] is None) != (sample["anc_aug_rotation"] is None)
    dd = registration_collate_fn_stack_mode([sample], 4, 0.3, 1.275, [16, 16, 16, 16])
    for key in ("points", "lengths", "neighbors", "subsampling", "upsampling"):
        assert all(t.is_cuda for t in dd[key]), key
    assert torch.equal(dd["points"][0], torch.cat([sample["ref_points"], sample["src_points"]]))
    assert dd["lengths"][0].cpu().tolist() == [40, 36] and dd["features"].is_cuda and dd["features"].shape == (76, 1)
    assert torch.equal(dd["transform"], torch.from_numpy(sample["transform"])) and dd["batch_size"] == 1
    # the same draws replayed: the device clouds are the restatement of the per-cloud values the augmenter drew
    aug.reseed()
    again = aug(ref, src, T)
    assert torch.equal(again["ref_points"], sample["ref_points"]) and torch.equal(again["src_points"], sample["src_points"])
    assert np.array_equal(again["transform"], sample["transform"])
    two = aug.many([(ref, src, T), (src, ref, np.linalg.inv(T))])
    assert [s["ref_points"].shape[0] for s in two] == [40, 36] and not torch.equal(two[0]["ref_points"], sample["ref_points"])


@pytest.mark.parametrize("seed,rotate_ref", [(1, True), (2, True), (7, False), (8, False)])
def test_collated_pair_stays_aligned(seed, rotate_ref):
    from lcrnet_amd.augment import RegistrationAugmenter
    from lcrnet_amd.data import registration_collate_fn_stack_mode
    ref, src, T = _pair(np.random.default_rng(3))
    aug = RegistrationAugmenter(dict(TRAIN, augmentation_noise=0.0), seed=seed)
    dd = registration_collate_fn_stack_mode([aug(ref, src, T)], 4, 0.3, 1.275, [16, 16, 16, 16])
    assert (dd["pos_aug_rotation"] is not None) == rotate_ref and (dd["anc_aug_rotation"] is None) == rotate_ref      # both branches are run
    pts, T2 = dd["points"][0].cpu().numpy().astype(np.float64), dd["transform"].numpy().astype(np.float64)
    moved = pts[40:] @ T2[:3, :3].T + T2[:3, 3]
    err = float(np.abs(moved - pts[:36]).max())
    bnd = R.bound(np.concatenate([ref, src]), 1.2, [2.0], 0.0)          # the largest scale and shift the configuration can draw
    print("seed %d: |T' src' - ref'| %.3e, bound %.3e" % (seed, err, bnd))
    assert err <= bnd and float(np.abs(pts[40:] @ T[:3, :3].T + T[:3, 3] - pts[:36]).max()) > 1e3 * bnd


def test_loop_augmenter_feeds_the_online_triplet_collate():
    from lcrnet_amd.augment import LoopAugmenter
    from lcrnet_amd.data import train_loop_detection_collate_fn_stack_mode_online
    g = np.random.default_rng(8)
    scans = [g.uniform(-3.0, 3.0, size=(n, 4)).astype(np.float32) for n in (30, 50, 41, 22, 35)]
    aug = LoopAugmenter(dict(TRAIN, point_limit=40), seed=5)
    sample = aug(scans[0], scans[1:3], scans[3:5])
    assert sample["anc_points"].shape == (30, 3) and sample["pos_points"].shape == (80, 3) and sample["neg_points"].shape == (57, 3)
    assert sample["pos_lengths"].tolist() == [40, 40] and sample["neg_lengths"].tolist() == [22, 35] and sample["anc_lengths"].tolist() == [30]
    assert sample["pos_lengths"].dtype == np.int64 and sample["pos_num"] == 2 and sample["neg_num"] == 2
    assert all(sample[k].is_cuda for k in ("anc_points", "pos_points", "neg_points", "anc_feats", "pos_feats", "neg_feats"))
    dd = train_loop_detection_collate_fn_stack_mode_online([sample], 4, 0.3, 1.275, [16, 16, 16, 16])
    assert dd["lengths"][0].cpu().tolist() == [40, 40, 30, 22, 35]                                            # [pos.., anc, neg..]
    assert torch.equal(dd["points"][0], torch.cat([sample["pos_points"], sample["anc_points"], sample["neg_points"]]))
    assert dd["features"].shape == (167, 1) and dd["features"].is_cuda
    # every cloud is the restatement of its own draws: the anchor is cloud 0 of the call, sample ids run 0 .. 4
    aug.reseed()
    from lcrnet_amd.augment import draw_params
    rng = np.random.default_rng(5)
    per = [draw_params(rng, 1, 0.01, 0.8, 1.2, 2.0, 1.0) for _ in range(5)]
    want = [R.augment_cloud(c, i, p["rotation"][0], p["scale"][0], p["shift"][0], p["noise"][0], 5, 40)[0] for i, (c, p) in enumerate(zip(scans, per))]
    assert _same(sample["anc_points"].cpu().numpy(), want[0]) and _same(sample["pos_points"].cpu().numpy(), np.concatenate(want[1:3]))
    assert _same(sample["neg_points"].cpu().numpy(), np.concatenate(want[3:5]))
