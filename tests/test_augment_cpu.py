"""CPU: the pieces of the training augmentation that need no GPU — Philox4x32-10 of the restatement against the published vectors (the
library's generator is held to the restatement bit for bit on the GPU), the fp32 restatement (tests/augment_restatement.py) against
its fp64 form within a derived bound, the reference's pair augmentation (tests/golden/augment_pair.npz, written by make_golden_augment.py from the imported reference) against
compose_pair_transform and the restatement fed the recorded draws, alignment of an augmented pair, the selection, draw_params and the
augmenters' reseed(), and the argument refusals of lcr_augment_clouds / lcr_augment_clouds_ws_bytes."""
import ctypes
import os

import numpy as np
import pytest

import augment_restatement as R
from conftest import GOLDEN

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert tuple(int(x) for x in R.philox4x32(counter, key)) == want


def test_philox_vectorised_form_matches_the_scalar_one():
    idx = np.array([0, 1, 2, 70000, 2 ** 31 - 3], dtype=np.uint64)
    got = R.philox4x32((idx, 0, 9, 1), R.seed_key(0x0123456789ABCDEF))
    for i, row in zip(idx, got):
        assert np.array_equal(row, R.philox4x32((int(i), 0, 9, 1), (0x89ABCDEF, 0x01234567)))


def _params(seed, n=1, rotation="yaw"):
    from lcrnet_amd.augment import draw_params
    return draw_params(np.random.default_rng(seed), n, 0.01, 0.8, 1.2, 2.0, 1.0, rotation)


@pytest.mark.parametrize("rotation", ["yaw", "euler"])
def test_fp32_restatement_is_its_fp64_form_within_the_rounding_bound(rotation):
    g = np.random.default_rng(5)
    for case in range(6):
        p = g.uniform(-120.0, 120.0, size=(400, 3)).astype(np.float32)
        q = {k: v[0].astype(np.float32) for k, v in _params(case, 1, rotation).items()}
        u = R.uniforms(np.arange(len(p)), case, 77)
        assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
        a = R.transform_f32(p, u, q["rotation"], q["scale"], q["shift"], q["noise"])
        b = R.transform_f64(p, u, q["rotation"], q["scale"], q["shift"], q["noise"])
        err, bnd = float(np.abs(a.astype(np.float64) - b).max()), R.bound(p, q["scale"], q["shift"], q["noise"])
        print("case %d: fp32 - fp64 %.3e, bound %.3e" % (case, err, bnd))
        assert a.dtype == np.float32 and err <= bnd


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "augment_pair.npz"), allow_pickle=False)


def _case(golden, s):
    return {k[len("s%d_" % s):]: golden[k] for k in golden.files if k.startswith("s%d_" % s)}


def _fields(golden):
    return dict(zip([str(n) for n in golden["field_names"]], [float(v) for v in golden["fields"]]))


def test_golden_holds_both_branches(golden):
    sides = {int(s): bool(_case(golden, s)["rotate_ref"]) for s in golden["seeds"]}
    assert sorted(sides) == list(range(8))
    assert [s for s, r in sides.items() if r] == [0, 2, 5, 6] and [s for s, r in sides.items() if not r] == [1, 3, 4, 7]


def _replayed(golden, s):
    """The per-pair values that the recorded draws give through this package's formulas."""
    from lcrnet_amd.augment import yaw_matrix
    c, f = _case(golden, s), _fields(golden)
    A = yaw_matrix(c["u_rot"][0] * np.pi * 2 / f["augmentation_rotation"])
    scale = f["augmentation_min_scale"] + (f["augmentation_max_scale"] - f["augmentation_min_scale"]) * float(c["u_scale"])
    return c, f, A, scale, bool(float(c["u_side"]) > 0.5)


@pytest.mark.parametrize("s", range(8))
def test_compose_pair_transform_is_the_reference(golden, s):
    from lcrnet_amd.augment import compose_pair_transform
    c, f, A, scale, rotate_ref = _replayed(golden, s)
    assert rotate_ref == bool(c["rotate_ref"])
    T, pos, anc = compose_pair_transform(c["transform"], A, rotate_ref, scale, c["ref_shift"], c["src_shift"])
    want = c["transform_out"]
    rel = float(np.abs(T - want).max() / np.abs(want).max())
    print("seed %d: transform rel. difference %.3e" % (s, rel))
    assert T.dtype == np.float64 and rel <= 1e-12
    named = pos if rotate_ref else anc
    assert (pos is None) == (not rotate_ref) and (anc is None) == rotate_ref
    assert named.dtype == np.float32 and np.array_equal(named, c["aug_rotation"].astype(np.float32))


@pytest.mark.parametrize("s", range(8))
def test_points_from_the_recorded_draws(golden, s):
    c, f, A, scale, rotate_ref = _replayed(golden, s)
    eye = np.eye(3)
    for name, R_cloud in (("ref", A if rotate_ref else eye), ("src", eye if rotate_ref else A)):
        p, shift = c[name].astype(np.float32), c[name + "_shift"]
        assert np.array_equal(p.astype(np.float64), c[name])
        got = R.transform_f32(p, c["u_" + name].astype(np.float32), R_cloud, scale, shift, f["augmentation_noise"])
        err, bnd = float(np.abs(got.astype(np.float64) - c[name + "_out"]).max()), R.bound(p, scale, shift, f["augmentation_noise"])
        print("seed %d %s: restatement - reference %.3e, bound %.3e" % (s, name, err, bnd))
        assert err <= bnd


def _exact_pair(g):
    """src and ref = R0 src + t0 with every value exact in fp32: a quarter-turn yaw, coordinates and translation on a 2^-8 grid."""
    src = np.round(g.uniform(-60.0, 60.0, size=(50, 3)) * 256.0) / 256.0
    R0 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t0 = np.array([3.25, -7.5, 0.75])
    ref = src @ R0.T + t0
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R0, t0
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    return ref.astype(np.float32), src.astype(np.float32), T0


@pytest.mark.parametrize("rotation", ["yaw", "euler"])
@pytest.mark.parametrize("rotate_ref", [True, False])
def test_alignment_is_preserved(rotation, rotate_ref):
    from lcrnet_amd.augment import compose_pair_transform
    g = np.random.default_rng(11)
    ref, src, T0 = _exact_pair(g)
    q = {k: v.astype(np.float32).astype(np.float64) for k, v in _params(3, 2, rotation).items()}       # the values the device applies
    A, eye, scale = q["rotation"][0], np.eye(3), q["scale"][0]
    assert q["scale"][0] == q["scale"][1]
    half = np.full((50, 3), 0.5, np.float32)
    ref2 = R.transform_f32(ref, half, A if rotate_ref else eye, scale, q["shift"][0], 0.0)
    src2 = R.transform_f32(src, half, eye if rotate_ref else A, scale, q["shift"][1], 0.0)
    T, _, _ = compose_pair_transform(T0, A, rotate_ref, scale, q["shift"][0], q["shift"][1])
    moved = src2.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    err = float(np.abs(moved - ref2).max())
    bnd = R.bound(np.concatenate([ref, src]), scale, q["shift"], 0.0)
    print("%s rotate_ref=%s: |T' src' - ref'| %.3e, bound %.3e" % (rotation, rotate_ref, err, bnd))
    assert err <= bnd
    wrong = src2.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]                                           # the old transform no longer aligns
    assert float(np.abs(wrong - ref2).max()) > 1e3 * bnd


def test_selection_restatement():
    for L, limit in ((7, 7), (7, 9), (7, 0), (1, 1)):
        assert np.array_equal(R.select(L, limit, 3, 1), np.arange(L))
    for L, limit in ((7, 6), (300, 1), (2119, 2118), (2119, 700)):
        keep = R.select(L, limit, 3, 1)
        assert len(keep) == limit and len(np.unique(keep)) == limit and keep.min() >= 0 and keep.max() < L
        w = R.select_words(L, 3, 1).astype(np.int64)
        pairs = list(zip(w[keep], keep))
        assert pairs == sorted(zip(w, range(L)))[:limit]
    keep = R.select(300, 200, 3, 1, mask=0xF)
    w = R.select_words(300, 3, 1, 0xF)
    assert len(np.unique(w)) <= 16 and len(np.unique(keep)) == 200
    for a, b in zip(keep, keep[1:]):                       # ties abound and are resolved by the original index
        assert (w[a], a) < (w[b], b)
    assert not np.array_equal(R.select(300, 200, 3, 1, mask=0xF, plant="unstable"), keep)
    assert not np.array_equal(R.select(300, 200, 4, 1), R.select(300, 200, 3, 1))


def test_draw_params():
    from lcrnet_amd.augment import draw_params
    for factor in (1.0, 4.0):
        q = draw_params(np.random.default_rng(2), 13, 0.01, 0.8, 1.2, 2.0, factor)
        assert q["rotation"].shape == (13, 3, 3) and q["rotation"].dtype == np.float64
        assert np.all(q["scale"] == q["scale"][0]) and 0.8 <= q["scale"][0] < 1.2            # one scale per sample
        assert q["shift"].shape == (13, 3) and np.abs(q["shift"]).max() <= 2.0 and len(np.unique(q["shift"])) == 39
        assert np.all(q["noise"] == 0.01)
        yaw = np.arctan2(q["rotation"][:, 1, 0], q["rotation"][:, 0, 0]) % (2 * np.pi)
        assert np.all(yaw >= 0.0) and np.all(yaw < 2 * np.pi / factor) and len(np.unique(yaw)) == 13
        assert np.all(q["rotation"][:, 2, :] == [0.0, 0.0, 1.0]) and np.all(q["rotation"][:, :2, 2] == 0.0)
        again = draw_params(np.random.default_rng(2), 13, 0.01, 0.8, 1.2, 2.0, factor)
        assert all(np.array_equal(q[k], again[k]) for k in q)
    e = draw_params(np.random.default_rng(2), 4, 0.01, 0.8, 1.2, 2.0, 1.0, rotation="euler")["rotation"]
    assert np.abs(e @ e.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14 and np.abs(e[:, 2, 2] - 1.0).min() > 1e-3
    with pytest.raises(ValueError):
        draw_params(np.random.default_rng(2), 1, 0.01, 0.8, 1.2, 2.0, 1.0, rotation="axis")


def test_augmenters_take_the_reference_field_names_and_reseed_replays():
    from lcrnet_amd.augment import LoopAugmenter, RegistrationAugmenter
    train = {"point_limit": 30000, "use_augmentation": True, "augmentation_noise": 0.01, "augmentation_min_scale": 0.8,
             "augmentation_max_scale": 1.2, "augmentation_shift": 2.0, "augmentation_rotation": 1.0, "pos_num": 3, "neg_num": 3,
             "batch_size": 1, "num_workers": 6}
    for cls in (RegistrationAugmenter, LoopAugmenter):
        a = cls.from_cfg({"seed": 7351, "train": train})
        assert a.seed == 7351 and a.point_limit == 30000 and a.noise == 0.01 and a.pos_num == 3
        first = [a._draw(2), a._ids(2)]
        second = [a._draw(2), a._ids(2)]
        assert not np.array_equal(first[0]["shift"], second[0]["shift"]) and list(first[1]) == [0, 1] and list(second[1]) == [2, 3]
        a.reseed()
        again = [a._draw(2), a._ids(2)]
        assert all(np.array_equal(first[0][k], again[0][k]) for k in first[0]) and np.array_equal(first[1], again[1])
        a.reseed(5)
        assert a.seed == 5 and not np.array_equal(a._draw(2)["shift"], first[0]["shift"])
    off = RegistrationAugmenter({"use_augmentation": False}, seed=1)._draw(2)
    assert np.all(off["rotation"] == np.eye(3)) and np.all(off["scale"] == 1.0) and not off["shift"].any() and not off["noise"].any()


def test_functional_wrapper_refuses_cpu_tensors():
    import torch
    from lcrnet_amd import functional as F
    with pytest.raises(RuntimeError, match="GPU only"):
        F.augment_clouds(torch.zeros(4, 3), [4], [0], np.eye(3)[None], [1.0], np.zeros((1, 3)), [0.0], 0)


# ---- argument refusals: nothing here reaches a launch ------------------------------------------------------------------------------
def _entry_args(B=2, row_floats=3, n_cap=10, out=True, ws_short=0, limit=4, out_cap=None):
    import lcrnet_amd._lib as L
    keep = [np.zeros(64 * 64, np.float32), np.zeros(128, np.int64), np.zeros(128, np.uint32), np.zeros(128 * 9, np.float32),
            np.zeros(128, np.float32), np.zeros(128 * 3, np.float32), np.zeros(128, np.float32), np.zeros(64 * 3, np.float32),
            np.zeros(128, np.int64), np.zeros(1, np.uint32)]
    need = ctypes.c_size_t(0)
    ok_B, ok_n = min(max(B, 1), 128), max(n_cap, 0)
    assert L.lib().lcr_augment_clouds_ws_bytes(ok_n, ok_B, limit, ctypes.byref(need)) == 0 and need.value > 0
    ws = np.zeros(need.value, np.uint8)
    keep.append(ws)
    p = [a.ctypes.data for a in keep]
    args = (p[0], row_floats, p[1], B, n_cap, p[2], p[3], p[4], p[5], p[6], 12345, limit, p[7] if out else None,
            n_cap if out_cap is None else out_cap, p[8], p[9], p[10], need.value - ws_short, None)
    return args, keep


@pytest.mark.parametrize("what,kw", [("B = 0", dict(B=0)), ("B = 129", dict(B=129)), ("row_floats 2", dict(row_floats=2)),
                                     ("row_floats 65", dict(row_floats=65)), ("negative n_cap", dict(n_cap=-1)),
                                     ("NULL output", dict(out=False)), ("workspace one byte short", dict(ws_short=1)),
                                     ("workspace short without a limit", dict(ws_short=1, limit=0)),
                                     ("output capacity above n_cap", dict(out_cap=11))])
def test_entry_refuses_with_earg_and_text(what, kw):
    import lcrnet_amd._lib as L
    lib = L.lib()
    args, keep = _entry_args(**kw)
    lib.lcr_augment_clouds_ws_bytes(-1, 0, 0, None)                 # leaves some other text behind
    before = lib.lcr_last_error()
    assert lib.lcr_augment_clouds(*args) == -1, what
    text = lib.lcr_last_error().decode()
    assert text.startswith("lcr_augment_clouds:") and text != before.decode(), (what, text)
    with pytest.raises(RuntimeError, match="lcr_augment_clouds"):
        L.call.lcr_augment_clouds(*args)


def test_ws_bytes_is_a_host_function_and_refuses_its_arguments():
    import lcrnet_amd._lib as L
    lib, n = L.lib(), ctypes.c_size_t(0)
    assert L.ws_size("lcr_augment_clouds_ws_bytes", 0, 1, 0) > 0
    plain, cut = L.ws_size("lcr_augment_clouds_ws_bytes", 100000, 78, 0), L.ws_size("lcr_augment_clouds_ws_bytes", 100000, 78, 30000)
    assert plain < 4096 and cut >= plain + 100000 * 24                              # without a limit: the header only
    assert L.ws_size("lcr_augment_clouds_ws_bytes", 100000, 78, 1) == cut
    for bad in ((10, 0, 0), (10, 129, 0), (-1, 1, 0), (2 ** 31 - 1, 1, 0)):
        assert lib.lcr_augment_clouds_ws_bytes(*bad, ctypes.byref(n)) == -1, bad
        assert lib.lcr_last_error().decode().startswith("lcr_augment_clouds_ws_bytes:"), bad
    assert lib.lcr_augment_clouds_ws_bytes(10, 1, 0, None) == -1 and lib.lcr_last_error().decode().startswith("lcr_augment_clouds_ws_bytes:")
    assert "lcr_augment_clouds" not in L._RELEASES_GIL and "lcr_augment_clouds_ws_bytes" not in L._RELEASES_GIL
