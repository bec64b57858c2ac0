"""CPU: the yardsticks of lcr_voxel_down_sample (Open3D's VoxelDownSample).  The product's host mirror of the hash-order replay is
pinned against a real libstdc++ unordered_map keyed on hash_eigen (with colliding codes); the fp64 restatement
(tests/o3d_voxel_restatement.py) is checked on clouds with known answers; hash_eigen against Python integers; the exact bucket
reduction against `%`."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from o3d_voxel_restatement import hash_eigen, hash_eigen_int, hashmap_order, voxel_down_sample, voxel_indices

HERE = os.path.dirname(os.path.abspath(__file__))
SCHED = [13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753, 42043, 85229, 172933, 351061, 712697, 1447153, 2938679, 5967347,
         12117689, 24607243, 49969847, 101473717, 206062531, 418453099, 849745171, 1725584621, 3504127453]


@pytest.fixture(scope="module")
def container(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine to build the libstdc++ container check")
    d = tmp_path_factory.mktemp("o3d_map")
    exe = str(d / "o3d_hashmap_order")
    subprocess.run([gxx, "-O1", "-std=c++17", os.path.join(HERE, "o3d_hashmap_order.cpp"), "-o", exe], check=True)

    def run(idx):
        src, dst = str(d / "idx.bin"), str(d / "order.bin")
        np.ascontiguousarray(idx, dtype=np.int32).tofile(src)
        subprocess.run([exe, src, dst], check=True)
        return np.fromfile(dst, dtype=np.int64)
    return run


def _distinct_in_first_order(idx):
    _, first = np.unique(idx, axis=0, return_index=True)
    return idx[np.sort(first)]


def _synthetic_indices(seed):
    import lcrnet_amd.synthetic as synthetic
    _, idx = voxel_indices(synthetic.synthetic_scan(seed, n_azimuth=900), 0.3)
    return _distinct_in_first_order(idx)


def test_collision_family_shares_codes():
    z = np.arange(-5, 40)
    a = np.stack([np.full_like(z, 1), np.full_like(z, 65), z], 1)
    b = np.stack([np.full_like(z, 2), np.full_like(z, 2), z], 1)
    assert np.array_equal(hash_eigen(a), hash_eigen(b))


@pytest.mark.parametrize("case", ["collisions", "collisions_shuffled", "dense_box", "syn0", "syn1", "syn5"])
def test_host_mirror_matches_libstdcxx_container(container, case):
    rng = np.random.default_rng(len(case))
    if case.startswith("collisions"):
        z = np.arange(0, 3000)
        idx = np.concatenate([np.stack([np.full_like(z, 1), np.full_like(z, 65), z], 1), np.stack([np.full_like(z, 2), np.full_like(z, 2), z], 1)])
        if case.endswith("shuffled"):
            idx = idx[rng.permutation(len(idx))]
    elif case == "dense_box":
        g = np.stack(np.meshgrid(np.arange(40), np.arange(40), np.arange(12), indexing="ij"), -1).reshape(-1, 3)
        idx = g[rng.permutation(len(g))]
    else:
        idx = _synthetic_indices(int(case[3:]))
    idx = _distinct_in_first_order(idx)
    codes = hash_eigen(idx)
    assert len(np.unique(codes)) < len(codes), "the set must contain colliding codes"
    assert np.array_equal(hashmap_order(codes), container(idx))


def test_host_mirror_distinct_codes_against_oracle(container):
    """Where no two codes are equal, the oracle's own container (which asserts distinct keys) agrees too."""
    from oracle import ops
    rng = np.random.default_rng(11)
    idx = _distinct_in_first_order(rng.integers(0, 50, size=(2500, 3)))
    codes = hash_eigen(idx)
    _, keep = np.unique(codes, return_index=True)
    idx, codes = idx[np.sort(keep)], codes[np.sort(keep)]
    assert np.array_equal(hashmap_order(codes), ops.hashmap_order(codes))
    assert np.array_equal(hashmap_order(codes), container(idx))


def test_hash_eigen_matches_python_integers():
    rng = np.random.default_rng(5)
    idx = np.concatenate([rng.integers(-2**31, 2**31 - 1, size=(300, 3)), rng.integers(-3, 600, size=(300, 3)),
                          np.array([[0, 0, 0], [1, 65, 7], [2, 2, 7], [-1, -1, -1], [2**31 - 1, -2**31, 0]])])
    got = hash_eigen(idx)
    want = np.array([hash_eigen_int(*map(int, t)) for t in idx], dtype=np.uint64)
    assert np.array_equal(got, want)


def test_bucket_reduction_matches_modulo():
    import lcrnet_amd._lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    rng = np.random.default_rng(9)
    codes = np.concatenate([rng.integers(0, 2**63, size=20000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1),
                            rng.integers(0, 2**52, size=2000, dtype=np.int64).astype(np.uint64),
                            np.array([0, 1, 2**64 - 1, 2**64 - 2, 2**63, 2**52, 3504127453 * 5, 3504127452], dtype=np.uint64)])
    out = np.empty(len(codes), np.int64)
    for p, d in enumerate(SCHED):
        for c in (codes, codes - np.uint64(1), codes // np.uint64(d) * np.uint64(d)):
            c = np.ascontiguousarray(c)
            rc = lib.lcr_hashmap_bucket_host(ctypes.c_void_p(c.ctypes.data), ctypes.c_int64(len(c)), ctypes.c_int(p), ctypes.c_void_p(out.ctypes.data))
            assert rc == 0
            assert np.array_equal(out.astype(np.uint64), c % np.uint64(d)), d


# ---- the restatement on clouds with known answers ----------------------------------------------------------------------------------
def test_points_on_voxel_faces():
    """Points exactly on the faces of the min - v/2 grid belong to the cell above the face (floor)."""
    v = 0.5
    # min = 0 -> origin -0.25; faces at 0.25, 0.75, ...: 0.0 and 0.2 lie in cell 0, 0.25 and 0.7 in cell 1, 0.75 in cell 2
    x = np.array([[0.0, 0, 0], [0.25, 0, 0], [0.2, 0, 0], [0.75, 0, 0], [0.7, 0, 0]], np.float32)
    f32, f64, codes = voxel_down_sample(x, v)
    assert len(f32) == 3
    a = x[:, 0].astype(np.float64)
    got = {tuple(r) for r in f64.tolist()}
    assert got == {((a[0] + a[2]) / 2.0, 0.0, 0.0), ((a[1] + a[4]) / 2.0, 0.0, 0.0), (0.75, 0.0, 0.0)}
    assert sorted(codes.tolist()) == sorted(hash_eigen(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]])).tolist())


def test_one_point_voxel_and_single_voxel():
    x = np.array([[1.5, -2.25, 3.0]], np.float32)
    f32, f64, _ = voxel_down_sample(x, 0.3)
    assert np.array_equal(f32, x) and np.array_equal(f64, x.astype(np.float64))
    y = np.array([[0.01, 0.02, 0.03], [0.02, 0.01, 0.0], [0.1, 0.05, 0.11]], np.float32)
    f32, f64, _ = voxel_down_sample(y, 0.3)
    assert f32.shape == (1, 3)
    want = np.zeros(3)
    for r in y.astype(np.float64):
        want = want + r
    assert np.array_equal(f64[0], want / 3.0)


def test_negative_coordinates_and_extra_column():
    x = np.array([[-10.0, -20.0, -1.0, 5.0], [-9.9, -19.95, -0.9, 7.0], [-10.5, -20.0, -1.0, 1.0]], np.float32)
    f32, f64, _ = voxel_down_sample(x, 0.3, out_cols=4)
    # min (-10.5, -20, -1), origin (-10.65, -20.15, -1.15): rows 0 and 1 share voxel (2, 0, 0), row 2 is voxel (0, 0, 0)
    o, idx = voxel_indices(x[:, :3], 0.3)
    assert idx.tolist() == [[2, 0, 0], [2, 0, 0], [0, 0, 0]]
    rows = {tuple(r) for r in f64.tolist()}
    a = x.astype(np.float64)
    assert rows == {tuple((a[0] + a[1]) / 2.0), tuple(a[2])}
    assert f32.dtype == np.float32 and np.array_equal(f32, f64.astype(np.float32))


def test_insertion_order_and_sequential_sums():
    """Averages are sums in input order: a voxel whose fp64 sum depends on the order (1e17 + 1 rounds back to 1e17)."""
    x = np.array([[1e17, 0, 0], [1.0, 0, 0], [-1e17, 0, 0], [1.0, 0, 0]], np.float32)
    f32, f64, _ = voxel_down_sample(x, 1e18)
    s = 0.0
    for r in x[:, 0].astype(np.float64):
        s += r
    assert s == 1.0 and f64[0, 0] == 0.25
