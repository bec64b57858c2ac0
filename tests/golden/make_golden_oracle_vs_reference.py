"""What the REFERENCE's own compiled C++ (oracle/_ref/libref_ops.so, built by oracle/Makefile from the reference's extension sources)
returns on the inputs of tests/test_oracle_vs_reference.py, stored as digests -> oracle_vs_reference_golden.json.

    python tests/golden/make_golden_oracle_vs_reference.py          (needs oracle/_ref/libref_ops.so)

Each entry is the shape, dtype and SHA-256 of one array in the canonical form the test compares: float32 points as their uint32 bits,
lengths and index lists as int64 (the reference's padding included; the cross search's rows sorted, its order inside equal-d2 runs
being open).  The arrays themselves would be ~4 MB; equal digests are equal bytes.  The test imports the case functions from here, so
the oracle's arrays are built exactly as the reference's were."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ops  # noqa: E402

OUT = os.path.join(HERE, "oracle_vs_reference_golden.json")
GRID_VOXELS = [0.3, 0.6, 1.2, 2.4, 0.45]
GRID_SCANS = ["003854", "000026"]
CLOUDS = [(0.3, [3.299999952316284, 5.099999904632568, 6.599999904632568]),
          (0.77, [-923.2300415039062, -922.4600219726562, -920.9200439453125])]


def scan(name):
    return np.load(os.path.join(HERE, "scans", name + ".npy"))


def digest(a):
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def grid_case(voxel, impl):
    out = {}
    for name in GRID_SCANS:
        xyz = scan(name)
        p, l = ops.grid_subsample(xyz, np.array([7000, len(xyz) - 7000]), voxel, impl=impl)
        out["grid_%s_%s_points" % (name, voxel)] = p.view(np.uint32)
        out["grid_%s_%s_lengths" % (name, voxel)] = l.astype(np.int64)
    return out


def radius_self_case(impl):
    xyz = scan("000560")
    lens = np.array([len(xyz)])
    return {"radius_self_000560": ops.radius_search(xyz, xyz, lens, lens, 1.275, -1, impl=impl).astype(np.int64)}


def radius_cross_case(impl):
    xyz = scan("000560")
    lens = np.array([len(xyz)])
    sub, sl = ops.grid_subsample(xyz, lens, 0.6)                       # the query points: the oracle's subsample for both sides
    b = ops.radius_search(sub, xyz, sl, lens, 1.275, -1, impl=impl)
    return {"radius_cross_000560_sorted": np.sort(b, 1).astype(np.int64)}


def clouds_case(voxel, cs, impl):
    """Planes / lines / a point at coordinates c with floor(c * fl(1/v)) * v > c (see the test)."""
    c = [np.float32(x) for x in cs]
    rng = np.random.default_rng(7)
    a = (rng.random((500, 3)) * 20).astype(np.float32)
    pl_z, pl_x, pl_y, ln, ln2 = a.copy(), a.copy(), a.copy(), a.copy(), a.copy()
    pl_z[:, 2] = c[0]
    pl_x[:, 0] = c[1]
    pl_y[:, 1] = c[2]
    ln[:, 1], ln[:, 2] = c[2], c[0]
    ln2[:, 0], ln2[:, 1] = c[1], c[2]
    pt = np.array([[c[0], c[1], c[2]]], np.float32)
    clouds = [a, pl_z, pl_x, pl_y, ln, ln2, pt]
    xyz = np.concatenate(clouds)
    lens = np.array([len(x) for x in clouds], dtype=np.int64)
    p, l = ops.grid_subsample(xyz, lens, voxel, impl=impl)
    return {"clouds_%s_points" % voxel: p.view(np.uint32), "clouds_%s_lengths" % voxel: l.astype(np.int64)}


def all_cases(impl):
    out = {}
    for v in GRID_VOXELS:
        out.update(grid_case(v, impl))
    out.update(radius_self_case(impl))
    out.update(radius_cross_case(impl))
    for v, cs in CLOUDS:
        out.update(clouds_case(v, cs, impl))
    return out


if __name__ == "__main__":
    if not ops.have_ref():
        sys.exit("oracle/_ref/libref_ops.so not built (make -C oracle ref, where the reference sources are)")
    ref = all_cases("ref")
    json.dump({k: digest(a) for k, a in sorted(ref.items())}, open(OUT, "w"), indent=1)
    print("%d arrays -> %s" % (len(ref), OUT))
