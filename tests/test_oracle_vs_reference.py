"""CPU: the oracle against the REFERENCE's own compiled C++.  What the reference returns on these inputs is stored as digests of its
arrays (tests/golden/oracle_vs_reference_golden.json, written from oracle/_ref/libref_ops.so by make_golden_oracle_vs_reference.py),
so the comparison needs no reference on the machine; where oracle/_ref/libref_ops.so is built, the oracle is also compared with it live."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import ops

sys.path.insert(0, GOLDEN)
import make_golden_oracle_vs_reference as gen  # noqa: E402

REF = json.load(open(gen.OUT))


def check(got, live_ref=None):
    """got: {key: the oracle's array in the canonical form}; each equals the reference's stored array (digest: shape, dtype, bytes)
    and, where the compiled reference is present, its live one."""
    for key, a in got.items():
        d = gen.digest(a)
        assert d["shape"] == REF[key]["shape"] and d["dtype"] == REF[key]["dtype"], (key, d, REF[key])
        assert d["sha256"] == REF[key]["sha256"], "%s: the oracle's bytes differ from the reference's" % key
        if live_ref is not None:
            assert np.array_equal(a, live_ref[key]), key


def live(fn, *args):
    return fn(*args, impl="ref") if ops.have_ref() else None


@pytest.mark.parametrize("voxel", [0.3, 0.6, 1.2, 2.4, 0.45])
def test_grid_subsample_bit_exact(voxel):
    check(gen.grid_case(voxel, "oracle"), live(gen.grid_case, voxel))      # 2 scans, lengths and points (bits) each


def test_radius_self_search_identical():
    # width == max count; self lists have no exact ties on these scans -> identical including order
    check(gen.radius_self_case("oracle"), live(gen.radius_self_case))


def test_radius_cross_search_equal_up_to_ties():
    # same width, same sets; order differs only inside equal-d2 runs (the rows are compared sorted)
    check(gen.radius_cross_case("oracle"), live(gen.radius_cross_case))


@pytest.mark.parametrize("voxel,cs", [(0.3, [3.299999952316284, 5.099999904632568, 6.599999904632568]), (0.77, [-923.2300415039062, -922.4600219726562, -920.9200439453125])])
def test_grid_subsample_clouds_below_the_voxel_origin(voxel, cs):
    """Planes / lines / a point at coordinates c with floor(c * fl(1/v)) * v > c: the whole cloud lands one cell below its own origin, the
    reference's extent on that axis is (size_t)(-1) + 1 = 0 and its keys wrap mod 2^64 (a plane x = c collapses into one voxel).  The
    oracle must restate exactly that — the compiled reference decides (the GPU twin of this test: tests/test_ops_gpu.py)."""
    got = gen.clouds_case(voxel, cs, "oracle")
    assert got["clouds_%s_lengths" % voxel][2] == 1
    check(got, live(gen.clouds_case, voxel, cs))
