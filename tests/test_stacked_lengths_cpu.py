"""CPU: the six entry points that take B stacked clouds by host lengths refuse a bad table on the host, before anything is launched:
B outside 1..64, a negative length, a length or a total above 2^31-1, a null lengths array.  Each returns LCR_EARG (a launch without a
GPU would give LCR_EHIP) and lcr_last_error() names the entry point.  Every other argument is a dummy, non-null and never dereferenced."""
import ctypes

import numpy as np
import pytest

EARG = -1
FAKE = ctypes.c_void_p(256)
BIG = 1 << 40                                                          # workspace bytes: never the reason for a refusal

# (B, lengths); None = a null lengths array
BAD = {
    "B=0": (0, (10,)),
    "B=65": (65, (10,) * 65),
    "negative length": (2, (10, -1)),
    "length 2^31": (2, (10, 2**31)),
    "total 2^31": (2, (2**31 - 1, 1)),
    "null lengths": (2, None),
}


def _lens(lengths):
    if lengths is None:
        return None, None
    a = np.asarray(list(lengths) + [10] * 65, np.int64)                # readable up to any B the call names
    return a, a.ctypes.data


def _icp(L, name, B, src, tgt):
    head = (FAKE, src, FAKE, tgt) + ((FAKE,) if name.endswith("plane") else ())
    return getattr(L, name)(*head, B, FAKE, 0.5, 3, 1e-6, 1e-6, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, BIG, None)


def _calls(L, B, ln):
    """(entry point, thunk) for every way the table (B, ln) reaches the six entry points; ICP takes it as source and as target lengths."""
    keep, good = _lens((10,) * 65)
    out = [
        ("lcr_estimate_normals", lambda: L.lcr_estimate_normals(FAKE, ln, B, 0.5, 30, FAKE, FAKE, FAKE, FAKE, FAKE, BIG, None)),
        ("lcr_fpfh", lambda: L.lcr_fpfh(FAKE, FAKE, ln, B, 0.5, 30, FAKE, FAKE, FAKE, FAKE, BIG, None)),
        ("lcr_range_images", lambda: L.lcr_range_images(FAKE, ln, B, 16, 64, 3.0, -25.0, 50.0, FAKE, FAKE, FAKE, BIG, None)),
        ("lcr_scan_overlap", lambda: L.lcr_scan_overlap(FAKE, ln, B, FAKE, FAKE, FAKE, FAKE, 1, 16, 64, 3.0, -25.0, 50.0, 1.0, FAKE, FAKE,
                                                        FAKE, BIG, None)),
    ]
    for name in ("lcr_icp_point_to_point", "lcr_icp_point_to_plane"):
        out.append((name, lambda name=name: _icp(L, name, B, ln, good)))
        out.append((name, lambda name=name: _icp(L, name, B, good, ln)))
    return keep, out


@pytest.mark.parametrize("case", sorted(BAD))
def test_bad_length_tables_are_refused_on_the_host(case):
    from lcrnet_amd import _lib
    L = _lib.lib()
    B, lengths = BAD[case]
    keep, ln = _lens(lengths)
    keep2, calls = _calls(L, B, ln)
    assert len(calls) == 8
    for name, thunk in calls:
        assert thunk() == EARG, (case, name)
        assert L.lcr_last_error().startswith(name.encode() + b":"), (case, name, L.lcr_last_error())
