"""CPU: the ctypes binding (lcr-net_amd/_lib.py) takes its signatures from include/*.h and offers two views of the library — lib(), whose
functions return their code, and call, whose functions raise on a nonzero code.  Nothing here needs a GPU."""
import ctypes
import re

import pytest
import torch

import lcrnet_amd._lib as L

vp, i32, i64, f32, f64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t

# typed out by hand from the headers; together they cover every type the parser maps
ANCHORS = {
    "lcr_voxel_down_sample": (i32, [vp, i32, i32, vp, i32, i64, f64, i32, vp, vp, vp, vp, vp, sz, vp]),
    "lcr_ransac_correspondences": (i32, [vp, vp, vp, i32, f32, i32, i32, ctypes.c_uint64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "lcr_ktimer_kinds": (None, [ctypes.c_uint]),
    "lcr_last_error": (ctypes.c_char_p, []),
    "lcr_adan_grad_norm": (i32, [vp, i32, f64, f64, vp, vp, sz, vp]),
    "lcr_gap_loss": (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, i64, i64, i64, i32, vp, vp, vp,
                           f64, vp, vp, vp, i64, i64, f64, vp, vp, f64, vp, vp, vp,
                           vp, vp, vp, vp, vp, vp, sz, vp]),
}


def _declared():
    """name -> parameter count, read from the headers with a parser of the test's own (names and commas only)"""
    out = {}
    for header in L.HEADERS:
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        for name, params in re.findall(r"\b(lcr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
            out[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return out


def _keeps_gil(fn):
    return bool(fn._flags_ & ctypes._FUNCFLAG_PYTHONAPI)


def test_every_declared_function_is_bound_in_both_views():
    lib, declared = L.lib(), _declared()
    assert len(declared) >= 127
    for name, n in declared.items():
        raw, checked = getattr(lib, name), getattr(L.call, name)
        assert raw is not checked, name
        assert len(raw.argtypes) == n and list(checked.argtypes) == list(raw.argtypes) and checked.restype is raw.restype, name


@pytest.mark.parametrize("name", sorted(ANCHORS))
def test_hand_written_anchor(name):
    res, args = ANCHORS[name]
    for fn in (getattr(L.lib(), name), getattr(L.call, name)):
        assert fn.restype is res and list(fn.argtypes) == args


def test_anchors_cover_every_mapped_type():
    assert len(ANCHORS["lcr_gap_loss"][1]) == 37
    assert set(L._SCALARS.values()) | {vp} == {t for _, a in ANCHORS.values() for t in a}
    assert set(L._RESULTS.values()) == {r for r, _ in ANCHORS.values()}


def test_refusal_is_a_code_in_the_raw_view_and_an_exception_in_the_checked_view():
    from lcrnet_amd.data import PrecomputeLayout
    lay, lim = PrecomputeLayout(), (ctypes.c_int * 2)(4, 4)
    args = (10, 65, 2, ctypes.cast(lim, vp), 1, 0, ctypes.addressof(lay))   # B = 65 > 64
    assert L.lib().lcr_precompute_layout(*args) != 0
    text = L.lib().lcr_last_error().decode()
    assert text
    with pytest.raises(RuntimeError) as e:
        L.call.lcr_precompute_layout(*args)
    assert "lcr_precompute_layout" in str(e.value) and "rc=" in str(e.value) and text in str(e.value)
    assert L.call.lcr_precompute_layout(10, 1, 2, ctypes.cast(lim, vp), 1, 0, ctypes.addressof(lay)) == 0
    assert L.call.lcr_version() == L.lib().lcr_version() >= 1               # a value, not a code: no exception


def test_workspace_helper_on_the_cpu_device():
    n = ctypes.c_size_t(0)
    assert L.lib().lcr_greedy_nms_ws_bytes(1000, ctypes.byref(n)) == 0
    assert L.ws_size("lcr_greedy_nms_ws_bytes", 1000) == n.value
    ws = L.ws("lcr_greedy_nms_ws_bytes", 1000, device=torch.device("cpu"))
    assert ws.dtype == torch.uint8 and ws.device.type == "cpu" and ws.numel() == max(n.value, 256)


def test_interpreter_lock_rule_holds_in_both_views():
    import os
    assert os.environ.get("LCR_CTYPES_KEEP_GIL", "1") != "0", "this test describes the default setting"
    lib, declared = L.lib(), _declared()
    assert L._RELEASES_GIL <= set(declared) and len(L._RELEASES_GIL) == 20
    for name in declared:
        for fn in (getattr(lib, name), getattr(L.call, name)):
            assert _keeps_gil(fn) == (name not in L._RELEASES_GIL), name


def test_parser_refuses_what_it_does_not_understand():
    with pytest.raises(RuntimeError, match="lcr_x"):
        L.parse_header("int lcr_x(long double v);")
    with pytest.raises(RuntimeError, match="lcr_y"):
        L.parse_header("long lcr_y(int v);")
    with pytest.raises(RuntimeError, match="lcr_z"):
        L.parse_header("int lcr_z(int (*callback)(int));")
    assert L.parse_header("/* lcr_no(int) */ const char * lcr_a(void);\nvoid lcr_b(const float* const* p, unsigned flags /* x, y */, size_t n);") == {
        "lcr_a": (ctypes.c_char_p, []), "lcr_b": (None, [vp, ctypes.c_uint, sz])}
