"""CPU: every nonzero code of the C ABI comes with a text of the form `<called entry>: ...` (include/lcr_hip.h, top comment).

The text is thread-local and never cleared, so an entry point that returns a code without setting one leaves the text of an earlier,
unrelated failure behind and Python raises with it.  Three checks: a sweep of every code-returning entry point with all-zero arguments
(refused, or accepted, on the host before any HIP call), a source rule that keeps the bare `return LCR_E...` from coming back, and a
table of refusals that sit behind a first check that passes (dummy non-null pointers, never dereferenced)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from lcrnet_amd import _lib

EARG, ESPACE = -1, -2
FAKE = ctypes.c_void_p(256)
CSRC = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")


def _signatures():
    sigs = {}
    for header in _lib.HEADERS:
        with open(header) as f:
            sigs.update(_lib.parse_header(f.read()))
    return {n: a for n, (res, a) in sigs.items() if res is ctypes.c_int and n not in _lib._RETURNS_VALUE}


SIGS = _signatures()
# the entry points whose all-zero call is in their domain (nothing to do: n == 0, or a host helper over no elements)
ACCEPT_ALL_ZERO = ["lcr_gather_rows", "lcr_hashmap_bucket_host", "lcr_hashmap_order_host", "lcr_inlier_weights", "lcr_neighbor_mean",
                   "lcr_scan_overlap", "lcr_upsample_concat", "lcr_vote_shift", "lcr_vote_shift_grad"]
# the one entry point whose all-zero call is in its domain AND would launch (a spin of 0 microseconds): it is swept with -1 microseconds
# instead, so that this file makes no HIP call.  Every call of the sweep is decided on the host: LCR_OK or LCR_EARG.
OUT_OF_DOMAIN = {"lcr_stream_spin": (-1, None)}


def _prime(L, name):
    """Leave a known refusal of ANOTHER entry point in this thread's text; returns it."""
    n = ctypes.c_size_t(0)
    if name == "lcr_icp_ws_bytes":
        assert L.lcr_teaser_ws_bytes(0, 0, 0, 0, ctypes.byref(n)) == EARG
        other = b"lcr_teaser_ws_bytes:"
    else:
        assert L.lcr_icp_ws_bytes(0, 0, 0, ctypes.byref(n)) == EARG
        other = b"lcr_icp_ws_bytes:"
    primed = L.lcr_last_error()
    assert primed.startswith(other)
    return primed


def _all_zero(L, name):
    """(code, text after) of `name` called with every scalar 0 and every pointer NULL (OUT_OF_DOMAIN apart), over a primed text; and that text."""
    primed = _prime(L, name)
    rc = getattr(L, name)(*OUT_OF_DOMAIN.get(name, [None if t is ctypes.c_void_p else t(0) for t in SIGS[name]]))
    return rc, L.lcr_last_error(), primed


def test_the_sweep_covers_the_library():
    assert len(SIGS) >= 140 and set(ACCEPT_ALL_ZERO) <= set(SIGS)


@pytest.mark.parametrize("name", sorted(SIGS))
def test_all_zero_call_is_accepted_or_refused_in_its_own_name(name):
    rc, text, primed = _all_zero(_lib.lib(), name)
    assert rc in (0, EARG), (rc, text)
    if rc == 0:
        assert text == primed, "a successful call does not touch the text"
    else:
        assert text.startswith(name.encode() + b":"), (rc, text)


def test_the_all_zero_calls_that_are_accepted():
    L = _lib.lib()
    assert sorted(n for n in SIGS if _all_zero(L, n)[0] == 0) == ACCEPT_ALL_ZERO


def test_no_bare_error_return_in_the_sources():
    """Outside common.h / common.hip no `return LCR_E...` (every nonzero code leaves through refuse()) and no set_error( at all."""
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) >= 40
    bare, setters = [], []
    for path in files:
        base = os.path.basename(path)
        with open(path) as f:
            for i, line in enumerate(f, 1):
                if base not in ("common.h", "common.hip") and re.search(r"return LCR_E", line):
                    bare.append("%s:%d" % (base, i))
                if base != "common.hip" and "set_error(" in line:
                    setters.append("%s:%d" % (base, i))
    assert bare == [] and setters == []


def _increasing(n, step=10):
    return np.arange(n, dtype=np.int64) * step


def _second_level(L):
    """{case: (entry point, thunk, code)}: refusals behind a first check that passes.  The codes are those of the parent commit."""
    up = _increasing(3)                      # offsets of one cloud pair ... the arrays outlive the thunks through the closure
    down = np.asarray([0, 10, 5], np.int64)
    layout = np.zeros(512, np.int64)         # room for an LcrPrecomputeLayout (about 600 bytes), filled on the host by lcr_precompute_layout
    limits = np.asarray([8, 8, 8, 8], np.int32)
    assert L.lcr_precompute_layout(100, 1, 4, limits.ctypes.data, 0, 1000, layout.ctypes.data) == 0        # raw mode: n_raw = 1000
    return {
        # the row width is the voxelisation's domain; the driver refuses it itself, in the name of the twin that was called
        "precompute rows of 65 floats": ("lcr_precompute_batch_rows_ex",
                                         lambda: L.lcr_precompute_batch_rows_ex(FAKE, 65, FAKE, layout.ctypes.data, 0.3, 1.0, 0.3, 0, 0, FAKE,
                                                                                1 << 40, FAKE, 1 << 40, FAKE, FAKE, None), EARG),
        "top1 workspace": ("lcr_top1_matching_ex",
                           lambda: L.lcr_top1_matching_ex(FAKE, 2, 8, 8, FAKE, FAKE, 0, FAKE, FAKE, FAKE, FAKE, 0, None), ESPACE),
        "topk workspace": ("lcr_topk_matching_ex",
                           lambda: L.lcr_topk_matching_ex(FAKE, 2, 8, 8, FAKE, FAKE, 3, 0, 1, 0.05, FAKE, FAKE, FAKE, FAKE, FAKE, 0, None), ESPACE),
        "lgr workspace": ("lcr_local_global_registration_ex",
                          lambda: L.lcr_local_global_registration_ex(FAKE, FAKE, FAKE, 100, FAKE, 4, FAKE, 1, 0.1, 3, 5, 0, FAKE, FAKE, FAKE, FAKE,
                                                                     FAKE, 0, None), ESPACE),
        "lgr correspondence_limit": ("lcr_local_global_registration_ex",
                                     lambda: L.lcr_local_global_registration_ex(FAKE, FAKE, FAKE, 100, FAKE, 4, FAKE, 1, 0.1, 3, 5, -1, FAKE, FAKE,
                                                                                FAKE, FAKE, FAKE, 1 << 40, None), EARG),
        "p2n decreasing point_off": ("lcr_point_to_node_partition_stack",
                                     lambda: L.lcr_point_to_node_partition_stack(FAKE, down.ctypes.data, FAKE, up.ctypes.data, 2, 4, FAKE, FAKE,
                                                                                 FAKE, FAKE, FAKE, FAKE, 1 << 40, None), EARG),
        "legacy lgr workspace": ("lcr_local_global_registration",
                                 lambda: L.lcr_local_global_registration(FAKE, FAKE, FAKE, 100, FAKE, 4, FAKE, 1, 0.1, 3, 5, FAKE, FAKE, FAKE,
                                                                         FAKE, FAKE, 0, None), ESPACE),
        "radius search workspace": ("lcr_radius_search",
                                    lambda: L.lcr_radius_search(FAKE, FAKE, FAKE, FAKE, 1, 10, 10, 0.5, 8, None, FAKE, None, FAKE, FAKE, 0, None),
                                    ESPACE),
        # past its own first check (a row mask, block_k = 32 with K <= 512, M*K < 2^29) the masked twin shares lcr_gemm_f32_bsplit's body
        "bsplit_masked null A": ("lcr_gemm_f32_bsplit_masked",
                                 lambda: L.lcr_gemm_f32_bsplit_masked(None, FAKE, FAKE, 64, 64, 480, None, None, None, 0, 0, None, FAKE, 32, None), EARG),
        "bsplit_masked bad stats": ("lcr_gemm_f32_bsplit_masked",
                                    lambda: L.lcr_gemm_f32_bsplit_masked(FAKE, FAKE, FAKE, 64, 64, 480, None, None, None, 0, 0, FAKE, FAKE, 32, None), EARG),
        # the launch-per-half-iteration form (a matrix beyond LDS) is chosen on the host and takes at most 65535 problems
        "sinkhorn_ex B=65536": ("lcr_log_sinkhorn_ex", lambda: L.lcr_log_sinkhorn_ex(FAKE, FAKE, FAKE, 65536, 300, 300, 10, 1e12, FAKE, 0, None), EARG),
        "sinkhorn B=65536": ("lcr_log_sinkhorn", lambda: L.lcr_log_sinkhorn(FAKE, FAKE, FAKE, 65536, 300, 300, 10, 1e12, FAKE, None), EARG),
    }


SECOND_LEVEL = ["top1 workspace", "topk workspace", "lgr workspace", "lgr correspondence_limit", "p2n decreasing point_off",
                "legacy lgr workspace", "radius search workspace", "sinkhorn_ex B=65536", "sinkhorn B=65536",
                "bsplit_masked null A", "bsplit_masked bad stats", "precompute rows of 65 floats"]


@pytest.mark.parametrize("case", SECOND_LEVEL)
def test_second_level_refusals_keep_their_code_and_name_the_called_entry(case):
    L = _lib.lib()
    name, thunk, code = _second_level(L)[case]
    _prime(L, name)
    assert thunk() == code, (case, L.lcr_last_error())
    assert L.lcr_last_error().startswith(name.encode() + b":"), (case, L.lcr_last_error())
