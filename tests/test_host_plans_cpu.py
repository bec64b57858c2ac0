"""CPU: the host-side plans of the library — every workspace size that a layout function reports, the Sinkhorn form and
lcr_kpconv_mask_ok — against the values recorded before each of them was reduced to one function (tests/golden/make_host_plans_golden.py
describes the grid).  A caller sizes its buffers by these numbers and the kernels find their regions by the same layouts, so none may
move.  The library loads and answers without a GPU."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_host_plans_golden", os.path.join(GOLDEN, "make_host_plans_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "host_plans_golden.json")) as _f:
    ROWS = json.load(_f)
ENTRIES = sorted({r[0] for r in ROWS})


def test_golden_covers_the_grid():
    """the recorded rows are the generator's grid, in its order: no case dropped on either side"""
    assert [(r[0], r[1]) for r in ROWS] == [(e, a) for e, a in gen.cases()]
    assert ENTRIES == sorted(["lcr_point_to_node_ws_bytes", "lcr_top1_matching_ws_bytes", "lcr_topk_matching_ws_bytes", "lcr_lgr_ws_bytes",
                              "lcr_netvlad_ws_bytes", "lcr_retrieval_ws_bytes", "lcr_feature_nn_ws_bytes",
                              "lcr_feature_correspondences_ws_bytes", "lcr_log_sinkhorn_ws_floats", "lcr_log_sinkhorn_form",
                              "lcr_kpconv_mask_ok"])
    forms = {tuple(r[1]): r[3] for r in ROWS if r[0] == "lcr_log_sinkhorn_form"}
    # both sides of every form boundary were recorded as such
    assert forms[(1, 131, 131)] == 0 and forms[(1, 132, 131)] == 1 and forms[(1, 131, 132)] == 1
    assert forms[(1, 192, 192)] == 1 and forms[(1, 193, 193)] == 2
    assert forms[(32, 193, 193)] == 2 and forms[(33, 193, 193)] == 3
    assert forms[(16, 350, 330)] == 2 and forms[(17, 350, 330)] == 3
    assert forms[(1, 2000, 1100)] == 3 and forms[(1, 128, 128)] == 0 and forms[(16, 128, 128)] == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_host_plan_values_do_not_move(entry):
    from lcrnet_amd import _lib
    L = _lib.lib()
    rows = [r for r in ROWS if r[0] == entry]
    assert rows
    bad = []
    for _, args, rc, value in rows:
        got = gen.evaluate(L, entry, args)
        if got != (rc, value):
            bad.append((args, (rc, value), got))
    assert not bad, bad[:10]
