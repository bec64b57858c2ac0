"""GPU: lcr_node_correspondences (csrc/node_corr.hip) against the fp32 NumPy restatement of tests/node_corr_restatement.py, bit for bit:
rows, start, and the overlaps compared as uint32; batch against single calls; a test-owned workspace filled with NaN and canary words
behind every output; a capacity that is too small; refusals; `get_node_correspondences_batched` on the pair model's own outputs through
the saved pair files into tools/registration_eval.py's coarse block; evaluation.correspondence_overlap against a brute-force search."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import node_corr_restatement as R
from conftest import GOLDEN, LIMITS, NUM_STAGES, RADIUS, ROOT, VOXEL, load_scan

pytestmark = pytest.mark.gpu
CANARY = 64               # words behind every output
FILL = 0x5A


def native(case, cap=None):
    """One native call on test-owned buffers: the workspace filled with 0xFF bytes (every float a NaN, every int -1), every output filled
    with a canary byte and CANARY words longer than asked for.  -> (corr (C,2), overlap (C,), start, status, tails intact?, cap used)."""
    from lcrnet_amd import functional as F
    dev = torch.device("cuda")
    P = case["P"]
    m = np.diff(case["node_off"])
    full = int((m[0::2] * m[1::2]).sum())
    cap = full if cap is None else cap
    nbytes = F.node_correspondences_ws_bytes(case["point_off"], case["node_off"], case["K"])
    ws = torch.full((nbytes + 4 * CANARY,), 0xFF, dtype=torch.uint8, device=dev)
    corr = torch.full((cap + CANARY, 2), FILL * 0x01010101, dtype=torch.int32, device=dev)
    ov = torch.full((cap + CANARY,), FILL * 0x01010101, dtype=torch.int32, device=dev).view(torch.float32)
    start = torch.full((P + 1 + CANARY,), FILL * 0x01010101, dtype=torch.int32, device=dev)
    status = torch.full((1 + CANARY,), FILL * 0x01010101, dtype=torch.int32, device=dev)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev)
    F.node_correspondences_raw(t("points"), case["point_off"], t("nodes"), case["node_off"], t("knn"), t("knn_mask"), t("node_mask"),
                               t("transforms"), case["pos_radius"], cap=cap, ws=ws[:nbytes], corr=corr, overlap=ov, start=start, status=status)
    torch.cuda.synchronize()
    start_h, status_h = start.cpu().numpy(), status.cpu().numpy()
    total = int(start_h[P])
    n = min(total, cap)
    corr_h, ov_h = corr.cpu().numpy(), ov.view(torch.int32).cpu().numpy()
    word = np.int32(FILL * 0x01010101)
    intact = bool((corr_h[n:] == word).all() and (ov_h[n:] == word).all() and (start_h[P + 1:] == word).all() and (status_h[1:] == word).all()
                  and (ws[nbytes:].cpu().numpy() == 0xFF).all())
    return corr_h[:n], ov_h[:n].view(np.uint32), start_h[:P + 1], int(status_h[0]), intact, cap


def check(case, labels=None):
    labels = R.batch_labels(case) if labels is None else labels
    want_corr, want_ov, want_start = R.stacked(labels)
    corr, ov, start, status, intact, _ = native(case)
    assert np.array_equal(start, want_start), (start, want_start)
    assert np.array_equal(corr, want_corr)
    assert np.array_equal(ov, want_ov.view(np.uint32))
    assert status == 0 and intact
    return corr, ov, start


SIZES3 = [(65, 130), (130, 2), (1, 65)]


@pytest.mark.parametrize("K", [1, 63, 64, 65, 128])
def test_rows_start_and_overlaps_equal_the_restatement_bit_for_bit(K):
    """P = 3, node counts 1 / 2 / 65 / 130 (one, two and three 64-node tiles with ragged edges), patches of K entries that share points,
    masked entries with real indices, padded tails, a node with every entry masked and a node with node_mask = 0 on each side."""
    case = R.make_case(100 + K, SIZES3, K, "generic", 0.45, n_pts=400 if K > 1 else 60)
    corr, _, start = check(case)
    assert start[-1] > 0 and len(corr) == start[-1]


@pytest.mark.parametrize("sizes", [[(2, 1)], [(0, 5)], [(5, 0)], [(0, 0)], [(130, 130)]])
def test_single_pairs_with_empty_and_small_sides(sizes):
    check(R.make_case(7, sizes, 64, "generic", 0.45, n_pts=200, special=sizes[0] == (130, 130)))


def test_thirty_two_pairs_with_pairs_that_do_not_overlap():
    counts = [0, 1, 2, 65, 130]
    sizes = [(counts[p % 5], counts[(p // 5 + p) % 5]) for p in range(32)]
    sizes[3], sizes[7] = (20, 20), (65, 2)                  # p % 4 == 3: the pairs whose clouds lie tens of metres apart
    case = R.make_case(32, sizes, 16, "generic", 0.45, n_pts=150)
    labels = R.batch_labels(case)
    assert len(labels[3]["rows"]) == 0 and len(labels[7]["rows"]) == 0 and sum(len(l["rows"]) for l in labels) > 100
    check(case, labels)


def test_empty_clouds_are_legal():
    """A pair whose clouds have no points and no nodes, in front of and behind an ordinary pair."""
    case = R.make_case(5, [(9, 11)], 24, "generic", 0.45, n_pts=120)
    po, mo = case["point_off"], case["node_off"]
    case.update(P=3, point_off=np.concatenate([[0, 0], po, [po[-1], po[-1]]]), node_off=np.concatenate([[0, 0], mo, [mo[-1], mo[-1]]]),
                transforms=np.concatenate([np.eye(4, dtype=np.float32)[None], case["transforms"], np.eye(4, dtype=np.float32)[None]]))
    _, _, start = check(case)
    assert start[0] == start[1] == 0 and start[2] == start[3] > 0


def test_lattice_case_with_pairs_at_exactly_the_radius():
    """r = 0.5 on the 1/16 m lattice with planted point pairs at exactly d^2 = 0.25: the comparison is strict."""
    case = R.make_case(12, [(9, 9), (1, 12)], 40, "lattice", 0.5, n_pts=120)
    good, le = R.batch_labels(case), R.batch_labels(case, mistake="le")
    assert any(not np.array_equal(a["cr"], b["cr"]) for a, b in zip(good, le))
    check(case, good)


def test_non_finite_coordinates_are_never_near():
    case = R.make_case(9, [(12, 12)], 20, "generic", 0.45, n_pts=100)
    case["points"][[3, 50, 130]] = [[np.nan, 0, 0], [np.inf, 1, 1], [0, -np.inf, np.nan]]
    check(case)


def test_demo_pair_at_full_size_equals_the_restatement_and_the_reference_rows():
    gold = np.load(os.path.join(GOLDEN, "matching_golden.npz"))
    case = R.golden_case(gold, load_scan("003854"), load_scan("000958"))
    corr, _, start = check(case)
    assert start[1] == 579 and np.array_equal(corr.astype(np.int64), gold["eval_gt_node_corr_indices"].astype(np.int64))


def test_each_pair_alone_gives_the_bytes_it_gives_in_the_batch():
    case = R.make_case(164, SIZES3, 64, "generic", 0.45, n_pts=400)
    corr, ov, start, _, _, _ = native(case)
    for p in range(case["P"]):
        c1, o1, s1, status, intact, _ = native(R.slice_pair(case, p))
        assert status == 0 and intact and s1.tolist() == [0, start[p + 1] - start[p]]
        assert c1.tobytes() == corr[start[p]:start[p + 1]].tobytes() and o1.tobytes() == ov[start[p]:start[p + 1]].tobytes()


def test_a_capacity_that_is_too_small_sets_the_status_bit_and_keeps_the_counts():
    case = R.make_case(164, SIZES3, 64, "generic", 0.45, n_pts=400)
    want_corr, want_ov, want_start = R.stacked(R.batch_labels(case))
    cap = int(want_start[-1]) // 2
    assert cap > 10
    corr, ov, start, status, intact, _ = native(case, cap=cap)
    assert status == 4                                       # LCR_STATUS_CAP_EXCEEDED
    assert np.array_equal(start, want_start)                 # the true counts
    assert len(corr) == cap and np.array_equal(corr, want_corr[:cap]) and np.array_equal(ov, want_ov[:cap].view(np.uint32))
    assert intact                                            # nothing at or beyond cap was touched
    corr0, _, start0, status0, intact0, _ = native(case, cap=0)
    assert status0 == 4 and np.array_equal(start0, want_start) and intact0 and len(corr0) == 0
    _, _, _, status1, intact1, _ = native(case, cap=int(want_start[-1]))        # exactly enough
    assert status1 == 0 and intact1


def test_refusals():
    from lcrnet_amd import _lib
    L = _lib.lib()
    case = R.make_case(1, [(4, 4)], 8, "generic", 0.45, n_pts=50)
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("points", "nodes", "knn", "knn_mask", "node_mask", "transforms")}
    po, mo = case["point_off"], case["node_off"]
    nbytes = ctypes.c_size_t(0)
    ws_bytes = lambda P, K, po_=po, mo_=mo, out=nbytes: L.lcr_node_correspondences_ws_bytes(po_.ctypes.data, mo_.ctypes.data, P, K, ctypes.byref(out))
    assert ws_bytes(1, 8) == 0 and nbytes.value > 0
    big = np.zeros(67, np.int64)
    assert ws_bytes(0, 8) == -1 and ws_bytes(33, 8, big, big) == -1 and ws_bytes(1, 0) == -1 and ws_bytes(1, 2049) == -1
    assert L.lcr_node_correspondences_ws_bytes(None, mo.ctypes.data, 1, 8, ctypes.byref(nbytes)) == -1
    assert L.lcr_node_correspondences_ws_bytes(po.ctypes.data, mo.ctypes.data, 1, 8, None) == -1
    assert ws_bytes(1, 8, po[::-1].copy(), mo) == -1                                            # decreasing offsets
    assert ws_bytes(1, 8) == 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    corr = torch.empty((16, 2), dtype=torch.int32, device=dev)
    ov = torch.empty(16, dtype=torch.float32, device=dev)
    start = torch.empty(2, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr

    def call(P=1, K=8, radius=0.45, cap=16, **null):
        a = dict(points=p(t["points"]), po=po.ctypes.data, nodes=p(t["nodes"]), mo=mo.ctypes.data, knn=p(t["knn"]), km=p(t["knn_mask"]),
                 nm=p(t["node_mask"]), T=p(t["transforms"]), corr=p(corr), ov=p(ov), start=p(start), status=p(status), ws=p(ws))
        a.update({k: None for k in null})
        return L.lcr_node_correspondences(a["points"], a["po"], a["nodes"], a["mo"], a["knn"], a["km"], a["nm"], a["T"], P, K, radius, cap,
                                          a["corr"], a["ov"], a["start"], a["status"], a["ws"], ws.numel(), _lib.stream_ptr(dev))

    assert call(P=0) == -1 and call(P=33) == -1 and call(K=0) == -1 and call(K=2049) == -1
    for name in ("points", "po", "mo", "knn", "km", "nm", "T", "corr", "ov", "start", "status", "ws"):
        assert call(**{name: True}) == -1, name
    assert call(radius=-1.0) == -1 and call(radius=float("nan")) == -1 and call(radius=1e30) == -1 and call(cap=-1) == -1
    assert L.lcr_node_correspondences(p(t["points"]), po.ctypes.data, p(t["nodes"]), mo.ctypes.data, p(t["knn"]), p(t["knn_mask"]), p(t["node_mask"]),
                                      p(t["transforms"]), 1, 8, 0.45, 16, p(corr), p(ov), p(start), p(status), p(ws), 16,
                                      _lib.stream_ptr(dev)) == -2                               # LCR_ESPACE: workspace too small
    assert call() == 0                                                                          # and the same call with everything in place runs
    torch.cuda.synchronize()
    want = R.stacked(R.batch_labels(case))
    assert start.cpu().numpy().tolist() == want[2].tolist()
    with pytest.raises(RuntimeError):
        from lcrnet_amd import functional as F
        F.node_correspondences(t["points"].cpu(), po, t["nodes"], mo, t["knn"], t["knn_mask"], t["node_mask"], t["transforms"], 0.45)


def test_batched_labels_of_the_pair_model_round_trip_through_the_pair_files(tmp_path):
    """`get_node_correspondences_batched` on what `forward_pairs` returns for the two planted-motion pairs (seeded weights): labels equal
    to the restatement's on the same tensors; saved with io_formats.save_registration they come back non-empty and
    tools/registration_eval.py prints the coarse block computed from them."""
    from lcrnet_amd import evaluation as ev
    from lcrnet_amd import io_formats as io
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family import LCRNet
    from lcrnet_amd.modules.registration import get_node_correspondences_batched
    from lcrnet_amd.pipeline import PairPipeline
    from lcrnet_amd.weights import seeded_state_dict
    cfg = make_cfg()
    cfg["neighbor_limits"] = LIMITS
    m = LCRNet(cfg).eval()
    m.load_state_dict(seeded_state_dict(m.state_dict(), 7351), strict=True)
    m = m.cuda()
    a = load_scan("003854")
    golds = [np.load(os.path.join(GOLDEN, "pose_e2e_%s_golden.npz" % c)) for c in ("shift", "rot3")]
    work = []
    for g in golds:
        pa, pb = torch.from_numpy(a).cuda(), torch.from_numpy(np.ascontiguousarray(g["cloud_b"], dtype=np.float32)).cuda()
        work.append((torch.cat([pa, pb]), torch.tensor([len(pa), len(pb)], dtype=torch.int64, device="cuda")))
    Ts = [torch.from_numpy(g["transform_gt"].astype(np.float32)) for g in golds]
    with PairPipeline(m, VOXEL, RADIUS, NUM_STAGES, LIMITS, workers=1, pairs_per_call=2) as pipe:
        outs = list(pipe.run(work))
        res = get_node_correspondences_batched(outs, Ts, 0.45)
        outs = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in o.items()} for o in outs]
    assert len(res) == 2 and len(outs) == 2
    files = []
    for p, (o, g) in enumerate(zip(outs, golds)):
        h = lambda k: o[k].cpu().numpy()
        km_p, km_a = h("pos_node_knn_masks").astype(np.uint8), h("anc_node_knn_masks").astype(np.uint8)
        want = R.pair_labels(h("pos_points_f"), h("anc_points_f"), h("pos_node_knn_indices"), h("anc_node_knn_indices"), km_p, km_a,
                             km_p.any(1), km_a.any(1), g["transform_gt"].astype(np.float32), 0.45)
        gi, go = o["gt_node_corr_indices"].cpu().numpy(), o["gt_node_corr_overlaps"].cpu().numpy()
        assert gi.dtype == np.int64 and go.dtype == np.float32 and len(gi) > 50
        assert np.array_equal(gi, want["rows"]) and np.array_equal(go.view(np.uint32), want["overlaps"].view(np.uint32))
        files.append(io.save_registration(str(tmp_path), 0, 10 + p, 20 + p, o, g["transform_gt"]))
        back = io.load_registration(files[-1])
        assert np.array_equal(back["gt_node_corr_indices"], gi) and np.array_equal(back["gt_node_corr_overlaps"], go)
    spec = importlib.util.spec_from_file_location("registration_eval_tool", os.path.join(ROOT, "tools", "registration_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.main([str(tmp_path)])
    ms, nums = [], []
    for o in outs:
        h = lambda k: o[k].cpu().numpy()
        ms.append(ev.coarse_matching_metrics(h("pos_points_c"), h("anc_points_c"), h("pos_node_corr_indices"), h("anc_node_corr_indices"),
                                             h("gt_node_corr_indices")))
        nums.append(len(h("pos_node_corr_indices")))
    want = ev.coarse_matching_summary(nums, ms)
    assert out["coarse_matching"] == want and 0 <= want["PIR"] <= 1 and want["NUM"] > 0
    print("coarse block of the two planted pairs (seeded weights):", want)


def test_correspondence_overlap_equals_a_brute_force_nearest_neighbour():
    from lcrnet_amd import evaluation as ev
    g = np.load(os.path.join(GOLDEN, "coarse_metrics_golden.npz"))
    for c in range(3):
        ref, src, T, radius = g["ov%d_ref" % c], g["ov%d_src" % c], g["ov%d_T" % c], float(g["ov%d_radius" % c])
        moved = np.ascontiguousarray(src @ T[:3, :3].T + T[:3, 3], dtype=np.float32)
        d = ref[:, None, :] - moved[None, :, :]                                                 # fp32, the chain of lcr_feature_nn with C = 3
        d2 = ((np.float32(0) + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        want = float(np.mean(np.sqrt(d2.min(1)) < np.float32(radius)))
        got = ev.correspondence_overlap(ref, src, T, radius)
        assert got == want, (c, got, want)
        if float(g["ov%d_margin" % c]) == 0:                                                    # no ref point within 1e-4 of the radius: the
            assert got == float(g["ov%d_overlap" % c])                                          # KD-tree of the reference's recipe says the same
    assert np.isnan(ev.correspondence_overlap(np.zeros((0, 3), np.float32), g["ov0_src"], None, 0.1))
