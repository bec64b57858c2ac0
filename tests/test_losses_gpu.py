"""GPU: the native registration loss terms (csrc/losses.hip behind lcrnet_amd.functional / lcrnet_amd.losses) against the fp64
restatement of tests/losses_restatement.py.

Tolerance rule (R.bound): a float quantity may differ from the restatement by at most 4 x e_ref, e_ref being the error of the reference's
own fp32 module against the same restatement (from tests/golden/losses_golden.npz), with a floor of 2^-20 relative to the largest
magnitude in the tensor.  Quantities the reference does not expose (the row and column terms on their own) are held to the floor alone.
Integer outputs — label planes, kept / positive / active counts, nearest rows — are exact.  Every caller-owned buffer is NaN-filled and
followed by canaries, which must survive."""
import json
import os

import numpy as np
import pytest
import torch

import losses_restatement as R
import lcrnet_amd.losses as L
from lcrnet_amd import functional as F
from lcrnet_amd.config import make_cfg
from test_losses_cpu import check_case_margins

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


# ---- caller-owned buffers with canaries ---------------------------------------------------------------------------------------------------------
class Guarded:
    def __init__(self):
        self.full = []

    def buf(self, n, dtype):
        n = int(np.prod(n))
        canary = {torch.uint8: 0xA5, torch.int32: -7777}.get(dtype, 12345.0)
        fill = {torch.uint8: 0xEE, torch.int32: -1}.get(dtype, float("nan"))
        t = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=DEV)
        t[PAD:PAD + n] = fill
        self.full.append((t, n, canary))
        return t[PAD:PAD + n]

    def check(self):
        torch.cuda.synchronize()
        for t, n, canary in self.full:
            assert bool((t[:PAD] == canary).all()) and bool((t[PAD + n:] == canary).all()), "a canary was overwritten"


def geometry(cases):
    """The cases' slices back to back, every pair of every case a pair of the call."""
    n, m, seg = [], [], [0]
    for c in cases:
        B, N1, M1 = c["scores"].shape
        n += [N1 - 1] * B
        m += [M1 - 1] * B
        seg += [seg[-1] + s for s in c["seg"][1:]]
    return F.GapGeometry(n, m, seg, DEV)


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_gap(cases, source):
    """gap_loss + gap_loss_grad (upstream 0.5, 0.5) over `cases` in ONE call, into guarded buffers."""
    g = geometry(cases)
    flat = lambda k, w=None: cu(np.concatenate([c[k].reshape(-1) if w is None else c[k].reshape(-1, w) for c in cases]))
    S = flat("scores")
    gd = Guarded()
    lines = g.rows + g.cols
    out = {"terms": gd.buf((g.P, 3), torch.float32).view(g.P, 3), "kept": gd.buf((g.P, 2), torch.int32).view(g.P, 2),
           "labels": gd.buf(g.elems, torch.uint8), "line_pos": gd.buf(lines, torch.float64), "line_hinge": gd.buf(lines, torch.float64),
           "line_count": gd.buf(lines, torch.int32), "line_active": gd.buf(lines, torch.int32), "status": gd.buf(1, torch.int32)}
    import ctypes
    nbytes = ctypes.c_size_t(0)
    assert F._L().lcr_gap_loss_ws_bytes(g.rows, g.cols, ctypes.byref(nbytes)) == 0
    ws = gd.buf(max(nbytes.value, 256), torch.uint8)
    if source == "points":
        kw = {"points": (flat("p_pts", 3), flat("q_pts", 3), cu(np.concatenate([c["transforms"] for c in cases])), R.RADIUS)}
    else:
        kw = {"overlaps": (cu(np.concatenate([c["corr"] for c in cases])), cu(np.concatenate([c["overlaps"] for c in cases])),
                           [len(c["corr"]) for c in cases], R.THR)}
    F.gap_loss(S, g, R.GAMMA, flat("pmask"), flat("qmask"), out=out, ws=ws, **kw)
    dS = gd.buf(g.elems, torch.float32)
    F.gap_loss_grad(S, g, R.GAMMA, out, torch.full((g.P, 2), 0.5, device=DEV), dS=dS)
    gd.check()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["dS"], res["geom"] = dS.cpu().numpy(), g
    assert res["status"][0] == 0
    return res


def split(res, cases):
    """The one-call result cut back into per-case pieces shaped like the restatement's."""
    g, out, b0, p0 = res["geom"], [], 0, 0
    for c in cases:
        B, N1, M1 = c["scores"].shape
        P = len(c["seg"]) - 1
        s0, s1 = g.soff_h[b0], g.soff_h[b0 + B]
        r0, r1, c0, c1 = g.roff_h[b0], g.roff_h[b0 + B], g.rows + g.coff_h[b0], g.rows + g.coff_h[b0 + B]
        piece = {"terms": res["terms"][p0:p0 + P], "kept": res["kept"][p0:p0 + P], "labels": res["labels"][s0:s1].reshape(B, N1, M1),
                 "dS": res["dS"][s0:s1].reshape(B, N1, M1)}
        for k in ("line_pos", "line_hinge", "line_count", "line_active"):
            piece["row_" + k] = res[k][r0:r1].reshape(B, N1 - 1)
            piece["col_" + k] = res[k][c0:c1].reshape(B, M1 - 1)
        out.append(piece)
        b0, p0 = b0 + B, p0 + P
    return out


def compare_gap(got, c, r, e_loss, e_grad, what):
    """One case's native result against its restatement r.  Returns the figures; asserts nothing about floats (the caller does)."""
    seg = c["seg"]
    want_labels = torch.cat([q["labels"] for q in r["pairs"]]).numpy()
    assert np.array_equal(got["labels"], want_labels), what + ": label plane"
    assert np.array_equal(got["kept"], r["kept"]), what + ": kept counts"
    for side in ("row", "col"):
        keep = torch.cat([q[side]["keep"] for q in r["pairs"]]).numpy()
        cnt = torch.cat([q[side]["count"] for q in r["pairs"]]).numpy()
        act = torch.cat([q[side]["active"] for q in r["pairs"]]).numpy()
        assert np.array_equal(got[side + "_line_count"], cnt), what + ": positive counts"
        assert np.array_equal(got[side + "_line_active"], np.where(keep, act, -1)), what + ": active counts"
    const = torch.cat([R.constant_entries(q) for q in r["pairs"]]).numpy()
    assert (got["dS"][const] == 0).all() and (got["dS"][:, -1, -1] == 0).all(), what + ": dS must be exactly zero on constant entries"
    keep_r = torch.cat([q["row"]["keep"] for q in r["pairs"]]).numpy()
    keep_c = torch.cat([q["col"]["keep"] for q in r["pairs"]]).numpy()
    assert (got["dS"][:, :-1, :][~keep_r] == 0).all() and (got["dS"][:, :, :-1].transpose(0, 2, 1)[~keep_c] == 0).all(), \
        what + ": dS must be exactly zero on dropped lines"
    fig = {"mean": (R.err(got["terms"][:, 2], r["terms"][:, 2]), R.bound(e_loss, r["terms"][:, 2])),
           "row": (R.err(got["terms"][:, 0], r["terms"][:, 0]), R.bound(0, r["terms"][:, 0])),
           "col": (R.err(got["terms"][:, 1], r["terms"][:, 1]), R.bound(0, r["terms"][:, 1])),
           "dS": (R.err(got["dS"], r["grad"]), R.bound(e_grad, r["grad"]))}
    print(what, {k: "%.3g (bound %.3g, e_ref %.3g)" % (v[0], v[1], {"mean": e_loss, "dS": e_grad}.get(k, 0)) for k, v in fig.items()})
    return fig


def holds(fig):
    return all(e <= b for e, b in fig.values())


@pytest.fixture(scope="module")
def gap_runs():
    """Every point-label case run alone, once."""
    return {ci: split(run_gap([R.cached("gap", ci)[0]], "points"), [R.cached("gap", ci)[0]])[0] for ci in range(len(R.GAP_SHAPES))}


@pytest.mark.parametrize("ci", range(len(R.GAP_SHAPES)))
def test_gap_core_point_labels(gold, gap_runs, ci):
    c, r = check_case_margins("gap", ci)
    e_loss = R.err(r["terms"][:, 2], gold["gap%d_loss" % ci])
    e_grad = R.err(r["grad"], gold["gap%d_grad" % ci])
    assert holds(compare_gap(gap_runs[ci], c, r, e_loss, e_grad, "gap %s" % (R.GAP_SHAPES[ci],)))


def test_gap_core_overlap_labels(gold):
    c, r = check_case_margins("node")
    got = split(run_gap([c], "overlaps"), [c])[0]
    e_loss, e_grad = R.err(r["terms"][0, 2], gold["node_loss"]), R.err(r["grad"][0], gold["node_grad"])
    assert holds(compare_gap(got, c, r, e_loss, e_grad, "node gap %s" % (R.NODE_SHAPE,)))


def test_gap_batch_invariance(gap_runs):
    """Pairs of different patch counts and sizes in one call give, bit for bit, the bytes of the single calls: forward and gradient."""
    ids = [1, 3, 2]
    cases = [R.cached("gap", ci)[0] for ci in ids]
    for piece, ci in zip(split(run_gap(cases, "points"), cases), ids):
        for k, v in piece.items():
            assert np.array_equal(v, gap_runs[ci][k], equal_nan=True), (ci, k)
    a, b = R.node_case(), R.node_case((1, 23, 19), seed=1)
    one = [split(run_gap([c], "overlaps"), [c])[0] for c in (a, b)]
    for piece, alone in zip(split(run_gap([a, b], "overlaps"), [a, b]), one):
        for k, v in piece.items():
            assert np.array_equal(v, alone[k], equal_nan=True), k


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_are_seen(gold, gap_runs, mistake):
    """The restatement with one definition changed must FAIL the comparison the correct one passes, on these inputs."""
    if mistake == "ge_at_4r2":
        c = R.tie_case()
        got = split(run_gap([c], "points"), [c])[0]
        good, bad = R.gap_results(None, case=c)[1], R.gap_results(None, mistake=mistake, case=c)[1]
        R.assert_margins(d2=good["pairs"][0]["decision"], radius=R.RADIUS, cores=good["pairs"], tie_at_4r2=True)
        assert np.array_equal(got["labels"], good["pairs"][0]["labels"].numpy()) and not np.array_equal(got["labels"], bad["pairs"][0]["labels"].numpy())
        assert R.err(got["terms"], good["terms"]) <= R.bound(0, good["terms"]) < R.err(got["terms"], bad["terms"])
        return
    seen = False
    for ci in ("masked", 1, 2, 3):
        c, r = R.cached("gap", ci)
        tag = "m" if ci == "masked" else ci
        got = gap_runs[ci] if ci != "masked" else split(run_gap([c], "points"), [c])[0]
        bad = R.gap_results(None, mistake=mistake, case=c)[1]
        e_loss, e_grad = R.err(r["terms"][:, 2], gold["gap%s_loss" % tag]), R.err(r["grad"], gold["gap%s_grad" % tag])
        if ci == "masked":
            assert holds(compare_gap(got, c, r, e_loss, e_grad, "gap with scored masked points"))
        nan_differs = not np.array_equal(np.isnan(bad["terms"]), np.isnan(got["terms"]))
        seen |= nan_differs or np.abs(np.nan_to_num(bad["terms"][:, 2]) - np.nan_to_num(got["terms"][:, 2])).max() > R.bound(e_loss, r["terms"][:, 2]) \
            or np.abs(np.nan_to_num(bad["grad"]) - got["dS"]).max() > R.bound(e_grad, r["grad"])
    assert seen


# ---- nearest distance -----------------------------------------------------------------------------------------------------------------------------
def run_md(cases, valids):
    A, D = cu(np.concatenate([c["A"] for c in cases])), cu(np.concatenate([c["D"] for c in cases]))
    ac, dc = [len(c["A"]) for c in cases], [len(c["D"]) for c in cases]
    gd = Guarded()
    out = {"dist": gd.buf(len(A), torch.float32), "arg": gd.buf(len(A), torch.int32), "mean": gd.buf(len(cases), torch.float32),
           "count": gd.buf(len(cases), torch.int32)}
    saved = F.min_dist(A, D, ac, dc, cu(np.concatenate(valids)), out=out)
    dA = gd.buf(3 * len(A), torch.float32).view(-1, 3)
    F.min_dist_grad(A, D, ac, dc, saved, torch.ones(len(cases), device=DEV), dA=dA)
    gd.check()
    res = {k: out[k].cpu().numpy() for k in ("dist", "arg", "mean", "count")}
    res["dA"] = dA.cpu().numpy()
    return res


@pytest.mark.parametrize("size", R.MD_SIZES)
def test_min_dist(gold, size):
    c, r = check_case_margins("md", size)
    got = run_md([c], [c["valid"]])
    tag = "md_%d_%d_" % size
    assert np.array_equal(got["arg"], r["arg"]) and got["count"][0] == c["valid"].sum()
    want_grad = r["grad"]
    fig = {"dist": (R.err(got["dist"], r["dist"]), R.bound(R.err(r["dist"], gold[tag + "dist"]), r["dist"]), R.err(r["dist"], gold[tag + "dist"])),
           "mean": (R.err(got["mean"][0], r["mean"]), R.bound(R.err(r["mean"], gold[tag + "mean"]), r["mean"]), R.err(r["mean"], gold[tag + "mean"])),
           "dA": (R.err(got["dA"], want_grad), R.bound(R.err(want_grad, gold[tag + "grad"]), want_grad), R.err(want_grad, gold[tag + "grad"]))}
    print("min dist %s" % (size,), {k: "%.3g (bound %.3g, e_ref %.3g)" % v for k, v in fig.items()})
    for k, (e, b, e_ref) in fig.items():
        assert e <= b, k
        assert e <= max(e_ref, 2.0 ** -20 * np.abs(r["dist"]).max()), k + ": differences should come in below the expansion's error"
    assert (got["dA"][~c["valid"]] == 0).all()
    if c["tie_rows"]:
        assert got["arg"][0] == 0
    none = run_md([c], [np.zeros(len(c["A"]), bool)])
    assert np.isnan(none["mean"][0]) and none["count"][0] == 0 and (none["dA"] == 0).all() and np.array_equal(none["arg"], r["arg"])


def test_min_dist_uneven_segments_equal_single_calls():
    cases = [R.min_dist_case(37, 1000), R.min_dist_case(1, 1), R.min_dist_case(300, 5000)]
    valids = [cases[0]["valid"], np.zeros(1, bool), cases[2]["valid"]]
    got = run_md(cases, valids)
    assert np.isnan(got["mean"][1]) and not np.isnan(got["mean"][[0, 2]]).any()
    q0 = 0
    for p, (c, v) in enumerate(zip(cases, valids)):
        one = run_md([c], [v])
        sl = slice(q0, q0 + len(c["A"]))
        for k in ("dist", "arg", "dA"):
            assert np.array_equal(got[k][sl], one[k], equal_nan=True), (p, k)
        assert np.array_equal(got["mean"][p:p + 1], one["mean"], equal_nan=True) and got["count"][p] == one["count"][0]
        q0 += len(c["A"])


# ---- the modules -------------------------------------------------------------------------------------------------------------------------------------
def test_overall_loss_autograd_wiring(gold):
    """OverallLoss_new(...)['loss'].backward() fills .grad on leaf score and node tensors with the restatement's gradients; vote_mask gives
    the reference's mask vectors; the list form returns the same bytes per pair."""
    c, r = R.cached("overall")
    o = R.as_tensors(c, device=DEV)
    vp, va = L.vote_mask(o["ori_pos_points_c"], o["ori_anc_points_c"], o["transform"], R.CORRES_RADIUS)
    assert np.array_equal(vp.cpu().numpy(), gold["overall_mask_pos"]) and np.array_equal(va.cpu().numpy(), gold["overall_mask_anc"])
    o["mask"] = (vp, va)
    loss = L.OverallLoss_new(make_cfg())
    res = loss(o, {"transform": o["transform"]})
    assert list(res) == gold["overall_keys"].tolist()
    res["loss"].backward()
    for k, v in res.items():
        e_ref = abs(r["losses"][k] - float(gold["overall_" + k]))
        e = abs(float(v.detach()) - r["losses"][k])
        print("overall %s: %.3g (bound %.3g, e_ref %.3g)" % (k, e, R.bound(e_ref, r["losses"][k]), e_ref))
        assert e <= R.bound(e_ref, r["losses"][k]), k
    for k in R.GRAD_KEYS:
        e_ref = R.err(r["grads"][k], gold["overall_grad_" + k])
        e = R.err(o[k].grad.cpu().numpy(), r["grads"][k])
        print("overall d loss / d %s: %.3g (bound %.3g, e_ref %.3g)" % (k, e, R.bound(e_ref, r["grads"][k]), e_ref))
        assert e <= R.bound(e_ref, r["grads"][k]), k
    # the full (M, N) mask is accepted too; a mask of the wrong size raises
    full = R.as_tensors(c, device=DEV, grad=False)
    full["mask"] = vp[:, None] & va[None, :]
    assert float(L.VoteLoss_new(make_cfg()["Vote"])(full, {"transform": full["transform"]})) == float(res["v_loss"].detach()) / 0.25
    full["mask"] = (vp[:-1], va)
    with pytest.raises(RuntimeError):
        L.VoteLoss_new(make_cfg()["Vote"])(full, {"transform": full["transform"]})
    # two pairs of different sizes in one call
    c2 = R.overall_case(seed=1, n_pos=17, n_anc=29, B=4, N=9, M=14)
    o1, o2 = R.as_tensors(c, device=DEV, grad=False), R.as_tensors(c2, device=DEV, grad=False)
    o1["mask"] = (vp, va)
    o2["mask"] = L.vote_mask(o2["ori_pos_points_c"], o2["ori_anc_points_c"], o2["transform"], R.CORRES_RADIUS)
    both = loss([o1, o2], {"transform": torch.stack([o1["transform"], o2["transform"]])})
    assert len(both) == 2
    for pair, alone in zip(both, (loss(o1, {"transform": o1["transform"]}), loss(o2, {"transform": o2["transform"]}))):
        for k in ("c_loss", "g_loss", "v_loss", "d_loss", "n_loss", "reg_loss"):
            assert float(pair[k]) == float(alone[k]), k
    want2 = R.overall(R.as_tensors(c2, grad=False), mask=tuple(m.cpu() for m in o2["mask"]))
    for k in ("c_loss", "g_loss"):
        assert abs(float(both[1][k]) - float(want2[k])) <= R.bound(0, float(want2[k])), k


def test_end_to_end_on_the_model_outputs():
    """Seeded-weight LCRNet_Matching.forward_pairs on the two demo pairs of tests/test_matching_models_gpu.py -> OverallLoss_new with
    vote_mask: the native result equals the restatement on the same dicts.  No claim about the value (no trained checkpoint).
    Bounds: the gap terms and the torch terms to the floor of the rule (2^-20 relative); the two distance terms additionally carry the
    fp32 rounding of the transformed anc nodes the kernel is given — three roundings of a coordinate of magnitude X, 3 * 2^-24 * X per
    axis, sqrt(3) of that in a distance — which the fp64 restatement does not have."""
    from conftest import GOLDEN, LIMITS, NUM_STAGES, RADIUS, VOXEL, load_scan
    from oracle import ops as oracle_ops
    from lcrnet_amd.model_family import LCRNet_Matching
    from lcrnet_amd.weights import seeded_state_dict
    a, b = load_scan("003854"), load_scan("000958")
    st = oracle_ops.precompute_data_stack_mode(np.concatenate([a, b, b, a]), np.array([len(a), len(b), len(b), len(a)]), NUM_STAGES, VOXEL, RADIUS, LIMITS)
    dd = {k: [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in v] for k, v in st.items()}
    dd["features"] = torch.ones(2 * (len(a) + len(b)), 1, device=DEV)
    T = torch.from_numpy(np.load(os.path.join(GOLDEN, "matching_golden.npz"))["transform"]).float()
    dd["transform"] = torch.stack([T, torch.linalg.inv(T.double()).float()]).cuda()
    cfg = make_cfg()
    cfg["neighbor_limits"] = LIMITS
    m = LCRNet_Matching.create_model(cfg).eval()
    m.load_state_dict(seeded_state_dict(m.state_dict(), json.load(open(os.path.join(GOLDEN, "model_manifest.json")))["seed"]), strict=True)
    with torch.no_grad():
        outs = m.cuda().forward_pairs(dd)
    assert len(outs) == 2
    for p, o in enumerate(outs):
        o["mask"] = L.vote_mask(o["ori_pos_points_c"], o["ori_anc_points_c"], dd["transform"][p], cfg["model"]["ground_truth_corres_radius"])
    got = L.OverallLoss_new(cfg)(outs, {"transform": dd["transform"]})
    keys = ("matching_scores", "pos_node_corr_knn_points", "anc_node_corr_knn_points", "pos_node_corr_knn_masks", "anc_node_corr_knn_masks",
            "node_matching_scores", "gt_node_corr_indices", "gt_node_corr_overlaps", "pos_node_masks", "anc_node_masks", "shifted_pos_points_c",
            "shifted_anc_points_c", "pos_points_f", "anc_points_f", "pos_points_c", "anc_points_c", "score", "pos_emb", "anc_emb")
    for p, o in enumerate(outs):
        oc = {k: o[k].detach().cpu() for k in keys}
        oc["transform"] = dd["transform"][p].cpu()
        want = R.overall(oc, mask=tuple(v.cpu() for v in o["mask"]))
        X = max(float(o[k].abs().max()) for k in ("shifted_pos_points_c", "shifted_anc_points_c", "pos_points_f", "anc_points_f"))
        moved_err = 3 * 2.0 ** -24 * X * np.sqrt(3.0)
        for k, v in got[p].items():
            w = float(want[k])
            reg_err = 2.0 ** -23 * max(float(o["pos_emb"].abs().max()), float(o["anc_emb"].abs().max()))
            tol = R.bound(0, w) + {"v_loss": 2 * 0.25 * moved_err, "reg_loss": reg_err,
                                   "loss": 2 * 0.25 * moved_err + reg_err + 6 * 2.0 ** -20 * abs(w)}.get(k, 0.0)
            print("pair %d %s: native %.7g restated %.7g |diff| %.3g (bound %.3g)" % (p, k, float(v), w, abs(float(v) - w), tol))
            assert abs(float(v) - w) <= tol or (np.isnan(w) and np.isnan(float(v))), (p, k)
