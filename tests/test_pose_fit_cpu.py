"""CPU: what tests/test_pose_fit_gpu.py rests on, shown without a GPU.

  * The unmutated fp64 restatement (tests/pose_fit_restatement.py) is pinned to oracle.torch_ref run in fp64 — weighted_procrustes, greedy_nms
    and local_global_registration fed the same correspondences — to 1e-10 on the well-conditioned cases, and to closed-form answers where
    torch_ref cannot run a case (zero scores cannot be planted as correspondences; the vote shift and the neighbour mean have no oracle entry).
  * The fp32 floor of every operator (the same restatement on float32 inputs, sums in plain index order) is recomputed over every GPU case
    and held within 2x of the committed FLOOR constants; TOL = min(1e-4, 4 FLOOR) x max(1, |want|max).
  * The margins that make exact integer comparisons legitimate: no fp64 residual within DELTA of the radius (inlier and LGR cases), no
    pairwise distance within 1e-3 of the NMS radius; at least 100 NMS points with more than 24 lower-index in-range neighbours; the tie run
    of the quantised scores straddles rows 256 and 512 and the cut falls inside it.
  * Every planted mutation moves the fp64 result by >= 20 TOL, or changes an integer output, on a case assigned to it.
"""
import contextlib

import numpy as np
import pytest
import torch

import pose_fit_restatement as pr
from oracle import torch_ref

PIN = 1e-10


@contextlib.contextmanager
def fp64_default():
    """torch_ref builds its identity matrices in the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def rel_err(got, want):
    want = np.asarray(want, np.float64)
    return pr.shift_of(got, want) / max(1.0, float(np.abs(want).max()) if want.size else 0.0)


# ------------------------------------------------------------------------------------------------ pinning
@pytest.mark.parametrize("geometry,weights", [("generic", "uniform"), ("generic", "random"), ("generic", "negative"), ("pi", "uniform"),
                                              ("mirrored", "random"), ("planar", "uniform"), ("far100", "tiny_sum")])
def test_procrustes_pinned_to_torch_ref(geometry, weights):
    c = pr.procrustes_case(geometry, weights)
    got = pr.procrustes_reference(geometry, weights)
    worst = 0.0
    with fp64_default():
        for p in np.flatnonzero(pr.unique_chunks(c)):
            a, b = c["start"][p], c["start"][p + 1]
            want = torch_ref.weighted_procrustes(t64(c["src"][a:b]), t64(c["ref"][a:b]), t64(c["w"][a:b])).numpy()
            worst = max(worst, pr.shift_of(got[p], want))
    print(f"pose_fit pin procrustes {geometry} {weights}: {worst:.3e}")
    assert worst <= PIN


def test_procrustes_zero_and_deficient_closed_form():
    """H == 0 (no rows, or all weights zero): the identity with t = 0, as torch.svd of a zero matrix gives.  One row: any rotation that maps
    s to r is a best fit; the restatement's is proper and has residual (1 - 1 / (1 + eps)) |r - R s| of the shrunk centroids at most."""
    with fp64_default():
        assert torch.equal(torch_ref.weighted_procrustes(torch.zeros(4, 3), torch.ones(4, 3), torch.zeros(4)), torch.eye(4))
    for geometry in pr.GEOMETRIES:
        c = pr.procrustes_case(geometry, "zero")
        assert all(k == "zero" for k in c["kind"])
        assert np.array_equal(pr.procrustes_reference(geometry, "zero"), np.tile(np.eye(4), (len(pr.CHUNKS), 1, 1)))
    for geometry, weights in pr.procrustes_case_names():
        c, T = pr.procrustes_case(geometry, weights), pr.procrustes_reference(geometry, weights)
        assert np.isfinite(T).all() and np.array_equal(T[:, 3], np.tile([0.0, 0, 0, 1], (len(T), 1)))
        R = T[:, :3, :3]
        assert np.abs(np.einsum("pji,pjk->pik", R, R) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12
        assert c["kind"][0] == "zero" and np.array_equal(T[0], np.eye(4))          # the empty chunk


def _lgr_inputs_for_torch_ref(c):
    """Patch tensors from which torch_ref.local_global_registration derives exactly the rows of the single-pair case c, in order: chunk b's rows
    sit on the diagonal of patch b's score matrix (use_dustbin=False, threshold 0: a row is a correspondence iff its score is > 0)."""
    hs = c["hyp_start"]
    B, K = len(hs) - 1, int(np.diff(hs).max())
    refp, srcp = np.zeros((B, K, 3)), np.zeros((B, K, 3))
    S = np.zeros((B, K + 1, K + 1))
    for b in range(B):
        m = hs[b + 1] - hs[b]
        refp[b, :m], srcp[b, :m] = c["ref"][hs[b]:hs[b + 1]], c["src"][hs[b]:hs[b + 1]]
        S[b, np.arange(m), np.arange(m)] = c["score"][hs[b]:hs[b + 1]]
    with np.errstate(divide="ignore"):
        return t64(refp), t64(srcp), torch.ones(B, K, dtype=torch.bool), torch.ones(B, K, dtype=torch.bool), t64(np.log(S))


@pytest.mark.parametrize("name,s", [("branches", 0), ("branches", 1), ("branches", 2), ("limit", 0), ("limit", 1)])
@pytest.mark.parametrize("steps", pr.LGR_STEPS)
def test_lgr_pinned_to_torch_ref(name, s, steps):
    c = pr.lgr_pair_alone(pr.lgr_case(name), s)
    assert (c["score"] > 0).all()
    with fp64_default():
        rp, sp, sc, want = torch_ref.local_global_registration(*_lgr_inputs_for_torch_ref(c), acceptance_radius=c["radius"], threshold=c["min_count"],
                                                               steps=steps, use_dustbin=False, correspondence_limit=c["limit"] or None)
    assert np.array_equal(sp.numpy(), c["src"]) and np.array_equal(rp.numpy(), c["ref"]) and pr.shift_of(sc, c["score"]) < 1e-15
    T, _, _, best = pr.lgr_of(c, steps)
    err = pr.shift_of(T[0], want.numpy())
    print(f"pose_fit pin lgr {name} pair {s} steps {steps}: {err:.3e} (best {best[0]})")
    assert err <= PIN
    # and the stacked form of the restatement gives each pair what it gives alone
    assert np.array_equal(pr.lgr_reference(name, steps)[0][s], T[0])


def test_lgr_branches_are_the_intended_ones():
    for steps in pr.LGR_STEPS:
        T, hyp, counts, best = pr.lgr_reference("branches", steps)
        c = pr.lgr_case("branches")
        ss, ln = c["seg_hyp_start"], np.diff(c["hyp_start"])
        assert best[0] >= 0 and counts[best[0]] > 50 and (ln[ss[0]:ss[1]] == 0).any()                       # a: a real winner, an empty chunk
        assert best[1] == -1 and (counts[ss[1]:ss[2]] == -1).all() and np.abs(T[1] - np.eye(4)).max() > 0.1   # b: the fit over all rows
        assert best[2] == ss[2] and (counts[ss[2]:ss[3]] <= 0).all() and np.array_equal(T[2], np.eye(4))      # c: no inlier -> the identity
        assert np.array_equal(counts == -1, ln < c["min_count"])


def test_nms_pinned_to_torch_ref():
    for name in ("stack", "edge"):
        c = pr.nms_case(name)
        keep, out_len = pr.nms_reference(name)
        wmask, wlen = torch_ref.greedy_nms(t64(c["pts"]), torch.from_numpy(c["lens"]), c["radius"])
        assert np.array_equal(keep, wmask.numpy()) and np.array_equal(out_len, wlen.numpy())
    keep, out_len = pr.nms_reference("edge")
    assert out_len.tolist() == [1, 150] and keep[0] and not keep[1:200].any()
    assert np.array_equal(keep[200:], np.arange(300) % 2 == 0)                    # the chain: decisions alternate


def test_vote_shift_and_neighbor_mean_closed_form():
    c = pr.vote_case(257)
    got = pr.vote_shift(c["xyz"], c["off"], c["max_range"])
    assert np.isfinite(got).all()
    moved = np.linalg.norm(got - c["xyz"], axis=1)
    length = np.linalg.norm(c["off"], axis=1)
    assert (moved <= c["max_range"] * (1 + 1e-12)).all() and (length > 1e17).sum() == 2 and (length == 0).sum() == 1
    assert np.array_equal(got[length <= c["max_range"]], (c["xyz"] + c["off"])[length <= c["max_range"]])
    assert (length == c["max_range"]).sum() == 2 and ((length > c["max_range"]) & (length < c["max_range"] * 1.001)).sum() == 2
    far = length > c["max_range"]
    assert np.abs(moved[far] - c["max_range"]).max() < 1e-9 * 20          # |xyz| ~ 20: the difference xyz + v - xyz rounds at that size
    for M in pr.NM_MS:
        for H in pr.NM_HS:
            c = pr.neighbor_case(M, H)
            got = pr.neighbor_mean(c["pts"], c["idx"], c["pad"])
            padded = np.concatenate([c["pts"], np.zeros((1, 3))])
            valid = (c["idx"] >= 0) & (c["idx"] < c["pad"])
            with np.errstate(invalid="ignore", divide="ignore"):
                want = padded[np.where(valid, c["idx"], c["pad"])].sum(1) / valid.sum(1, keepdims=True)
            none = ~valid.any(1)
            assert np.isnan(got[none]).all() and pr.shift_of(got[~none], want[~none]) < 1e-12
            if M == 257:
                assert none.sum() >= 30 and (c["idx"] > c["pad"]).any() and (c["idx"] == c["pad"]).any() and (c["idx"] == -1).any()


def test_top_l_closed_form():
    """The quantised scores cannot go through torch_ref (zero scores are no correspondences): the answer is known in closed form."""
    c = pr.lgr_pair_alone(pr.lgr_case("limit"), 2)
    sc = c["score"]
    assert len(sc) == 700 and (sc == 0).sum() == 60 and ((sc > 0) & (sc < 1.2e-38)).sum() == 60 and (sc >= 0).all()
    ties = np.flatnonzero(sc == 0.5)
    assert (sc > 0.5).sum() == 100 and len(ties) == 400
    want = sc > 0.5
    want[ties[:200]] = True
    assert np.array_equal(pr.top_l(sc, pr.LIMIT), want)
    # the tie run straddles rows 256 and 512, and so does the admitted part of it straddle 256: the rank carried between passes decides
    cut = ties[199]
    assert (ties < 256).sum() > 0 and ((ties >= 256) & (ties < 512)).sum() > 0 and (ties >= 512).sum() > 0 and 256 < cut < 512
    assert 0 < (ties < 256).sum() < 200
    for n, lim in ((5, 5), (5, 7), (6, 5)):
        s = np.array([0.5, 0.25, 0.5, 1.0, 0.5, 0.5][:n])
        assert pr.top_l(s, lim).sum() == min(n, lim)
    assert pr.top_l(np.array([0.5, 0.25, 0.5, 1.0, 0.5, 0.5]), 3).tolist() == [True, False, True, True, False, False]
    sizes = np.diff(pr.lgr_case("limit")["hyp_start"][pr.lgr_case("limit")["seg_hyp_start"]])
    assert sizes.tolist() == [120, pr.LIMIT + 1, 700]


# ------------------------------------------------------------------------------------------------ the fp32 floor
def _f32(c):
    return pr.cast(c, np.float32)


def measured_floors():
    out = dict.fromkeys(pr.FLOOR, 0.0)
    for geometry, weights in pr.procrustes_case_names():
        c = pr.procrustes_case(geometry, weights)
        u = pr.unique_chunks(c)
        if u.any():
            f = _f32(c)
            got = pr.procrustes(f["src"], f["ref"], f["w"], f["start"])
            want = pr.procrustes_reference(geometry, weights)[u]
            out["procrustes_R"] = max(out["procrustes_R"], rel_err(got[u][:, :3, :3], want[:, :3, :3]))
            out["procrustes_t"] = max(out["procrustes_t"], rel_err(got[u][:, :3, 3], want[:, :3, 3]))
    for name in pr.LGR_STACKS:
        c = pr.lgr_case(name)
        valid = np.diff(c["hyp_start"]) >= c["min_count"]
        for steps in pr.LGR_STEPS:
            T, hyp, counts, best = pr.lgr_reference(name, steps)
            T32, hyp32, counts32, best32 = pr.lgr_of(_f32(c), steps)
            assert np.array_equal(counts, counts32) and np.array_equal(best, best32)
            out["lgr_hyp"] = max(out["lgr_hyp"], rel_err(hyp32[valid], hyp[valid]))
            out["lgr_T"] = max(out["lgr_T"], rel_err(T32, T))
    for N in pr.VOTE_NS:
        c = pr.vote_case(N)
        f = _f32(c)
        out["vote_shift"] = max(out["vote_shift"], rel_err(pr.vote_shift(f["xyz"], f["off"], np.float32(c["max_range"])),
                                                           pr.vote_shift(c["xyz"], c["off"], c["max_range"])))
    for M in pr.NM_MS:
        for H in pr.NM_HS:
            c = pr.neighbor_case(M, H)
            want = pr.neighbor_mean(c["pts"], c["idx"], c["pad"])
            got = pr.neighbor_mean(c["pts"].astype(np.float32), c["idx"], c["pad"])
            ok = np.isfinite(want).all(1)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            out["neighbor_mean"] = max(out["neighbor_mean"], rel_err(got[ok], want[ok]))
    return out


def test_fp32_floor_matches_committed_constant():
    got = measured_floors()
    for k, v in got.items():
        print(f"pose_fit floor {k}: measured {v:.3e} committed {pr.FLOOR[k]:.3e} TOL {pr.TOL[k]:.3e}")
    for k, v in got.items():
        assert pr.FLOOR[k] / 2 <= v <= 2 * pr.FLOOR[k], (k, v, pr.FLOOR[k])
        assert pr.TOL[k] == min(pr.NORTH_STAR, pr.MARGIN * pr.FLOOR[k])


# ------------------------------------------------------------------------------------------------ margins
def test_inlier_margin():
    cases = [pr.inlier_case(n, P) for n in pr.INLIER_NS for P in pr.INLIER_PS] + [pr.chunked_inlier_case(k) for k in pr.CHUNKED]
    for c in cases:
        assert max(np.abs(c["src"]).max(initial=0), np.abs(c["ref"]).max(initial=0)) <= 20
        assert pr.radius_margin([pr.residual(c["T"], c["src"], c["ref"])], c["radius"]) > pr.DELTA
    e = pr.exact_inlier_case()
    res = pr.residual(e["T"], e["src"], e["ref"])[0]
    assert np.array_equal(res[::2], np.full(30, 0.5)) and np.array_equal(res[1::2], np.full(30, 0.25))   # exactly at the radius / inside
    assert pr.inlier_count(e["T"], e["src"], e["ref"], e["radius"])[0].tolist() == [30]
    c = pr.chunked_inlier_case("counted")
    counts, best = pr.inlier_count(c["T"], c["src"], c["ref"], c["radius"], c["start"], c["min_count"])
    assert counts[0] == -1 and counts[1] == counts[2] > 0 and best == 1          # 2 rows: never; 3 rows: counts; equal tops: the first
    c = pr.chunked_inlier_case("all_short")
    counts, best = pr.inlier_count(c["T"], c["src"], c["ref"], c["radius"], c["start"], c["min_count"])
    assert counts.tolist() == [-1, -1, -1] and best == 0
    c = pr.inlier_case(1000, 7)
    counts, best = pr.inlier_count(c["T"], c["src"], c["ref"], c["radius"])
    assert counts[2] == counts[5] == counts.max() and best == 2


@pytest.mark.parametrize("name", tuple(pr.LGR_STACKS))
def test_lgr_margin_and_structure(name):
    c = pr.lgr_case(name)
    assert np.abs(c["src"]).max() <= 20 and np.abs(c["ref"]).max() <= 20 and (c["score"] >= 0).all()
    trace = []
    for steps in pr.LGR_STEPS:
        pr.lgr_of(c, steps, trace=trace)
    margin = pr.radius_margin(trace, c["radius"])
    print(f"pose_fit lgr {name}: {sum(t.size for t in trace)} residuals, nearest to the radius {margin:.3e}")
    assert margin > pr.DELTA
    if name == "branches":                          # pair a as specified: 60 % within 0.25 x radius of a motion, the rest >= 3 x radius away
        a = pr.lgr_pair_alone(c, 0)
        T, _, _, _ = pr.lgr_of(a, 5)
        res = pr.residual(T[0], a["src"], a["ref"])
        assert 0.5 < (res < 0.3 * c["radius"]).mean() < 0.7 and ((res < 0.3 * c["radius"]) | (res > 2.7 * c["radius"])).all()
        ln = np.diff(a["hyp_start"])
        assert ln.min() == 0 and ln.max() == 40 and 1 in ln


@pytest.mark.parametrize("name", ("stack", "edge"))
def test_nms_margin_and_crowding(name):
    c = pr.nms_case(name)
    assert np.array_equal(c["pts"] * 8, np.round(c["pts"] * 8))
    margin, crowded = pr.nms_facts(c["pts"], c["lens"], c["radius"])
    print(f"pose_fit nms {name}: nearest distance to the radius {margin:.3e}, {crowded} points with > 24 lower in-range neighbours")
    assert margin > pr.NMS_DELTA
    if name == "stack":
        assert np.abs(c["pts"]).max() <= 64 and crowded >= 100 and c["lens"].tolist() == [0, 1, 1023, 1024, 1025, 2500]
        _, out_len = pr.nms_reference(name)
        assert out_len[0] == 0 and out_len[1] == 1 and (out_len[2:] < c["lens"][2:]).all()


# ------------------------------------------------------------------------------------------------ planted mutations
PROCRUSTES_ASSIGNED = {"no_eps": ("far100", "tiny_sum"), "negative_kept": ("generic", "negative"), "renormalised_centroid": ("far100", "tiny_sum"),
                       "no_reflection_fix": ("mirrored", "uniform"), "reflection_on_largest": ("mirrored", "uniform"), "u_vt": ("generic", "uniform"),
                       "t_without_R": ("generic", "random"), "rows_past_64_dropped": ("late", "uniform")}


@pytest.mark.parametrize("mutation", pr.MUTATIONS["procrustes"])
def test_procrustes_mutation_is_caught(mutation):
    geometry, weights = PROCRUSTES_ASSIGNED[mutation]
    u = pr.unique_chunks(pr.procrustes_case(geometry, weights))
    want = pr.procrustes_reference(geometry, weights)[u]
    with np.errstate(all="ignore"):
        (eR, bR), (et, bt) = pr.pose_errors(pr.procrustes_reference(geometry, weights, mutation)[u], want)
    print(f"pose_fit mutation {mutation} on {geometry} {weights}: R moves by {eR / bR:.1f} TOL, t by {et / bt:.1f} TOL")
    assert max(eR / bR, et / bt) >= pr.SENSITIVITY


@pytest.mark.parametrize("mutation", pr.MUTATIONS["inlier"])
def test_inlier_mutation_changes_an_integer(mutation):
    if mutation == "le_instead_of_lt":
        c, kw = pr.exact_inlier_case(), {}
    elif mutation == "le_min_count":
        c = pr.chunked_inlier_case("counted")
        kw = {"start": c["start"], "min_count": c["min_count"]}
    else:
        c, kw = pr.inlier_case(1000, 7), {}
    counts, best = pr.inlier_count(c["T"], c["src"], c["ref"], c["radius"], **kw)
    mcounts, mbest = pr.inlier_count(c["T"], c["src"], c["ref"], c["radius"], mutate=mutation, **kw)
    assert not np.array_equal(counts, mcounts) or best != mbest


@pytest.mark.parametrize("mutation", pr.MUTATIONS["lgr"])
def test_lgr_mutation_is_caught(mutation):
    name, steps = {"counts_over_all_rows": ("branches", 5), "hyp_from_verification": ("limit", 5), "refit_unmasked": ("limit", 5),
                   "one_step_fewer": ("branches", 1)}[mutation]
    T, hyp, counts, best = pr.lgr_reference(name, steps)
    mT, mhyp, mcounts, mbest = pr.lgr_reference(name, steps, mutation)
    valid = counts >= 0
    sT, sh = pr.shift_of(mT, T) / pr.bound_of("lgr_T", T), pr.shift_of(mhyp[valid], hyp[valid]) / pr.bound_of("lgr_hyp", hyp[valid])
    integers = not np.array_equal(counts, mcounts) or not np.array_equal(best, mbest)
    print(f"pose_fit mutation {mutation} on {name} steps {steps}: T {sT:.1f} TOL, hyp {sh:.1f} TOL, integers changed: {integers}")
    assert integers or max(sT, sh) >= pr.SENSITIVITY


@pytest.mark.parametrize("mutation", pr.MUTATIONS["top_l"])
def test_top_l_mutation_changes_the_set(mutation):
    sc = pr.lgr_pair_alone(pr.lgr_case("limit"), 2)["score"]
    assert not np.array_equal(pr.top_l(sc, pr.LIMIT), pr.top_l(sc, pr.LIMIT, mutation))


@pytest.mark.parametrize("mutation", pr.MUTATIONS["nms"])
def test_nms_mutation_changes_the_mask(mutation):
    keep, out_len = pr.nms_reference("stack")
    mkeep, mlen = pr.nms_reference("stack", mutation)
    assert not np.array_equal(keep, mkeep) and not np.array_equal(out_len, mlen)


def test_neighbor_mean_mutation_is_caught():
    c = pr.neighbor_case(257, 20)
    want = pr.neighbor_mean(c["pts"], c["idx"], c["pad"])
    ok = np.isfinite(want).all(1)
    shift = pr.shift_of(pr.neighbor_mean(c["pts"], c["idx"], c["pad"], "divide_by_H")[ok], want[ok])
    assert shift >= pr.SENSITIVITY * pr.bound_of("neighbor_mean", want[ok])
