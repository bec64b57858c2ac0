"""CPU: tests/matching_restatement.py guarded against being wrong itself, and its cases against being vacuous.  No GPU, no kernel: what
tests/test_matching_gpu.py compares csrc/matching.hip with is checked here against

  * a deliberately naive per-line loop (pick the best remaining entry K times) on the small shapes, every switch;
  * oracle/torch_ref.superpoint_matching_ot (superpoint_matching.py:130-162) for K = 1, one problem, no masks, on every shape;
  * the correspondence part of oracle/torch_ref.local_global_registration (local_global_registration.py:48-93, :236-237) for every switch,
    read back through index-coded points (ref_knn_pts[b, i] = (b, i, 0), src_knn_pts[b, j] = (b, j, 1)),

and the generator against its own promises: every planted tie is where make_case says it is, the zero-pair problems give zero pairs, the
K-th element of a line does fall inside a run of equal values, every case with min(M, N) >= 63 has row-side-only, column-side-only and
both-sides pairs (so neither the OR nor the AND of `mutual` can be dropped unseen) and `mutual` returns strictly fewer pairs."""
import numpy as np
import pytest
import torch

import matching_restatement as mr
from oracle import torch_ref

LEVELS = tuple(mr.LEVELS)


def _all_switches(case):
    N = case.shape[2]
    for K in mr.ks_for(N):
        for mutual in (0, 1):
            for dust, thr in mr.switches(case.level):
                for gs in (None, case.global_scores):
                    yield K, mutual, dust, thr, gs


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_planted_structures_are_there(shape, level):
    B, M, N = shape
    for mode in mr.MASK_MODES:
        c = mr.make_case(shape, level, mode)
        x, pl = c.logs, c.planted
        assert x.dtype == np.float32 and x.shape == (B, M + 1, N + 1)
        assert np.array_equal(x[x > -1e11] * 64, np.round(x[x > -1e11] * 64)), "every ordinary log is a multiple of 1/64"
        assert x.max() <= 0 and x[x > -1e11].min() > -20
        rv = c.row_mask[0] if c.row_mask is not None else np.ones(M, bool)
        cv = c.col_mask[0] if c.col_mask is not None else np.ones(N, bool)
        if c.row_mask is not None:
            assert c.row_mask[:, 0].all() and c.col_mask[:, 0].all()
            masked = (~c.row_mask[:, :, None] | ~c.col_mask[:, None, :])
            if mode == "inf":
                assert (x[:, :M, :N][masked] == mr.MASKED).all()
            else:
                keep = np.ones(B, bool)
                keep[list(c.zero_pair[:1])] = False
                assert (x[keep, :M, :N][masked[keep]] > -20).all(), "gate: masked lines keep ordinary values"
        i, cols = pl["row_max"]
        assert rv[i] and cv[list(cols)].all() and cols[0] == 0 and len(cols) == 1 + (N > 64) + (N > 128)
        rest = np.delete(x[0, i], list(cols))
        assert (x[0, i, list(cols)] == 0).all() and (rest.size == 0 or rest.max() < 0)
        if "col_max" in pl:
            j, rows = pl["col_max"]
            assert cv[j] and rv[list(rows)].all() and (x[0, list(rows), j] == 0).all() and np.delete(x[0, :, j], list(rows)).max() < 0
            assert rows[:2] == (1, 2) and (M <= 5 or rows == (1, 2, 5))
        assert ("col_max" in pl) == (M >= 3 and N >= 3)
        assert ("row_run" in pl) == ("col_run" in pl) == (M >= 40 and N >= 40)
        if "row_run" in pl:
            i, cols = pl["row_run"]
            j, rows = pl["col_run"]
            assert rv[i] and cv[list(cols)].all() and cv[j] and rv[list(rows)].all()
            assert (x[0, i, list(cols)] == -1 / 64).all() and np.delete(x[0, i], list(cols)).max() < -1 / 64
            assert (x[0, list(rows), j] == -1 / 64).all() and np.delete(x[0, :, j], list(rows)).max() < -1 / 64
        assert ("row_dust" in pl) == (M > 3) and ("col_dust" in pl) == (N > 4)
        if "row_dust" in pl:
            i = pl["row_dust"]
            assert rv[i] and x[0, i, N] == x[0, i, :N].max() > -20
        if "col_dust" in pl:
            j = pl["col_dust"]
            assert cv[j] and x[0, M, j] == x[0, :M, j].max() > -20
        assert bool(c.zero_pair) == (B == 3)
        if c.zero_pair:
            assert (x[1] == mr.MASKED).all()
            ok = np.ones((M, N), bool) if mode != "inf" else c.row_mask[2][:, None] & c.col_mask[2][None, :]   # an "inf" line ties with its dustbin
            assert (x[2, :M, :N] < x[2, :M, N:])[ok].all() and (x[2, :M, :N] < x[2, M:, :N])[ok].all()
            assert (x[2, :M, :N] <= x[2, :M, N:]).all() and (x[2, :M, :N] <= x[2, M:, :N]).all()
        assert c.global_scores.dtype == np.float32 and c.global_scores.min() >= 0.5 and c.global_scores.max() <= 2
        lo, hi = np.exp(-np.array([3, 101]) / 64), np.exp(-np.array([2, 100]) / 64)
        t = c.positive_threshold
        assert (lo[0] < t < hi[0]) if level == "coarse" else (lo[1] < t < hi[1])


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_exp_levels_cannot_be_confused_by_one_ulp(shape, level):
    """The premise of the exact comparison: two different values of P in one case differ by more than 1 %, a thousand times what any fp32 exp
    can be off by, and no value of P lies within 1 % of a positive threshold."""
    c = mr.make_case(shape, level, "inf")
    v = np.unique(np.exp(c.logs.astype(np.float64)).astype(np.float32))
    v = v[v > 0]
    assert len(v) >= 2 or shape[1] * shape[2] == 1
    assert (v[1:] / v[:-1] > 1.01).all()
    assert (np.abs(v / np.float32(c.positive_threshold) - 1) > 0.005).all()


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", mr.SMALL_SHAPES + [(3, 63, 64)], ids=mr.shape_id)
def test_restatement_equals_naive_loop(shape, level):
    n = 0
    for mode in mr.MASK_MODES:
        c = mr.make_case(shape, level, mode)
        if shape in mr.SMALL_SHAPES:
            logs, rm, cm, gsv, sw = c.logs, c.row_mask, c.col_mask, c.global_scores, list(_all_switches(c))
        else:                                                        # problem 0 (every planted tie is in it), a cut of the switches
            logs, gsv = c.logs[:1], c.global_scores[:1]
            rm, cm = (None, None) if c.row_mask is None else (c.row_mask[:1], c.col_mask[:1])
            sw = [(K, mutual, dust, thr, gsv) for K in (1, 2, 3, shape[2] + 1) for mutual in (0, 1) for dust, thr in mr.switches(level)[::3]]
        m = mr.Matcher(logs)
        for K, mutual, dust, thr, gs in sw:
            gs = None if gs is None else gsv
            bij, sc = m.match(rm, cm, K, mutual, dust, thr, gs)
            nb, ns = mr.naive_match(logs, rm, cm, K, mutual, dust, thr, gs)
            assert np.array_equal(bij, nb) and np.array_equal(sc, ns), (mode, K, mutual, dust, thr)
            assert bij.dtype == np.int32 and sc.dtype == np.float64
            n += len(bij)
    assert n > 0
    fb, fs = mr.match(logs, rm, cm, 2, 0, 1, 0.0, None)              # the one-call form is the same thing
    wb, ws = m.match(rm, cm, 2, 0, 1, 0.0, None)
    assert np.array_equal(fb, wb) and np.array_equal(fs, ws)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_top1_equals_superpoint_matching_ot(shape, level):
    c = mr.make_case(shape, level, "none")
    for b in sorted({0, shape[0] - 1}):
        ri, ci, sc = torch_ref.superpoint_matching_ot(torch.from_numpy(c.logs[b]))
        bij, want = mr.match(c.logs[b:b + 1], None, None, 1, 0, 1, 0.0, None)
        assert np.array_equal(bij[:, 1], ri.numpy()) and np.array_equal(bij[:, 2], ci.numpy()) and (bij[:, 0] == 0).all()
        assert len(bij) == 0 or np.abs(sc.numpy() - want).max() <= mr.SCORE_TOL
        if b not in c.zero_pair:
            assert len(bij) > 0


def _reference_rows(c, K, mutual, dust, thr, gs):
    B, M, N = c.shape
    ref_pts = torch.zeros(B, M, 3)
    src_pts = torch.ones(B, N, 3)
    ref_pts[:, :, 0] = src_pts[:, :, 0] = torch.arange(B, dtype=torch.float32)[:, None]
    ref_pts[:, :, 1] = torch.arange(M, dtype=torch.float32)[None]
    src_pts[:, :, 1] = torch.arange(N, dtype=torch.float32)[None]
    rm = torch.ones(B, M, dtype=torch.bool) if c.row_mask is None else torch.from_numpy(c.row_mask)
    cm = torch.ones(B, N, dtype=torch.bool) if c.col_mask is None else torch.from_numpy(c.col_mask)
    rp, sp, sc, _ = torch_ref.local_global_registration(ref_pts, src_pts, rm, cm, torch.from_numpy(c.logs), steps=1, mutual=bool(mutual), topk=K,
                                                        use_dustbin=bool(dust), confidence_threshold=thr,
                                                        global_scores=None if gs is None else torch.from_numpy(gs))
    rp, sp = rp.numpy(), sp.numpy()
    assert (rp[:, 2] == 0).all() and (sp[:, 2] == 1).all() and np.array_equal(rp[:, 0], sp[:, 0])
    return np.stack([rp[:, 0], rp[:, 1], sp[:, 1]], 1).astype(np.int32), sc.numpy()


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_equals_the_oracles_local_global_registration(shape, level):
    """Every switch against oracle/torch_ref.py:398-423.  The cross product is cut to what keeps the file quick (the oracle fits poses after
    the part that is compared): every K with the dustbin form, K = 1 / 3 / N + 1 with the threshold forms, masks "inf" and "gate" in turn,
    global scores on every other call."""
    B, M, N = shape
    n = t = 0
    for mode in mr.MASK_MODES:
        c = mr.make_case(shape, level, mode)
        if B > 8:                                                    # problems are independent: the first eight of the B = 64 cases
            c.logs, c.global_scores, c.shape = c.logs[:8], c.global_scores[:8], (8, M, N)
            if c.row_mask is not None:
                c.row_mask, c.col_mask = c.row_mask[:8], c.col_mask[:8]
        m = mr.Matcher(c.logs)
        for K in mr.ks_for(N):
            for dust, thr in mr.switches(level):
                if not dust and K not in (1, 3, N + 1):
                    continue
                if not dust and thr < 0 and B * M * N > 20000 and K != 3:
                    continue                                         # every valid pair is returned: one such call per large case is enough
                for mutual in (0, 1):
                    t += 1
                    gs = c.global_scores if t % 2 else None
                    bij, sc = m.match(c.row_mask, c.col_mask, K, mutual, dust, thr, gs)
                    if len(bij) == 0:
                        continue                                     # the oracle's pose fit needs a pair; zero-pair problems are checked below
                    rb, rs = _reference_rows(c, K, mutual, dust, thr, gs)
                    assert np.array_equal(bij, rb), (mode, K, mutual, dust, thr)
                    assert np.abs(rs - sc).max() <= mr.SCORE_TOL * max(1.0, float(c.global_scores.max()))
                    n += 1
    assert n >= 20 or M * N < 8


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("shape", [s for s in mr.SHAPES if s[0] == 3], ids=mr.shape_id)
def test_zero_pair_problems_give_zero_pairs(shape, level):
    for mode in mr.MASK_MODES:
        c = mr.make_case(shape, level, mode)
        m = mr.Matcher(c.logs)
        for K in mr.ks_for(shape[2]):
            for mutual in (0, 1):
                bij, _ = m.match(c.row_mask, c.col_mask, K, mutual, 1, 0.0, None)
                assert len(bij) > 0 or shape[1] * shape[2] == 1
                assert not np.isin(bij[:, 0], c.zero_pair).any(), (mode, K, mutual)
        z = mr.Matcher(c.logs[1:])                                   # a call that holds nothing else
        assert len(z.match(None, None, 1, 0, 1, 0.0, None)[0]) == 0
        # without the dustbin the all-masked problem still has its zeros: above a negative threshold, not above 0
        assert len(z.match(None, None, 1, 0, 0, -1.0, None)[0]) == 2 * shape[1] * shape[2]
        assert not (z.match(None, None, 1, 0, 0, 0.0, None)[0][:, 0] == 0).any()


@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_dustbin_entry_of_a_line_cannot_change_what_the_line_keeps(shape):
    """Why no case can tell whether the dustbin row takes part in a COLUMN's selection (or the dustbin column in a row's) in the dustbin form:
    the dustbin has the line's largest index, so an interior entry that it pushes out of the first K comes after it in the stable order, is
    therefore strictly smaller, and fails the strict dustbin comparison anyway.  (A kernel that walks M rows where it should walk M + 1 is an
    equivalent mutant; the calibration of tests/test_matching_gpu.py found it passing and this is the reason.)"""
    for level in LEVELS:
        c = mr.make_case(shape, level, "gate")
        m = mr.Matcher(c.logs)
        P = m.P
        rr, rc = mr._ranks(P[:, :, :-1], 2), mr._ranks(P[:, :-1, :], 1)
        for K in mr.ks_for(shape[2]):
            ref, src = m.sides(K, 1, 0.0)
            assert np.array_equal(ref, ((rr < K) & (P[:, :, :-1] > P[:, :, -1:]))[:, :-1])
            assert np.array_equal(src, ((rc < K) & (P[:, :-1, :] > P[:, -1:, :]))[:, :, :-1])


def _kinds_cases(shape):
    for level in LEVELS:
        for mode in mr.MASK_MODES:
            c = mr.make_case(shape, level, mode)
            m = mr.Matcher(c.logs)
            for K in (1, 2, 3):
                for dust, thr in ((1, 0.0), (0, c.positive_threshold)):
                    yield c, m, K, dust, thr


@pytest.mark.parametrize("shape", [s for s in mr.SHAPES if min(s[1:]) >= 63], ids=mr.shape_id)
def test_both_sides_and_their_overlap_are_present(shape):
    for c, m, K, dust, thr in _kinds_cases(shape):
        r, s, both = mr.side_kinds(m, c, K, dust, thr)
        tag = (c.level, c.mask_mode, K, dust)
        assert r > 0 and s > 0 and both > 0, tag
        n_or = len(m.match(c.row_mask, c.col_mask, K, 0, dust, thr, None)[0])
        n_and = len(m.match(c.row_mask, c.col_mask, K, 1, dust, thr, None)[0])
        assert n_or == r + s + both and n_and == both and n_and < n_or, tag


def test_small_shapes_cover_the_three_kinds_between_them():
    tot = np.zeros(3, np.int64)
    for shape in [s for s in mr.SHAPES if min(s[1:]) < 63]:
        per = np.zeros(3, np.int64)
        for c, m, K, dust, thr in _kinds_cases(shape):
            per += mr.side_kinds(m, c, K, dust, thr)
        assert per.sum() > 0, shape
        tot += per
    assert (tot > 0).all(), tot


@pytest.mark.parametrize("shape", [s for s in mr.SHAPES if min(s[1:]) >= 40], ids=mr.shape_id)
def test_kth_element_falls_inside_a_run_of_equal_values(shape):
    """What makes "value descending, index ascending" observable at K > 1: in the coarse cases the K-th and the (K + 1)-th value of a line are
    equal in some line for every K of 1, 2, 3, 5, along rows and down columns, and the planted runs are cut where make_case says: the first K
    members in index order."""
    c = mr.make_case(shape, "coarse", "gate")
    B, M, N = shape
    P = np.exp(c.logs.astype(np.float64)).astype(np.float32)
    for axis in (2, 1):
        srt = -np.sort(-P, axis=axis)
        for K in (1, 2, 3, 5):
            a, b = np.take(srt, K - 1, axis=axis), np.take(srt, K, axis=axis)
            assert (a == b).any(), (axis, K)
    i, cols = c.planted["row_run"]
    j, rows = c.planted["col_run"]
    for K in (1, 2):
        ref, src = mr.Matcher(c.logs).sides(K, 1, 0.0)
        assert ref[0, i].nonzero()[0].tolist() == list(cols[:K]) and src[0, :, j].nonzero()[0].tolist() == list(rows[:K])
