"""GPU: the pose fit of the registration tail (csrc/lgr.hip, csrc/rigid3.h) and the vote shift, greedy NMS and neighbour mean of
csrc/pose_tail.hip, each against the fp64 restatement of tests/pose_fit_restatement.py — an independent reference with known answers for the
branches the model-level tests never reach (ragged and empty chunks, zero weights, rank-deficient clouds, the degenerate LGR branch, an empty
inlier set, the rank carry of the verification set, the NMS overflow rescan, int32 neighbour indices).

Inputs, cases and tolerances come from pose_fit_restatement: TOL[op] = min(1e-4, 4 x the CPU fp32 floor) x max(1, |want|max), the rotation block
and the translation column of a Procrustes result each against its own |want|max.  Integer outputs (inlier counts, winners, NMS masks and
lengths, the verification set through the counts) must be EQUAL: tests/test_pose_fit_cpu.py shows without a GPU that no fp64 residual lies
within 1e-4 of the radius and no NMS distance within 1e-3 of it, and that every planted mutation moves the fp64 result by >= 20 TOL or
changes an integer on these cases.

Measured (MI355X; worst figure over every case of this file; errors absolute, next to the bound of the case they occurred in):

    operator / quantity                        | CPU fp32 floor | TOL     | worst GPU error (case)
    procrustes  rotation block                 | 2.5e-3 (*)     | 1e-4    | 3.0e-8 (mirrored, uniform), bound 1.0e-4
    procrustes  translation column             | 1.3e-3 (*)     | 1e-4    | 5.1e-7 (1000 m offset, random weights), bound 5.8e-3; 0.001 of the bound at worst
    procrustes  rank <= 1 chunks (147)         |                |         | |R^T R - I| <= 7.9e-8, det 1 +- 1e-7; residual at most 5.0e-5 above the restatement's
    lgr         hypotheses (chunks >= 3 rows)  | 9.4e-6         | 3.8e-5  | 3.2e-7 (branches), bound 3.2e-4
    lgr         T                              | 6.8e-7         | 2.7e-6  | 5.4e-8 (branches, 1 step), bound 5.4e-6 = 0.01 of it
    vote_shift  out                            | 3.1e-8         | 1.2e-7  | 2.0e-6 (N = 257), bound 7.9e-6 = 0.25 of it
    neighbor_mean out                          | 1.6e-7         | 6.4e-7  | 2.9e-6 (M = 257, H = 20), bound 1.2e-5 = 0.24 of it
    inlier counts / winners / weights, LGR counts and winners, NMS masks (6 073 decisions) and lengths, int32 vs int64 neighbour means: equal
    (*) the floor of the clouds 1000 m from the origin, where fp32 centring loses the +-1 m extent; the kernel centres in fp64.
83 cases in 3 s.

What these tests found, and what was changed for it (before -> after):
  * H == 0 (an empty chunk, or every weight zero): rotation_from_H (csrc/rigid3.h) left u0 = 0, completed u1 = e0 and took u2 = u0 x u1 = 0, so
    lcr_procrustes_batched returned the rank-1 "rotation"
        [[0 0 0 0] [1 0 0 0] [0 0 0 0] [0 0 0 1]]
    for the empty chunk of every one of the 48 Procrustes launches and for every all-zero-weight chunk, and lcr_local_global_registration
    returned it as the pose of pair (c), whose selected transform has no inlier within the radius (|T - I| = 1.0 against a bound of
    5.4e-6).  U now starts from the canonical basis when the largest singular value is zero: the identity, exactly, in all of them.  No other
    path of the header changed.
  * Zero rows through the wrappers: an empty tensor has a null data pointer, and lcr_vote_shift, lcr_neighbor_mean, lcr_inlier_weights and
    lcr_inlier_count refused it (LCR_EARG -> RuntimeError) before looking at the count.  With no row there is nothing to read: they now return
    LCR_OK untouched (lcr_inlier_count: zero counts), as lcr_gather_rows and lcr_upsample_concat already did.
  * Nothing else: the ragged and sub-wavefront chunks, negative and tiny weights, the reflection fix, the rank carry of the verification set
    across its 256-row passes, the degenerate LGR branch, the NMS overflow rescan (590 points of the 2500-point cloud have more than 24
    lower-index in-range neighbours) and its second and third strided trips, and the int32 neighbour mean all agree with the restatement.
"""
import numpy as np
import pytest
import torch

import pose_fit_restatement as pr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
ORTHO = 1e-6             # R is stored in fp32: each entry is off by <= 2^-24, so R^T R - I and det R - 1 by a few 1e-7 (9 entries x 2 x 6e-8)


def F():
    from lcrnet_amd import functional
    return functional


def L():
    from lcrnet_amd import _lib
    return _lib


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def report(op, case, what, err, bound):
    print(f"pose_fit {op} {case} {what}: err {err:.3e} bound {bound:.3e} ({err / bound:.3f} of it)")


def check_close(op, tol_key, case, what, got, want):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float32, (op, case, what, got.shape, want.shape)
    assert np.isfinite(got).all(), (op, case, what)
    err, bound = pr.shift_of(got, want), pr.bound_of(tol_key, want)
    report(op, case, what, err, bound)
    assert err <= bound, (op, case, what, err, bound)


def check_pose(op, case, got, want):
    """Transforms [..., 4, 4]: rotation block and translation column each under the Procrustes TOL; last row exact."""
    assert np.isfinite(got).all() and got.dtype == np.float32
    assert np.array_equal(got[..., 3, :], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), got[..., 3, :].shape)), (op, case)
    (eR, bR), (et, bt) = pr.pose_errors(got, want)
    report(op, case, "R", eR, bR)
    report(op, case, "t", et, bt)
    assert eR <= bR and et <= bt, (op, case, eR, bR, et, bt)


# ------------------------------------------------------------------------------------------------ weighted Procrustes: lcr_procrustes_batched
@pytest.mark.parametrize("geometry,weights", pr.procrustes_case_names())
def test_procrustes_against_fp64(geometry, weights):
    """One ragged launch (chunks of 0, 1, 2, 3, 63, 64, 65, 200 rows behind 5 rows that belong to no chunk).  Chunks with a unique answer are
    compared with the restatement; rank <= 1 ones must give a proper rotation that aligns no worse; H == 0 (no row, all weights zero) must give
    the identity."""
    c = pr.procrustes_case(geometry, weights)
    case = f"{geometry} {weights}"
    want = pr.procrustes_reference(geometry, weights)
    got = host(F().procrustes(dev(c["src"]), dev(c["ref"]), dev(c["w"]), dev(c["start"], torch.int32)))
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all(), case
    assert np.array_equal(got[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (len(got), 1))), case
    u = pr.unique_chunks(c)
    if u.any():
        check_pose("procrustes", case, got[u], want[u])
    for p, kind in enumerate(c["kind"]):
        a, b = c["start"][p], c["start"][p + 1]
        if kind == "zero":
            print(f"pose_fit procrustes {case} chunk of {b - a} rows, H == 0:\n{got[p]}")
            assert np.array_equal(got[p], np.eye(4, dtype=np.float32)), (case, p, got[p])
        elif kind == "deficient":
            R = got[p, :3, :3].astype(np.float64)
            ortho, det = np.abs(R.T @ R - np.eye(3)).max(), np.linalg.det(R)
            mine = pr.alignment_residual(got[p], c["src"][a:b], c["ref"][a:b], c["w"][a:b])
            theirs = pr.alignment_residual(want[p], c["src"][a:b], c["ref"][a:b], c["w"][a:b])
            bound = pr.bound_of("procrustes_t", np.concatenate([want[p, :3, 3], c["ref"][a:b].ravel()]))
            print(f"pose_fit procrustes {case} chunk of {b - a} rows, rank <= 1: |R^T R - I| {ortho:.2e} det {det:.7f} residual {mine:.3e} "
                  f"(restatement {theirs:.3e}, allowed excess {bound:.3e})")
            assert ortho <= ORTHO and abs(det - 1) <= ORTHO and mine <= theirs + bound, (case, p)


# ------------------------------------------------------------------------------------------------ lcr_inlier_count, lcr_inlier_weights
def _count(c, start=None, min_count=0):
    counts, best = F().inlier_count(dev(c["T"]), dev(c["src"]), dev(c["ref"]), c["radius"], None if start is None else dev(start, torch.int32), min_count)
    return host(counts), int(host(best)[0])


@pytest.mark.parametrize("P", pr.INLIER_PS)
@pytest.mark.parametrize("n", pr.INLIER_NS)
def test_inlier_count_and_weights_are_exact(n, P):
    c = pr.inlier_case(n, P)
    want_counts, want_best = pr.inlier_count(c["T"], c["src"], c["ref"], c["radius"])
    counts, best = _count(c)
    print(f"pose_fit inlier n={n} P={P}: counts {counts.tolist()} (want {want_counts.tolist()}) best {best} (want {want_best})")
    assert counts.dtype == np.int32 and np.array_equal(counts, want_counts) and best == want_best
    score = c["score"].astype(np.float32)
    for sel in (None, P - 2 if P > 1 else 0):
        w = host(F().inlier_weights(dev(c["T"]), None if sel is None else dev(np.array([sel]), torch.int32), dev(c["src"]), dev(c["ref"]),
                                    dev(c["score"]), c["radius"]))
        want = pr.inlier_weights(c["T"], sel, c["src"], c["ref"], c["score"], c["radius"]).astype(np.float32)
        assert w.dtype == np.float32 and np.array_equal(w.view(np.uint32), want.view(np.uint32)), (n, P, sel)     # score bit for bit, or +0.0
        assert np.array_equal(w != 0, (want != 0)) and np.array_equal(w[w != 0], score[w != 0])


def test_inlier_weights_of_no_rows_writes_nothing():
    lib, c = L(), pr.inlier_case(1, 1)
    out = torch.full((8,), SENTINEL, device="cuda")
    T, src, ref, sc = dev(c["T"]), dev(c["src"]), dev(c["ref"]), dev(c["score"])
    rc = lib.lib().lcr_inlier_weights(lib.ptr(T), lib.ptr(None), lib.ptr(src), lib.ptr(ref), lib.ptr(sc), 0, c["radius"], lib.ptr(out), lib.stream_ptr(out.device))
    assert rc == 0 and bool((host(out) == SENTINEL).all())


@pytest.mark.parametrize("name", tuple(pr.CHUNKED))
def test_inlier_count_with_chunks_and_min_count(name):
    c = pr.chunked_inlier_case(name)
    want_counts, want_best = pr.inlier_count(c["T"], c["src"], c["ref"], c["radius"], c["start"], c["min_count"])
    counts, best = _count(c, c["start"], c["min_count"])
    print(f"pose_fit inlier {name}: counts {counts.tolist()} (want {want_counts.tolist()}) best {best} (want {want_best})")
    assert np.array_equal(counts, want_counts) and best == want_best


def test_inlier_residual_equal_to_the_radius_is_no_inlier():
    c = pr.exact_inlier_case()
    counts, best = _count(c)
    w = host(F().inlier_weights(dev(c["T"]), None, dev(c["src"]), dev(c["ref"]), dev(c["score"]), c["radius"]))
    assert counts.tolist() == [30] and best == 0
    assert not w[::2].any() and np.array_equal(w[1::2], c["score"].astype(np.float32)[1::2])


# ------------------------------------------------------------------------------------------------ lcr_local_global_registration_ex
def _lgr(c, steps):
    T, hyp, counts, best = F().local_global_registration(dev(c["src"]), dev(c["ref"]), dev(c["score"]), dev(c["hyp_start"], torch.int32),
                                                         dev(c["seg_hyp_start"], torch.int32), c["radius"], c["min_count"], steps, want_details=True,
                                                         correspondence_limit=c["limit"] or None)
    return host(T), host(hyp), host(counts), host(best)


@pytest.mark.parametrize("steps", pr.LGR_STEPS)
@pytest.mark.parametrize("name", tuple(pr.LGR_STACKS))
def test_lgr_against_fp64(name, steps):
    """The S = 3 stack, then every pair of it alone (S = 1): integers equal to the restatement's, hypotheses (of the chunks that may win) and
    transforms within TOL, and a pair run alone gives the bytes it gives in the stack."""
    c = pr.lgr_case(name)
    case = f"{name} steps={steps}"
    wT, whyp, wcounts, wbest = pr.lgr_reference(name, steps)
    T, hyp, counts, best = _lgr(c, steps)
    print(f"pose_fit lgr {case}: counts {counts.tolist()} best {best.tolist()} (want {wbest.tolist()})")
    assert np.array_equal(counts, wcounts) and np.array_equal(best, wbest), case
    valid = wcounts >= 0
    assert np.isfinite(hyp).all() and np.isfinite(T).all()
    check_close("lgr", "lgr_hyp", case, "hyp", hyp[valid], whyp[valid].astype(np.float64))
    check_close("lgr", "lgr_T", case, "T", T, wT)
    assert np.array_equal(T[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (len(T), 1)))
    if name == "branches":
        print(f"pose_fit lgr {case} pair c (no inlier within the radius):\n{T[2]}")
        assert wbest[1] == -1 and np.array_equal(T[2], np.eye(4, dtype=np.float32)), T[2]
    ss, hs = c["seg_hyp_start"], c["hyp_start"]
    for s in range(len(ss) - 1):
        a = pr.lgr_pair_alone(c, s)
        aT, ahyp, acounts, abest = _lgr(a, steps)
        assert aT.tobytes() == T[s].tobytes() and ahyp.tobytes() == hyp[ss[s]:ss[s + 1]].tobytes(), (case, s)
        assert np.array_equal(acounts, counts[ss[s]:ss[s + 1]]) and abest[0] == (best[s] - ss[s] if best[s] >= 0 else -1), (case, s)


# ------------------------------------------------------------------------------------------------ lcr_vote_shift
@pytest.mark.parametrize("N", pr.VOTE_NS)
def test_vote_shift_against_fp64(N):
    c = pr.vote_case(N)
    got = host(F().vote_shift(dev(c["xyz"]), dev(c["off"]), c["max_range"]))
    want = pr.vote_shift(c["xyz"], c["off"], c["max_range"])
    check_close("vote_shift", "vote_shift", f"N={N}", "out", got, want)
    length = np.linalg.norm(c["off"], axis=1)
    at_or_below = length <= c["max_range"]           # not scaled: the sum of two floats, rounded once
    assert np.array_equal(got[at_or_below], (c["xyz"].astype(np.float32) + c["off"].astype(np.float32))[at_or_below])


# ------------------------------------------------------------------------------------------------ lcr_greedy_nms
@pytest.mark.parametrize("name", ("stack", "edge"))
def test_greedy_nms_is_the_sequential_rule(name):
    c = pr.nms_case(name)
    wkeep, wlen = pr.nms_reference(name)
    keep, out_len = F().greedy_nms(dev(c["pts"]), dev(c["lens"], torch.int64), c["radius"])
    keep, out_len = host(keep), host(out_len)
    wrong = int((keep.astype(bool) != wkeep).sum())
    print(f"pose_fit nms {name}: {wrong} of {len(wkeep)} decisions differ; kept {out_len.tolist()} (want {wlen.tolist()})")
    assert keep.dtype == np.uint8 and bool(((keep == 0) | (keep == 1)).all()) and out_len.dtype == np.int64
    assert wrong == 0 and np.array_equal(out_len, wlen)


# ------------------------------------------------------------------------------------------------ lcr_neighbor_mean
@pytest.mark.parametrize("H", pr.NM_HS)
@pytest.mark.parametrize("M", pr.NM_MS)
def test_neighbor_mean_against_fp64(M, H):
    lib, c = L(), pr.neighbor_case(M, H)
    want = pr.neighbor_mean(c["pts"], c["idx"], c["pad"])
    pts = dev(c["pts"])
    outs = []
    for dtype in (torch.int32, torch.int64):
        idx = dev(c["idx"], dtype)
        out = torch.full((max(M, 1) + 1, 3), SENTINEL, device="cuda")                 # one row more than M: it must stay untouched
        anchor = idx if M else torch.zeros(1, dtype=dtype, device="cuda")              # a valid pointer for M == 0 too
        rc = lib.lib().lcr_neighbor_mean(lib.ptr(pts), lib.ptr(anchor), int(dtype == torch.int64), M, H, c["pad"], lib.ptr(out), lib.stream_ptr(out.device))
        assert rc == 0
        out = host(out)
        assert bool((out[M:] == SENTINEL).all()), (M, H, dtype)
        outs.append(out[:M])
        if M:
            assert np.array_equal(host(F().neighbor_mean(pts, idx, c["pad"])).view(np.uint32), out[:M].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (M, H)      # int32 and int64 indices: the same bits
    none = np.isnan(want).all(1)
    assert np.array_equal(np.isnan(outs[0]), np.isnan(want)) and np.isnan(outs[0][none]).all()    # 0 / 0, not stale memory
    if M:
        check_close("neighbor_mean", "neighbor_mean", f"M={M} H={H}", "out", outs[0][~none], want[~none])


def test_empty_inputs_through_the_wrappers():
    """Zero rows reach the entry points as null pointers (an empty tensor has none): nothing to read, so nothing to refuse."""
    z3 = torch.zeros((0, 3), device="cuda")
    assert F().vote_shift(z3, z3, 5.0).shape == (0, 3)
    assert F().neighbor_mean(dev(pr.neighbor_case(1, 1)["pts"]), torch.zeros((0, 20), dtype=torch.int64, device="cuda"), pr.NM_PAD).shape == (0, 3)
    assert F().inlier_weights(dev(np.eye(4)[None]), None, z3, z3, torch.zeros((0,), device="cuda"), 0.45).shape == (0,)
