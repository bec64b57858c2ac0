"""GPU: feature-matching RANSAC (csrc/feature_nn.hip, lcr_ransac_correspondences_ex in csrc/ransac.hip, registration.ransac_from_feats_batched)
against the NumPy restatement of tests/feature_ransac_restatement.py: the nearest neighbour bit for bit on every row, batch against
single calls, the checked RANSAC per hypothesis, checks off against the old entry, the index form against the gathered one, the
correspondence list, planted pairs end to end, the pair model's own features, and tools/registration_eval.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_ransac_restatement as fr
import ransac_restatement as rr
from conftest import LIMITS, NUM_STAGES, RADIUS, ROOT, VOXEL, load_scan

pytestmark = pytest.mark.gpu

BORDER = 1e-5        # m, as tests/test_ransac_gpu.py


def starts(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()


def cat(xs, width):
    return torch.from_numpy(np.concatenate([np.asarray(x, np.float32).reshape(-1, width) for x in xs])).cuda()


def run_nn(pairs):
    """[(q [nq,C], d [nd,C])] -> [(nn, d2)] per pair, one native call"""
    from lcrnet_amd import functional as F
    C = pairs[0][0].shape[1]
    ql, dl = [len(q) for q, _ in pairs], [len(d) for _, d in pairs]
    nn, d2 = F.feature_nn(cat([q for q, _ in pairs], C), cat([d for _, d in pairs], C), starts(ql), starts(dl))
    torch.cuda.synchronize()
    nn, d2 = nn.cpu().numpy(), d2.cpu().numpy()
    o = np.concatenate([[0], np.cumsum(ql)])
    return [(nn[o[i]:o[i + 1]], d2[o[i]:o[i + 1]]) for i in range(len(pairs))]


def same_nn(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, int((got[1].view(np.uint32) != want[1].view(np.uint32)).sum()))


def unit_rows(rng, n, C):
    x = rng.normal(size=(n, C))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def planted_database(rng, nq, nd, C):
    """unit-norm rows with exact duplicates (tie -> smaller row), near-duplicates one ulp apart in one channel, and queries on top of them"""
    d = unit_rows(rng, nd, C)
    d[nd - 3] = d[5]
    d[nd - 7] = d[11]
    d[nd - 9] = d[20]
    d[nd - 9, C // 2] = np.nextafter(d[20, C // 2], np.float32(2))
    d[40] = d[nd - 12]
    d[40, 0] = np.nextafter(d[40, 0], np.float32(-2))
    q = unit_rows(rng, nq, C)
    q[:4] = d[[5, 11, 20, nd - 12]]
    q[4:8] = d[[5, 11, 20, nd - 12]] + np.float32(1e-3) * unit_rows(rng, 4, C)
    return q, d


@pytest.mark.parametrize("C", [1, 3, 32, 33, 256, 1024])
def test_feature_nn_equals_the_restatement_on_every_row(C):
    rng = np.random.default_rng(1000 + C)
    pairs = [planted_database(rng, 300, 257, C), (unit_rows(rng, 70, C), unit_rows(rng, 1, C)),         # a database of one row
             (np.zeros((0, C), np.float32), unit_rows(rng, 9, C)),                                      # an empty-query pair
             (unit_rows(rng, 33, C), np.zeros((0, C), np.float32)),                                     # an empty-database pair
             planted_database(rng, 129, 64, C), (unit_rows(rng, 128, C), unit_rows(rng, 1100, C))]
    got = run_nn(pairs)
    for i, (q, d) in enumerate(pairs):
        same_nn(got[i], fr.feature_nn(q, d), (C, i))
    assert (got[3][0] == -1).all() and np.isnan(got[3][1]).all() and got[2][0].shape == (0,)
    if C > 1:
        assert got[0][0][0] == 5 and got[0][0][1] == 11 and got[0][1][0] == 0            # the duplicates' tie went to the smaller row


def test_feature_nn_with_a_common_offset_and_non_finite_rows():
    """A common offset of 100 on every channel (what costs an |q|^2 + |d|^2 - 2 q.d form about 14 bits) changes nothing for the plain
    chain, which every (i, j) goes through: there is no screening pass and hence no fall-back to count.  NaN distances never win; a row
    whose every distance is NaN gets -1; +inf is an ordinary value."""
    rng = np.random.default_rng(7)
    q, d = planted_database(rng, 300, 400, 256)
    q, d = q + np.float32(100), d + np.float32(100)
    dn = d.copy()
    dn[3, 17] = np.nan
    dn[5, 0] = np.inf
    qn = q.copy()
    qn[10, 200] = np.nan
    qn[0] = dn[3]                                                   # would be at distance 0 of the NaN row
    big = np.full((4, 256), np.float32(3e38))
    pairs = [(q, d), (qn, dn), (q[:5], np.full((3, 256), np.nan, np.float32)), (big, -big)]
    got = run_nn(pairs)
    for i, (a, b) in enumerate(pairs):
        same_nn(got[i], fr.feature_nn(a, b), i)
    assert got[1][0][10] == -1 and (got[2][0] == -1).all() and got[1][0][0] != 3
    assert (got[3][0] == 0).all() and np.isinf(got[3][1]).all()


def test_feature_nn_full_size_pair():
    """12 000 x 12 000 x 256 (about a level-0 KITTI cloud at 0.3 m): 1 024 seeded query rows against the whole database."""
    rng = np.random.default_rng(3)
    q, d = unit_rows(rng, 12000, 256), unit_rows(rng, 12000, 256)
    d[11000] = d[77]
    q[123] = d[77]
    got = run_nn([(q, d)])[0]
    rows = np.sort(np.concatenate([[123], rng.choice(12000, 1023, replace=False)]))
    want = fr.feature_nn(q[rows], d)
    same_nn((got[0][rows], got[1][rows]), want, "full")
    assert got[0][123] == 77 and (got[0] >= 0).all() and (got[0] < 12000).all()


def test_feature_nn_batch_equals_single_calls_bitwise():
    rng = np.random.default_rng(5)
    pairs = []
    for i in range(16):
        nq, nd = [700, 129, 0, 64, 2500][i % 5] + i, [900, 1, 300, 0, 1700][(i + i // 5) % 5] + 2 * i
        pairs.append((unit_rows(rng, nq, 32), unit_rows(rng, nd, 32)))
    a, b = run_nn(pairs), run_nn(pairs)
    for i, p in enumerate(pairs):
        one = run_nn([p])[0]
        for x, y, z in zip(a[i], b[i], one):
            assert x.tobytes() == y.tobytes() == z.tobytes(), i


def run_ex(pairs, thr, k, iters, seed, edge, dist, details=True):
    from lcrnet_amd import functional as F
    out = F.ransac_correspondences_ex(cat([p[0] for p in pairs], 3), cat([p[1] for p in pairs], 3), starts([len(p[0]) for p in pairs]), thr, k, iters,
                                      seed, edge_similarity=edge, checker_distance=dist, want_details=details, want_reject=True)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def borderline(src, ref, R, t, thr):
    src, ref = src.astype(np.float64), ref.astype(np.float64)
    out = np.zeros(len(R), np.int64)
    for a in range(0, len(R), 256):
        d = np.linalg.norm(np.matmul(src[None], np.transpose(R[a:a + 256], (0, 2, 1))) + t[a:a + 256, None] - ref[None], axis=2)
        out[a:a + 256] = (np.abs(d - thr) < BORDER).sum(axis=1)
    return out


def planted(k):
    cfg = dict(fr.PLANTED[k])
    rn = cfg.pop("ransac_n")
    return fr.planted_feature_pair(**cfg), rn


@pytest.mark.parametrize("which", [0, 1])
def test_checked_ransac_per_hypothesis_parity_with_the_restatement(which):
    (sp, rp, sf, rf, Tp, _), k = planted(which)
    nn, _ = fr.feature_nn(sf, rf)
    corr, _ = fr.correspondences(nn, None, n_ref=len(rp), min_rows=k)
    p5 = rr.planted_pair(5, 0.0, 0.01, seed=4)[:2]
    pairs = [p5, (sp[corr[:, 0]], rp[corr[:, 1]]), (sp[:2], rp[:2])]
    thr, iters, seed = fr.PLANTED_THR, fr.PLANTED_ITERS, fr.PLANTED_SEED
    T, inl, rmse, best, T_all, counts, sse, reject = run_ex(pairs, thr, k, iters, seed, 0.9, thr)
    for s, (src, ref) in enumerate(pairs):
        want = fr.ransac_checked(src, ref, thr, k, iters, seed, 0.9, thr)
        sl = slice(s * iters, (s + 1) * iters)
        c, e, Ta, rj = counts[sl], sse[sl], T_all[sl], reject[sl].astype(np.int64)
        exempt = (np.abs(want["sample_dist"] - thr) < BORDER).any(axis=1)
        assert exempt.sum() <= 0.01 * iters
        assert np.array_equal(rj == fr.REJECT_EDGE, want["reject"] == fr.REJECT_EDGE), s       # exact fp32 arithmetic: no exemption
        assert np.array_equal(rj[~exempt], want["reject"][~exempt]), (s, np.bincount(rj, minlength=4), np.bincount(want["reject"], minlength=4))
        valid = c >= 0
        assert np.array_equal(valid, rj == 0)
        both = valid & want["valid"]
        print("pair %d: reject shares device %s restatement %s, %d exempt" % (
            s, (np.bincount(rj, minlength=4) / iters).round(4).tolist(), (np.bincount(want["reject"], minlength=4) / iters).round(4).tolist(),
            int(exempt.sum())))
        if s == 1:
            assert 0 < valid.sum() < iters and (rj == 2).any() and (rj == 3).any()
        if s == 2:
            assert (rj == 1).all() and inl[s] == 0 and best[s] == -1            # fewer rows than ransac_n
        assert np.array_equal(Ta[~valid], np.broadcast_to(np.eye(4, dtype=np.float32), Ta[~valid].shape))
        assert (e[~valid] == 0).all()
        if both.any():
            assert np.abs(Ta[both, :3, :3] - want["R"][both]).max() < 1e-5
            assert np.abs(Ta[both, :3, 3] - want["t"][both]).max() < 1e-5 * max(1.0, np.abs(want["t"]).max())
            bl = borderline(src, ref, want["R"], want["t"], thr)
            dc = np.abs(c - want["counts"])
            assert (dc[both] <= bl[both]).all(), (s, int(dc[both].max()))
            assert np.allclose(e[both], want["sse"][both], rtol=1e-3, atol=thr * thr * bl[both] + 1e-4)
        if s < 2:
            b, wb = int(best[s]), want["best_h"]
            if not exempt[b] and not exempt[wb]:
                assert b == wb or abs(int(want["counts"][b]) - int(want["counts"][wb])) <= bl[b] + bl[wb], (s, b, wb)
            assert int(inl[s]) == int(c[b]) and np.array_equal(T[s], Ta[b])
            assert rmse[s] == pytest.approx(np.sqrt(np.float64(e[b]) / c[b]), rel=1e-6)
            order = np.lexsort((np.arange(iters), e, -c))                       # the winner is the best of the device's own scores
            assert order[0] == b


def test_checks_off_equals_the_old_entry_bitwise():
    from lcrnet_amd import functional as F
    pairs = []
    for i in range(16):
        n = [4096, 1000, 7, 333, 2048][i % 5] + i
        src, ref, _, _ = rr.planted_pair(n, 0.3 + 0.04 * i, 0.03, seed=100 + i)
        pairs.append((src, ref))
    src, ref, st = cat([p[0] for p in pairs], 3), cat([p[1] for p in pairs], 3), starts([len(p[0]) for p in pairs])
    old = F.ransac_correspondences(src, ref, st, 0.3, 4, 3000, 5, want_details=True)
    new = F.ransac_correspondences_ex(src, ref, st, 0.3, 4, 3000, 5, edge_similarity=0.0, checker_distance=-1.0, want_details=True, want_reject=True)
    torch.cuda.synchronize()
    for x, y in zip(old, new[:7]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    rj = new[7].cpu().numpy()
    assert np.array_equal(rj == 0, new[5].cpu().numpy() >= 0) and set(np.unique(rj)) <= {0, 1}


def test_index_form_equals_the_gathered_form_bitwise():
    from lcrnet_amd import functional as F
    clouds, rows = [], []
    for which in (0, 1):
        (sp, rp, sf, rf, _, _), _ = planted(which)
        nn, _ = fr.feature_nn(sf, rf)
        corr, _ = fr.correspondences(nn, fr.feature_nn(rf, sf)[0] if which else None, n_ref=len(rp), min_rows=3)
        clouds.append((sp, rp))
        rows.append(corr)
    clouds.insert(1, (clouds[0][0][:10], clouds[0][1][:0]))                     # a pair without correspondences in the middle
    rows.insert(1, np.zeros((0, 2), np.int32))
    corr = torch.from_numpy(np.concatenate(rows + [np.full((37, 2), 123456, np.int32)])).cuda()       # capacity beyond start[S]: never read
    st = starts([len(r) for r in rows])
    sc, rc = cat([c[0] for c in clouds], 3), cat([c[1] for c in clouds], 3)
    ss, rs = starts([len(c[0]) for c in clouds]), starts([len(c[1]) for c in clouds])
    a = F.ransac_correspondences_ex(sc, rc, st, 0.3, 3, 3000, 9, edge_similarity=0.9, checker_distance=0.3, corr=corr, src_start=ss, ref_start=rs,
                                    want_details=True, want_reject=True)
    gs = cat([c[0][r[:, 0]] for c, r in zip(clouds, rows)], 3)
    gr = cat([c[1][r[:, 1]] for c, r in zip(clouds, rows)], 3)
    b = F.ransac_correspondences_ex(gs, gr, st, 0.3, 3, 3000, 9, edge_similarity=0.9, checker_distance=0.3, want_details=True, want_reject=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert (a[1].cpu().numpy()[[0, 2]] > 100).all() and a[1].cpu().numpy()[1] == 0


def test_feature_correspondences_equal_the_restatement():
    from lcrnet_amd import functional as F
    rng = np.random.default_rng(2)
    (sp, rp, sf, rf, _, _), _ = planted(0)
    nn0, nr0 = fr.feature_nn(sf, rf)[0], fr.feature_nn(rf, sf)[0]
    # a pair whose mutual set has 2 rows (< 3): falls back; a pair with unmatched (-1) rows; an empty pair; a pair with an empty reference
    nn1, nr1 = np.array([1, 0, 1, 0, 1, 1], np.int32), np.array([1, 0], np.int32)
    nn2 = rng.integers(-1, 300, size=700).astype(np.int32)
    nr2 = rng.integers(0, 700, size=300).astype(np.int32)
    nr2[nn2[nn2 >= 0][:200]] = np.nonzero(nn2 >= 0)[0][:200]
    items = [(nn0, nr0), (nn1, nr1), (nn2, nr2), (np.zeros(0, np.int32), np.zeros(5, np.int32)), (np.full(4, -1, np.int32), np.zeros(0, np.int32))]
    ss, rs = starts([len(a) for a, _ in items]), starts([len(b) for _, b in items])
    nn_sr = torch.from_numpy(np.concatenate([a for a, _ in items])).cuda()
    nn_rs = torch.from_numpy(np.concatenate([b for _, b in items])).cuda()
    for mutual in (False, True):
        corr, st, used = F.feature_correspondences(nn_sr, ss, rs, nn_rs if mutual else None, min_rows=3)
        torch.cuda.synchronize()
        corr, st, used = corr.cpu().numpy(), st.cpu().numpy(), used.cpu().numpy()
        want = [fr.correspondences(a, b if mutual else None, n_ref=len(b), min_rows=3) for a, b in items]
        assert np.array_equal(st, np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]))
        for i, (w, u) in enumerate(want):
            assert np.array_equal(corr[st[i]:st[i + 1]], w), (mutual, i)
            assert bool(used[i]) == u, (mutual, i)
        if mutual:
            assert used.tolist() == [1, 0, 1, 0, 0] and st[2] - st[1] == 6


def feats_batched(items, k, iters, seed, mutual, edge=0.9):
    from lcrnet_amd.registration import ransac_from_feats_batched
    r = ransac_from_feats_batched(cat([i[0] for i in items], 3), cat([i[1] for i in items], 3), cat([i[2] for i in items], items[0][2].shape[1]),
                                  cat([i[3] for i in items], items[0][2].shape[1]), [len(i[0]) for i in items], [len(i[1]) for i in items],
                                  fr.PLANTED_THR, k, iters, seed, mutual_filter=mutual, edge_similarity=edge, want_corr=True, want_reject=True)
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in r.items()}


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("mutual", [False, True])
def test_planted_pairs_end_to_end(which, mutual):
    from lcrnet_amd import evaluation as ev
    item, k = planted(which)
    sp, rp, sf, rf, Tp, _ = item
    thr, iters, seed = fr.PLANTED_THR, fr.PLANTED_ITERS, fr.PLANTED_SEED
    got = feats_batched([item], k, iters, seed, mutual)
    want = fr.feature_ransac(sp, rp, sf, rf, thr, k, iters, seed, mutual_filter=mutual)
    n = int(got["num_corr"][0])
    assert n == len(want["corr"]) and np.array_equal(got["corr"][:n], want["corr"]) and got["start"].tolist() == [0, n]
    rre, rte = ev.compute_registration_error(Tp, got["T"][0].astype(np.float64))[:2]
    assert rre < 0.5 and rte < 0.1
    src, ref = sp[want["corr"][:, 0]], rp[want["corr"][:, 1]]
    bl = borderline(src, ref, want["R"], want["t"], thr)
    b, wb = int(got["best_h"][0]), want["best_h"]
    assert b == wb or abs(int(want["counts"][b]) - int(want["counts"][wb])) <= bl[b] + bl[wb], (b, wb)
    exempt = int((np.abs(want["sample_dist"] - thr) < BORDER).any(axis=1).sum())
    scored, wscored = float((got["reject_all"] == 0).mean()), float((want["reject"] == 0).mean())
    print("planted %d mutual %d: %d corr, RRE %.4f deg RTE %.4f m, %d inliers (h %d); %.2f %% of the hypotheses reach scoring (restatement "
          "%.2f %%, %d exempt)" % (which, mutual, n, rre, rte, got["inliers"][0], b, 100 * scored, 100 * wscored, exempt))
    assert abs(scored - wscored) * iters <= exempt
    if not mutual:                                              # the same pair inside a batch: the same bytes
        other, _ = planted(1 - which)
        many = feats_batched([other, item], k, iters, seed, mutual)
        for key in ("T", "inliers", "rmse", "best_h", "num_corr"):
            assert many[key][1:2].tobytes() == got[key].tobytes(), key


def pair_model_outputs(pairs, checkpoint=None):
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family import LCRNet
    from lcrnet_amd.pipeline import PairPipeline
    from lcrnet_amd.weights import load_snapshot, seeded_state_dict
    cfg = make_cfg()
    cfg["neighbor_limits"] = LIMITS
    m = LCRNet(cfg).eval()
    if checkpoint:
        missing, _ = load_snapshot(m, checkpoint, strict=False)
        assert not missing
    else:
        m.load_state_dict(seeded_state_dict(m.state_dict(), 7351), strict=True)
    m = m.cuda()
    work = []
    for a, b in pairs:
        pa, pb = torch.from_numpy(load_scan(a)).cuda(), torch.from_numpy(load_scan(b)).cuda()
        work.append((torch.cat([pa, pb]), torch.tensor([len(pa), len(pb)], dtype=torch.int64, device="cuda")))
    with PairPipeline(m, VOXEL, RADIUS, NUM_STAGES, LIMITS, workers=1, pairs_per_call=1) as pipe:
        return list(pipe.run(work))


def test_on_the_pair_models_own_features():
    """Seeded weights do not give descriptive features (tests/test_ransac_gpu.py, the note on the demo pair), so no pose is asserted: the
    path runs on anc -> pos with the model's dense features (cfg's fine width), is finite and repeatable, keeps one correspondence per source point, and its
    nearest neighbours are the restatement's (every row of the first pair, 1 024 seeded rows of the second)."""
    from lcrnet_amd import functional as F
    from lcrnet_amd.registration import ransac_from_feats_batched
    outs = pair_model_outputs([("003854", "000958"), ("000026", "000560")])
    g = lambda k: [o[k].float().contiguous() for o in outs]
    sp, rp, sf, rf = g("anc_points_f"), g("pos_points_f"), g("anc_feats_f"), g("pos_feats_f")
    sl, rl = [len(x) for x in sp], [len(x) for x in rp]
    assert sf[0].shape[1] == rf[0].shape[1] >= 128 and sf[0].shape[0] == sl[0] and rf[1].shape[0] == rl[1]
    args = (torch.cat(sp), torch.cat(rp), torch.cat(sf), torch.cat(rf), sl, rl, 0.3, 4, 2000, 1)
    a = ransac_from_feats_batched(*args, want_corr=True, want_reject=True)
    b = ransac_from_feats_batched(*args, want_corr=True, want_reject=True)
    torch.cuda.synchronize()
    for key in a:
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key
    assert torch.isfinite(a["T"]).all() and torch.isfinite(a["rmse"]).all()
    assert a["num_corr"].tolist() == sl
    nn, d2 = F.feature_nn(torch.cat(sf), torch.cat(rf), starts(sl), starts(rl))
    nn, d2 = nn.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(a["corr"].cpu().numpy()[:, 1], nn)
    rows1 = np.sort(np.random.default_rng(0).choice(sl[1], min(1024, sl[1]), replace=False))
    for i, rows in ((0, np.arange(sl[0])), (1, rows1)):
        o = sum(sl[:i])
        want = fr.feature_nn(sf[i].cpu().numpy()[rows], rf[i].cpu().numpy())
        same_nn((nn[o + rows], d2[o + rows]), want, i)
    print("model features: %s source points, %s inliers, %.1f %% of the hypotheses reach scoring" % (
        sl, a["inliers"].tolist(), 100 * float((a["reject_all"] == 0).float().mean())))


def _checkpoint():
    for p in (os.environ.get("LCR_WEIGHTS", ""), os.path.join(ROOT, "weights", "best-model-mixed.tar")):
        if p and os.path.isfile(p):
            return p
    return None


@pytest.mark.skipif(_checkpoint() is None, reason="best-model-mixed.tar not present (README.md:57-68: external download)")
def test_trained_features_register_the_demo_pair():
    """With the trained checkpoint (the skip rule of tests/test_real_weights_gpu.py): feature-matching RANSAC on the demo pair lands
    within eval.py's acceptance (RRE < 5 deg, RTE < 2 m) of the README's pose."""
    from lcrnet_amd import evaluation as ev
    from lcrnet_amd.registration import ransac_from_feats_batched
    from test_real_weights_gpu import README_T
    o = pair_model_outputs([("003854", "000958")], _checkpoint())[0]
    r = ransac_from_feats_batched(o["anc_points_f"].float(), o["pos_points_f"].float(), o["anc_feats_f"].float(), o["pos_feats_f"].float(),
                                  [len(o["anc_points_f"])], [len(o["pos_points_f"])], 0.3, 4, 50000)
    rre, rte = ev.compute_registration_error(README_T, r["T"][0].cpu().numpy().astype(np.float64))[:2]
    assert rre < 5 and rte < 2, (rre, rte)


def test_registration_eval_ransac_featurematch_end_to_end(tmp_path):
    from lcrnet_amd import io_formats as io
    (sp, rp, sf, rf, Tp, match), k = planted(0)
    hit = np.nonzero(match >= 0)[0]

    def out_dict():
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
        return dict(pos_points_f=t(rp), anc_points_f=t(sp), pos_points_c=t(rp[:50]), anc_points_c=t(sp[:50]), pos_feats_f=t(rf), anc_feats_f=t(sf),
                    pos_corr_points=t(rp[match[hit]]), anc_corr_points=t(sp[hit]), corr_scores=torch.ones(len(hit)),
                    pos_node_corr_indices=torch.zeros(0, dtype=torch.int64), anc_node_corr_indices=torch.zeros(0, dtype=torch.int64),
                    estimated_transform=t(Tp.astype(np.float32)), pos_feature_global=torch.zeros(1, 256), anc_feature_global=torch.zeros(1, 256))

    with_dir, without_dir = tmp_path / "with", tmp_path / "without"
    with_dir.mkdir()
    without_dir.mkdir()
    for i in range(3):
        p = io.save_registration(str(with_dir), 0, 100 + i, 200 + i, out_dict(), Tp, with_feats=True)
        assert {"pos_feats_f", "anc_feats_f"} <= set(np.load(p).files)
    p = io.save_registration(str(without_dir), 0, 100, 200, out_dict(), Tp)
    assert not {"pos_feats_f", "anc_feats_f"} & set(np.load(p).files)           # the default keeps the reference's key set

    def tool(folder, *extra):
        return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_eval.py"), str(folder), "--method", "ransac_featurematch",
                               "--ransac-n", str(k), "--num-iterations", str(fr.PLANTED_ITERS), "--seed", str(fr.PLANTED_SEED)] + list(extra),
                              capture_output=True, text=True, timeout=600)

    r = tool(with_dir, "--pairs-per-call", "2")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["pairs"] == 3 and got["registration"]["RR"] == 1.0 and got["registration"]["RRE"] < 0.5 and got["registration"]["RTE"] < 0.1
    fm = got["ransac_featurematch"]
    assert fm["num_corr"] == len(sp) and 0.9 < fm["rejected"]["edge_length"] < 1 and fm["rejected"]["distance"] > 0
    r = tool(with_dir, "--mutual-filter", "--refine", "icp")
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["registration"]["RR"] == 1.0 and got["ransac_featurematch"]["num_corr"] < len(sp) and got["refine"]["method"] == "icp"
    r = tool(without_dir)
    assert r.returncode != 0 and "with_feats=True" in r.stderr and "pos_feats_f" in r.stderr
