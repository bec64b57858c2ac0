"""GPU: the dustbin top-1 / top-K matching kernels (csrc/matching.hip: k_top1_stats, k_top1_stats_small, k_top1_emit, k_topk_stats,
k_topk_emit) against the exact restatement of tests/matching_restatement.py, through the C ABI with buffers of the test's own.

Cases (matching_restatement.SHAPES x {coarse, fine} x mask modes {none, inf, gate}) reach: M != N, single lines, lines shorter than K (the
`exhausted` branch), the small top-1 kernel at 64 / 65 / 128 / 129 / 192-wide lines and at its 192-line limit, the generic kernel with 1, 4, 13,
22 and the capped 32 slices, B >= 64, and the planted ties of make_case (a row maximum repeated in one lane's three columns, a column maximum
repeated in the next row and four rows on, runs of equal values at the K-th element along rows and down columns, maxima equal to their
dustbin, an all-masked problem and one that loses to its dustbins everywhere).  logs are multiples of 1/64, so no decision can hang on
the last ulp of expf and the comparison is EXACT: the count after phase 1, out_bij in order and content; scores within 1e-6 max(1, global_scores[b]).

Every call: the workspace is filled with 0xff bytes before phase 1 (phase 2 may only read what phase 1 wrote), guard bands round ws, out_bij and
out_score must be intact after phase 2, and a second phase 1 + phase 2 on the workspace as the first left it must give the same bytes.

Measured (MI355X): 222 tests in 50 s, the slowest 3.5 s (351 x 332: 126 two-phase calls run twice, up to 5.5 M pairs compared), the next 0.7 s;
worst score error 0.074 of the bound.  No difference from the restatement in any case: the kernels are unchanged.  Scratch builds with one
comparison changed (`j <= rj` or `i <= coli[..]` to `<` in k_topk_emit, the index tie-break dropped from any of the three butterflies,
`p > rdust` to `>=`, `pv > cb[c]` to `>=`) fail 33 to 119 of the 119 tests that run the changed kernel; `Mr` -> `M` in the column loop of
k_topk_stats passes, and cannot fail: tests/test_matching_cpu.py::test_dustbin_entry_of_a_line_cannot_change_what_the_line_keeps."""
import ctypes

import numpy as np
import pytest
import torch

import matching_restatement as mr

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 256, 0xA5
LEVELS = tuple(mr.LEVELS)


def L():
    from lcrnet_amd import _lib
    return _lib


class Guarded:
    """`nbytes` device bytes filled with `fill` between two guard bands; the band after starts at the first byte past the buffer."""

    def __init__(self, nbytes, fill):
        self.n = int(nbytes)
        self.whole = torch.full((GUARD + self.n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.whole[GUARD:GUARD + self.n] = fill
        assert self.whole.data_ptr() % 256 == 0
        self.ptr = ctypes.c_void_p(self.whole.data_ptr() + GUARD)

    def host(self):
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == GUARD_BYTE).all() and (w[GUARD + self.n:] == GUARD_BYTE).all(), "a guard band was written"
        return w[GUARD:GUARD + self.n]


class Device:
    """One case on the device."""

    def __init__(self, case):
        self.case = case
        self.B, self.M, self.N = case.shape
        self.logs = torch.from_numpy(case.logs).cuda().contiguous()
        self.rm = None if case.row_mask is None else torch.from_numpy(case.row_mask.astype(np.uint8)).cuda().contiguous()
        self.cm = None if case.col_mask is None else torch.from_numpy(case.col_mask.astype(np.uint8)).cuda().contiguous()
        self.gs = torch.from_numpy(case.global_scores).cuda().contiguous()
        self.head = (L().ptr(self.logs), self.B, self.M, self.N, L().ptr(self.rm), L().ptr(self.cm))
        self.ws_bytes = {}

    def ws_size(self, kind):
        if kind not in self.ws_bytes:
            n = ctypes.c_size_t(0)
            L().check(getattr(L().lib(), "lcr_%s_matching_ws_bytes" % kind)(self.B, self.M, self.N, ctypes.byref(n)), "ws_bytes")
            self.ws_bytes[kind] = n.value
        return self.ws_bytes[kind]

    def call(self, entry, *mid):
        """Phase 1 + phase 2 of `entry` twice over one workspace -> (total, out_bij int32 [total, 3], out_score f32 [total])."""
        lib, fn = L(), getattr(L().lib(), entry)
        nws = self.ws_size("top1" if "top1" in entry else "topk")
        ws = Guarded(nws, 0xFF)
        sp = lib.stream_ptr(self.logs.device)
        runs = []
        for _ in range(2):
            total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            lib.check(fn(*self.head, *mid, lib.ptr(total), None, None, ws.ptr, nws, sp), entry + " phase 1")
            n = int(total.item())
            assert 0 <= n <= self.B * self.M * self.N, n
            bij, sc = Guarded(12 * n, 0xEE), Guarded(4 * n, 0xEE)
            lib.check(fn(*self.head, *mid, lib.ptr(total), bij.ptr, sc.ptr, ws.ptr, nws, sp), entry + " phase 2")
            assert int(total.item()) == n, "phase 2 leaves *total alone"
            runs.append((n, bij.host().copy(), sc.host().copy()))
            ws.host()
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2]), \
            entry + ": the second run differs from the first"
        n, bij, sc = runs[0]
        return n, bij.view(np.int32).reshape(n, 3), sc.view(np.float32)


def compare(tag, got, want, gs):
    """Count, rows (order and content) exact; scores within SCORE_TOL max(1, global_scores[b]).  Returns the worst score error / bound."""
    (n, bij, sc), (wb, ws) = got, want
    assert n == len(wb), (tag, "count", n, len(wb))
    assert np.array_equal(bij, wb), (tag, "rows", bij[(bij != wb).any(1)][:5], wb[(bij != wb).any(1)][:5])
    if n == 0:
        return 0.0
    bound = mr.SCORE_TOL * (np.maximum(1.0, gs.astype(np.float64)[wb[:, 0]]) if gs is not None else np.ones(n))
    assert np.isfinite(sc).all(), tag
    err = np.abs(sc.astype(np.float64) - ws) / bound
    assert err.max() <= 1.0, (tag, "score", float(err.max()))
    return float(err.max())


CASES = [pytest.param(s, lv, md, id="%s-%s-%s" % (mr.shape_id(s), lv, md)) for s in mr.SHAPES for lv in LEVELS for md in mr.MASK_MODES]


@pytest.mark.parametrize("shape,level,mode", CASES)
def test_top1_against_the_restatement(shape, level, mode):
    c = mr.make_case(shape, level, mode)
    d, m = Device(c), mr.Matcher(c.logs)
    worst = pairs = 0
    for mutual in (0, 1):
        got = d.call("lcr_top1_matching_ex", mutual)
        worst = max(worst, compare(("top1_ex", mutual), got, m.match(c.row_mask, c.col_mask, 1, mutual, 1, 0.0, None), None))
        pairs += got[0]
        if not mutual:
            plain = d.call("lcr_top1_matching")
            assert plain[0] == got[0] and plain[1].tobytes() == got[1].tobytes() and plain[2].tobytes() == got[2].tobytes()
    assert pairs > 0 or shape[1] * shape[2] == 1
    print("top1 %s %s %s: %d pairs, worst score error %.3f of the bound" % (mr.shape_id(shape), level, mode, pairs, worst))


@pytest.mark.parametrize("shape,level,mode", CASES)
def test_topk_against_the_restatement(shape, level, mode):
    """lcr_topk_matching_ex over K x mutual x (dustbin | three thresholds) x global scores, and lcr_topk_matching wherever it applies: against
    the restatement and byte for byte equal to the _ex form with use_dustbin = 1 and no global scores."""
    c = mr.make_case(shape, level, mode)
    d, m = Device(c), mr.Matcher(c.logs)
    gs_none = ctypes.c_void_p(0)
    worst, pairs, calls = 0.0, 0, 0
    for K in mr.ks_for(shape[2]):
        for mutual in (0, 1):
            for dust, thr in mr.switches(level):
                for gs in (None, c.global_scores):
                    tag = (K, mutual, dust, thr, gs is not None)
                    got = d.call("lcr_topk_matching_ex", K, mutual, dust, thr, gs_none if gs is None else L().ptr(d.gs))
                    worst = max(worst, compare(tag, got, m.match(c.row_mask, c.col_mask, K, mutual, dust, thr, gs), gs))
                    pairs += got[0]
                    calls += 1
                    if dust and gs is None:
                        plain = d.call("lcr_topk_matching", K, mutual)
                        assert plain[0] == got[0] and plain[1].tobytes() == got[1].tobytes() and plain[2].tobytes() == got[2].tobytes(), tag
                        calls += 1
    assert pairs > 0
    print("topk %s %s %s: %d calls, %d pairs, worst score error %.3f of the bound" % (mr.shape_id(shape), level, mode, calls, pairs, worst))


@pytest.mark.parametrize("shape", mr.SHAPES, ids=mr.shape_id)
def test_topk_at_k1_equals_top1_ex(shape):
    """The two kernel families agree where they overlap, on every shape (test_pose_chain_gpu.py has the square ones on near-ulp inputs)."""
    pairs = 0
    for level in LEVELS:
        for mode in mr.MASK_MODES:
            d = Device(mr.make_case(shape, level, mode))
            for mutual in (0, 1):
                a, b = d.call("lcr_top1_matching_ex", mutual), d.call("lcr_topk_matching", 1, mutual)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]), (level, mode, mutual)
                assert a[0] == 0 or np.abs(a[2].astype(np.float64) - b[2]).max() <= mr.SCORE_TOL
                pairs += a[0]
    assert pairs > 0


def test_functional_top1_matching_every_dispatch_branch():
    """F.top1_matching chooses among lcr_top1_matching_ex, lcr_topk_matching and lcr_topk_matching_ex: each branch once against the restatement,
    and on the zero-pair problems alone, where it must return empty tensors."""
    from lcrnet_amd import functional as F
    c = mr.make_case((3, 63, 64), "coarse", "inf")
    m, z = mr.Matcher(c.logs), mr.Matcher(c.logs[1:])
    logs, rm, cm, gs = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c.logs, c.row_mask, c.col_mask, c.global_scores))
    thr = c.positive_threshold
    branches = {"top1": dict(topk=1), "top1 mutual": dict(topk=1, mutual=True), "topk": dict(topk=3), "topk mutual": dict(topk=3, mutual=True),
                "ex threshold": dict(topk=2, use_dustbin=False, confidence_threshold=thr),
                "ex global scores": dict(topk=1, global_scores=gs), "ex both": dict(topk=5, mutual=True, use_dustbin=False, confidence_threshold=0.0,
                                                                                   global_scores=gs)}
    for name, kw in branches.items():
        want = dict(K=kw.get("topk", 1), mutual=int(kw.get("mutual", False)), use_dustbin=int(kw.get("use_dustbin", True)),
                    threshold=kw.get("confidence_threshold", 0.0))
        g = c.global_scores if "global_scores" in kw else None
        bij, sc = F.top1_matching(logs, rm, cm, **kw)
        assert bij.dtype == torch.int32 and sc.dtype == torch.float32 and bij.shape == (sc.shape[0], 3)
        wb, ws = m.match(c.row_mask, c.col_mask, global_scores=g, **want)
        assert len(wb) > 0
        compare(name, (bij.shape[0], bij.cpu().numpy(), sc.cpu().numpy()), (wb, ws), g)
        if want["use_dustbin"]:
            kz = dict(kw, global_scores=gs[1:]) if "global_scores" in kw else kw
            bij, sc = F.top1_matching(logs[1:], rm[1:], cm[1:], **kz)
            assert len(z.match(c.row_mask[1:], c.col_mask[1:], global_scores=None, **want)[0]) == 0
            assert tuple(bij.shape) == (0, 3) and tuple(sc.shape) == (0,), name
