"""Exact NumPy restatement of the dustbin top-1 / top-K matching (csrc/matching.hip) as include/lcr_hip.h states it (lcr_top1_matching*,
lcr_topk_matching*) and as oracle/torch_ref.py:398-423 spells the reference (local_global_registration.py:48-93, :236-237); the shared
inputs and case tables of tests/test_matching_cpu.py and tests/test_matching_gpu.py.

    match(logs, row_mask, col_mask, K, mutual, use_dustbin, threshold, global_scores) -> (bij int32 [C, 3] row-major, scores float64 [C])

The selection runs on P = float32(exp(float64(logs))).  Every line of P (rows and columns; the dustbin column and row take part when
use_dustbin is set, only the M x N interior otherwise) is put into a STABLE descending order — equal values in index order — and its first K
entries are the line's selection; a line with fewer than K entries is selected whole.  Dustbin form: a selected entry counts if it is strictly
greater than its line's dustbin.  Without the dustbin the selected values are scattered into a zero matrix and an entry counts where that
matrix is strictly greater than the threshold, so an unselected entry counts as 0.  `mutual` takes the row side AND the column side, else OR.
The masks are applied last: a masked line that holds ordinary values still occupies slots of the lines that cross it.  Scores are
exp(logs) * global_scores[b] in fp64.  The kernel keeps the K-th (value, index) of each line and tests membership by comparison; nothing of that
is here: this file ranks.

Why the comparison with the device is EXACT (make_case): logs = -(q / 64) as float32 with integer q, so neighbouring exp values differ by
1.6 % and equal logs give equal exps on any exp; no decision can depend on the last ulp of the device's expf.  (Near-ulp and underflowing
logs stay with test_pose_chain_gpu.py::test_top1_candidate_rule_equals_exp_of_everything.)
"""
import numpy as np

MASKED = -1e12           # what the transport leaves in a masked line
LEVELS = {"coarse": 8, "fine": 1280}                                         # q uniform in [0, L): eight levels with ties everywhere / logs in (-20, 0]
POSITIVE_THRESHOLD = {"coarse": float(np.exp(-2.5 / 64)), "fine": float(np.exp(-100.5 / 64))}    # between two levels
MASK_MODES = ("none", "inf", "gate")
SCORE_TOL = 1e-6         # x max(1, global_scores[b]): the bound test_pose_chain_gpu.py holds these scores to; every exp value is <= 1

# (B, M, N): the smallest shapes that reach each path of the kernels
SHAPES = [
    (3, 1, 1), (2, 1, 7), (2, 7, 1),                     # single lines
    (2, 5, 70), (2, 70, 5),                              # lines shorter than K on one side, longer than a wavefront on the other
    (3, 63, 64), (3, 64, 65), (2, 127, 128), (2, 129, 130),      # line widths N + 1 = 65, 66, 129, 131 and M + 1 = 64, 65, 128, 130
    (2, 191, 100), (2, 100, 191),                        # the small top-1 kernel at its limit (192 lines), not square
    (2, 192, 50), (2, 50, 192),                          # the first shapes past it: the generic kernel with 13 and 4 slices
    (1, 351, 332),                                       # the node-level shape, 22 slices
    (1, 600, 40),                                        # the slice cap of 32
    (64, 9, 11), (64, 200, 10),                          # B >= 64: one slice; small and generic
]
SMALL_SHAPES = [s for s in SHAPES if s[0] * (s[1] + 1) * (s[2] + 1) <= 2 * 6 * 71]


def shape_id(s):
    return "%dx%dx%d" % s


# ------------------------------------------------------------------------------------------------------------------------- the restatement
def _ranks(S, axis):
    """Position of every entry in the stable descending order of its line along `axis`."""
    order = np.argsort(-S, axis=axis, kind="stable")
    shape = [1] * S.ndim
    shape[axis] = S.shape[axis]
    r = np.empty(S.shape, np.int64)
    np.put_along_axis(r, order, np.arange(S.shape[axis]).reshape(shape), axis=axis)
    return r


class Matcher:
    """match() for one `logs` with the rankings kept between calls (they depend on use_dustbin only)."""

    def __init__(self, logs):
        self.logs = np.ascontiguousarray(np.asarray(logs, np.float32))
        assert self.logs.ndim == 3
        self.P64 = np.exp(self.logs.astype(np.float64))
        self.P = self.P64.astype(np.float32)
        self._r = {}

    def _rank(self, use_dustbin):
        if use_dustbin not in self._r:
            S = self.P if use_dustbin else self.P[:, :-1, :-1]
            self._r[use_dustbin] = (S, _ranks(S, 2), _ranks(S, 1))
        return self._r[use_dustbin]

    def sides(self, K, use_dustbin, threshold):
        """(row side, column side) as bool [B, M, N], before `mutual` and the masks."""
        S, rr, rc = self._rank(bool(use_dustbin))
        row_sel, col_sel = rr < K, rc < K
        if use_dustbin:
            ref = row_sel & (S > S[:, :, -1:])
            src = col_sel & (S > S[:, -1:, :])
            return ref[:, :-1, :-1], src[:, :-1, :-1]
        thr, zero = np.float32(threshold), np.float32(0)
        return np.where(row_sel, S, zero) > thr, np.where(col_sel, S, zero) > thr

    def match(self, row_mask, col_mask, K, mutual, use_dustbin, threshold, global_scores):
        B, M1, N1 = self.logs.shape
        assert K >= 1
        ref, src = self.sides(K, use_dustbin, threshold)
        corr = (ref & src) if mutual else (ref | src)
        if row_mask is not None:
            corr = corr & np.asarray(row_mask, bool)[:, :, None]
        if col_mask is not None:
            corr = corr & np.asarray(col_mask, bool)[:, None, :]
        b, i, j = np.nonzero(corr)                                   # row-major
        scores = self.P64[b, i, j]
        if global_scores is not None:
            scores = scores * np.asarray(global_scores, np.float32).astype(np.float64)[b]
        return np.stack([b, i, j], 1).astype(np.int32).reshape(-1, 3), scores


def match(logs, row_mask, col_mask, K, mutual, use_dustbin, threshold, global_scores):
    return Matcher(logs).match(row_mask, col_mask, K, mutual, use_dustbin, threshold, global_scores)


def naive_match(logs, row_mask, col_mask, K, mutual, use_dustbin, threshold, global_scores):
    """The same contract as slowly as it can be said: per line, K times, pick the best entry not picked yet (first index among equal values)."""
    logs = np.asarray(logs, np.float32)
    P64 = np.exp(logs.astype(np.float64))
    P = P64.astype(np.float32)
    B, M, N = logs.shape[0], logs.shape[1] - 1, logs.shape[2] - 1
    Mr, Nr = (M + 1, N + 1) if use_dustbin else (M, N)
    thr = np.float32(threshold)
    rows = []
    for b in range(B):
        picked_r = [[False] * Nr for _ in range(Mr)]
        picked_c = [[False] * Nr for _ in range(Mr)]
        for i in range(Mr):
            for _ in range(min(K, Nr)):
                best = None
                for j in range(Nr):
                    if not picked_r[i][j] and (best is None or P[b, i, j] > P[b, i, best]):
                        best = j
                picked_r[i][best] = True
        for j in range(Nr):
            for _ in range(min(K, Mr)):
                best = None
                for i in range(Mr):
                    if not picked_c[i][j] and (best is None or P[b, i, j] > P[b, best, j]):
                        best = i
                picked_c[best][j] = True
        for i in range(M):
            for j in range(N):
                p = P[b, i, j]
                if use_dustbin:
                    fr, fc = picked_r[i][j] and p > P[b, i, N], picked_c[i][j] and p > P[b, M, j]
                else:
                    fr, fc = (p if picked_r[i][j] else np.float32(0)) > thr, (p if picked_c[i][j] else np.float32(0)) > thr
                keep = (fr and fc) if mutual else (fr or fc)
                if keep and (row_mask is None or row_mask[b][i]) and (col_mask is None or col_mask[b][j]):
                    rows.append((b, i, j))
    bij = np.array(rows, np.int32).reshape(-1, 3)
    sc = P64[bij[:, 0], bij[:, 1], bij[:, 2]]
    if global_scores is not None:
        sc = sc * np.asarray(global_scores, np.float32).astype(np.float64)[bij[:, 0]]
    return bij, sc


# ------------------------------------------------------------------------------------------------------------------------------ the inputs
class Case:
    """logs f32 [B, M+1, N+1], row_mask / col_mask bool [B, M] / [B, N] (None in mask mode "none"), global_scores f32 [B], `planted`: what was
    constructed on top of the draw (name -> indices), `zero_pair`: the problems that must give no pair in the dustbin form."""


def make_case(shape, level, mask_mode, seed=1):
    """Integer levels q in [0, L), logs = -(q / 64).  Planted in problem 0 wherever the shape has room (each is ASSERTED by
    tests/test_matching_cpu.py::test_planted_structures_are_there, none is left to the draw):
      row_max    row 0's maximum (strictly above the rest of the row, dustbin included) in columns 0, 64 and 128: one lane of the small kernel
      col_max    column 2's maximum in rows 1, 2 and 5: i and i + 1 are different wavefronts, i and i + 4 the same one
      row_run    row 6: the three largest values are equal, in columns 1, 3 and N - 1, everything else in the row (its dustbin too) is lower,
                 so the K-th element of K = 1 and 2 falls inside a run of equal values and that of K = 3 on its last member
      col_run    column 6: the same down rows 7, 9 and M - 1
      row_dust   row 3's dustbin equals the row's interior maximum;  col_dust: column 4's dustbin equals the column's interior maximum
    and, where B == 3: problem 1 is all MASKED, problem 2 has every interior entry below both of its dustbins.
    Masks are valid with probability 0.8, index 0 and the planted lines always; "inf" sets masked lines to MASKED, "gate" leaves their values."""
    B, M, N = shape
    L = LEVELS[level]
    rng = np.random.default_rng([seed, B, M, N, L, MASK_MODES.index(mask_mode)])
    q = rng.integers(0, L, size=(B, M + 1, N + 1))
    rm = rng.random((B, M)) < 0.8
    cm = rng.random((B, N)) < 0.8
    rm[:, 0] = True
    cm[:, 0] = True
    gs = rng.uniform(0.5, 2.0, size=B).astype(np.float32)
    planted = {}
    if M >= 40 and N >= 40:
        q[0, 6, :] = np.maximum(q[0, 6, :], 2)                   # the dustbins too: the run is at the top of the line in both forms
        q[0, :, 6] = np.maximum(q[0, :, 6], 2)
        q[0, 6, [1, 3, N - 1]] = 1
        q[0, [7, 9, M - 1], 6] = 1
        planted["row_run"], planted["col_run"] = (6, (1, 3, N - 1)), (6, (7, 9, M - 1))
        rm[0, [6, 7, 9, M - 1]] = True
        cm[0, [6, 1, 3, N - 1]] = True
    if M >= 3 and N >= 3:
        rows = [i for i in (1, 2, 5) if i < M]
        q[0, :, 2] = np.maximum(q[0, :, 2], 1)
        q[0, rows, 2] = 0
        planted["col_max"] = (2, tuple(rows))
        rm[0, rows] = True
        cm[0, 2] = True
    cols = [j for j in (0, 64, 128) if j < N]
    q[0, 0, :] = np.maximum(q[0, 0, :], 1)
    q[0, 0, cols] = 0
    planted["row_max"] = (0, tuple(cols))
    cm[0, cols] = True
    zero_pair = ()
    if B == 3:
        q[2, :M, :N] = np.maximum(q[2, :M, :N], 1)
        q[2, M, :] = 0
        q[2, :, N] = 0
        zero_pair = (1, 2)
    logs = (-(q.astype(np.float64) / 64)).astype(np.float32)
    if B == 3:
        logs[1] = MASKED
    rm[0, 3:4] = True                                                # row_dust / col_dust below: set after the masked lines are written
    cm[0, 4:5] = True
    if mask_mode == "inf":
        for b in range(B):
            logs[b, :M][~rm[b]] = MASKED
            logs[b, :, :N][:, ~cm[b]] = MASKED
    if M > 3:
        logs[0, 3, N] = logs[0, 3, :N].max()
        planted["row_dust"] = 3
    if N > 4:
        logs[0, M, 4] = logs[0, :M, 4].max()
        planted["col_dust"] = 4
    c = Case()
    c.shape, c.level, c.mask_mode = shape, level, mask_mode
    c.logs, c.global_scores, c.planted, c.zero_pair = logs, gs, planted, zero_pair
    c.row_mask, c.col_mask = (None, None) if mask_mode == "none" else (rm, cm)
    c.positive_threshold = POSITIVE_THRESHOLD[level]
    return c


def ks_for(N):
    return (1, 2, 3, 5, N, N + 1, N + 5)


def switches(level):
    """(use_dustbin, threshold) of the top-K sweep."""
    return ((1, 0.0), (0, -1.0), (0, 0.0), (0, POSITIVE_THRESHOLD[level]))


def side_kinds(m, case, K, use_dustbin, threshold):
    """(row side only, column side only, both) pair counts after the masks: what a test needs to know that `mutual` and the OR are both at work."""
    ref, src = m.sides(K, use_dustbin, threshold)
    B, M, N = case.shape
    v = np.ones((B, M, N), bool)
    if case.row_mask is not None:
        v = case.row_mask[:, :, None] & case.col_mask[:, None, :]
    return int((ref & ~src & v).sum()), int((~ref & src & v).sum()), int((ref & src & v).sum())
