"""Scan Context loop detection (Kim & Kim, IROS 2018): the learning-free counterpart of `loop_closure.detect_loops`.

A polar max-height image per scan (include/lcr_hip.h, lcr_scan_context), compared under all column shifts.  No checkpoint is needed, so
this is what a loop-detection claim can be made with before any training; the best shift also gives the yaw the registration that follows
can start from, which a global descriptor cannot.  Two searches over a sequence:
  * `scan_context_topk`: the exhaustive causal search (every admissible pair on the fp32 MFMA path), the paper's definition;
  * `two_stage_topk`: the classical form, a ring-key nearest-neighbour search (`retrieval.retrieval_topk` at D = R) whose candidates are
    re-scored by `functional.scan_context_distance`.
`detect_loops` returns rows in the layout of `loop_closure.detect_loops`, so `io_formats.save_pair_dist`, `io_formats.top1_with_threshold`
and `evaluation.compute_*` work on them unchanged.  Everything runs on the GPU; there is no CPU fallback."""
import collections
import math

import numpy as np
import torch

from . import functional as F
from . import io_formats as io
from .retrieval import retrieval_topk

K, EXCLUDE, START = 50, 100, 101          # the search window of loop_closure.detect_loops

ScanContexts = collections.namedtuple("ScanContexts", "desc ring_key unit mask")


def sequence_scan_contexts(clouds, batch=F.SCAN_CONTEXT_MAX_CLOUDS, **params):
    """clouds: device f32 [n_i, >= 3] per frame -> ScanContexts of the sequence (desc [C,R,W], ring_key [C,R], unit [C,R,W], mask [C]),
    `batch` <= 64 scans per native call.  params: R, W, max_length, lidar_height (functional.SCAN_CONTEXT_PARAMS)."""
    if not 1 <= batch <= F.SCAN_CONTEXT_MAX_CLOUDS:
        raise ValueError("sequence_scan_contexts: 1 <= batch <= %d" % F.SCAN_CONTEXT_MAX_CLOUDS)
    parts = []
    for f0 in range(0, len(clouds), batch):
        chunk = [c[:, :3] for c in clouds[f0:f0 + batch]]
        parts.append(F.scan_context(torch.cat(chunk).contiguous(), [len(c) for c in chunk], **params))
    return ScanContexts(*(torch.cat([p[i] for p in parts]) for i in range(4)))


def scan_context_topk(sc, q0, q1, k=K, exclude=EXCLUDE):
    """The exhaustive causal search for query frames [q0, q1): frame i sees frames [0, i - exclude) -> (idx int32 [q1-q0, k], dist f32,
    shift int32), rows ascending in (dist, index), padded with (-1, +inf, -1)."""
    return F.scan_context_topk(sc.unit, sc.mask, q0, q1 - q0, k, exclude)


def two_stage_topk(sc, n_candidates, k=K, exclude=EXCLUDE, q0=0, q1=None):
    """The classical two-stage search for query frames [q0, q1): the `n_candidates` nearest ring keys among frames [0, i - exclude), re-scored
    by the full distance -> (idx, dist, shift) as scan_context_topk returns them, k <= n_candidates."""
    C = sc.unit.shape[0]
    q1 = C if q1 is None else q1
    if not 1 <= k <= n_candidates:
        raise ValueError("two_stage_topk: 1 <= k <= n_candidates")
    Q = q1 - q0
    cand, _ = retrieval_topk(sc.ring_key[q0:q1], q0, sc.ring_key, n_candidates, exclude)            # int32 [Q, n], -1 = none
    rows = torch.arange(q0, q1, dtype=torch.int32, device=cand.device)[:, None].expand(Q, n_candidates)
    dist, shift, _ = F.scan_context_distance(sc.unit, sc.mask, torch.stack([rows, cand], -1).reshape(-1, 2))    # a -1 candidate: (NaN, -1)
    dist, shift = dist.reshape(Q, n_candidates), shift.reshape(Q, n_candidates)
    none = cand < 0
    dist = torch.where(none, torch.full_like(dist, math.inf), dist)
    # ascending in (dist, index), the missing candidates last: two stable sorts
    o1 = torch.argsort(torch.where(none, torch.full_like(cand, 2 ** 31 - 1), cand), dim=1, stable=True)
    o2 = torch.argsort(torch.gather(dist, 1, o1), dim=1, stable=True)
    order = torch.gather(o1, 1, o2)[:, :k]
    return torch.gather(cand, 1, order), torch.gather(dist, 1, order), torch.gather(shift, 1, order)


def detect_loops(sc, thres, k=K, exclude=EXCLUDE, start=START, n_candidates=None):
    """ScanContexts of a sequence -> (rows float64 [Q*k,3] = (i, j, dist) as loop_closure.detect_loops lays them out, kept float32 [n,3] =
    the rows under `thres`, yaw = dict(shift int32 [Q,k], yaw float64 [Q,k] = shift * 2 pi / W in radians: Rz(-yaw) brings frame j into
    frame i's heading)).  Query frames are [start, C - 1); n_candidates selects the two-stage search instead of the exhaustive one."""
    C, W = sc.unit.shape[0], sc.unit.shape[2]
    if C - 1 <= start:
        return np.zeros((0, 3)), np.zeros((0, 3), np.float32), dict(shift=np.zeros((0, k), np.int32), yaw=np.zeros((0, k)))
    if n_candidates is None:
        idx, dist, shift = scan_context_topk(sc, start, C - 1, k, exclude)
    else:
        idx, dist, shift = two_stage_topk(sc, n_candidates, k, exclude, start, C - 1)
    idx_h, dist_h, shift_h = idx.cpu().numpy(), dist.cpu().numpy(), shift.cpu().numpy()
    rows = io.pair_dist_rows(np.arange(start, C - 1), idx_h, np.where(idx_h >= 0, dist_h, np.inf))
    yaw = np.where(shift_h >= 0, shift_h * (2.0 * np.pi / W), np.nan)
    return rows, io.top1_with_threshold(rows, C, thres), dict(shift=shift_h, yaw=yaw)
