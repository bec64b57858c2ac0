"""fp64 torch restatement of the global-descriptor head (lcr_netvlad_forward, csrc/netvlad.hip), stage by stage, for a stack of scans;
the shared inputs of tests/test_netvlad_cpu.py and tests/test_netvlad_gpu.py; and the calibration constants the GPU tolerance comes from.

The stages (GlobalDescritionHEAD = F.normalize -> NetVLADLoupe2 (eval) -> GatingContext -> F.normalize), per scan:
   1 row L2-normalise, eps 1e-12            6 V = x^T·a - asum·cluster_weights2         10 BatchNorm (bn2)
   2 x·cluster_weights                      7 per-cluster normalise over the 1024       11 gating GEMV, BatchNorm, sigmoid
   3 eval BatchNorm (bn1), eps 1e-5           features, eps 1e-6                        12 product
   4 softmax over the 64 clusters           8 normalise the 65536-vector, eps 1e-6      13 L2-normalise, eps 1e-12
   5 column sums asum                       9 ·hidden1_weights
Stages 1-4 act on single rows, so they run once over the stack; 5-8 run per segment; 9-13 act on single scans again.

`mutate=` plants exactly ONE wrong step (MUTATIONS).  The CPU test measures how far each one moves the fp64 descriptor on the cases meant to
catch it and demands 20 x the GPU tolerance: a GPU comparison that could not see the planted mistake fails there, without a GPU and without a
kernel being broken on purpose.
"""
import contextlib
import functools

import numpy as np
import torch

F_DIM, K_DIM, D_DIM = 1024, 64, 256
BN_EPS = 1e-5

MUTATIONS = ("asum_drop_last_row", "asum_take_next_row", "v_drop_last_row", "v_take_next_row", "asum_from_previous_segment",
             "hidden_drop_last_slice", "bn_eps_zero", "skip_global_norm", "no_gate")

# ------------------------------------------------------------------------------------------------ calibration (tests/test_netvlad_cpu.py)
# max |fp32 oracle.torch_ref.global_descriptor - fp64 restatement| over every case of the GPU file, per weight set, the fp32 run with its
# sums in plain index order (pinned_fp32_matmul below: the BLAS of the machine at hand does not enter).
# test_fp32_floor_matches_committed_constant recomputes it and fails when it leaves [FLOOR / 2, 2 FLOOR].
FLOOR = {"seeded": 4.8e-6, "stress": 3.9e-5}
DESC_TOL = 1e-4          # the project's descriptor bound (smoke(), test_descriptor_matches_reference_golden, ...)
MARGIN = 4               # HIP re-associates the same fp32 sums three more ways (256-slice split-K, 16-way column partials, MFMA K-blocking),
                         # each worth about one floor
TOL = {k: min(DESC_TOL, MARGIN * v) for k, v in FLOOR.items()}
SENSITIVITY = 20         # every mutation moves the fp64 descriptor by >= SENSITIVITY * TOL on the cases assigned to it

# ------------------------------------------------------------------------------------------------ the cases (shared by both test files)
WEIGHT_SEED = 11
KINDS = ("seeded", "stress")
EDGE_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 350)   # k_colsum64 splits rows 16 ways; the batched GEMM steps K by 32
BATCH_SIZES = (1, 7, 8, 9, 16, 17, 63, 64, 65, 66, 129)                  # k_hidden_splitk<8> groups of 8; aggregation chunks of 64
SMALL_SEGMENT = 65       # row mutations are assigned to segments of at most this many rows


def batch_lengths(S):
    """S segment lengths in 1..40 from a fixed seeded pattern (the same prefix for every S; 129 of them total 2572 rows < 3000)."""
    pattern = np.random.default_rng(20240).integers(1, 41, size=max(BATCH_SIZES))
    return tuple(int(v) for v in pattern[:S])


def cases():
    """name -> (seg_lens, feature seed): every stack the GPU file runs.  Single lengths, the ragged batch of all of them both ways round,
    the batch-size edges, the workspace test's in-between call."""
    out = {}
    for i, n in enumerate(EDGE_LENGTHS):
        out[f"len{n}"] = ((n,), 100 + i)
    out["ragged"] = (tuple(EDGE_LENGTHS), 200)
    out["ragged_rev"] = (tuple(reversed(EDGE_LENGTHS)), 201)
    for S in BATCH_SIZES:
        out[f"batch{S}"] = (batch_lengths(S), 300 + S)
    out["hygiene3"] = (batch_lengths(3), 400)            # the small call between the two identical 17-scan calls of the workspace test
    return out


def _stacked(seg_lens):
    return len(seg_lens) >= 2


def _has_small(seg_lens):
    return any(n <= SMALL_SEGMENT for n in seg_lens)


# (mutation, weight set) -> (predicate on seg_lens, mode): the cases meant to catch the mutation.  mode "every": EVERY judged segment of such a
# case moves by SENSITIVITY * TOL; mode "any": at least one does, which is what makes the case's comparison fail.
#   * A row taken from, or an a_sum borrowed from, a neighbouring segment needs a neighbour: those belong to stacks.
#   * The row mutations belong to segments of <= SMALL_SEGMENT rows (the 350-row case is a workload-sized sample, assigned to none) and to the
#     seeded set: its flat softmax spreads every row over all 64 columns.  Under the stress set's saturated softmax a row lands in one or
#     two columns whose per-column normalisation absorbs most of it (fp64 shifts down to 8e-4) while TOL sits at the 1e-4 cap; the kernels and
#     the segment shapes are the same for both sets, so the seeded comparison is the one that sees a row mistake.
#   * bn_eps_zero shows only where a variance is of the epsilon's size: the stress set.  How far one scan moves depends on where its
#     pre-BatchNorm values fall (4e-4 .. 1e-1), so it is assigned to stacks of >= 7 scans, one of which always moves enough.
#   * skip_global_norm: with the seeded set all 64 columns have unit norm and the skipped divisor is 8 in every scan.  With the stress set a
#     one-row scan has a single live column (divisor 1: nothing to skip), so there it is assigned to stacks.
_EVERY_CASE = lambda L: True
_ROW_DROP = lambda L: _has_small(L)
_ROW_TAKE = lambda L: _stacked(L) and _has_small(L[:-1])
ASSIGNED = {
    ("asum_drop_last_row", "seeded"): (_ROW_DROP, "every"),
    ("v_drop_last_row", "seeded"): (_ROW_DROP, "every"),
    ("asum_take_next_row", "seeded"): (_ROW_TAKE, "every"),
    ("v_take_next_row", "seeded"): (_ROW_TAKE, "every"),
    ("asum_from_previous_segment", "seeded"): (_stacked, "every"),
    ("asum_from_previous_segment", "stress"): (_stacked, "every"),
    ("hidden_drop_last_slice", "seeded"): (_EVERY_CASE, "every"),
    ("hidden_drop_last_slice", "stress"): (_EVERY_CASE, "every"),
    ("bn_eps_zero", "stress"): (lambda L: len(L) >= 7, "any"),
    ("skip_global_norm", "seeded"): (_EVERY_CASE, "every"),
    ("skip_global_norm", "stress"): (_stacked, "any"),
    ("no_gate", "seeded"): (_EVERY_CASE, "every"),
    ("no_gate", "stress"): (_EVERY_CASE, "every"),
}


def judged_segments(mutation, seg_lens):
    """Indices of the segments the mutation is judged on: for the row mutations the segments of <= SMALL_SEGMENT rows that the mutation
    changes at all, otherwise every segment it changes."""
    S = len(seg_lens)
    idx = list(range(S))
    if mutation in ("asum_take_next_row", "v_take_next_row"):
        idx = idx[:-1]                                   # the last segment has no following row
    if mutation == "asum_from_previous_segment":
        idx = idx[1:]                                    # the first has no predecessor
    if mutation in ("asum_drop_last_row", "asum_take_next_row", "v_drop_last_row", "v_take_next_row"):
        idx = [s for s in idx if seg_lens[s] <= SMALL_SEGMENT]
    return idx


# ------------------------------------------------------------------------------------------------ inputs
_SHAPES = {
    "cluster_weights": (F_DIM, K_DIM), "cluster_weights2": (1, F_DIM, K_DIM), "hidden1_weights": (F_DIM * K_DIM, D_DIM),
    "bn1.weight": (K_DIM,), "bn1.bias": (K_DIM,), "bn1.running_mean": (K_DIM,), "bn1.running_var": (K_DIM,),
    "bn2.weight": (D_DIM,), "bn2.bias": (D_DIM,), "bn2.running_mean": (D_DIM,), "bn2.running_var": (D_DIM,),
    "context_gating.gating_weights": (D_DIM, D_DIM),
    "context_gating.bn1.weight": (D_DIM,), "context_gating.bn1.bias": (D_DIM,), "context_gating.bn1.running_mean": (D_DIM,),
    "context_gating.bn1.running_var": (D_DIM,),
}


@functools.lru_cache(maxsize=None)
def netvlad_weights(kind, seed=WEIGHT_SEED):
    """The 16 `netvlad.*` tensors (fp32, keys WITH the prefix) from lcrnet_amd.weights.seeded_tensor; no encoder is built.  Treat as
    read-only (cached).  kind "stress" puts BatchNorm, the softmax and the clamps where a mistake in them shows: a sharp softmax with one
    negative scale, a dead cluster whose column falls under the 1e-6 clamp, running variances of the size of the epsilon's neighbourhood,
    shifted bn2 means, two saturated gates."""
    from lcrnet_amd.weights import seeded_tensor
    assert kind in KINDS, kind
    sd = {"netvlad." + k: seeded_tensor("netvlad." + k, shape, torch.float32, seed) for k, shape in _SHAPES.items()}
    if kind == "stress":
        p = "netvlad."
        sd[p + "bn1.weight"] *= 4.0
        sd[p + "bn1.weight"][5] *= -1.0
        sd[p + "bn1.bias"][9] = -200.0
        sd[p + "bn1.running_var"][[3, 40]] = 1e-3
        sd[p + "bn2.running_var"][[0, 100, 255]] = 1e-3
        sd[p + "context_gating.bn1.running_var"][[1, 77]] = 1e-3
        sd[p + "bn2.running_mean"][[7, 8]] = 3.0
        sd[p + "context_gating.bn1.bias"][20] += 30.0
        sd[p + "context_gating.bn1.bias"][21] -= 30.0
    return sd


@functools.lru_cache(maxsize=None)
def netvlad_weights64(kind, seed=WEIGHT_SEED):
    return {k: v.double() for k, v in netvlad_weights(kind, seed).items()}


def middle_zero_rows(seg_lens):
    """Stack row index of the middle row of every segment of >= 3 rows."""
    rows, o = [], 0
    for n in seg_lens:
        if n >= 3:
            rows.append(o + n // 2)
        o += n
    return rows


def netvlad_features(seg_lens, seed, zero_rows="middle"):
    """fp32 [sum(seg_lens), 1024] ReLU-like rows: randn scaled per row by U(0.1, 40), clamped at 0 (row norms ~2 .. ~1000: inside the range
    where neither fp32 path underflows the squared norm).  zero_rows: stack rows set to exactly 0 — "middle" = middle_zero_rows."""
    n = int(sum(seg_lens))
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(n, F_DIM, generator=g) * (0.1 + 39.9 * torch.rand(n, 1, generator=g))
    x = x.clamp_(min=0.0)
    rows = middle_zero_rows(seg_lens) if isinstance(zero_rows, str) else list(zero_rows or [])
    if rows:
        x[rows] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ the restatement
def _bn(sd, pfx, x, eps):
    return (x - sd[pfx + "running_mean"]) / torch.sqrt(sd[pfx + "running_var"] + eps) * sd[pfx + "weight"] + sd[pfx + "bias"]


def describe(sd, feats, seg_lens, mutate=None, intermediates=False, pfx="netvlad."):
    """sd: the netvlad.* tensors as fp64; feats [sum(seg_lens), 1024] -> fp64 [S, 256] descriptors (and, on request, a dict of the
    intermediates in the layout of the HIP workspace: xn [n,1024], act [n,64], asum [S,64], V [S,1024,64] after both normalisations,
    hidden [S,256] before bn2, gates [S,256])."""
    assert mutate is None or mutate in MUTATIONS, mutate
    x = feats.double()
    n_rows = x.shape[0]
    assert x.shape[1] == F_DIM and n_rows == sum(seg_lens) and all(n > 0 for n in seg_lens)
    eps = 0.0 if mutate == "bn_eps_zero" else BN_EPS
    xn = x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)                                    # 1
    act = xn @ sd[pfx + "cluster_weights"]                                                   # 2
    act = torch.softmax(_bn(sd, pfx + "bn1.", act, eps), dim=1)                              # 3, 4
    w2 = sd[pfx + "cluster_weights2"][0]
    offs = np.concatenate([[0], np.cumsum(seg_lens)]).astype(np.int64)
    rows_of = lambda s: (int(offs[s]), int(offs[s + 1]))
    asums, Vs = [], []
    for s in range(len(seg_lens)):
        lo, hi = rows_of(s)
        alo, ahi, vlo, vhi = lo, hi, lo, hi
        if mutate == "asum_drop_last_row":
            ahi = hi - 1
        elif mutate == "asum_take_next_row":
            ahi = min(hi + 1, n_rows)
        elif mutate == "v_drop_last_row":
            vhi = hi - 1
        elif mutate == "v_take_next_row":
            vhi = min(hi + 1, n_rows)
        elif mutate == "asum_from_previous_segment" and s > 0:
            alo, ahi = rows_of(s - 1)
        asum = act[alo:ahi].sum(0)                                                           # 5
        V = xn[vlo:vhi].t() @ act[vlo:vhi] - asum[None, :] * w2                              # 6   (1024, 64)
        V = V / V.norm(dim=0, keepdim=True).clamp(min=1e-6)                                  # 7
        if mutate != "skip_global_norm":
            V = V / V.norm().clamp(min=1e-6)                                                 # 8
        asums.append(asum)
        Vs.append(V)
    asum, V = torch.stack(asums), torch.stack(Vs)
    flat, H = V.reshape(len(seg_lens), -1), sd[pfx + "hidden1_weights"]
    if mutate == "hidden_drop_last_slice":
        cut = F_DIM * K_DIM - 256
        flat, H = flat[:, :cut], H[:cut]
    hidden = flat @ H                                                                        # 9
    o = _bn(sd, pfx + "bn2.", hidden, eps)                                                   # 10
    g = o @ sd[pfx + "context_gating.gating_weights"]                                        # 11
    gates = torch.sigmoid(_bn(sd, pfx + "context_gating.bn1.", g, eps))
    a = o if mutate == "no_gate" else o * gates                                              # 12
    desc = a / a.norm(dim=1, keepdim=True).clamp(min=1e-12)                                  # 13
    if intermediates:
        return desc, {"xn": xn, "act": act, "asum": asum, "V": V, "hidden": hidden, "gates": gates}
    return desc


@functools.lru_cache(maxsize=None)
def reference(kind, case, mutate=None):
    """fp64 descriptors [S,256] of a named case (cached; computed once and shared by the tests — do not modify)."""
    seg_lens, seed = cases()[case]
    return describe(netvlad_weights64(kind), netvlad_features(seg_lens, seed), seg_lens, mutate=mutate)


# ------------------------------------------------------------------------------------------------ the fp32 floor, with a pinned summation order
# torch's fp32 matmul sums in whatever order the BLAS kernel of the machine at hand uses, and for the 65536-term hidden projection that
# order IS the floor: the same inputs gave 4.9e-6 / 4.5e-5 (seeded / stress) on one CPU and 1.0e-6 / 1.1e-5 on another, so no committed
# constant could hold within 2x.  The floor is therefore taken with the one order that needs no choice: plain fp32 in index order — every
# product rounded to fp32, the products added one after the other for k = 0, 1, 2, ..., every addition rounded to fp32, no fused
# multiply-add.  Products and additions of IEEE fp32 are the same on every machine, so the constant is too (what is left to the machine
# are the fp32 norms, exp and sigmoid of the oracle, 1e-7 relative).  It is the largest of the orders above: blocked or vectorised
# kernels, the HIP ones included, shorten the chain of roundings and only come closer to fp64.
_torch_matmul = torch.matmul
_CHUNK_ELEMS = 1 << 19


def fp32_matmul(a, b):
    """a [..., m, K] @ b [K, n] or [..., K, n] in plain index-order fp32 (see above); other dtypes go to torch.matmul."""
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        return _torch_matmul(a, b)
    K, n = a.shape[-1], b.shape[-1]
    assert b.shape[-2] == K and K > 0
    A = np.moveaxis(a.numpy(), -1, 0)[..., None]                                     # [K, ..., m, 1]
    B = np.moveaxis(b.numpy(), -2, 0)                                                # [K, ..., n] or [K, n]
    B = B.reshape(K, *([1] * (A.ndim - 3)), 1, n) if b.dim() == 2 else B[..., None, :]
    shape = np.broadcast_shapes(A.shape[1:], B.shape[1:])
    step = max(1, _CHUNK_ELEMS // max(1, int(np.prod(shape))))
    acc = np.zeros(shape, np.float32)
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        buf = np.empty((k1 - k0 + 1,) + shape, np.float32)
        buf[0] = acc
        np.multiply(A[k0:k1], B[k0:k1], out=buf[1:])
        # numpy reduces an OUTER axis row by row (out += row, in order); pairwise summation is its inner-axis path only
        # (test_fp32_matmul_is_index_order_fp32 holds it against the explicit loop)
        acc = np.add.reduce(buf, axis=0)
    return torch.from_numpy(acc)


@contextlib.contextmanager
def pinned_fp32_matmul():
    """Inside: torch.matmul(fp32, fp32) is fp32_matmul (oracle.torch_ref spells every product of the head torch.matmul)."""
    torch.matmul = fp32_matmul
    try:
        yield
    finally:
        torch.matmul = _torch_matmul
