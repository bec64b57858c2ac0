"""Thin tensor-level wrappers over the C ABI (include/lcr_hip.h).  No arithmetic happens in Python: every function
allocates the outputs with torch and launches HIP kernels on the current stream.  Inference only (no autograd), with two exceptions:
gap_loss / min_dist have the gradient launchers gap_loss_grad / min_dist_grad beside them, which losses.py wraps in
torch.autograd.Functions (gradients to the scores and to the queries only); and log_optimal_transport / patch_log_optimal_transport
are differentiable (_TransportFn over lcr_log_sinkhorn_grad: gradients to the raw scores and to alpha; _PatchTransportFn adds
lcr_patch_scores_grad: gradients to the two point-feature tensors); bmm_nt and the plain gemm(a, b, trans_b=True) carry a graph; and the ops of the 3D-RoFormer —
linear, rotary_embed, attention, add_layernorm — return a graph when grad mode is on and an input requires grad (backwards in
csrc/attention_grad.hip and on lcr_gemm_f32), and otherwise make exactly the calls of the inference path."""
import ctypes
import os
import threading

import numpy as np
import torch

from . import _lib

GN_EPS = 1e-5
GN_REPLICAS = 8   # must match csrc/common.h: statistics tables are [GN_REPLICAS, S, groups, 2]


class KernelTimer:
    """Opt-in per-launch timing of lcr_gemm_f32 ("gemm", meta (M,N,K)) and lcr_kpconv_aggregate ("kpconv_aggregate", meta
    (M,Ns,H,C,index bytes)) with HIP events on the launch stream, recorded inside the library (so launches issued by the native
    encoder driver are seen too).  set_timer(t) starts a fresh log, set_timer(None) stops logging, t.summary() synchronises."""
    KINDS = {"gemm": 0, "kpconv_aggregate": 1, "radius_query": 2, "attention": 3, "kpconv_fused": 4, "sinkhorn": 5}

    def __init__(self, names):
        self.names = set(names)
        self._cache = None

    def summary(self):
        """name -> [(seconds between the events bracketing the launch on its stream, meta)]"""
        return {k: [(b, m) for b, _, m in v] for k, v in self.records().items()}

    def records(self):
        """name -> [(bracketed seconds, the kernel's own begin-to-end seconds or None, meta)].  The bracketed time contains whatever
        the launch waited for in its queue (other streams' kernels holding the CUs); the kernel's own time is what a profiler's kernel
        trace reports."""
        if self._cache is None:
            out = {}
            L = _lib.lib()
            for name in self.names:
                kind = self.KINDS[name]
                n = L.lcr_ktimer_read2(kind, 0, None, None, None)
                sec = (ctypes.c_double * max(n, 1))()
                ksec = (ctypes.c_double * max(n, 1))()
                meta = (ctypes.c_int64 * (5 * max(n, 1)))()
                L.lcr_ktimer_read2(kind, n, ctypes.cast(sec, ctypes.c_void_p), ctypes.cast(ksec, ctypes.c_void_p), ctypes.cast(meta, ctypes.c_void_p))
                width = 3 if name == "gemm" else 5            # radius_query: (nq_cap, ns_cap, limit, index bytes, B); attention: (sum Nq*Nk, P, heads, head_dim, 0); sinkhorn: (B, M, N, iters, form)
                out[name] = [(sec[i], ksec[i] if ksec[i] >= 0 else None, tuple(int(meta[5 * i + k]) for k in range(width))) for i in range(n)]
            self._cache = out
        return self._cache


def set_timer(timer, sample_every=1):
    """sample_every = n: only every n-th instrumented launch of each kind is timed (a timed launch is a profiled dispatch; with all
    of them timed the bench pipeline runs 7 % slower)."""
    _lib.lib().lcr_ktimer_sample(int(sample_every))
    mask = 0
    for name in (timer.names if timer is not None else ()):
        mask |= 1 << KernelTimer.KINDS[name]
    _lib.lib().lcr_ktimer_kinds(mask if timer is not None else 0xffffffff)     # only the kinds the timer asked for are clocked
    _lib.lib().lcr_ktimer_enable(1 if timer is not None else 0)


def _seg(seg_len, n, device):
    """GroupNorm segment lengths: None = the reference's behaviour (one segment = the whole stack)."""
    if seg_len is None:
        # a fill launch, NOT torch.tensor([n], device=...): that is a pageable host-to-device copy, after which torch synchronises the
        # stream — 25 pipeline drains per registration pair (profiles/r06_pair_host_profile.log)
        return torch.full((1,), int(n), dtype=torch.int64, device=device)
    return seg_len


def host_values(values, dtype, device):
    """A small host list as a device tensor without draining the stream: staged in pinned memory (torch's caching host allocator) and
    copied asynchronously on the current stream."""
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def host_tensor(t, device):
    """same for a host tensor / numpy array"""
    if not torch.is_tensor(t):
        t = torch.from_numpy(t)
    return t.pin_memory().to(device, non_blocking=True)


def _idx_args(idx):
    if idx.dtype == torch.int64:
        return 1
    if idx.dtype == torch.int32:
        return 0
    raise RuntimeError("neighbor indices must be int32 or int64")


class _StatsArena(threading.local):
    buf = None
    off = 0


_ARENA = _StatsArena()


class stats_arena:
    """Context manager: GroupNorm statistics tables of every GEMM / groupnorm_stats call inside are carved out of ONE zeroed
    fp64 buffer (one fill launch per forward pass instead of one per layer).  Per host thread; nests by replacement."""

    def __init__(self, device, entries=1 << 18):
        self.device, self.entries = device, entries

    def __enter__(self):
        self.prev = (_ARENA.buf, _ARENA.off)
        _ARENA.buf = torch.zeros(self.entries, dtype=torch.float64, device=self.device)
        _ARENA.off = 0
        return self

    def __exit__(self, *exc):
        _ARENA.buf, _ARENA.off = self.prev
        return False


def _zero_stats(S, groups, device):
    n = GN_REPLICAS * S * groups * 2
    buf = _ARENA.buf
    if buf is not None and buf.device == device and _ARENA.off + n <= buf.numel():
        v = buf[_ARENA.off:_ARENA.off + n].view(GN_REPLICAS, S, groups, 2)
        _ARENA.off += n
        return v
    return torch.zeros((GN_REPLICAS, S, groups, 2), dtype=torch.float64, device=device)


def _gemm_out(M, N, seg_len, groups, device, always_seg=False):
    """What every GEMM wrapper allocates: (C [M,N], the segment table to pass or None, S, the zeroed statistics table or None).
    The table is passed with `groups` only; always_seg: also without (gemm_anorm normalises A by it)."""
    c = torch.empty((M, N), dtype=torch.float32, device=device)
    if not (groups or always_seg):
        return c, None, 0, None
    if seg_len is None:
        seg_len = torch.full((1,), int(M), dtype=torch.int64, device=device)      # see _seg
    S = seg_len.numel()
    return c, seg_len, S, (_zero_stats(S, groups, device) if groups else None)


def gemm(a, b, trans_b=False, trans_a=False, bias=None, rowdiv=None, seg_len=None, groups=0, row_mask=None):
    """C = A·B (+ fused epilogue).  a: [M,K] ([K,M] if trans_a); b: [K,N] ([N,K] if trans_b, i.e. an nn.Linear weight).
    Returns (C, stats) where stats is the fp64 [GN_REPLICAS,S,groups,2] GroupNorm accumulator (sum the replicas; None if
    groups == 0).  The plain form a . b^T (trans_b alone, no epilogue) carries a graph when a or b requires grad and grad mode is on
    (_GemmNTFn: both gradient products on lcr_gemm_f32); every other form is a plain launch.  row_mask: the int16 [M] mask of kpconv_aggregate(emit_mask=True) for a = its aggregate (trans_b only): blocks
    whose bit is clear are read as zeros (lcr_gemm_f32_masked; where kpconv_mask_ok(M, N, K, False) holds)."""
    if row_mask is not None:
        return _gemm_masked(a, b, trans_b, trans_a, bias, rowdiv, seg_len, groups, row_mask)
    _lib.require_cuda(a, b)
    if trans_b and not trans_a and bias is None and rowdiv is None and seg_len is None and not groups and _wants_grad(a, b):
        return _GemmNTFn.apply(a, b), None          # the plain product A.B^T (the node-level scores): differentiable in both factors
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    N = b.shape[0] if trans_b else b.shape[1]
    assert (b.shape[1] if trans_b else b.shape[0]) == K, "inner dimensions differ"
    c, seg_len, S, stats = _gemm_out(M, N, seg_len, groups, a.device)
    _lib.call.lcr_gemm_f32(
        _lib.ptr(a), _lib.ptr(b), _lib.ptr(c), M, N, K, int(trans_a), int(trans_b), _lib.ptr(bias), _lib.ptr(rowdiv),
        _lib.ptr(seg_len), S, int(groups), _lib.ptr(stats), _lib.stream_ptr(a.device))
    return c, stats


def kpconv_mask_ok(M, N, K, split):
    """Whether the KPConv contraction [M, K = 15 C] x [K, N] may read a row-masked aggregate on the split-bf16 (split) or fp32 form and
    compute what the unmasked call computes (lcr_kpconv_mask_ok; environment LCR_KP_MASK=0: never)."""
    return bool(_lib.lib().lcr_kpconv_mask_ok(int(M), int(N), int(K), int(bool(split))))


def _mask_args(a, row_mask):
    M, K = a.shape
    assert row_mask.dtype == torch.int16 and row_mask.is_contiguous() and row_mask.numel() == M and row_mask.device == a.device
    assert K % 15 == 0
    return K // 15


def _gemm_masked(a, b, trans_b, trans_a, bias, rowdiv, seg_len, groups, row_mask):
    _lib.require_cuda(a, b)
    assert trans_b and not trans_a, "the masked form takes A [M,K] and B [N,K]"
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    block_k = _mask_args(a, row_mask)
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K, "inner dimensions differ"
    c, seg_len, S, stats = _gemm_out(M, N, seg_len, groups, a.device)
    _lib.call.lcr_gemm_f32_masked(
        _lib.ptr(a), _lib.ptr(b), _lib.ptr(c), M, N, K, _lib.ptr(bias), _lib.ptr(rowdiv), _lib.ptr(seg_len), S,
        int(groups), _lib.ptr(stats), _lib.ptr(row_mask), block_k, _lib.stream_ptr(a.device))
    return c, stats


# ---- split-bf16 form of the K-deep GEMMs (csrc/gemm_split.hip): fp32 operands as three bf16 terms, six products on the bf16 matrix cores.
# DEFAULT since round 5 for the K-deep shapes (K >= 288, K % 32 == 0, N >= 64): every fp32 operand enters as its three bf16 terms (exact), six
# of the nine cross products are accumulated in fp32 — measured error against fp64 at or below the fp32-MFMA kernel's own, non-finite values
# propagate to the same outputs (tests/test_gemm_split_gpu.py).  Since R12.1 also for the K = 128 / 256 Linears where it measured >= 1.10x the
# light fp32 kernel (gemm_split_ok below; LCR_GEMM_SPLIT_LIGHT=0: K >= 288 only).  LCR_GEMM_SPLIT=0 selects the true-fp32 MFMA kernel everywhere;
# `set_gemm_split` is the run-time switch (tests, bench A/B).  Domain of the split form: |x| <= 3.3895e38 (the largest bf16), beyond which
# the first term rounds to infinity.
_GEMM_SPLIT = [os.environ.get("LCR_GEMM_SPLIT", "1") not in ("", "0")]


def gemm_split_enabled():
    return _GEMM_SPLIT[0]


def set_gemm_split(on):
    _GEMM_SPLIT[0] = bool(on)


_GEMM_SPLIT_LIGHT = os.environ.get("LCR_GEMM_SPLIT_LIGHT", "1") not in ("", "0")


_GEMM_SPLIT_LIGHT_CLASSES = {(64, 128), (256, 128), (512, 128), (64, 256), (128, 256), (512, 256), (1024, 256)}     # (N, K), profiles/r12_light_split.md


def _gemm_split_light(N, K):
    return (N, K) in _GEMM_SPLIT_LIGHT_CLASSES


def gemm_split_ok(N, K):
    """The one dispatch rule for the Linears, a function of (N, K) alone: the mirror of lcr_gemm_split_ok (csrc/gemm_f32.hip, where the
    K <= 256 classes and their measurement are described; tests/test_gemm_split_light_gpu.py compares the two on every encoder shape)."""
    if N < 64 or K < 32 or K % 32 != 0:
        return False
    return K >= 288 or (_GEMM_SPLIT_LIGHT and K <= ANORM_MAX_K and _gemm_split_light(N, K))


# Derived weight tensors (transposed KPConv weights, bf16 planes, the native encoder's table) are built lazily by whichever host thread gets
# there first, on ITS current stream, and then used by every thread on other streams: the builder holds this lock and drains its stream before
# publishing, so a second worker (PairPipeline runs two) never launches a GEMM on a half-written operand.
derived_lock = threading.RLock()


class WeightStamp:
    """Identity of a weight tensor for the derived-tensor caches (transposed / split weights, host copies, the native encoder's table):
    the tensor OBJECT (weak reference), its address, its version counter and its device.  Address + version alone are not an identity: a
    buffer replaced by Module._apply (.cpu() / .cuda() / .to()) is a NEW tensor with version 0 that the caching allocator readily
    places at the address of the one it replaces — found by tools/fuzz_float_parity_gpu.py, which reloads seeded weights through
    .cpu() -> load_state_dict -> .cuda() and got the previous seed's kernel points in one case of eight."""
    __slots__ = ("ref", "ptr", "ver", "dev")

    def __init__(self, t):
        import weakref
        self.ref, self.ptr, self.ver, self.dev = weakref.ref(t), t.data_ptr(), t._version, t.device

    def same(self, t):
        return self.ref is not None and self.ref() is t and self.ptr == t.data_ptr() and self.ver == t._version and self.dev == t.device

    def __reduce__(self):                                   # pickled / copied modules start with caches that match nothing
        return (_dead_stamp, ())


def _dead_stamp():
    s = WeightStamp.__new__(WeightStamp)
    s.ref, s.ptr, s.ver, s.dev = None, 0, -1, None
    return s


def drop_derived(module, *names):
    """forget cached derived tensors of a module (called from its _apply override: every .to() / .cuda() / .cpu() / .float())"""
    for n in names:
        if n in module.__dict__:
            module.__dict__[n] = None



def publish_derived(t):
    """Call on a freshly built derived tensor before storing it where other threads / streams can see it."""
    torch.cuda.current_stream(t.device).synchronize()
    return t


def split_bf16x3(w):
    """The three bf16 terms of a constant fp32 operand [N,K] (K % 32 == 0) in the layout lcr_gemm_f32_bsplit reads them in
    (lcr_split_bf16x3_tiles; made once per weight): int16 [ceil(N/64), K/32, 3, 64, 32], i.e. one opaque 12 KB block per (64 columns,
    K-step of 32) whose 16-byte chunks (8 bf16 of one plane, column and 8-k group) are ordered as the MFMA's B operand is read:
    [column quarter wn 0..3][plane 0..2][lane 0..63], lane l holding column 16 wn + (l & 15), k 8 (l >> 4) .. + 7.
    Rows beyond N are zero.  The tensor carries N as `.lcr_n`."""
    w = w.detach().contiguous()
    N, K = w.shape
    assert K % 32 == 0
    tiles = torch.empty(((N + 63) // 64, K // 32, 3, 64, 32), dtype=torch.int16, device=w.device)
    _lib.call.lcr_split_bf16x3_tiles(_lib.ptr(w), int(N), int(K), _lib.ptr(tiles), _lib.stream_ptr(w.device))
    tiles.lcr_n = int(N)
    return tiles


def unsplit_bf16x3(tiles, padded=False):
    """Inverse view of split_bf16x3 for tests: the three terms as float32 [3, N, K] (columns and k back in order); padded=True keeps the
    zero rows of the last 64-column tile ([3, 64 ceil(N/64), K])."""
    CT, KS = tiles.shape[0], tiles.shape[1]
    t = tiles.view(CT, KS, 4, 3, 4, 16, 8)                                         # [ct, ks, wn, plane, lane >> 4, lane & 15, 8 k]
    t = t.permute(3, 0, 2, 5, 1, 4, 6).reshape(3, CT * 64, KS * 32)                # [plane, (ct, wn, lane & 15), (ks, lane >> 4, 8 k)]
    if not padded:
        t = t[:, :tiles.lcr_n]
    return t.contiguous().view(torch.bfloat16).float()


def gemm_bsplit(a, planes, bias=None, rowdiv=None, seg_len=None, groups=0, row_mask=None):
    """C = A[M,K] . B[N,K]^T with B given as the planes of split_bf16x3 (same epilogue and return value as gemm()).  row_mask: as in
    gemm() (lcr_gemm_f32_bsplit_masked)."""
    _lib.require_cuda(a, planes)
    assert a.dtype == torch.float32 and a.is_contiguous() and planes.dtype == torch.int16 and planes.is_contiguous() and planes.dim() == 5
    M, K = a.shape
    N = planes.lcr_n
    assert planes.shape[1] * 32 == K and planes.shape[0] == (N + 63) // 64, "inner dimensions differ"
    c, seg_len, S, stats = _gemm_out(M, N, seg_len, groups, a.device)
    if row_mask is not None:
        block_k = _mask_args(a, row_mask)
        _lib.call.lcr_gemm_f32_bsplit_masked(_lib.ptr(a), _lib.ptr(planes), _lib.ptr(c), M, N, K, _lib.ptr(bias), _lib.ptr(rowdiv), _lib.ptr(seg_len),
                                             S, int(groups), _lib.ptr(stats), _lib.ptr(row_mask), block_k, _lib.stream_ptr(a.device))
        return c, stats
    _lib.call.lcr_gemm_f32_bsplit(_lib.ptr(a), _lib.ptr(planes), _lib.ptr(c), M, N, K, _lib.ptr(bias), _lib.ptr(rowdiv),
                                  _lib.ptr(seg_len), S, int(groups), _lib.ptr(stats), _lib.stream_ptr(a.device))
    return c, stats


ANORM_MAX_K, ANORM_MIN_SEG_ROWS = 256, 64


def gemm_anorm_ok(K, N):
    """Shapes lcr_gemm_f32_anorm takes (the light GEMM form)."""
    return K <= ANORM_MAX_K and K % 4 == 0 and N > 32


def gemm_anorm(a, a_stats, a_gamma, a_beta, a_groups, weight, bias=None, seg_len=None, groups=0, slope=0.1):
    """C = LeakyReLU(GroupNorm(a)) · weight^T (+ bias), a being the RAW output whose sums are a_stats; the normalised tensor is
    never materialised (lcr_gemm_f32_anorm).  The caller guarantees every segment holds >= ANORM_MIN_SEG_ROWS rows.
    Returns (C, stats) like gemm()."""
    _lib.require_cuda(a, weight)
    assert a.dtype == torch.float32 and weight.dtype == torch.float32 and a.is_contiguous() and weight.is_contiguous()
    M, K = a.shape
    N = weight.shape[0]
    assert weight.shape[1] == K and gemm_anorm_ok(K, N)
    c, seg_len, S, stats = _gemm_out(M, N, seg_len, groups, a.device, always_seg=True)
    _lib.call.lcr_gemm_f32_anorm(
        _lib.ptr(a), _lib.ptr(weight), _lib.ptr(c), M, N, K, _lib.ptr(bias), _lib.ptr(a_stats), _lib.ptr(a_gamma), _lib.ptr(a_beta),
        int(a_groups), GN_EPS, float(slope), _lib.ptr(seg_len), S, int(groups), _lib.ptr(stats), _lib.stream_ptr(a.device))
    return c, stats


def gemm_bsplit_anorm(a, a_stats, a_gamma, a_beta, a_groups, planes, bias=None, seg_len=None, groups=0, slope=0.1):
    """gemm_anorm on the split-bf16 form: `planes` = split_bf16x3(weight) in place of the weight (lcr_gemm_f32_bsplit_anorm; N >= 64,
    K <= 256, K % 32 == 0).  The normalised operand is bit-equal to gemm_anorm's; the product has the split form's rounding points."""
    _lib.require_cuda(a, planes)
    assert a.dtype == torch.float32 and a.is_contiguous() and planes.dtype == torch.int16 and planes.is_contiguous() and planes.dim() == 5
    M, K = a.shape
    N = planes.lcr_n
    assert planes.shape[1] * 32 == K and planes.shape[0] == (N + 63) // 64, "inner dimensions differ"
    c, seg_len, S, stats = _gemm_out(M, N, seg_len, groups, a.device, always_seg=True)
    _lib.call.lcr_gemm_f32_bsplit_anorm(
        _lib.ptr(a), _lib.ptr(planes), _lib.ptr(c), M, N, K, _lib.ptr(bias), _lib.ptr(a_stats), _lib.ptr(a_gamma), _lib.ptr(a_beta),
        int(a_groups), GN_EPS, float(slope), _lib.ptr(seg_len), S, int(groups), _lib.ptr(stats), _lib.stream_ptr(a.device))
    return c, stats


def groupnorm_stats(x, groups, seg_len=None):
    seg_len = _seg(seg_len, x.shape[0], x.device)
    stats = _zero_stats(seg_len.numel(), groups, x.device)
    _lib.call.lcr_groupnorm_stats(_lib.ptr(x), x.shape[0], x.shape[1], groups, _lib.ptr(seg_len), seg_len.numel(),
                                  _lib.ptr(stats), _lib.stream_ptr(x.device))
    return stats


def groupnorm_apply(x, stats, gamma, beta, groups, seg_len=None, res=None, res_norm=None, slope=0.1, act=True, want_pos=False):
    """y = act(GN(x) [+ res | + GN(res)]); res_norm = (stats, gamma, beta) of the residual branch or None.  Differentiable in x, gamma,
    beta, res and the residual's gamma / beta (_GroupNormApplyFn: the full GroupNorm reverse pass, the terms through `stats` included,
    wherever the table was produced) when one of them requires grad and grad mode is on; the bytes are the no-grad call's.  The row flags
    of want_pos carry no gradient."""
    rs, rg, rb = res_norm if res_norm is not None else (None, None, None)
    if _wants_grad(x, gamma, beta, res, rg, rb):
        out = _GroupNormApplyFn.apply(x, gamma, beta, res, rg, rb, stats, rs, int(groups), seg_len, float(slope), bool(act), bool(want_pos))
        return out if want_pos else out[0]
    return _groupnorm_apply(x, stats, gamma, beta, groups, seg_len, res, res_norm, slope, act, want_pos)


def _groupnorm_apply(x, stats, gamma, beta, groups, seg_len=None, res=None, res_norm=None, slope=0.1, act=True, want_pos=False):
    seg_len = _seg(seg_len, x.shape[0], x.device)
    y = torch.empty_like(x)
    pos = torch.empty((x.shape[0],), dtype=torch.uint8, device=x.device) if want_pos else None
    rs, rg, rb = res_norm if res_norm is not None else (None, None, None)
    _lib.call.lcr_groupnorm_apply(_lib.ptr(x), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(res), _lib.ptr(rs), _lib.ptr(rg),
                                  _lib.ptr(rb), _lib.ptr(y), x.shape[0], x.shape[1], groups, _lib.ptr(seg_len), seg_len.numel(), GN_EPS, float(slope),
                                  int(act), _lib.ptr(pos), _lib.stream_ptr(x.device))
    return (y, pos) if want_pos else y


def row_positive(x):
    pos = torch.empty((x.shape[0],), dtype=torch.uint8, device=x.device)
    _lib.call.lcr_row_positive(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(pos), _lib.stream_ptr(x.device))
    return pos


def _kp_host(kernel_points):
    kp = np.ascontiguousarray(kernel_points, dtype=np.float32)
    assert kp.shape == (15, 3)
    return kp


def kpconv_aggregate(s_feats, s_pos, q_points, s_points, idx, kernel_points_host, sigma, order=None, emit_mask=False):
    """(A [M, 15*C], nn [M]) — the gather/influence/aggregate half of KPConv.forward.  emit_mask: (A, nn, mask) with mask int16 [M], bit k
    set when the kernel-point block A[m, kC:(k+1)C] holds a value other than +-0; the other blocks of A are NOT written (read A only
    through gemm / gemm_bsplit with row_mask=mask)."""
    _lib.require_cuda(s_feats, q_points, s_points, idx)
    M, H = idx.shape
    Ns, C = s_feats.shape
    assert idx.is_contiguous() and s_feats.is_contiguous() and q_points.is_contiguous() and s_points.is_contiguous()
    A = torch.empty((M, 15 * C), dtype=torch.float32, device=s_feats.device)
    nn = torch.empty((M,), dtype=torch.float32, device=s_feats.device)
    kp = _kp_host(kernel_points_host)
    if emit_mask:
        mask = torch.empty((M,), dtype=torch.int16, device=s_feats.device)
        _lib.call.lcr_kpconv_aggregate_mask(
            _lib.ptr(s_feats), _lib.ptr(s_pos), _lib.ptr(q_points), _lib.ptr(s_points), _lib.ptr(idx), _idx_args(idx), M, Ns, H, C,
            ctypes.c_void_p(kp.ctypes.data), float(sigma), _lib.ptr(A), _lib.ptr(nn), _lib.ptr(mask), _lib.ptr(order), 0,
            _lib.stream_ptr(s_feats.device))
        return A, nn, mask
    _lib.call.lcr_kpconv_aggregate(
        _lib.ptr(s_feats), _lib.ptr(s_pos), _lib.ptr(q_points), _lib.ptr(s_points), _lib.ptr(idx), _idx_args(idx), M, Ns, H, C,
        ctypes.c_void_p(kp.ctypes.data), float(sigma), _lib.ptr(A), _lib.ptr(nn), _lib.ptr(order), _lib.stream_ptr(s_feats.device))
    return A, nn


KPCONV_FUSED_C = 32


def kpconv_fused(s_feats, s_pos, q_points, s_points, idx, kernel_points_host, sigma, weights, bias, seg_len=None, groups=0, order=None):
    """Whole rigid KPConv for C_in = C_out = 32 in one launch (lcr_kpconv_fused): the (M, 15*C) aggregate stays in LDS.
    weights: (15, C, C).  Returns (out [M, C], stats) like gemm()."""
    _lib.require_cuda(s_feats, q_points, s_points, idx)
    M, H = idx.shape
    Ns, C = s_feats.shape
    assert C == KPCONV_FUSED_C and tuple(weights.shape) == (15, C, C) and weights.is_contiguous()
    assert idx.is_contiguous() and s_feats.is_contiguous() and q_points.is_contiguous() and s_points.is_contiguous()
    out = torch.empty((M, C), dtype=torch.float32, device=s_feats.device)
    stats, S = None, 0
    if groups:
        seg_len = _seg(seg_len, M, s_feats.device)
        S = seg_len.numel()
        stats = _zero_stats(S, groups, s_feats.device)
    kp = _kp_host(kernel_points_host)
    _lib.call.lcr_kpconv_fused(
        _lib.ptr(s_feats), _lib.ptr(s_pos), _lib.ptr(q_points), _lib.ptr(s_points), _lib.ptr(idx), _idx_args(idx), M, Ns, H, C,
        ctypes.c_void_p(kp.ctypes.data), float(sigma), _lib.ptr(weights), _lib.ptr(bias), _lib.ptr(out),
        _lib.ptr(seg_len) if groups else None, S, int(groups), _lib.ptr(stats), _lib.ptr(order), _lib.stream_ptr(s_feats.device))
    return out, stats


def kpconv_cin1(s_feats, q_points, s_points, idx, kernel_points_host, sigma, weights, bias, order=None):
    """Whole KPConv for one input channel: weights (15,1,Cout) -> out [M,Cout]."""
    M, H = idx.shape
    Ns = s_feats.shape[0]
    Cout = weights.shape[-1]
    out = torch.empty((M, Cout), dtype=torch.float32, device=s_feats.device)
    kp = _kp_host(kernel_points_host)
    _lib.call.lcr_kpconv_cin1(_lib.ptr(s_feats), _lib.ptr(q_points), _lib.ptr(s_points), _lib.ptr(idx), _idx_args(idx), M, Ns, H,
                              ctypes.c_void_p(kp.ctypes.data), float(sigma), _lib.ptr(weights), _lib.ptr(bias), Cout,
                              _lib.ptr(out), _lib.ptr(order), _lib.stream_ptr(s_feats.device))
    return out


def maxpool(x, idx, order=None):
    """Max over the neighbours with a zero shadow row.  Differentiable in x (_MaxPoolFn: the gradient goes to the FIRST real entry of the row
    that holds the maximum, nowhere when the shadow row owns it) when x requires grad and grad mode is on."""
    if _wants_grad(x):
        return _MaxPoolFn.apply(x, idx, order)
    return _maxpool(x, idx, order)


def _maxpool(x, idx, order=None):
    M, H = idx.shape
    out = torch.empty((M, x.shape[1]), dtype=torch.float32, device=x.device)
    _lib.call.lcr_maxpool(_lib.ptr(x), _lib.ptr(idx), _idx_args(idx), M, x.shape[0], H, x.shape[1], _lib.ptr(out),
                          _lib.ptr(order), _lib.stream_ptr(x.device))
    return out


# ---- reverse passes of the encoder (csrc/kpconv_grad.hip, csrc/groupnorm_grad.hip) -------------------------------------------------------
class InvertedList:
    """The inverted form of a neighbour list idx [M,H] over Ns supports, built on first use (lcr_neighbor_transpose) and then kept: every
    block of a pass that gathers over the same list shares one object (inverted())."""

    def __init__(self, idx, Ns):
        self.idx, self.Ns, self._built = idx, int(Ns), None

    def get(self):
        if self._built is None:
            self._built = neighbor_transpose(self.idx, self.Ns)
        return self._built


class _InvertedCache(threading.local):
    lists = None


_INVERTED = _InvertedCache()


class inverted_lists:
    """Context manager: inside, inverted() hands out ONE InvertedList per index tensor (keyed on its storage, shape and support count), so
    the seven lists of an encoder pass are inverted once per pass, not once per block.  Per host thread; nests by replacement.  The objects
    outlive the context in the graph that refers to them."""

    def __enter__(self):
        self.prev = _INVERTED.lists
        _INVERTED.lists = {}
        return self

    def __exit__(self, *exc):
        _INVERTED.lists = self.prev
        return False


def inverted(idx, Ns):
    cache = _INVERTED.lists
    if cache is None:
        return InvertedList(idx, Ns)
    key = (idx.data_ptr(), tuple(idx.shape), idx.dtype, int(Ns))
    inv = cache.get(key)
    if inv is None:
        inv = cache[key] = InvertedList(idx, Ns)        # holds idx: the address cannot be reused while the cache lives
    return inv


def neighbor_transpose(idx, Ns):
    """(row_start int32 [Ns + 1], edges int32 [M * H]) of lcr_neighbor_transpose: the edges of support n, edges[row_start[n]:row_start[n + 1]],
    are the flat positions m * H + h with idx[m, h] == n, ascending; padding (an index outside [0, Ns)) appears nowhere, and the entries of
    `edges` from row_start[Ns] on are unspecified.  No host synchronisation."""
    _lib.require_cuda(idx)
    assert idx.dim() == 2 and idx.is_contiguous()
    M, H = idx.shape
    row_start = torch.empty((int(Ns) + 1,), dtype=torch.int32, device=idx.device)
    edges = torch.empty((max(M * H, 1),), dtype=torch.int32, device=idx.device)
    ws = _lib.ws("lcr_neighbor_transpose_ws_bytes", M, H, device=idx.device)
    _lib.call.lcr_neighbor_transpose(_lib.ptr(idx), _idx_args(idx), M, int(Ns), H, _lib.ptr(row_start), _lib.ptr(edges), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr(idx.device))
    return row_start, edges


def _inv_args(inv, M, H, Ns):
    row_start, edges = inv.get() if isinstance(inv, InvertedList) else inv
    _lib.require_cuda(row_start, edges)
    assert row_start.dtype == torch.int32 and edges.dtype == torch.int32 and row_start.is_contiguous() and edges.is_contiguous()
    assert row_start.numel() == Ns + 1 and edges.numel() >= M * H, "the inverted list belongs to another index list"
    return row_start, edges


def kpconv_aggregate_grad(dA, q_points, s_points, inv, H, kernel_points_host, sigma):
    """d_s_feats [Ns, C] of lcr_kpconv_aggregate_grad from dA [M, 15 C]; inv: the InvertedList (or (row_start, edges)) of the forward's
    index list [M, H]."""
    _lib.require_cuda(dA, q_points, s_points)
    M, Ns = q_points.shape[0], s_points.shape[0]
    C = dA.shape[1] // 15
    assert dA.dtype == torch.float32 and dA.is_contiguous() and tuple(dA.shape) == (M, 15 * C)
    assert q_points.is_contiguous() and s_points.is_contiguous() and q_points.dtype == torch.float32 and s_points.dtype == torch.float32
    row_start, edges = _inv_args(inv, M, H, Ns)
    out = torch.empty((Ns, C), dtype=torch.float32, device=dA.device)
    kp = _kp_host(kernel_points_host)
    _lib.call.lcr_kpconv_aggregate_grad(_lib.ptr(dA), _lib.ptr(q_points), _lib.ptr(s_points), _lib.ptr(row_start), _lib.ptr(edges), M, Ns, int(H), C,
                                        ctypes.c_void_p(kp.ctypes.data), float(sigma), _lib.ptr(out), _lib.stream_ptr(dA.device))
    return out


def kpconv_points_grad(dA, s_feats, q_points, s_points, idx, kernel_points_host, sigma, inv=None, want_q=True, want_s=True):
    """(d_q_points [M, 3] or None, d_s_points [Ns, 3] or None) of lcr_kpconv_points_grad from dA [M, 15 C]: the gradient of the KPConv aggregate
    through its influence weights.  A zero-length edge contributes nothing.  want_s needs the inverted list of idx."""
    _lib.require_cuda(dA, s_feats, q_points, s_points, idx)
    M, H = idx.shape
    Ns, C = s_feats.shape
    assert dA.dtype == torch.float32 and dA.is_contiguous() and tuple(dA.shape) == (M, 15 * C)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (s_feats, q_points, s_points)) and idx.is_contiguous()
    assert tuple(q_points.shape) == (M, 3) and tuple(s_points.shape) == (Ns, 3)
    row_start, edges = _inv_args(inv, M, H, Ns) if want_s else (None, None)
    dq = torch.empty((M, 3), dtype=torch.float32, device=dA.device) if want_q else None
    ds = torch.empty((Ns, 3), dtype=torch.float32, device=dA.device) if want_s else None
    ws = _lib.ws("lcr_kpconv_points_grad_ws_bytes", M, H, device=dA.device) if want_s else None
    kp = _kp_host(kernel_points_host)
    _lib.call.lcr_kpconv_points_grad(_lib.ptr(dA), _lib.ptr(s_feats), _lib.ptr(q_points), _lib.ptr(s_points), _lib.ptr(idx), _idx_args(idx),
                                     _lib.ptr(row_start), _lib.ptr(edges), M, Ns, H, C, ctypes.c_void_p(kp.ctypes.data), float(sigma), _lib.ptr(dq),
                                     _lib.ptr(ds), _lib.ptr(ws), ws.numel() if want_s else 0, _lib.stream_ptr(dA.device))
    return dq, ds


def kpconv_cin1_grad(d_out, s_feats, q_points, s_points, idx, kernel_points_host, sigma, weights, inv=None, want_feats=False, nn=None):
    """(dW [15, 1, Cout], dbias [Cout], d_s_feats [Ns] or None) of lcr_kpconv_cin1_grad.  want_feats needs the inverted list."""
    _lib.require_cuda(d_out, s_feats, q_points, s_points, idx, weights)
    M, H = idx.shape
    Ns, Cout = s_feats.shape[0], weights.shape[-1]
    assert d_out.dtype == torch.float32 and d_out.is_contiguous() and tuple(d_out.shape) == (M, Cout)
    assert idx.is_contiguous() and s_feats.is_contiguous() and q_points.is_contiguous() and s_points.is_contiguous() and weights.is_contiguous()
    assert s_feats.numel() == Ns and weights.numel() == 15 * Cout
    row_start, edges = _inv_args(inv, M, H, Ns) if want_feats else (None, None)
    dW = torch.empty((15, 1, Cout), dtype=torch.float32, device=d_out.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=d_out.device)
    df = torch.empty((Ns,), dtype=torch.float32, device=d_out.device) if want_feats else None
    ws = _lib.ws("lcr_kpconv_cin1_grad_ws_bytes", M, Cout, int(bool(want_feats)), device=d_out.device)
    kp = _kp_host(kernel_points_host)
    _lib.call.lcr_kpconv_cin1_grad(_lib.ptr(d_out), _lib.ptr(s_feats), _lib.ptr(q_points), _lib.ptr(s_points), _lib.ptr(idx), _idx_args(idx), _lib.ptr(nn),
                                   _lib.ptr(row_start), _lib.ptr(edges), M, Ns, H, ctypes.c_void_p(kp.ctypes.data), float(sigma), _lib.ptr(weights), Cout,
                                   _lib.ptr(dW), _lib.ptr(db), _lib.ptr(df), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(d_out.device))
    return dW, db, df


def maxpool_grad(d_out, x, pooled, idx, inv):
    """d_x [Ns, C] of lcr_maxpool_grad; pooled = maxpool(x, idx)."""
    _lib.require_cuda(d_out, x, pooled, idx)
    M, H = idx.shape
    Ns, C = x.shape
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (d_out, x, pooled)) and idx.is_contiguous()
    assert tuple(d_out.shape) == (M, C) and tuple(pooled.shape) == (M, C)
    row_start, edges = _inv_args(inv, M, H, Ns)
    winners = torch.empty((max(M * C, 1),), dtype=torch.uint8, device=x.device)
    dx = torch.empty((Ns, C), dtype=torch.float32, device=x.device)
    _lib.call.lcr_maxpool_grad(_lib.ptr(d_out), _lib.ptr(x), _lib.ptr(pooled), _lib.ptr(idx), _idx_args(idx), _lib.ptr(row_start), _lib.ptr(edges), M, Ns, H,
                               C, _lib.ptr(winners), _lib.ptr(dx), _lib.stream_ptr(x.device))
    return dx


def groupnorm_apply_grad(x, stats, gamma, y, dy, groups, seg_len=None, slope=0.1, act=True, want_dz=False):
    """(dx, dgamma, dbeta, dz or None) of lcr_groupnorm_apply_grad: x the raw input of groupnorm_apply, stats its table, y its output (the
    LeakyReLU mask; None with act=False), dy the gradient of y.  dz is the gradient of a plain residual."""
    _lib.require_cuda(x, stats, gamma, y, dy)
    N, C = x.shape
    assert all(t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (N, C)) for t in (x, y, dy))
    assert stats.dtype == torch.float64 and stats.is_contiguous() and gamma.is_contiguous() and gamma.numel() == C and (y is not None or not act)
    seg_len = _seg(seg_len, N, x.device)
    S = seg_len.numel()
    assert stats.numel() == GN_REPLICAS * S * groups * 2
    dx = torch.empty_like(x)
    dgamma = torch.empty((C,), dtype=torch.float32, device=x.device)
    dbeta = torch.empty((C,), dtype=torch.float32, device=x.device)
    dz = torch.empty_like(x) if want_dz else None
    ws = _lib.ws("lcr_groupnorm_apply_grad_ws_bytes", N, C, int(groups), S, device=x.device)
    _lib.call.lcr_groupnorm_apply_grad(_lib.ptr(x), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(y), _lib.ptr(dy), N, C, int(groups), _lib.ptr(seg_len), S, GN_EPS,
                                       float(slope), int(bool(act)), _lib.ptr(dx), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dz), _lib.ptr(ws), ws.numel(),
                                       _lib.stream_ptr(x.device))
    return dx, dgamma, dbeta, dz


def _det(t):
    return None if t is None else t.detach().contiguous()


class _GroupNormApplyFn(torch.autograd.Function):
    """groupnorm_apply with the full GroupNorm reverse pass (lcr_groupnorm_apply_grad).  The statistics tables are inputs without a gradient of
    their own: they are functions of x (of res), and the backward carries their terms."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, rgamma, rbeta, stats, rstats, groups, seg_len, slope, act, want_pos):
        x, gamma, beta, res, rgamma, rbeta = (_det(t) for t in (x, gamma, beta, res, rgamma, rbeta))
        res_norm = None if rstats is None else (rstats, rgamma, rbeta)
        out = _groupnorm_apply(x, stats, gamma, beta, groups, seg_len, res, res_norm, slope, act, want_pos)
        y, pos = out if want_pos else (out, None)
        ctx.save_for_backward(x, gamma, y if act else None, res if rstats is not None else None, rgamma, stats, rstats, seg_len)
        ctx.groups, ctx.slope, ctx.act, ctx.has_res = groups, slope, act, res is not None
        if pos is None:
            pos = torch.empty(0, dtype=torch.uint8, device=x.device)
        ctx.mark_non_differentiable(pos)
        return y, pos

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _dpos):
        x, gamma, y, res, rgamma, stats, rstats, seg_len = ctx.saved_tensors
        dy = dy.contiguous().float()
        dx, dgamma, dbeta, dz = groupnorm_apply_grad(x, stats, gamma, y, dy, ctx.groups, seg_len, ctx.slope, ctx.act, want_dz=ctx.has_res)
        dres = drg = drb = None
        if ctx.has_res:
            if rstats is None:
                dres = dz
            else:
                dres, drg, drb, _ = groupnorm_apply_grad(res, rstats, rgamma, None, dz, ctx.groups, seg_len, ctx.slope, False)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dgamma if need[1] else None, dbeta if need[2] else None, dres if need[3] else None,
                drg if need[4] else None, drb if need[5] else None, None, None, None, None, None, None, None)


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, order):
        x = x.detach().contiguous()
        out = _maxpool(x, idx, order)
        ctx.save_for_backward(x, out, idx)
        ctx.inv = inverted(idx, x.shape[0])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        x, out, idx = ctx.saved_tensors
        return maxpool_grad(d_out.contiguous().float(), x, out, idx, ctx.inv), None, None


def linear_stats(x, weight, bias, planes=None, seg_len=None, groups=0):
    """(y, stats) = the Linear with GroupNorm sums fused (gemm / gemm_bsplit with `planes`, a callable that returns split_bf16x3(weight)), with
    a graph when x, weight or bias requires grad: dx = dy W and dW = dy^T x on the same GEMMs as _LinearFn (the row-chunked _weight_grad
    included), db the column sum.  stats carries no gradient: groupnorm_apply's backward holds the terms through it."""
    if _wants_grad(x, weight, bias):
        return _LinearStatsFn.apply(x, weight, bias, planes, seg_len, int(groups))
    return _linear_stats(x.contiguous(), weight, bias, planes, seg_len, groups)


def _linear_stats(x, weight, bias, planes, seg_len, groups):
    if planes is not None:
        return gemm_bsplit(x, planes(), bias=bias, seg_len=seg_len, groups=groups)
    return gemm(x, weight, trans_b=True, bias=bias, seg_len=seg_len, groups=groups)


class _LinearStatsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, planes, seg_len, groups):
        xc, w = x.detach().contiguous(), weight.detach().contiguous()
        y, stats = _linear_stats(xc, w, _det(bias), planes, seg_len, groups)
        ctx.save_for_backward(xc, w)
        if stats is None:
            stats = torch.empty(0, dtype=torch.float64, device=y.device)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy, _dstats):
        x, w = ctx.saved_tensors
        dy = dy.contiguous().float()
        dx = gemm(dy, w)[0] if ctx.needs_input_grad[0] else None
        dw = _weight_grad(dy, x) if ctx.needs_input_grad[1] else None
        db = dy.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None, None


class _KPConvFn(torch.autograd.Function):
    """KPConv.forward_raw with a backward.  Forward: the module's own no-grad path (masked aggregate, split-bf16 contraction; C_in = 1: the fused
    kernel).  Backward, with dOut' = dOut / nn: dbias = the column sum of dOut, A recomputed by the unmasked kpconv_aggregate (15 x the
    activation: never kept), dW = dOut'^T A on _weight_grad, dA = dOut' W^T on the GEMM, d_s_feats = lcr_kpconv_aggregate_grad over the inverted
    list.  The neighbour count is an integer and carries no gradient (as in the reference's autograd); kernel points get none.  q_points /
    s_points, when they require grad (the vote encoder's node centres), get lcr_kpconv_points_grad from the same dA — one tensor passed as both
    receives the sum of the two from autograd.  A zero-length edge sends nothing; C_in = 1 has no such form and refuses."""

    @staticmethod
    def forward(ctx, s_feats, weights, bias, module, q_points, s_points, idx, s_pos, seg_len, groups, order):
        need = ctx.needs_input_grad
        if module.in_channels == 1 and (need[4] or need[5]):
            raise NotImplementedError("KPConv with in_channels == 1 has no gradient to the points (no model of this package needs one)")
        s_feats, q_points, s_points = s_feats.detach().contiguous(), q_points.detach().contiguous(), s_points.detach().contiguous()
        if module.in_channels != 1 and s_pos is None:
            s_pos = row_positive(s_feats)
        out, stats, nn = module.run_raw(s_feats, q_points, s_points, idx, s_pos, seg_len, groups, order, want_nn=True)
        ctx.save_for_backward(s_feats, q_points, s_points, idx, s_pos, nn)
        ctx.module, ctx.order = module, order
        ctx.inv = inverted(idx, s_feats.shape[0]) if ((need[0] or need[5]) and module.in_channels != 1) else None
        if stats is None:
            stats = torch.empty(0, dtype=torch.float64, device=out.device)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, _dstats):
        s_feats, q_points, s_points, idx, s_pos, nn = ctx.saved_tensors
        mod, need = ctx.module, ctx.needs_input_grad
        d_out = d_out.contiguous().float()
        kp = mod.kernel_points_host()
        if mod.in_channels == 1:
            want = need[0]
            inv = inverted(idx, s_feats.shape[0]) if want else None
            dW, db, df = kpconv_cin1_grad(d_out, s_feats.view(-1), q_points, s_points, idx, kp, mod.sigma, mod.weights.detach(), inv, want_feats=want)
            return (df.view(-1, 1) if want else None, dW if need[1] else None, db if need[2] else None) + (None,) * 8
        db = d_out.sum(0) if need[2] else None
        g = d_out / nn[:, None]
        dW = df = None
        if need[1]:
            A, _ = kpconv_aggregate(s_feats, s_pos, q_points, s_points, idx, kp, mod.sigma, order=ctx.order)
            dW = _weight_grad(g, A).t().reshape(mod.kernel_size, mod.in_channels, mod.out_channels)
            del A
        dq = ds = None
        if need[0] or need[4] or need[5]:
            dA = gemm(g, mod.weights_t())[0]
            if need[0]:
                df = kpconv_aggregate_grad(dA, q_points, s_points, ctx.inv, idx.shape[1], kp, mod.sigma)
            if need[4] or need[5]:
                dq, ds = kpconv_points_grad(dA, s_feats, q_points, s_points, idx, kp, mod.sigma, ctx.inv, want_q=need[4], want_s=need[5])
        return (df, dW, db, None, dq, ds) + (None,) * 5


class NetvladWeights(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "cluster_weights", "cluster_weights2", "hidden1_weights", "bn1_w", "bn1_b", "bn1_mean", "bn1_var",
        "bn2_w", "bn2_b", "bn2_mean", "bn2_var", "gating_weights", "gbn_w", "gbn_b", "gbn_mean", "gbn_var")]


def _netvlad_seg(feats, seg_len_host):
    _lib.require_cuda(feats)
    seg = np.ascontiguousarray(seg_len_host, dtype=np.int64)
    assert seg.ndim == 1 and feats.dim() == 2 and feats.shape[1] == 1024 and feats.dtype == torch.float32 and feats.is_contiguous()
    assert int(seg.sum()) == feats.shape[0], "seg_len does not add up to the rows of feats"
    return seg, int(seg.shape[0])


def netvlad_forward(feats, seg_len_host, weights_struct):
    """feats [sum(seg_len),1024] stacked coarse features -> [S,256] unit-norm descriptors."""
    seg, S = _netvlad_seg(feats, seg_len_host)
    ws = _lib.ws("lcr_netvlad_ws_bytes", feats.shape[0], S, device=feats.device)
    out = torch.empty((S, 256), dtype=torch.float32, device=feats.device)
    _lib.call.lcr_netvlad_forward(_lib.ptr(feats), ctypes.c_void_p(seg.ctypes.data), S, ctypes.byref(weights_struct),
                                  _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(feats.device))
    return out


NETVLAD_GRAD_NAMES = ("cluster_weights", "cluster_weights2", "hidden1_weights", "bn1_w", "bn1_b", "bn2_w", "bn2_b", "gating_weights", "gbn_w", "gbn_b")
_NETVLAD_GRAD_SHAPES = {"cluster_weights": (1024, 64), "cluster_weights2": (1, 1024, 64), "hidden1_weights": (65536, 256), "bn1_w": (64,), "bn1_b": (64,),
                        "bn2_w": (256,), "bn2_b": (256,), "gating_weights": (256, 256), "gbn_w": (256,), "gbn_b": (256,)}
NETVLAD_STAT_FLOATS = 2 * 64 + 4 * 256


class NetvladGrads(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in NETVLAD_GRAD_NAMES]


def netvlad_train(feats, seg_len_host, weights_struct):
    """The head in training mode (lcr_netvlad_train_forward: cyclic padding by multiplicities, batch statistics, uniform assignment on the
    padding rows): feats [sum(seg_len),1024] -> (out [S,256], batch_stats [1152] = mean and biased variance of bn1, bn2 and
    context_gating.bn1, saved = the opaque buffer netvlad_backward reads).  No host synchronisation.  One cloud has no batch statistics:
    ValueError, as nn.BatchNorm1d raises for one value per channel."""
    seg, S = _netvlad_seg(feats, seg_len_host)
    if S == 1:
        raise ValueError("Expected more than 1 value per channel when training, got one cloud (batch statistics of bn2)")
    dev = feats.device
    out = torch.empty((S, 256), dtype=torch.float32, device=dev)
    stats = torch.empty((NETVLAD_STAT_FLOATS,), dtype=torch.float32, device=dev)
    saved = _lib.ws("lcr_netvlad_train_saved_bytes", feats.shape[0], S, device=dev)
    ws = _lib.ws("lcr_netvlad_train_ws_bytes", feats.shape[0], S, device=dev)
    _lib.call.lcr_netvlad_train_forward(_lib.ptr(feats), ctypes.c_void_p(seg.ctypes.data), S, ctypes.byref(weights_struct), _lib.ptr(out), _lib.ptr(stats),
                                        _lib.ptr(saved), saved.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return out, stats, saved


def netvlad_backward(d_out, feats, seg_len_host, weights_struct, saved, want=NETVLAD_GRAD_NAMES, want_feats=True):
    """lcr_netvlad_backward: d_out [S,256] -> (d_feats [N,1024] or None, {name: gradient} for the names of `want`).  feats, seg_len_host, the
    weights and `saved` are those of the netvlad_train call.  No host synchronisation."""
    seg, S = _netvlad_seg(feats, seg_len_host)
    _lib.require_cuda(d_out, saved)
    assert d_out.dtype == torch.float32 and d_out.is_contiguous() and tuple(d_out.shape) == (S, 256)
    dev = feats.device
    grads = {n: torch.empty(_NETVLAD_GRAD_SHAPES[n], dtype=torch.float32, device=dev) for n in want}
    table = NetvladGrads()
    for n, t in grads.items():
        setattr(table, n, t.data_ptr())
    d_feats = torch.empty_like(feats) if want_feats else None
    ws = _lib.ws("lcr_netvlad_backward_ws_bytes", feats.shape[0], S, device=dev)
    _lib.call.lcr_netvlad_backward(_lib.ptr(d_out), _lib.ptr(feats), ctypes.c_void_p(seg.ctypes.data), S, ctypes.byref(weights_struct), _lib.ptr(saved),
                                   saved.numel(), _lib.ptr(d_feats), ctypes.byref(table), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return d_feats, grads


class _NetvladTrainFn(torch.autograd.Function):
    """netvlad_train with lcr_netvlad_backward behind it.  `module` is the NetVLADLoupe2 (its _weights() gives the pointer table); the ten
    parameters follow in NETVLAD_GRAD_NAMES order so that autograd routes their gradients.  Returns (out, batch_stats)."""

    @staticmethod
    def forward(ctx, feats, module, seg, *params):
        x = feats.detach().contiguous()
        out, stats, saved = netvlad_train(x, seg, module._weights())
        ctx.save_for_backward(x, saved)
        ctx.module, ctx.seg = module, seg
        ctx.versions = [p._version for p in params]
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, _dstats):
        x, saved = ctx.saved_tensors
        if [p._version for p in ctx.module._grad_params()] != ctx.versions:
            raise RuntimeError("a NetVLAD parameter was modified in place between the training forward and its backward")
        want = [n for i, n in enumerate(NETVLAD_GRAD_NAMES) if ctx.needs_input_grad[3 + i]]
        d_feats, grads = netvlad_backward(d_out.contiguous().float(), x, ctx.seg, ctx.module._weights(), saved, want, ctx.needs_input_grad[0])
        return (d_feats, None, None) + tuple(grads.get(n) for n in NETVLAD_GRAD_NAMES)


def gemm_batched_ta(a, b, c, M, N, k, a_off, b_off, c_off):
    """c[c_off[z] : c_off[z] + M*N] <- A_z^T · B_z for every entry z, in place, where A_z = a[a_off[z]:] read as [k[z], M] and
    B_z = b[b_off[z]:] as [k[z], N] (lcr_gemm_f32_batched_ta: a, b, c flat fp32 device buffers; k and the ELEMENT offsets are host sequences,
    at most 64 entries; offsets into a and b and M, N are multiples of 4).  The entry point's own refusals surface as RuntimeError."""
    _lib.require_cuda(a, b, c)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (a, b, c))
    kk = np.ascontiguousarray(k, dtype=np.int32)
    ao, bo, co = (np.ascontiguousarray(v, dtype=np.int64) for v in (a_off, b_off, c_off))
    count = int(kk.shape[0])
    assert ao.shape == bo.shape == co.shape == (count,)
    for i in range(count):                                  # nothing outside the three buffers is addressed, whatever the entry point accepts
        assert 0 <= ao[i] and ao[i] + max(int(kk[i]), 0) * M <= a.numel(), "A entry out of range"
        assert 0 <= bo[i] and bo[i] + max(int(kk[i]), 0) * N <= b.numel(), "B entry out of range"
        assert 0 <= co[i] and co[i] + M * N <= c.numel(), "C entry out of range"
    _lib.call.lcr_gemm_f32_batched_ta(_lib.ptr(a), _lib.ptr(b), _lib.ptr(c), int(M), int(N), count, ctypes.c_void_p(kk.ctypes.data),
                                      ctypes.c_void_p(ao.ctypes.data), ctypes.c_void_p(bo.ctypes.data),
                                      ctypes.c_void_p(co.ctypes.data), _lib.stream_ptr(a.device))
    return c


def linear(x, weight, bias=None, relu=False):
    """nn.Linear (weight [out,in]) on the MFMA GEMM, optional ReLU.  Differentiable in x, weight and bias (_LinearFn) when one of them
    requires grad and grad mode is on; the bytes are the no-grad call's."""
    if _wants_grad(x, weight, bias):
        return _LinearFn.apply(x, weight, bias, bool(relu))
    y = gemm(x.contiguous(), weight, trans_b=True, bias=bias)[0]
    if relu:
        _lib.call.lcr_relu_inplace(_lib.ptr(y), y.numel(), _lib.stream_ptr(y.device))
    return y


WEIGHT_GRAD_SPLIT_ROWS = 512      # from this many rows on dW = dy^T·x is summed over row chunks (one batched launch)


def _weight_grad(dy, x):
    """dW [out,in] = dy^T·x over the rows.  The output is a handful of 64 x 64 tiles however many rows there are, so one lcr_gemm_f32 call
    walks all rows in 2 - 32 workgroups, adding them one after the other in fp32: slow at the rows of 16 pairs per call, and at 1023 rows
    already 4.4 x the error of torch's blocked fp32 sum (tests/test_attention_grad_gpu.py).  From WEIGHT_GRAD_SPLIT_ROWS rows on the rows
    are cut into equal chunks of at most 256 rows (at most 64 chunks, so longer ones beyond 16 384 rows) whose products are ONE
    lcr_gemm_f32_batched_ta launch, added in chunk order.  The chunking depends on the shape alone: results repeat to the bit.  That entry
    wants out and in to be multiples of 4: x is padded with zero columns (the position embedding's in = 3); another `out` takes the plain
    call."""
    rows, M, N = dy.shape[0], dy.shape[1], x.shape[1]
    if rows < WEIGHT_GRAD_SPLIT_ROWS or M % 4:
        return gemm(dy, x, trans_a=True)[0]
    if N % 4:
        return _weight_grad(dy, torch.nn.functional.pad(x, (0, 4 - N % 4)))[:, :N].contiguous()
    count = min(64, (rows + 255) // 256)
    per = (rows + count - 1) // count
    count = (rows + per - 1) // per
    ks = [min(per, rows - z * per) for z in range(count)]
    c = torch.empty((count, M, N), dtype=torch.float32, device=dy.device)
    gemm_batched_ta(dy, x, c, M, N, ks, [z * per * M for z in range(count)], [z * per * N for z in range(count)], [z * M * N for z in range(count)])
    return c.sum(0)


class _LinearFn(torch.autograd.Function):
    """linear() with a backward on the same GEMM: dx = dy·W, dW = dy^T·x (lcr_gemm_f32 with trans_a), db = the column sum of dy; the ReLU
    mask is read off the saved output."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        xc, w = x.detach().contiguous(), weight.detach().contiguous()
        y = gemm(xc, w, trans_b=True, bias=None if bias is None else bias.detach())[0]
        if relu:
            _lib.call.lcr_relu_inplace(_lib.ptr(y), y.numel(), _lib.stream_ptr(y.device))
        ctx.save_for_backward(xc, w, y if relu else None)
        ctx.relu = relu
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous().float()
        if ctx.relu:
            dy = dy * (y > 0)
        dx = gemm(dy, w)[0] if ctx.needs_input_grad[0] else None
        dw = _weight_grad(dy, x) if ctx.needs_input_grad[1] else None
        db = dy.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


def relu_(x):
    _lib.call.lcr_relu_inplace(_lib.ptr(x), x.numel(), _lib.stream_ptr(x.device))
    return x


def rotary_embed_(x, theta, heads):
    """In place rotary position embedding (rpetransformer.py:41-54): x [N, heads*32], theta [N, heads*16]."""
    assert x.is_contiguous() and theta.is_contiguous() and x.shape[1] == heads * 32 and theta.shape[1] == heads * 16
    _lib.call.lcr_rotary_embed(_lib.ptr(x), _lib.ptr(theta), x.shape[0], heads, _lib.stream_ptr(x.device))
    return x


def rotary_embed(x, theta, heads):
    """Out-of-place rotary position embedding, differentiable in x and theta (lcr_rotary_embed on a copy; backward lcr_rotary_embed_grad from
    the rotated tensor).  The bytes are rotary_embed_'s."""
    if _wants_grad(x, theta):
        return _RotaryFn.apply(x, theta, int(heads))
    return rotary_embed_(x.detach().clone(memory_format=torch.contiguous_format), theta.contiguous(), heads)


class _RotaryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, theta, heads):
        _lib.require_cuda(x, theta)
        th = theta.detach().contiguous()
        y = rotary_embed_(x.detach().clone(memory_format=torch.contiguous_format), th, heads)
        ctx.save_for_backward(y, th)
        ctx.heads = heads
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y, th = ctx.saved_tensors
        dy = dy.contiguous().float()
        dx, dth = torch.empty_like(y), torch.empty_like(th)
        _lib.call.lcr_rotary_embed_grad(_lib.ptr(y), _lib.ptr(dy), _lib.ptr(th), y.shape[0], ctx.heads, _lib.ptr(dx), _lib.ptr(dth),
                                        _lib.stream_ptr(y.device))
        return (dx if ctx.needs_input_grad[0] else None), (dth if ctx.needs_input_grad[1] else None), None


def _attention_forward(q, k, v, heads, q_lens, k_lens):
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    out = torch.empty_like(q)
    if q_lens is not None:
        P = len(q_lens)
        assert len(k_lens) == P and sum(q_lens) == q.shape[0] and sum(k_lens) == k.shape[0]
        ql, kl = (ctypes.c_int64 * P)(*[int(x) for x in q_lens]), (ctypes.c_int64 * P)(*[int(x) for x in k_lens])
        _lib.call.lcr_attention_seg_f32(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ctypes.cast(ql, ctypes.c_void_p), ctypes.cast(kl, ctypes.c_void_p), P,
                                        heads, q.shape[1] // heads, _lib.ptr(out), _lib.stream_ptr(q.device))
        return out
    _lib.call.lcr_attention_f32(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), q.shape[0], k.shape[0], heads, q.shape[1] // heads,
                                _lib.ptr(out), _lib.stream_ptr(q.device))
    return out


def attention(q, k, v, heads, q_lens=None, k_lens=None):
    """Fused softmax(q k^T / sqrt(d)) v per head; q [Nq, heads*32], k/v [Nk, heads*32].  With q_lens / k_lens (host sequences of
    equal length P <= 64, summing to Nq / Nk): P independent problems over the stacked rows in one launch.  Differentiable in q, k and v
    (_AttentionFn over lcr_attention_seg_grad_f32) when one of them requires grad and grad mode is on; the bytes are the no-grad call's."""
    if _wants_grad(q, k, v):
        return _AttentionFn.apply(q, k, v, int(heads), None if q_lens is None else tuple(int(x) for x in q_lens),
                                  None if k_lens is None else tuple(int(x) for x in k_lens))
    return _attention_forward(q, k, v, heads, q_lens, k_lens)


def attention_grad(q, k, v, out, d_out, heads, q_lens=None, k_lens=None):
    """(dq, dk, dv) of lcr_attention_seg_grad_f32 for the problems of `attention`: q, k, v as the forward consumed them, out its result,
    d_out = dL/d(out).  No host synchronisation."""
    _lib.require_cuda(q, k, v, out, d_out)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (q, k, v, out, d_out)) and out.shape == q.shape and d_out.shape == q.shape
    ql = [q.shape[0]] if q_lens is None else [int(x) for x in q_lens]
    kl = [k.shape[0]] if k_lens is None else [int(x) for x in k_lens]
    P = len(ql)
    assert len(kl) == P and sum(ql) == q.shape[0] and sum(kl) == k.shape[0] and k.shape == v.shape
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ws = _lib.ws("lcr_attention_grad_ws_bytes", q.shape[0], int(heads), device=q.device)
    qa, ka = (ctypes.c_int64 * P)(*ql), (ctypes.c_int64 * P)(*kl)
    _lib.call.lcr_attention_seg_grad_f32(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), _lib.ptr(d_out), ctypes.cast(qa, ctypes.c_void_p),
                                         ctypes.cast(ka, ctypes.c_void_p), P, int(heads), q.shape[1] // int(heads), _lib.ptr(dq), _lib.ptr(dk),
                                         _lib.ptr(dv), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(q.device))
    return dq, dk, dv


class _AttentionFn(torch.autograd.Function):
    """attention() with a backward: keeps q, k, v, the output and the lens; the backward is lcr_attention_seg_grad_f32, which recomputes the
    softmax row statistic itself (the forward entry and its bytes are unchanged)."""

    @staticmethod
    def forward(ctx, q, k, v, heads, q_lens, k_lens):
        _lib.require_cuda(q, k, v)
        qc, kc, vc = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
        out = _attention_forward(qc, kc, vc, heads, q_lens, k_lens)
        ctx.save_for_backward(qc, kc, vc, out)
        ctx.heads, ctx.q_lens, ctx.k_lens = heads, q_lens, k_lens
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        q, k, v, out = ctx.saved_tensors
        dq, dk, dv = attention_grad(q, k, v, out, d_out.contiguous().float(), ctx.heads, ctx.q_lens, ctx.k_lens)
        need = ctx.needs_input_grad
        return (dq if need[0] else None), (dk if need[1] else None), (dv if need[2] else None), None, None, None


ATTENTION_TOPK_MAX_KEYS = 4096     # ATK_MAXK of csrc/attention.hip: one row of scores per (query, head) in LDS


def attention_topk(q, k, v, heads, q_lens, k_lens, kks):
    """dynamic_attention with k != None (rpetransformer.py:19-39): per problem p (rows stacked like `attention`), query and head, only the
    kks[p] largest scores are soft-maxed.  kks[p] = int(n_queries_p * fraction) is computed by the caller as the reference does."""
    if _wants_grad(q, k, v):
        raise NotImplementedError("top-k attention (cfg.GAT.k) has no backward: train with cfg.GAT.k = None (the shipped configuration), "
                                  "the dense form")
    assert q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
    P = len(q_lens)
    assert len(k_lens) == P and len(kks) == P and sum(q_lens) == q.shape[0] and sum(k_lens) == k.shape[0]
    out = torch.empty_like(q)
    ql, kl = (ctypes.c_int64 * P)(*[int(x) for x in q_lens]), (ctypes.c_int64 * P)(*[int(x) for x in k_lens])
    kk = (ctypes.c_int * P)(*[int(x) for x in kks])
    _lib.call.lcr_attention_topk_f32(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ctypes.cast(ql, ctypes.c_void_p), ctypes.cast(kl, ctypes.c_void_p),
                                     ctypes.cast(kk, ctypes.c_void_p), P, heads, q.shape[1] // heads, _lib.ptr(out), _lib.stream_ptr(q.device))
    return out


def add_layernorm(a, b, gamma, beta, eps=1e-5):
    """y = LayerNorm(a + b) (b may be None).  Differentiable in a, b, gamma and beta (_AddLayerNormFn over lcr_add_layernorm_grad) when one of
    them requires grad and grad mode is on; the bytes are the no-grad call's."""
    if _wants_grad(a, b, gamma, beta):
        return _AddLayerNormFn.apply(a, b, gamma, beta, float(eps))
    y = torch.empty_like(a)
    _lib.call.lcr_add_layernorm(_lib.ptr(a), _lib.ptr(b), _lib.ptr(gamma), _lib.ptr(beta), a.shape[0], a.shape[1], float(eps),
                                _lib.ptr(y), _lib.stream_ptr(a.device))
    return y


def add_layernorm_grad(a, b, gamma, dy, eps=1e-5):
    """(d(a + b) [N,D], dgamma [D], dbeta [D]) of lcr_add_layernorm_grad.  No host synchronisation."""
    _lib.require_cuda(a, b, gamma, dy)
    assert all(t is None or (t.dtype == torch.float32 and t.is_contiguous()) for t in (a, b, gamma, dy)) and dy.shape == a.shape
    N, D = a.shape
    dx = torch.empty_like(a)
    dg, db = torch.empty((D,), dtype=torch.float32, device=a.device), torch.empty((D,), dtype=torch.float32, device=a.device)
    ws = _lib.ws("lcr_add_layernorm_grad_ws_bytes", N, D, device=a.device)
    _lib.call.lcr_add_layernorm_grad(_lib.ptr(a), _lib.ptr(b), _lib.ptr(gamma), _lib.ptr(dy), N, D, float(eps), _lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(a.device))
    return dx, dg, db


class _AddLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, gamma, beta, eps):
        _lib.require_cuda(a, b, gamma, beta)
        ac, bc, g, be = a.detach().contiguous(), None if b is None else b.detach().contiguous(), gamma.detach().contiguous(), beta.detach().contiguous()
        y = torch.empty_like(ac)
        _lib.call.lcr_add_layernorm(_lib.ptr(ac), _lib.ptr(bc), _lib.ptr(g), _lib.ptr(be), ac.shape[0], ac.shape[1], eps, _lib.ptr(y),
                                    _lib.stream_ptr(ac.device))
        ctx.save_for_backward(ac, bc, g)
        ctx.eps = eps
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        a, b, g = ctx.saved_tensors
        dx, dg, db = add_layernorm_grad(a, b, g, dy.contiguous().float(), ctx.eps)
        need = ctx.needs_input_grad
        return (dx if need[0] else None), (dx if need[1] and b is not None else None), (dg if need[2] else None), (db if need[3] else None), None


# ------------------------------------------------------------------------------------------------ pose tail (a-10)
_L = _lib.lib     # the raw view under its old name here, for callers outside the package that assert on a return code


def vote_shift(xyz, offsets, max_range):
    """xyz + offsets clipped to max_range; differentiable in both (_VoteShiftFn) when one requires grad and grad mode is on."""
    _lib.require_cuda(xyz, offsets)
    if _wants_grad(xyz, offsets):
        return _VoteShiftFn.apply(xyz, offsets, float(max_range))
    return _vote_shift(xyz, offsets, max_range)


def _vote_shift(xyz, offsets, max_range):
    out = torch.empty_like(xyz)
    _lib.call.lcr_vote_shift(_lib.ptr(xyz.contiguous()), _lib.ptr(offsets.contiguous()), xyz.shape[0], float(max_range), _lib.ptr(out),
                             _lib.stream_ptr(xyz.device))
    return out


def vote_shift_grad(offsets, d_out, max_range):
    """d_offsets [N, 3] of lcr_vote_shift_grad (d_xyz is d_out itself)."""
    _lib.require_cuda(offsets, d_out)
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 3 for t in (offsets, d_out)) and offsets.shape == d_out.shape
    d_off = torch.empty_like(offsets)
    _lib.call.lcr_vote_shift_grad(_lib.ptr(offsets), _lib.ptr(d_out), offsets.shape[0], float(max_range), _lib.ptr(d_off), _lib.stream_ptr(offsets.device))
    return d_off


class _VoteShiftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, offsets, max_range):
        offsets = offsets.detach().contiguous().float()
        ctx.save_for_backward(offsets)
        ctx.max_range = max_range
        return _vote_shift(xyz.detach().contiguous(), offsets, max_range)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        offsets, = ctx.saved_tensors
        d_out = d_out.contiguous().float()
        d_off = vote_shift_grad(offsets, d_out, ctx.max_range) if ctx.needs_input_grad[1] else None
        return (d_out if ctx.needs_input_grad[0] else None), d_off, None


def greedy_nms(points, lengths, radius):
    """(keep mask uint8 [N], kept count per cloud i64 [B]) — modules/vote/vote.py:13-70."""
    n, B = points.shape[0], lengths.numel()
    keep = torch.empty((n,), dtype=torch.uint8, device=points.device)
    out_len = torch.empty((B,), dtype=torch.int64, device=points.device)
    ws = _lib.ws("lcr_greedy_nms_ws_bytes", n, device=points.device)
    _lib.call.lcr_greedy_nms(_lib.ptr(points.contiguous()), _lib.ptr(lengths), B, n, float(radius), _lib.ptr(keep), _lib.ptr(out_len),
                             _lib.ptr(ws), _lib.stream_ptr(points.device))
    return keep, out_len


def neighbor_mean(points, idx, pad):
    """Mean of points[idx[m, h]] over the valid (0 <= idx < pad) entries of every row; differentiable in points (_NeighborMeanFn) when they
    require grad and grad mode is on."""
    _lib.require_cuda(points, idx)
    if _wants_grad(points):
        return _NeighborMeanFn.apply(points, idx, int(pad))
    return _neighbor_mean(points, idx, pad)


def _neighbor_mean(points, idx, pad):
    out = torch.empty((idx.shape[0], 3), dtype=torch.float32, device=points.device)
    _lib.call.lcr_neighbor_mean(_lib.ptr(points.contiguous()), _lib.ptr(idx.contiguous()), _idx_args(idx), idx.shape[0], idx.shape[1], int(pad),
                                _lib.ptr(out), _lib.stream_ptr(points.device))
    return out


def neighbor_mean_grad(d_out, idx, pad, inv):
    """d_points [pad, 3] of lcr_neighbor_mean_grad; inv: the InvertedList (or (row_start, edges)) of idx [M, H] over `pad` points."""
    _lib.require_cuda(d_out, idx)
    M, H = idx.shape
    assert d_out.dtype == torch.float32 and d_out.is_contiguous() and tuple(d_out.shape) == (M, 3) and idx.is_contiguous()
    row_start, edges = _inv_args(inv, M, H, int(pad))
    d_pts = torch.empty((int(pad), 3), dtype=torch.float32, device=d_out.device)
    _lib.call.lcr_neighbor_mean_grad(_lib.ptr(d_out), _lib.ptr(idx), _idx_args(idx), _lib.ptr(row_start), _lib.ptr(edges), M, H, int(pad), _lib.ptr(d_pts),
                                     _lib.stream_ptr(d_out.device))
    return d_pts


class _NeighborMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx, pad):
        idx = idx.contiguous()
        assert pad <= points.shape[0]
        ctx.save_for_backward(idx)
        ctx.pad, ctx.rows = pad, points.shape[0]
        ctx.inv = inverted(idx, pad)
        return _neighbor_mean(points.detach(), idx, pad)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        idx, = ctx.saved_tensors
        d = neighbor_mean_grad(d_out.contiguous().float(), idx, ctx.pad, ctx.inv)
        if ctx.rows != ctx.pad:                               # rows behind `pad` are never read
            d = torch.cat([d, d.new_zeros((ctx.rows - ctx.pad, 3))])
        return d, None, None


def point_to_node_partition(points, nodes, point_limit):
    """(point_to_node i32[N], node_masks bool[M], node_knn_indices i64[M,K], node_knn_masks bool[M,K]) —
    modules/ops/pointcloud_partition.py:60-107."""
    N, M, dev = points.shape[0], nodes.shape[0], points.device
    ws = _lib.ws("lcr_point_to_node_ws_bytes", N, M, device=dev)
    p2n = torch.empty((N,), dtype=torch.int32, device=dev)
    knn = torch.empty((M, point_limit), dtype=torch.int64, device=dev)
    km = torch.empty((M, point_limit), dtype=torch.uint8, device=dev)
    nm = torch.empty((M,), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call.lcr_point_to_node_partition(_lib.ptr(points.contiguous()), N, _lib.ptr(nodes.contiguous()), M, int(point_limit), _lib.ptr(p2n),
                                          _lib.ptr(knn), _lib.ptr(km), _lib.ptr(nm), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points.device))
    return p2n, nm.bool(), knn, km.bool()


def point_to_node_partition_stack(points, point_off, nodes, node_off, point_limit):
    """`point_to_node_partition` of every cloud of a stack in ONE launch sequence: cloud c owns points[point_off[c]:point_off[c+1]] and
    nodes[node_off[c]:node_off[c+1]] (host offset lists).  -> (point_to_node i32[N], node_masks bool[M], node_knn_indices i64[M,K],
    node_knn_masks bool[M,K]) stacked in cloud order; indices are local to their cloud, knn rows padded with the cloud's point count —
    slices of these are exactly what the per-cloud call returns."""
    import numpy as np
    C = len(point_off) - 1
    assert len(node_off) == C + 1 and C >= 1
    dev = points.device
    N, M = int(point_off[-1] - point_off[0]), int(node_off[-1] - node_off[0])
    po = np.ascontiguousarray(point_off, dtype=np.int64)
    mo = np.ascontiguousarray(node_off, dtype=np.int64)
    ws = _lib.ws("lcr_point_to_node_ws_bytes", N, M, device=dev)
    p2n = torch.empty((N,), dtype=torch.int32, device=dev)
    knn = torch.empty((M, point_limit), dtype=torch.int64, device=dev)
    km = torch.empty((M, point_limit), dtype=torch.uint8, device=dev)
    nm = torch.empty((M,), dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call.lcr_point_to_node_partition_stack(_lib.ptr(points.contiguous()), po.ctypes.data, _lib.ptr(nodes.contiguous()), mo.ctypes.data, C,
                                                int(point_limit), _lib.ptr(p2n), _lib.ptr(knn), _lib.ptr(km), _lib.ptr(nm), _lib.ptr(status),
                                                _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points.device))
    return p2n, nm.bool(), knn, km.bool()


class _PendingStatus(threading.local):
    def __init__(self):
        self.items = []


_pending_ot_status = _PendingStatus()
_PENDING_OT_MAX = 32


def check_transport_status():
    """Raise if a persistent optimal-transport launch issued by this thread reported a timed-out hand-off (its result is invalid).
    One host read; called where the caller synchronises anyway (top1_matching reads a count back right after the transport)."""
    items, _pending_ot_status.items = _pending_ot_status.items, []
    if items and any(int(t.reshape(()).item()) != 0 for t in items):       # one entry per device after folding; a handful otherwise
        raise RuntimeError("lcr_log_sinkhorn: a workgroup hand-off of the persistent form timed out (set LCR_SINKHORN_COOP=0)")


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def eval_without_graph(forward):
    """Decorator for the forward of the encoder's modules: in eval mode the forward runs with grad mode off, i.e. it makes the calls and returns
    the plain tensors it always did, whatever requires grad (models are evaluated with `.eval()` and not always under torch.no_grad()).  A
    graph is built in training mode only."""
    import functools

    @functools.wraps(forward)
    def wrapped(self, *args, **kwargs):
        if not self.training and torch.is_grad_enabled():
            with torch.no_grad():
                return forward(self, *args, **kwargs)
        return forward(self, *args, **kwargs)
    return wrapped


def log_optimal_transport(raw_scores, row_masks, col_masks, alpha, scale=1.0, iters=100, inf=1e12):
    """LearnableLogOptimalTransport on raw products [B,M,N] (scaled by `scale`) -> log scores [B,M+1,N+1].  Differentiable in raw_scores and
    alpha: when either requires grad (and grad mode is on) the result carries a graph whose backward is lcr_log_sinkhorn_grad; its bytes
    are the no-grad call's."""
    if _wants_grad(raw_scores, alpha):
        return _TransportFn.apply(raw_scores, alpha, row_masks, col_masks, float(scale), int(iters), float(inf))
    _lib.require_cuda(raw_scores, row_masks, col_masks, alpha)      # as _TransportFn.forward: a host pointer must never reach a launch
    B, M, N = raw_scores.shape
    dev = raw_scores.device
    rm, cm = row_masks.to(torch.uint8).contiguous(), col_masks.to(torch.uint8).contiguous()
    S = torch.empty((B, M + 1, N + 1), dtype=torch.float32, device=dev)
    _lib.call.lcr_build_padded_scores(_lib.ptr(raw_scores.contiguous()), _lib.ptr(rm), _lib.ptr(cm), B, M, N, float(scale),
                                      _lib.ptr(alpha.reshape(1).float()), float(inf), _lib.ptr(S), _lib.stream_ptr(S.device))
    return _transport_padded(S, rm, cm, iters, inf)


def log_sinkhorn_grad(S0, G, rm, cm, iters=100, inf=1e12):
    """(dS [B,M+1,N+1], d_alpha_part [B]) of lcr_log_sinkhorn_grad: S0 the padded scores before the transport, G = dL/d(log scores), rm / cm
    the uint8 masks.  No host synchronisation."""
    _lib.require_cuda(S0, G, rm, cm)
    B, M, N = S0.shape[0], S0.shape[1] - 1, S0.shape[2] - 1
    assert S0.dtype == torch.float32 and S0.is_contiguous() and G.dtype == torch.float32 and G.is_contiguous() and G.shape == S0.shape
    assert rm.dtype == torch.uint8 and cm.dtype == torch.uint8 and rm.is_contiguous() and cm.is_contiguous()
    assert tuple(rm.shape) == (B, M) and tuple(cm.shape) == (B, N)
    dS = torch.empty_like(S0)
    part = torch.empty((B,), dtype=torch.float32, device=S0.device)
    ws = _lib.ws("lcr_log_sinkhorn_grad_ws_bytes", B, M, N, int(iters), device=S0.device)
    _lib.call.lcr_log_sinkhorn_grad(_lib.ptr(S0), _lib.ptr(G), _lib.ptr(rm), _lib.ptr(cm), B, M, N, int(iters), float(inf), _lib.ptr(dS), _lib.ptr(part),
                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(S0.device))
    return dS, part


class _TransportFn(torch.autograd.Function):
    """log_optimal_transport with a backward: the forward pads the scores (S0), keeps them and runs the transport of the no-grad path on a
    copy; the backward is lcr_log_sinkhorn_grad on S0 (it recomputes the duals itself), d_raw = scale * dS[:, :M, :N] and d_alpha = the sum
    of the per-problem dustbin sums (in fp64: a long sum with cancellation)."""

    @staticmethod
    def forward(ctx, raw_scores, alpha, row_masks, col_masks, scale, iters, inf):
        _lib.require_cuda(raw_scores, row_masks, col_masks, alpha)
        B, M, N = raw_scores.shape
        rm, cm = row_masks.to(torch.uint8).contiguous(), col_masks.to(torch.uint8).contiguous()
        S0 = torch.empty((B, M + 1, N + 1), dtype=torch.float32, device=raw_scores.device)
        raw, a1 = raw_scores.detach().contiguous(), alpha.detach().reshape(1).float()     # named: copies must outlive the argument list
        _lib.call.lcr_build_padded_scores(_lib.ptr(raw), _lib.ptr(rm), _lib.ptr(cm), B, M, N, scale, _lib.ptr(a1), inf, _lib.ptr(S0),
                                          _lib.stream_ptr(S0.device))
        ctx.save_for_backward(S0, rm, cm)
        ctx.scale, ctx.iters, ctx.inf, ctx.alpha_shape = scale, iters, inf, alpha.shape
        return _transport_padded(S0.clone(), rm, cm, iters, inf)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        S0, rm, cm = ctx.saved_tensors
        dS, part = log_sinkhorn_grad(S0, G.contiguous().float(), rm, cm, ctx.iters, ctx.inf)
        d_raw = dS[:, :-1, :-1] * ctx.scale if ctx.needs_input_grad[0] else None
        d_alpha = part.double().sum().float().reshape(ctx.alpha_shape) if ctx.needs_input_grad[1] else None
        return d_raw, d_alpha, None, None, None, None, None


PATCH_SCORES_FUSED = [os.environ.get("LCR_PATCH_SCORES_FUSED", "1") != "0"]      # A/B switch (tests, tools): 0 = gather + batched product + padding


def patch_log_optimal_transport(feats_a, idx_a, feats_b, idx_b, mask_a, mask_b, alpha, scale=1.0, iters=100, inf=1e12):
    """The patch-level transport of DenseMatchingHEAD (LCRNet.py:236-250): log scores [P,K+1,K+1] of P patch pairs whose point features are
    rows idx_a[p] of feats_a / idx_b[p] of feats_b (index == number of rows: the zero row of the padded tensor).  The gathers, the batched
    product, the scaling and the dustbin / mask padding are ONE kernel (lcr_patch_scores); LCR_PATCH_SCORES_FUSED=0 runs them apart.
    Differentiable in feats_a, feats_b and alpha: where the fused form applies the graph is _PatchTransportFn (lcr_log_sinkhorn_grad, then
    lcr_patch_scores_grad) and the bytes are the no-grad call's."""
    P, K = idx_a.shape
    if _wants_grad(feats_a, feats_b, alpha):
        if PATCH_SCORES_FUSED[0] and K == 128 and feats_a.shape[1] % 32 == 0 and P > 0:
            # training: the forward's one kernel, and its reverse lcr_patch_scores_grad behind the transport's
            return _PatchTransportFn.apply(feats_a, feats_b, alpha, idx_a, idx_b, mask_a, mask_b, float(scale), int(iters), float(inf))
        # outside the fused form: the gather (on the zero-row-padded features) and the product are torch's, which differentiates them; the
        # transport and its reverse pass are the library's
        fa = torch.cat([feats_a, feats_a.new_zeros(1, feats_a.shape[1])])[idx_a]
        fb = torch.cat([feats_b, feats_b.new_zeros(1, feats_b.shape[1])])[idx_b]
        return log_optimal_transport(torch.bmm(fa, fb.transpose(1, 2)), mask_a, mask_b, alpha, scale=scale, iters=iters, inf=inf)
    if not PATCH_SCORES_FUSED[0] or K != 128 or feats_a.shape[1] % 32 != 0 or P == 0:
        fa, fb = gather_rows(feats_a, idx_a.contiguous()), gather_rows(feats_b, idx_b.contiguous())
        return log_optimal_transport(bmm_nt(fa, fb), mask_a, mask_b, alpha, scale=scale, iters=iters, inf=inf)
    rm, cm = mask_a.to(torch.uint8).contiguous(), mask_b.to(torch.uint8).contiguous()
    S = _patch_scores(feats_a.contiguous(), feats_b.contiguous(), idx_a.contiguous(), idx_b.contiguous(), rm, cm, alpha, scale, inf)
    return _transport_padded(S, rm, cm, iters, inf)


def _patch_scores(fa, fb, ia, ib, rm, cm, alpha, scale, inf):
    """lcr_patch_scores on checked, contiguous operands -> the padded scores S0 [P,K+1,K+1]"""
    P, K = ia.shape
    assert ia.dtype == torch.int64 and ib.dtype == torch.int64 and fa.dtype == torch.float32 and fa.shape[1] == fb.shape[1]
    S = torch.empty((P, K + 1, K + 1), dtype=torch.float32, device=fa.device)
    a1 = alpha.reshape(1).float()                     # named: a copy must outlive the argument list
    _lib.call.lcr_patch_scores(_lib.ptr(fa), fa.shape[0], _lib.ptr(fb), fb.shape[0], fa.shape[1], _lib.ptr(ia), _lib.ptr(ib), _lib.ptr(rm),
                               _lib.ptr(cm), P, K, float(scale), _lib.ptr(a1), float(inf), _lib.ptr(S), _lib.stream_ptr(S.device))
    return S


def patch_scores_grad(dS, feats_a, feats_b, idx_a, idx_b, mask_a, mask_b, scale, inv_a=None, inv_b=None, want_a=True, want_b=True):
    """(d_feats_a [Na,C] or None, d_feats_b [Nb,C] or None) of lcr_patch_scores_grad from dS [P,K+1,K+1] (what log_sinkhorn_grad returns) and
    the operands of the forward; inv_*: the InvertedList (or (row_start, edges)) of idx_* as a [P,K] list over the rows of feats_* (built here
    when None).  No host synchronisation."""
    _lib.require_cuda(dS, feats_a, feats_b, idx_a, idx_b, mask_a, mask_b)
    P, K = idx_a.shape
    Na, Nb, C = feats_a.shape[0], feats_b.shape[0], feats_a.shape[1]
    assert dS.dtype == torch.float32 and dS.is_contiguous() and tuple(dS.shape) == (P, K + 1, K + 1)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (feats_a, feats_b)) and feats_b.shape[1] == C
    assert all(t.dtype == torch.int64 and t.is_contiguous() and tuple(t.shape) == (P, K) for t in (idx_a, idx_b))
    assert all(t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (P, K) for t in (mask_a, mask_b))
    ra = ea = rb = eb = None
    if want_a and P > 0:
        ra, ea = _inv_args(inv_a if inv_a is not None else inverted(idx_a, Na), P, K, Na)
    if want_b and P > 0:
        rb, eb = _inv_args(inv_b if inv_b is not None else inverted(idx_b, Nb), P, K, Nb)
    da = torch.empty((Na, C), dtype=torch.float32, device=dS.device) if want_a else None
    db = torch.empty((Nb, C), dtype=torch.float32, device=dS.device) if want_b else None
    ws = _lib.ws("lcr_patch_scores_grad_ws_bytes", P, K, C, device=dS.device)
    _lib.call.lcr_patch_scores_grad(_lib.ptr(dS), _lib.ptr(feats_a), Na, _lib.ptr(feats_b), Nb, C, _lib.ptr(idx_a), _lib.ptr(idx_b), _lib.ptr(mask_a),
                                    _lib.ptr(mask_b), P, K, float(scale), _lib.ptr(ra), _lib.ptr(ea), _lib.ptr(rb), _lib.ptr(eb), _lib.ptr(da),
                                    _lib.ptr(db), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dS.device))
    return da, db


class _PatchTransportFn(torch.autograd.Function):
    """patch_log_optimal_transport with a backward, in the manner of _TransportFn: the forward writes the padded scores S0 straight from the
    feature tensors (lcr_patch_scores), keeps them and runs the transport on a copy; the backward is lcr_log_sinkhorn_grad on S0, then
    lcr_patch_scores_grad (the gathered feature copies exist in neither direction), d_alpha = the fp64 sum of the per-problem dustbin sums.
    The inverted lists come through inverted(): a stack call (feats_a is feats_b) inside an inverted_lists() context builds each once."""

    @staticmethod
    def forward(ctx, feats_a, feats_b, alpha, idx_a, idx_b, mask_a, mask_b, scale, iters, inf):
        _lib.require_cuda(feats_a, feats_b, alpha, idx_a, idx_b, mask_a, mask_b)
        fa, fb = feats_a.detach().contiguous(), feats_b.detach().contiguous()
        ia, ib = idx_a.contiguous(), idx_b.contiguous()
        rm, cm = mask_a.to(torch.uint8).contiguous(), mask_b.to(torch.uint8).contiguous()
        S0 = _patch_scores(fa, fb, ia, ib, rm, cm, alpha.detach(), scale, inf)
        ctx.save_for_backward(S0, fa, fb, ia, ib, rm, cm)
        ctx.inv_a = inverted(ia, fa.shape[0]) if ctx.needs_input_grad[0] else None
        ctx.inv_b = inverted(ib, fb.shape[0]) if ctx.needs_input_grad[1] else None
        ctx.scale, ctx.iters, ctx.inf, ctx.alpha_shape = scale, iters, inf, alpha.shape
        return _transport_padded(S0.clone(), rm, cm, iters, inf)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, G):
        S0, fa, fb, ia, ib, rm, cm = ctx.saved_tensors
        dS, part = log_sinkhorn_grad(S0, G.contiguous().float(), rm, cm, ctx.iters, ctx.inf)
        da = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            da, db = patch_scores_grad(dS, fa, fb, ia, ib, rm, cm, ctx.scale, ctx.inv_a, ctx.inv_b, want_a=ctx.needs_input_grad[0],
                                       want_b=ctx.needs_input_grad[1])
        d_alpha = part.double().sum().float().reshape(ctx.alpha_shape) if ctx.needs_input_grad[2] else None
        return da, db, d_alpha, None, None, None, None, None, None, None


def _transport_padded(S, rm, cm, iters, inf):
    """Sinkhorn on padded scores S [B,M+1,N+1] in place -> log scores (the second half of LearnableLogOptimalTransport)."""
    B, M, N = S.shape[0], S.shape[1] - 1, S.shape[2] - 1
    dev = S.device
    uv = torch.empty((_lib.ws_size("lcr_log_sinkhorn_ws_floats", B, M, N),), dtype=torch.float32, device=dev)
    form = ctypes.c_int(0)
    _lib.call.lcr_log_sinkhorn_form(B, M, N, ctypes.byref(form))
    persistent = form.value == 2                      # the only form with hand-offs, i.e. the only one that writes a status word
    if persistent:
        uv[-1:].zero_()                               # status word: bit 0 = a hand-off of the persistent form timed out
    _lib.call.lcr_log_sinkhorn_ex(_lib.ptr(S), _lib.ptr(rm), _lib.ptr(cm), B, M, N, int(iters), float(inf), _lib.ptr(uv), uv.numel(),
                                  _lib.stream_ptr(dev))
    if persistent:
        # a stream-ordered 1-element copy (not a view: a view would pin the whole workspace until somebody drains the list)
        items = _pending_ot_status.items
        items.append(uv[-1:].view(torch.int32).clone())
        if len(items) > _PENDING_OT_MAX:              # callers that never reach top1_matching: fold on the device, no host sync
            # bitwise OR per device (the word is a set of flags; one host thread may drive several GPUs)
            by_dev = {}
            for t in items:
                by_dev.setdefault(t.device, []).append(t.reshape(()))
            folded = []
            for ts in by_dev.values():
                acc = ts[0]
                for t in ts[1:]:
                    acc = torch.bitwise_or(acc, t)
                folded.append(acc.reshape(1))
            _pending_ot_status.items = folded
    return S


def top1_matching(log_scores, row_masks=None, col_masks=None, mutual=False, topk=1, use_dustbin=True, confidence_threshold=0.0,
                  global_scores=None):
    """(bij int32 [C,3], scores f32 [C], per-row offsets are internal) — dustbin top-k matching (k = 1 in the shipped configuration),
    row-major order.  mutual: keep a pair only if it is kept from its row AND from its column (local_global_registration.py:84-85)
    instead of either.  topk > 1: the k largest of a row / column, dustbin included, each against the dustbin (:56-82; lcr_topk_matching).
    use_dustbin=False: selection over the interior, kept where the selected value exceeds confidence_threshold (:62-65); global_scores [B]:
    use_global_score (:236-237) — both through lcr_topk_matching_ex.  One host sync for the (data-dependent) number of correspondences."""
    B, M1, N1 = log_scores.shape
    M, N, dev = M1 - 1, N1 - 1, log_scores.device
    topk = int(topk)
    assert topk >= 1
    ws_fn = "lcr_top1_matching_ws_bytes" if (topk == 1 and use_dustbin and global_scores is None) else "lcr_topk_matching_ws_bytes"
    ws = _lib.ws(ws_fn, B, M, N, device=dev)
    rm = row_masks.to(torch.uint8).contiguous() if row_masks is not None else None
    cm = col_masks.to(torch.uint8).contiguous() if col_masks is not None else None
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    if not use_dustbin or global_scores is not None:
        gs = global_scores.float().contiguous() if global_scores is not None else None
        assert gs is None or gs.numel() == B
        fn, args = _lib.call.lcr_topk_matching_ex, (_lib.ptr(log_scores.contiguous()), B, M, N, _lib.ptr(rm), _lib.ptr(cm), topk, int(bool(mutual)),
                                                    int(bool(use_dustbin)), float(confidence_threshold), _lib.ptr(gs))
    elif topk == 1:
        fn, args = _lib.call.lcr_top1_matching_ex, (_lib.ptr(log_scores.contiguous()), B, M, N, _lib.ptr(rm), _lib.ptr(cm), int(bool(mutual)))
    else:
        fn, args = _lib.call.lcr_topk_matching, (_lib.ptr(log_scores.contiguous()), B, M, N, _lib.ptr(rm), _lib.ptr(cm), topk, int(bool(mutual)))
    fn(*args, _lib.ptr(total), None, None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    n = int(total.item())
    check_transport_status()
    bij = torch.empty((max(n, 1), 3), dtype=torch.int32, device=dev)
    sc = torch.empty((max(n, 1),), dtype=torch.float32, device=dev)
    if n:
        fn(*args, _lib.ptr(total), _lib.ptr(bij), _lib.ptr(sc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return bij[:n], sc[:n]


def upsample_concat(x, idx, skip):
    """[x[idx[:, 0]] (zeros for the shadow index), skip]; differentiable in x and skip (_UpsampleConcatFn) when one requires grad and grad
    mode is on."""
    _lib.require_cuda(x, idx, skip)
    if _wants_grad(x, skip):
        return _UpsampleConcatFn.apply(x, idx, skip)
    return _upsample_concat(x, idx, skip)


def upsample_concat_grad(d_out, idx, Nx, C1, inv=None, want_x=True, want_skip=True):
    """(d_x [Nx, C1] or None, d_skip [N, C - C1] or None) of lcr_upsample_concat_grad from d_out [N, C]; inv: the InvertedList (or
    (row_start, edges)) of COLUMN 0 of idx as an [N, 1] list over Nx rows (built here when None)."""
    _lib.require_cuda(d_out, idx)
    N, C = d_out.shape
    C1, C2 = int(C1), C - int(C1)
    assert d_out.dtype == torch.float32 and d_out.is_contiguous() and idx.shape[0] == N and 0 < C1 < C
    row_start = edges = None
    if want_x:
        if inv is None:
            inv = inverted(idx[:, :1].contiguous(), Nx)
        row_start, edges = _inv_args(inv, N, 1, int(Nx))
    dx = torch.empty((int(Nx), C1), dtype=torch.float32, device=d_out.device) if want_x else None
    ds = torch.empty((N, C2), dtype=torch.float32, device=d_out.device) if want_skip else None
    _lib.call.lcr_upsample_concat_grad(_lib.ptr(d_out), _lib.ptr(row_start), _lib.ptr(edges), N, int(Nx), C1, C2, _lib.ptr(dx), _lib.ptr(ds),
                                       _lib.stream_ptr(d_out.device))
    return dx, ds


class _UpsampleConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, skip):
        ctx.Nx, ctx.C1 = x.shape[0], x.shape[1]
        col0 = idx[:, :1].contiguous()
        ctx.save_for_backward(col0)
        ctx.inv = inverted(col0, x.shape[0]) if ctx.needs_input_grad[0] else None
        return _upsample_concat(x.detach(), idx, skip.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        col0, = ctx.saved_tensors
        dx, ds = upsample_concat_grad(d_out.contiguous().float(), col0, ctx.Nx, ctx.C1, ctx.inv, want_x=ctx.needs_input_grad[0],
                                      want_skip=ctx.needs_input_grad[2])
        return dx, None, ds


def _upsample_concat(x, idx, skip):
    out = torch.empty((skip.shape[0], x.shape[1] + skip.shape[1]), dtype=torch.float32, device=x.device)
    _lib.call.lcr_upsample_concat(_lib.ptr(x.contiguous()), x.shape[0], x.shape[1], _lib.ptr(idx.contiguous()), _idx_args(idx), idx.shape[1],
                                  _lib.ptr(skip.contiguous()), skip.shape[1], skip.shape[0], _lib.ptr(out), _lib.stream_ptr(x.device))
    return out


def gather_rows(src, idx):
    """src[idx] with zero rows where idx == src.shape[0] (index_select on the zero-padded tensor); idx int64 any shape."""
    idx = idx.contiguous()
    out = torch.empty(tuple(idx.shape) + (src.shape[1],), dtype=torch.float32, device=src.device)
    _lib.call.lcr_gather_rows(_lib.ptr(src.contiguous()), src.shape[0], src.shape[1], _lib.ptr(idx), idx.numel(), _lib.ptr(out), _lib.stream_ptr(src.device))
    return out


def bmm_nt(a, b):
    """[P,M,K] x [P,N,K]^T -> [P,M,N] on the MFMA GEMM (einsum 'bnd,bmd->bnm').  With a graph when a or b requires grad and grad mode is on
    (_BmmNTFn: both gradient products on the same batched GEMM)."""
    if _wants_grad(a, b):
        return _BmmNTFn.apply(a, b)
    return _bmm(a.contiguous(), b.contiguous(), False, True)


def _bmm(a, b, trans_a, trans_b):
    """C_z = op(a_z) . op(b_z) on lcr_gemm_f32_strided_batched: a [P,M,K] ([P,K,M] with trans_a), b [P,K,N] ([P,N,K] with trans_b), both
    contiguous.  The entry wants leading dimensions and strides of a and b in multiples of 4 floats."""
    P = a.shape[0]
    M, K = (a.shape[2], a.shape[1]) if trans_a else (a.shape[1], a.shape[2])
    N = b.shape[1] if trans_b else b.shape[2]
    c = torch.empty((P, M, N), dtype=torch.float32, device=a.device)
    for z0 in range(0, P, 65535):
        cnt = min(65535, P - z0)
        _lib.call.lcr_gemm_f32_strided_batched(_lib.ptr(a[z0:]), _lib.ptr(b[z0:]), _lib.ptr(c[z0:]), M, N, K, int(trans_a), int(trans_b), M * K, N * K,
                                               M * N, cnt, _lib.stream_ptr(a.device))
    return c


class _BmmNTFn(torch.autograd.Function):
    """bmm_nt with a backward: for C = A.B^T, dA = dC.B and dB = dC^T.A on lcr_gemm_f32_strided_batched.  That entry reads dC with leading
    dimension N and stride M N, which it wants in multiples of 4 floats: where N % 4 != 0 the cotangent batch is padded with zero columns to
    the next multiple (and B with zero rows for dA, whose contraction runs over them: exact zeros added last), and dB drops the rows."""

    @staticmethod
    def forward(ctx, a, b):
        _lib.require_cuda(a, b)
        ac, bc = a.detach().contiguous(), b.detach().contiguous()
        ctx.save_for_backward(ac, bc)
        return _bmm(ac, bc, False, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        N = b.shape[1]
        dc = dc.contiguous().float()
        pad = -N % 4
        if pad:
            dc = torch.nn.functional.pad(dc, (0, pad))
        da = db = None
        if ctx.needs_input_grad[0]:
            da = _bmm(dc, torch.nn.functional.pad(b, (0, 0, 0, pad)) if pad else b, False, False)
        if ctx.needs_input_grad[1]:
            db = _bmm(dc, a, True, False)
            if pad:
                db = db[:, :N].contiguous()
        return da, db


class _GemmNTFn(torch.autograd.Function):
    """gemm(a, b, trans_b=True) with a backward on the same entry: dA = dC.B, dB = dC^T.A (lcr_gemm_f32 with trans_a)."""

    @staticmethod
    def forward(ctx, a, b):
        ac, bc = a.detach().contiguous(), b.detach().contiguous()
        ctx.save_for_backward(ac, bc)
        return gemm(ac, bc, trans_b=True)[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = dc.contiguous().float()
        da = gemm(dc, b)[0] if ctx.needs_input_grad[0] else None
        db = gemm(dc, a, trans_a=True)[0] if ctx.needs_input_grad[1] else None
        return da, db


def procrustes(src, ref, w, start=None):
    """Batched weighted Procrustes: problems = ranges [start[p], start[p+1]) (int32 device) or one problem over all rows."""
    dev = src.device
    if start is None:
        start = host_values([0, src.shape[0]], torch.int32, dev)
    P = start.numel() - 1
    T = torch.empty((P, 4, 4), dtype=torch.float32, device=dev)
    _lib.call.lcr_procrustes_batched(_lib.ptr(src.contiguous()), _lib.ptr(ref.contiguous()), _lib.ptr(w.contiguous()), _lib.ptr(start), P, 1e-5,
                                     _lib.ptr(T), _lib.stream_ptr(src.device))
    return T


def inlier_count(T, src, ref, radius, start=None, min_count=0):
    P, dev = T.shape[0], T.device
    counts = torch.empty((P,), dtype=torch.int32, device=dev)
    best = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.call.lcr_inlier_count(_lib.ptr(T), P, _lib.ptr(src), _lib.ptr(ref), src.shape[0], float(radius), _lib.ptr(start), int(min_count),
                               _lib.ptr(counts), _lib.ptr(best), _lib.stream_ptr(T.device))
    return counts, best


def local_global_registration(src, ref, score, hyp_start, seg_hyp_start, radius, min_count, steps, want_details=False, correspondence_limit=None):
    """local_to_global_registration (local_global_registration.py:134-201) for S pairs in one native call: correspondences stacked
    pair-major, hyp_start int32 [H+1] (one chunk per patch correspondence), seg_hyp_start int32 [S+1] (the chunks of every pair)
    -> T [S,4,4] (and, with want_details, the hypotheses [H,4,4], their inlier counts [H] and the winner per pair [S]).
    correspondence_limit (:152-160): a pair with more correspondences verifies and refits on its highest-scoring `limit` ones only."""
    dev = src.device
    n, H, S = src.shape[0], hyp_start.numel() - 1, seg_hyp_start.numel() - 1
    ws = _lib.ws("lcr_lgr_ws_bytes", n, H, S, device=dev)
    T = torch.empty((S, 4, 4), dtype=torch.float32, device=dev)
    hyp = torch.empty((H, 4, 4), dtype=torch.float32, device=dev) if want_details else None
    counts = torch.empty((H,), dtype=torch.int32, device=dev) if want_details else None
    best = torch.empty((S,), dtype=torch.int32, device=dev) if want_details else None
    _lib.call.lcr_local_global_registration_ex(_lib.ptr(src.contiguous()), _lib.ptr(ref.contiguous()), _lib.ptr(score.contiguous()), n,
                                               _lib.ptr(hyp_start.contiguous()), H, _lib.ptr(seg_hyp_start.contiguous()), S, float(radius),
                                               int(min_count), int(steps), int(correspondence_limit or 0), _lib.ptr(T), _lib.ptr(hyp),
                                               _lib.ptr(counts), _lib.ptr(best), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(src.device))
    return (T, hyp, counts, best) if want_details else T


def inlier_weights(T_all, sel, src, ref, score, radius):
    w = torch.empty_like(score)
    _lib.call.lcr_inlier_weights(_lib.ptr(T_all), _lib.ptr(sel), _lib.ptr(src), _lib.ptr(ref), _lib.ptr(score), src.shape[0], float(radius),
                                 _lib.ptr(w), _lib.stream_ptr(T_all.device))
    return w


def ransac_correspondences(src, ref, start, distance_threshold, ransac_n, num_iterations, seed=0, want_details=False):
    """Deterministic correspondence RANSAC (include/lcr_hip.h, lcr_ransac_correspondences) for S pairs in one native call:
    src / ref f32 [n,3] stacked pair-major, start int32 [S+1] -> T [S,4,4] (src onto ref), inliers int32 [S], rmse f32 [S], best_h int32 [S]
    (and with want_details every hypothesis [S*iters,4,4], its inlier count [S*iters] (-1 = invalid) and inlier SSE [S*iters])."""
    _lib.require_cuda(src, ref, start)
    dev = src.device
    S, iters = start.numel() - 1, int(num_iterations)
    ws = _lib.ws("lcr_ransac_ws_bytes", S, iters, device=dev)
    T = torch.empty((S, 4, 4), dtype=torch.float32, device=dev)
    inliers = torch.empty((S,), dtype=torch.int32, device=dev)
    rmse = torch.empty((S,), dtype=torch.float32, device=dev)
    best = torch.empty((S,), dtype=torch.int32, device=dev)
    T_all = torch.empty((S * iters, 4, 4), dtype=torch.float32, device=dev) if want_details else None
    counts = torch.empty((S * iters,), dtype=torch.int32, device=dev) if want_details else None
    sse = torch.empty((S * iters,), dtype=torch.float32, device=dev) if want_details else None
    _lib.call.lcr_ransac_correspondences(_lib.ptr(src.contiguous()), _lib.ptr(ref.contiguous()), _lib.ptr(start.contiguous()), S,
                                         float(distance_threshold), int(ransac_n), iters, int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(T),
                                         _lib.ptr(inliers), _lib.ptr(rmse), _lib.ptr(best), _lib.ptr(T_all), _lib.ptr(counts), _lib.ptr(sse),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr(src.device))
    if want_details:
        return T, inliers, rmse, best, T_all, counts, sse
    return T, inliers, rmse, best


def ransac_correspondences_ex(src, ref, start, distance_threshold, ransac_n, num_iterations, seed=0, edge_similarity=0.0, checker_distance=0.0,
                              corr=None, src_start=None, ref_start=None, want_details=False, want_reject=False):
    """Correspondence RANSAC with Open3D's correspondence checkers (include/lcr_hip.h, lcr_ransac_correspondences_ex): the arguments and
    outputs of ransac_correspondences, plus edge_similarity / checker_distance (<= 0: off) and the index form: with corr int32 [n,2]
    (pair-local src row, ref row; start [S+1] offsets its rows) src / ref are the pairs' point clouds stacked with src_start / ref_start.
    want_reject appends reject_all uint8 [S*iters] (0 valid, 1 degenerate, 2 edge check, 3 distance check).  Both checks off and no corr:
    the bits of ransac_correspondences."""
    _lib.require_cuda(src, ref, start)
    dev = src.device
    S, iters = start.numel() - 1, int(num_iterations)
    n_corr = 0
    if corr is not None:
        if src_start is None or ref_start is None:
            raise ValueError("ransac_correspondences_ex: corr needs src_start and ref_start")
        _lib.require_cuda(corr, src_start, ref_start)
        if corr.dtype != torch.int32 or corr.dim() != 2 or corr.shape[1] != 2 or src_start.numel() != S + 1 or ref_start.numel() != S + 1:
            raise ValueError("ransac_correspondences_ex: corr must be int32 [n,2] and src_start / ref_start int32 [S+1]")
        corr, src_start, ref_start = corr.contiguous(), src_start.contiguous(), ref_start.contiguous()
        n_corr = corr.shape[0]
    ws = _lib.ws("lcr_ransac_ex_ws_bytes", S, iters, n_corr, device=dev)
    T = torch.empty((S, 4, 4), dtype=torch.float32, device=dev)
    inliers = torch.empty((S,), dtype=torch.int32, device=dev)
    rmse = torch.empty((S,), dtype=torch.float32, device=dev)
    best = torch.empty((S,), dtype=torch.int32, device=dev)
    T_all = torch.empty((S * iters, 4, 4), dtype=torch.float32, device=dev) if want_details else None
    counts = torch.empty((S * iters,), dtype=torch.int32, device=dev) if want_details else None
    sse = torch.empty((S * iters,), dtype=torch.float32, device=dev) if want_details else None
    reject = torch.empty((S * iters,), dtype=torch.uint8, device=dev) if want_reject else None
    _lib.call.lcr_ransac_correspondences_ex(_lib.ptr(src.contiguous()), _lib.ptr(ref.contiguous()), _lib.ptr(start.contiguous()), S, _lib.ptr(corr),
                                            _lib.ptr(src_start), _lib.ptr(ref_start), n_corr, float(distance_threshold), int(ransac_n), iters,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, float(edge_similarity), float(checker_distance), _lib.ptr(T),
                                            _lib.ptr(inliers), _lib.ptr(rmse), _lib.ptr(best), _lib.ptr(T_all), _lib.ptr(counts), _lib.ptr(sse),
                                            _lib.ptr(reject), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(src.device))
    out = (T, inliers, rmse, best) + ((T_all, counts, sse) if want_details else ())
    return out + ((reject,) if want_reject else ())


def feature_nn(qf, df, q_start, d_start):
    """Exact nearest neighbour in feature space (include/lcr_hip.h, lcr_feature_nn) for S pairs in one native call: qf f32 [nq,C] /
    df f32 [nd,C] stacked pair-major, q_start / d_start int32 [S+1] -> (nn int32 [nq]: the pair-local database row with the smallest
    (d2, row), -1 where the pair's database is empty or every distance is NaN; d2 f32 [nq])."""
    _lib.require_cuda(qf, df, q_start, d_start)
    if qf.dim() != 2 or df.dim() != 2 or qf.shape[1] != df.shape[1] or qf.dtype != torch.float32 or df.dtype != torch.float32:
        raise ValueError("feature_nn: qf [nq,C] and df [nd,C] must be float32 with the same C")
    if q_start.dtype != torch.int32 or d_start.dtype != torch.int32 or q_start.numel() != d_start.numel():
        raise ValueError("feature_nn: q_start and d_start must be int32 [S+1]")
    dev = qf.device
    S, C, nq, nd = q_start.numel() - 1, qf.shape[1], qf.shape[0], df.shape[0]
    ws = _lib.ws("lcr_feature_nn_ws_bytes", S, nq, nd, device=dev)
    nn = torch.empty((nq,), dtype=torch.int32, device=dev)
    d2 = torch.empty((nq,), dtype=torch.float32, device=dev)
    _lib.call.lcr_feature_nn(_lib.ptr(qf.contiguous()), _lib.ptr(df.contiguous()), _lib.ptr(q_start.contiguous()),
                             _lib.ptr(d_start.contiguous()), S, C, nq, nd, _lib.ptr(nn), _lib.ptr(d2), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(qf.device))
    return nn, d2


def feature_correspondences(nn_sr, src_start, ref_start, nn_rs=None, min_rows=3):
    """Correspondences from nearest-neighbour rows (include/lcr_hip.h, lcr_feature_correspondences): nn_sr int32 [ns] (src -> ref, stacked
    with src_start [S+1]) and, for the mutual filter, nn_rs int32 [nr] (ref -> src, stacked with ref_start [S+1]) -> (corr int32 [ns,2] of
    which the first start[S] rows are written: (src row, ref row) pair-local in ascending src row; start int32 [S+1]; mutual_used
    int32 [S]).  A pair whose mutual set has fewer than min_rows rows falls back to its unfiltered set."""
    _lib.require_cuda(nn_sr, src_start, ref_start, *([nn_rs] if nn_rs is not None else []))
    for t in (nn_sr, src_start, ref_start) + ((nn_rs,) if nn_rs is not None else ()):
        if t.dtype != torch.int32:
            raise ValueError("feature_correspondences: int32 tensors expected")
    dev = nn_sr.device
    S = src_start.numel() - 1
    if ref_start.numel() != S + 1:
        raise ValueError("feature_correspondences: src_start and ref_start must both be int32 [S+1]")
    ws = _lib.ws("lcr_feature_correspondences_ws_bytes", S, device=dev)
    corr = torch.empty((nn_sr.numel(), 2), dtype=torch.int32, device=dev)
    start = torch.empty((S + 1,), dtype=torch.int32, device=dev)
    used = torch.empty((S,), dtype=torch.int32, device=dev)
    _lib.call.lcr_feature_correspondences(_lib.ptr(nn_sr.contiguous()), _lib.ptr(src_start.contiguous()),
                                          _lib.ptr(nn_rs.contiguous() if nn_rs is not None else None), _lib.ptr(ref_start.contiguous()), S,
                                          int(min_rows), _lib.ptr(corr), _lib.ptr(start), _lib.ptr(used), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr(nn_sr.device))
    return corr, start, used


def node_correspondences_ws_bytes(point_off, node_off, K):
    """Workspace bytes of lcr_node_correspondences for these host offset lists (2P+1 entries each)."""
    po, mo = np.ascontiguousarray(point_off, dtype=np.int64), np.ascontiguousarray(node_off, dtype=np.int64)
    return _lib.ws_size("lcr_node_correspondences_ws_bytes", po.ctypes.data, mo.ctypes.data, (len(po) - 1) // 2, int(K))


def node_correspondences_raw(points_f, point_off, nodes, node_off, knn, knn_mask, node_mask, transforms, pos_radius, cap=None, ws=None, corr=None,
                             overlap=None, start=None, status=None):
    """lcr_node_correspondences (include/lcr_hip.h) as it is: no host synchronisation.  -> (corr int32 [cap,2], overlap f32 [cap],
    start int32 [P+1], status int32 [1]); rows at or beyond start[P] are not written.  cap defaults to sum M_p * N_p, which cannot
    overflow; ws / corr / overlap / start / status may be caller-owned buffers (uint8 / int32 / float32 / int32 / int32)."""
    po, mo = np.ascontiguousarray(point_off, dtype=np.int64), np.ascontiguousarray(node_off, dtype=np.int64)
    if len(po) != len(mo) or len(po) < 3 or len(po) % 2 == 0:
        raise ValueError("node_correspondences: point_off and node_off must have 2P+1 entries, P >= 1")
    P = (len(po) - 1) // 2
    _lib.require_cuda(points_f, nodes, knn, knn_mask, node_mask, transforms)
    if points_f.dtype != torch.float32 or transforms.dtype != torch.float32 or knn.dtype != torch.int64 or knn.dim() != 2:
        raise ValueError("node_correspondences: points_f / transforms float32, knn int64 [M,K]")
    if transforms.numel() != 16 * P or knn.shape[0] != mo[-1] - mo[0] or knn_mask.shape != knn.shape or node_mask.numel() != knn.shape[0]:
        raise ValueError("node_correspondences: one 4x4 transform per pair, knn / knn_mask [sum M, K], node_mask [sum M]")
    if points_f.shape[0] < po[-1] or nodes.shape[0] < mo[-1]:
        raise ValueError("node_correspondences: offsets beyond the stacked rows")
    dev = points_f.device
    K = knn.shape[1]
    as_u8 = lambda t: (t.to(torch.uint8) if t.dtype != torch.uint8 else t).contiguous()
    km, nm = as_u8(knn_mask), as_u8(node_mask)
    m = np.diff(mo)
    if cap is None:
        cap = int((m[0::2] * m[1::2]).sum())
    if ws is None:
        ws = _lib.workspace(node_correspondences_ws_bytes(po, mo, K), dev)
    corr = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=dev) if corr is None else corr
    overlap = torch.empty((max(cap, 1),), dtype=torch.float32, device=dev) if overlap is None else overlap
    start = torch.empty((P + 1,), dtype=torch.int32, device=dev) if start is None else start
    status = torch.empty((1,), dtype=torch.int32, device=dev) if status is None else status
    _lib.call.lcr_node_correspondences(_lib.ptr(points_f.contiguous()), po.ctypes.data, _lib.ptr(nodes.contiguous()), mo.ctypes.data,
                                       _lib.ptr(knn.contiguous()), _lib.ptr(km), _lib.ptr(nm), _lib.ptr(transforms.contiguous()), P, K,
                                       float(pos_radius), int(cap), _lib.ptr(corr), _lib.ptr(overlap), _lib.ptr(start), _lib.ptr(status),
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points_f.device))
    return corr, overlap, start, status


def node_correspondences(points_f, point_off, nodes, node_off, knn, knn_mask, node_mask, transforms, pos_radius):
    """Ground-truth node correspondences of P pairs in one native call (include/lcr_hip.h, lcr_node_correspondences): the stacked outputs
    of `point_to_node_partition_stack` for the clouds [pos_0, anc_0, pos_1, anc_1, ...] (host offset lists of 2P+1 entries), transforms
    f32 [P,4,4] (anc onto pos) -> (corr int64 [C,2]: pair-local (ref node, src node) rows, row-major within a pair, pairs in order;
    overlaps f32 [C]; start int32 [P+1]: pair p owns rows start[p] .. start[p+1]).  One host synchronisation, to size the result."""
    corr, overlap, start, _ = node_correspondences_raw(points_f, point_off, nodes, node_off, knn, knn_mask, node_mask, transforms, pos_radius)
    C = int(start[-1].item())
    return corr[:C].long(), overlap[:C].clone(), start


def ransac_sample_host(seed, h0, count, ransac_n, n):
    """The RANSAC sampler on the host (no GPU): int32 [count, ransac_n] row indices of hypotheses h0 .. h0+count-1 for a pair of n rows."""
    out = np.empty((int(count), int(ransac_n)), dtype=np.int32)
    _lib.call.lcr_ransac_sample_host(int(seed) & 0xFFFFFFFFFFFFFFFF, int(h0), int(count), int(ransac_n), int(n), out.ctypes.data)
    return out


TEASER_MAX_ROWS = 4096                                   # rows per problem at most (csrc/teaser.hip TZ_MAX_ROWS)
TEASER_MODES = {"kcore": 0, "none": 1}


def teaser_registration(src, ref, start, noise_bound=0.01, cbar2=1.0, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12,
                        inlier_selection="kcore", max_rows=None, want_details=False):
    """TEASER-style robust registration (include/lcr_hip.h, lcr_teaser_registration) for S problems in one native call: src / ref f32 [n,3]
    stacked problem-major, start int32 [S+1] -> T f32 [S,4,4] (src onto ref), valid int32 [S], n_selected int32 [S], rot_inliers int64 [S],
    t_count int32 [S,3] (and with want_details iterations int32 [S], cost f64 [S], selected_mask uint8 [n], core int32 [n]).  max_rows: an
    upper bound on the rows of one problem (default min(n, 4096); a problem above it comes back invalid).  Nothing is read back."""
    if inlier_selection not in TEASER_MODES:
        raise ValueError("teaser_registration: inlier_selection must be 'kcore' or 'none', got %r" % (inlier_selection,))
    nb, cb, gf, ct, mi = float(noise_bound), float(cbar2), float(gnc_factor), float(cost_threshold), int(max_iterations)
    if not (np.isfinite([nb, cb, gf, ct]).all() and nb > 0 and cb > 0 and gf > 1 and ct >= 0 and 1 <= mi <= 1000):
        raise ValueError("teaser_registration: needs noise_bound > 0, cbar2 > 0, gnc_factor > 1, 1 <= max_iterations <= 1000 and "
                         "cost_threshold >= 0 (noise_bound=%r cbar2=%r gnc_factor=%r max_iterations=%r cost_threshold=%r)"
                         % (noise_bound, cbar2, gnc_factor, max_iterations, cost_threshold))
    _lib.require_cuda(src, ref, start)
    if src.dtype != torch.float32 or ref.dtype != torch.float32 or src.dim() != 2 or src.shape[1] != 3 or src.shape != ref.shape:
        raise ValueError("teaser_registration: src and ref must be float32 [n,3] of the same shape")
    if start.dtype != torch.int32 or start.dim() != 1 or start.numel() < 2:
        raise ValueError("teaser_registration: start must be int32 [S+1] with S >= 1")
    dev = src.device
    S, n, mode = start.numel() - 1, src.shape[0], TEASER_MODES[inlier_selection]
    max_rows = min(n, TEASER_MAX_ROWS) if max_rows is None else int(max_rows)
    ws = _lib.ws("lcr_teaser_ws_bytes", S, n, max_rows, mode, device=dev)
    T = torch.empty((S, 4, 4), dtype=torch.float32, device=dev)
    valid = torch.empty((S,), dtype=torch.int32, device=dev)
    nsel = torch.empty((S,), dtype=torch.int32, device=dev)
    rot = torch.empty((S,), dtype=torch.int64, device=dev)
    tcount = torch.empty((S, 3), dtype=torch.int32, device=dev)
    iters = torch.empty((S,), dtype=torch.int32, device=dev) if want_details else None
    cost = torch.empty((S,), dtype=torch.float64, device=dev) if want_details else None
    mask = torch.empty((n,), dtype=torch.uint8, device=dev) if want_details else None
    core = torch.empty((n,), dtype=torch.int32, device=dev) if want_details else None
    _lib.call.lcr_teaser_registration(_lib.ptr(src.contiguous()), _lib.ptr(ref.contiguous()), _lib.ptr(start.contiguous()), S, n, max_rows, nb, cb,
                                      gf, mi, ct, mode, _lib.ptr(T), _lib.ptr(valid), _lib.ptr(nsel), _lib.ptr(rot), _lib.ptr(tcount),
                                      _lib.ptr(iters), _lib.ptr(cost), _lib.ptr(mask), _lib.ptr(core), _lib.ptr(ws), ws.numel(),
                                      _lib.stream_ptr(dev))
    out = (T, valid, nsel, rot, tcount)
    return out + (iters, cost, mask, core) if want_details else out


def icp_point_to_point(src, src_len, tgt, tgt_len, init, max_correspondence_distance, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                       check_every=16, want_corr=False, want_history=False):
    """Point-to-point ICP (include/lcr_hip.h, lcr_icp_point_to_point) for S <= 64 pairs in one native call: src f32 [ns,3] / tgt f32 [nt,3]
    stacked pair-major with host lengths src_len / tgt_len (S ints), init f64 [S,4,4] (source onto target) on the device ->
    dict(T f64 [S,4,4], fitness f64 [S], inlier_rmse f64 [S], iterations int32 [S]; with want_corr corr int32 [ns] (pair-local target row or -1);
    with want_history T_hist f64 [S, max_iteration+1, 4, 4], fitness_hist / rmse_hist f64 [S, max_iteration+1], NaN after `iterations`)."""
    return _icp("icp_point_to_point", src, src_len, tgt, tgt_len, None, init, max_correspondence_distance, max_iteration, relative_fitness,
                relative_rmse, check_every, want_corr, want_history)


def icp_point_to_plane(src, src_len, tgt, tgt_len, tgt_normals, init, max_correspondence_distance, max_iteration=30, relative_fitness=1e-6,
                       relative_rmse=1e-6, check_every=16, want_corr=False, want_history=False):
    """Point-to-plane ICP (include/lcr_hip.h, lcr_icp_point_to_plane): icp_point_to_point's arguments and outputs, plus the target normals
    tgt_normals f32 [nt,3] on the device (estimate_normals writes them; zero rows stay out of the update)."""
    if tgt_normals is None:
        raise ValueError("icp_point_to_plane: the target needs normals")
    return _icp("icp_point_to_plane", src, src_len, tgt, tgt_len, tgt_normals, init, max_correspondence_distance, max_iteration, relative_fitness,
                relative_rmse, check_every, want_corr, want_history)


def icp_generalized(src, src_len, src_normals, tgt, tgt_len, tgt_normals, init, max_correspondence_distance, epsilon=1e-3, max_iteration=30,
                    relative_fitness=1e-6, relative_rmse=1e-6, check_every=16, want_corr=False, want_history=False):
    """Generalized (plane-to-plane) ICP (include/lcr_hip.h, lcr_icp_generalized): icp_point_to_plane's arguments and outputs, plus the source
    normals src_normals f32 [ns,3] on the device and epsilon in [1e-6, 1], the covariance along a normal against 1 across it (zero normal
    rows count as isotropic)."""
    if src_normals is None or tgt_normals is None:
        raise ValueError("icp_generalized: both clouds need normals")
    return _icp("icp_generalized", src, src_len, tgt, tgt_len, tgt_normals, init, max_correspondence_distance, max_iteration, relative_fitness,
                relative_rmse, check_every, want_corr, want_history, src_normals=src_normals, epsilon=epsilon)


def _icp(name, src, src_len, tgt, tgt_len, tgt_normals, init, max_correspondence_distance, max_iteration, relative_fitness, relative_rmse,
         check_every, want_corr, want_history, src_normals=None, epsilon=None):
    plane, gicp = tgt_normals is not None, src_normals is not None
    _lib.require_cuda(src, tgt, init, *([tgt_normals] if plane else []), *([src_normals] if gicp else []))
    dev = src.device
    S, iters = len(src_len), int(max_iteration)
    sl = np.ascontiguousarray(np.asarray(src_len, dtype=np.int64).reshape(-1))
    tl = np.ascontiguousarray(np.asarray(tgt_len, dtype=np.int64).reshape(-1))
    if len(tl) != S or init.shape != (S, 4, 4) or init.dtype != torch.float64:
        raise ValueError("%s: src_len, tgt_len and init [S,4,4] float64 must describe the same S pairs" % name)
    if src.shape[0] != int(sl.sum()) or tgt.shape[0] != int(tl.sum()):
        raise ValueError("%s: the point arrays do not hold sum(src_len) / sum(tgt_len) rows" % name)
    if plane and (tuple(tgt_normals.shape) != tuple(tgt.shape) or tgt_normals.dtype != torch.float32):
        raise ValueError("%s: tgt_normals must be float32 with the shape of tgt" % name)
    if gicp and (tuple(src_normals.shape) != tuple(src.shape) or src_normals.dtype != torch.float32):
        raise ValueError("%s: src_normals must be float32 with the shape of src" % name)
    src, tgt, init = src.contiguous(), tgt.contiguous(), init.contiguous()
    ws = _lib.ws("lcr_icp_generalized_ws_bytes" if gicp else "lcr_icp_plane_ws_bytes" if plane else "lcr_icp_ws_bytes", S, src.shape[0],
                 tgt.shape[0], device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"T": torch.empty((S, 4, 4), **f64), "fitness": torch.empty((S,), **f64), "inlier_rmse": torch.empty((S,), **f64),
           "iterations": torch.empty((S,), dtype=torch.int32, device=dev)}
    corr = torch.empty((src.shape[0],), dtype=torch.int32, device=dev) if want_corr else None
    hist = [torch.full((S, iters + 1, 4, 4), float("nan"), **f64), torch.full((S, iters + 1), float("nan"), **f64),
            torch.full((S, iters + 1), float("nan"), **f64)] if want_history else [None, None, None]
    tail = (iters, float(relative_fitness), float(relative_rmse), _lib.ptr(out["T"]), _lib.ptr(out["fitness"]),
            _lib.ptr(out["inlier_rmse"]), _lib.ptr(out["iterations"]), _lib.ptr(corr), _lib.ptr(hist[0]), _lib.ptr(hist[1]), _lib.ptr(hist[2]),
            int(check_every), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(src.device))
    tail = (float(max_correspondence_distance),) + ((float(epsilon),) if gicp else ()) + tail
    if gicp:
        sn, nrm = src_normals.contiguous(), tgt_normals.contiguous()
        _lib.call.lcr_icp_generalized(_lib.ptr(src), sl.ctypes.data, _lib.ptr(sn), _lib.ptr(tgt), tl.ctypes.data, _lib.ptr(nrm), S, _lib.ptr(init),
                                      *tail)
    elif plane:
        nrm = tgt_normals.contiguous()
        _lib.call.lcr_icp_point_to_plane(_lib.ptr(src), sl.ctypes.data, _lib.ptr(tgt), tl.ctypes.data, _lib.ptr(nrm), S, _lib.ptr(init), *tail)
    else:
        _lib.call.lcr_icp_point_to_point(_lib.ptr(src), sl.ctypes.data, _lib.ptr(tgt), tl.ctypes.data, S, _lib.ptr(init), *tail)
    if want_corr:
        out["corr"] = corr
    if want_history:
        out["T_hist"], out["fitness_hist"], out["rmse_hist"] = hist
    return out


NORMALS_MAX_CLOUDS = 64   # clouds per lcr_estimate_normals call (the support grid's limit)
NORMALS_MAX_NN = 128


def estimate_normals(points, lengths, radius, max_nn, viewpoint=None, want_curvature=False, want_count=False):
    """Surface normals (include/lcr_hip.h, lcr_estimate_normals; Open3D's EstimateNormals(KDTreeSearchParamHybrid(radius, max_nn))) for
    B <= 64 clouds in one native call: points f32 [N,3] on the device stacked cloud-major, lengths host ints [B], viewpoint f32 [B,3] (or
    None: each cloud's origin) -> dict(normals f32 [N,3] (zero rows where degenerate); with want_curvature curvature f32 [N]; with
    want_count count int32 [N], the neighbours used).  Asynchronous on the current stream."""
    _lib.require_cuda(points)
    dev = points.device
    ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    B = len(ln)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32 or points.shape[0] != int(ln.sum()):
        raise ValueError("estimate_normals: points must be float32 [sum(lengths), 3]")
    points = points.contiguous()
    vp = None
    if viewpoint is not None:
        vp = (viewpoint if torch.is_tensor(viewpoint) else torch.from_numpy(np.asarray(viewpoint, dtype=np.float32)))
        vp = vp.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        if vp.shape[0] != B:
            raise ValueError("estimate_normals: viewpoint must be [B,3] for the B clouds")
    ws = _lib.ws("lcr_normals_ws_bytes", B, points.shape[0], device=dev)
    n = points.shape[0]
    out = {"normals": torch.empty((n, 3), dtype=torch.float32, device=dev)}
    curv = torch.empty((n,), dtype=torch.float32, device=dev) if want_curvature else None
    cnt = torch.empty((n,), dtype=torch.int32, device=dev) if want_count else None
    _lib.call.lcr_estimate_normals(_lib.ptr(points), ln.ctypes.data, B, float(radius), int(max_nn), _lib.ptr(vp), _lib.ptr(out["normals"]),
                                   _lib.ptr(curv), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points.device))
    if want_curvature:
        out["curvature"] = curv
    if want_count:
        out["count"] = cnt
    return out


FPFH_MAX_CLOUDS = 64      # clouds per lcr_fpfh call (the support grid's limit)
FPFH_MAX_NN = 128
FPFH_BINS = 33


def fpfh(points, normals, lengths, radius, max_nn, want_spfh=False, want_count=False):
    """FPFH descriptors (include/lcr_hip.h, lcr_fpfh; Open3D's compute_fpfh_feature(KDTreeSearchParamHybrid(radius, max_nn))) for B <= 64
    clouds in one native call: points / normals f32 [N,3] on the device stacked cloud-major, lengths host ints [B] -> dict(features f32
    [N,33]; with want_spfh spfh f32 [N,33]; with want_count count int32 [N], the neighbours that voted).  Asynchronous on the current
    stream."""
    _lib.require_cuda(points, normals)
    dev = points.device
    ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    B = len(ln)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32 or points.shape[0] != int(ln.sum()):
        raise ValueError("fpfh: points must be float32 [sum(lengths), 3]")
    if tuple(normals.shape) != tuple(points.shape) or normals.dtype != torch.float32 or normals.device != dev:
        raise ValueError("fpfh: normals must be float32 with the shape and device of points")
    points, normals = points.contiguous(), normals.contiguous()
    n = points.shape[0]
    ws = _lib.ws("lcr_fpfh_ws_bytes", B, n, int(max_nn), device=dev)
    out = {"features": torch.empty((n, FPFH_BINS), dtype=torch.float32, device=dev)}
    spfh = torch.empty((n, FPFH_BINS), dtype=torch.float32, device=dev) if want_spfh else None
    cnt = torch.empty((n,), dtype=torch.int32, device=dev) if want_count else None
    _lib.call.lcr_fpfh(_lib.ptr(points), _lib.ptr(normals), ln.ctypes.data, B, float(radius), int(max_nn), _lib.ptr(out["features"]),
                       _lib.ptr(spfh), _lib.ptr(cnt), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points.device))
    if want_spfh:
        out["spfh"] = spfh
    if want_count:
        out["count"] = cnt
    return out


SCAN_OVERLAP_MAX_CLOUDS = 64   # clouds per lcr_range_images / lcr_scan_overlap call
SCAN_OVERLAP_PROJ = dict(H=64, W=900, fov_up=3.0, fov_down=-25.0, max_range=50.0)    # the 64-beam defaults of include/lcr_hip.h


def _scan_clouds(who, points, lengths):
    _lib.require_cuda(points)
    ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32 or points.shape[0] != int(ln.sum()):
        raise ValueError("%s: points must be float32 [sum(lengths), 3]" % who)
    return points.contiguous(), ln


def range_images(points, lengths, H=64, W=900, fov_up=3.0, fov_down=-25.0, max_range=50.0):
    """Spherical range images (include/lcr_hip.h, lcr_range_images) of B <= 64 clouds in one native call: points f32 [N,3] on the device
    stacked cloud-major, lengths host ints [B] -> (images f32 [B,H,W] with -1 in empty pixels, valid int32 [B]).  Asynchronous on the
    current stream."""
    points, ln = _scan_clouds("range_images", points, lengths)
    dev, B = points.device, len(ln)
    ws = _lib.ws("lcr_range_images_ws_bytes", B, device=dev)
    images = torch.empty((B, int(H), int(W)), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.call.lcr_range_images(_lib.ptr(points), ln.ctypes.data, B, int(H), int(W), float(fov_up), float(fov_down), float(max_range),
                               _lib.ptr(images), _lib.ptr(valid), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points.device))
    return images, valid


def scan_overlap(points, lengths, images, valid, pairs, rel, H=64, W=900, fov_up=3.0, fov_down=-25.0, max_range=50.0, eps=1.0):
    """Range-image overlap counts (include/lcr_hip.h, lcr_scan_overlap) of P pairs of the B <= 64 clouds in one native call: images / valid
    as range_images returned them for the same clouds and projection, pairs int32 [P,2] (i, j) and rel f64 [P,3,4] = inv(T_i) T_j on the
    device -> (counts int32 [P,3] = (matches, valid_cur, valid_ref), status int32 [1]: 0, or p + 1 of a pair with an index outside
    0..B-1, whose counts are -1).  Raw form: asynchronous on the current stream, the status is not read here."""
    points, ln = _scan_clouds("scan_overlap", points, lengths)
    dev, B = points.device, len(ln)
    _lib.require_cuda(images, valid, pairs, rel)
    if tuple(images.shape) != (B, int(H), int(W)) or images.dtype != torch.float32 or tuple(valid.shape) != (B,) or valid.dtype != torch.int32:
        raise ValueError("scan_overlap: images must be float32 [B,H,W] and valid int32 [B]")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32:
        raise ValueError("scan_overlap: pairs must be int32 [P,2]")
    P = pairs.shape[0]
    if tuple(rel.shape) != (P, 3, 4) or rel.dtype != torch.float64:
        raise ValueError("scan_overlap: rel must be float64 [P,3,4]")
    images, valid, pairs, rel = images.contiguous(), valid.contiguous(), pairs.contiguous(), rel.contiguous()
    counts = torch.empty((P, 3), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = _lib.ws("lcr_scan_overlap_ws_bytes", B, P, device=dev)
    _lib.call.lcr_scan_overlap(_lib.ptr(points), ln.ctypes.data, B, _lib.ptr(images), _lib.ptr(valid), _lib.ptr(pairs), _lib.ptr(rel), P,
                               int(H), int(W), float(fov_up), float(fov_down), float(max_range), float(eps), _lib.ptr(counts),
                               _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(points.device))
    return counts, status


SCAN_CONTEXT_MAX_CLOUDS = 64   # clouds per lcr_scan_context call
SCAN_CONTEXT_PARAMS = dict(R=20, W=60, max_length=80.0, lidar_height=2.0)    # the defaults of include/lcr_hip.h
SCAN_CONTEXT_MAX_K = 128


def scan_context(points, lengths, R=20, W=60, max_length=80.0, lidar_height=2.0):
    """Scan Context descriptors (include/lcr_hip.h, lcr_scan_context) of B <= 64 clouds in one native call: points f32 [N,3] on the device
    stacked cloud-major, lengths host ints [B] -> (desc f32 [B,R,W], ring_key f32 [B,R], unit f32 [B,R,W], mask int64 [B] holding the
    u64 column bits).  Asynchronous on the current stream."""
    points, ln = _scan_clouds("scan_context", points, lengths)
    dev, B, R, W = points.device, len(ln), int(R), int(W)
    ws = _lib.ws("lcr_scan_context_ws_bytes", B, R, W, device=dev)
    desc = torch.empty((B, R, W), dtype=torch.float32, device=dev)
    ring_key = torch.empty((B, R), dtype=torch.float32, device=dev)
    unit = torch.empty((B, R, W), dtype=torch.float32, device=dev)
    mask = torch.empty((B,), dtype=torch.int64, device=dev)
    _lib.call.lcr_scan_context(_lib.ptr(points), ln.ctypes.data, B, R, W, float(max_length), float(lidar_height), _lib.ptr(desc),
                               _lib.ptr(ring_key), _lib.ptr(unit), _lib.ptr(mask), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return desc, ring_key, unit, mask


def _scan_context_db(who, unit, mask):
    _lib.require_cuda(unit, mask)
    if unit.dim() != 3 or unit.dtype != torch.float32 or mask.dtype != torch.int64 or tuple(mask.shape) != (unit.shape[0],):
        raise ValueError("%s: unit must be float32 [B,R,W] and mask int64 [B]" % who)
    return unit.contiguous(), mask.contiguous()


def scan_context_distance(unit, mask, pairs):
    """Scan Context distances (include/lcr_hip.h, lcr_scan_context_distance) of P pairs of the B descriptors: unit / mask as scan_context
    returned them, pairs int32 [P,2] (i, j) on the device -> (dist f32 [P], shift int32 [P], status int32 [1]: 0, or p + 1 of a pair with
    an index outside 0..B-1, whose result is (NaN, -1)).  Raw form: asynchronous on the current stream, the status is not read here."""
    unit, mask = _scan_context_db("scan_context_distance", unit, mask)
    _lib.require_cuda(pairs)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int32:
        raise ValueError("scan_context_distance: pairs must be int32 [P,2]")
    pairs = pairs.contiguous()
    dev, (B, R, W), P = unit.device, unit.shape, pairs.shape[0]
    dist = torch.empty((P,), dtype=torch.float32, device=dev)
    shift = torch.empty((P,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    _lib.call.lcr_scan_context_distance(_lib.ptr(unit), _lib.ptr(mask), B, R, W, _lib.ptr(pairs), P, _lib.ptr(dist), _lib.ptr(shift),
                                        _lib.ptr(status), None, 0, _lib.stream_ptr(dev))
    return dist, shift, status


def scan_context_topk(unit, mask, q0, Q, k, exclude):
    """The exhaustive causal Scan Context search (include/lcr_hip.h, lcr_scan_context_topk): query row r is frame q0 + r of unit f32
    [C,R,W] / mask int64 [C] and sees frames [0, q0 + r - exclude) -> (idx int32 [Q,k], dist f32 [Q,k], shift int32 [Q,k]), rows ascending
    in (dist, index), padded with (-1, +inf, -1).  Asynchronous on the current stream."""
    unit, mask = _scan_context_db("scan_context_topk", unit, mask)
    dev, (C, R, W), Q, k = unit.device, unit.shape, int(Q), int(k)
    ws = _lib.ws("lcr_scan_context_topk_ws_bytes", Q, int(q0), C, int(exclude), device=dev)
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
    shift = torch.empty((Q, k), dtype=torch.int32, device=dev)
    _lib.call.lcr_scan_context_topk(_lib.ptr(unit), _lib.ptr(mask), C, R, W, Q, int(q0), k, int(exclude), _lib.ptr(idx), _lib.ptr(dist),
                                    _lib.ptr(shift), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return idx, dist, shift


# ------------------------------------------------------------------------------------------------ registration loss terms
class GapGeometry:
    """The slice tables of lcr_gap_loss (include/lcr_hip.h) for B score slices of (n_b + 1) x (m_b + 1) grouped into pairs: n, m = host
    lists of the slices' inner sizes, seg = the host list [P+1] of every pair's first slice.  Device tables are built once per object."""

    def __init__(self, n, m, seg, device):
        n, m, seg = np.asarray(n, dtype=np.int64).reshape(-1), np.asarray(m, dtype=np.int64).reshape(-1), np.asarray(seg, dtype=np.int64)
        if len(n) != len(m) or len(n) < 1 or len(seg) < 2 or seg[0] != 0 or seg[-1] != len(n) or (np.diff(seg) < 1).any() or (n < 0).any() \
                or (m < 0).any():
            raise ValueError("GapGeometry: n and m per slice (>= 0), seg = [P+1] increasing slice offsets from 0 to B")
        self.B, self.P, self.device = len(n), len(seg) - 1, device
        self.n, self.m, self.seg = n, m, seg
        pre = lambda x: np.concatenate([[0], np.cumsum(x)])
        self.soff_h, self.roff_h, self.coff_h = pre((n + 1) * (m + 1)), pre(n), pre(m)
        self.elems, self.rows, self.cols = int(self.soff_h[-1]), int(self.roff_h[-1]), int(self.coff_h[-1])
        self.n_max, self.m_max = int(n.max()), int(m.max())
        tab = host_values(np.stack([self.soff_h, self.roff_h, self.coff_h]), torch.int64, device)
        self.soff, self.roff, self.coff = tab[0], tab[1], tab[2]
        self.seg_start = host_values(seg, torch.int32, device)

    @classmethod
    def uniform(cls, B, N, M, device, seg=None):
        return cls([N] * B, [M] * B, [0, B] if seg is None else seg, device)


def _gap_u8(t, n, what):
    if t is None or t.numel() != n:
        raise ValueError("gap_loss: %s must have %d entries" % (what, n))
    return (t.to(torch.uint8) if t.dtype != torch.uint8 else t).contiguous().view(-1)


def gap_loss(scores, geom, gamma, pmask, qmask, points=None, overlaps=None, out=None, ws=None):
    """lcr_gap_loss (include/lcr_hip.h): scores f32 [geom.elems] (the slices back to back), pmask [rows], qmask [cols] and ONE label source:
    points = (p_pts f32 [rows,3], q_pts f32 [cols,3], transforms f32 [P,4,4], positive_radius) or
    overlaps = (corr int64 [C,2], overlap f32 [C], counts: host list of the pairs' entry counts, positive_overlap).
    -> dict: terms f32 [P,3] (row term, column term, mean), kept int32 [P,2], labels uint8 [elems], line_pos / line_hinge f64 and
    line_count / line_active int32 [rows + cols], status int32 [1] (not read here: no host synchronisation).  out / ws: caller-owned
    buffers under the same names."""
    if (points is None) == (overlaps is None):
        raise ValueError("gap_loss: exactly one of points / overlaps")
    _lib.require_cuda(scores, pmask, qmask)
    dev, g = scores.device, geom
    if scores.dtype != torch.float32 or scores.numel() != g.elems:
        raise ValueError("gap_loss: scores must be float32 with %d elements" % g.elems)
    scores = scores.contiguous().view(-1)
    pm, qm = _gap_u8(pmask, g.rows, "pmask"), _gap_u8(qmask, g.cols, "qmask")
    null = None
    pp = qp = T = corr = ov = cstart = null
    radius = thr = 0.0
    C = c_max = 0
    if points is not None:
        pp, qp, T, radius = points
        _lib.require_cuda(pp, qp, T)
        if pp.dtype != torch.float32 or qp.dtype != torch.float32 or T.dtype != torch.float32 or pp.numel() != 3 * g.rows \
                or qp.numel() != 3 * g.cols or T.numel() != 16 * g.P:
            raise ValueError("gap_loss: points f32 [rows,3] / [cols,3] and one f32 4x4 transform per pair")
        pp, qp, T = pp.contiguous(), qp.contiguous(), T.contiguous()
        source = 0
    else:
        corr, ov, counts, thr = overlaps
        _lib.require_cuda(corr, ov)
        counts = [int(c) for c in counts]
        C = corr.shape[0]
        if corr.dtype != torch.int64 or corr.dim() != 2 or corr.shape[1] != 2 or ov.dtype != torch.float32 or ov.numel() != C \
                or len(counts) != g.P or sum(counts) != C:
            raise ValueError("gap_loss: corr int64 [C,2], overlap f32 [C], one entry count per pair summing to C")
        corr, ov = corr.contiguous(), ov.contiguous()
        cstart = host_values(np.concatenate([[0], np.cumsum(counts)]), torch.int32, dev)
        c_max = max(counts)
        source = 1
    out = {} if out is None else out
    lines = g.rows + g.cols
    for name, shape, dt in (("terms", (g.P, 3), torch.float32), ("kept", (g.P, 2), torch.int32), ("labels", (g.elems,), torch.uint8),
                            ("line_pos", (lines,), torch.float64), ("line_hinge", (lines,), torch.float64),
                            ("line_count", (lines,), torch.int32), ("line_active", (lines,), torch.int32), ("status", (1,), torch.int32)):
        if name not in out:
            out[name] = torch.empty(shape, dtype=dt, device=dev)
    if ws is None:
        ws = _lib.ws("lcr_gap_loss_ws_bytes", g.rows, g.cols, device=dev)
    P = _lib.ptr
    _lib.call.lcr_gap_loss(P(scores), P(g.soff), P(g.roff), P(g.coff), P(g.seg_start), g.B, g.P, g.n_max, g.m_max, g.elems, g.rows, g.cols,
                           source, P(pp), P(qp), P(T), float(radius), P(corr), P(ov), P(cstart), C, c_max, float(thr), P(pm), P(qm),
                           float(gamma), P(out["terms"]), P(out["kept"]), P(out["labels"]), P(out["line_pos"]), P(out["line_hinge"]),
                           P(out["line_count"]), P(out["line_active"]), P(out["status"]), P(ws), ws.numel(), _lib.stream_ptr(scores.device))
    return out


def gap_loss_grad(scores, geom, gamma, saved, upstream, dS=None):
    """lcr_gap_loss_grad: saved = what gap_loss returned for the same scores, upstream f32 [P,2] (d loss / d row term, d column term)
    -> dS f32 [geom.elems], every element written once."""
    g = geom
    _lib.require_cuda(scores, upstream)
    if scores.dtype != torch.float32 or scores.numel() != g.elems or upstream.dtype != torch.float32 or upstream.numel() != 2 * g.P:
        raise ValueError("gap_loss_grad: scores f32 [elems], upstream f32 [P,2]")
    scores, upstream = scores.contiguous().view(-1), upstream.contiguous()
    dS = torch.empty((g.elems,), dtype=torch.float32, device=scores.device) if dS is None else dS
    P = _lib.ptr
    _lib.call.lcr_gap_loss_grad(P(scores), P(g.soff), P(g.roff), P(g.coff), P(g.seg_start), g.B, g.P, g.n_max, g.m_max, g.elems, g.rows,
                                g.cols, float(gamma), P(upstream), P(saved["kept"]), P(saved["labels"]), P(saved["line_pos"]),
                                P(saved["line_hinge"]), P(saved["line_count"]), P(saved["line_active"]), P(dS), _lib.stream_ptr(scores.device))
    return dS


def _md_args(who, A, D, a_counts, d_counts, valid):
    _lib.require_cuda(A, D, valid)
    a_counts, d_counts = [int(c) for c in a_counts], [int(c) for c in d_counts]
    if A.dtype != torch.float32 or D.dtype != torch.float32 or A.dim() != 2 or D.dim() != 2 or A.shape[1] != 3 or D.shape[1] != 3:
        raise ValueError("%s: A [na,3] and D [nd,3] must be float32" % who)
    if len(a_counts) != len(d_counts) or len(a_counts) < 1 or sum(a_counts) != A.shape[0] or sum(d_counts) != D.shape[0]:
        raise ValueError("%s: one query count and one data count per segment, summing to the stacked rows" % who)
    if valid is not None:
        if valid.numel() != A.shape[0]:
            raise ValueError("%s: valid must have one entry per query" % who)
        valid = (valid.to(torch.uint8) if valid.dtype != torch.uint8 else valid).contiguous().view(-1)
    return a_counts, d_counts, valid


def min_dist(A, D, a_counts, d_counts, valid=None, starts=None, out=None):
    """lcr_min_dist (include/lcr_hip.h): stacked queries A f32 [na,3] against stacked data D f32 [nd,3] in P segments given by the host
    lists a_counts / d_counts -> dict: dist f32 [na], arg int32 [na] (segment-local, lower row on a tie), mean f32 [P] over the queries
    with valid != 0, count int32 [P], and the device offset tables a_start / d_start for min_dist_grad.  out: caller-owned buffers under the same names."""
    a_counts, d_counts, valid = _md_args("min_dist", A, D, a_counts, d_counts, valid)
    dev, P_ = A.device, len(a_counts)
    A, D = A.contiguous(), D.contiguous()
    if starts is None:
        tab = host_values(np.stack([np.concatenate([[0], np.cumsum(a_counts)]), np.concatenate([[0], np.cumsum(d_counts)])]), torch.int32, dev)
        starts = (tab[0], tab[1])
    out = {} if out is None else out
    for name, shape, dt in (("dist", (A.shape[0],), torch.float32), ("arg", (A.shape[0],), torch.int32), ("mean", (P_,), torch.float32),
                            ("count", (P_,), torch.int32)):
        if name not in out:
            out[name] = torch.empty(shape, dtype=dt, device=dev)
    out.update({"a_start": starts[0], "d_start": starts[1], "valid": valid})
    P = _lib.ptr
    _lib.call.lcr_min_dist(P(A), P(starts[0]), A.shape[0], P(D), P(starts[1]), D.shape[0], P(valid), P_, max(a_counts), P(out["dist"]),
                           P(out["arg"]), P(out["mean"]), P(out["count"]), _lib.stream_ptr(A.device))
    return out


def min_dist_grad(A, D, a_counts, d_counts, saved, upstream, dA=None):
    """lcr_min_dist_grad: saved = what min_dist returned for the same inputs, upstream f32 [P] -> dA f32 [na,3]."""
    a_counts, d_counts, _ = _md_args("min_dist_grad", A, D, a_counts, d_counts, None)
    _lib.require_cuda(upstream)
    if upstream.dtype != torch.float32 or upstream.numel() != len(a_counts):
        raise ValueError("min_dist_grad: upstream must be float32 [P]")
    A, D, upstream = A.contiguous(), D.contiguous(), upstream.contiguous()
    dA = torch.empty_like(A) if dA is None else dA
    P = _lib.ptr
    _lib.call.lcr_min_dist_grad(P(A), P(saved["a_start"]), A.shape[0], P(D), P(saved["d_start"]), D.shape[0], P(saved["valid"]), len(a_counts),
                                max(a_counts), P(saved["arg"]), P(saved["dist"]), P(saved["count"]), P(upstream), P(dA), _lib.stream_ptr(A.device))
    return dA


# ------------------------------------------------------------------------------------------------ Adan optimiser step
class AdanHyper(ctypes.Structure):
    """LcrAdanHyper (include/lcr_hip.h)."""
    _fields_ = [(k, ctypes.c_double) for k in ("beta1", "beta2", "beta3", "bias1", "bias2", "bias3_sqrt", "lr", "weight_decay", "eps")] + \
               [("no_prox", ctypes.c_int32), ("pad", ctypes.c_int32)]


ADAN_TENSOR_WORDS = 8       # LcrAdanTensor as int64 words: p, g, m, n, d, pg, numel, fresh (low half; the high half is padding)


def adan_table(params, grads, exp_avgs, exp_avg_sqs, exp_avg_diffs, pre_grads, fresh):
    """The HOST LcrAdanTensor array of lcr_adan_grad_norm / lcr_adan_step as an int64 array [T, 8].  The tensors must be CUDA, float32
    and contiguous (checked by the caller: lcrnet_amd.adan); the table holds raw pointers, so it is only good while they live."""
    T = len(grads)
    tab = np.zeros((T, ADAN_TENSOR_WORDS), dtype=np.int64)
    for col, ts in enumerate((params, grads, exp_avgs, exp_avg_sqs, exp_avg_diffs, pre_grads)):
        if ts is not None:
            tab[:, col] = [t.data_ptr() for t in ts]
    tab[:, 6] = [t.numel() for t in grads]
    if fresh is not None:
        tab[:, 7] = fresh
    return tab


def adan_ws_bytes(table):
    return _lib.ws_size("lcr_adan_ws_bytes", table.ctypes.data, len(table))


def adan_grad_norm(table, max_grad_norm, eps, device, norm_clip=None, ws=None):
    """lcr_adan_grad_norm over the gradients of `table` (adan_table; only g and numel are read) -> norm_clip f32 [2] on the device:
    the global L2 norm and min(max_grad_norm / (norm + eps), 1).  No host synchronisation."""
    if norm_clip is None:
        norm_clip = torch.empty(2, dtype=torch.float32, device=device)
    if ws is None:
        ws = _lib.workspace(adan_ws_bytes(table), device)
    _lib.call.lcr_adan_grad_norm(table.ctypes.data, len(table), float(max_grad_norm), float(eps), _lib.ptr(norm_clip), _lib.ptr(ws),
                                 ws.numel() * ws.element_size(), _lib.stream_ptr(device))
    return norm_clip


def adan_step(table, hyper, clip, device):
    """lcr_adan_step: one fused pass over the tensors of `table` (adan_table); hyper = AdanHyper, clip = a device float32 tensor of one
    element (the second entry of adan_grad_norm's result) or None.  No host synchronisation."""
    _lib.call.lcr_adan_step(table.ctypes.data, len(table), ctypes.addressof(hyper), _lib.ptr(clip), _lib.stream_ptr(device))


AUGMENT_MAX_CLOUDS = 128   # clouds per lcr_augment_clouds call (AUG_MAX_B in csrc/augment.hip)


def augment_clouds(rows, lengths, sample_id, rotation, scale, shift, noise, seed, limit=0):
    """Training augmentation and point-limit sampling (include/lcr_hip.h, lcr_augment_clouds) of B <= 128 stacked clouds in one native
    call: rows f32 [N, C] on the device (C = 3 .. 64, x, y, z first: an [N,4] xyzi scan as it lies), lengths host ints [B]; per cloud, host
    arrays (any float type, narrowed to fp32) sample_id [B], rotation [B,3,3], scale [B], shift [B,3], noise [B]; a 64-bit seed;
    limit <= 0 = no point limit -> (points f32 [M,3], lengths i64 [B]) on the device, M = sum(min(L, limit)).  The host knows every
    length, so a limit that cuts no cloud is passed as 0 (no sort is launched) and nothing is read back: the per-cloud values travel in
    one pinned upload and the call is asynchronous on the current stream."""
    _lib.require_cuda(rows)
    if rows.dim() != 2 or not 3 <= rows.shape[1] <= 64 or rows.dtype != torch.float32:
        raise ValueError("augment_clouds: rows must be float32 [N, C] with 3 <= C <= 64 (x, y, z first)")
    ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    B, n = len(ln), int(rows.shape[0])
    if not 1 <= B <= AUGMENT_MAX_CLOUDS:
        raise ValueError("augment_clouds: %d clouds (1 .. %d per call)" % (B, AUGMENT_MAX_CLOUDS))
    if (ln < 0).any() or int(ln.sum()) != n:
        raise ValueError("augment_clouds: lengths must be non-negative and sum to the number of rows")
    limit = int(limit) if limit is not None else 0
    out_ln = np.minimum(ln, limit) if limit > 0 else ln
    if limit > 0 and int(ln.max()) <= limit:
        limit = 0
    m = int(out_ln.sum())
    # one host record -> one asynchronous upload: [len i64 B | sample_id u32 B | rotation f32 9B | scale B | shift 3B | noise B]
    fields = [(ln, np.int64, B), (sample_id, np.uint32, B), (rotation, np.float32, 9 * B), (scale, np.float32, B), (shift, np.float32, 3 * B),
              (noise, np.float32, B)]
    host = torch.empty(8 * B + 4 * 16 * B, dtype=torch.uint8).pin_memory()
    hv, offs, o = host.numpy(), [], 0
    for value, dtype, count in fields:
        a = np.ascontiguousarray(np.asarray(value).astype(dtype, copy=False).reshape(-1))
        if a.size != count:
            raise ValueError("augment_clouds: a per-cloud argument has %d values, %d expected" % (a.size, count))
        nbytes = count * a.itemsize
        hv[o:o + nbytes] = a.view(np.uint8)
        offs.append(o)
        o += nbytes
    dev = rows.device
    rec = host.to(dev, non_blocking=True)
    base = rec.data_ptr()
    rows = rows.contiguous()
    out = torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_len = torch.empty((B,), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _lib.ws("lcr_augment_clouds_ws_bytes", n, B, limit, device=dev)
    _lib.call.lcr_augment_clouds(_lib.ptr(rows), int(rows.shape[1]), base + offs[0], B, n, base + offs[1], base + offs[2], base + offs[3],
                                 base + offs[4], base + offs[5], int(seed) & 0xFFFFFFFFFFFFFFFF, limit, _lib.ptr(out), m, _lib.ptr(out_len),
                                 _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return out, out_len
