"""GPU: training the pair model — lcr_patch_scores_grad (csrc/patch_scores.hip), the Python layer over it (functional._PatchTransportFn, the
graphs of bmm_nt and gemm(trans_b)), the matching head of the training branch on fixed tables, and LCRNet_Matching.train() end to end.

Tolerance throughout: encoder_grad_restatement.bound(e_ref, scale) = max(4 e_ref, 2^-20 scale), e_ref being the error of fp32 torch autograd
of the same formula against fp64 on the same input (computed here on the CPU), scale the largest fp64 entry (for an alpha: the sum of |dS|
over its dustbin entries, as in tests/test_sinkhorn_grad_gpu.py — it is a long sum with cancellation).  Exact: rows nobody lists, the
untouched output when only one is asked for, P = 0, run-to-run bytes, a patch alone against the stack (pairwise disjoint idx), the forward
bytes of the graph path against the no-grad fused call.  Outputs and workspace are NaN-filled and sit between canaries.

On the parent commit the kernel tests fail for want of the entry point, the graph tests because bmm_nt carries no graph, the model tests with
"inference only"."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_grad_restatement as ER
import patch_scores_grad_restatement as R
import sinkhorn_grad_restatement as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
CANARY = 12345.0
K = 128
LCR_EARG = -1                # include/lcr_hip.h


# ------------------------------------------------------------------------------------------------ helpers
def guarded(shape):
    """(whole buffer, NaN-filled view of `shape` between two canary bands)"""
    n = int(math.prod(shape))
    t = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
    t[PAD:PAD + n].fill_(float("nan"))
    return t, t[PAD:PAD + n].view(*shape)


def intact(*ts):
    return all(bool((t[:PAD] == CANARY).all()) and bool((t[-PAD:] == CANARY).all()) for t in ts)


def same_bytes(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != torch.float32:
        return torch.equal(a, b)
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(label, got, g64, g32, scale=None):
    """print err / tol and err / e_ref, then hold `got` to ER.bound"""
    g64 = g64.double()
    err = float((got.double().cpu() - g64).abs().max())
    e_ref = float((g32.double() - g64).abs().max())
    scale = float(g64.abs().max()) if scale is None else scale
    tol = ER.bound(e_ref, scale)
    print("%-52s err %.3e  tol %.3e  err/tol %6.3f  err/e_ref %8.3f" % (label, err, tol, err / tol if tol > 0 else 0.0,
                                                                         err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))))
    assert torch.isfinite(got).all(), label + ": not finite"
    assert err <= tol, (label, err, tol)


def lib():
    from lcrnet_amd import _lib
    return _lib


def fn():
    from lcrnet_amd import functional
    return functional


def stream():
    return lib().stream_ptr(torch.device(DEV, 0))


# ------------------------------------------------------------------------------------------------ lcr_patch_scores_grad
def run_kernel(c, want_a=True, want_b=True, patches=None):
    """the entry on case c (or on its patches [lo, hi)) into guarded buffers -> (d_feats_a, d_feats_b) on the CPU"""
    L, F = lib(), fn()
    lo, hi = patches if patches is not None else (0, c.P)
    P = hi - lo
    dS, fa, fb = (t.to(DEV).contiguous() for t in (c.dS[lo:hi], c.fa, c.fb))
    ia, ib, ma, mb = (t[lo:hi].to(DEV).contiguous() for t in (c.ia, c.ib, c.ma8, c.mb8))
    ra, ea = F.neighbor_transpose(ia, c.Na) if want_a and P else (None, None)
    rb, eb = F.neighbor_transpose(ib, c.Nb) if want_b and P else (None, None)
    t_a, da = guarded((c.Na, c.C))
    t_b, db = guarded((c.Nb, c.C))
    nws = L.ws_size("lcr_patch_scores_grad_ws_bytes", P, K, c.C)
    assert nws == 4 * 2 * P * K * c.C
    t_w, ws = guarded((max(nws // 4, 4),))
    L.call.lcr_patch_scores_grad(L.ptr(dS), L.ptr(fa), c.Na, L.ptr(fb), c.Nb, c.C, L.ptr(ia), L.ptr(ib), L.ptr(ma), L.ptr(mb), P, K, c.scale,
                                 L.ptr(ra), L.ptr(ea), L.ptr(rb), L.ptr(eb), L.ptr(da if want_a else None), L.ptr(db if want_b else None),
                                 L.ptr(ws), nws, stream())
    torch.cuda.synchronize()
    assert intact(t_a, t_b, t_w), "a canary was overwritten"
    if not want_a:
        assert bool(torch.isnan(da).all()), "d_feats_a was written although it was not asked for"
    if not want_b:
        assert bool(torch.isnan(db).all()), "d_feats_b was written although it was not asked for"
    return da.cpu(), db.cpu()


CASES = {c.name: c for c in R.cases()}
_REF = {}


def reference(name):
    """(fp64 restatement, fp32 autograd of the dense formula) of a case, computed once"""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = (R.patch_scores_grad(*c.args(torch.float64)), R.autograd_grad(*c.args(), torch.float32))
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_matches_fp64(name):
    c = CASES[name]
    (a64, b64), (a32, b32) = reference(name)
    da, db = run_kernel(c)
    check(name + " d_feats_a", da, a64, a32)
    check(name + " d_feats_b", db, b64, b32)
    ua, ub = c.unlisted()
    assert int(ua.sum()) >= 1 and int(ub.sum()) >= 1
    assert bool((da[ua] == 0).all()) and bool((db[ub] == 0).all()), "a row nobody lists is exactly zero"
    # run-to-run bytes, and each output alone (the other stays NaN: run_kernel asserts it)
    da2, db2 = run_kernel(c)
    assert same_bytes(da, da2) and same_bytes(db, db2)
    assert same_bytes(run_kernel(c, want_b=False)[0], da) and same_bytes(run_kernel(c, want_a=False)[1], db)


def test_no_patches_gives_zeros():
    c = CASES["C32"]
    da, db = run_kernel(c, patches=(0, 0))
    assert bool((da == 0).all()) and bool((db == 0).all())
    L = lib()
    assert L.lib().lcr_patch_scores_grad(None, None, 0, None, 0, 32, None, None, None, None, 0, K, 1.0, None, None, None, None, None, None, None, 0,
                                         stream()) == 0


def test_a_patch_alone_equals_its_rows_in_the_stack():
    """pairwise disjoint idx: every row is listed by one slot, so a patch alone must give the bytes it gives inside the stack"""
    c = R.Case("disjoint", 2, 32, 300, 290, 21, disjoint=True)
    da, db = run_kernel(c)
    a64, b64 = R.patch_scores_grad(*c.args(torch.float64))
    a32, b32 = R.autograd_grad(*c.args(), torch.float32)
    check("disjoint d_feats_a", da, a64, a32)
    check("disjoint d_feats_b", db, b64, b32)
    for p in range(c.P):
        pa, pb = run_kernel(c, patches=(p, p + 1))
        rows_a, rows_b = c.ia[p][c.ia[p] < c.Na], c.ib[p][c.ib[p] < c.Nb]
        assert same_bytes(pa[rows_a], da[rows_a]) and same_bytes(pb[rows_b], db[rows_b])
        other_a = torch.ones(c.Na, dtype=torch.bool)
        other_a[rows_a] = False
        assert bool((pa[other_a] == 0).all())


def test_entry_refuses_outside_its_domain():
    L = lib()
    c = CASES["C32"]
    dS, fa, fb, ia, ib, ma, mb = (t.to(DEV).contiguous() for t in (torch.zeros(c.P, K + 1, K + 1), c.fa, c.fb, c.ia, c.ib, c.ma8, c.mb8))
    F = fn()
    ra, ea = F.neighbor_transpose(ia, c.Na)
    rb, eb = F.neighbor_transpose(ib, c.Nb)
    t_a, da = guarded((c.Na + 1, c.C))
    t_b, db = guarded((c.Nb, c.C))
    ws = torch.empty(2 * c.P * K * c.C + 4, dtype=torch.float32, device=DEV)

    def call(Kk=K, C=c.C, fa_=fa, da_=da, ws_=ws, nws=4 * 2 * c.P * K * c.C):
        return L.lib().lcr_patch_scores_grad(L.ptr(dS), L.ptr(fa_), c.Na, L.ptr(fb), c.Nb, C, L.ptr(ia), L.ptr(ib), L.ptr(ma), L.ptr(mb), c.P, Kk,
                                             c.scale, L.ptr(ra), L.ptr(ea), L.ptr(rb), L.ptr(eb), L.ptr(da_), L.ptr(db), L.ptr(ws_), nws, stream())
    unaligned = fa.new_zeros(fa.numel() + 1)[1:].view_as(fa)
    for what, kw in (("K", dict(Kk=64)), ("C", dict(C=48)), ("C small", dict(C=16)), ("features unaligned", dict(fa_=unaligned)),
                     ("gradient unaligned", dict(da_=da.view(-1)[1:1 + c.Na * c.C].view(c.Na, c.C))), ("workspace unaligned", dict(ws_=ws[1:])),
                     ("workspace short", dict(nws=4 * 2 * c.P * K * c.C - 4))):
        assert call(**kw) == LCR_EARG and L.lib().lcr_last_error().startswith(b"lcr_patch_scores_grad:"), what
    import ctypes
    n = ctypes.c_size_t(0)
    assert L.lib().lcr_patch_scores_grad_ws_bytes(3, 64, 32, ctypes.byref(n)) == LCR_EARG
    torch.cuda.synchronize()
    assert intact(t_a, t_b) and bool(torch.isnan(da).all()) and bool(torch.isnan(db).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ the Python layer
def dense_patch_transport(fa, ia, fb, ib, ma, mb, alpha, scale):
    """patch_log_optimal_transport on the CPU: gather on the zero-row-padded features, product, oracle transport"""
    from oracle import torch_ref
    pa = torch.cat([fa, fa.new_zeros(1, fa.shape[1])])[ia]
    pb = torch.cat([fb, fb.new_zeros(1, fb.shape[1])])[ib]
    return torch_ref.log_optimal_transport(torch.bmm(pa, pb.transpose(1, 2)) * scale, ma, mb, alpha, iters=100)


def valid_entries(ma, mb):
    P = ma.shape[0]
    V = torch.ones(P, ma.shape[1] + 1, mb.shape[1] + 1, dtype=torch.bool)
    V[:, :-1, :] &= ma[:, :, None]
    V[:, :, :-1] &= mb[:, None, :]
    return V


def dust_scale(raw64, ma, mb, alpha, scale, G):
    """sum |dS| over the dustbin row and column: the scale of d_alpha"""
    dS = SR.restate(raw64, ma, mb, torch.tensor(float(alpha)), scale, G, 100)[2]
    return float(dS[:, -1, :].abs().sum() + dS[:, :-1, -1].abs().sum())


def test_patch_transport_graph_on_one_feature_tensor():
    """feats_a is feats_b (the stack call of the model), C = 128: d_feats (both sides summed) and d_alpha against fp64 autograd through
    oracle/torch_ref.log_optimal_transport; the forward bytes are the no-grad fused call's"""
    F = fn()
    P, C, n = 2, 128, 210
    g = torch.Generator().manual_seed(31)
    f = torch.randn(n, C, generator=g) * 0.5
    ia, ib = torch.randint(0, n, (P, K), generator=g), torch.randint(0, n, (P, K), generator=g)
    ma, mb = torch.rand(P, K, generator=g) > 0.1, torch.rand(P, K, generator=g) > 0.1
    ma[:, 0] = mb[:, 0] = True
    ia[~ma], ib[~mb] = n, n
    V = valid_entries(ma, mb)
    G = torch.where(V, torch.randn(P, K + 1, K + 1, generator=g), torch.zeros(()))
    scale = 1.0 / C ** 0.5
    ref = {}
    for dt in (torch.float64, torch.float32):
        x, al = f.to(dt).clone().requires_grad_(), torch.tensor(0.7, dtype=dt).requires_grad_()
        (dense_patch_transport(x, ia, x, ib, ma, mb, al, scale) * G.to(dt)).sum().backward()
        ref[dt] = (x.grad.double(), al.grad.double())
    x = f.to(DEV).requires_grad_()
    al = torch.nn.Parameter(torch.tensor(0.7, device=DEV))
    dev = [t.to(DEV) for t in (ia, ib, ma, mb)]
    assert F.PATCH_SCORES_FUSED[0]
    with F.inverted_lists():
        out = F.patch_log_optimal_transport(x, dev[0], x, dev[1], dev[2], dev[3], al, scale=scale, iters=100)
    assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_PatchTransportFn")
    (out * G.to(DEV)).sum().backward()
    pa, pb = torch.cat([f, f.new_zeros(1, C)])[ia].double(), torch.cat([f, f.new_zeros(1, C)])[ib].double()
    check("patch transport d_feats (one tensor)", x.grad, ref[torch.float64][0], ref[torch.float32][0])
    check("patch transport d_alpha", al.grad, ref[torch.float64][1], ref[torch.float32][1],
          scale=dust_scale(torch.bmm(pa, pb.transpose(1, 2)), ma, mb, 0.7, scale, G))
    with torch.no_grad():
        fused = F.patch_log_optimal_transport(x, dev[0], x, dev[1], dev[2], dev[3], al, scale=scale, iters=100)
    assert fused.grad_fn is None and same_bytes(fused, out.detach()), "the graph path's forward is the no-grad fused call"


def test_products_carry_a_graph():
    """bmm_nt and gemm(trans_b): the smallest batch the GEMM takes with M, N off the tile size and M N not a multiple of 4 (K % 4 == 0 is the
    entry's own rule for its inputs): M = 67, N = 35 (M N = 2345), K = 8, two problems"""
    F = fn()
    P, M, N, Kd = 2, 67, 35, 8
    assert (M * N) % 4 and M % 64 and N % 64
    g = torch.Generator().manual_seed(41)
    a, b, G = torch.randn(P, M, Kd, generator=g), torch.randn(P, N, Kd, generator=g), torch.randn(P, M, N, generator=g)
    ref = {}
    for dt in (torch.float64, torch.float32):
        x, y = a.to(dt).clone().requires_grad_(), b.to(dt).clone().requires_grad_()
        (torch.bmm(x, y.transpose(1, 2)) * G.to(dt)).sum().backward()
        ref[dt] = (x.grad, y.grad)
    x, y = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    out = F.bmm_nt(x, y)
    assert out.grad_fn is not None
    with torch.no_grad():
        assert same_bytes(out.detach(), F.bmm_nt(x, y))
    (out * G.to(DEV)).sum().backward()
    check("bmm_nt d_a", x.grad, ref[torch.float64][0], ref[torch.float32][0])
    check("bmm_nt d_b", y.grad, ref[torch.float64][1], ref[torch.float32][1])
    x1 = a[0].to(DEV).requires_grad_()
    out = F.bmm_nt(x1[None], y.detach()[:1])                 # one factor alone
    (out * G[:1].to(DEV)).sum().backward()
    check("bmm_nt d_a alone", x1.grad, ref[torch.float64][0][0], ref[torch.float32][0][0])
    x, y = a[1].to(DEV).requires_grad_(), b[1].to(DEV).requires_grad_()
    out, stats = F.gemm(x, y, trans_b=True)
    assert out.grad_fn is not None and stats is None
    with torch.no_grad():
        assert same_bytes(out.detach(), F.gemm(x, y, trans_b=True)[0])
    (out * G[1].to(DEV)).sum().backward()
    check("gemm(trans_b) d_a", x.grad, ref[torch.float64][0][1], ref[torch.float32][0][1])
    check("gemm(trans_b) d_b", y.grad, ref[torch.float64][1][1], ref[torch.float32][1][1])


# ------------------------------------------------------------------------------------------------ the model
LIMITS = [24, 24, 24, 24]
# The smallest pair found on which the training branch has something to do at num_targets = 2: 420 points per cloud in a 14 x 14 x 1.2 m box
# (coarse voxels of 2.4 m: ~30 coarse points, of which the vote NMS keeps >= 2 nodes per cloud), the second cloud the first under a known
# motion (8 degrees about z, 0.4 / -0.3 / 0.05 m) plus 5 mm of noise — its part beyond x = 4.5 m only, so that some nodes of the first cloud
# have no counterpart (with every node matched the weighted BCE of node_overlap_Loss weighs every label by zero and the overlap score gets no
# gradient).  The seed was picked on the CPU through oracle/torch_ref (encoder,
# transformer, vote encoder, partition) and the package's torch labels; the test asserts the three conditions again on the device's values.
E2E = dict(seed=3, points=420, box=(14.0, 14.0, 1.2), cut=4.5, weights_seed=7351, noise=0.005, steps=5, lr=1e-3)


def pair_clouds(seed=None, pairs=1):
    """([pos_0, anc_0, pos_1, anc_1, ...] float32 arrays, [T_p (4, 4) anc -> pos])"""
    clouds, Ts = [], []
    for p in range(pairs):
        gen = torch.Generator().manual_seed(500 + 17 * p + (E2E["seed"] if seed is None else seed))
        pos = (torch.rand(E2E["points"] - 40 * p, 3, generator=gen) * torch.tensor(E2E["box"])).double()
        a = math.radians(8.0 + 3.0 * p)
        Rm = torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
        t = torch.tensor([0.4, -0.3, 0.05], dtype=torch.float64)
        part = pos[pos[:, 0] > E2E["cut"]]                                                            # the clouds overlap in part only
        anc = (part + E2E["noise"] * torch.randn(part.shape, generator=gen).double() - t) @ Rm        # R^T (x - t), row vectors
        T = torch.eye(4, dtype=torch.float64)
        T[:3, :3], T[:3, 3] = Rm, t
        clouds += [pos.float().numpy(), anc.float().numpy()]
        Ts.append(T.float())
    return clouds, Ts


def oracle_dict(clouds):
    from oracle import ops as oracle_ops
    st = oracle_ops.precompute_data_stack_mode(np.concatenate(clouds), np.array([len(c) for c in clouds], dtype=np.int64), 4, 0.3, 1.275, LIMITS)
    return {k: [torch.from_numpy(np.ascontiguousarray(t)) for t in v] for k, v in st.items()}


def make_model(num_targets=2):
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family.LCRNet_Matching import LCRNet_Matching
    from lcrnet_amd.weights import seeded_state_dict
    cfg = make_cfg()
    cfg["neighbor_limits"] = LIMITS
    cfg["coarse_matching"]["num_targets"] = num_targets
    m = LCRNet_Matching(cfg)
    m.load_state_dict(seeded_state_dict(m.state_dict(), E2E["weights_seed"]), strict=True)
    return m, cfg


def device_dict(pairs):
    from lcrnet_amd.data import precompute_batch
    clouds, Ts = pair_clouds(pairs=pairs)
    pts = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    d = precompute_batch(pts.contiguous(), torch.tensor([len(c) for c in clouds], device=DEV), 4, 0.3, 1.275, LIMITS)
    if pairs == 1:
        d.pop("segment_lengths", None)
    d["features"] = torch.ones(d["points"][0].shape[0], 1, device=DEV)
    d["transform"] = torch.stack(Ts).to(DEV)
    return d


_MODEL = {}


def model_on_device():
    if "m" not in _MODEL:
        m, cfg = make_model()
        _MODEL["m"], _MODEL["cfg"] = m.to(DEV), cfg
    return _MODEL["m"], _MODEL["cfg"]


def head_tables(P, seed):
    """fixed tables of the matching head for P pairs with unequal node counts: node features (32 channels), point features (64 channels),
    node masks (one node without points), per-node patch tables of K slots local to the cloud (pad = its point count), selected
    correspondences"""
    g = torch.Generator().manual_seed(seed)
    m = [5, 7, 6, 4][:2 * P]
    n_f = [150, 140, 130, 160][:2 * P]
    off_m, off_f = [0], [0]
    for x in m:
        off_m.append(off_m[-1] + x)
    for x in n_f:
        off_f.append(off_f[-1] + x)
    fc = torch.randn(off_m[-1], 32, generator=g) * 0.7       # scaled node scores of spread 0.5, the spread tests/test_sinkhorn_grad_gpu.py holds
                                                             # the transport's reverse pass to its bound at (see the docstring of the head test)
    ff = torch.randn(off_f[-1], 64, generator=g) * 0.7
    nm = torch.ones(off_m[-1], dtype=torch.bool)
    nm[1] = False
    knn, km = [], []
    for c in range(2 * P):
        k = torch.randint(0, n_f[c], (m[c], K), generator=g)
        msk = torch.rand(m[c], K, generator=g) > 0.15
        msk[:, 0] = True
        k[~msk] = n_f[c]
        knn.append(k)
        km.append(msk)
    sel = [(torch.tensor([0, 2, 4]), torch.tensor([1, 3, 6]), None), (torch.tensor([1, 5]), torch.tensor([0, 3]), None)][:P]
    pts = torch.randn(off_f[-1], 3, generator=g)
    return dict(P=P, m=m, n_f=n_f, off_m=off_m, off_f=off_f, fc=fc, ff=ff, nm=nm, knn=torch.cat(knn), km=torch.cat(km), sel=sel, pts=pts, gen=g)


def head_reference(t, Gn, Gm, dtype, alphas=(0.7, 0.9)):
    """the head by the dense formula on the CPU in `dtype` -> gradients of sum <scores, G> to (fc, ff, node alpha, patch alpha)"""
    from oracle import torch_ref
    P, off_m, off_f = t["P"], t["off_m"], t["off_f"]
    fc, ff = t["fc"].to(dtype).clone().requires_grad_(), t["ff"].to(dtype).clone().requires_grad_()
    an, ap = torch.tensor(alphas[0], dtype=dtype).requires_grad_(), torch.tensor(alphas[1], dtype=dtype).requires_grad_()
    loss = 0
    q = 0
    for p in range(P):
        c = 2 * p
        fp, fa = fc[off_m[c]:off_m[c + 1]], fc[off_m[c + 1]:off_m[c + 2]]
        ns = torch_ref.log_optimal_transport((fp @ fa.t() / fc.shape[1] ** 0.5)[None], t["nm"][off_m[c]:off_m[c + 1]][None],
                                             t["nm"][off_m[c + 1]:off_m[c + 2]][None], an, iters=100)[0]
        loss = loss + (ns * Gn[p].to(dtype)).sum()
        pi, ai, _ = t["sel"][p]
        kp, ka = t["knn"][off_m[c]:off_m[c + 1]][pi], t["knn"][off_m[c + 1]:off_m[c + 2]][ai]
        mp, ma = t["km"][off_m[c]:off_m[c + 1]][pi], t["km"][off_m[c + 1]:off_m[c + 2]][ai]
        ms = dense_patch_transport(ff[off_f[c]:off_f[c + 1]], kp, ff[off_f[c + 1]:off_f[c + 2]], ka, mp, ma, ap, 1.0 / ff.shape[1] ** 0.5)
        loss = loss + (ms * Gm[q:q + len(pi)].to(dtype)).sum()
        q += len(pi)
    loss.backward()
    return fc.grad, ff.grad, an.grad, ap.grad


@pytest.mark.parametrize("pairs", [1, 2])
def test_matching_head_on_fixed_tables(pairs):
    """leaf feats_c / feats_f, fixed masks, partition tables and selected correspondences (no decision in the graph): the gradients of
    sum <scores, G> over the node-level and the patch-level scores to both feature tensors and both alphas, against the fp64 dense formula —
    one pair, and two pairs with unequal node counts (the padded batch).

    The node features are drawn so that the scaled node scores have spread 0.5, the spread at which tests/test_sinkhorn_grad_gpu.py holds
    lcr_log_sinkhorn_grad to this bound ("tiny": 5 x 9, normal x 0.5).  Measured with unit-variance features (spread 1) on the 5 x 7 problem
    of the one-pair case: the transport's own d_raw is 1.9e-6 off its fp64 restatement, 5.35 x ITS bound (fp32 torch autograd is 5e-8 off
    there, so the 2^-20 floor carries the bound), and d_feats_c, which sums 7 such entries times a feature, was 5.2e-6 off against a bound
    of 1.7e-6.  That is the precision of the existing transport kernel on a sharper tiny problem, not of the chain this test is about; it is
    recorded in LABNOTES R18.1."""
    model, _ = model_on_device()
    t = head_tables(pairs, 50 + pairs)
    P, m, off_m, off_f = t["P"], t["m"], t["off_m"], t["off_f"]
    g = t["gen"]
    Gn, Vn = [], []
    for p in range(P):
        V = valid_entries(t["nm"][off_m[2 * p]:off_m[2 * p + 1]][None], t["nm"][off_m[2 * p + 1]:off_m[2 * p + 2]][None])[0]
        Gn.append(torch.where(V, torch.randn(V.shape, generator=g), torch.zeros(())))
        Vn.append(V)
    mp = torch.cat([t["km"][off_m[2 * p]:off_m[2 * p + 1]][t["sel"][p][0]] for p in range(P)])
    ma = torch.cat([t["km"][off_m[2 * p + 1]:off_m[2 * p + 2]][t["sel"][p][1]] for p in range(P)])
    Gm = torch.where(valid_entries(mp, ma), torch.randn(mp.shape[0], K + 1, K + 1, generator=g), torch.zeros(()))
    r64, r32 = head_reference(t, Gn, Gm, torch.float64), head_reference(t, Gn, Gm, torch.float32)
    an0, ap0 = model.node_optimal_transport.alpha.detach().clone(), model.optimal_transport.alpha.detach().clone()
    try:
        with torch.no_grad():
            model.node_optimal_transport.alpha.fill_(0.7)
            model.optimal_transport.alpha.fill_(0.9)
        model.zero_grad()
        fc, ff = t["fc"].to(DEV).requires_grad_(), t["ff"].to(DEV).requires_grad_()
        sel = [(a.to(DEV), b.to(DEV), None) for a, b, _ in t["sel"]]
        mm, Mx, Nx, tab, ns = model._node_transport_padded(P, fc, t["nm"].to(DEV), off_f, off_m)
        assert mm == m and (P == 1 or (Mx, Nx) != (m[2], m[3]))
        q_off, pkp, akp, pkm, akm, ms = model._patch_transport_selected(P, t["pts"].to(DEV), ff, off_m, t["knn"].to(DEV), t["km"].to(DEV), tab, sel)
        assert q_off == [0, 3, 5][:P + 1] and torch.equal(pkm.cpu(), mp) and torch.equal(akm.cpu(), ma)
        loss = (ms * Gm.to(DEV)).sum()
        for p in range(P):
            loss = loss + (model._pair_node_scores(ns, p, m[2 * p], m[2 * p + 1], Mx, Nx) * Gn[p].to(DEV)).sum()
        loss.backward()
        # scales of the two alphas: the dustbin sums of |dS| of their transports
        dn = 0.0
        for p in range(P):
            c = 2 * p
            raw = (t["fc"][off_m[c]:off_m[c + 1]].double() @ t["fc"][off_m[c + 1]:off_m[c + 2]].double().t())[None]
            dn += dust_scale(raw, t["nm"][off_m[c]:off_m[c + 1]][None], t["nm"][off_m[c + 1]:off_m[c + 2]][None], 0.7, 1.0 / 32 ** 0.5, Gn[p][None])
        pad = torch.cat([t["ff"], t["ff"].new_zeros(1, 64)]).double()
        n_all = t["ff"].shape[0]
        gk = lambda c, rows: torch.where(t["knn"][off_m[c]:off_m[c + 1]][rows] == t["n_f"][c], torch.tensor(n_all),
                                         t["knn"][off_m[c]:off_m[c + 1]][rows] + off_f[c])
        ka = torch.cat([gk(2 * p, t["sel"][p][0]) for p in range(P)])
        kb = torch.cat([gk(2 * p + 1, t["sel"][p][1]) for p in range(P)])
        dp = dust_scale(torch.bmm(pad[ka], pad[kb].transpose(1, 2)), mp, ma, 0.9, 1.0 / 64 ** 0.5, Gm)
        tag = "head, %d pair(s): " % P
        check(tag + "d_feats_c", fc.grad, r64[0], r32[0])
        check(tag + "d_feats_f", ff.grad, r64[1], r32[1])
        check(tag + "d_alpha (nodes)", model.node_optimal_transport.alpha.grad, r64[2], r32[2], scale=dn)
        check(tag + "d_alpha (patches)", model.optimal_transport.alpha.grad, r64[3], r32[3], scale=dp)
    finally:
        with torch.no_grad():
            model.node_optimal_transport.alpha.copy_(an0)
            model.optimal_transport.alpha.copy_(ap0)
        model.zero_grad()


def eval_outputs(model, d):
    model.eval()
    with torch.no_grad():
        outs = model.forward_pairs(d)
    return [{k: v.detach().clone() for k, v in o.items() if torch.is_tensor(v)} for o in outs]


@pytest.mark.parametrize("pairs", [1, 2])
def test_pair_model_trains(pairs):
    from lcrnet_amd.losses import OverallLoss_new
    from lcrnet_amd.model_family import LCRNet
    model, cfg = model_on_device()
    d = device_dict(pairs)
    before = eval_outputs(model, d)
    crit = OverallLoss_new(cfg)
    model.train()
    model.zero_grad()
    model.coarse_target.reseed()
    outs = model.forward_pairs(d)
    assert len(outs) == pairs
    for p, o in enumerate(outs):
        n_pos, n_anc = o["pos_points_c"].shape[0], o["anc_points_c"].shape[0]
        above = int((o["gt_node_corr_overlaps"] > cfg["coarse_matching"]["overlap_threshold"]).sum())
        vp, va = o["mask"]
        print("pair %d: %d + %d voted nodes, %d ground-truth node correspondences above the threshold, vote mask %d + %d"
              % (p, n_pos, n_anc, above, int(vp.sum()), int(va.sum())))
        assert n_pos >= 2 and n_anc >= 2 and above >= 3 and int(vp.sum()) >= 1 and int(va.sum()) >= 1
        assert o["matching_scores"].shape == (2, K + 1, K + 1), "num_targets = 2 of >= 3: sampled"
        assert o["pos_emb"].requires_grad and o["anc_emb"].requires_grad and o["score"].requires_grad
        assert o["matching_scores"].requires_grad and o["node_matching_scores"].requires_grad and o["shifted_pos_points_c"].requires_grad
        assert "estimated_transform" not in o and "pos_corr_points" not in o, "no patch matching and no registration in training"
    losses = crit(outs, d)
    for ld in losses:
        assert all(bool(torch.isfinite(v).all()) for v in ld.values()), ld
    sum(ld["loss"] for ld in losses).backward()
    named = dict(model.named_parameters())
    for k, prm in named.items():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), k
    first_kpconv = next(k for k in named if k.startswith("encoder.") and k.endswith("KPConv.weights"))
    for k in [first_kpconv, "proj_node_overlap_score.weight", "node_optimal_transport.alpha", "optimal_transport.alpha"] + \
            [k for k in named if k.startswith("transformer.") and k.endswith("weight")][:3]:
        assert bool((named[k].grad != 0).any()), k + ": the gradient is all zero"
    # a repeated step with the generator reseeded is the same step; eval mode is untouched by the training call
    model.coarse_target.reseed()
    again = model.forward_pairs(d)
    assert all(torch.equal(a["pos_node_corr_indices"], o["pos_node_corr_indices"]) for a, o in zip(again, outs))
    after = eval_outputs(model, d)
    for b, a in zip(before, after):
        assert b.keys() == a.keys() and all(same_bytes(b[k], a[k]) for k in b), "eval mode changed"
    model.zero_grad()
    with pytest.raises(RuntimeError, match="inference only"):
        LCRNet.forward_pairs(model.train(), d)
    model.eval()


def test_five_adan_steps_lower_the_loss():
    """five fused Adan steps on the fixed pair, the target generator reseeded before each: the loss falls.

    The step size, found by a sweep on the device (the run repeats to the digit): the loss is not smooth in the weights here — a vote that
    crosses the NMS radius changes the node set — so even lr 1e-6 wanders by +-0.3 (6.558 6.532 6.288 6.274 6.604) and the trainer's own 1e-4
    (config optimadan.lr) ends only 0.48 lower (6.558 7.036 7.069 5.893 6.080); 3e-5 and 1e-5 end higher than they start (6.730, 7.382),
    3e-4 ends at 5.056.  At 1e-3 the fall is well clear of that wander: 6.558 8.841 6.137 4.731 3.688 (Adan's first update moves every
    weight by lr * sign(g), hence the first step up)."""
    from lcrnet_amd.adan import Adan
    from lcrnet_amd.losses import OverallLoss_new
    m, cfg = make_model()
    model = m.to(DEV).train()
    d = device_dict(1)
    crit = OverallLoss_new(cfg)
    opt = Adan(model.parameters(), lr=E2E["lr"], fused=True)
    losses = []
    for _ in range(E2E["steps"]):
        model.coarse_target.reseed()
        loss = crit(model.forward_pairs(d), d)[0]["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print("losses: " + " ".join("%.6f" % v for v in losses))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


def test_a_pair_without_correspondences_raises():
    model, cfg = model_on_device()
    d = device_dict(1)
    T = d["transform"].clone()
    T[0, :3, 3] += 500.0                                     # the clouds no longer meet: no node correspondence at all
    d["transform"] = T
    model.train()
    try:
        with pytest.raises(RuntimeError, match="no ground-truth node correspondence"):
            model.forward_pairs(d)
    finally:
        model.eval()
