"""GPU: the descriptor head in training mode and its reverse pass (csrc/netvlad.hip, csrc/netvlad_grad.hip behind lcrnet_amd.functional.netvlad_train /
netvlad_backward, NetVLADLoupe2.describe and LCRNet_GlobalDescrition.forward) against the fp64 restatement of
tests/netvlad_grad_restatement.py, the reference's own numbers (tests/golden/netvlad_grad_golden.npz) and a CPU training run.

Tolerances.  `out` within 1e-4 of fp64 (the project's descriptor bound).  Every gradient tensor, dx and every running buffer:
max|got - g64| <= max(4 e_ref, 2^-20 max|g64|), e_ref = the error of fp32 torch autograd of the reference's padded formula on the same input,
computed here on the CPU (R.bound).  Outputs, the saved buffer and the workspaces are NaN-filled before every call and sit between canaries.

On the parent commit every test of this file fails: the kernel tests for want of the entry points, the module tests because training mode
raises "inference only"."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netvlad_grad_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
CANARY = 12345.0
_W = {"cluster_weights": "cluster_weights", "cluster_weights2": "cluster_weights2", "hidden1_weights": "hidden1_weights",
      "bn1_w": "bn1.weight", "bn1_b": "bn1.bias", "bn1_mean": "bn1.running_mean", "bn1_var": "bn1.running_var",
      "bn2_w": "bn2.weight", "bn2_b": "bn2.bias", "bn2_mean": "bn2.running_mean", "bn2_var": "bn2.running_var",
      "gating_weights": "context_gating.gating_weights", "gbn_w": "context_gating.bn1.weight", "gbn_b": "context_gating.bn1.bias",
      "gbn_mean": "context_gating.bn1.running_mean", "gbn_var": "context_gating.bn1.running_var"}
C2P = dict(zip(R.C_NAMES, R.PARAMS))
SHAPES = {"cluster_weights": (1024, 64), "cluster_weights2": (1, 1024, 64), "hidden1_weights": (65536, 256), "bn1_w": (64,), "bn1_b": (64,),
          "bn2_w": (256,), "bn2_b": (256,), "gating_weights": (256, 256), "gbn_w": (256,), "gbn_b": (256,)}


# ------------------------------------------------------------------------------------------------ helpers
def guarded(shape):
    n = int(math.prod(shape))
    t = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device=DEV)
    t[PAD:PAD + n].fill_(float("nan"))
    return t, t[PAD:PAD + n].view(*shape)


def intact(ts):
    return all(bool((t[:PAD] == CANARY).all()) and bool((t[-PAD:] == CANARY).all()) for t in ts)


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def lib():
    from lcrnet_amd import _lib
    return _lib


def fn():
    from lcrnet_amd import functional as F
    return F


_DEV_WEIGHTS = {}


def dev_weights():
    """(struct, device tensors) of the seeded fp32 weights, uploaded once"""
    if not _DEV_WEIGHTS:
        sd = R.weights(torch.float32)
        t = {c: sd[R.PFX + k].to(DEV).contiguous() for c, k in _W.items()}
        w = fn().NetvladWeights()
        for c, v in t.items():
            setattr(w, c, v.data_ptr())
        _DEV_WEIGHTS.update(w=w, t=t)
    return _DEV_WEIGHTS["w"], _DEV_WEIGHTS["t"]


def run_head(x, seg_lens, dout, want=R.C_NAMES, want_feats=True):
    """lcr_netvlad_train_forward + lcr_netvlad_backward into guarded buffers -> dict of CPU tensors (out, stats, dx, the gradients by C name)"""
    L = lib()
    w, _ = dev_weights()
    seg = np.ascontiguousarray(seg_lens, dtype=np.int64)
    S, N = len(seg_lens), int(x.shape[0])
    xd, dd = x.to(DEV).contiguous(), dout.to(DEV).contiguous()
    st = L.stream_ptr(torch.device(DEV, 0))
    n_saved, n_ws, n_bws = (L.ws_size(q, N, S) for q in ("lcr_netvlad_train_saved_bytes", "lcr_netvlad_train_ws_bytes", "lcr_netvlad_backward_ws_bytes"))
    bufs = {k: guarded(s) for k, s in (("out", (S, 256)), ("stats", (1152,)), ("saved", ((n_saved + 3) // 4,)), ("ws", ((n_ws + 3) // 4,)),
                                       ("bws", ((n_bws + 3) // 4,)), ("dx", (N, 1024)))}
    bufs.update({c: guarded(SHAPES[c]) for c in R.C_NAMES})
    v = {k: b[1] for k, b in bufs.items()}
    L.call.lcr_netvlad_train_forward(L.ptr(xd), ctypes.c_void_p(seg.ctypes.data), S, ctypes.byref(w), L.ptr(v["out"]), L.ptr(v["stats"]), L.ptr(v["saved"]),
                                     n_saved, L.ptr(v["ws"]), n_ws, st)
    table = fn().NetvladGrads()
    for c in want:
        setattr(table, c, v[c].data_ptr())
    L.call.lcr_netvlad_backward(L.ptr(dd), L.ptr(xd), ctypes.c_void_p(seg.ctypes.data), S, ctypes.byref(w), L.ptr(v["saved"]), n_saved,
                                L.ptr(v["dx"]) if want_feats else None, ctypes.byref(table), L.ptr(v["bws"]), n_bws, st)
    torch.cuda.synchronize()
    assert intact([b[0] for b in bufs.values()]), "a canary was overwritten"
    for c in R.C_NAMES:
        assert c in want or bool(torch.isnan(v[c]).all()), c + " was written though not asked for"
    assert want_feats or bool(torch.isnan(v["dx"]).all())
    return {k: v[k].cpu() for k in ("out", "stats", "dx") + tuple(R.C_NAMES)}


def stats_dict(stats, S, Lmax):
    s = stats.double()
    return {"bn1.": (s[0:64], s[64:128], S * Lmax), "bn2.": (s[128:384], s[384:640], S), "context_gating.bn1.": (s[640:896], s[896:1152], S)}


def check(label, got, g64, g32, scale=None):
    g64 = g64.double()
    err = float((got.double().cpu() - g64).abs().max())
    e_ref = float((g32.double() - g64).abs().max())
    scale = float(g64.abs().max()) if scale is None else scale
    tol = R.bound(e_ref, scale)
    print("%-52s err %.3e  tol %.3e  err/tol %6.3f  e_ref %.3e" % (label, err, tol, err / tol if tol > 0 else 0.0, e_ref))
    assert torch.isfinite(got).all(), label + ": not finite"
    assert err <= tol, (label, err, tol)


def check_all(name, got, ref, rows=None):
    """every gradient, dx (optionally only `rows`) and the running buffers of one run against the shared references"""
    err = float((got["out"].double() - ref["out64"]).abs().max())
    print("%-52s err %.3e" % (name + " out", err))
    assert err <= 1e-4, ("out", err)
    for c in R.C_NAMES:
        check(name + " " + c, got[c].reshape(ref["g64"][C2P[c]].shape), ref["g64"][C2P[c]], ref["g32"][C2P[c]])
    if rows is None:
        check(name + " dx", got["dx"], ref["dx64"], ref["dx32"])
    else:
        check(name + " dx", got["dx"][rows], ref["dx64"][rows], ref["dx32"][rows])
    S, Lmax = len(ref["seg_lens"]), max(ref["seg_lens"])
    run = R.running_update(R.weights(torch.float32), stats_dict(got["stats"], S, Lmax))
    for k, v in ref["run64"].items():
        if not k.endswith("num_batches_tracked"):
            check(name + " " + k, run[k], v, ref["run32"][k])


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("case", list(R.CASES))
def test_head_matches_fp64(case):
    ref = R.reference(case)
    got = run_head(ref["x"], ref["seg_lens"], ref["dout"])
    check_all(case, got, ref)
    again = run_head(ref["x"], ref["seg_lens"], ref["dout"])
    assert all(same_bytes(got[k], again[k]) for k in got), "a second run gave other bytes"


def test_two_clouds_give_finite_values():
    """S = 2: every BatchNorm over the descriptors sees +-1, bn2's gradient is ~0 and ruled by rounding noise — finite is what is asked"""
    seg = (3, 5)
    got = run_head(R.features(seg, 21), seg, R.upstream(2, 21))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


def test_null_gradients_leave_the_others_unchanged():
    ref = R.reference("wraps")
    full = run_head(ref["x"], ref["seg_lens"], ref["dout"])
    for want, feats in ((("bn2_w", "gating_weights"), False), (("hidden1_weights",), False), (("cluster_weights2", "gbn_b"), False),
                        (("bn1_b",), False), ((), True), (("cluster_weights", "bn1_w"), False)):
        part = run_head(ref["x"], ref["seg_lens"], ref["dout"], want=want, want_feats=feats)
        assert same_bytes(part["out"], full["out"]) and same_bytes(part["stats"], full["stats"])
        assert all(same_bytes(part[c], full[c]) for c in want), want
        assert not feats or same_bytes(part["dx"], full["dx"])


def test_zero_upstream_gives_exact_zeros():
    ref = R.reference("wraps")
    got = run_head(ref["x"], ref["seg_lens"], torch.zeros_like(ref["dout"]))
    assert all(bool((got[k] == 0).all()) for k in ("dx",) + tuple(R.C_NAMES))


def test_zero_feature_row_follows_normalize():
    """F.normalize's backward at a zero row is dx = dx^ / 1e-12: that row is 1e12 times the others and is compared on its own scale"""
    seg, _ = R.CASES["wraps"]
    zr = 7
    ref = R.reference("wraps", zero_row=zr)
    assert float(ref["x"][zr].abs().max()) == 0.0
    got = run_head(ref["x"], seg, ref["dout"])
    others = [i for i in range(sum(seg)) if i != zr]
    check_all("zero-row", got, ref, rows=others)
    check("zero-row dx[zero row]", got["dx"][zr], ref["dx64"][zr], ref["dx32"][zr])
    assert float(ref["dx64"][zr].abs().max()) > 1e6 * float(ref["dx64"][others].abs().max())


def test_entries_refuse_outside_their_domain():
    F, L = fn(), lib()
    w, _ = dev_weights()
    with pytest.raises(ValueError):
        F.netvlad_train(torch.zeros(5, 1024, device=DEV), [5], w)
    x = torch.zeros(129 * 1024, device=DEV)
    small = torch.zeros(1 << 16, device=DEV)
    st = L.stream_ptr(torch.device(DEV, 0))
    table = F.NetvladGrads()
    for seg in ([1] * 129, [3, 0, 2], [4]):
        s = np.ascontiguousarray(seg, dtype=np.int64)
        rc = L.lib().lcr_netvlad_train_forward(L.ptr(x), ctypes.c_void_p(s.ctypes.data), len(seg), ctypes.byref(w), L.ptr(small), L.ptr(small), L.ptr(small),
                                               small.numel() * 4, L.ptr(small), small.numel() * 4, st)
        assert rc == -1 and L.lib().lcr_last_error().startswith(b"lcr_netvlad_train_forward:"), seg
        rc = L.lib().lcr_netvlad_backward(L.ptr(small), L.ptr(x), ctypes.c_void_p(s.ctypes.data), len(seg), ctypes.byref(w), L.ptr(small), small.numel() * 4,
                                          None, ctypes.byref(table), L.ptr(small), small.numel() * 4, st)
        assert rc == -1 and L.lib().lcr_last_error().startswith(b"lcr_netvlad_backward:"), seg
    torch.cuda.synchronize()
    assert bool((small == 0).all()), "a refused call launched something"


# ------------------------------------------------------------------------------------------------ the reference's own numbers
def test_gradients_match_reference_golden():
    """the IMPORTED reference NetVLADLoupe2.train() through GlobalDescritionHEAD's own padding code (tests/golden/make_golden_netvlad_grad.py),
    fp64; e_ref = the reference's fp32 run against it.  hidden1_weights (67 MB) by a seeded sample of 256 rows, all row sums and column sums."""
    sys.path.insert(0, os.path.join(R.ROOT, "tests", "golden"))
    from make_golden_netvlad_grad import load_golden, sample_rows
    gold = load_golden()
    seg, seed = R.CASES[R.GOLDEN_CASE]
    assert tuple(gold["seg_lens"]) == tuple(seg)
    got = run_head(R.features(seg, seed), seg, R.upstream(len(seg), seed))
    err = float((got["out"].double() - torch.from_numpy(gold["out"])).abs().max())
    assert err <= 1e-4, ("out", err)
    dH = got["hidden1_weights"].double()
    views = {"hidden1_weights/rows": dH[torch.from_numpy(sample_rows())], "hidden1_weights/row_sums": dH.sum(1), "hidden1_weights/col_sums": dH.sum(0)}
    views.update({C2P[c]: got[c].double() for c in R.C_NAMES if c != "hidden1_weights"})
    views["dx"] = got["dx"].double()
    for k, v in views.items():
        ref, e_ref = torch.from_numpy(gold["grad/" + k]), float(gold["err/" + k])
        err = float((v.reshape(ref.shape) - ref).abs().max())
        tol = R.bound(e_ref, float(ref.abs().max()))
        print("%-52s err %.3e  tol %.3e  err/tol %6.3f  e_ref %.3e" % ("golden " + k, err, tol, err / tol, e_ref))
        assert err <= tol, (k, err, tol)
    run = R.running_update(R.weights(torch.float32), stats_dict(got["stats"], len(seg), max(seg)))
    for k in run:
        if not k.endswith("num_batches_tracked"):
            ref, e_ref = torch.from_numpy(gold["buffer/" + k]), float(gold["err/buffer/" + k])
            err = float((run[k] - ref).abs().max())
            assert err <= R.bound(e_ref, float(ref.abs().max())), (k, err)


# ------------------------------------------------------------------------------------------------ the module
def head_module():
    from lcrnet_amd.modules.netvlad import NetVLADLoupe2
    m = NetVLADLoupe2(1024, 64, 256)
    keys = list(m.state_dict().keys())
    m.load_state_dict({k[len(R.PFX):]: v for k, v in R.weights(torch.float32).items()}, strict=False)
    return m.to(DEV), keys


def test_module_contract():
    F = fn()
    ref = R.reference("wraps")
    seg = ref["seg_lens"]
    m, keys = head_module()
    assert keys == list(m.state_dict().keys()) and sorted(k for k in keys) == sorted(
        [k[len(R.PFX):] for k in R.weights()] + [b + "num_batches_tracked" for b in R.BNS]), "state_dict keys changed"
    x = ref["x"].to(DEV).requires_grad_(True)
    # eval: today's call, today's bytes, no graph — also outside no_grad with everything requiring grad
    m.eval()
    quiet = m.describe(x, seg)
    assert quiet.grad_fn is None and not quiet.requires_grad
    assert same_bytes(quiet, F.netvlad_forward(x.detach().contiguous(), np.asarray(seg, dtype=np.int64), m._weights()))
    assert int(m.bn1.num_batches_tracked) == 0
    # training under no_grad: batch statistics, buffers updated, no graph
    m.train()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        plain = m.describe(x, seg)
    assert plain.grad_fn is None and not plain.requires_grad
    assert float((plain.cpu().double() - ref["out64"]).abs().max()) <= 1e-4
    for b in R.BNS:
        assert int(m.state_dict()[b + "num_batches_tracked"]) == 1
        for leaf in ("running_mean", "running_var"):
            check("module " + b + leaf, m.state_dict()[b + leaf].cpu(), ref["run64"][b + leaf], ref["run32"][b + leaf])
            assert not torch.equal(m.state_dict()[b + leaf], before[b + leaf])
    # training with a graph: the same bytes, every parameter and the input get the kernel's gradients
    out = m.describe(x, seg)
    assert out.grad_fn is not None and same_bytes(out.detach(), plain)
    (out * ref["dout"].to(DEV)).sum().backward()
    for b in R.BNS:
        assert int(m.state_dict()[b + "num_batches_tracked"]) == 2
    named = dict(m.named_parameters())
    for k in R.PARAMS:
        assert named[k].grad is not None, k + " has no gradient"
        check("module " + k, named[k].grad, ref["g64"][k], ref["g32"][k])
    check("module dx", x.grad, ref["dx64"], ref["dx32"])
    with pytest.raises(ValueError):
        m.describe(x[:5], [5])
    with pytest.raises(RuntimeError):
        F.netvlad_train(ref["x"], seg, m._weights())              # a CPU tensor
    with pytest.raises(RuntimeError):
        F.netvlad_backward(ref["dout"], ref["x"], seg, m._weights(), torch.zeros(8))


# ------------------------------------------------------------------------------------------------ end to end: encoder -> head -> triplet loss -> Adan
# one anchor, two positives, two negatives of 16-20 points; GroupNorm over the whole stack (the reference's training behaviour).
# searched on the CPU (e2e_margins): the lowest seed whose fp64 run keeps every LeakyReLU / KPConv row count / max-pool / hinge / farthest-positive
# decision >= 1e-5 of its scale with at least one active triplet.  Five clouds hold ~1e5 pre-activations: with 16 - 20 points in a 3 x 3 x 1.2 m
# box no seed of 0 .. 39 999 keeps the encoder's margin (best 8.3e-6, seed 34 848); with 16 points each in a 2 x 2 x 1 m box seed 460 is the first
# of 0 .. 460 (encoder 1.30e-5, hinge 0.296, farthest-positive gap 0.146, both triplets active).  tests/test_netvlad_grad_cpu.py asserts them.
# lr 1e-6: Adan's first update is lr * sign(g) on every one of the 67 M hidden weights at once; from 1e-5 on the CPU run's hinge is dead (loss
# exactly 0) at the third step.  At 1e-6 it falls 0.800 -> 0.719 -> 0.642 -> 0.568 -> 0.495 with both triplets active throughout.
E2E = dict(seed=460, points=(16, 16, 16, 16, 16), box=(2.0, 2.0, 1.0), weights_seed=7351, lr=1e-6, margin=0.5, steps=5)
LIMITS = [12, 12, 12, 12]


def e2e_clouds(seed=None):
    gen = torch.Generator().manual_seed(900 + (E2E["seed"] if seed is None else seed))
    return [(torch.rand(n, 3, generator=gen) * torch.tensor(E2E["box"])).float().numpy() for n in E2E["points"]]


def e2e_inputs(seed=None):
    """(oracle data dict of CPU tensors, coarse lengths)"""
    from oracle import ops as oracle_ops
    import encoder_grad_restatement as ER
    clouds = e2e_clouds(seed)
    st = oracle_ops.precompute_data_stack_mode(np.concatenate(clouds), np.array([len(c) for c in clouds], dtype=np.int64), 4, 0.3, ER.RADIUS, LIMITS)
    dd = {k: [torch.from_numpy(np.ascontiguousarray(t)) for t in v] for k, v in st.items()}
    return dd, [int(v) for v in dd["lengths"][-1]]


def e2e_model(cfg_extra=None):
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family import LCRNet_GlobalDescrition
    from lcrnet_amd.weights import seeded_state_dict
    import encoder_grad_restatement as ER
    cfg = make_cfg()
    cfg["backbone"].update(init_radius=ER.RADIUS, init_sigma=ER.SIGMA)
    cfg.update(cfg_extra or {})
    m = LCRNet_GlobalDescrition(cfg)
    m.load_state_dict(seeded_state_dict(m.state_dict(), E2E["weights_seed"], init_radius=ER.RADIUS), strict=True)
    return m


def e2e_trainable(k, v):
    return v.dtype.is_floating_point and not k.endswith("kernel_points") and "running_" not in k


def e2e_loss(sd, dd, lens, dtype, record=None):
    """(loss, descriptors, decision margins of the loss) of one forward through oracle/torch_ref's encoder, the padded head and TripletLoss"""
    from oracle import torch_ref
    import encoder_grad_restatement as ER
    from lcrnet_amd.losses import TripletLoss
    d = {k: [t.to(dtype) if t.dtype.is_floating_point else t for t in v] for k, v in dd.items()}
    feats = torch.ones(d["points"][0].shape[0], 1, dtype=dtype)
    f = torch_ref.kp_encoder(sd, feats, d, init_sigma=ER.SIGMA, groups=32, segment_lengths=None)[-1]
    g = R.padded_reference(sd, f, lens)
    out = {"anc_global": g[:1].reshape(1, -1, 256), "pos_global": g[1:3].reshape(1, -1, 256), "neg_global": g[3:].reshape(1, -1, 256)}
    loss = TripletLoss(E2E["margin"])(out)["loss"]
    pos = ((out["pos_global"] - out["anc_global"]) ** 2).sum(2).detach()[0]
    neg = ((out["neg_global"] - out["anc_global"]) ** 2).sum(2).detach()[0]
    hinge = E2E["margin"] + pos.max() - neg
    return loss, {"hinge": float(hinge.abs().min()), "farthest": float((pos.max() - pos.min()).abs()), "active": int((hinge > 0).sum())}


def e2e_margins(seed=None):
    """decision margins of the first step in fp64: (encoder LeakyReLU / row-count / max-pool margin, hinge, farthest-positive gap, active triplets)"""
    import test_encoder_grad_gpu as G
    dd, lens = e2e_inputs(seed)
    sd = {k: v.double() if v.dtype.is_floating_point else v for k, v in e2e_model().state_dict().items()}
    with G.Recorder() as rec:
        _, m = e2e_loss(sd, dd, lens, torch.float64)
    return dict(encoder=rec.margin(), **m)


def e2e_reference_run(steps):
    """(losses, {key: moved?}) of `steps` CPU steps in fp32: torch_ref encoder + padded head + TripletLoss + the torch form of Adan"""
    from lcrnet_amd.adan import Adan
    dd, lens = e2e_inputs()
    sd = {k: v.detach().clone() for k, v in e2e_model().state_dict().items()}
    start = {k: v.clone() for k, v in sd.items()}
    params = [v.requires_grad_(True) for k, v in sd.items() if e2e_trainable(k, v)]
    opt = Adan(params, lr=E2E["lr"], fused=False)
    losses = []
    for _ in range(steps):
        loss, _ = e2e_loss(sd, dd, lens, torch.float32)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: not torch.equal(v.detach(), start[k]) for k, v in sd.items() if e2e_trainable(k, v)}


def e2e_device_dict():
    from lcrnet_amd.data import precompute_batch
    import encoder_grad_restatement as ER
    clouds = e2e_clouds()
    pts = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    d = precompute_batch(pts.contiguous(), torch.tensor([len(c) for c in clouds], device=DEV), 4, 0.3, ER.RADIUS, LIMITS)
    dd, lens = e2e_inputs()
    assert d["lengths_host"][-1] == lens and torch.equal(d["points"][3].cpu(), dd["points"][3])
    d.pop("segment_lengths")                                   # GroupNorm over the whole stack
    d["features"] = torch.ones(d["points"][0].shape[0], 1, device=DEV)
    d["batch_size"], d["pos_num"] = 1, [2]
    return d


def test_descriptor_model_trains():
    from lcrnet_amd.adan import Adan
    from lcrnet_amd.losses import TripletLoss
    mg = e2e_margins()
    assert min(mg["encoder"], mg["hinge"], mg["farthest"]) >= 1e-5 and mg["active"] >= 1, mg
    ref_losses, ref_moved = e2e_reference_run(E2E["steps"])
    d = e2e_device_dict()
    model = e2e_model().to(DEV).train()
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    opt = Adan(model.parameters(), lr=E2E["lr"], fused=True)
    crit = TripletLoss(E2E["margin"])
    losses = []
    for _ in range(E2E["steps"]):
        out = model(d)
        assert tuple(out["anc_global"].shape) == (1, 1, 256) and tuple(out["pos_global"].shape) == (1, 2, 256) and tuple(out["neg_global"].shape) == (1, 2, 256)
        loss = crit(out)["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print("device losses:    " + " ".join("%.6f" % v for v in losses))
    print("reference losses: " + " ".join("%.6f" % v for v in ref_losses))
    assert all(math.isfinite(v) for v in losses)
    assert abs(losses[0] - ref_losses[0]) <= 1e-4, (losses[0], ref_losses[0])
    for k in range(1, E2E["steps"]):
        assert abs(losses[k] - ref_losses[k]) <= 1e-2 * abs(ref_losses[k]), (k, losses[k], ref_losses[k])
    for k, prm in model.named_parameters():
        assert not ref_moved[k] or not torch.equal(prm.detach(), start[k]), k + " did not move"
    assert int(model.netvlad.bn2.num_batches_tracked) == E2E["steps"]
    with pytest.raises(RuntimeError):
        from lcrnet_amd.model_family import LCRNet
        LCRNet().train().forward_pairs({})


def test_half_mode_trains_the_head_only():
    """train_mode 'half': the encoder runs without a graph on the stack, the precomputed feats_c / lengths_c are appended; the head's gradients
    are those of the head alone on the same features, to the bit"""
    from lcrnet_amd.losses import TripletLoss
    d = e2e_device_dict()
    gen = torch.Generator().manual_seed(77)
    extra_lens = [3, 6]
    d["feats_c"] = torch.randn(sum(extra_lens), 1024, generator=gen).clamp_(min=0).to(DEV)
    d["lengths_c"] = torch.tensor(extra_lens)
    model = e2e_model({"train_mode": "half"}).to(DEV).train()
    crit = TripletLoss(E2E["margin"])
    out = model(d)
    assert tuple(out["neg_global"].shape) == (1, 4, 256)
    crit(out)["loss"].backward()
    assert all(p.grad is None for p in model.encoder.parameters())
    got = {k: p.grad.clone() for k, p in model.netvlad.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in got.values()) and any(float(g.abs().max()) > 0 for g in got.values())
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        feats_c = torch.cat([model.encoder(d["features"], d)[-1], d["feats_c"]])
    g = model.netvlad.describe(feats_c, d["lengths_host"][-1] + extra_lens)
    crit({"anc_global": g[:1].reshape(1, -1, 256), "pos_global": g[1:3].reshape(1, -1, 256), "neg_global": g[3:].reshape(1, -1, 256)})["loss"].backward()
    for k, p in model.netvlad.named_parameters():
        assert same_bytes(p.grad, got[k]), k
