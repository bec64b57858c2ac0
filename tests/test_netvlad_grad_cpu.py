"""CPU: the yardsticks of tests/test_netvlad_grad_gpu.py, without a GPU.  The fp64 restatement of the training head (forward by row multiplicities,
hand-derived reverse pass; tests/netvlad_grad_restatement.py) is pinned to fp64 autograd through a plain-torch form of the reference's padded
formula and to the imported reference's own numbers (the golden); every planted mistake must move a gradient (or a buffer) by >= 1e-3 of its
scale on a case meant to see it; the multiplicity formula is held against explicit padding; the end-to-end case's decision margins are asserted."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netvlad_grad_restatement as R

TOL = 1e-12
NEW_ENTRIES = ("lcr_netvlad_train_ws_bytes", "lcr_netvlad_train_saved_bytes", "lcr_netvlad_train_forward", "lcr_netvlad_backward_ws_bytes",
               "lcr_netvlad_backward")


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def case_inputs(case):
    seg, seed = R.CASES[case]
    return seg, R.features(seg, seed), R.upstream(len(seg), seed)


@pytest.mark.parametrize("case", ["no-padding", "wraps", "one-row-x130", "nine-clouds"])
def test_restatement_equals_fp64_autograd_of_the_padded_formula(case):
    seg, x, dout = case_inputs(case)
    sd = R.weights()
    out, g, dx, st = R.gradients(sd, x, seg, dout)
    out_a, g_a, dx_a, st_a = R.autograd(sd, x, seg, dout, torch.float64)
    assert float((out - out_a).abs().max()) <= TOL
    for k in R.PARAMS:
        assert rel(g[k], g_a[k]) <= TOL, (k, rel(g[k], g_a[k]))
    assert rel(dx, dx_a) <= TOL
    for bn in R.BNS:
        assert float((st[bn][0] - st_a[bn][0]).abs().max()) <= TOL and float((st[bn][1] - st_a[bn][1]).abs().max()) <= TOL and st[bn][2] == st_a[bn][2]


def test_restatement_equals_the_reference_golden():
    sys.path.insert(0, os.path.join(R.ROOT, "tests", "golden"))
    from make_golden_netvlad_grad import load_golden, sample_rows
    gold = load_golden()
    seg, x, dout = case_inputs(R.GOLDEN_CASE)
    assert tuple(gold["seg_lens"]) == tuple(seg)
    sd = R.weights()
    out, g, dx, st = R.gradients(sd, x, seg, dout)
    assert float((out - torch.from_numpy(gold["out"])).abs().max()) <= TOL
    dH = g["hidden1_weights"]
    views = {"hidden1_weights/rows": dH[torch.from_numpy(sample_rows())], "hidden1_weights/row_sums": dH.sum(1), "hidden1_weights/col_sums": dH.sum(0), "dx": dx}
    views.update({k: g[k] for k in R.PARAMS if k != "hidden1_weights"})
    for k, v in views.items():
        assert rel(v, torch.from_numpy(gold["grad/" + k]).reshape(v.shape)) <= TOL, k
    for k, v in R.running_update(sd, st).items():
        if not k.endswith("num_batches_tracked"):
            assert rel(v, torch.from_numpy(gold["buffer/" + k])) <= TOL, k
    assert len([k for k in gold if k.startswith("err/")]) == 20 and all(float(gold[k]) > 0 for k in gold if k.startswith("err/"))


@pytest.mark.parametrize("mutate", [m for m in R.MUTATIONS if m != "running_var_biased"])
def test_planted_mistake_moves_a_gradient(mutate):
    seg, x, dout = case_inputs("wraps")               # a partial and a multiple wrap: every padding mistake shows; S = 4: every statistic matters
    sd = R.weights()
    _, g, dx, _ = R.gradients(sd, x, seg, dout)
    _, gm, dxm, _ = R.gradients(sd, x, seg, dout, mutate=mutate)
    moved = {k: rel(gm[k], g[k]) for k in R.PARAMS}
    moved["dx"] = rel(dxm, dx)
    print(mutate, {k: "%.1e" % v for k, v in moved.items()})
    assert max(moved.values()) >= 1e-3, moved


def test_biased_running_variance_shows():
    seg, x, dout = case_inputs("wraps")
    sd = R.weights()
    _, _, _, st = R.gradients(sd, x, seg, dout)
    good, bad = R.running_update(sd, st), R.running_update(sd, st, mutate="running_var_biased")
    for bn in R.BNS[1:]:                              # n = S = 4: a third of the batch variance
        assert rel(bad[bn + "running_var"], good[bn + "running_var"]) >= 1e-3
    # torch's own BatchNorm1d agrees with the update rule
    bn = torch.nn.BatchNorm1d(256).double().train()
    bn.running_mean.copy_(sd[R.PFX + "bn2.running_mean"])
    bn.running_var.copy_(sd[R.PFX + "bn2.running_var"])
    h = torch.randn(4, 256, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    bn(h)
    want = R.running_update(sd, dict(st, **{"bn2.": (h.mean(0), h.var(0, unbiased=False), 4)}))
    assert rel(want["bn2.running_var"], bn.running_var) <= TOL and rel(want["bn2.running_mean"], bn.running_mean) <= TOL
    assert int(bn.num_batches_tracked) == want["bn2.num_batches_tracked"]


@pytest.mark.parametrize("seg", [(4, 4, 4), (5, 9, 7, 2), (1, 130, 67), (3, 1, 2, 7)])
def test_multiplicity_counts_the_cyclic_padding(seg):
    """the reference pads by cat(t, t) until long enough, then cuts: count how often every row lands in the padded tensor"""
    Lmax, o, want = max(seg), 0, []
    for L in seg:
        t = torch.arange(o, o + L)
        while len(t) < Lmax:
            t = torch.cat((t, t))
        want.append(torch.bincount(t[:Lmax] - o, minlength=L))
        o += L
    c = R.multiplicity(seg)
    assert torch.equal(c, torch.cat(want)) and int(c.sum()) == len(seg) * Lmax


def test_single_cloud_raises_like_batchnorm():
    with pytest.raises(ValueError):
        R.forward(R.weights(), R.features((5,), 1).double(), (5,))


def test_end_to_end_case_keeps_its_decision_margins():
    """the seeded training case of tests/test_netvlad_grad_gpu.py: every LeakyReLU / KPConv row count / max-pool decision of the encoder, every
    hinge and the farthest-positive choice stay >= 1e-5 of their scale in fp64, and at least one triplet is active"""
    import test_netvlad_grad_gpu as G
    m = G.e2e_margins()
    print(m)
    assert m["active"] >= 1
    assert min(m["encoder"], m["hinge"], m["farthest"]) >= 1e-5, m


def test_header_declares_and_library_exports_the_entries():
    from lcrnet_amd import _lib
    with open(os.path.join(R.ROOT, "include", "lcr_hip.h")) as f:
        sigs = _lib.parse_header(f.read())
    for name in NEW_ENTRIES:
        assert name in sigs, name + " is not declared in include/lcr_hip.h"
    assert os.path.exists(_lib.LIB_PATH), "the library has not been built"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(lcr_\w+)", out))
    for name in NEW_ENTRIES:
        assert name in exported, name + " is not exported by the library"


def test_wrappers_refuse_cpu_tensors():
    from lcrnet_amd import functional as F
    w = F.NetvladWeights()
    x = torch.zeros(5, 1024)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.netvlad_train(x, [2, 3], w)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.netvlad_backward(torch.zeros(2, 256), x, [2, 3], w, torch.zeros(8))


def test_training_mode_no_longer_refuses_the_descriptor_model():
    """forward_pairs still has no backward behind its decoder, vote modules and top-k attention: it keeps refusing training mode"""
    from lcrnet_amd.model_family import LCRNet
    with pytest.raises(RuntimeError, match="inference only"):
        LCRNet().train().forward_pairs({})
    with open(os.path.join(R.ROOT, "lcr-net_amd", "modules", "netvlad", "NetVlad.py")) as f:
        assert "inference only" not in f.read()
