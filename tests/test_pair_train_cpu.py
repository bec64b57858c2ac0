"""CPU: the yardsticks of tests/test_pair_train_gpu.py, without a GPU.  The restatement of lcr_patch_scores_grad
(tests/patch_scores_grad_restatement.py) is pinned to fp64 autograd through the dense formula (cat a zero row -> index -> bmm -> masked
select), and every planted mistake must exceed the tolerance the GPU test holds the kernel to — encoder_grad_restatement.bound(e_ref, scale)
with e_ref the error of fp32 torch autograd of the same formula against fp64 — on an output meant to see it.  SuperPointTargetGenerator is
held against a direct restatement of superpoint_target.py:27-40; the new wrappers refuse host tensors; make_cfg() carries the reference's
two coarse_matching values; the base LCRNet still refuses training mode."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_grad_restatement as ER
import patch_scores_grad_restatement as R

CASES = {c.name: c for c in R.cases()}


def finite_case(name):
    c = CASES[name]
    return R.Case(c.name, c.P, c.C, c.Na, c.Nb, 11 if name == "C32" else 12, single=1, nan=False)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_fp64_autograd_of_the_dense_formula(name):
    c = CASES[name]
    assert bool(torch.isnan(c.dS[:, -1, :]).all()) and bool(torch.isnan(c.dS[:, :, -1]).all()), "NaN at every dustbin entry"
    da, db = R.patch_scores_grad(*c.args(torch.float64))
    ga, gb = R.autograd_grad(*c.args(), torch.float64)
    assert torch.isfinite(da).all() and torch.isfinite(db).all()
    assert float((da - ga).abs().max()) <= 1e-12 * float(ga.abs().max())
    assert float((db - gb).abs().max()) <= 1e-12 * float(gb.abs().max())
    ua, ub = c.unlisted()
    assert int(ua.sum()) >= 1 and int(ub.sum()) >= 1, "the case must leave rows unlisted"
    assert float(da[ua].abs().max()) == 0.0 and float(db[ub].abs().max()) == 0.0
    assert int(c.ma[1].sum()) == 1, "one patch with a single live row"
    cnt = torch.bincount(c.ia[c.ia < c.Na], minlength=c.Na)
    assert int(cnt.max()) >= 2 and any(len(set(r.tolist())) < c.K for r in c.ia), "rows repeat within and across patches"


@pytest.mark.parametrize("mistake", R.MISTAKES)
@pytest.mark.parametrize("name", list(CASES))
def test_planted_mistakes_exceed_the_tolerance(name, mistake):
    c = finite_case(name) if mistake in ("no_mask", "dustbin") else CASES[name]       # these two read entries where the NaN sits
    a64 = R.patch_scores_grad(*c.args(torch.float64))
    a32 = R.autograd_grad(*c.args(), torch.float32)
    bad = R.patch_scores_grad(*c.args(torch.float64), mistake=mistake)
    caught = False
    for g64, g32, gb in zip(a64, a32, bad):
        tol = ER.bound(float((g32.double() - g64).abs().max()), float(g64.abs().max()))
        err = float((gb - g64).abs().max())
        caught |= not (err <= tol)                                                      # a NaN counts as caught
    assert caught, mistake


# ---- SuperPointTargetGenerator against superpoint_target.py:27-40 ---------------------------------------------------------------------
def _targets():
    from lcrnet_amd.modules.registration import SuperPointTargetGenerator
    return SuperPointTargetGenerator


def test_target_generator_threshold_and_sampling():
    Gen = _targets()
    g = torch.Generator().manual_seed(5)
    idx = torch.stack([torch.arange(40), torch.randperm(40, generator=g)], 1)
    ov = torch.rand(40, generator=g)
    ov[3] = 0.1                                              # equality with the threshold is excluded (torch.gt)
    ov[4] = float(np.nextafter(np.float32(0.1), np.float32(1)))
    keep = ov > 0.1
    assert not bool(keep[3]) and bool(keep[4])
    n = int(keep.sum())
    # at or below num_targets: no sampling, the kept rows in order, whatever the generator's state
    for num in (n, n + 7):
        t = Gen(num, 0.1, seed=1)
        state = t.rng.bit_generator.state
        r, s, o = t(idx, ov)
        assert torch.equal(r, idx[keep, 0]) and torch.equal(s, idx[keep, 1]) and torch.equal(o, ov[keep])
        assert t.rng.bit_generator.state == state, "nothing may be drawn at or below num_targets"
    # above: num_targets distinct rows of the kept ones, drawn by the module's own generator
    t = Gen(n - 1, 0.1, seed=1)
    r, s, o = t(idx, ov)
    assert r.numel() == n - 1 and len(set(r.tolist())) == n - 1, "an index was repeated"
    want = np.random.default_rng(1).choice(n, n - 1, replace=False)
    assert torch.equal(r, idx[keep, 0][want]) and torch.equal(s, idx[keep, 1][want]) and torch.equal(o, ov[keep][want])
    t(idx, ov)                                               # a second draw moves the generator on ...
    t.reseed()
    assert torch.equal(t(idx, ov)[0], r), "... and reseeding brings the first one back"
    t.reseed(9)
    assert t.seed == 9 and torch.equal(t(idx, ov)[0], idx[keep, 0][np.random.default_rng(9).choice(n, n - 1, replace=False)])
    # nothing above the threshold: empty results
    r, s, o = Gen(4, 0.1)(idx, torch.full((40,), 0.1))
    assert r.numel() == 0 and s.numel() == 0 and o.numel() == 0


def test_target_generator_is_seeded_from_the_config():
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family import LCRNet_Matching as module
    cfg = make_cfg()
    assert cfg["coarse_matching"] == {"num_targets": 128, "overlap_threshold": 0.1}
    m = module.LCRNet_Matching(cfg)
    assert m.coarse_target.num_targets == 128 and m.coarse_target.overlap_threshold == 0.1 and m.coarse_target.seed == cfg["seed"]
    assert not list(m.coarse_target.state_dict()), "the generator adds nothing to the checkpoint layout"
    assert "inference only" not in module.__doc__


def test_wrappers_refuse_host_tensors():
    from lcrnet_amd import functional as F
    c = CASES["C32"]
    with pytest.raises(RuntimeError, match="GPU only"):
        F.patch_scores_grad(torch.zeros(c.P, 129, 129), c.fa, c.fb, c.ia, c.ib, c.ma8, c.mb8, c.scale)
    fa, fb, al = c.fa.clone().requires_grad_(True), c.fb.clone().requires_grad_(True), torch.tensor(1.0, requires_grad=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.patch_log_optimal_transport(fa, c.ia, fb, c.ib, c.ma, c.mb, al, scale=c.scale)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.bmm_nt(torch.zeros(2, 5, 8, requires_grad=True), torch.zeros(2, 7, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        F.gemm(torch.zeros(5, 8, requires_grad=True), torch.zeros(7, 8), trans_b=True)


def test_base_model_still_refuses_training_mode():
    from lcrnet_amd.model_family import LCRNet
    with pytest.raises(RuntimeError, match="inference only"):
        LCRNet().train().forward_pairs({})


def test_header_declares_the_new_entries():
    from lcrnet_amd import _lib
    sigs = {}
    for h in _lib.HEADERS:
        with open(h) as f:
            sigs.update(_lib.parse_header(f.read()))
    assert len(sigs["lcr_patch_scores_grad"][1]) == 22 and len(sigs["lcr_patch_scores_grad_ws_bytes"][1]) == 4
