"""CPU: the fp64 restatement of the Adan step (tests/adan_restatement.py) against goldens of the IMPORTED reference optimiser
(tests/golden/make_golden_adan.py), the planted mistakes, the torch path of lcrnet_amd.adan.Adan (fused=False), the state_dict
interchange with the reference's layout, and the argument checks that need no GPU.

The reference runs in fp32 and the restatement in fp64, so they differ by the reference's own rounding error e_ref.  Here e_ref is
bounded by reasoning: every quantity is a handful of fp32 operations on values of magnitude <= ~4 (parameters 0.5 * randn, gradients up
to 1.1 * randn), each rounding at 2^-24 relative to its operands, a few of them amplified by 1 / bias (<= 10) or lr / den; 64 units of
2^-24 at the largest magnitude the quantity takes in any tensor of the case at that step (a one-element tensor can cancel to far less
than its operands) is ample for four steps.  The GPU tests take e_ref as measured, per case and quantity."""
import ctypes

import numpy as np
import pytest
import torch

import adan_restatement as R
from lcrnet_amd.config import make_cfg


@pytest.fixture(scope="module")
def gold():
    return R.Golden()


@pytest.fixture(scope="module")
def e_ref(gold):
    return R.e_ref_table(gold)


def build_optimizer(name, cls, device="cpu", **kw):
    """A case's parameters (float32 leaves) and an optimiser of class `cls` over its groups."""
    p0, grads = R.case_inputs(name)
    groups, max_norm = R.case_groups(name)
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(device)) for p in p0]
    pg = [dict(params=[params[i] for i in idx], **{k: h[k] for k in ("lr", "betas", "eps", "weight_decay", "no_prox")}) for idx, h in groups]
    return params, grads, cls(pg, max_grad_norm=max_norm, **kw)


def set_grads(params, gk):
    for p, g in zip(params, gk):
        p.grad = None if g is None else torch.from_numpy(g.copy()).to(p.device)


def figures(params, opt, want_step, e_ref, name):
    """max over the tensors of (error / bound) per quantity after one step; a tensor without state must have none on either side."""
    worst = {}
    for q in R.QUANTITIES:
        for i, p in enumerate(params):
            want = want_step[q][i]
            if want is None:
                assert len(opt.state.get(p, {})) == 0, (name, q, i)
                continue
            got = (p.detach() if q == "p" else opt.state[p][q]).cpu().numpy()
            worst[q] = max(worst.get(q, 0.0), R.err(got, want) / R.bound(e_ref[(name, q)], want))
    return worst


def test_seeded_inputs_are_the_ones_the_golden_was_made_from(gold):
    for name in R.CASES:
        assert R.digest(name) == gold.z[name + "_digest"], name


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_equals_the_reference(gold, e_ref, name):
    r = R.run(name)
    for q in R.QUANTITIES:
        print("%s %s: e_ref %.3g" % (name, q, e_ref[(name, q)]))
        for form in ("foreach", "single"):
            for k in range(1, R.K + 1):
                scale = max(np.abs(w).max() for w in r[k - 1][q] if w is not None)
                for i, want in enumerate(r[k - 1][q]):
                    have = gold.get(name, form, k, q, i)
                    if want is None:
                        assert have is None
                        continue
                    assert R.err(have, want) <= 64 * 2.0 ** -24 * scale, (q, form, k, i)
                    if q == "exp_avg_diff" and k == 1:
                        assert not np.any(have) and not np.any(want)     # diff is exactly zero on a first step
    if name == "c5":                                                      # tensor 3 gains its gradient at step 3: fresh there
        assert r[1]["p"][3] is None and not np.any(r[2]["exp_avg_diff"][3]) and not np.any(gold.get(name, "single", 3, "exp_avg_diff", 3))
    if name in ("c3", "c4", "c5"):
        assert all(s["clip"] < 1 for s in r)                              # these cases do clip
        assert np.array_equal(r[0]["pre_grad"][0], r[0]["grad"][0])


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_move_the_restatement_beyond_the_tolerance(e_ref, mistake):
    """Every planted mistake moves at least one compared tensor of at least one case by at least 8 x that tensor's tolerance: the goldens
    (and the GPU tests, which use the same inputs and tolerance) can see it."""
    best, where = 0.0, None
    for name in sorted(R.CASES):
        r, rm = R.run(name), R.run(name, mistake=mistake)
        for k in range(R.K):
            for q in R.QUANTITIES:
                for i, (a, b) in enumerate(zip(r[k][q], rm[k][q])):
                    if a is not None:
                        ratio = R.err(b, a) / R.bound(e_ref[(name, q)], a)
                        if ratio > best:
                            best, where = ratio, (name, k + 1, q, i)
    print("%s: %.3g x the tolerance at %s" % (mistake, best, where))
    assert best >= 8
    if mistake == "prox_swap":                                            # invisible without weight decay, as it must be
        assert all(np.array_equal(a, b) for a, b in zip(R.run("c1")[-1]["p"], R.run("c1", mistake=mistake)[-1]["p"]))
    if mistake == "preclip":                                              # invisible without clipping
        assert all(np.array_equal(a, b) for a, b in zip(R.run("c2")[-1]["p"], R.run("c2", mistake=mistake)[-1]["p"]))


@pytest.mark.parametrize("foreach", [True, False])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_torch_path_equals_the_restatement(e_ref, name, foreach):
    from lcrnet_amd.adan import Adan
    params, grads, opt = build_optimizer(name, Adan, foreach=foreach, fused=False)
    r = R.run(name)
    for k, gk in enumerate(grads):
        set_grads(params, gk)
        opt.step()
        fig = figures(params, opt, r[k], e_ref, name)
        print(name, foreach, k + 1, {q: "%.3g" % v for q, v in fig.items()})
        assert all(v <= 1 for v in fig.values()), (k + 1, fig)
        for i, p in enumerate(params):
            if gk[i] is not None:                                         # the gradient is clipped in place, or untouched
                want = r[k]["grad"][i]
                if r[k]["clip"] >= 1:
                    assert np.array_equal(p.grad.numpy(), gk[i])
                else:
                    assert R.err(p.grad.numpy(), want) <= R.bound(e_ref[(name, "pre_grad")], want)
                if k == 0:
                    assert not opt.state[p]["exp_avg_diff"].any()
                assert opt.state[p]["pre_grad"].data_ptr() != p.grad.data_ptr()


def reference_state_dict(gold, name, form="single"):
    """The state_dict the reference's optimiser holds after the golden's last step, rebuilt from the golden file."""
    groups, max_norm = R.case_groups(name)
    state, pgs, n = {}, [], 0
    for idx, h in groups:
        ids = []
        for i in idx:
            state[n] = {q: torch.from_numpy(gold.get(name, form, R.K, q, i).copy()) for q in R.QUANTITIES if q != "p"}
            ids.append(n)
            n += 1
        pgs.append(dict(lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"], max_grad_norm=max_norm,
                        no_prox=h["no_prox"], foreach=True, step=R.K, params=ids))
    return {"state": state, "param_groups": pgs}


def test_state_dict_interchange_with_the_reference_layout(gold, e_ref):
    from lcrnet_amd.adan import Adan
    name = "c4"
    groups, max_norm = R.case_groups(name)
    params, grads, opt = build_optimizer(name, Adan, fused=False)
    set_grads(params, grads[0])
    opt.step()
    sd = opt.state_dict()
    assert sorted(sd) == gold.z["state_dict_keys"].tolist()
    assert sorted(sd["param_groups"][0]) == gold.z["state_dict_group_keys"].tolist()
    assert sorted(sd["state"][0]) == gold.z["state_dict_state_keys"].tolist() == sorted(R.QUANTITIES[1:])
    # a reference-format state_dict of the golden's last step loads, and step K + 1 is the restatement's
    order = [i for idx, _ in groups for i in idx]
    with torch.no_grad():
        for n, i in enumerate(order):
            params[i].copy_(torch.from_numpy(gold.get(name, "single", R.K, "p", i).copy()))
    opt.load_state_dict(reference_state_dict(gold, name))
    assert [g["step"] for g in opt.param_groups] == [R.K, R.K]
    rng = np.random.RandomState(77)
    extra = [(1.3 * rng.randn(n)).astype(np.float32) for n in R.SIZES]
    st = R.new_state([gold.get(name, "single", R.K, "p", i) for i in range(len(R.SIZES))])
    for i, s in enumerate(st["tensors"]):
        s.update({q: gold.get(name, "single", R.K, q, i).astype(np.float64) for q in R.QUANTITIES[1:]})
    st["steps"] = {gi: R.K for gi in range(len(groups))}
    R.step(st, groups, max_norm, extra)
    set_grads(params, extra)
    opt.step()
    fig = figures(params, opt, R.snapshot(st), e_ref, name)
    print(fig)
    assert all(v <= 1 for v in fig.values()), fig
    # restart_opt: zero moments, step 0, and the next step is a first step
    opt.restart_opt()
    assert all(g["step"] == 0 for g in opt.param_groups) and not opt.state[params[0]]["exp_avg"].any()
    set_grads(params, extra)
    opt.step()
    assert all(not opt.state[p]["exp_avg_diff"].any() for p in params)


def test_constructor_validation_and_config():
    from lcrnet_amd.adan import Adan
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-1e-3), dict(betas=(1.0, 0.9, 0.9)), dict(betas=(0.9, -0.1, 0.9)), dict(betas=(0.9, 0.9, 1.5)), dict(max_grad_norm=-1.0),
               dict(eps=-1e-8), dict(fused="yes")):
        with pytest.raises(ValueError):
            Adan(p, **kw)
    with pytest.raises(RuntimeError):                                     # fused=True refuses what the kernel cannot take
        opt = Adan(p, fused=True)
        p[0].grad = torch.ones(3)
        opt.step()
    cfg = make_cfg()
    assert cfg["optimadan"] == {"lr": 1e-4, "lr_decay": 0.95, "lr_decay_steps": 4, "weight_decay": 1e-6, "opt_betas": None, "opt_eps": None,
                                "max_grad_norm": 0, "no_prox": False}
    opt = Adan.from_cfg(p, cfg)
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["betas"], g["eps"], g["max_grad_norm"], g["no_prox"], g["foreach"]) == \
        (1e-4, 1e-6, (0.98, 0.92, 0.99), 1e-8, 0, False, True)
    q = torch.nn.Parameter(torch.ones(4))                                 # a parameter without a gradient keeps no state
    opt = Adan([p[0], q], fused=False)
    p[0].grad = torch.ones(3)
    opt.step()
    assert len(opt.state[q]) == 0 and torch.equal(q.detach(), torch.ones(4)) and opt.param_groups[0]["step"] == 1


def test_entry_points_refuse_bad_tables_without_a_gpu():
    """T < 0, numel < 0, a null pointer with numel > 0, a pointer that is not 4-byte aligned and a short workspace are refused before any
    launch; T == 0 workspace queries and numel == 0 entries are legal."""
    from lcrnet_amd import functional as F
    lib = F._L()
    hyper = F.AdanHyper(beta1=0.98, beta2=0.92, beta3=0.99, bias1=0.02, bias2=0.08, bias3_sqrt=0.1, lr=1e-3, weight_decay=0.0, eps=1e-8,
                        no_prox=0)
    assert ctypes.sizeof(F.AdanHyper) == 80 and F.ADAN_TENSOR_WORDS * 8 == 64

    def table(rows):
        return np.array(rows, dtype=np.int64).reshape(-1, F.ADAN_TENSOR_WORDS)

    good = [4096, 8192, 12288, 16384, 20480, 24576, 10, 0]
    nbytes = ctypes.c_size_t(0)
    assert lib.lcr_adan_ws_bytes(table(good).ctypes.data, 1, ctypes.byref(nbytes)) == 0 and nbytes.value >= 8
    assert lib.lcr_adan_ws_bytes(None, 0, ctypes.byref(nbytes)) == 0
    big = table([good[:6] + [3 * 4096 + 1, 0], good[:6] + [0, 0], good[:6] + [4096, 0]])
    assert lib.lcr_adan_ws_bytes(big.ctypes.data, 3, ctypes.byref(nbytes)) == 0 and nbytes.value >= 5 * 8      # 4 + 0 + 1 chunks
    assert lib.lcr_adan_ws_bytes(table(good).ctypes.data, -1, ctypes.byref(nbytes)) != 0
    out = ctypes.c_void_p(4096)
    for bad in ([4096, 8192, 12288, 16384, 20480, 24576, -1, 0],           # numel < 0
                [4096, 0, 12288, 16384, 20480, 24576, 10, 0],              # null gradient
                [4096, 8194, 12288, 16384, 20480, 24576, 10, 0]):          # gradient at a 2-byte offset
        t = table(bad)
        assert lib.lcr_adan_ws_bytes(t.ctypes.data, 1, ctypes.byref(nbytes)) != 0
        assert lib.lcr_adan_grad_norm(t.ctypes.data, 1, 1.0, 1e-8, out, out, 1 << 20, None) != 0
        assert lib.lcr_adan_step(t.ctypes.data, 1, ctypes.addressof(hyper), None, None) != 0
        assert b"tensor 0" in lib.lcr_last_error()
    for col in (0, 2, 3, 4, 5):                                            # the other five arrays: null, then misaligned
        for v in (0, good[col] + 1):
            t = table(good)
            t[0, col] = v
            assert lib.lcr_adan_step(t.ctypes.data, 1, ctypes.addressof(hyper), None, None) != 0
    assert lib.lcr_adan_step(table(good).ctypes.data, -2, ctypes.addressof(hyper), None, None) != 0
    assert lib.lcr_adan_step(table(good).ctypes.data, 1, None, None, None) != 0
    assert lib.lcr_adan_grad_norm(big.ctypes.data, 3, 1.0, 1e-8, out, out, 4 * 8, None) != 0                     # 5 partials do not fit
    assert lib.lcr_adan_grad_norm(table(good).ctypes.data, 1, -1.0, 1e-8, out, out, 1 << 20, None) != 0
    assert lib.lcr_adan_grad_norm(table(good).ctypes.data, 1, 1.0, 1e-8, None, out, 1 << 20, None) != 0
