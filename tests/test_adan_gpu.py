"""GPU: the fused Adan step and its global gradient norm (csrc/adan.hip behind lcrnet_amd.functional / lcrnet_amd.adan) against the fp64
restatement of tests/adan_restatement.py.

Tolerance rule (R.bound): a float may differ from the restatement by at most 4 x e_ref, e_ref being the error of the reference's own fp32
optimiser against the same restatement (per case and quantity, from tests/golden/adan_golden.npz), with a floor of 2^-20 relative to the
largest magnitude in the tensor.  Exact: exp_avg_diff after a first or fresh step (the old value times beta2), everything of a tensor
without a gradient, and p.grad when nothing is clipped.  Every parameter, gradient and state array is a view inside a buffer with
canaries on both sides (state arrays are handed to the optimiser pre-made; pre_grad starts as NaN, which a first step must not read)."""
import numpy as np
import pytest
import torch

import adan_restatement as R
import lcrnet_amd.losses as L
from lcrnet_amd import functional as F
from lcrnet_amd.adan import Adan
from lcrnet_amd.config import make_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 64
CANARY = 12345.0
CHUNK = 4096
STATE = R.QUANTITIES[1:]
SETTINGS = ("lr", "betas", "eps", "weight_decay", "no_prox")


@pytest.fixture(scope="module")
def e_ref():
    return R.e_ref_table(R.Golden())


class Guarded:
    """Float32 arrays as views inside canary-filled buffers; `off` shifts a view by that many elements (0: 16-byte aligned, odd: 4-byte)."""

    def __init__(self):
        self.full = []

    def buf(self, n, off=0, fill=float("nan")):
        t = torch.full((n + 2 * PAD + 4,), CANARY, dtype=torch.float32, device=DEV)
        assert t.data_ptr() % 16 == 0
        v = t[PAD + off:PAD + off + n]
        v.fill_(fill)
        self.full.append((t, PAD + off, n))
        return v

    def put(self, a, off=0):
        v = self.buf(len(a), off)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        return v

    def check(self):
        torch.cuda.synchronize()
        for t, lo, n in self.full:
            assert bool((t[:lo] == CANARY).all()) and bool((t[lo + n:] == CANARY).all()), "a canary was overwritten"


class Harness:
    """An optimiser over guarded tensors.  groups = [(tensor indices, settings)]; offsets[i] = the element shifts of tensor i's six
    arrays (p, grad, exp_avg, exp_avg_sq, exp_avg_diff, pre_grad)."""

    def __init__(self, groups, max_norm, p0, offsets=None, seed_pre_grad=True, **kw):
        self.gd = Guarded()
        offsets = offsets or [(0,) * 6] * len(p0)
        self.params = [torch.nn.Parameter(self.gd.put(a, o[0])) for a, o in zip(p0, offsets)]
        self.gbuf = [self.gd.buf(len(a), o[1]) for a, o in zip(p0, offsets)]
        pg = [dict(params=[self.params[i] for i in idx], **{k: h[k] for k in SETTINGS}) for idx, h in groups]
        self.opt = Adan(pg, max_grad_norm=max_norm, **kw)
        for p, a, o in zip(self.params, p0, offsets):
            self.opt.state[p] = {"exp_avg": self.gd.buf(len(a), o[2], 0.0), "exp_avg_sq": self.gd.buf(len(a), o[3], 0.0),
                                 "exp_avg_diff": self.gd.buf(len(a), o[4], 0.0)}
            if seed_pre_grad:                                    # NaN: a first step must not read it.  Without it the optimiser makes its own
                self.opt.state[p]["pre_grad"] = self.gd.buf(len(a), o[5])

    def step(self, gk):
        for p, b, g in zip(self.params, self.gbuf, gk):
            if g is None:
                p.grad = None
            else:
                b.copy_(torch.from_numpy(g))
                p.grad = b
        self.opt.step()

    def get(self, q, i):
        p = self.params[i]
        t = p.detach() if q == "p" else p.grad if q == "grad" else self.opt.state[p].get(q)
        return None if t is None else t.cpu().numpy()

    def everything(self):
        out = [self.get(q, i).copy() for i in range(len(self.params)) for q in R.QUANTITIES if self.get(q, i) is not None]
        out += [b.cpu().numpy().copy() for b in self.gbuf]
        if self.opt._norm_buffers is not None:
            out.append(self.opt._norm_buffers[1].cpu().numpy().copy())
        return out


def run_and_compare(groups, max_norm, p0, grads, e_ref, family, offsets=None, what="", seed_pre_grad=True):
    """The fused path step by step against the restatement under the tolerance rule with `family`'s e_ref, plus the exact properties."""
    h = Harness(groups, max_norm, p0, offsets, seed_pre_grad=seed_pre_grad, fused=True)
    want = R.run_groups(groups, max_norm, p0, grads)
    had_grad = [False] * len(p0)
    beta2 = {i: np.float32(s["betas"][1]) for idx, s in groups for i in idx}
    worst = {}
    for k, gk in enumerate(grads):
        before = [[h.get(q, i) for q in R.QUANTITIES] for i in range(len(p0))]
        h.step(gk)
        for i, g in enumerate(gk):
            if g is None:                                        # skipped: parameter and state keep their bytes
                for q, b in zip(R.QUANTITIES, before[i]):
                    now = h.get(q, i)
                    assert (now is None and b is None) or np.array_equal(now.view(np.uint32), b.view(np.uint32)), (what, k, i, q)
                continue
            for q in R.QUANTITIES + ("grad",):
                w = want[k][q][i]
                fam = (family, "pre_grad" if q == "grad" else q)
                ratio = R.err(h.get(q, i), w) / max(R.bound(e_ref[fam], w), 1e-300) if len(w) else 0.0
                worst[q] = max(worst.get(q, 0.0), ratio)
            if want[k]["clip"] >= 1:
                assert np.array_equal(h.get("grad", i).view(np.uint32), g.view(np.uint32)), (what, k, i, "p.grad must be untouched")
            if k == 0 or not had_grad[i]:                        # first or fresh step: exp_avg_diff is exactly the old value times beta2
                assert np.array_equal(h.get("exp_avg_diff", i), before[i][3] * beta2[i]), (what, k, i, "exp_avg_diff on a fresh step")
            had_grad[i] = True
        print(what, "step", k + 1, {q: "%.3g" % v for q, v in worst.items()}, "(error / bound)")
    h.gd.check()
    assert all(v <= 1 for v in worst.values()), (what, worst)
    return h


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_golden_cases_through_the_fused_path(e_ref, name):
    groups, max_norm = R.case_groups(name)
    p0, grads = R.case_inputs(name)
    if name == "c5":                                             # a fifth step that skips a tensor WITH state
        extra = R.family_inputs(R.SIZES, 1, 55)[1][0]
        grads = grads + [[None] + extra[1:]]
    h = run_and_compare(groups, max_norm, p0, grads, e_ref, name, what=name, seed_pre_grad=False)
    assert [g["step"] for g in h.opt.param_groups] == [len(grads)] * len(groups)


SHAPES = (0, 1, 3, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_tails_and_chunk_edges(e_ref, name):
    groups, max_norm = R.case_groups(name)
    groups = [(tuple(range(len(SHAPES))), groups[0][1])]
    p0, grads = R.family_inputs(SHAPES, 2, 21)
    run_and_compare(groups, max_norm, p0, grads, e_ref, name, what=name + " shapes")


def test_many_tiny_tensors_in_several_launches(e_ref):
    sizes = [1 + (7 * i) % 13 for i in range(170)]               # 170 tensors: four step launches, two norm launches
    groups = [(tuple(range(0, 170, 2)), R.case_groups("c4")[0][0][1]), (tuple(range(1, 170, 2)), R.case_groups("c4")[0][1][1])]
    p0, grads = R.family_inputs(sizes, 2, 22)
    run_and_compare(groups, R.case_groups("c4")[1], p0, grads, e_ref, "c4", what="170 tiny tensors")


@pytest.mark.parametrize("mixed", [False, True])
def test_views_at_odd_offsets(e_ref, mixed):
    sizes = (1, 5, 64, 257, CHUNK + 3)
    rng = np.random.RandomState(5)
    offsets = [tuple(int(x) for x in (rng.randint(0, 4, 6) if mixed else 1 + 2 * rng.randint(0, 2, 6))) for _ in sizes]
    if mixed:
        offsets[2], offsets[4] = (0, 0, 0, 0, 0, 1), (0, 3, 0, 0, 0, 0)     # one array off among six aligned ones
    groups, max_norm = R.case_groups("c3")
    groups = [(tuple(range(len(sizes))), groups[0][1])]
    p0, grads = R.family_inputs(sizes, 2, 23)
    run_and_compare(groups, max_norm, p0, grads, e_ref, "c3", offsets=offsets, what="offsets %s" % ("mixed" if mixed else "odd"))


def test_same_inputs_give_the_same_bytes():
    sizes = (3, 65, CHUNK + 1, 2 * CHUNK + 5) + tuple(1 + i % 5 for i in range(60))
    groups, max_norm = R.case_groups("c3")
    groups = [(tuple(range(len(sizes))), groups[0][1])]
    p0, grads = R.family_inputs(sizes, 2, 24)
    runs = []
    for _ in range(2):
        h = Harness(groups, max_norm, p0, fused=True)
        for gk in grads:
            h.step(gk)
        runs.append(h.everything())
        h.gd.check()
    assert len(runs[0]) == len(runs[1]) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*runs))
    # without clipping a tensor's bytes do not depend on the list it is stepped in
    settings = R.case_groups("c2")[0][0][1]
    alone = Harness([((0,), settings)], 0.0, [p0[2]], fused=True)
    order = list(np.random.RandomState(3).permutation(len(sizes)))
    among = Harness([(tuple(range(len(sizes))), settings)], 0.0, [p0[i] for i in order], fused=True)
    for gk in grads:
        alone.step([gk[2]])
        among.step([gk[i] for i in order])
    at = order.index(2)
    for q in R.QUANTITIES:
        assert np.array_equal(alone.get(q, 0).view(np.uint32), among.get(q, at).view(np.uint32)), q


def test_grad_norm_on_its_own():
    sizes = (0, 1, 3, 65, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 5) + tuple(1 + i % 7 for i in range(170))
    gd = Guarded()
    host = R.family_inputs(sizes, 1, 25)[1][0]
    offs = [i % 3 for i in range(len(sizes))]
    grads = [gd.put(g, o) for g, o in zip(host, offs)]
    table = F.adan_table(None, grads, None, None, None, None, None)
    norm64, _ = R.grad_norm(host, 1.0, 1e-8)
    seen = []
    for max_norm in (0.5 * norm64, 2.0 * norm64, 0.0):
        out = gd.buf(2)
        ws = gd.buf(F.adan_ws_bytes(table) // 4)
        F.adan_grad_norm(table, max_norm, 1e-8, torch.device(DEV), norm_clip=out, ws=ws)
        norm, clip = out.cpu().numpy()
        seen.append(out.cpu().numpy().copy())
        want_clip = R.grad_norm(host, max_norm, 1e-8)[1]
        print("max %.4g: norm %.9g (fp64 %.12g) clip %.9g (fp64 %.12g)" % (max_norm, norm, norm64, clip, want_clip))
        assert abs(norm - norm64) <= 2.0 ** -22 * norm64
        if want_clip >= 1:
            assert clip == 1.0
        else:
            assert abs(clip - want_clip) <= 2.0 ** -22 * want_clip and clip < 1
    assert seen[0][0].tobytes() == seen[1][0].tobytes() == seen[2][0].tobytes()           # the norm itself: the same bytes each time
    empty = gd.buf(2)
    F.adan_grad_norm(F.adan_table(None, [], None, None, None, None, None), 3.0, 1e-8, torch.device(DEV), norm_clip=empty, ws=gd.buf(64))
    assert empty.cpu().tolist() == [0.0, 1.0]                                            # the norm of nothing
    gd.check()
    for g, hg in zip(grads, host):
        assert np.array_equal(g.cpu().numpy(), hg)
    # the optimiser with max_grad_norm = 0 launches no norm kernel and leaves the gradients alone
    h = Harness([((0, 1), R.case_groups("c2")[0][0][1])], 0.0, [host[3], host[4]], fused=True)
    h.step([host[3], host[4]])
    assert h.opt._norm_buffers is None and h.opt.grad_norm is None
    assert np.array_equal(h.get("grad", 1), host[4])
    h.gd.check()


def test_fused_equals_the_torch_path_on_the_device(e_ref):
    sizes = (1, 3, 65, 257, CHUNK + 1)
    groups, max_norm = R.case_groups("c4")
    p0, grads = R.family_inputs(sizes, 4, 26)
    a = Harness(groups, max_norm, p0, fused=True)
    worst = {}
    for foreach in (True, False):
        b = Harness(groups, max_norm, p0, fused=False, foreach=foreach)
        for gk in grads:
            if foreach:
                a.step(gk)
            b.step(gk)
        for i in range(len(sizes)):
            for q in R.QUANTITIES + ("grad",):
                w = b.get(q, i)
                worst[q] = max(worst.get(q, 0.0), R.err(a.get(q, i), w) / R.bound(e_ref[("c4", "pre_grad" if q == "grad" else q)], w))
        b.gd.check()
    a.gd.check()
    print({q: "%.3g" % v for q, v in worst.items()}, "(difference / bound)")
    assert all(v <= 1 for v in worst.values()), worst
    with pytest.raises(RuntimeError):                                                    # fused=True refuses a strided parameter
        p = torch.nn.Parameter(torch.zeros(8, 2, device=DEV)[:, 0])
        opt = Adan([p], fused=True)
        p.grad = torch.ones(8, device=DEV)
        opt.step()


def test_step_does_not_synchronise_with_the_host():
    """torch's sync debug mode raises on any synchronising torch call inside step().  The ctypes calls are outside its view: that
    lcr_adan_grad_norm / lcr_adan_step only enqueue launches (no copy, no allocation, no stream or device wait) is established by
    reading csrc/adan.hip."""
    groups, max_norm = R.case_groups("c4")
    p0, grads = R.family_inputs(R.SIZES, 3, 27)
    h = Harness(groups, max_norm, p0, fused=True)
    h.step(grads[0])
    before = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                                               # pragma: no cover
        pytest.skip("this torch build rejects the sync debug mode: %s" % e)
    try:
        h.opt.step()
        h.opt.step()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    h.gd.check()


def test_end_to_end_scores_through_the_gap_loss(e_ref):
    """A leaf tensor of matching scores optimised for 20 steps through lcrnet_amd.losses.gap (GapCore's autograd) with the settings of case
    c1: the loss goes down, and the fused run follows the torch-path run.  Scores: the tolerance rule with c1's e_ref for p.  Losses: a
    loss is a function of the scores, so two runs whose scores differ by at most t per element differ in loss by at most t * sum |dS| to
    first order; that, doubled for the curvature, plus the rule's floor."""
    import losses_restatement as LR
    c = LR.gap_case((2, 4, 4))
    cfg = make_cfg()
    mod = L.gap(cfg)
    settings = R.case_groups("c1")[0][0][1]
    runs = {}
    for fused in (True, False):
        S = torch.nn.Parameter(torch.from_numpy(c["scores"].copy()).to(DEV))
        od = {"pos_node_corr_knn_points": LR.t(c["p_pts"]).to(DEV), "anc_node_corr_knn_points": LR.t(c["q_pts"]).to(DEV),
              "pos_node_corr_knn_masks": LR.t(c["pmask"]).to(DEV), "anc_node_corr_knn_masks": LR.t(c["qmask"]).to(DEV), "matching_scores": S}
        dd = {"transform": LR.t(c["transforms"][0]).to(DEV)}
        opt = Adan([S], fused=fused, **{k: settings[k] for k in SETTINGS})
        traj = []
        for _ in range(20):
            opt.zero_grad()
            loss = mod(od, dd)
            loss.backward()
            traj.append((float(loss.detach()), S.detach().cpu().numpy().copy(), float(S.grad.abs().sum())))
            opt.step()
        runs[fused] = traj
    first, last = runs[True][0][0], runs[True][-1][0]
    print("loss %.6f -> %.6f over 20 fused steps" % (first, last))
    assert last < first and runs[False][-1][0] < runs[False][0][0]
    for (la, sa, ga), (lb, sb, _) in zip(runs[True], runs[False]):
        t = R.bound(e_ref[("c1", "p")], sb)
        assert R.err(sa, sb) <= t
        assert abs(la - lb) <= 2 * t * ga + 2.0 ** -20 * abs(lb)
