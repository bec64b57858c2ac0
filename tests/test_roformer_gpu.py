"""GPU: the forward kernels of the 3D-RoFormer (csrc/attention.hip: k_rotary, k_attention, k_attention_seg, k_add_layernorm, k_relu_inplace,
and the Linears around them) against the fp64 restatements of tests/roformer_restatement.py, called through the C entries.

Tolerance rule (R.bound), unchanged everywhere: max|got - w64| <= max(4 e_ref, 2^-20 max|w64|), e_ref being the error of fp32 torch through
the reference's formula on the same fp32 inputs (computed here, on the CPU), per output tensor of a launch.  Every test prints err / tol and err / e_ref; the
attention stacks print them per problem as well.  test_roformer_cpu.py shows that each planted mistake of the restatement file moves these
cases by at least 20 tolerances.  Exact: alone-versus-stack, dense-versus-stacked entry and run-to-run bytes, zero-query problems, theta = 0, ReLU.
Outputs are NaN-filled and sit between canaries; refusals return LCR_EARG with a message and leave them NaN.

Measured on the MI355X (LABNOTES R20.1): attention 0.13 - 0.34 of the tolerance over the six value regimes (0.5 - 1.3 of the fp32 reference's
own error), rotary <= 0.10 up to |theta| = 5e4 rad, LayerNorm <= 0.27, the Linears <= 0.82, layers and whole transformer <= 0.36.  Before
k_add_layernorm corrected its mean, the constant rows of test_add_layernorm_forward failed at 18 - 93 tolerances (D = 100, 1000, 1024) and a
tiny_spread row at 3.1."""
import ctypes
import os
import sys

import pytest
import torch

import roformer_restatement as R
from lcrnet_amd import _lib
from lcrnet_amd import functional as F
from test_attention_grad_gpu import _over, guarded, intact, same_bytes

pytestmark = pytest.mark.gpu
LCR_EARG = -1
SPARE_ROWS = 3                                # rows of the guarded output past the last query: they must stay NaN


def check(label, got, w64, w32):
    """print err / tol and err / e_ref, then hold `got` to R.bound"""
    w64 = w64.double()
    err, e_ref = (got.detach().cpu().double() - w64).abs().max().item(), (w32.double() - w64).abs().max().item()
    tol = R.bound(e_ref, w64.abs().max().item())
    print("%-64s err %.3e  tol %.3e  err/tol %6.3f  err/e_ref %8.3f" % (label, err, tol, err / tol if tol > 0 else 0.0, _over(err, e_ref)))
    assert bool(torch.isfinite(got).all()), label + ": not finite"
    assert err <= tol, (label, err, tol)


def _lens(values):
    return ctypes.cast((ctypes.c_int64 * len(values))(*[int(x) for x in values]), ctypes.c_void_p)


def _dev(t):
    """the tensor on the device; an empty one still gets a pointer that is not null"""
    return t.cuda().contiguous() if t.numel() else torch.zeros((1, t.shape[1]), device="cuda")


def run_attention(q, k, v, heads, q_lens=None, k_lens=None):
    """lcr_attention_seg_f32 (lcr_attention_f32 without lens) into a NaN-filled guarded buffer -> out on the CPU"""
    qd, kd, vd = _dev(q), _dev(k), _dev(v)
    nq, w = q.shape[0], heads * 32
    t, out = guarded((nq + SPARE_ROWS, w))
    stream = _lib.stream_ptr(qd.device)
    if q_lens is None:
        _lib.call.lcr_attention_f32(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), nq, k.shape[0], heads, 32, _lib.ptr(out), stream)
    else:
        assert sum(q_lens) == nq and sum(k_lens) == k.shape[0]
        _lib.call.lcr_attention_seg_f32(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), _lens(q_lens), _lens(k_lens), len(q_lens), heads, 32, _lib.ptr(out), stream)
    torch.cuda.synchronize()
    assert intact(t), "a canary was overwritten"
    assert bool(torch.isnan(out[nq:]).all()), "rows past the last query were written"
    return out[:nq].cpu()


class Stack:
    """one value regime over the edge grid in ONE launch, its fp64 result and its tolerance; made once, never modified"""

    def __init__(self, regime, heads):
        self.heads = heads
        self.q, self.k, self.v, self.q_lens, self.k_lens = R.attention_stack(regime, heads)
        self.want, self.e_ref, self.tol, self.rows = R.attention_reference(self.q, self.k, self.v, heads, self.q_lens, self.k_lens)
        self.got = run_attention(self.q, self.k, self.v, heads, self.q_lens, self.k_lens)


_STACKS = {}


def stack(regime, heads=4):
    if (regime, heads) not in _STACKS:
        _STACKS[regime, heads] = Stack(regime, heads)
    return _STACKS[regime, heads]


# ---- attention: every value regime over the edge grid ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,regime", [(4, r) for r in R.REGIMES] + [(1, "unit"), (8, "unit")])
def test_attention_stack_within_the_fp32_reference_error(heads, regime):
    s = stack(regime, heads)
    for (qs, e_ref), (nq, nk) in zip(s.rows, R.GRID):
        err = (s.got[qs].double() - s.want[qs]).abs().max().item()
        print("attention %-9s heads=%d  %3d x %3d  err %.3e  err/tol %6.3f  err/e_ref of these rows %8.3f" % (regime, heads, nq, nk, err, err / s.tol, _over(err, e_ref)))
    err = (s.got.double() - s.want).abs().max().item()
    print("attention %-9s heads=%d  the stack   err %.3e  tol %.3e  err/tol %6.3f  err/e_ref %8.3f" % (regime, heads, err, s.tol, err / s.tol, _over(err, s.e_ref)))
    assert bool(torch.isfinite(s.got).all())
    assert err <= s.tol, (regime, heads, err, s.tol)


CHOSEN = [0, 3, 11, 16, 20]                      # 33 x 1, 33 x 33, 33 x 129, 33 x 257, 65 x 97


@pytest.mark.parametrize("regime", ["unit", "two_peaks"])
def test_a_problem_alone_and_through_the_dense_entry_gives_its_bytes_in_the_stack(regime):
    s = stack(regime)
    probs = R._problems(s.q.shape[0], s.k.shape[0], s.q_lens, s.k_lens)
    for p in CHOSEN:
        qs, ks = probs[p]
        alone = run_attention(s.q[qs], s.k[ks], s.v[ks], s.heads, [s.q_lens[p]], [s.k_lens[p]])
        dense = run_attention(s.q[qs], s.k[ks], s.v[ks], s.heads)
        assert same_bytes(alone, s.got[qs]), ("alone", R.GRID[p])
        assert same_bytes(dense, alone), ("lcr_attention_f32 against lcr_attention_seg_f32 with P = 1", R.GRID[p])


def test_a_second_run_of_the_stack_gives_the_same_bytes():
    s = stack("unit")
    assert same_bytes(run_attention(s.q, s.k, s.v, s.heads, s.q_lens, s.k_lens), s.got)


# ---- attention: the shape of the stack ------------------------------------------------------------------------------------------------------
def test_sixty_four_small_problems_in_one_launch():
    problems = [(1 + i % 9, 1 + (i + 4) % 9) for i in range(64)]
    q, k, v, ql, kl = R.attention_stack("unit", 4, problems, seed=64)
    want, e_ref, tol, _ = R.attention_reference(q, k, v, 4, ql, kl)
    got = run_attention(q, k, v, 4, ql, kl)
    err = (got.double() - want).abs().max().item()
    print("attention P=64 (1..9 rows): err %.3e  tol %.3e  err/tol %.3f  err/e_ref %.2f" % (err, tol, err / tol, _over(err, e_ref)))
    assert bool(torch.isfinite(got).all()) and err <= tol


def test_zero_query_problems_leave_their_neighbours_bytes():
    base = [(33, 65), (5, 7), (40, 129), (1, 3)]
    q, k, v, ql, kl = R.attention_stack("unit", 4, base, seed=5)
    want = run_attention(q, k, v, 4, ql, kl)
    g = torch.Generator().manual_seed(6)
    extra = [torch.randn(n, 128, generator=g) for n in (2, 40, 33)]                    # the keys of the three zero-query problems
    ks = list(torch.split(k, kl))
    vs = list(torch.split(v, kl))
    for where in ([0], [2], [4], [0, 2, 4]):                                           # first, middle, last, all three (positions in the base list)
        ql2, k2, v2, n = [], [], [], 0
        for p in range(len(base) + 1):
            if p in where:
                ql2.append(0), k2.append(extra[n]), v2.append(extra[n] * 0.5)
                n += 1
            if p < len(base):
                ql2.append(ql[p]), k2.append(ks[p]), v2.append(vs[p])
        got = run_attention(q, torch.cat(k2), torch.cat(v2), 4, ql2, [t.shape[0] for t in k2])
        assert same_bytes(got, want), where


def test_no_queries_at_all_is_ok_and_writes_nothing():
    g = torch.Generator().manual_seed(7)
    k = torch.randn(12, 128, generator=g)
    empty = torch.zeros(0, 128)
    assert run_attention(empty, k, k, 4, [0, 0], [5, 7]).shape[0] == 0                 # run_attention asserts the spare rows stay NaN
    assert run_attention(empty, k, k, 4).shape[0] == 0


def test_calls_outside_the_domain_are_refused_and_write_nothing():
    L = _lib.lib()
    g = torch.Generator().manual_seed(8)
    q = torch.randn(40, 128, generator=g).cuda()
    t, out = guarded((40, 128))
    p, o, st = _lib.ptr(q), _lib.ptr(out), _lib.stream_ptr(q.device)
    one65, one0 = [1] * 65, [1] * 64
    seg = [("P = 65", (p, p, p, _lens(one65), _lens(one65), 65, 4, 32, o, st)),
           ("P = 0", (p, p, p, _lens([1]), _lens([1]), 0, 4, 32, o, st)),
           ("a problem without keys", (p, p, p, _lens([3, 4]), _lens([5, 0]), 2, 4, 32, o, st)),
           ("head_dim 64", (p, p, p, _lens([3]), _lens([5]), 1, 2, 64, o, st)),
           ("null q", (None, p, p, _lens([3]), _lens([5]), 1, 4, 32, o, st)),
           ("null out", (p, p, p, _lens([3]), _lens([5]), 1, 4, 32, None, st)),
           ("null lens", (p, p, p, None, _lens([5]), 1, 4, 32, o, st))]
    for what, args in seg:
        assert L.lcr_attention_seg_f32(*args) == LCR_EARG, what
        assert b"lcr_attention_seg_f32" in L.lcr_last_error(), what
    dense = [("Nk = 0", (p, p, p, 3, 0, 4, 32, o, st)), ("head_dim 16", (p, p, p, 3, 5, 4, 16, o, st)), ("null k", (p, None, p, 3, 5, 4, 32, o, st))]
    for what, args in dense:
        assert L.lcr_attention_f32(*args) == LCR_EARG, what
        assert b"lcr_attention_f32" in L.lcr_last_error(), what
    assert L.lcr_attention_seg_f32(p, p, p, _lens(one0), _lens(one0), 64, 4, 32, None, st) == LCR_EARG
    torch.cuda.synchronize()
    assert intact(t) and bool(torch.isnan(out).all()), "a refused call wrote"


# ---- rotary ---------------------------------------------------------------------------------------------------------------------------------
def run_rotary(x, theta, heads):
    t, xd = guarded(x.shape)
    xd.copy_(x)
    th = theta.cuda().contiguous()
    _lib.call.lcr_rotary_embed(_lib.ptr(xd), _lib.ptr(th), x.shape[0], heads, _lib.stream_ptr(th.device))
    torch.cuda.synchronize()
    assert intact(t), "a canary was overwritten"
    return xd.cpu()


# 16 421 rows x 64 pairs is past the 4096 x 256 threads of the capped grid: the stride loop runs
@pytest.mark.parametrize("scale", R.ROTARY_SCALES)
@pytest.mark.parametrize("n,heads", [(1, 4), (37, 4), (16421, 4), (37, 1), (37, 8)])
def test_rotary_against_fp64_sin_and_cos_of_the_fp32_theta(n, heads, scale):
    x, th = R.rotary_case(n, heads, scale, n + heads)
    assert n * heads * 16 > 4096 * 256 or n < 16421
    got = run_rotary(x, th, heads)
    check("rotary N=%d heads=%d theta x %g (|theta| max %.0f)" % (n, heads, scale, th.abs().max().item()), got, R.rotary_forward(x, th), R.rotary_formula(x, th, heads))
    assert same_bytes(F.rotary_embed(x.cuda(), th.cuda(), heads).cpu(), got), "the out-of-place wrapper gives the in-place bytes"


def test_rotary_by_zero_returns_the_input_bytes():
    x, _ = R.rotary_case(300, 4, 1.0, 9)
    assert same_bytes(run_rotary(x, torch.zeros(300, 64), 4), x)


# ---- LayerNorm(a + b) -----------------------------------------------------------------------------------------------------------------------
def run_add_layernorm(a, b, gamma, beta):
    ad, bd, gd, be = a.cuda().contiguous(), (None if b is None else b.cuda().contiguous()), gamma.cuda(), beta.cuda()
    t, y = guarded(a.shape)
    _lib.call.lcr_add_layernorm(_lib.ptr(ad), _lib.ptr(bd), _lib.ptr(gd), _lib.ptr(be), a.shape[0], a.shape[1], 1e-5, _lib.ptr(y), _lib.stream_ptr(ad.device))
    torch.cuda.synchronize()
    assert intact(t), "a canary was overwritten"
    return y.cpu()


# 16 421 rows are past the 4096 x 4 rows of the capped grid
@pytest.mark.parametrize("n,d", [(n, d) for d in (1, 32, 100, 128, 256, 1000, 1024) for n in (1, 37)] + [(16421, 128)])
def test_add_layernorm_forward(n, d):
    failed = []
    for kind in R.ROW_KINDS:
        for with_b in (False, True):
            a, b, gamma, beta = R.layernorm_case(kind, n, d, with_b, n + d)
            got = run_add_layernorm(a, b, gamma, beta)
            try:
                check("layernorm %-11s N=%d D=%d b=%s" % (kind, n, d, with_b), got, R.add_layernorm_forward(a, b, gamma, beta),
                      R.add_layernorm_formula(a, b, gamma, beta))
                # a constant row: the residuals of the first mean are all the same few ulps, their sum and its division by D are exact, the
                # corrected mean is the constant itself and y is beta to the bit (before the correction step: beta + up to 3e-4 gamma)
                assert kind != "constant" or torch.equal(got, beta.expand(n, d)), "a constant row gives beta exactly"
            except AssertionError as e:                               # every kind is printed before the test fails
                failed.append(e.args[0])
    assert not failed, failed


def test_add_layernorm_refuses_more_than_1024_features():
    a = torch.randn(2, 1025).cuda()
    t, y = guarded((2, 1025))
    assert _lib.lib().lcr_add_layernorm(_lib.ptr(a), None, _lib.ptr(a), _lib.ptr(a), 2, 1025, 1e-5, _lib.ptr(y), _lib.stream_ptr(a.device)) == LCR_EARG
    assert b"lcr_add_layernorm" in _lib.lib().lcr_last_error()
    torch.cuda.synchronize()
    assert intact(t) and bool(torch.isnan(y).all())


# ---- ReLU -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2 ** 20 + 5])                                    # 2^20 + 5 is past the 4096 x 256 threads of the capped grid
def test_relu_in_place_equals_clamp(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(max(n, 1), generator=g)
    x[::7] = 0.0
    x[3::11] = -0.0
    if n == 1:
        x[0] = -1.5
    t, xd = guarded((max(n, 1),))
    xd.copy_(x)
    _lib.call.lcr_relu_inplace(_lib.ptr(xd), n, _lib.stream_ptr(xd.device))
    torch.cuda.synchronize()
    assert intact(t)
    want = torch.clamp(x, min=0) if n else x
    assert torch.equal(xd.cpu(), want), "values equal torch.clamp(min=0) (the sign of zero aside)"


# ---- F.linear at the transformer's shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 37, 300])
@pytest.mark.parametrize("cin,cout,relu", [(3, 128, False), (128, 64, False), (1024, 128, False), (128, 128, False), (128, 256, True), (256, 128, False)])
def test_linear_forward(cin, cout, relu, rows):
    g = torch.Generator().manual_seed(rows + cin + cout)
    x, w, b = torch.randn(rows, cin, generator=g), torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    ref = lambda dt: (lambda y: torch.relu(y) if relu else y)(torch.nn.functional.linear(x.to(dt), w.to(dt), b.to(dt)))
    with torch.no_grad():
        got = F.linear(x.cuda(), w.cuda(), b.cuda(), relu=relu)
    check("linear %4d x %4d -> %3d relu=%s" % (rows, cin, cout, relu), got, ref(torch.float64), ref(torch.float32))


# ---- composite: one layer and the whole transformer, at the theta the model really runs -------------------------------------------------------
def _golden_module():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_roformer_grad as mg
    return mg


_MODEL = {}


def model():
    """the seeded model of the gradient golden: (module on the device, fp32 state dict, fp64 state dict, config)"""
    if not _MODEL:
        from lcrnet_amd.modules.thdroformer.thdroformer_linear import ThDRoFormer
        from lcrnet_amd.weights import seeded_state_dict
        mg = _golden_module()
        m = ThDRoFormer(*mg.CONFIG)
        sd = seeded_state_dict(m.state_dict(), mg.SEED)
        m.load_state_dict(sd, strict=True)
        _MODEL["m"] = (m.cuda().eval(), {k: v.float() for k, v in sd.items()}, {k: v.double() for k, v in sd.items()}, mg.CONFIG)
    return _MODEL["m"]


PAIRS = [([37], [45]), ([37, 1, 64], [45, 33, 2])]


def _theta32(sd32, pts):
    return torch.nn.functional.linear(torch.nn.functional.linear(pts, sd32["embedding.encoder.weight"], sd32["embedding.encoder.bias"]),
                                      sd32["embedding.encoder2.weight"], sd32["embedding.encoder2.bias"])


def _per_pair(fn, lens_x, lens_m, x, mem, *more):
    """torch_ref knows one pair: run `fn` pair by pair over the stacks and stack the results"""
    outs, ox, om = [], 0, 0
    for a, b in zip(lens_x, lens_m):
        outs.append(fn(x[ox:ox + a], mem[om:om + b], *[t[ox:ox + a] for t in more]))
        ox, om = ox + a, om + b
    return torch.cat(outs)


@pytest.mark.parametrize("lens0,lens1", PAIRS)
def test_one_self_layer(lens0, lens1):
    from oracle import torch_ref
    m, sd32, sd64, config = model()
    p0, _, _, _ = R.composite_inputs(lens0, lens1, config[0], 21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(sum(lens0), config[2], generator=g)
    theta = _theta32(sd32, p0)                                        # the SAME fp32 angles go to the kernel, the fp32 formula and the restatement
    print("self layer: |theta| max %.1f rad" % theta.abs().max().item())
    assert theta.abs().max().item() > 30.0, "the angles are in the range real scans give"
    lens = None if len(lens0) == 1 else lens0
    pfx = "transformer.layers.0."
    with torch.no_grad():
        xd = x.cuda()
        got = m.transformer.layers[0](xd, xd, theta.cuda(), lens, lens)
    w32 = _per_pair(lambda a, b, th: torch_ref.attention_layer(sd32, pfx, a, b, config[3], th), lens0, lens0, x, x, theta)
    check("self layer %s" % (lens0,), got, R.layer_forward(sd64, pfx, x, x, config[3], theta, lens, lens), w32)


@pytest.mark.parametrize("lens0,lens1", PAIRS)
def test_one_cross_layer(lens0, lens1):
    from oracle import torch_ref
    m, sd32, sd64, config = model()
    g = torch.Generator().manual_seed(23)
    x, mem = torch.randn(sum(lens0), config[2], generator=g), torch.randn(sum(lens1), config[2], generator=g)
    single = len(lens0) == 1
    pfx = "transformer.layers.1."
    with torch.no_grad():
        got = m.transformer.layers[1](x.cuda(), mem.cuda(), None, None if single else lens0, None if single else lens1)
    w32 = _per_pair(lambda a, b: torch_ref.attention_layer(sd32, pfx, a, b, config[3]), lens0, lens1, x, mem)
    check("cross layer %s x %s" % (lens0, lens1), got, R.layer_forward(sd64, pfx, x, mem, config[3], None, None if single else lens0, None if single else lens1), w32)


@pytest.mark.parametrize("lens0,lens1", PAIRS)
def test_the_whole_transformer_on_the_native_path(lens0, lens1):
    from oracle import torch_ref
    m, sd32, sd64, config = model()
    p0, p1, f0, f1 = R.composite_inputs(lens0, lens1, config[0], 24)
    single = len(lens0) == 1
    args = [t.cuda() for t in (p0, p1, f0, f1)] + ([] if single else [lens0, lens1])
    with torch.no_grad():
        got = m(*args, return_pos_emb=True)
    assert "_native_table" in m.__dict__, "under no_grad the model takes the native one-call path"
    want = R.roformer_forward(sd64, p0, p1, f0, f1, config[3], config[4], None if single else lens0, None if single else lens1)
    tmax = max(want[2].abs().max().item(), want[3].abs().max().item())
    print("whole transformer %s x %s: |theta| max %.1f rad" % (lens0, lens1, tmax))
    assert tmax > 30.0, "the angles are in the range real scans give"
    outs0, outs1, o0, o1 = [], [], 0, 0
    for a, b in zip(lens0, lens1):
        w0, w1 = torch_ref.thd_roformer(sd32, p0[o0:o0 + a], p1[o1:o1 + b], f0[o0:o0 + a], f1[o1:o1 + b], pfx="", heads=config[3], num_layers=config[4])
        outs0.append(w0), outs1.append(w1)
        o0, o1 = o0 + a, o1 + b
    w32 = (torch.cat(outs0), torch.cat(outs1), _theta32(sd32, p0), _theta32(sd32, p1))
    for name, g_, w64_, w32_ in zip(("out0", "out1", "theta0", "theta1"), got, want, w32):
        check("whole transformer %s %s" % (lens0, name), g_, w64_, w32_)
