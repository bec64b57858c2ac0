"""GPU: the encoder's GroupNorm and KPConv operators (csrc/groupnorm.hip, csrc/kpconv.hip, the statistics epilogue of csrc/gemm.h and the
normalise-on-load form of csrc/gemm_f32.hip), each against the fp64 restatement of tests/encoder_ops_restatement.py — an independent reference, where the
older operator tests compare one HIP form with another.

Inputs, cases and tolerances come from encoder_ops_restatement: TOL[op] = min(1e-4, 4 x the CPU fp32 floor) x max(1, |want|max) for the centred
cases; the offset cases (|mean| / std = 9, twice the worst ratio measured in the encoder) are held to the north star alone,
1e-4 x max(1, |want|max), because one-pass statistics have a floor of their own there.  tests/test_encoder_ops_cpu.py shows without a GPU that
every planted mutation moves the fp64 result by >= 20 TOL on these cases.  Variances are compared relative to (variance + eps), the quantity
the normalisation uses (the CPU floor is taken in the same metric): TOL["gn_var"] for the centred cases, the north star 1e-4 for the
offset ones.

Measured (MI355X; worst figure over every case of this file, as a share of its bound where the bound depends on the case):

    operator / quantity                   | CPU fp32 floor | TOL     | worst GPU error (case)
    groupnorm_stats  mean, centred        | 1.8e-7         | 7.2e-7  | 0 (fp64 sums of <= 64-row partials are exact here)
    groupnorm_stats  variance, centred    | 1.4e-5         | 5.6e-5  | 3.2e-7 (C=32 small)
    groupnorm_stats  variance, offset 9   |                | 1e-4    | 7.3e-5 (C=32 edges64)
    groupnorm_apply  y, centred           | 5.5e-6         | 2.2e-5  | 7.0e-7 = 0.006 of its bound (C=32 empty)
    groupnorm_apply  y, offset 9          |                | 1e-4    | 1.1e-4 = 0.15 of its bound (C=32 empty)
    gemm epilogue    variance, centred    | 1.4e-5         | 5.6e-5  | 1.8e-5 (N=64 edges64)
    gemm epilogue    variance, offset 9   |                | 1e-4    | 2.8e-5 (N=64 mixed)
    gemm epilogue    -> apply             | 5.5e-6         | 2.2e-5  | 3.5e-5 = 0.30 of its bound (N=64 edges64); offset 9: 0.05 of its bound
    gemm_anorm       C                    | 5.8e-7         | 2.3e-6  | 4.4e-7 = 0.03 of its bound (K=4 N=36 M=64)
    gemm_anorm       output variance      | 1.4e-5         | 5.6e-5  | 6.9e-7 (K=64 N=64 M=777)
    kpconv_aggregate A (nn and mask exact)| 2.7e-7         | 1.1e-6  | 4.1e-6 = 0.26 of its bound (C=128 H=128)
    kpconv_fused     out                  | 5.7e-7         | 2.3e-6  | 3.2e-7 = 0.11 of its bound (mixed, H=65)
    kpconv_fused     variance             | 1.4e-5         | 5.6e-5  | 4.3e-7 (empty); offset 9: 5.1e-7
    kpconv_cin1      out                  | 2.5e-7         | 1.0e-6  | 3.0e-7 = 0.19 of its bound (Cout=256 H=100)
    maxpool, row flags, counts            | exact          |         | equal on every row compared

What these tests found, and what was changed for it (figures: before -> after):
  * lcr_groupnorm_stats took three channels per group and returned a wrong table; it now refuses (LCR_EARG).
  * Statistics of groups of one or two values: the fp32 rounding of x^2 stood in for a variance of 0.  variance + eps was off by 8.9e-2
    relative from lcr_groupnorm_stats (C=32 edges64, centred; 1.4e-2 at offset 9, C=64 one) and by 9.5e-2 from the GEMM epilogue (N=32 edges64;
    3.3e-2 at offset 9, N=64 mixed).  Segments shorter than 64 rows (GEMM epilogue: 32) are now summed in fp64 from the first addition: 3.2e-7 / 7.3e-5 and 1.8e-5 / 2.8e-5.
  * lcr_groupnorm_apply in the scale / shift form x a + (beta - mean a) rounded at the size of mean a: 6.8e-3 off fp64 against a bound of
    3.2e-4 (C=64, one row, offset 9), 3.1e-4 against 1.8e-4 centred (C=64 mixed).  It now evaluates (x - mean) a + beta with the mean as
    two floats: 0.15 and 0.006 of the bounds; groups of one value give beta exactly (error 0).
"""
import ctypes

import numpy as np
import pytest
import torch

import encoder_ops_restatement as er

pytestmark = pytest.mark.gpu

EARG = -1
SENTINEL = -7.0
TABLES = tuple(er.SEG_TABLES)


def F():
    from lcrnet_amd import functional
    return functional


def dev(t):
    return None if t is None else t.cuda().contiguous()


def seg_dev(seg_lens):
    return torch.tensor(list(seg_lens), dtype=torch.int64, device="cuda")


def last_error():
    from lcrnet_amd import _lib
    return _lib.lib().lcr_last_error() or b""


def report(op, case, what, err, bound):
    print(f"encoder_ops {op} {case} {what}: err {err:.3e} bound {bound:.3e} ({err / bound:.3f} of it)")


def check_close(op, case, what, got, want, tol):
    """got (device or host, fp32) against the fp64 `want` at tol x max(1, |want|max); finite everywhere.  Prints the figure before asserting."""
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == torch.float32, (op, case, what, got.shape, want.shape)
    assert torch.isfinite(got).all(), (op, case, what)
    bound = tol * max(1.0, want.abs().max().item()) if want.numel() else tol
    err = er.shift_of(got, want)
    report(op, case, what, err, bound)
    assert err <= bound, (op, case, what, err, bound)
    return err


def check_moments(op, case, sums, want_mean, want_var, seg_lens, gs, offset):
    """The (mean, biased variance) a statistics table [replicas, S, groups, 2] stands for, against fp64.  Zero-length segments: untouched zeros."""
    sums = sums.sum(0).cpu()
    assert torch.isfinite(sums).all()
    mean, var = er.moments_from_sums(sums, seg_lens, gs)
    live = torch.tensor([n > 0 for n in seg_lens])
    assert not sums[~live].any(), (op, case)
    tol_m = er.NORTH_STAR if offset else er.TOL["gn_mean"]
    tol_v = er.NORTH_STAR if offset else er.TOL["gn_var"]
    bm = tol_m * max(1.0, want_mean.abs().max().item())
    em = er.shift_of(mean[live], want_mean[live])
    ev = ((var - want_var).abs() / (want_var + er.EPS))[live].max().item()
    report(op, case, "mean", em, bm)
    report(op, case, "variance (relative to variance + eps)", ev, tol_v)
    assert em <= bm and ev <= tol_v, (op, case, em, bm, ev, tol_v)


def check_flags(op, case, got, want_flag, y64):
    """Row flags against the fp64 ones, outside the rows whose sum is a matter of rounding (at most 1 % of the rows)."""
    amb = er.ambiguous_rows(y64)
    assert amb.float().mean().item() <= er.AMBIGUOUS_CAP, (op, case)
    got = got.cpu()
    assert got.dtype == torch.uint8 and bool(((got == 0) | (got == 1)).all())
    wrong = int(((got != 0) != want_flag)[~amb].sum())
    print(f"encoder_ops {op} {case} flags: {wrong} wrong of {int((~amb).sum())} compared ({int(amb.sum())} ambiguous)")
    assert wrong == 0, (op, case, wrong)


def gn_tols(shift):
    return er.NORTH_STAR if shift else er.TOL["gn_apply"]


# ------------------------------------------------------------------------------------------------ GroupNorm statistics: lcr_groupnorm_stats
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("C,groups", er.GN_SHAPES)
def test_groupnorm_stats_against_fp64(C, groups, table):
    for shift in er.SHIFTS:
        c = er.gn_case(C, groups, table, shift)
        case = f"C={C} groups={groups} {table} shift={shift}"
        x, seg = dev(c["x"]), seg_dev(c["seg_lens"])
        stats = F().groupnorm_stats(x, groups, seg)
        mean, var = er.gn_moments_reference(C, groups, table, shift)
        check_moments("groupnorm_stats", case, stats, mean, var, c["seg_lens"], C // groups, shift)
        y = F().groupnorm_apply(x, stats, dev(c["gamma"]), dev(c["beta"]), groups, seg, act=False)
        check_close("groupnorm_stats", case, "-> apply", y, er.gn_reference(C, groups, table, shift, 0, False)[0], gn_tols(shift))


@pytest.mark.parametrize("C,groups", er.GN_NON_POW2)
def test_groupnorm_stats_non_power_of_two_group_is_right_or_refused(C, groups):
    """Three channels per group: the lane fold of k_gn_stats cannot add them; the entry must say so (like the GEMM entries) or be right."""
    from lcrnet_amd import _lib
    seg_lens = er.SEG_TABLES["small"]
    n = sum(seg_lens)
    x = torch.randn(n, C, generator=torch.Generator().manual_seed(C))
    xd, seg = dev(x), seg_dev(seg_lens)
    stats = torch.full((8, len(seg_lens), groups, 2), SENTINEL, dtype=torch.float64, device="cuda")
    rc = _lib.lib().lcr_groupnorm_stats(_lib.ptr(xd), n, C, groups, _lib.ptr(seg), len(seg_lens), _lib.ptr(stats), _lib.stream_ptr(xd.device))
    torch.cuda.synchronize()
    if rc == EARG:
        assert b"lcr_groupnorm_stats" in last_error() and bool((stats == SENTINEL).all())
        with pytest.raises(RuntimeError):
            F().groupnorm_stats(xd, groups, seg)
        return
    assert rc == 0
    got = (stats - SENTINEL).sum(0).cpu()
    want = er.gn_stats(x.double(), seg_lens, groups)
    assert (got - want).abs().max().item() <= er.TOL["gn_mean"] * max(1.0, want.abs().max().item())


# ------------------------------------------------------------------------------------------------ GroupNorm statistics: the GEMM epilogue
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("C,groups", er.GN_SHAPES)
def test_gemm_epilogue_statistics_against_fp64(C, groups, table):
    for shift in er.SHIFTS:
        k = er.gemm_stats_case(C, groups, table, shift)
        case = f"N={C} groups={groups} {table} shift={shift}"
        seg = seg_dev(k["seg_lens"])
        c, stats = F().gemm(dev(k["a"]), dev(k["b"]), trans_b=True, bias=dev(k["bias"]), seg_len=seg, groups=groups)
        c64, mean, var, y64 = er.gemm_stats_reference(C, groups, table, shift)
        check_close("gemm_stats", case, "C", c, c64, er.NORTH_STAR)
        check_moments("gemm_stats", case, stats, mean, var, k["seg_lens"], C // groups, shift)
        y = F().groupnorm_apply(c, stats, dev(k["gamma"]), dev(k["beta"]), groups, seg, act=False)
        check_close("gemm_stats", case, "-> apply", y, y64, gn_tols(shift))


# ------------------------------------------------------------------------------------------------ GroupNorm apply
def _apply_case(C, groups, table, shift, pos_ok):
    c = er.gn_case(C, groups, table, shift)
    x, r, seg = dev(c["x"]), dev(c["res"]), seg_dev(c["seg_lens"])
    ga, be, rg, rb = (dev(c[k]) for k in ("gamma", "beta", "res_gamma", "res_beta"))
    st, rst = F().groupnorm_stats(x, groups, seg), F().groupnorm_stats(r, groups, seg)
    one_value = [(lo, hi) for lo, hi in er._bounds(c["seg_lens"]) if (hi - lo) * (C // groups) == 1]
    for rm in er.RES_MODES:
        for act in (True, False):
            for want_pos in ((True, False) if pos_ok else (False,)):
                case = f"C={C} groups={groups} {table} shift={shift} res={rm} act={int(act)} pos={int(want_pos)}"
                kw = dict(seg_len=seg, act=act, want_pos=want_pos)
                if rm >= 1:
                    kw["res"] = r
                if rm == 2:
                    kw["res_norm"] = (rst, rg, rb)
                got = F().groupnorm_apply(x, st, ga, be, groups, **kw)
                y64, flag64 = er.gn_reference(C, groups, table, shift, rm, act)
                y = got[0] if want_pos else got
                check_close("groupnorm_apply", case, "y", y, y64, gn_tols(shift))
                if one_value and rm == 0 and not act:                # one value per group: the answer is beta
                    rows = torch.cat([torch.arange(lo, hi) for lo, hi in one_value])
                    e1 = er.shift_of(y.cpu()[rows], y64[rows])
                    print(f"encoder_ops groupnorm_apply {case} one-value groups: err {e1:.3e}")
                    assert torch.equal(y.cpu()[rows], c["beta"][None].expand(len(rows), C)), (case, e1)      # x - mean = 0: beta, to the bit
                if want_pos:
                    check_flags("groupnorm_apply", case, got[1], flag64, y64)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_groupnorm_apply_against_fp64(C, table):
    for shift in er.SHIFTS:
        _apply_case(C, 32, table, shift, pos_ok=True)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("C,groups", ((1024, 32),) + er.GN_ODD_SHAPES)
def test_groupnorm_apply_wide_and_odd_channel_counts_against_fp64(C, groups, table):
    """C = 1024 (no row flags) and C / 4 not dividing the workgroup: the general form with a per-element channel offset."""
    for shift in er.SHIFTS:
        _apply_case(C, groups, table, shift, pos_ok=False)


# ------------------------------------------------------------------------------------------------ normalise-on-load GEMM
@pytest.mark.parametrize("K,N,seg_i,with_bias", er.anorm_case_names())
def test_normalise_on_load_gemm_against_fp64(K, N, seg_i, with_bias):
    c = er.anorm_case(K, N, seg_i, with_bias)
    case = f"K={K} N={N} segs={c['seg_lens']} bias={int(with_bias)}"
    a, seg = dev(c["a"]), seg_dev(c["seg_lens"])
    a_stats = F().groupnorm_stats(a, c["a_groups"], seg)
    got, stats = F().gemm_anorm(a, a_stats, dev(c["gamma"]), dev(c["beta"]), c["a_groups"], dev(c["weight"]), bias=dev(c["bias"]), seg_len=seg,
                                groups=c["groups"])
    want, _ = er.anorm_reference(K, N, seg_i, with_bias)
    check_close("gemm_anorm", case, "C", got, want, er.TOL["anorm_gemm"])
    mean, var = er.gn_moments(want, c["seg_lens"], c["groups"])
    check_moments("gemm_anorm", case, stats, mean, var, c["seg_lens"], N // c["groups"], False)
    g2, b2 = torch.linspace(0.5, 1.5, N), torch.linspace(-1, 1, N)
    y = F().groupnorm_apply(got, stats, dev(g2), dev(b2), c["groups"], seg)
    y64, _ = er.gn_apply(want, c["seg_lens"], c["groups"], g2.double(), b2.double())
    check_close("gemm_anorm", case, "-> apply", y, y64, er.TOL["gn_apply"])


# ------------------------------------------------------------------------------------------------ KPConv
def _kp_inputs(c, feats64):
    """Device inputs of a KPConv case; the support flags are the REFERENCE's (fp64 row sums > 0), so that the count is exact on every row —
    lcr_row_positive has its own test."""
    pos = er.row_positive(feats64).to(torch.uint8)
    return dev(c["feats"]), dev(pos), dev(c["q_pts"]), dev(c["s_pts"])


def _variants(c):
    """(label, index tensor, order): int32 and int64 indices, with and without a processing order."""
    for dt in (torch.int32, torch.int64):
        for use_order in (False, True):
            yield f"{'i64' if dt == torch.int64 else 'i32'}{'+order' if use_order else ''}", dev(c["idx"].to(dt)), dev(c["order"]) if use_order else None


@pytest.mark.parametrize("H", er.AGG_H)
@pytest.mark.parametrize("C", er.AGG_C)
def test_kpconv_aggregate_against_fp64(C, H):
    c = er.kpconv_case(C, H)
    A64, cnt64 = er.aggregate_reference(C, H)
    feats, pos, q, s = _kp_inputs(c, c["feats"].double())
    kp, M = er.kernel_points(), c["idx"].shape[0]
    valid = (c["idx"] >= 0) & (c["idx"] < er.KP_NS)
    assert int(cnt64.max()) < int(valid.sum(1).max()) or H == 1           # count != number of valid neighbours somewhere
    for label, idx, order in _variants(c):
        case = f"C={C} H={H} {label}"
        A, nn = F().kpconv_aggregate(feats, pos, q, s, idx, kp, c["sigma"], order=order)
        check_close("kpconv_aggregate", case, "A", A.view(M, 15, C), A64, er.TOL["kpconv_aggregate"])
        assert torch.equal(nn.cpu().double(), cnt64.double()), case            # every row: all-shadow rows 1, non-positive supports not counted
        assert not A.view(M, 15, C)[~valid.any(1)].any()
        # emit_mask: bit k <=> block k holds a non-zero.  Blocks in which a neighbour sits within 1e-5 of the influence's zero crossing may go
        # either way; the blocks of a clear bit are not written
        Am, nm, mask = F().kpconv_aggregate(feats, pos, q, s, idx, kp, c["sigma"], order=order, emit_mask=True)
        bits = ((mask.cpu().to(torch.int32)[:, None] >> torch.arange(15)[None]) & 1).bool()
        assert not (mask.cpu().to(torch.int32) & ~0x7FFF).any() and torch.equal(nm, nn)
        nonzero64 = (A64 != 0).any(2)
        d = (c["s_pts"].double()[c["idx"].clamp(0, er.KP_NS - 1)] - c["q_pts"].double()[:, None])[:, :, None, :] - c["kp"].double()[None, None]
        edge = (((1 - d.norm(dim=3) / c["sigma"]).abs() < 1e-5) & valid[:, :, None]).any(1)               # [M,15]
        assert edge.float().mean().item() <= er.AMBIGUOUS_CAP
        assert torch.equal(bits[~edge], nonzero64[~edge]), case
        Am = torch.where(bits[:, :, None], Am.cpu().view(M, 15, C), torch.zeros(()))
        check_close("kpconv_aggregate", case, "A under its mask", Am, A64 * (bits | ~edge)[:, :, None], er.TOL["kpconv_aggregate"])


@pytest.mark.parametrize("groups", er.FUSED_GROUPS)
@pytest.mark.parametrize("table", er.FUSED_TABLES)
def test_kpconv_fused_against_fp64(table, groups):
    for shift in er.SHIFTS:
        c = er.fused_case(table, shift)
        out64, sums64, cnt64 = er.fused_reference(table, shift, groups)
        feats, pos, q, s = _kp_inputs(c, c["feats"].double())
        seg, kp = seg_dev(c["seg_lens"]), er.kernel_points()
        mean, var = er.gn_moments(out64, c["seg_lens"], groups)
        ga, be = torch.linspace(0.5, 1.5, 32), torch.linspace(-1, 1, 32)
        y64, _ = er.gn_apply(out64, c["seg_lens"], groups, ga.double(), be.double())
        for label, idx, order in _variants(c):
            case = f"{table} H={er.FUSED_H[table]} groups={groups} shift={shift} {label}"
            out, stats = F().kpconv_fused(feats, pos, q, s, idx, kp, c["sigma"], dev(c["weights"]), dev(c["bias"]), seg_len=seg, groups=groups,
                                          order=order)
            check_close("kpconv_fused", case, "out", out, out64, er.TOL["kpconv"])
            check_moments("kpconv_fused", case, stats, mean, var, c["seg_lens"], 32 // groups, shift)
            y = F().groupnorm_apply(out, stats, dev(ga), dev(be), groups, seg)
            check_close("kpconv_fused", case, "-> apply", y, y64, gn_tols(shift))


@pytest.mark.parametrize("Cout,H,with_bias", er.cin1_case_names())
def test_kpconv_cin1_against_fp64(Cout, H, with_bias):
    c = er.cin1_case(Cout, H, with_bias)
    out64, cnt64 = er.cin1_reference(Cout, H, with_bias)
    kp = er.kernel_points()
    valid = (c["idx"] >= 0) & (c["idx"] < er.KP_NS)
    empty = ~valid.any(1)
    assert empty.any() and (H == 1 or int(cnt64.max()) < int(valid.sum(1).max()))
    for label, idx, order in _variants(c):
        case = f"Cout={Cout} H={H} bias={int(with_bias)} {label}"
        out = F().kpconv_cin1(dev(c["feats"]), dev(c["q_pts"]), dev(c["s_pts"]), idx, kp, c["sigma"], dev(c["weights"]), dev(c["bias"]), order=order)
        check_close("kpconv_cin1", case, "out", out, out64, er.TOL["kpconv_cin1"])
        want_empty = c["bias"][None].expand(int(empty.sum()), Cout) if with_bias else torch.zeros(int(empty.sum()), Cout)
        assert torch.equal(out.cpu()[empty], want_empty), case                                           # all-shadow rows give the bias, exactly


# ------------------------------------------------------------------------------------------------ max-pool and row flags
@pytest.mark.parametrize("H", er.POOL_H)
@pytest.mark.parametrize("C", er.POOL_C)
def test_maxpool_equals_restatement(C, H):
    for mixed in (False, True):                    # all-negative features: the initial value; mixed signs: every neighbour of a ragged list
        c = er.pool_case(C, H, mixed)
        want = er.pool_reference(C, H, mixed)
        n = ((c["idx"] >= 0) & (c["idx"] < c["x"].shape[0])).sum(1)
        assert bool((want[n == 0] == 0).all()) and bool((want[n < H] >= 0).all())
        if not mixed:
            assert bool((want[n == H] < 0).all()) and bool((want[(n > 0) & (n < H)] == 0).all())
        x = dev(c["x"])
        for label, idx, order in _variants(c):
            got = F().maxpool(x, idx, order=order)
            assert torch.equal(got.cpu().double(), want), (C, H, mixed, label)


@pytest.mark.parametrize("C", [1, 32, 64, 65, 96, 256, 1024])
def test_row_positive_against_fp64(C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(777, C, generator=g)
    x[::5] = -x[::5].abs()
    x[::11] = 0.0
    got = F().row_positive(dev(x))
    check_flags("row_positive", f"C={C}", got, er.row_positive(x.double()), x.double())
    assert not got.cpu()[::11].any()


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_argument_refusals_leave_the_output_alone():
    from lcrnet_amd import _lib
    L = _lib.lib()
    M, Ns, C, H = 8, 16, 32, 129
    g = torch.Generator().manual_seed(3)
    feats, q, s = dev(torch.randn(Ns, C, generator=g)), dev(torch.rand(M, 3, generator=g)), dev(torch.rand(Ns, 3, generator=g))
    pos = torch.ones(Ns, dtype=torch.uint8, device="cuda")
    idx = torch.randint(0, Ns, (M, H), generator=g, dtype=torch.int32).cuda()
    kp = er.kernel_points()
    kpp = ctypes.c_void_p(kp.ctypes.data)
    st = _lib.stream_ptr(feats.device)
    fill = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")
    untouched = lambda *ts: all(bool((t == SENTINEL).all()) for t in ts)

    A, nn = fill(M, 15 * C), fill(M)
    for what, h, feats_c, cc in (("H > 128", H, feats, C), ("C = 48", 9, dev(torch.randn(Ns, 48, generator=g)), 48)):
        Ac = fill(M, 15 * cc)
        rc = L.lcr_kpconv_aggregate(_lib.ptr(feats_c), _lib.ptr(pos), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), 0, M, Ns, h, cc, kpp, 1.2,
                                    _lib.ptr(Ac), _lib.ptr(nn), None, st)
        torch.cuda.synchronize()
        assert rc == EARG and b"lcr_kpconv_aggregate" in last_error() and untouched(Ac, nn), what

    W, out = dev(torch.randn(15, C, C, generator=g)), fill(M, C)
    stats = torch.full((8, 1, 32, 2), SENTINEL, dtype=torch.float64, device="cuda")
    seg = seg_dev((M,))
    rc = L.lcr_kpconv_fused(_lib.ptr(feats), _lib.ptr(pos), _lib.ptr(q), _lib.ptr(s), _lib.ptr(idx), 0, M, Ns, H, C, kpp, 1.2, _lib.ptr(W), None,
                            _lib.ptr(out), _lib.ptr(seg), 1, 32, _lib.ptr(stats), None, st)
    torch.cuda.synchronize()
    assert rc == EARG and b"lcr_kpconv_fused" in last_error() and untouched(out, stats)

    pooled = fill(M, C)
    rc = L.lcr_maxpool(_lib.ptr(feats), _lib.ptr(idx), 0, M, Ns, H, C, _lib.ptr(pooled), None, st)
    torch.cuda.synchronize()
    assert rc == EARG and b"lcr_maxpool" in last_error() and untouched(pooled)

    # row flags need the C / 4 lanes of a row inside one wavefront: C = 1024 with flags is refused, without them it runs
    n, Cw = 70, 1024
    x = dev(torch.randn(n, Cw, generator=g))
    gam, bet = dev(torch.ones(Cw)), dev(torch.zeros(Cw))
    segw = seg_dev((n,))
    gst = F().groupnorm_stats(x, 32, segw)
    y, flags = fill(n, Cw), torch.full((n,), 7, dtype=torch.uint8, device="cuda")

    def apply(flag_ptr):
        rc = L.lcr_groupnorm_apply(_lib.ptr(x), _lib.ptr(gst), _lib.ptr(gam), _lib.ptr(bet), None, None, None, None, _lib.ptr(y), n, Cw, 32,
                                   _lib.ptr(segw), 1, 1e-5, 0.1, 1, flag_ptr, st)
        torch.cuda.synchronize()
        return rc

    assert apply(_lib.ptr(flags)) == EARG and b"lcr_groupnorm_apply" in last_error() and untouched(y) and bool((flags == 7).all())
    with pytest.raises(RuntimeError):
        F().groupnorm_apply(x, gst, gam, bet, 32, segw, want_pos=True)
    assert apply(None) == 0 and bool(torch.isfinite(y).all()) and not untouched(y)
