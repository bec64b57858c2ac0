"""GPU: every form lcr_gemm_f32 can dispatch to (csrc/gemm_f32.hip, csrc/gemm_deep.hip), at test-sized shapes, against the fp64 product.

The forced tiles 1..5 (lcr_gemm_debug_force_tile) are the only way to the 128x128, 128x64 and 64x128 instantiations at such shapes and the
scalar loaders (VEC = false) are only reached by operands whose leading dimension is no multiple of four floats; the rest of the suite
reaches neither.  Shapes: M = 132, N = 200, K = 104 — M and N ragged against every tile, four K-steps with a partial last one (the
branch-free body and both tails of the K loop run), M % 4 == 0 so that trans_a stays on the vector loaders; the scalar form at
M = 131, N = 199, K = 102.  Every form runs once with bias + rowdiv + GroupNorm statistics (groups = 8, N = 256, three segments with a
one-row one in the middle) and once with no epilogue.

Outputs are held to the project's bound, er.NORTH_STAR x max(1, |want|max), against the fp64 product of the same fp32 operands (randn
and 0.05 randn, as in the stream-K test); the statistics to the same bound through check_moments (its `offset` branch: the tighter
centred tolerances of encoder_ops_restatement are CPU fp32 floors of ITS cases, and no floor was measured for these).  Where N > 32 the
K-deep form is bit-identical to the forced 64x64 tile (same K pairing and summation order: the kernel's comment), as
test_k_deep_gemm_form asserts at large shapes.

K <= 256 without trans_a is the light form whatever lcr_gemm_debug_streamk says (gemm_form asks for it first), so the stream-K case runs
K = 128 as a dispatch check and K = 288, the smallest K-step multiple beyond the light form, on the stream-K kernel itself."""
import ctypes
import functools

import pytest
import torch

import encoder_ops_restatement as er
from test_encoder_ops_gpu import check_close, check_moments

pytestmark = pytest.mark.gpu

M_V, N_V, K_V = 132, 200, 104          # vector forms
M_S, N_S, K_S = 131, 199, 102          # scalar form: no leading dimension is a multiple of four
N_EP, GROUPS = 256, 8                  # the runs with an epilogue


def hooks():
    from lcrnet_amd import _lib
    return ctypes.CDLL(_lib.LIB_PATH)


def reset(lib):
    lib.lcr_gemm_debug_force_tile(0)
    lib.lcr_gemm_debug_deep(-1)
    lib.lcr_gemm_debug_streamk(-1)


def seg_of(M):
    return (50, 1, M - 51)


@functools.lru_cache(maxsize=None)
def problem(M, N, K, epilogue):
    """Host operands a [M,K], b [K,N] (+ bias, rowdiv) and the fp64 result with its (mean, variance) per (segment, group); made once."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + int(epilogue))
    a = torch.randn(M, K, generator=g)
    b = torch.randn(K, N, generator=g) * 0.05
    want = a.double() @ b.double()
    if not epilogue:
        return dict(a=a, b=b, bias=None, rowdiv=None, want=want)
    bias = torch.randn(N, generator=g)
    rowdiv = torch.randint(1, 40, (M,), generator=g).float()
    want = want / rowdiv.double()[:, None] + bias.double()
    mean, var = er.gn_moments(want, seg_of(M), GROUPS)
    return dict(a=a, b=b, bias=bias, rowdiv=rowdiv, want=want, mean=mean, var=var)


def run(form, M, N, K, trans_a, trans_b, epilogue):
    """One lcr_gemm_f32 call under the hooks the caller has set, checked against fp64; returns C."""
    from lcrnet_amd import functional as F
    p = problem(M, N, K, epilogue)
    a = (p["a"].t() if trans_a else p["a"]).contiguous().cuda()
    b = (p["b"].t() if trans_b else p["b"]).contiguous().cuda()
    case = f"M={M} N={N} K={K} ta={int(trans_a)} tb={int(trans_b)} epilogue={int(epilogue)}"
    if not epilogue:
        c, stats = F.gemm(a, b, trans_b=trans_b, trans_a=trans_a)
        assert stats is None
    else:
        seg = torch.tensor(seg_of(M), dtype=torch.int64, device="cuda")
        c, stats = F.gemm(a, b, trans_b=trans_b, trans_a=trans_a, bias=p["bias"].cuda(), rowdiv=p["rowdiv"].cuda(), seg_len=seg, groups=GROUPS)
        check_moments(form, case, stats, p["mean"], p["var"], seg_of(M), N // GROUPS, True)
    check_close(form, case, "C", c, p["want"], er.NORTH_STAR)
    return c


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5])
def test_forced_tiles_against_fp64(tile):
    """tile 0: the dispatcher's own choice (K = 104: the light form without trans_a, the 64x64 tile with it); 1..5: 128x128, 128x64, 128x32,
    64x64, 64x128 — each with the four operand layouts."""
    lib = hooks()
    try:
        lib.lcr_gemm_debug_force_tile(tile)
        for trans_a in (False, True):
            for trans_b in (False, True):
                run(f"tile{tile}", M_V, N_V, K_V, trans_a, trans_b, False)
                run(f"tile{tile}", M_V, N_EP, K_V, trans_a, trans_b, True)
    finally:
        reset(lib)


def test_scalar_loaders_against_fp64():
    lib = hooks()
    reset(lib)
    for trans_a in (False, True):
        for trans_b in (False, True):
            run("scalar", M_S, N_S, K_S, trans_a, trans_b, False)
            run("scalar", M_S, N_EP, K_S, trans_a, trans_b, True)


def test_k_deep_form_against_fp64_and_the_64x64_tile():
    lib = hooks()
    try:
        for N, epilogue in ((N_V, False), (N_EP, True)):
            lib.lcr_gemm_debug_deep(2)
            deep = run("deep", M_V, N, 128, False, True, epilogue)
            lib.lcr_gemm_debug_deep(-1)
            lib.lcr_gemm_debug_force_tile(4)
            tile = run("tile4", M_V, N, 128, False, True, epilogue)
            lib.lcr_gemm_debug_force_tile(0)
            assert torch.equal(deep, tile), (N, epilogue)
    finally:
        reset(lib)


@pytest.mark.parametrize("K", [128, 288])
def test_stream_k_switch_against_fp64(K):
    lib = hooks()
    try:
        lib.lcr_gemm_debug_streamk(2)
        run("streamk", M_V, N_V, K, False, False, False)
        run("streamk", M_V, N_EP, K, False, False, True)
    finally:
        reset(lib)


def test_bmm_nt_two_problems_against_fp64():
    from lcrnet_amd import functional as F
    g = torch.Generator().manual_seed(7)
    a = torch.randn(2, M_V, K_V, generator=g)
    b = torch.randn(2, N_V, K_V, generator=g) * 0.05
    c = F.bmm_nt(a.cuda(), b.cuda())
    check_close("bmm_nt", f"P=2 M={M_V} N={N_V} K={K_V}", "C", c, torch.matmul(a.double(), b.double().transpose(1, 2)), er.NORTH_STAR)
