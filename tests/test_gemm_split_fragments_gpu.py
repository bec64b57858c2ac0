"""GPU: the split-bf16 K-deep GEMM with B fed from the fragment-ordered planes (lcr_split_bf16x3_tiles -> lcr_gemm_f32_bsplit: four
wavefronts per 64 x 64 tile, each 64 rows x 16 columns, B straight from global memory into the MFMA's registers, A through LDS) on the
smallest shapes that reach each edge of that kernel: one K-step (prologue and tail only), even and odd trip counts of the two-step loop,
a last row block inside the second half of a wavefront's rows, empty / partial / full column parts of a tile, more than one column tile,
segment borders inside a tile's second 32 rows, and the row-masked form at each mask granularity."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [1, 63, 64, 65, 129]
NS = [1, 31, 32, 33, 64, 96, 130]
# three segments; borders inside the first tile's second row block (rows 32..63) and, for M = 129, inside the second tile
SEGS = {1: [1], 63: [35, 20, 8], 64: [35, 20, 9], 65: [35, 20, 10], 129: [40, 50, 39]}


def _planar(x):
    from lcrnet_amd import _lib
    n = x.numel()
    planes = torch.empty(3 * n, dtype=torch.int16, device=x.device)
    _lib.check(_lib.lib().lcr_split_bf16x3(_lib.ptr(x), n, _lib.ptr(planes), _lib.stream_ptr(x.device)), "lcr_split_bf16x3")
    return planes


def _sums(c, seg, groups):
    """fp64 [S, groups, 2]: sum and sum of squares of c [M,N] per (row segment, group of N / groups consecutive columns)"""
    out, r0 = [], 0
    for n in seg.tolist():
        blk = c[r0:r0 + n].reshape(n, groups, -1)
        out.append(torch.stack([blk.sum((0, 2)), (blk * blk).sum((0, 2))], -1))
        r0 += n
    return torch.stack(out)


def _groups(N):
    """32 groups where N allows (the groups must divide N into power-of-two sized groups), no statistics elsewhere"""
    return 32 if N % 32 == 0 and ((N // 32) & (N // 32 - 1)) == 0 else 0


@pytest.mark.parametrize("epilogue", [True, False], ids=["rowdiv_bias", "plain"])
@pytest.mark.parametrize("K", [32, 64, 96, 480])
def test_fragment_fed_gemm_against_fp64(K, epilogue):
    """Inputs and bounds of test_gemm_split_gpu.py::test_split_gemm_against_fp64: split error below 3e-6 of max |ref| and below
    max(4 x the fp32 kernel's error, 4e-7); statistics within 1e-6 (sums relative to sqrt(n * sum of squares)) of fp64 sums of the kernel's
    own output, and within 1e-6 of the fp32 kernel's table beyond what the two outputs' difference accounts for (see below)."""
    from lcrnet_amd import _lib, functional as F
    L = _lib.lib()
    dev = torch.device("cuda")
    for M in MS:
        for N in NS:
            g = torch.Generator(device=dev).manual_seed(M + N + K)
            a = torch.randn(M, K, device=dev, generator=g) * (torch.rand(M, 1, device=dev, generator=g) * 4 + 0.01)
            if epilogue:
                a = torch.where(torch.rand(M, K, device=dev, generator=g) < 0.35, torch.zeros_like(a), a.abs())
            b = torch.randn(N, K, device=dev, generator=g) * 0.05
            bias = torch.randn(N, device=dev, generator=g)
            div = (torch.rand(M, device=dev, generator=g) * 40 + 1).floor() if epilogue else None
            seg = torch.tensor(SEGS[M], dtype=torch.int64, device=dev)
            S, groups = seg.numel(), _groups(N)
            planes = F.split_bf16x3(b)
            outs, stats = [], []
            for which in (0, 1):
                c = torch.full((M, N), float("nan"), device=dev)
                st = torch.zeros(8, S, max(groups, 1), 2, dtype=torch.float64, device=dev)
                args = (_lib.ptr(bias) if epilogue else None, _lib.ptr(div) if epilogue else None, _lib.ptr(seg) if groups else None, S, groups,
                        _lib.ptr(st) if groups else None, _lib.stream_ptr(dev))
                if which == 0:
                    _lib.check(L.lcr_gemm_f32(_lib.ptr(a), _lib.ptr(b), _lib.ptr(c), M, N, K, 0, 1, *args), "lcr_gemm_f32")
                else:
                    _lib.check(L.lcr_gemm_f32_bsplit(_lib.ptr(a), _lib.ptr(planes), _lib.ptr(c), M, N, K, *args), "lcr_gemm_f32_bsplit")
                outs.append(c)
                stats.append(st.sum(0))
            ref = a.double() @ b.double().t()
            if epilogue:
                ref = ref / div.double()[:, None] + bias.double()
            scale = ref.abs().max().item()
            e0, e1 = (outs[0].double() - ref).abs().max().item() / scale, (outs[1].double() - ref).abs().max().item() / scale
            tag = "M=%d N=%d K=%d" % (M, N, K)
            print("%s: max err / max |ref|: fp32 MFMA %.2e, split %.2e" % (tag, e0, e1))
            assert torch.isfinite(outs[1]).all(), tag
            assert e1 < 3e-6 and e1 < max(4 * e0, 4e-7), (tag, e0, e1)
            if groups:
                # (1) the split kernel's table against fp64 sums of ITS OWN output: the statistics path alone, whatever the product's rounding
                n_el = seg.double()[:, None] * (N // groups)
                own = _sums(outs[1].double(), seg, groups)
                rel_own = max(((own[..., 0] - stats[1][..., 0]).abs() / (n_el * own[..., 1]).sqrt()).max().item(),
                              ((own[..., 1] - stats[1][..., 1]).abs() / own[..., 1]).max().item())
                # (2) against the fp32 kernel's table.  The two kernels' outputs differ (by <= ~2e-7 of max |ref|, above), and a group of these
                # shapes can be ONE value far below max |ref| (M = 1, 32 groups of 32 columns), where that difference alone is 1e-5 of the value:
                # the tables may differ by what the outputs do, |sum0 - sum1| <= sum |c0 - c1| and |ss0 - ss1| <= sum |c0^2 - c1^2|, plus 1e-6.
                d1 = _sums((outs[0].double() - outs[1].double()).abs(), seg, groups)[..., 0]
                d2 = _sums((outs[0].double() ** 2 - outs[1].double() ** 2).abs().sqrt(), seg, groups)[..., 1]
                den1, den2 = (n_el * stats[0][..., 1]).sqrt(), stats[0][..., 1]
                ex1 = ((stats[0][..., 0] - stats[1][..., 0]).abs() - d1) / den1
                ex2 = ((stats[0][..., 1] - stats[1][..., 1]).abs() - d2) / den2
                rel = max(ex1.max().item(), ex2.max().item())
                print("%s: statistics vs own output %.2e, vs the fp32 kernel's beyond the outputs' difference %.2e" % (tag, rel_own, rel))
                assert rel_own < 1e-6 and rel < 1e-6, (tag, rel_own, rel)


@pytest.mark.parametrize("N,K", [(1, 32), (64, 32), (65, 64), (100, 352)])
def test_fragment_order_holds_the_planar_terms(N, K):
    """unsplit_bf16x3(split_bf16x3(w)) is lcr_split_bf16x3's three terms bit for bit; the rows that pad the last 64-column tile are zero."""
    from lcrnet_amd import functional as F
    g = torch.Generator(device="cuda").manual_seed(N * 1000 + K)
    w = torch.randn(N, K, device="cuda", generator=g) * torch.exp(torch.randn(N, K, device="cuda", generator=g) * 4)
    w[0, :4] = torch.tensor([0.0, -0.0, 1.0, -3.0e38], device="cuda")
    tiles = F.split_bf16x3(w)
    assert tiles.dtype == torch.int16 and tiles.numel() * 2 == ((N + 63) // 64) * (K // 32) * 12288
    want = _planar(w).view(3, N, K).view(torch.bfloat16).float()
    got = F.unsplit_bf16x3(tiles)
    assert got.shape == (3, N, K) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    full = F.unsplit_bf16x3(tiles, padded=True)
    assert full.shape == (3, (N + 63) // 64 * 64, K) and torch.equal(full[:, :N].view(torch.int32), want.view(torch.int32))
    assert (full[:, N:].view(torch.int32) == 0).all()


@pytest.mark.parametrize("C", [32, 64, 128])            # K = 15 C: one mask bit per 32 << kshift columns, kshift 0, 1, 2
def test_masked_form_is_bit_identical(C):
    """gemm_bsplit(row_mask=...) on an A whose cleared blocks were never written (NaN here) equals the unmasked call on the zero-filled A:
    masks all ones, all zeros, and random with some rows all zero."""
    from lcrnet_amd import functional as F
    M, N, K = 130, 64, 15 * C
    g = torch.Generator().manual_seed(77 + C)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    bias = torch.randn(N, generator=g).cuda()
    div = (torch.rand(M, generator=g) * 8 + 1).floor().cuda()
    seg_len = torch.tensor([40, 50, 40], dtype=torch.int64, device="cuda")
    kw = dict(bias=bias, rowdiv=div, seg_len=seg_len, groups=32)
    planes = F.split_bf16x3(w)
    full = torch.randn(M, 15, C, generator=g)
    rnd = torch.rand(M, 15, generator=g) < 0.6
    rnd[::7] = False                                               # rows with no block at all
    rnd[5] = True
    for name, keep in (("ones", torch.ones(M, 15, dtype=torch.bool)), ("zeros", torch.zeros(M, 15, dtype=torch.bool)), ("random", rnd)):
        A = torch.where(keep[:, :, None], full, torch.zeros(()))
        P = torch.where(keep[:, :, None], full, torch.full((), float("nan")))
        mask = (keep.long() * torch.tensor([1 << k for k in range(15)])).sum(1).to(torch.int16).cuda()
        A, P = A.reshape(M, K).contiguous().cuda(), P.reshape(M, K).contiguous().cuda()
        c0, s0 = F.gemm_bsplit(A, planes, **kw)
        c1, s1 = F.gemm_bsplit(A, planes, row_mask=mask, **kw)
        c2, s2 = F.gemm_bsplit(P, planes, row_mask=mask, **kw)
        assert torch.isfinite(c0).all(), name
        assert torch.equal(c0, c1) and torch.equal(c0, c2), name
        assert torch.equal(s0.sum(0), s1.sum(0)) and torch.equal(s0.sum(0), s2.sum(0)), name
