"""GPU: KPConv aggregates with row masks (lcr_kpconv_aggregate_mask) and the contractions that zero-fill the masked kernel-point blocks
instead of reading them (lcr_gemm_f32_masked, lcr_gemm_f32_bsplit_masked).  Skipping an all-zero block is exact, so everything here is
compared bit for bit with the unmasked path."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def surface_cloud(Ns, M, H, C, seed, interior_padding=False):
    """Supports on a wavy sheet (like a lidar surface: kernel points above / below it see no neighbour), queries among them, lists of H
    random supports padded with Ns (valid first, or with holes)."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(Ns, 2, generator=g) * 6
    z = 0.3 * torch.sin(xy[:, :1] * 1.3) + 0.05 * torch.randn(Ns, 1, generator=g)
    s_pts = torch.cat([xy, z], 1)
    q_pts = s_pts[torch.randperm(Ns, generator=g)[:M]].clone()
    feats = torch.randn(Ns, C, generator=g)
    d = torch.cdist(q_pts, s_pts)
    nb = d.topk(H, largest=False).indices.int()
    cnt = torch.randint(0, H + 1, (M,), generator=g)
    col = torch.arange(H)[None, :]
    if interior_padding:
        nb[torch.rand(M, H, generator=g) < 0.3] = Ns
    else:
        nb[col >= cnt[:, None]] = Ns
    return s_pts, q_pts, feats, nb, g


def kp_sigma():
    from lcrnet_amd.weights import base_kernel_points
    return base_kernel_points() * 0.6, 0.3


def block_bits(A, M, C):
    nz = (A.view(M, 15, C) != 0).any(-1) | A.view(M, 15, C).isnan().any(-1)
    w = torch.tensor([1 << k for k in range(15)], dtype=torch.int64, device=A.device)
    return (nz.long() * w).sum(1)


@pytest.mark.parametrize("C", [32, 64, 128, 256])
@pytest.mark.parametrize("ordered", [False, True])
def test_mask_marks_exactly_the_nonzero_blocks_and_only_those_are_stored(C, ordered):
    from lcrnet_amd import functional as F
    Ns, M, H = 3000, 1234, 40
    s_pts, q_pts, feats, idx, g = surface_cloud(Ns, M, H, C, C + ordered)
    kp, sigma = kp_sigma()
    dev = dict(device="cuda")
    s_pts, q_pts, feats, idx = s_pts.cuda(), q_pts.cuda(), feats.cuda(), idx.cuda()
    pos = F.row_positive(feats)
    order = torch.randperm(M, generator=g).int().cuda() if ordered else None
    A0, n0 = F.kpconv_aggregate(feats, pos, q_pts, s_pts, idx, kp, sigma, order=order)
    A1, n1, mask = F.kpconv_aggregate(feats, pos, q_pts, s_pts, idx, kp, sigma, order=order, emit_mask=True)
    bits = block_bits(A0, M, C)
    got = mask.long() & 0x7FFF
    assert torch.equal(got, bits)
    assert 0.1 < 1 - (bits[:, None] >> torch.arange(15, **dev) & 1).float().mean().item() < 0.9      # the case has zero blocks to skip
    keep = ((mask.long()[:, None] >> torch.arange(15, **dev)) & 1).bool()[:, :, None].expand(M, 15, C)
    assert torch.equal(A1.view(M, 15, C)[keep], A0.view(M, 15, C)[keep]) and torch.equal(n0, n1)
    # the influences themselves (fp64 restatement): a block with no influence > 0 is zero; with one clearly > 0 it is marked (random
    # features never cancel exactly)
    sp = np.concatenate([s_pts.cpu().numpy(), np.full((1, 3), 1e6, np.float32)]).astype(np.float64)
    rel = sp[idx.cpu().numpy().astype(np.int64)] - q_pts.cpu().numpy().astype(np.float64)[:, None, :]
    infl = 1 - np.linalg.norm(rel[:, :, None, :] - kp[None, None].astype(np.float64), axis=3) / sigma           # [M, H, 15]
    infl_max = infl.max(1)
    m_np = got.cpu().numpy()[:, None] >> np.arange(15) & 1
    assert not m_np[infl_max < -1e-5].any()
    assert m_np[infl_max > 1e-5].all()


def test_mask_keeps_nonfinite_features():
    """A NaN / Inf feature gathered with influence 0 makes its block NaN (0 * Inf): the block is marked and stored, as before."""
    from lcrnet_amd import functional as F
    C, Ns, M, H = 64, 2000, 500, 32
    s_pts, q_pts, feats, idx, _ = surface_cloud(Ns, M, H, C, 5)
    feats[::37, 3] = float("inf")
    feats[::53, 9] = float("nan")
    kp, sigma = kp_sigma()
    s_pts, q_pts, feats, idx = s_pts.cuda(), q_pts.cuda(), feats.cuda(), idx.cuda()
    pos = F.row_positive(feats)
    A0, _ = F.kpconv_aggregate(feats, pos, q_pts, s_pts, idx, kp, sigma)
    A1, _, mask = F.kpconv_aggregate(feats, pos, q_pts, s_pts, idx, kp, sigma, emit_mask=True)
    assert A0.isnan().any()
    assert torch.equal(mask.long() & 0x7FFF, block_bits(A0, M, C))
    keep = ((mask.long()[:, None] >> torch.arange(15, device="cuda")) & 1).bool()[:, :, None].expand(M, 15, C)
    assert torch.equal(A1.view(M, 15, C)[keep].isnan(), A0.view(M, 15, C)[keep].isnan())


def masked_operand(M, C, seed, zero_frac=0.4):
    """A [M, 15 C] with random all-zero blocks, the same A with those blocks poisoned (NaN), and the mask."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, 15, C, generator=g)
    z = torch.rand(M, 15, generator=g) < zero_frac
    z[:, 7] = False
    A[z] = 0.0
    mask = ((~z).long() * torch.tensor([1 << k for k in range(15)])).sum(1).to(torch.int16)
    P = A.clone()
    P[z] = float("nan")
    return A.view(M, 15 * C).cuda(), P.view(M, 15 * C).cuda(), mask.cuda(), g


SHAPES = [(32, 32), (64, 64), (128, 128), (256, 256), (64, 32)]


@pytest.mark.parametrize("C,N,split", [(c, n, False) for c, n in SHAPES] + [(c, n, True) for c, n in SHAPES if n >= 64])   # split: N >= 64
@pytest.mark.parametrize("M", [1, 63, 1000, 4097])
def test_masked_contraction_is_bit_identical(C, N, M, split):
    from lcrnet_amd import functional as F
    K = 15 * C
    assert F.kpconv_mask_ok(M, N, K, split)
    A, P, mask, g = masked_operand(M, C, 31 * C + M + N + split)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).cuda()
    bias = torch.randn(N, generator=g).cuda()
    div = (torch.rand(M, generator=g) * 8 + 1).floor().cuda()
    seg = [M // 3, M // 3 + 1, M - 2 * (M // 3) - 1] if M > 8 else [M]
    seg_len = torch.tensor(seg, dtype=torch.int64, device="cuda")
    kw = dict(bias=bias, rowdiv=div, seg_len=seg_len, groups=N // 4 if N >= 32 else 0)
    if split:
        planes = F.split_bf16x3(w)
        c0, s0 = F.gemm_bsplit(A, planes, **kw)
        c1, s1 = F.gemm_bsplit(P, planes, row_mask=mask, **kw)
        c2, s2 = F.gemm_bsplit(P, planes, row_mask=mask, **kw)
    else:
        c0, s0 = F.gemm(A, w, trans_b=True, **kw)
        c1, s1 = F.gemm(P, w, trans_b=True, row_mask=mask, **kw)
        c2, s2 = F.gemm(P, w, trans_b=True, row_mask=mask, **kw)
    assert torch.equal(c0, c1) and torch.equal(c1, c2)
    assert torch.equal(s0.sum(0), s1.sum(0)) and torch.equal(s1, s2)


def test_masked_contraction_refuses_what_it_cannot_describe():
    from lcrnet_amd import _lib, functional as F
    A, _, mask, _ = masked_operand(100, 64, 1)
    w = torch.randn(64, 960).cuda()
    L = _lib.lib()
    c = torch.empty(100, 64, device="cuda")
    for bk in (48, 16, 512):
        rc = L.lcr_gemm_f32_masked(_lib.ptr(A), _lib.ptr(w), _lib.ptr(c), 100, 64, 960, None, None, None, 0, 0, None, _lib.ptr(mask), bk,
                                   _lib.stream_ptr(A.device))
        assert rc != 0
    assert F.kpconv_mask_ok(100, 64, 960, True) and not F.kpconv_mask_ok(100, 64, 961, True)


@pytest.mark.parametrize("cin", [32, 64, 128])
@pytest.mark.parametrize("interior", [False, True])
def test_kpconv_module_with_masks_equals_the_full_aggregate(cin, interior):
    """KPConv.forward_raw (masked wherever kpconv_mask_ok holds) against aggregate-everything + unmasked contraction, both GEMM forms,
    with a processing order and GroupNorm segments; lists valid-first and with interior padding."""
    from lcrnet_amd import functional as F
    from lcrnet_amd.modules.kpconv.kpconv import KPConv
    Ns, M, H = 4000, 2500, 38
    s_pts, q_pts, feats, idx, g = surface_cloud(Ns, M, H, cin, 7 * cin + interior, interior_padding=interior)
    torch.manual_seed(cin)
    conv = KPConv(cin, cin, 15, 0.6, 0.3, bias=True)
    with torch.no_grad():
        conv.weights.normal_(0.0, (15 * cin) ** -0.5)
        conv.bias.normal_()
    conv = conv.cuda()
    s_pts, q_pts, feats, idx = s_pts.cuda(), q_pts.cuda(), feats.cuda(), idx.cuda()
    order = torch.randperm(M, generator=g).int().cuda()
    seg_len = torch.tensor([1000, 700, 800], dtype=torch.int64, device="cuda")
    pos = F.row_positive(feats)
    kp = conv.kernel_points_host()
    was = F.gemm_split_enabled()
    try:
        for split in (False, True):
            F.set_gemm_split(split)
            out, st = conv.forward_raw(feats, q_pts, s_pts, idx, s_pos=pos, seg_len=seg_len, groups=8, order=order)
            A, nn_cnt = F.kpconv_aggregate(feats, pos, q_pts, s_pts, idx, kp, conv.sigma, order=order)
            wt = conv.weights_t()
            if split and F.gemm_split_ok(wt.shape[0], wt.shape[1]):
                want, wst = F.gemm_bsplit(A, conv.weights_t_split(), bias=conv.bias, rowdiv=nn_cnt, seg_len=seg_len, groups=8)
            else:
                want, wst = F.gemm(A, wt, trans_b=True, bias=conv.bias, rowdiv=nn_cnt, seg_len=seg_len, groups=8)
            assert torch.equal(out, want), split
            assert torch.equal(st.sum(0), wst.sum(0)), split
    finally:
        F.set_gemm_split(was)
