"""GPU: the split-bf16 GEMM at the light depths (K <= 256) — its normalise-on-load form lcr_gemm_f32_bsplit_anorm and the plain form —
against fp64, next to the fp32 kernels on the same inputs; the domain of the new entry point; and the one dispatch rule
(lcr_gemm_split_ok / functional.gemm_split_ok) in the native encoder driver and the module tree."""
import numpy as np
import pytest
import torch

from conftest import LIMITS, NUM_STAGES, RADIUS, VOXEL, load_scan

pytestmark = pytest.mark.gpu
GN_EPS, SLOPE = 1e-5, 0.1


def _errors(c0, c1, ref):
    scale = ref.abs().max().item()
    return (c0.double() - ref).abs().max().item() / scale, (c1.double() - ref).abs().max().item() / scale


def _stats_rel(s0, s1, seg, gs):
    """sums against their Cauchy-Schwarz bound sqrt(n * sum of squares), sums of squares relative (tests/test_gemm_split_gpu.py)"""
    n_el = seg.double()[:, None] * gs
    return max(((s0[..., 0] - s1[..., 0]).abs() / (n_el * s0[..., 1]).sqrt()).max().item(),
               ((s0[..., 1] - s1[..., 1]).abs() / s0[..., 1]).max().item())


@pytest.mark.parametrize("M,N,K,seg,groups", [(200, 64, 32, [64, 70, 66], 32), (200, 96, 64, [64, 70, 66], 24), (333, 256, 256, [100, 64, 169], 32),
                                              (130, 128, 128, [64, 66], 32)])
def test_split_anorm_against_fp64(M, N, K, seg, groups):
    """C = LReLU(GN(a)) . W^T + b in fp64 from the SAME statistics table, against lcr_gemm_f32_bsplit_anorm (e1) and lcr_gemm_f32_anorm (e0):
    a row block straddling a segment boundary, a segment of exactly 64 rows, M not a multiple of 64, N not a multiple of 64.  Bounds of
    tests/test_gemm_split_gpu.py: e1 < 3e-6 of the largest output and e1 < max(4 e0, 4e-7); output statistics within 1e-6."""
    from lcrnet_amd import functional as F
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a = torch.randn(M, K, device=dev, generator=g) * 2.0 + 0.7
    for s0, n in zip(np.cumsum([0] + seg[:-1]), seg):                   # different statistics per segment
        a[s0:s0 + n] *= 1.0 + 0.5 * (int(s0) % 3)
    w = torch.randn(N, K, device=dev, generator=g) / K ** 0.5
    bias = torch.randn(N, device=dev, generator=g)
    gamma, beta = torch.rand(K, device=dev, generator=g) + 0.5, torch.randn(K, device=dev, generator=g)
    seg_len = torch.tensor(seg, dtype=torch.int64, device=dev)
    a_groups = 32
    a_stats = F.groupnorm_stats(a, a_groups, seg_len)
    c0, st0 = F.gemm_anorm(a, a_stats, gamma, beta, a_groups, w, bias=bias, seg_len=seg_len, groups=groups)
    c1, st1 = F.gemm_bsplit_anorm(a, a_stats, gamma, beta, a_groups, F.split_bf16x3(w), bias=bias, seg_len=seg_len, groups=groups)
    torch.cuda.synchronize()
    tab = a_stats.sum(0)                                                # [S, a_groups, 2]
    gs = K // a_groups
    cnt = seg_len.double()[:, None] * gs
    mean = tab[..., 0] / cnt
    rstd = 1.0 / ((tab[..., 1] / cnt - mean * mean).clamp_min(0.0) + GN_EPS).sqrt()
    rows = torch.repeat_interleave(torch.arange(len(seg), device=dev), seg_len)
    y = (a.double().view(M, a_groups, gs) - mean[rows][..., None]) * rstd[rows][..., None]
    y = y.view(M, K) * gamma.double() + beta.double()
    y = torch.where(y > 0, y, y * SLOPE)
    ref = y @ w.double().t() + bias.double()
    e0, e1 = _errors(c0, c1, ref)
    print("M=%d N=%d K=%d: max err / max |ref|: fp32 anorm %.2e, split anorm %.2e" % (M, N, K, e0, e1))
    assert torch.isfinite(c1).all()
    assert e1 < 3e-6 and e1 < max(4 * e0, 4e-7)
    rel = _stats_rel(st0.sum(0), st1.sum(0), seg_len, N // groups)
    print("statistics: %.2e" % rel)
    assert rel < 1e-6, rel


@pytest.mark.parametrize("M,N,K", [(500, 256, 128), (70, 64, 256)])
def test_plain_split_at_light_depth_against_fp64(M, N, K):
    """lcr_gemm_f32_bsplit with bias and statistics at K <= 256 (four and eight K-steps; two row blocks with a ragged last one), next to
    lcr_gemm_f32, under the same bounds."""
    from lcrnet_amd import functional as F
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a = torch.randn(M, K, device=dev, generator=g) * (torch.rand(M, 1, device=dev, generator=g) * 4 + 0.01)
    w = torch.randn(N, K, device=dev, generator=g) * 0.05
    bias = torch.randn(N, device=dev, generator=g)
    seg_len = torch.tensor([M // 3, M // 3 + 5, M - 2 * (M // 3) - 5], dtype=torch.int64, device=dev)
    c0, st0 = F.gemm(a, w, trans_b=True, bias=bias, seg_len=seg_len, groups=32)
    c1, st1 = F.gemm_bsplit(a, F.split_bf16x3(w), bias=bias, seg_len=seg_len, groups=32)
    torch.cuda.synchronize()
    ref = a.double() @ w.double().t() + bias.double()
    e0, e1 = _errors(c0, c1, ref)
    print("M=%d N=%d K=%d: max err / max |ref|: fp32 MFMA %.2e, split %.2e" % (M, N, K, e0, e1))
    assert torch.isfinite(c1).all()
    assert e1 < 3e-6 and e1 < max(4 * e0, 4e-7)
    rel = _stats_rel(st0.sum(0), st1.sum(0), seg_len, N // 32)
    assert rel < 1e-6, rel


@pytest.mark.parametrize("N,K", [(64, 288), (64, 40), (32, 64)])
def test_split_anorm_refuses_shapes_outside_its_domain(N, K):
    """K > 256, K % 32 != 0 and N < 64: an argument error with text, no launch — C keeps its contents."""
    from lcrnet_amd import _lib
    dev = torch.device("cuda")
    M = 128
    a = torch.ones(M, K, device=dev)
    planes = torch.zeros(((N + 63) // 64) * ((K + 31) // 32) * 3 * 64 * 32, dtype=torch.int16, device=dev)
    c = torch.full((M, N), 7.0, device=dev)
    gamma, beta = torch.ones(K, device=dev), torch.zeros(K, device=dev)
    a_groups = 8
    seg_len = torch.tensor([M], dtype=torch.int64, device=dev)
    a_stats = torch.zeros(8, 1, a_groups, 2, dtype=torch.float64, device=dev)
    rc = _lib.lib().lcr_gemm_f32_bsplit_anorm(_lib.ptr(a), _lib.ptr(planes), _lib.ptr(c), M, N, K, None, _lib.ptr(a_stats), _lib.ptr(gamma),
                                              _lib.ptr(beta), a_groups, GN_EPS, SLOPE, _lib.ptr(seg_len), 1, 0, None, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    assert rc == -1 and _lib.lib().lcr_last_error().startswith(b"lcr_gemm_f32_bsplit_anorm:")
    assert (c == 7.0).all()


def test_python_rule_equals_the_native_rule():
    """functional.gemm_split_ok == lcr_gemm_split_ok on every Linear and KPConv contraction of the encoder, and on a grid around them."""
    from lcrnet_amd import _lib
    from lcrnet_amd import functional as F
    from lcrnet_amd.backbone4 import KPEncoder
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.modules.kpconv.modules import UnaryBlock
    b = make_cfg()["backbone"]
    enc = KPEncoder(b["input_dim"], b["init_dim"], b["kernel_size"], b["init_radius"], b["init_sigma"], b["group_norm"])
    shapes = {(m.out_channels, m.in_channels) for m in enc.modules() if isinstance(m, UnaryBlock)}
    assert {(128, 32), (256, 64), (512, 128), (1024, 256), (256, 128), (512, 256), (64, 128), (64, 256), (128, 256), (32, 64)} <= shapes
    shapes |= {(c, 15 * c) for c in (32, 64, 128, 256)}
    shapes |= {(n, k) for n in (16, 32, 48, 64, 96, 128, 256, 512, 1024) for k in (16, 32, 40, 64, 96, 128, 160, 192, 224, 256, 272, 288, 320, 512)}
    L = _lib.lib()
    for n, k in sorted(shapes):
        assert bool(L.lcr_gemm_split_ok(n, k)) == bool(F.gemm_split_ok(n, k)), (n, k)
        if n < 64 or k % 32:
            assert not F.gemm_split_ok(n, k), (n, k)                    # N = 32 layers stay on the fp32 form
        if k >= 288 and n >= 64 and k % 32 == 0:
            assert F.gemm_split_ok(n, k), (n, k)                        # the K-deep rule is unchanged


@pytest.fixture(scope="module")
def toy():
    """two scans, one batch (per-scan GroupNorm segments, processing order), and the seeded encoder"""
    from lcrnet_amd.data import precompute_batch
    from lcrnet_amd.model_family import create_model
    from lcrnet_amd.weights import seeded_state_dict
    model = create_model().eval()
    model.load_state_dict(seeded_state_dict(model.state_dict(), 7351))
    model = model.cuda()
    scans = [load_scan(n) for n in ["003854", "000958"]]
    pts = torch.from_numpy(np.concatenate(scans)).cuda()
    lens = torch.tensor([len(s) for s in scans], dtype=torch.int64, device="cuda")
    dd = precompute_batch(pts, lens, NUM_STAGES, VOXEL, RADIUS, LIMITS)
    return model.encoder, torch.ones(pts.shape[0], 1, device="cuda"), dd


def _run(enc, feats, dd, native):
    enc.native = native
    with torch.no_grad():
        out = [t.clone() for t in enc(feats, dd)]
    torch.cuda.synchronize()
    return out


def test_native_driver_and_module_tree_agree_bit_for_bit_under_the_rule(toy, monkeypatch):
    """the same launches on both sides of the rule: lcr_encoder_forward and the module tree give equal bits with the split form on"""
    from lcrnet_amd import functional as F
    enc, feats, dd = toy
    monkeypatch.delenv("LCR_NATIVE_ENCODER", raising=False)
    was_native, was = enc.native, F.gemm_split_enabled()
    F.set_gemm_split(True)
    try:
        nat = _run(enc, feats, dd, True)
        ref = _run(enc, feats, dd, False)
    finally:
        F.set_gemm_split(was)
        enc.native = was_native
    for a, b in zip(nat, ref):
        assert a.shape == b.shape and torch.equal(a, b)


def test_rule_on_stays_within_the_split_bound_of_fp32_everywhere(toy, monkeypatch):
    """every stage output with the rule on against the same pass with every GEMM on the fp32 matrix instruction (LCR_GEMM_SPLIT=0's
    switch): within 1e-4 of the stage's largest value (>= 1), the bound tests/test_float_parity_gpu.py holds either form to."""
    from lcrnet_amd import functional as F
    enc, feats, dd = toy
    monkeypatch.delenv("LCR_NATIVE_ENCODER", raising=False)
    was_native, was = enc.native, F.gemm_split_enabled()
    try:
        F.set_gemm_split(True)
        on = _run(enc, feats, dd, True)
        F.set_gemm_split(False)
        off = _run(enc, feats, dd, True)
    finally:
        F.set_gemm_split(was)
        enc.native = was_native
    for i, (a, b) in enumerate(zip(on, off)):
        d, scale = (a - b).abs().max().item(), b.abs().max().item()
        print("stage %d: max |on - off| %.3e at max |x| %.2f" % (i + 1, d, scale))
        assert torch.isfinite(a).all() and d < 1e-4 * max(1.0, scale), (i, d, scale)
