"""CPU: calibration of the NetVLAD-head tests (tests/netvlad_restatement.py), no GPU.

  * the unmutated fp64 restatement IS oracle.torch_ref.global_descriptor run on a .double() state dict (1e-12), so the reference of the GPU
    file is pinned to the oracle the rest of the suite uses;
  * the fp32 floor — max |fp32 torch_ref - fp64 restatement| over every case of the GPU file, the fp32 sums taken in plain index order so
    that the figure does not depend on the BLAS of the machine — is recomputed and held within 2x of the committed FLOOR constants that
    the GPU tolerance TOL = min(1e-4, 4 FLOOR) is derived from;
  * every planted mutation moves the fp64 descriptor by >= 20 TOL on the cases it is assigned to (netvlad_restatement.ASSIGNED says which
    and why), so the GPU comparison at TOL cannot pass a kernel that makes that mistake.
"""
import numpy as np
import pytest
import torch

import netvlad_restatement as nv
from oracle import torch_ref


@pytest.mark.parametrize("kind", nv.KINDS)
def test_restatement_is_torch_ref_in_double(kind):
    sd = nv.netvlad_weights64(kind)
    for i, n in enumerate((1, 17, 350)):
        x = nv.netvlad_features((n,), 900 + i)
        got, mid = nv.describe(sd, x, (n,), intermediates=True)
        want = torch_ref.global_descriptor(sd, x.double())
        assert got.dtype == torch.float64 and got.shape == (1, 256)
        assert (got - want).abs().max().item() < 1e-12, (kind, n)
        assert abs(got.norm().item() - 1.0) < 1e-12
        assert mid["V"].shape == (1, 1024, 64) and mid["act"].shape == (n, 64)


def test_weight_sets_are_what_the_tests_assume():
    sd = nv.netvlad_weights("seeded")
    assert len(sd) == 16 and all(k.startswith("netvlad.") and v.dtype == torch.float32 for k, v in sd.items())
    # the seeded softmax is nearly flat, the stress one saturates, and its dead cluster lands under the 1e-6 clamp of stage 7
    x = nv.netvlad_features((17,), 900)
    flat = nv.describe(nv.netvlad_weights64("seeded"), x, (17,), intermediates=True)[1]
    sharp = nv.describe(nv.netvlad_weights64("stress"), x, (17,), intermediates=True)[1]
    assert flat["act"].max().item() < 0.1
    assert sharp["act"].max().item() > 0.999
    assert sharp["act"][:, 9].max().item() < 1e-30
    col = sharp["V"][0, :, 9].norm().item()
    assert col < 1e-6, col                                      # clamped, not normalised: the column stays (almost) zero
    assert sharp["gates"][0, 20].item() > 1 - 1e-9 and sharp["gates"][0, 21].item() < 1e-9
    # the exact zero row survives stage 1 as zeros (0 / 1e-12) and still casts a soft assignment
    z = nv.middle_zero_rows((17,))[0]
    assert not x[z].any() and not sharp["xn"][z].any() and abs(sharp["act"][z].sum().item() - 1.0) < 1e-12


def test_cases_cover_the_edges():
    c = nv.cases()
    assert c["ragged"][0] == nv.EDGE_LENGTHS and c["ragged_rev"][0] == nv.EDGE_LENGTHS[::-1]
    for S in nv.BATCH_SIZES:
        L = c[f"batch{S}"][0]
        assert len(L) == S and min(L) >= 1 and max(L) <= 40 and sum(L) < 3000
    assert nv.batch_lengths(129)[:66] == nv.batch_lengths(66)


def test_fp32_matmul_is_index_order_fp32():
    g = torch.Generator().manual_seed(0)
    for sa, sb in (((3, 200), (200, 5)), ((1, 7, 300), (300, 4)), ((1, 6, 9), (1, 9, 11)), ((2, 70000), (70000, 3))):
        a, b = torch.randn(*sa, generator=g), torch.randn(*sb, generator=g)
        acc = torch.zeros(())
        for k in range(sa[-1]):                                  # the definition: one rounded product, one rounded addition per k
            acc = acc + a[..., :, k, None] * b[..., k, None, :]
        got = nv.fp32_matmul(a, b)
        assert got.dtype == torch.float32 and torch.equal(got, acc), (sa, sb)
        assert (got.double() - a.double() @ b.double()).abs().max().item() < 1e-6 * sa[-1]
    a64 = torch.randn(4, 9, generator=g, dtype=torch.float64)
    assert torch.equal(nv.fp32_matmul(a64, a64.t()), a64 @ a64.t())   # only fp32 products are re-ordered
    with nv.pinned_fp32_matmul():
        assert torch.matmul is nv.fp32_matmul
    assert torch.matmul is not nv.fp32_matmul
    assert np.add.reduce(np.array([[1e8], [1.0], [-1e8], [1.0]], np.float32), axis=0)[0] == 1.0      # (1e8 + 1) - 1e8 + 1 in fp32 order


def _floor(kind):
    sd32 = nv.netvlad_weights(kind)
    worst = {}
    for name, (seg_lens, seed) in nv.cases().items():
        x = nv.netvlad_features(seg_lens, seed)
        want = nv.reference(kind, name)
        o, err = 0, 0.0
        for s, n in enumerate(seg_lens):
            with nv.pinned_fp32_matmul():
                got = torch_ref.global_descriptor(sd32, x[o:o + n])
            err = max(err, (got.double()[0] - want[s]).abs().max().item())
            o += n
        worst[name] = err
    return worst


@pytest.mark.parametrize("kind", nv.KINDS)
def test_fp32_floor_matches_committed_constant(kind):
    worst = _floor(kind)
    floor = max(worst.values())
    print(f"fp32 floor [{kind}] = {floor:.3e} (committed {nv.FLOOR[kind]:.1e}); worst case {max(worst, key=worst.get)}")
    assert nv.FLOOR[kind] / 2 <= floor <= nv.FLOOR[kind] * 2, (floor, nv.FLOOR[kind])
    assert nv.TOL[kind] == min(1e-4, 4 * nv.FLOOR[kind])


def test_every_mutation_is_assigned():
    assert {m for m, _ in nv.ASSIGNED} == set(nv.MUTATIONS)
    assert all(k in nv.KINDS for _, k in nv.ASSIGNED)
    # bn_eps_zero moves the seeded descriptor by ~1e-6, below any bound: only the stress set is claimed to see it
    assert ("bn_eps_zero", "stress") in nv.ASSIGNED and ("bn_eps_zero", "seeded") not in nv.ASSIGNED
    # the drop mutations are seen by every single small length on its own; the 350-row sample is assigned to no row mutation
    for m in ("asum_drop_last_row", "v_drop_last_row", "asum_take_next_row", "v_take_next_row"):
        wanted = nv.ASSIGNED[(m, "seeded")][0]
        assert not wanted((350,)) and nv.judged_segments(m, (350, 350)) == []
        if m.endswith("drop_last_row"):
            assert all(wanted((n,)) for n in nv.EDGE_LENGTHS if n <= nv.SMALL_SEGMENT)


@pytest.mark.parametrize("mutation,kind", sorted(nv.ASSIGNED))
def test_mutation_moves_descriptor_by_20_tol(mutation, kind):
    wanted, mode = nv.ASSIGNED[(mutation, kind)]
    need = nv.SENSITIVITY * nv.TOL[kind]
    smallest, n_cases = float("inf"), 0
    for name, (seg_lens, _) in nv.cases().items():
        if not wanted(seg_lens):
            continue
        judged = nv.judged_segments(mutation, seg_lens)
        assert judged, (mutation, name)
        shift = (nv.reference(kind, name, mutation) - nv.reference(kind, name)).abs().amax(dim=1)[judged]
        seen = (shift.min() if mode == "every" else shift.max()).item()
        smallest = min(smallest, seen)
        n_cases += 1
        assert seen >= need, (mutation, kind, name, mode, seen, need)
    print(f"{mutation} [{kind}]: smallest shift {smallest:.3e} over {n_cases} cases ({mode} segment) = {smallest / nv.TOL[kind]:.0f} x TOL")
    assert n_cases >= 10
