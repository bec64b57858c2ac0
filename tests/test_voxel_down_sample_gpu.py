"""GPU: lcr_voxel_down_sample (Open3D's VoxelDownSample) bit for bit against the fp64 restatement (tests/o3d_voxel_restatement.py,
whose order comes from the host mirror pinned against libstdc++ in test_voxel_down_sample_cpu.py): values, fp64 averages, lengths
and order, on raw scans with colliding hash_eigen codes, voxel faces, far coordinates, edge clouds and every batch size; batch
invariance; the grid path as a negative control; the one-call raw collate and DescriptorPipeline; the reference helper; key overflow."""
import numpy as np
import pytest
import torch

from o3d_voxel_restatement import hash_eigen, voxel_down_sample as restate, voxel_down_sample_stack, voxel_indices

pytestmark = pytest.mark.gpu

_SCANS = {}


def _scan(seed, step=1):
    """Synthetic raw scan with a deterministic intensity column: f32 [N, 4]."""
    key = (seed, step)
    if key not in _SCANS:
        import lcrnet_amd.synthetic as synthetic
        xyz = synthetic.synthetic_scan(seed)[::step]
        inten = ((np.arange(len(xyz)) * 37 + seed) % 101).astype(np.float32) / np.float32(101.0)
        _SCANS[key] = np.ascontiguousarray(np.concatenate([xyz, inten[:, None]], axis=1))
    return _SCANS[key]


def _device(clouds, out_cols, hint=0):
    from lcrnet_amd.downsample import voxel_down_sample_device
    rows = torch.from_numpy(np.concatenate(clouds) if clouds else np.zeros((0, 4), np.float32)).cuda()
    lens = torch.tensor([len(c) for c in clouds], dtype=torch.int64, device="cuda")
    out, out64, out_len, status = voxel_down_sample_device(rows.contiguous(), lens, 0.3, out_cols, want_f64=True, key_bits_hint=hint)
    lh = out_len.cpu().tolist()
    m = sum(lh)
    return out[:m].cpu().numpy(), out64[:m].cpu().numpy(), lh, int(status.item())


def _expect(clouds, out_cols):
    per = [restate(c, 0.3, out_cols) for c in clouds]
    return (np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per]), [len(p[0]) for p in per])


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                  b.view(np.uint32 if b.dtype == np.float32 else np.uint64))


@pytest.mark.parametrize("out_cols", [4, 3])
def test_raw_scans_bit_exact(out_cols):
    clouds = [_scan(s) for s in range(8)]
    for c in clouds:                                      # the scans do exercise distinct voxels with equal codes
        _, idx = voxel_indices(c[:, :3], 0.3)
        u = np.unique(idx, axis=0)
        assert len(np.unique(hash_eigen(u))) < len(u)
    f32, f64, lh, st = _device(clouds, out_cols)
    w32, w64, wl = _expect(clouds, out_cols)
    assert st == 0 and lh == wl
    assert _same(f32, w32) and _same(f64, w64)


def _edge_clouds():
    rng = np.random.default_rng(4)
    v = 0.3
    face = np.array([[0, 0, 0], [v / 2, 0, 0], [3 * v / 2, v / 2, 0], [v / 2, 3 * v / 2, 5 * v / 2], [-v, -v, -v]], np.float64)
    faces = np.concatenate([face + k * v for k in range(6)]).astype(np.float32)                 # exactly on the min - v/2 grid faces
    far = (rng.uniform(-40, 40, size=(20000, 3)) + np.array([1.0e4, -1.2e4, 9.7e3])).astype(np.float32)
    one = np.array([[3.0, -4.0, 5.0]], np.float32)
    single = (rng.uniform(0, 0.05, size=(50, 3)) + 7.0).astype(np.float32)
    clouds = [faces, np.zeros((0, 3), np.float32), far, one, single, np.zeros((0, 3), np.float32)]
    return [np.concatenate([c, rng.random((len(c), 1), dtype=np.float32)], axis=1) for c in clouds]


def test_faces_far_coordinates_and_edge_clouds():
    clouds = _edge_clouds()
    for out_cols in (3, 4):
        f32, f64, lh, st = _device(clouds, out_cols)
        w32, w64, wl = _expect(clouds, out_cols)
        assert st == 0 and lh == wl and lh[1] == 0 and lh[3] == 1 and lh[4] == 1 and lh[5] == 0
        assert _same(f32, w32) and _same(f64, w64)
    # far from the origin, fp32 keys (grid subsampling's arithmetic) put points in other voxels than fp64 ones
    from lcrnet_amd.data import voxelize_raw_scans
    far = torch.from_numpy(clouds[2][:, :3].copy()).cuda()
    g, _, gl = voxelize_raw_scans(far, torch.tensor([len(far)], device="cuda"), 0.3)
    assert gl[0] != lh[2] or not np.array_equal(np.sort(g.cpu().numpy(), axis=0), np.sort(w32[lh[0] + lh[1]:][:lh[2], :3], axis=0))


@pytest.mark.parametrize("B", [1, 8, 64, 100])
def test_batch_sizes_and_invariance(B):
    from lcrnet_amd.downsample import voxel_down_sample
    step = 1 if B <= 8 else 16
    clouds = [_scan(s % 8, step)[(s // 8) * 7:] for s in range(B)]        # distinct clouds
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    lens = torch.tensor([len(c) for c in clouds], dtype=torch.int64, device="cuda")
    f32, f64, dl, lh = voxel_down_sample(rows, lens, 0.3, 4, want_f64=True)
    w32, w64, wl = voxel_down_sample_stack(np.concatenate(clouds), [len(c) for c in clouds], 0.3, 4)
    assert lh == wl.tolist() and dl.cpu().tolist() == lh
    assert _same(f32.cpu().numpy(), w32) and _same(f64.cpu().numpy(), w64)
    if B in (8, 64):                                      # every cloud alone gives the rows it got inside the batch
        for k in (0, B // 2, B - 1):
            a32, a64, al, st = _device([clouds[k]], 4)
            o = sum(lh[:k])
            assert st == 0 and al == [lh[k]]
            assert _same(a32, f32[o:o + lh[k]].cpu().numpy()) and _same(a64, f64[o:o + lh[k]].cpu().numpy())


def test_grid_path_is_a_different_function():
    """Negative control: the collate's grid subsampling does not reproduce Open3D on these scans, method="open3d" does."""
    from lcrnet_amd.data import voxelize_raw_scans
    clouds = [_scan(s) for s in range(3)]
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    lens = torch.tensor([len(c) for c in clouds], dtype=torch.int64, device="cuda")
    w32, _, wl = voxel_down_sample_stack(np.concatenate(clouds), [len(c) for c in clouds], 0.3, 3)
    g, _, gl = voxelize_raw_scans(rows, lens, 0.3)
    assert not (gl == wl.tolist() and _same(g.cpu().numpy(), w32))
    o, ol_dev, ol = voxelize_raw_scans(rows, lens, 0.3, method="open3d")
    assert ol == wl.tolist() and ol_dev.cpu().tolist() == ol and _same(o.cpu().numpy(), w32)
    with pytest.raises(ValueError):
        voxelize_raw_scans(rows, lens, 0.3, method="o3d")


def test_one_call_raw_collate_open3d():
    from lcrnet_amd.data import precompute_batch, precompute_batch_native
    clouds = [_scan(s, 3) for s in range(3)]
    rows = torch.from_numpy(np.concatenate(clouds)).cuda()
    lens = torch.tensor([len(c) for c in clouds], dtype=torch.int64, device="cuda")
    w32, _, wl = voxel_down_sample_stack(np.concatenate(clouds), [len(c) for c in clouds], 0.3, 3)
    limits = [40, 40, 40, 40]
    a = precompute_batch(torch.from_numpy(w32).cuda(), torch.from_numpy(wl).cuda(), 4, 0.3, 1.275, limits)
    for cap in (None, 100):                               # default capacity guess; one far too small (device-detected retry)
        b = precompute_batch_native(rows, lens, 4, 0.3, 1.275, limits, raw_voxel=0.3, capacity=cap, raw_method="open3d")
        assert b["lengths_host"] == a["lengths_host"] and b["lengths_host"][0] == wl.tolist()
        for key in ("points", "lengths", "neighbors", "subsampling", "upsampling"):
            assert len(a[key]) == len(b[key])
            for x, y in zip(a[key], b[key]):
                assert x.shape == y.shape and torch.equal(x, y), key
    g = precompute_batch_native(rows, lens, 4, 0.3, 1.275, limits, raw_voxel=0.3)      # the default stays the grid path
    assert g["lengths_host"][0] != wl.tolist() or not torch.equal(g["points"][0].cpu(), torch.from_numpy(w32))


@pytest.mark.parametrize("two_calls", [False, True])
def test_descriptor_pipeline_open3d_ingest(monkeypatch, two_calls):
    from lcrnet_amd.model_family import create_model
    from lcrnet_amd.pipeline import DescriptorPipeline
    from lcrnet_amd.weights import seeded_state_dict
    if two_calls:
        monkeypatch.setenv("LCR_PRE_TWO_CALLS", "1")
    else:
        monkeypatch.delenv("LCR_PRE_TWO_CALLS", raising=False)
    m = create_model().eval()
    m.load_state_dict(seeded_state_dict(m.state_dict(), 7351))
    m = m.cuda()
    clouds = [_scan(s, 2) for s in range(8)]
    lens = [len(c) for c in clouds]
    host = [(torch.from_numpy(np.concatenate(clouds[:5])), torch.tensor(lens[:5])), (torch.from_numpy(np.concatenate(clouds[5:])), torch.tensor(lens[5:]))]
    vox = []
    for g in (clouds[:5], clouds[5:]):
        w32, _, wl = voxel_down_sample_stack(np.concatenate(g), [len(c) for c in g], 0.3, 3)
        vox.append((torch.from_numpy(w32).cuda(), torch.from_numpy(wl).cuda()))
    limits = [74, 68, 70, 67]
    with DescriptorPipeline(m, neighbor_limits=limits, raw_voxel=None) as pipe:
        want = [d.clone() for d in pipe.run(vox)]
    with DescriptorPipeline(m, neighbor_limits=limits, raw_voxel=0.3, raw_method="open3d") as pipe:
        got = [d.clone() for d in pipe.run(host)]
    torch.cuda.synchronize()
    assert len(got) == len(want) == 2
    for a, b in zip(want, got):
        assert a.shape == b.shape and torch.equal(a, b)


def test_reference_helper_voxel_downsample():
    from lcrnet_amd.downsample import voxel_downsample
    xyz = _scan(6)[:, :3].copy()
    got = voxel_downsample(xyz, 0.3)
    _, w64, _ = restate(xyz, 0.3, 3)
    assert got.dtype == np.float64 and _same(got, w64)
    assert _same(voxel_downsample(torch.from_numpy(xyz).cuda(), 0.3), w64)
    with pytest.raises(ValueError):
        voxel_downsample(xyz, 0.3, normals=np.zeros_like(xyz))


def test_key_overflow_takes_the_status_path():
    from lcrnet_amd.downsample import voxel_down_sample, voxel_down_sample_device
    rng = np.random.default_rng(8)
    # ~2^12 voxels per axis: 36 key bits, more than a 32-bit promise -> status bit; the wrapper retries with full key bits
    wide = np.concatenate([rng.uniform(0, 1200, size=(3000, 3)), rng.random((3000, 1))], axis=1).astype(np.float32)
    _, _, _, st = _device([wide], 4, hint=32)
    assert st & 1
    f32, f64, _, lh = voxel_down_sample(torch.from_numpy(wide).cuda(), torch.tensor([len(wide)], device="cuda"), 0.3, 4, want_f64=True)
    w32, w64, _ = restate(wide, 0.3, 4)
    assert lh == [len(w32)] and _same(f32.cpu().numpy(), w32) and _same(f64.cpu().numpy(), w64)
    # an axis of more than INT_MAX voxels (Open3D refuses it) cannot be retried: the call raises
    huge = np.array([[0, 0, 0, 0], [1.0e9, 1.0, 1.0, 0]], np.float32)
    with pytest.raises(RuntimeError):
        voxel_down_sample(torch.from_numpy(huge).cuda(), torch.tensor([2], device="cuda"), 0.3, 3)
    out, _, _, status = voxel_down_sample_device(torch.from_numpy(huge).cuda(), torch.tensor([2], device="cuda"), 0.3, 3)
    assert int(status.item()) & 1
