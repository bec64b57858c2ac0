"""Open3D's voxel down-sampling on the GPU: `PointCloud.voxel_down_sample(v)` of the reference's dataset scripts
(data/Kitti/downsample_pcd.py:29, data/Kitti_360/downsample_pcd.py, data/mulran/downsample_pcd_mulran.py) and of its helper
`voxel_downsample` (utils/utils/open3d.py:61-69), through `lcr_voxel_down_sample` (csrc/grid_subsample.hip).  The semantics —
fp64 origin min - v/2, fp64 in-order averages, libstdc++ unordered_map order over hash_eigen codes — are stated in
include/lcr_hip.h; this is a different function from the grid subsampling of the model's collate (`modules/ops/grid_subsample.py`)."""

import numpy as np
import torch

from . import _lib

MAX_CLOUDS = 64          # clouds per native call (GS_MAX_B)
STATUS_KEY_OVERFLOW, STATUS_LEN_MISMATCH = 1, 2


def voxel_down_sample_device(rows, lengths, voxel_size, out_cols=3, want_f64=False, key_bits_hint=0):
    """Sync-free form for <= 64 clouds: rows device f32 [N, R] (x, y, z first, 3 <= R <= 64), lengths i64 [B].
    Returns (out_f32 [N, out_cols] capacity buffer, out_f64 or None, out_len i64 [B] on device, status i32 [1]).
    key_bits_hint > 0 promises packed-index-key bits + cloud-id bits <= hint (fewer radix passes); a broken promise sets
    LCR_STATUS_KEY_OVERFLOW in `status` and the caller must retry with 0."""
    _lib.require_cuda(rows, lengths)
    if rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous():
        raise RuntimeError("rows must be a contiguous float tensor [N, R]")
    if lengths.dtype != torch.int64:
        raise RuntimeError("lengths must be an long tensor")
    R = int(rows.shape[1])
    if not 3 <= out_cols <= R <= 64:
        raise RuntimeError("voxel_down_sample: need 3 <= out_cols (%d) <= row width (%d) <= 64" % (out_cols, R))
    dev = rows.device
    lengths = lengths.to(dev, non_blocking=True).contiguous()
    B, n = lengths.numel(), rows.shape[0]
    if not 1 <= B <= MAX_CLOUDS:
        raise RuntimeError("voxel_down_sample_device: 1..%d clouds per call" % MAX_CLOUDS)
    ws = _lib.ws("lcr_voxel_down_sample_ws_bytes", n, B, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty((max(n, 1), out_cols), dtype=torch.float32, device=dev)
    out64 = torch.empty((max(n, 1), out_cols), dtype=torch.float64, device=dev) if want_f64 else None
    out_len = torch.empty((B,), dtype=torch.int64, device=dev)
    _lib.call.lcr_voxel_down_sample(_lib.ptr(rows), R, int(out_cols), _lib.ptr(lengths), B, n, float(voxel_size), int(key_bits_hint), _lib.ptr(out),
                                    _lib.ptr(out64), _lib.ptr(out_len), _lib.ptr(status), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    return out, out64, out_len, status


def _one_call(rows, lengths, voxel_size, out_cols, want_f64, key_bits_hint):
    out, out64, out_len, status = voxel_down_sample_device(rows, lengths, voxel_size, out_cols, want_f64, key_bits_hint)
    host = torch.cat([out_len, status.long()]).cpu()        # host sync: the output shape is data dependent
    st = int(host[-1])
    if st & STATUS_KEY_OVERFLOW and key_bits_hint:
        return _one_call(rows, lengths, voxel_size, out_cols, want_f64, 0)
    if st:
        raise RuntimeError("voxel_down_sample: device status 0x%x (voxel index key overflow / length mismatch)" % st)
    lh = host[:-1].tolist()
    m = sum(lh)
    return out[:m], (out64[:m] if want_f64 else None), out_len, lh


def voxel_down_sample(rows, lengths, voxel_size, out_cols=3, want_f64=False, key_bits_hint=32):
    """Stacked clouds on the device -> (points f32 [M, out_cols], points f64 [M, out_cols] or None, lengths i64 [B] on device,
    lengths as a host list).  Stacks of more than 64 clouds are processed 64 at a time (clouds are independent)."""
    if lengths.numel() <= MAX_CLOUDS:
        return _one_call(rows.contiguous(), lengths, voxel_size, out_cols, want_f64, key_bits_hint)
    lens = [int(x) for x in lengths.tolist()]
    if sum(lens) != rows.shape[0]:
        raise RuntimeError("voxel_down_sample: lengths do not match the row tensor")
    parts, parts64, dlens, hlens, o = [], [], [], [], 0
    for g in range(0, len(lens), MAX_CLOUDS):
        n_g = sum(lens[g:g + MAX_CLOUDS])
        p, p64, dl, hl = _one_call(rows[o:o + n_g].contiguous(), lengths[g:g + MAX_CLOUDS].contiguous(), voxel_size, out_cols, want_f64,
                                   key_bits_hint)
        parts.append(p)
        parts64.append(p64)
        dlens.append(dl)
        hlens += hl
        o += n_g
    return torch.cat(parts), (torch.cat(parts64) if want_f64 else None), torch.cat(dlens), hlens


def voxel_downsample(points, voxel_size, normals=None, device="cuda"):
    """The reference helper (utils/utils/open3d.py:61-69) with its name and argument order: points [N, 3] (numpy or tensor) ->
    float64 numpy [M, 3], what `np.asarray(pcd.voxel_down_sample(voxel_size).points)` returns.  The input is taken as float32 (the
    reference's clouds are); normals are not supported (no reference caller passes them)."""
    if normals is not None:
        raise ValueError("voxel_downsample: normals are not supported (Open3D's normal averaging is not reproduced)")
    t = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if t.dim() != 2 or t.shape[1] < 3:
        raise ValueError("voxel_downsample: points must be [N, >= 3]")
    _, p64, _, _ = voxel_down_sample(t, torch.tensor([t.shape[0]], dtype=torch.int64, device=t.device), voxel_size, 3, want_f64=True)
    return p64.cpu().numpy()
