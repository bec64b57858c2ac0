"""Loop ground truth of a sequence from its scans and poses: range-image overlap labels ("the frames that overlap frame i by more than
0.3", the format of the reference's `loop_gt_seq00_0.3overlap_inactive.npz` that `evaluation.compute_topN` / `compute_PR_overlap` consume)
and the distance-based loop pairs of the reference's `generate_*_loop_pairs_distance_npz` (data/Kitti/generate_kitti_loop_pairs.py).

The overlaps run on the GPU (include/lcr_hip.h, lcr_range_images / lcr_scan_overlap; no CPU fallback); the pair screens, the labels and
the loop pairs are host work on the poses alone."""
import numpy as np
import torch

from . import functional as F

BLOCK = F.SCAN_OVERLAP_MAX_CLOUDS // 2      # frames per block: a call sees the clouds of at most two blocks
MAX_PAIRS_PER_CALL = 1 << 16


def relative_transforms(poses, pairs):
    """rel f64 [P,3,4] = inv(T_i) T_j for pairs (i, j): frame j's points expressed in frame i, in fp64 on the host."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return np.zeros((0, 3, 4))
    inv = np.linalg.inv(poses)
    return np.ascontiguousarray(np.matmul(inv[pairs[:, 0]], poses[pairs[:, 1]])[:, :3, :4])


def overlap_from_counts(counts, denom="current"):
    """counts int [P,3] = (matches, valid_cur, valid_ref) -> overlap f64 [P]: matches / valid_cur ("current", the default), or
    matches / min(valid_cur, valid_ref) ("min"); 0 where the denominator is 0."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    if denom == "current":
        den = c[:, 1]
    elif denom == "min":
        den = np.minimum(c[:, 1], c[:, 2])
    else:
        raise ValueError("denom must be 'current' or 'min', got %r" % (denom,))
    out = np.zeros(len(c), dtype=np.float64)
    np.divide(c[:, 0], den, out=out, where=den > 0)
    return out


def scan_overlaps(points, lengths, poses, pairs, denom="current", eps=1.0, **proj):
    """Range-image overlap of P pairs of a sequence's scans.

    points f32 [N,3] (torch on the device, or NumPy: uploaded block by block) stacked frame-major, lengths ints [F], poses f64 [F,4,4]
    (sensor to world), pairs ints [P,2] of (i, j): frame j is projected into frame i through inv(T_i) T_j and compared with frame i's
    range image.  proj: H, W, fov_up, fov_down, max_range (functional.SCAN_OVERLAP_PROJ).  Returns (overlap f64 [P], counts int32 [P,3]
    = (matches, valid_cur, valid_ref)) as NumPy arrays.  More than 64 frames are handled in blocks of 32 (a call holds the two blocks a
    pair touches), large P in calls of 65 536 pairs."""
    bad = set(proj) - set(F.SCAN_OVERLAP_PROJ)
    if bad:
        raise TypeError("scan_overlaps: unknown projection parameters %s" % sorted(bad))
    ln = np.asarray(lengths, dtype=np.int64).reshape(-1)
    nf = len(ln)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(poses) != nf:
        raise ValueError("scan_overlaps: %d poses for %d frames" % (len(poses), nf))
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= nf):
        raise ValueError("scan_overlaps: pair index outside 0..%d" % (nf - 1))
    counts = np.zeros((len(pairs), 3), dtype=np.int32)
    if len(pairs) == 0:
        return overlap_from_counts(counts, denom), counts
    on_device = torch.is_tensor(points)
    if on_device:
        F._lib.require_cuda(points)
    dev = points.device if on_device else torch.device("cuda", torch.cuda.current_device())
    off = np.concatenate([[0], np.cumsum(ln)])
    rel = relative_transforms(poses, pairs)
    blk = pairs // BLOCK
    lo, hi = blk.min(axis=1), blk.max(axis=1)
    key = lo * (nf // BLOCK + 1) + hi
    order = np.argsort(key, kind="stable")
    bounds = np.flatnonzero(np.diff(key[order])) + 1
    for grp in np.split(order, bounds):
        a, b = int(lo[grp[0]]), int(hi[grp[0]])
        frames = np.concatenate([np.arange(k * BLOCK, min((k + 1) * BLOCK, nf)) for k in ([a] if a == b else [a, b])])
        local = np.full(nf, -1, dtype=np.int64)
        local[frames] = np.arange(len(frames))
        parts = [points[off[f]:off[f + 1]] for f in frames]
        if on_device:
            pts = torch.cat(parts)
        else:
            pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)).to(dev)
        images, valid = F.range_images(pts, ln[frames], **proj)
        for s in range(0, len(grp), MAX_PAIRS_PER_CALL):
            sel = grp[s:s + MAX_PAIRS_PER_CALL]
            pr = torch.from_numpy(local[pairs[sel]].astype(np.int32)).to(dev)
            c, status = F.scan_overlap(pts, ln[frames], images, valid, pr, torch.from_numpy(rel[sel]).to(dev), eps=eps, **proj)
            c, status = c.cpu().numpy(), int(status.cpu()[0])
            if status != 0:
                raise RuntimeError("lcr_scan_overlap refused pair %d of a call (cloud index out of range)" % (status - 1))
            counts[sel] = c
    return overlap_from_counts(counts, denom), counts


def candidate_pairs(poses, exclude=100, max_range=50.0):
    """Host screen of the pairs worth projecting: int64 [P,2] of (i, j) with j < i - exclude and |t_i - t_j| < 2 max_range, ascending in
    (i, j).  The screen is exact: beyond 2 max_range no point of frame j (within max_range of its sensor) can fall inside max_range of
    frame i, so the projected image is empty and the overlap 0."""
    t = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)[:, :3, 3]
    out = []
    for i in range(int(exclude) + 1, len(t)):
        d = np.sqrt(((t[:i - int(exclude)] - t[i]) ** 2).sum(axis=1))
        j = np.flatnonzero(d < 2.0 * max_range)
        out.append(np.stack([np.full(len(j), i, dtype=np.int64), j.astype(np.int64)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def loop_labels_from_overlap(n_frames, pairs, overlap, thres=0.3):
    """Labels in the format of the reference's overlap ground truth: an object array of length n_frames whose entry i is the ascending
    float64 array of the frames j with overlap(i, j) > thres (empty where there are none)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    overlap = np.asarray(overlap, dtype=np.float64).reshape(-1)
    if len(pairs) != len(overlap):
        raise ValueError("loop_labels_from_overlap: %d pairs, %d overlaps" % (len(pairs), len(overlap)))
    keep = overlap > thres
    labels = np.empty(int(n_frames), dtype=object)
    for i in range(int(n_frames)):
        labels[i] = np.zeros(0, dtype=np.float64)
    for i in np.unique(pairs[keep, 0]):
        labels[i] = np.unique(pairs[keep & (pairs[:, 0] == i), 1]).astype(np.float64)
    return labels


def save_loop_labels(path, labels):
    """Write labels as the reference's asset is stored (np.load(path, allow_pickle=True)['arr_0'])."""
    np.savez_compressed(path, labels)


def load_loop_labels(path):
    z = np.load(path, allow_pickle=True)
    return z["arr_0"] if "arr_0" in z.files else z["data"]


def loop_pairs_by_distance(poses, dis=4.0, start=100, gap=50, seq=0):
    """The contract of the reference's generate_*_loop_pairs_distance_npz: for every frame i >= start, the frames I of 0 .. i - gap whose
    squared position distance to frame i is < dis^2, in ascending index; a frame with at least one gives
    {'seq_id': seq, 'anc_idx': i, 'pos_idx': I, 'pose': inv(poses[I[k]]) poses[i] per k}; frames without a hit are left out.

    The reference searches with faiss, whose fp32 summation order is not pinned; the distance here is the canonical
    ((dx^2 + dy^2) + dz^2) in fp32 on fp32-rounded positions, compared with dis^2 rounded to fp32."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    t = poses[:, :3, 3].astype(np.float32)
    thr = np.float32(dis) * np.float32(dis)
    data = []
    for i in range(int(start), len(poses)):
        hi = i - int(gap) + 1
        if hi <= 0:
            continue
        d = t[:hi] - t[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        idx = np.flatnonzero(d2 < thr).astype(np.int64)
        if len(idx):
            rel = np.stack([np.linalg.inv(poses[k]) @ poses[i] for k in idx])
            data.append({"seq_id": seq, "anc_idx": i, "pos_idx": idx, "pose": rel})
    return data


def save_loop_pairs(path, data):
    """np.savez_compressed(path, data=...) as the reference writes it; io_formats.load_loop_pairs reads it back."""
    data = list(data)
    arr = np.empty(len(data), dtype=object)
    arr[:] = data
    np.savez_compressed(path, data=arr)
