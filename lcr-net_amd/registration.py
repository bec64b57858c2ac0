"""Correspondence RANSAC registration on the GPU: the counterpart of utils/utils/open3d.py:145-173
(`registration_with_ransac_from_correspondences`, Open3D's registration_ransac_based_on_correspondence), which
experiments/registration/eval.py:175-185 runs as the robust baseline (`--method ransac`) against LCR-Net's local-to-global registration.

Open3D samples at random; this RANSAC is deterministic: hypothesis h draws its rows from a counter-based hash of (seed, h, draw), is
scored in fp32 against every correspondence of its pair, and the winner is the hypothesis with the most inliers (ties: smaller inlier
SSE, then smaller h).  The exact definition is in include/lcr_hip.h (lcr_ransac_correspondences).  All of it runs in HIP kernels
(csrc/ransac.hip); a pair gives the same bits alone or inside a batch."""
import numpy as np
import torch

from . import functional as F

# the reference's evaluation settings (experiments/lcrnet/config_reg.py:69-73, config_model.py:24-28)
REF_DISTANCE_THRESHOLD = 0.3
REF_RANSAC_N = 4
REF_NUM_ITERATIONS = 50000


def _device_points(x, device):
    if torch.is_tensor(x):
        return x.detach().to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32).reshape(-1, 3))).to(device)


def ransac_batched(src, ref, start, distance_threshold=REF_DISTANCE_THRESHOLD, ransac_n=REF_RANSAC_N, num_iterations=REF_NUM_ITERATIONS, seed=0):
    """S pairs in one native call.  src / ref: f32 [n,3] device tensors stacked pair-major (pair s = rows [start[s], start[s+1])),
    start: int32 [S+1] device tensor.  -> (T f32 [S,4,4] mapping src onto ref, inliers int32 [S], rmse f32 [S]), all on the device,
    nothing synchronised.  A pair with fewer rows than ransac_n or without a valid hypothesis gets the identity and 0 inliers."""
    T, inliers, rmse, _ = F.ransac_correspondences(src, ref, start, distance_threshold, ransac_n, num_iterations, seed)
    return T, inliers, rmse


def registration_with_ransac_from_correspondences(src_points, ref_points, correspondences=None, distance_threshold=0.05, ransac_n=3,
                                                  num_iterations=10000, seed=0):
    """The reference helper's name, argument order and defaults (utils/utils/open3d.py:145-152), plus `seed`.  src_points / ref_points:
    numpy arrays or torch tensors [N,3] / [M,3]; correspondences: optional [K,2] (src index, ref index), default the identity pairing
    (which needs N == M).  Returns the float64 (4,4) ndarray transform from src to ref, as the reference does."""
    dev = ref_points.device if torch.is_tensor(ref_points) and ref_points.is_cuda else torch.device("cuda", torch.cuda.current_device())
    src = _device_points(src_points, dev)
    ref = _device_points(ref_points, dev)
    if correspondences is not None:
        c = correspondences if torch.is_tensor(correspondences) else torch.from_numpy(np.asarray(correspondences, dtype=np.int64))
        c = c.to(device=dev, dtype=torch.int64).reshape(-1, 2)
        src, ref = src[c[:, 0]].contiguous(), ref[c[:, 1]].contiguous()
    elif src.shape[0] != ref.shape[0]:
        raise ValueError("without correspondences src and ref need the same number of points (%d vs %d)" % (src.shape[0], ref.shape[0]))
    start = torch.tensor([0, src.shape[0]], dtype=torch.int32, device=dev)
    T, _, _ = ransac_batched(src, ref, start, distance_threshold, ransac_n, num_iterations, seed)
    return T[0].cpu().numpy().astype(np.float64)
