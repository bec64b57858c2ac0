"""Correspondence RANSAC registration on the GPU: the counterpart of utils/utils/open3d.py:145-173
(`registration_with_ransac_from_correspondences`, Open3D's registration_ransac_based_on_correspondence), which
experiments/registration/eval.py:175-185 runs as the robust baseline (`--method ransac`) against LCR-Net's local-to-global registration.

Open3D samples at random; this RANSAC is deterministic: hypothesis h draws its rows from a counter-based hash of (seed, h, draw), is
scored in fp32 against every correspondence of its pair, and the winner is the hypothesis with the most inliers (ties: smaller inlier
SSE, then smaller h).  The exact definition is in include/lcr_hip.h (lcr_ransac_correspondences).  All of it runs in HIP kernels
(csrc/ransac.hip); a pair gives the same bits alone or inside a batch.

Feature-matching RANSAC (utils/utils/open3d.py:109-142, `registration_with_ransac_from_feats`: Open3D's
registration_ransac_based_on_feature_matching with an edge-length checker at 0.9 and a distance checker, eval.py's `ransac_featurematch`):
`ransac_from_feats_batched` / `registration_with_ransac_from_feats`.  Exact nearest neighbours in feature space (csrc/feature_nn.hip),
the correspondence list with the optional mutual filter, and the RANSAC above with both checkers, all on the device.

Point-to-point ICP on the dense clouds (Open3D's registration_icp with TransformationEstimationPointToPoint, which the reference's pair
generators run for their ground truth, data/Kitti/generate_kitti_pairs.py:145-147): `registration_icp` (Open3D's call shape) and
`icp_batched` (S pairs per native call, csrc/icp.hip), exact and batch-invariant as include/lcr_hip.h (lcr_icp_point_to_point) states.
Both also run point-to-plane ICP (estimation_method="point_to_plane", Open3D's TransformationEstimationPointToPlane), which needs target
normals: `estimate_normals` / `estimate_normals_batched` compute them on the GPU (csrc/normals.hip; utils/utils/open3d.py:53-58 with a
radius, KDTreeSearchParamHybrid).  Generalized ICP (plane-to-plane, Open3D's registration_generalized_icp) has its own pair of functions,
`registration_generalized_icp` / `gicp_batched`, with the normals of both clouds (lcr_icp_generalized).

TEASER-style robust registration (experiments/registration/eval.py:197-218, `--method teaser`): `teaser_batched` /
`registration_with_teaser_from_correspondences` (csrc/teaser.hip; consistency graph, k-core selection, GNC-TLS rotation, voted
translation, as include/lcr_hip.h states under lcr_teaser_registration)."""
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


# ---- feature-matching RANSAC (utils/utils/open3d.py:109-142) ----
REF_EDGE_SIMILARITY = 0.9            # CorrespondenceCheckerBasedOnEdgeLength(0.9), utils/utils/open3d.py:131


def _starts(lengths, device):
    """int32 [S+1] row offsets on the device from per-pair lengths (a host sequence, or a device tensor: no synchronisation)."""
    if torch.is_tensor(lengths) and lengths.is_cuda:
        z = torch.zeros((1,), dtype=torch.int32, device=device)
        return torch.cat([z, torch.cumsum(lengths.to(device=device, dtype=torch.int64).reshape(-1), 0).to(torch.int32)])
    ln = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
    return torch.from_numpy(np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)).to(device)


def ransac_from_feats_batched(src_points, ref_points, src_feats, ref_feats, src_len, ref_len, distance_threshold=REF_DISTANCE_THRESHOLD,
                              ransac_n=REF_RANSAC_N, num_iterations=REF_NUM_ITERATIONS, seed=0, mutual_filter=False,
                              edge_similarity=REF_EDGE_SIMILARITY, want_corr=False, want_reject=False):
    """Feature-matching RANSAC for S pairs, everything on the device and nothing synchronised.  src_points f32 [ns,3] / ref_points
    f32 [nr,3] and src_feats f32 [ns,C] / ref_feats f32 [nr,C]: device tensors stacked pair-major; src_len / ref_len: S lengths (host
    sequences or device tensors).  Per pair: every source row is matched to its exact nearest reference row in feature space
    (functional.feature_nn), with mutual_filter only rows whose match points back are kept (a pair left with fewer than ransac_n rows
    falls back to all of them, as Open3D does), and the checked RANSAC (edge-length similarity `edge_similarity`, distance checker at
    `distance_threshold`) runs on those correspondences.  -> dict of device tensors: T f32 [S,4,4] (src onto ref), inliers int32 [S],
    rmse f32 [S], best_h int32 [S], num_corr int32 [S]; with want_corr also corr int32 [ns,2] (pair-local rows; the first start[S] are
    valid) and start int32 [S+1]; with want_reject reject_all uint8 [S*num_iterations] (0 valid, 1 degenerate, 2 edge, 3 distance)."""
    dev = src_points.device
    src_start, ref_start = _starts(src_len, dev), _starts(ref_len, dev)
    nn_sr, _ = F.feature_nn(src_feats, ref_feats, src_start, ref_start)
    nn_rs = F.feature_nn(ref_feats, src_feats, ref_start, src_start)[0] if mutual_filter else None
    corr, start, _ = F.feature_correspondences(nn_sr, src_start, ref_start, nn_rs, min_rows=ransac_n)
    out = F.ransac_correspondences_ex(src_points, ref_points, start, distance_threshold, ransac_n, num_iterations, seed,
                                      edge_similarity=edge_similarity, checker_distance=distance_threshold, corr=corr, src_start=src_start,
                                      ref_start=ref_start, want_reject=want_reject)
    res = {"T": out[0], "inliers": out[1], "rmse": out[2], "best_h": out[3], "num_corr": start[1:] - start[:-1]}
    if want_corr:
        res.update(corr=corr, start=start)
    if want_reject:
        res["reject_all"] = out[4]
    return res


def _device_feats(x, device):
    if torch.is_tensor(x):
        return x.detach().to(device=device, dtype=torch.float32).reshape(x.shape[0], -1).contiguous()
    x = np.asarray(x, dtype=np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], -1))).to(device)


def registration_with_ransac_from_feats(src_points, ref_points, src_feats, ref_feats, distance_threshold=0.05, ransac_n=3, num_iterations=50000,
                                        val_iterations=1000, seed=0, mutual_filter=False):
    """The reference helper's name, argument order and defaults (utils/utils/open3d.py:109-118), plus `seed` and `mutual_filter` (False:
    the reference calls the Open3D signature that has none).  src_points / ref_points: numpy arrays or torch tensors [N,3] / [M,3],
    src_feats / ref_feats [N,C] / [M,C].  Edge-length checker at 0.9 and distance checker at distance_threshold, as the reference sets
    them.  `val_iterations` (Open3D's validation budget of RANSACConvergenceCriteria) is accepted and ignored: every one of the
    num_iterations hypotheses runs, as for registration_with_ransac_from_correspondences.  Returns the float64 (4,4) ndarray transform
    from src to ref."""
    dev = ref_points.device if torch.is_tensor(ref_points) and ref_points.is_cuda else torch.device("cuda", torch.cuda.current_device())
    src, ref = _device_points(src_points, dev), _device_points(ref_points, dev)
    sf, rf = _device_feats(src_feats, dev), _device_feats(ref_feats, dev)
    if sf.shape[0] != src.shape[0] or rf.shape[0] != ref.shape[0] or sf.shape[1] != rf.shape[1]:
        raise ValueError("one feature row per point and the same feature width on both sides are needed")
    r = ransac_from_feats_batched(src, ref, sf, rf, [src.shape[0]], [ref.shape[0]], distance_threshold, ransac_n, num_iterations, seed,
                                  mutual_filter=mutual_filter)
    return r["T"][0].cpu().numpy().astype(np.float64)


# ---- point-to-point ICP (Open3D's registration_icp with TransformationEstimationPointToPoint; data/Kitti/generate_kitti_pairs.py:145-147) ----
ICP_MAX_PAIRS_PER_CALL = 64          # S per native call (the support grid's cloud limit); icp_batched splits larger batches


ICP_ESTIMATION_METHODS = ("point_to_point", "point_to_plane")


def _estimation(method, normals):
    if method not in ICP_ESTIMATION_METHODS:
        raise ValueError("estimation_method must be one of %s, not %r" % (ICP_ESTIMATION_METHODS, method))
    if method == "point_to_plane" and normals is None:
        raise ValueError("point-to-plane ICP needs target normals (estimate_normals computes them)")
    return method == "point_to_plane"


def icp_batched(src, src_len, tgt, tgt_len, init, max_correspondence_distance, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                check_every=16, want_history=False, want_corr=False, estimation_method="point_to_point", tgt_normals=None):
    """ICP for S pairs on the GPU.  src f32 [ns,3] / tgt f32 [nt,3]: device tensors stacked pair-major, src_len / tgt_len: host sequences
    of S ints, init: [S,4,4] source onto target (any float dtype, any device).  -> dict of device tensors (T f64 [S,4,4], fitness f64 [S],
    inlier_rmse f64 [S], iterations int32 [S], and with want_corr / want_history the corr rows and the per-step history; see
    functional.icp_point_to_point).  estimation_method "point_to_plane" needs tgt_normals f32 [nt,3] on the device (stacked like tgt).
    Batches of more than 64 pairs are split into chunks; every pair's result is the same in any chunk."""
    plane = _estimation(estimation_method, tgt_normals)
    tail = (max_correspondence_distance, max_iteration, relative_fitness, relative_rmse, check_every)
    kw = dict(want_corr=want_corr, want_history=want_history)
    if plane:
        return _icp_chunks(src_len, tgt_len, init, src.device,
                           lambda s, t, sl, tl, T0: F.icp_point_to_plane(src[s], sl, tgt[t], tl, tgt_normals[t], T0, *tail, **kw))
    return _icp_chunks(src_len, tgt_len, init, src.device, lambda s, t, sl, tl, T0: F.icp_point_to_point(src[s], sl, tgt[t], tl, T0, *tail, **kw))


def _icp_chunks(src_len, tgt_len, init, device, one):
    """The chunk loop of icp_batched / gicp_batched: one(source rows, target rows (slices of the stacked arrays), src_len, tgt_len, init
    f64 [s,4,4] on the device) per chunk of at most 64 pairs, the dicts concatenated pair-major."""
    src_len = [int(x) for x in np.asarray(src_len).reshape(-1)]
    tgt_len = [int(x) for x in np.asarray(tgt_len).reshape(-1)]
    S = len(src_len)
    init = (init if torch.is_tensor(init) else torch.from_numpy(np.asarray(init))).to(device=device, dtype=torch.float64).reshape(S, 4, 4)
    so = np.concatenate([[0], np.cumsum(src_len)]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum(tgt_len)]).astype(np.int64)
    parts = []
    for c0 in range(0, S, ICP_MAX_PAIRS_PER_CALL):
        c1 = min(S, c0 + ICP_MAX_PAIRS_PER_CALL)
        parts.append(one(slice(so[c0], so[c1]), slice(to[c0], to[c1]), src_len[c0:c1], tgt_len[c0:c1], init[c0:c1]))
    if len(parts) == 1:
        return parts[0]
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


class ICPResult:
    """What Open3D's RegistrationResult carries: transformation (float64 (4,4) ndarray, source onto target), fitness, inlier_rmse,
    correspondence_set (int64 [K,2]: source row, target row), plus iterations (the updates performed)."""

    def __init__(self, transformation, fitness, inlier_rmse, correspondence_set, iterations):
        self.transformation, self.fitness, self.inlier_rmse = transformation, fitness, inlier_rmse
        self.correspondence_set, self.iterations = correspondence_set, iterations

    def __repr__(self):
        return "ICPResult(fitness=%.6e, inlier_rmse=%.6e, correspondences=%d, iterations=%d)" % (
            self.fitness, self.inlier_rmse, len(self.correspondence_set), self.iterations)


def registration_icp(source, target, max_correspondence_distance, init=np.eye(4), max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
                     estimation_method="point_to_point", target_normals=None):
    """Open3D's call shape, registration_icp(source, target, max_correspondence_distance, init, TransformationEstimationPointToPoint() or
    TransformationEstimationPointToPlane(), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)), on the GPU.
    source / target: numpy arrays or torch tensors [N,3] / [M,3]; estimation_method "point_to_plane" needs target_normals [M,3] (as Open3D
    refuses a target without normals; estimate_normals computes them).  Returns an ICPResult."""
    _estimation(estimation_method, target_normals)
    if torch.is_tensor(target) and target.is_cuda:
        dev = target.device
    elif torch.is_tensor(source) and source.is_cuda:
        dev = source.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    src, tgt = _device_points(source, dev), _device_points(target, dev)
    T0 = (init if torch.is_tensor(init) else torch.from_numpy(np.asarray(init, dtype=np.float64))).to(device=dev, dtype=torch.float64).reshape(1, 4, 4)
    nrm = _device_points(target_normals, dev) if target_normals is not None else None
    r = icp_batched(src, [src.shape[0]], tgt, [tgt.shape[0]], T0, max_correspondence_distance, max_iteration, relative_fitness, relative_rmse,
                    want_corr=True, estimation_method=estimation_method, tgt_normals=nrm)
    corr = r["corr"].cpu().numpy().astype(np.int64)
    rows = np.nonzero(corr >= 0)[0]
    return ICPResult(r["T"][0].cpu().numpy(), float(r["fitness"][0].item()), float(r["inlier_rmse"][0].item()),
                     np.stack([rows, corr[rows]], axis=1).astype(np.int64), int(r["iterations"][0].item()))


# ---- generalized ICP (Open3D's registration_generalized_icp; plane-to-plane, normals of both clouds) ----
def gicp_batched(src, src_len, src_normals, tgt, tgt_len, tgt_normals, init, max_correspondence_distance, epsilon=1e-3, max_iteration=30,
                 relative_fitness=1e-6, relative_rmse=1e-6, check_every=16, want_history=False, want_corr=False):
    """Generalized ICP for S pairs on the GPU: icp_batched's arguments and outputs, with src_normals f32 [ns,3] / tgt_normals f32 [nt,3] on
    the device (stacked like src / tgt) and epsilon, the covariance along a normal (functional.icp_generalized).  Batches of more than 64
    pairs are split into chunks; every pair's result is the same in any chunk."""
    if src_normals is None or tgt_normals is None:
        raise ValueError("generalized ICP needs the normals of both clouds (estimate_normals computes them)")
    tail = (max_correspondence_distance, epsilon, max_iteration, relative_fitness, relative_rmse, check_every)
    return _icp_chunks(src_len, tgt_len, init, src.device,
                       lambda s, t, sl, tl, T0: F.icp_generalized(src[s], sl, src_normals[s], tgt[t], tl, tgt_normals[t], T0, *tail,
                                                                  want_corr=want_corr, want_history=want_history))


def registration_generalized_icp(source, target, max_correspondence_distance, init=np.eye(4), max_iteration=30, relative_fitness=1e-6,
                                 relative_rmse=1e-6, epsilon=1e-3, source_normals=None, target_normals=None, normal_radius=None,
                                 normal_max_nn=30):
    """Open3D's call shape, registration_generalized_icp(source, target, max_correspondence_distance, init,
    TransformationEstimationForGeneralizedICP(epsilon), ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)), on the
    GPU.  source / target: numpy arrays or torch tensors [N,3] / [M,3].  A side without normals gets them from estimate_normals_batched at
    normal_radius / normal_max_nn; without a radius that is a ValueError.  Returns an ICPResult."""
    if (source_normals is None or target_normals is None) and normal_radius is None:
        raise ValueError("generalized ICP needs the normals of both clouds, or normal_radius to estimate the missing ones")
    if torch.is_tensor(target) and target.is_cuda:
        dev = target.device
    elif torch.is_tensor(source) and source.is_cuda:
        dev = source.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    src, tgt = _device_points(source, dev), _device_points(target, dev)
    T0 = (init if torch.is_tensor(init) else torch.from_numpy(np.asarray(init, dtype=np.float64))).to(device=dev, dtype=torch.float64).reshape(1, 4, 4)

    def normals_of(given, cloud):
        if given is not None:
            return _device_points(given, dev)
        return estimate_normals_batched(cloud, [cloud.shape[0]], normal_radius, normal_max_nn)["normals"]

    r = gicp_batched(src, [src.shape[0]], normals_of(source_normals, src), tgt, [tgt.shape[0]], normals_of(target_normals, tgt), T0,
                     max_correspondence_distance, epsilon, max_iteration, relative_fitness, relative_rmse, want_corr=True)
    corr = r["corr"].cpu().numpy().astype(np.int64)
    rows = np.nonzero(corr >= 0)[0]
    return ICPResult(r["T"][0].cpu().numpy(), float(r["fitness"][0].item()), float(r["inlier_rmse"][0].item()),
                     np.stack([rows, corr[rows]], axis=1).astype(np.int64), int(r["iterations"][0].item()))


# ---- surface normals (utils/utils/open3d.py:53-58 with KDTreeSearchParamHybrid(radius, max_nn)) ----
def estimate_normals_batched(points, lengths, radius, max_nn=30, viewpoint=None, want_curvature=False, want_count=False):
    """Normals for B clouds on the GPU.  points f32 [N,3]: a device tensor stacked cloud-major, lengths: host sequence of B ints,
    viewpoint: None (every cloud's origin) or [B,3].  -> dict of device tensors (normals f32 [N,3], and curvature / count on request;
    see functional.estimate_normals).  Batches of more than 64 clouds are split; every cloud's result is the same in any chunk."""
    lengths = [int(x) for x in np.asarray(lengths).reshape(-1)]
    B = len(lengths)
    dev = points.device
    if viewpoint is not None:
        viewpoint = (viewpoint if torch.is_tensor(viewpoint) else torch.from_numpy(np.asarray(viewpoint, dtype=np.float32)))
        viewpoint = viewpoint.to(device=dev, dtype=torch.float32).reshape(B, 3)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    parts = []
    for c0 in range(0, B, F.NORMALS_MAX_CLOUDS):
        c1 = min(B, c0 + F.NORMALS_MAX_CLOUDS)
        parts.append(F.estimate_normals(points[off[c0]:off[c1]], lengths[c0:c1], radius, max_nn, viewpoint[c0:c1] if viewpoint is not None else None,
                                        want_curvature=want_curvature, want_count=want_count))
    if len(parts) == 1:
        return parts[0]
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


def estimate_normals(points, radius, max_nn=30, viewpoint=(0.0, 0.0, 0.0)):
    """Normals of one cloud, as utils/utils/open3d.py:estimate_normals computes them with a radius (Open3D's
    KDTreeSearchParamHybrid(radius, max_nn)), oriented toward `viewpoint` (default the sensor at the origin).  points: numpy array or torch
    tensor [N,3]; returns the same kind (numpy float32, or a float32 tensor on the GPU).  A radius is required: Open3D's parameterless
    default (KDTreeSearchParamKNN(30)) is not offered.  Degenerate rows (fewer than 3 neighbours, coincident or collinear ones) get the
    zero normal."""
    if radius is None:
        raise ValueError("estimate_normals needs a search radius")
    dev = points.device if torch.is_tensor(points) and points.is_cuda else torch.device("cuda", torch.cuda.current_device())
    pts = _device_points(points, dev)
    vp = torch.tensor(np.asarray(viewpoint, dtype=np.float32).reshape(1, 3), device=dev)
    n = estimate_normals_batched(pts, [pts.shape[0]], radius, max_nn, vp)["normals"]
    if torch.is_tensor(points):
        return n
    return n.cpu().numpy()


# ---- FPFH descriptors (Open3D's compute_fpfh_feature) and the learning-free chain normals -> FPFH -> feature-matching RANSAC ----
def compute_fpfh_feature_batched(points, normals, lengths, radius, max_nn=100):
    """FPFH for B clouds on the GPU.  points / normals f32 [N,3]: device tensors stacked cloud-major, lengths: host sequence of B ints.
    -> device f32 [N,33] (see functional.fpfh and include/lcr_hip.h, lcr_fpfh).  Batches of more than 64 clouds are split; every cloud's
    result is the same in any chunk."""
    lengths = [int(x) for x in np.asarray(lengths).reshape(-1)]
    B = len(lengths)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    parts = []
    for c0 in range(0, B, F.FPFH_MAX_CLOUDS):
        c1 = min(B, c0 + F.FPFH_MAX_CLOUDS)
        parts.append(F.fpfh(points[off[c0]:off[c1]], normals[off[c0]:off[c1]], lengths[c0:c1], radius, max_nn)["features"])
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def compute_fpfh_feature(points, normals, radius, max_nn=100):
    """FPFH of one cloud: Open3D's compute_fpfh_feature(cloud, KDTreeSearchParamHybrid(radius, max_nn)), as an (N,33) array, which is the
    (N,C) layout registration_with_ransac_from_feats and the reference's make_open3d_registration_feature take (Open3D's own Feature.data
    is the transpose).  points / normals: numpy arrays or torch tensors [N,3]; returns the same kind as points (numpy float32, or a
    float32 tensor on the GPU)."""
    dev = points.device if torch.is_tensor(points) and points.is_cuda else torch.device("cuda", torch.cuda.current_device())
    pts, nrm = _device_points(points, dev), _device_points(normals, dev)
    if pts.shape != nrm.shape:
        raise ValueError("compute_fpfh_feature needs one normal per point")
    f = compute_fpfh_feature_batched(pts, nrm, [pts.shape[0]], radius, max_nn)
    if torch.is_tensor(points):
        return f
    return f.cpu().numpy()


def fpfh_ransac_batched(src, src_len, ref, ref_len, normal_radius, normal_max_nn, feature_radius, feature_max_nn, src_viewpoint=None,
                        ref_viewpoint=None, **ransac_kw):
    """The learning-free registration chain for S pairs, everything on the device: normals of every cloud (oriented toward its viewpoint;
    None = each cloud's origin, the sensor) -> FPFH -> ransac_from_feats_batched (exact feature nearest neighbours, checked RANSAC;
    ransac_kw are its keyword arguments).  src f32 [ns,3] / ref f32 [nr,3]: device tensors stacked pair-major, src_len / ref_len: host
    sequences of S ints.  -> the dict of ransac_from_feats_batched (T f32 [S,4,4] maps src onto ref)."""
    feats = []
    for pts, ln, vp in ((src, src_len, src_viewpoint), (ref, ref_len, ref_viewpoint)):
        nrm = estimate_normals_batched(pts, ln, normal_radius, normal_max_nn, vp)["normals"]
        feats.append(compute_fpfh_feature_batched(pts, nrm, ln, feature_radius, feature_max_nn))
    return ransac_from_feats_batched(src, ref, feats[0], feats[1], src_len, ref_len, **ransac_kw)


# ---- TEASER-style robust registration (experiments/registration/eval.py:197-218, `--method teaser`) ----
# The reference's solver settings (eval.py:199-208).
REF_TEASER_NOISE_BOUND = 0.01
REF_TEASER_CBAR2 = 1.0
REF_TEASER_GNC_FACTOR = 1.4
REF_TEASER_MAX_ITERATIONS = 100
REF_TEASER_COST_THRESHOLD = 1e-12


def teaser_batched(src, ref, start, noise_bound=REF_TEASER_NOISE_BOUND, cbar2=REF_TEASER_CBAR2, gnc_factor=REF_TEASER_GNC_FACTOR,
                   max_iterations=REF_TEASER_MAX_ITERATIONS, cost_threshold=REF_TEASER_COST_THRESHOLD, inlier_selection="kcore",
                   max_rows=None):
    """S problems in one native call (csrc/teaser.hip; the definition is in include/lcr_hip.h, lcr_teaser_registration): consistency
    graph, k-core selection (inlier_selection "kcore", or "none" for every row), GNC-TLS rotation over all pairs of the selected rows and a
    truncated-least-squares vote per translation axis.  src / ref: f32 [n,3] device tensors stacked problem-major, start: int32 [S+1]
    device tensor, at most 4096 rows per problem.  -> dict of device tensors, nothing synchronised: T f32 [S,4,4] (src onto ref),
    valid int32 [S] (0: no edge or fewer than 3 selected rows, identity), n_selected int32 [S], rot_inliers int64 [S], t_count int32 [S,3]."""
    T, valid, nsel, rot, tcount = F.teaser_registration(src, ref, start, noise_bound, cbar2, gnc_factor, max_iterations, cost_threshold,
                                                        inlier_selection, max_rows)
    return {"T": T, "valid": valid, "n_selected": nsel, "rot_inliers": rot, "t_count": tcount}


def registration_with_teaser_from_correspondences(src_corr_points, ref_corr_points, noise_bound=0.01, cbar2=1.0, rotation_gnc_factor=1.4,
                                                  rotation_max_iterations=100, rotation_cost_threshold=1e-12, inlier_selection="kcore"):
    """What eval.py:197-218 asks of TEASER++ for one pair, in the argument order of registration_with_ransac_from_correspondences:
    src_corr_points / ref_corr_points are numpy arrays or torch tensors [N,3], row i of one corresponding to row i of the other (at most
    4096 rows).  Returns the float64 (4,4) ndarray transform from src to ref with the bottom row (0, 0, 0, 1); the identity when the
    problem is invalid."""
    if inlier_selection not in F.TEASER_MODES:
        raise ValueError("inlier_selection must be 'kcore' or 'none', got %r" % (inlier_selection,))
    n_src, n_ref = (int(np.prod(x.shape)) // 3 for x in (src_corr_points, ref_corr_points))
    if n_src != n_ref:
        raise ValueError("src_corr_points and ref_corr_points need the same number of rows (%d vs %d)" % (n_src, n_ref))
    if n_src > F.TEASER_MAX_ROWS:
        raise ValueError("at most %d correspondences per problem (%d given): keep the best by score first" % (F.TEASER_MAX_ROWS, n_src))
    dev = ref_corr_points.device if torch.is_tensor(ref_corr_points) and ref_corr_points.is_cuda else None
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError("lcr-net_amd ops run on the GPU only (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    src = _device_points(src_corr_points, dev)
    ref = _device_points(ref_corr_points, dev)
    start = torch.tensor([0, src.shape[0]], dtype=torch.int32, device=dev)
    r = teaser_batched(src, ref, start, noise_bound, cbar2, rotation_gnc_factor, rotation_max_iterations, rotation_cost_threshold,
                       inlier_selection)
    return r["T"][0].cpu().numpy().astype(np.float64)
