"""Training-time augmentation and point-limit sampling on the device — what the reference's dataset classes apply per cloud in NumPy
(datasets/registration/kitti/dataset.py:73-115, datasets/loop_detection/kitti/dataset_overlap_online.py:123-153): centred uniform
noise, a random yaw, a random scale, a random shift and `np.random.permutation(L)[:point_limit]`, with the pair's ground-truth transform
composed to match.  The per-cloud values are drawn on the host in fp64 from a seeded numpy Generator (draw_params); the per-point work
— noise, rotation, scale, shift and the selection — is one native call (functional.augment_clouds) over all clouds of a sample or of
several samples, whose random words depend only on (seed, sample_id, original point index).  Results are reproducible from the seed,
not equal to any run of the reference."""
import numpy as np
import torch

from . import functional as F

TRAIN_DEFAULTS = {"point_limit": 30000, "use_augmentation": True, "augmentation_noise": 0.01, "augmentation_min_scale": 0.8,
                  "augmentation_max_scale": 1.2, "augmentation_shift": 2.0, "augmentation_rotation": 1.0, "pos_num": 6, "neg_num": 6}


def yaw_matrix(angle):
    """Rotation.from_euler('zyx', [angle, 0, 0]).as_matrix(): a rotation about z."""
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=np.float64)


def euler_zyx_matrix(angles):
    """Rotation.from_euler('zyx', angles).as_matrix(): extrinsic rotations about z, then y, then x -> Rx(c) Ry(b) Rz(a)."""
    a, b, c = (float(v) for v in angles)
    Rz = yaw_matrix(a)
    Ry = np.array([[np.cos(b), 0.0, np.sin(b)], [0.0, 1.0, 0.0], [-np.sin(b), 0.0, np.cos(b)]], dtype=np.float64)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(c), -np.sin(c)], [0.0, np.sin(c), np.cos(c)]], dtype=np.float64)
    return Rx @ Ry @ Rz


def draw_params(rng, n_clouds, noise, min_scale, max_scale, shift, rotation_factor, rotation="yaw"):
    """The per-cloud values of one sample of `n_clouds` clouds, fp64, from the numpy Generator `rng`: rotation [n,3,3] — yaw
    2 pi u / rotation_factor about z as random_sample_yaw (utils/utils/pointcloud.py:132-138; three uniforms are drawn and the first
    used, as there), or with rotation="euler" the three-angle form of random_sample_rotation (:112-116); scale [n] — ONE value per
    sample, min + (max - min) u, shared by all its clouds; shift [n,3] uniform in [-shift, shift), one per cloud; noise [n] = the
    amplitude."""
    if rotation not in ("yaw", "euler"):
        raise ValueError("draw_params: rotation must be 'yaw' or 'euler'")
    n = int(n_clouds)
    R = np.empty((n, 3, 3), dtype=np.float64)
    for i in range(n):
        euler = rng.random(3) * np.pi * 2 / rotation_factor
        R[i] = yaw_matrix(euler[0]) if rotation == "yaw" else euler_zyx_matrix(euler)
    scale = np.full(n, min_scale + (max_scale - min_scale) * rng.random(), dtype=np.float64)
    shifts = rng.uniform(-shift, shift, size=(n, 3))
    return {"rotation": R, "scale": scale, "shift": shifts, "noise": np.full(n, float(noise), dtype=np.float64)}


def compose_pair_transform(transform, aug_rotation, rotate_ref, scale, ref_shift, src_shift):
    """dataset.py:83-107 in fp64: the transform (src onto ref) of a pair after the augmentation — aug_rotation applied to the ref cloud
    (rotate_ref) or to the src cloud, both clouds scaled by `scale` and shifted by ref_shift / src_shift -> (transform f64 [4,4],
    pos_aug_rotation, anc_aug_rotation): the rotation as float32 under the name the reference sets, None under the other."""
    T = np.asarray(transform, dtype=np.float64)
    A = np.asarray(aug_rotation, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    if rotate_ref:
        R, t = A @ R, A @ t
        pos, anc = A.astype(np.float32), None
    else:
        R = R @ A.T
        pos, anc = None, A.astype(np.float32)
    t = t * scale
    t = -(np.asarray(src_shift, dtype=np.float64) @ R.T) + t + np.asarray(ref_shift, dtype=np.float64)
    out = np.eye(4, dtype=np.float64)
    out[:3, :3], out[:3, 3] = R, t
    return out, pos, anc


def _upload(clouds, device):
    """Clouds as loaded ([N,3] or [N,4], host arrays or tensors on either side) -> (stacked float32 rows on the device, host lengths).  Host
    clouds are stacked in pinned memory and uploaded in one asynchronous copy."""
    lengths = [int(c.shape[0]) for c in clouds]
    cols = {int(c.shape[1]) for c in clouds}
    if len(cols) != 1:
        raise ValueError("augment: the clouds of one call must have the same number of columns")
    if all(torch.is_tensor(c) and c.is_cuda for c in clouds):
        return (clouds[0] if len(clouds) == 1 else torch.cat(clouds, dim=0)).to(torch.float32), lengths
    host = torch.empty((sum(lengths), cols.pop()), dtype=torch.float32).pin_memory()
    o = 0
    for c, n in zip(clouds, lengths):
        host[o:o + n] = c.detach().cpu() if torch.is_tensor(c) else torch.from_numpy(np.asarray(c))
        o += n
    return host.to(device, non_blocking=True), lengths


class _Augmenter:
    """Shared state of the two augmenters: the reference's cfg.train fields, a seed, the numpy Generator of the per-cloud draws and the
    running sample_id that keeps the device-side streams of different clouds apart.  reseed() puts both back, as
    SuperPointTargetGenerator.reseed does, so an epoch can be repeated."""

    def __init__(self, train_cfg=None, seed=0, rotation="yaw", device="cuda"):
        cfg = dict(TRAIN_DEFAULTS)
        cfg.update(dict(train_cfg or {}))
        self.point_limit = cfg["point_limit"]
        self.use_augmentation = bool(cfg["use_augmentation"])
        self.noise, self.min_scale, self.max_scale = cfg["augmentation_noise"], cfg["augmentation_min_scale"], cfg["augmentation_max_scale"]
        self.shift, self.rotation_factor = cfg["augmentation_shift"], cfg["augmentation_rotation"]
        self.pos_num, self.neg_num = int(cfg["pos_num"]), int(cfg["neg_num"])
        self.rotation, self.device = rotation, torch.device(device)
        self.reseed(seed)

    @classmethod
    def from_cfg(cls, cfg, **kw):
        return cls(cfg.get("train"), seed=cfg.get("seed", 0), **kw)

    def reseed(self, seed=None):
        """Restart the generator and the sample counter (from `seed` if given, which becomes the augmenter's)."""
        if seed is not None:
            self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)
        self.next_id = 0

    def _draw(self, n_clouds):
        if self.use_augmentation:
            return draw_params(self.rng, n_clouds, self.noise, self.min_scale, self.max_scale, self.shift, self.rotation_factor, self.rotation)
        return {"rotation": np.tile(np.eye(3), (n_clouds, 1, 1)), "scale": np.ones(n_clouds), "shift": np.zeros((n_clouds, 3)),
                "noise": np.zeros(n_clouds)}

    def _ids(self, n):
        ids = (self.next_id + np.arange(n, dtype=np.int64)) & 0xFFFFFFFF
        self.next_id += n
        return ids.astype(np.uint32)

    def _run(self, clouds, params):
        """One native call over `clouds` with the concatenated per-cloud `params` -> (list of device clouds, host lengths)."""
        rows, lengths = _upload(clouds, self.device)
        limit = int(self.point_limit) if self.point_limit else 0
        points, _ = F.augment_clouds(rows, lengths, self._ids(len(clouds)), params["rotation"], params["scale"], params["shift"], params["noise"],
                                     self.seed, limit)
        out_lengths = [min(n, limit) if limit > 0 else n for n in lengths]
        return list(torch.split(points, out_lengths, dim=0)), out_lengths


def _concat(params):
    return {k: np.concatenate([p[k] for p in params], axis=0) for k in params[0]}


class RegistrationAugmenter(_Augmenter):
    """The pair dataset's sample (datasets/registration/kitti/dataset.py:117-161) from loaded clouds: point limit, augmentation of both
    clouds and the composed transform."""

    def many(self, pairs):
        """pairs: (ref_points, src_points, transform) triples, at most 64 -> the sample dicts, all clouds in ONE native call."""
        params, metas = [], []
        for _, _, transform in pairs:
            # the transform is composed from the values the device applies: the fp64 draws narrowed to fp32
            p = {k: v.astype(np.float32).astype(np.float64) for k, v in self._draw(2).items()}
            rotate_ref = bool(self.rng.random() > 0.5)
            A = p["rotation"][0].copy()
            p["rotation"][0] = A if rotate_ref else np.eye(3)
            p["rotation"][1] = np.eye(3) if rotate_ref else A
            params.append(p)
            if self.use_augmentation:
                metas.append(compose_pair_transform(transform, A, rotate_ref, p["scale"][0], p["shift"][0], p["shift"][1]))
            else:
                metas.append((np.asarray(transform, dtype=np.float64), None, None))
        clouds, _ = self._run([c for ref, src, _ in pairs for c in (ref, src)], _concat(params))
        samples = []
        for i, (T, pos, anc) in enumerate(metas):
            ref, src = clouds[2 * i], clouds[2 * i + 1]
            samples.append({"ref_points": ref, "src_points": src,
                            "ref_feats": torch.ones((ref.shape[0], 1), dtype=torch.float32, device=ref.device),
                            "src_feats": torch.ones((src.shape[0], 1), dtype=torch.float32, device=src.device),
                            "transform": T.astype(np.float32), "pos_aug_rotation": pos, "anc_aug_rotation": anc})
        return samples

    def __call__(self, ref_points, src_points, transform):
        return self.many([(ref_points, src_points, transform)])[0]


class LoopAugmenter(_Augmenter):
    """The online triplet dataset's sample (datasets/loop_detection/kitti/dataset_overlap_online.py:187-234) from loaded clouds: every cloud
    limited and augmented on its own (each gets its own rotation, scale and shift, as each `_augment_point_cloud` call there draws its
    own), positives and negatives stacked with their lengths."""

    def many(self, triplets):
        """triplets: (anc_points, [pos_points..], [neg_points..]); all clouds of all samples in ONE native call (<= 128 clouds)."""
        clouds, params = [], []
        for anc, pos, neg in triplets:
            for c in [anc] + list(pos) + list(neg):
                clouds.append(c)
                params.append(self._draw(1))
        out, lengths = self._run(clouds, _concat(params))
        samples, o = [], 0
        for anc, pos, neg in triplets:
            P, N = len(pos), len(neg)
            a, p, n = out[o], out[o + 1:o + 1 + P], out[o + 1 + P:o + 1 + P + N]
            lp, lq = lengths[o + 1:o + 1 + P], lengths[o + 1 + P:o + 1 + P + N]
            o += 1 + P + N
            dev = a.device
            s = {"anc_points": a, "anc_lengths": np.int64([a.shape[0]]), "pos_num": P, "neg_num": N,
                 "anc_feats": torch.ones((a.shape[0], 1), dtype=torch.float32, device=dev)}
            for name, parts, ln in (("pos", p, lp), ("neg", n, lq)):
                pts = torch.cat(list(parts), dim=0) if parts else torch.zeros((0, 3), dtype=torch.float32, device=dev)
                s[name + "_points"], s[name + "_lengths"] = pts, np.int64(ln)
                s[name + "_feats"] = torch.ones((pts.shape[0], 1), dtype=torch.float32, device=dev)
            samples.append(s)
        return samples

    def __call__(self, anc_points, pos_points, neg_points):
        return self.many([(anc_points, pos_points, neg_points)])[0]
