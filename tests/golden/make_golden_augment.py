"""Golden vectors for the pair augmentation from the IMPORTED reference (build container only, CPU).

    python tests/golden/make_golden_augment.py

Calls, unmodified and unbound, OdometryKittiPairDataset._augment_point_cloud of experiments/lcrnet/datasets/registration/kitti/dataset.py on
a namespace that holds its five augmentation fields, for seeds 0..7 (np.random.seed(s); random.seed(s) before each call): a 5-point ref
cloud, a 6-point src cloud and a transform with a translation.  Saves the inputs, the outputs, and the draws the method consumed, replayed
from the same seeds in its own call order: rand(5,3), rand(6,3), rand(3) (random_sample_yaw), random() for the side, random() for the
scale, two uniform(-shift, shift, 3).  Both branches (rotation on the ref side / on the src side) must occur.
Output: tests/golden/augment_pair.npz.
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "augment_pair.npz")
SEEDS = list(range(8))
FIELDS = dict(augmentation_noise=0.01, augmentation_min_scale=0.8, augmentation_max_scale=1.2, augmentation_shift=2.0, augmentation_rotation=1.0)


def inputs(seed):
    g = np.random.default_rng(1000 + seed)
    ref = g.uniform(-60.0, 60.0, size=(5, 3)).astype(np.float32).astype(np.float64)     # scan files are float32
    src = g.uniform(-60.0, 60.0, size=(6, 3)).astype(np.float32).astype(np.float64)
    a = g.uniform(0.0, 2.0 * np.pi)
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = g.uniform(-5.0, 5.0, size=3)
    return ref, src, T


def main():
    sys.path.insert(0, REF)
    from experiments.lcrnet.datasets.registration.kitti.dataset import OdometryKittiPairDataset
    holder = types.SimpleNamespace(**FIELDS)
    out = {"seeds": np.array(SEEDS), "fields": np.array([FIELDS[k] for k in sorted(FIELDS)]), "field_names": np.array(sorted(FIELDS))}
    sides = []
    for s in SEEDS:
        ref, src, T = inputs(s)
        np.random.seed(s)
        random.seed(s)
        ref2, src2, T2, pos, anc = OdometryKittiPairDataset._augment_point_cloud(holder, ref.copy(), src.copy(), T.copy())
        assert (pos is None) != (anc is None)
        np.random.seed(s)
        random.seed(s)
        u_ref, u_src, u_rot = np.random.rand(5, 3), np.random.rand(6, 3), np.random.rand(3)
        u_side, u_scale = random.random(), random.random()
        ref_shift = np.random.uniform(-FIELDS["augmentation_shift"], FIELDS["augmentation_shift"], 3)
        src_shift = np.random.uniform(-FIELDS["augmentation_shift"], FIELDS["augmentation_shift"], 3)
        assert (u_side > 0.5) == (pos is not None)
        sides.append(pos is not None)
        for name, value in (("ref", ref), ("src", src), ("transform", T), ("ref_out", ref2), ("src_out", src2), ("transform_out", T2),
                            ("aug_rotation", pos if pos is not None else anc), ("rotate_ref", np.array(pos is not None)), ("u_ref", u_ref),
                            ("u_src", u_src), ("u_rot", u_rot), ("u_side", np.array(u_side)), ("u_scale", np.array(u_scale)),
                            ("ref_shift", ref_shift), ("src_shift", src_shift)):
            out["s%d_%s" % (s, name)] = np.asarray(value)
    assert any(sides) and not all(sides), "both branches must occur"
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; ref-side seeds:", [s for s, r in zip(SEEDS, sides) if r])


if __name__ == "__main__":
    main()
