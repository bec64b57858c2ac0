"""SuperPointTargetGenerator — modules/geotransformer/superpoint_target.py:6-43: the ground-truth node correspondences a training step
matches patches on."""
import numpy as np
import torch
import torch.nn as nn


class SuperPointTargetGenerator(nn.Module):
    """Keeps the correspondences whose overlap is strictly above `overlap_threshold` and, only when more than `num_targets` remain, draws
    `num_targets` of them without replacement (superpoint_target.py:27-40).  The reference draws from numpy's global state; here the
    module owns a numpy.random.Generator seeded from `seed` (cfg['seed']), and reseed() puts it back, so a training step can be repeated."""

    def __init__(self, num_targets, overlap_threshold, seed=0):
        super().__init__()
        self.num_targets = int(num_targets)
        self.overlap_threshold = overlap_threshold
        self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)

    def reseed(self, seed=None):
        """Restart the generator (from `seed` if given, which becomes the module's)."""
        if seed is not None:
            self.seed = int(seed)
        self.rng = np.random.default_rng(self.seed)

    @torch.no_grad()
    def forward(self, gt_corr_indices, gt_corr_overlaps):
        """gt_corr_indices (N, 2), gt_corr_overlaps (N,) -> (ref indices, src indices, overlaps) of the selected correspondences."""
        keep = torch.gt(gt_corr_overlaps, self.overlap_threshold)
        gt_corr_overlaps = gt_corr_overlaps[keep]
        gt_corr_indices = gt_corr_indices[keep]
        n = gt_corr_indices.shape[0]
        if n > self.num_targets:
            sel = torch.from_numpy(self.rng.choice(n, self.num_targets, replace=False)).to(gt_corr_indices.device)
            gt_corr_indices = gt_corr_indices[sel]
            gt_corr_overlaps = gt_corr_overlaps[sel]
        return gt_corr_indices[:, 0], gt_corr_indices[:, 1], gt_corr_overlaps
