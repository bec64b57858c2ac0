"""NetVLADLoupe2 + GatingContext — parameters as in experiments/lcrnet/modules/netvlad/NetVlad.py:12-47, 165-186
(cluster_weights, cluster_weights2, hidden1_weights, bn1, bn2, context_gating.{gating_weights,bn1}); eval forward on the
HIP path (lcr_netvlad_forward), batched over scans; training forward and backward on lcr_netvlad_train_forward / lcr_netvlad_backward
(batch statistics, the reference's cyclic padding restated as row multiplicities)."""
import math

import numpy as np
import torch
import torch.nn as nn

from ... import functional as F


class GatingContext(nn.Module):
    def __init__(self, dim, add_batch_norm=True, normalization="batch"):
        super().__init__()
        assert add_batch_norm and normalization == "batch"
        self.dim = dim
        self.gating_weights = nn.Parameter(torch.randn(dim, dim) * 1 / math.sqrt(dim))
        self.bn1 = nn.BatchNorm1d(dim)


class NetVLADLoupe2(nn.Module):
    def __init__(self, feature_size, cluster_size, output_dim, gating=True, add_norm=True, is_training=True, normalization="batch"):
        super().__init__()
        assert (feature_size, cluster_size, output_dim) == (1024, 64, 256) and gating and add_norm and normalization == "batch", \
            "the HIP head implements the reference configuration (1024-D x 64 clusters -> 256-D, gating, BatchNorm)"
        self.feature_size, self.output_dim, self.cluster_size = feature_size, output_dim, cluster_size
        self.cluster_weights = nn.Parameter(torch.randn(feature_size, cluster_size) * 1 / math.sqrt(feature_size))
        self.cluster_weights2 = nn.Parameter(torch.randn(1, feature_size, cluster_size) * 1 / math.sqrt(feature_size))
        self.hidden1_weights = nn.Parameter(torch.randn(cluster_size * feature_size, output_dim) * 1 / math.sqrt(feature_size))
        self.bn1 = nn.BatchNorm1d(cluster_size)
        self.bn2 = nn.BatchNorm1d(output_dim)
        self.context_gating = GatingContext(output_dim)

    def _weights(self):
        g = self.context_gating
        w = F.NetvladWeights()
        for name, t in (("cluster_weights", self.cluster_weights), ("cluster_weights2", self.cluster_weights2),
                        ("hidden1_weights", self.hidden1_weights),
                        ("bn1_w", self.bn1.weight), ("bn1_b", self.bn1.bias), ("bn1_mean", self.bn1.running_mean), ("bn1_var", self.bn1.running_var),
                        ("bn2_w", self.bn2.weight), ("bn2_b", self.bn2.bias), ("bn2_mean", self.bn2.running_mean), ("bn2_var", self.bn2.running_var),
                        ("gating_weights", g.gating_weights),
                        ("gbn_w", g.bn1.weight), ("gbn_b", g.bn1.bias), ("gbn_mean", g.bn1.running_mean), ("gbn_var", g.bn1.running_var)):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
            setattr(w, name, t.data_ptr())
        return w

    def _grad_params(self):
        """the ten trainable tensors in functional.NETVLAD_GRAD_NAMES order"""
        g = self.context_gating
        return (self.cluster_weights, self.cluster_weights2, self.hidden1_weights, self.bn1.weight, self.bn1.bias, self.bn2.weight, self.bn2.bias,
                g.gating_weights, g.bn1.weight, g.bn1.bias)

    def _track(self, stats, rows):
        """nn.BatchNorm1d's running statistics from the batch statistics of one training call (mean, biased variance; `rows` values per
        channel for bn1, S for the other two): momentum 0.1, unbiased variance, device ops only."""
        S = rows[1]
        o = 0
        with torch.no_grad():
            for bn, n in ((self.bn1, rows[0]), (self.bn2, S), (self.context_gating.bn1, S)):
                c = bn.num_features
                mean, var = stats[o:o + c], stats[o + c:o + 2 * c]
                o += 2 * c
                if not bn.track_running_stats or bn.running_mean is None:
                    continue
                assert bn.momentum is not None, "cumulative-average BatchNorm would read the counter on the host"
                bn.num_batches_tracked += 1
                m = bn.momentum
                bn.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
                bn.running_var.mul_(1.0 - m).add_(var, alpha=m * n / (n - 1.0))

    def describe(self, feats, lengths_host):
        """Stacked coarse features [sum(len),1024] of S scans -> [S,256] L2-normalised descriptors
        (= GlobalDescritionHEAD per scan: F.normalize -> netvlad -> F.normalize).

        Eval mode: running statistics, one lcr_netvlad_forward call, never a graph.  Training mode: the reference's training branch
        (LCRNet_GlobalDescrition.py:40-57 — cyclic padding to the longest cloud, batch statistics in all three BatchNorm1d, uniform assignment
        on the padding rows) through lcr_netvlad_train_forward; the running buffers are updated as nn.BatchNorm1d does; with grad mode on and an
        input or parameter requiring grad the result carries a graph whose backward is lcr_netvlad_backward."""
        if not self.training:
            return F.netvlad_forward(feats.contiguous(), np.asarray(lengths_host, dtype=np.int64), self._weights())
        seg = np.asarray(lengths_host, dtype=np.int64)
        params = self._grad_params()
        if F._wants_grad(feats, *params):
            out, stats = F._NetvladTrainFn.apply(feats, self, seg, *params)
        else:
            out, stats, _ = F.netvlad_train(feats.detach().contiguous(), seg, self._weights())
        self._track(stats, (float(len(seg)) * float(seg.max()), float(len(seg))))
        return out
