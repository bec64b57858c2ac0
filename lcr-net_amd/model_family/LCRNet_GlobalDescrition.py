"""LCRNet_GlobalDescrition — descriptor-only model (experiments/lcrnet/model_family/LCRNet_GlobalDescrition.py:10-108), both
branches.  Same sub-module names (`encoder`, `netvlad`) => `best-model-ld.tar` / `best-model-mixed.tar` load unchanged with
strict=False (0 missing keys; the mixed tar has 203 unexpected ones)."""
import torch
import torch.nn as nn

from ..backbone4 import KPEncoder
from ..modules.netvlad import NetVLADLoupe2
from ..config import make_cfg


def _host_lengths(v):
    return [int(x) for x in (v.tolist() if torch.is_tensor(v) else v)]


class LCRNet_GlobalDescrition(nn.Module):
    def __init__(self, cfg=None):
        super().__init__()
        cfg = cfg or make_cfg()
        b = cfg["backbone"]
        self.encoder = KPEncoder(b["input_dim"], b["init_dim"], b["kernel_size"], b["init_radius"], b["init_sigma"], b["group_norm"])
        self.netvlad = NetVLADLoupe2(feature_size=1024, cluster_size=64, output_dim=256, gating=True, add_norm=True, is_training=False)
        if "train_mode" in cfg:
            self.train_mode = cfg["train_mode"]

    def forward(self, data_dict):
        """Eval (reference :66-74): one stack -> {'anc_global': (1,256)} treating the WHOLE stack as one scan (the reference runs test
        batch_size=1).  With data_dict['segment_lengths'] (per-stage per-scan lengths, device) and data_dict['lengths_c_host'] (coarse-stage
        lengths on the host) every scan of the stack gets its own descriptor: {'anc_global': (S,256)}.

        Training (reference :76-106): the stack holds batch_size anchors, then sum(pos_num) positives, then the negatives; the head runs on
        batch statistics over all of them (NetVLADLoupe2.describe) and the output is {'anc_global' (B,1,256), 'pos_global' (B,P,256),
        'neg_global' (B,Q,256)} — what losses.TripletLoss takes.  train_mode 'half' (from the cfg) runs the encoder without a graph and
        appends the precomputed data_dict['feats_c'] / ['lengths_c']; anything else builds the whole graph.  The coarse lengths come from
        data_dict['lengths_c_host'] or ['lengths_host'][-1] (host lists: no synchronisation), else from ['lengths'][-1]."""
        if not self.training:
            feats = data_dict["features"].detach()
            feats_list = self.encoder(feats, data_dict)
            feats_c = feats_list[-1]
            lens = data_dict.get("lengths_c_host")
            if lens is None:
                lens = [feats_c.shape[0]]
            return {"anc_global": self.netvlad.describe(feats_c, lens), "feats_c": feats_c}
        half = getattr(self, "train_mode", None) == "half"
        feats = data_dict["features"].detach()
        if half:
            with torch.no_grad():
                feats_c = self.encoder(feats, data_dict)[-1]
        else:
            feats_c = self.encoder(feats, data_dict)[-1]
        lens = data_dict.get("lengths_c_host")
        if lens is None:
            lens = data_dict["lengths_host"][-1] if "lengths_host" in data_dict else data_dict["lengths"][-1]
        lens = _host_lengths(lens)
        if half:
            feats_c = torch.cat([feats_c, data_dict["feats_c"].detach()], dim=0)
            lens = lens + _host_lengths(data_dict["lengths_c"])
        glob = self.netvlad.describe(feats_c, lens)
        batch_size, pos_total = int(data_dict["batch_size"]), int(sum(data_dict["pos_num"]))
        return {"anc_global": glob[:batch_size].reshape(batch_size, -1, 256),
                "pos_global": glob[batch_size:batch_size + pos_total].reshape(batch_size, -1, 256),
                "neg_global": glob[batch_size + pos_total:].reshape(batch_size, -1, 256)}


def create_model(cfg=None):
    return LCRNet_GlobalDescrition(cfg)
