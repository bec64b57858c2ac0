"""Golden for the trainable descriptor head from the IMPORTED reference (build container only):
    python tests/golden/make_golden_netvlad_grad.py

The reference's NetVLADLoupe2(1024, 64, 256).train() is driven through the reference's own GlobalDescritionHEAD (its training branch: cyclic
padding, mask, F.normalize; model_family/LCRNet_GlobalDescrition.py:40-57), called as the unbound method on a holder that carries `netvlad` and
`training` — the encoder the model class would also build plays no part in the head.  Case, weights, input and cotangent are those of
tests/netvlad_grad_restatement.py (GOLDEN_CASE; regenerated from their seeds by the test, so only results go into the file).  The scalar that is
differentiated is sum(out * d_out).  If `pytorch_metric_learning` (imported by the model file for its loss) is absent, an empty stand-in module
is registered under that name first.

Stored, from the fp64 run: "out", "grad/<parameter>" of the nine small parameters in full, "grad/dx", for hidden1_weights (67 MB) a seeded sample
of 256 rows ("grad/hidden1_weights/rows", sample_rows()), all 65 536 row sums and the 256 column sums, and the three BatchNorm running buffer
sets after the one call ("buffer/<key>").  Per stored array "err/<name>" = max|fp32 run - fp64 run| of the same reference code: what the
test's tolerance is built from.  Packed greedily into tests/golden/netvlad_grad_golden.npz (+ .partN.npz), every file below 1 MiB."""
import glob
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 900 * 1024
BASE = os.path.join(HERE, "netvlad_grad_golden")


def load_golden():
    out = {}
    for path in [BASE + ".npz"] + sorted(glob.glob(BASE + ".part*.npz")):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def sample_rows():
    return np.sort(np.random.default_rng(4242).choice(65536, size=256, replace=False))


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import make_golden_model as mgm
    mgm.install_stubs()
    mgm.install_ref_ext()
    sys.path.insert(0, mgm.REF)
    try:
        import pytorch_metric_learning  # noqa: F401
    except ImportError:
        for name in ("pytorch_metric_learning", "pytorch_metric_learning.losses", "pytorch_metric_learning.distances",
                     "pytorch_metric_learning.reducers", "pytorch_metric_learning.miners"):
            sys.modules[name] = types.ModuleType(name)
    import netvlad_grad_restatement as R
    from experiments.lcrnet.model_family.LCRNet_GlobalDescrition import LCRNet_GlobalDescrition
    from experiments.lcrnet.modules.netvlad.NetVlad import NetVLADLoupe2
    seg, seed = R.CASES[R.GOLDEN_CASE]
    x, dout = R.features(seg, seed), R.upstream(len(seg), seed)
    rows = torch.from_numpy(sample_rows())
    runs = {}
    for dt in (torch.float32, torch.float64):
        head = NetVLADLoupe2(feature_size=1024, cluster_size=64, output_dim=256, gating=True, add_norm=True, is_training=True)
        head.load_state_dict({k[len(R.PFX):]: v for k, v in R.weights(torch.float32).items()}, strict=False)
        head = head.to(dt).train()
        holder = torch.nn.Module()
        holder.netvlad = head
        holder.train()
        f = x.detach().clone().to(dt).requires_grad_(True)
        out = LCRNet_GlobalDescrition.GlobalDescritionHEAD(holder, f, torch.tensor(seg))
        (out * dout.to(dt)).sum().backward()
        named = dict(head.named_parameters())
        dH = named["hidden1_weights"].grad.double()
        store = {"out": out.detach().double(), "grad/dx": f.grad.double(), "grad/hidden1_weights/rows": dH[rows],
                 "grad/hidden1_weights/row_sums": dH.sum(1), "grad/hidden1_weights/col_sums": dH.sum(0)}
        store.update({"grad/" + k: named[k].grad.double() for k in R.PARAMS if k != "hidden1_weights"})
        sd = head.state_dict()
        for b in R.BNS:
            assert int(sd[b + "num_batches_tracked"]) == 1
            store["buffer/" + b + "running_mean"] = sd[b + "running_mean"].double()
            store["buffer/" + b + "running_var"] = sd[b + "running_var"].double()
        runs[dt] = store
    final = {"seg_lens": np.asarray(seg, dtype=np.int64)}
    for k, v64 in runs[torch.float64].items():
        final[k] = v64.numpy()
        name = k.split("/", 1)[1] if k.startswith("grad/") else k
        final["err/" + name] = np.float64((runs[torch.float32][k] - v64).abs().max().item())
        print("%-44s max|.| %.3e  fp32 error %.2e" % (k, v64.abs().max().item(), final["err/" + name]))
    for old in [BASE + ".npz"] + glob.glob(BASE + ".part*.npz"):
        if os.path.exists(old):
            os.remove(old)
    parts, size = [{}], 0
    for k in sorted(final, key=lambda k: (np.asarray(final[k]).nbytes > 4096, k)):
        n = np.asarray(final[k]).nbytes + 256
        if size + n > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = final[k]
        size += n
    for i, part in enumerate(parts):
        path = BASE + (".npz" if i == 0 else ".part%d.npz" % i)
        np.savez(path, **part)
        print(os.path.basename(path), "%.3f MB" % (os.path.getsize(path) / 1e6))
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
