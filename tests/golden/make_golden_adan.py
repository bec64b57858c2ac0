"""Golden vectors for the Adan optimiser from the IMPORTED reference (build container only, CPU).

    python tests/golden/make_golden_adan.py

Runs, unmodified, the Adan class of experiments/lcrnet/adan.py on the seeded cases of tests/adan_restatement.py for K steps, once with
foreach=True and once with foreach=False, and saves after every step the five tensors its state holds per parameter (p, exp_avg,
exp_avg_sq, exp_avg_diff, pre_grad; layout: adan_restatement.pack / Golden), a checksum of every case's inputs, and the key names of its
state_dict().  Output: tests/golden/adan_golden.npz.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"


def reference_adan():
    spec = importlib.util.spec_from_file_location("reference_adan", os.path.join(REF, "experiments", "lcrnet", "adan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Adan


def run_reference(Adan, R, name, foreach):
    p0, grads = R.case_inputs(name)
    groups, max_norm = R.case_groups(name)
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
    pg = []
    for idx, h in groups:
        pg.append(dict(params=[params[i] for i in idx], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["weight_decay"],
                       no_prox=h["no_prox"]))
    opt = Adan(pg, max_grad_norm=max_norm, foreach=foreach)
    per_q = {q: [] for q in R.QUANTITIES}
    for gk in grads:
        for p, g in zip(params, gk):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
        for q in R.QUANTITIES:
            row = []
            for p in params:
                st = opt.state.get(p, {})
                row.append(p.detach().numpy().copy() if q == "p" and len(st) else (st[q].numpy().copy() if q in st else None))
            per_q[q].append(row)
    return per_q, opt


def main():
    import adan_restatement as R
    Adan = reference_adan()
    out = {}
    for name in sorted(R.CASES):
        out[name + "_digest"] = R.digest(name)
        single, opt = run_reference(Adan, R, name, False)
        multi, _ = run_reference(Adan, R, name, True)
        for q in R.QUANTITIES:
            a, b = R.pack(single[q]), R.pack(multi[q])
            assert np.array_equal(np.isnan(a), np.isnan(b))
            out["%s_single_%s" % (name, q)] = a
            out["%s_foreach_%s_ulps" % (name, q)] = b.view(np.int32) - a.view(np.int32)
    sd = opt.state_dict()
    out["state_dict_keys"] = np.array(sorted(sd))
    out["state_dict_group_keys"] = np.array(sorted(sd["param_groups"][0]))
    out["state_dict_state_keys"] = np.array(sorted(sd["state"][0]))
    np.savez_compressed(R.GOLDEN, **out)
    print("wrote", R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
