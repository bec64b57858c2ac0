"""(GPU) One Adan step over the parameter list of the full model (model_family.LCRNet: 350 tensors, 25.1 M parameters): the fused HIP
pass (lcrnet_amd.adan.Adan, fused=True) against the torch path of the same class with foreach=True and foreach=False, without and
with global-norm clipping.

    python tools/adan_bench.py [--steps 30] [--rounds 3] [--out FILE]

Per variant: 3 warm-up steps, then `rounds` rounds of `steps` steps, the variants alternating round by round; a step is timed by a pair
of device events around opt.step() (the gradients are restored from a master copy outside the timed span, so every clipped step really
clips) and the median over all timed steps is reported, with the host's wall time per step() call beside it.  Traffic model of the fused
pass: six floats read and five written per element (44 B), six written when the clip factor is below one (48 B); the clipped step also
reads the gradients once more for the norm (52 B in all), which the achieved GB/s does not count.  Share of the HBM roofline: against
the 6.3 TB/s a streaming kernel achieves on this part and against the 8.0 TB/s of the datasheet.  One JSON line per variant."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lcrnet_amd.adan import Adan  # noqa: E402
from lcrnet_amd.config import make_cfg  # noqa: E402
from lcrnet_amd.model_family import LCRNet  # noqa: E402

HBM_ACHIEVABLE, HBM_SPEC = 6.3e12, 8.0e12


class Variant:
    def __init__(self, name, shapes, dev, clip, **kw):
        g = torch.Generator(device="cpu").manual_seed(1)
        self.name, self.clip = name, clip
        self.params = [torch.nn.Parameter((0.5 * torch.randn(s, generator=g)).to(dev)) for s in shapes]
        self.master = [(0.01 * torch.randn(s, generator=g)).to(dev) for s in shapes]
        for p, m in zip(self.params, self.master):
            p.grad = m.clone()
        self.grads = [p.grad for p in self.params]
        # max_grad_norm = a quarter of the gradients' norm: every step clips
        norm = float(torch.sqrt(sum((m.double() ** 2).sum() for m in self.master)))
        self.opt = Adan(self.params, lr=1e-4, weight_decay=1e-6, max_grad_norm=0.25 * norm if clip else 0.0, **kw)
        self.dev_ms, self.host_ms = [], []

    def run(self, steps, record=True):
        pairs = []
        for _ in range(steps):
            torch._foreach_copy_(self.grads, self.master)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            t0 = time.perf_counter()
            self.opt.step()
            t1 = time.perf_counter()
            b.record()
            pairs.append((a, b, (t1 - t0) * 1e3))
        torch.cuda.synchronize()
        if record:
            self.dev_ms += [a.elapsed_time(b) for a, b, _ in pairs]
            self.host_ms += [h for _, _, h in pairs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adan_bench needs a GPU")
    dev = torch.device("cuda:0")
    shapes = [tuple(p.shape) for p in LCRNet(make_cfg()).parameters()]
    elems = sum(int(torch.Size(s).numel()) for s in shapes)
    lines = []
    for clip in (False, True):
        variants = [Variant("fused", shapes, dev, clip, fused=True), Variant("torch_foreach", shapes, dev, clip, fused=False, foreach=True),
                    Variant("torch_single", shapes, dev, clip, fused=False, foreach=False)]
        for v in variants:
            v.run(3, record=False)
        for _ in range(args.rounds):
            for v in variants:
                v.run(args.steps)
        base = statistics.median(variants[1].dev_ms)
        for v in variants:
            ms = statistics.median(v.dev_ms)
            bytes_ = elems * (48 if clip else 44)
            lines.append({"variant": v.name, "clip": clip, "tensors": len(shapes), "elements": elems, "ms_per_step": round(ms, 4),
                          "ms_min": round(min(v.dev_ms), 4), "ms_max": round(max(v.dev_ms), 4), "host_ms_per_step": round(statistics.median(v.host_ms), 4),
                          "timed_steps": len(v.dev_ms), "model_GBps": round(bytes_ / (ms * 1e-3) / 1e9, 1),
                          "share_of_6.3TBps": round(bytes_ / (ms * 1e-3) / HBM_ACHIEVABLE, 3), "share_of_8TBps": round(bytes_ / (ms * 1e-3) / HBM_SPEC, 3),
                          "foreach_over_this": round(base / ms, 2)})
        del variants
        torch.cuda.empty_cache()
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
