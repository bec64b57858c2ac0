#!/usr/bin/env python
"""The reverse pass of the transport (lcr_log_sinkhorn_grad, csrc/sinkhorn_grad.hip) against the forward at the same shape and against
torch autograd through the dense device form of the transport, on the same card.

    python tools/sinkhorn_grad_bench.py [--steps 10] [--warmup 2] [--out FILE]

Shapes: the patch level, B = 256 and B = 3600 problems of 129 x 129 (128 points + dustbin); the node level, B = 16 of 351 x 331.  T = 100.
Random scores (normal, scale 1 / sqrt(channels) folded in), a tenth of the lines masked, random G zeroed on masked lines.

Per shape, device-synchronised wall clock around whole calls, the median of --steps calls after --warmup:
  backward_ms   lcr_log_sinkhorn_grad alone (it recomputes the duals itself)
  forward_ms    lcr_log_sinkhorn_ex on a copy of the padded scores (the copy is made outside the clock)
  torch_ms      forward + backward of the dense torch transport minus its forward, i.e. what autograd's backward costs — at B = 256 and the
                node shape only: at B = 3600 autograd keeps 200 tensors of 3600 x 129 x 129 floats (48 GB) and is not tried.
Every shape runs in a child process of its own under a time limit.  One JSON line per shape."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"patch256": (256, 128, 128, True), "patch3600": (3600, 128, 128, False), "node16": (16, 350, 330, True)}
ITERS = 100
STEP_TIMEOUT = 300


def timed(fn, steps, warmup, before=None):
    import torch
    ts = []
    for k in range(warmup + steps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def run_case(name, steps, warmup):
    import torch
    import sinkhorn_grad_restatement as R
    from lcrnet_amd import _lib
    from lcrnet_amd import functional as F
    B, M, N, with_torch = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    raw = torch.randn(B, M, N, generator=g).to(dev)
    rm, cm = (torch.rand(B, M, generator=g) > 0.1).to(dev), (torch.rand(B, N, generator=g) > 0.1).to(dev)
    rm[:, 0] = cm[:, 0] = True
    V = torch.ones(B, M + 1, N + 1, dtype=torch.bool, device=dev)
    V[:, :M, :] &= rm[:, :, None]
    V[:, :, :N] &= cm[:, None, :]
    G = torch.randn(B, M + 1, N + 1, generator=g).to(dev) * V
    alpha = torch.tensor(0.7, device=dev)
    rm8, cm8 = rm.to(torch.uint8), cm.to(torch.uint8)
    S0 = torch.empty((B, M + 1, N + 1), dtype=torch.float32, device=dev)
    _lib.call.lcr_build_padded_scores(_lib.ptr(raw), _lib.ptr(rm8), _lib.ptr(cm8), B, M, N, 1.0, _lib.ptr(alpha.reshape(1)), 1e12, _lib.ptr(S0),
                                      _lib.stream_ptr(dev))
    res = {"bench": "sinkhorn_grad_bench", "shape": name, "B": B, "M": M, "N": N, "iters": ITERS, "device": torch.cuda.get_device_name(0),
           "steps": steps, "warmup": warmup}
    res["backward_ms"] = timed(lambda: F.log_sinkhorn_grad(S0, G, rm8, cm8, ITERS), steps, warmup)
    work = [None]

    def fresh():
        work[0] = S0.clone()

    res["forward_ms"] = timed(lambda: F._transport_padded(work[0], rm8, cm8, ITERS, 1e12), steps, warmup, before=fresh)
    F.check_transport_status()
    res["backward_over_forward"] = res["backward_ms"] / res["forward_ms"]
    if with_torch:
        r, a = raw.clone().requires_grad_(), alpha.clone().requires_grad_()

        def fwd():
            with torch.no_grad():
                R.dense_transport(r, rm, cm, a, ITERS)

        def fwd_bwd():
            r.grad = a.grad = None
            (R.dense_transport(r, rm, cm, a, ITERS) * G).sum().backward()

        t_f, t_fb = timed(fwd, steps, warmup), timed(fwd_bwd, steps, warmup)
        res["torch_forward_ms"], res["torch_forward_backward_ms"], res["torch_ms"] = t_f, t_fb, t_fb - t_f
        res["torch_over_backward"] = res["torch_ms"] / res["backward_ms"]
        dS, part = F.log_sinkhorn_grad(S0, G, rm8, cm8, ITERS)
        res["max_difference_from_torch_over_max_gradient"] = ((dS[:, :M, :N] - r.grad).abs().max() / r.grad.abs().max()).item()
    else:
        res["torch_ms"] = None
        res["torch_note"] = "not run: autograd would keep 200 tensors of %d x %d x %d floats (%.0f GB)" % (
            B, M + 1, N + 1, 200 * B * (M + 1) * (N + 1) * 4 / 1e9)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--case", default=None, help="(internal) run this one shape in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.case:
        print(json.dumps(run_case(a.case, a.steps, a.warmup)))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sinkhorn_grad_bench needs a GPU: a timing without one says nothing")
    lines = []
    for name in a.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--steps", str(a.steps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit("sinkhorn_grad_bench: shape %s ended with status %d" % (name, p.returncode))
        lines.append(p.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
