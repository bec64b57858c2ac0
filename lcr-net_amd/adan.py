"""The Adan optimiser of the reference's trainers (experiments/lcrnet/adan.py; Xie et al., arXiv 2208.06677) under the reference's
constructor arguments and state layout: state[p] holds exp_avg, exp_avg_sq, exp_avg_diff and pre_grad, group['step'] the step count, so a
state_dict of either class loads into the other.

The step of a group whose parameters, gradients and state are all CUDA, float32 and contiguous is ONE fused pass in HIP (csrc/adan.hip,
lcr_adan_step in include/lcr_hip.h: six floats read and five or six written per element), preceded by one deterministic global-norm
reduction over all groups when max_grad_norm > 0 (lcr_adan_grad_norm).  Neither synchronises with the host: the clip factor stays on the
device.  Every other group takes a plain torch form of the same definition (`foreach` list ops or a per-tensor loop), which is also the
CPU path and the fused path's yardstick in tools/adan_bench.py.

    fused=None   the HIP pass where the tensors allow it, torch elsewhere
    fused=True   the HIP pass, an error where the tensors do not allow it
    fused=False  torch everywhere

Unlike the reference, pre_grad is a buffer the state owns and the step overwrites (the reference clones every gradient every step), and
the clip factor multiplies the gradients only when it is below one (the reference's per-tensor form multiplies by 1.0)."""
import math

import torch
from torch.optim.optimizer import Optimizer

_STATE = ("exp_avg", "exp_avg_sq", "exp_avg_diff", "pre_grad")


def _fusable(t):
    return t.is_cuda and t.dtype == torch.float32 and t.layout == torch.strided and t.is_contiguous()


def _torch_step(ps, gs, ms, ns, ds, pgs, fresh, hyper, clip, foreach):
    """The definition of lcr_adan_step (include/lcr_hip.h) in torch ops, each a rounded fp32 operation; clip = a one-element tensor or
    None.  g * 1 is exact, so the clip factor is applied as min(clip, 1) without reading it on the host."""
    b1, b2, b3 = hyper["beta1"], hyper["beta2"], hyper["beta3"]
    lr, wd = hyper["lr"], hyper["weight_decay"]
    c = None if clip is None else torch.where(clip < 1, clip, torch.ones_like(clip)).reshape(())
    if foreach:
        if c is not None:
            torch._foreach_mul_(gs, c)
        old = [i for i, f in enumerate(fresh) if not f]
        diffs = [None] * len(gs)
        if old:
            for i, x in zip(old, torch._foreach_sub([gs[i] for i in old], [pgs[i] for i in old])):
                diffs[i] = x
        diffs = [torch.zeros_like(g) if x is None else x for x, g in zip(diffs, gs)]
        torch._foreach_copy_(pgs, gs)
        u = torch._foreach_mul(diffs, b2)
        torch._foreach_add_(u, gs)
        torch._foreach_mul_(ms, b1)
        torch._foreach_add_(ms, torch._foreach_mul(gs, 1 - b1))
        torch._foreach_mul_(ds, b2)
        torch._foreach_add_(ds, torch._foreach_mul(diffs, 1 - b2))
        torch._foreach_mul_(ns, b3)
        uu = torch._foreach_mul(u, 1 - b3)
        torch._foreach_mul_(uu, u)
        torch._foreach_add_(ns, uu)
        den = torch._foreach_sqrt(ns)
        torch._foreach_div_(den, hyper["bias3_sqrt"])
        torch._foreach_add_(den, hyper["eps"])
        upd = torch._foreach_div(ms, hyper["bias1"])
        dd = torch._foreach_mul(ds, b2)
        torch._foreach_div_(dd, hyper["bias2"])
        torch._foreach_add_(upd, dd)
        torch._foreach_div_(upd, den)
        torch._foreach_mul_(upd, lr)
        if hyper["no_prox"]:
            torch._foreach_mul_(ps, 1 - lr * wd)
            torch._foreach_sub_(ps, upd)
        else:
            torch._foreach_sub_(ps, upd)
            torch._foreach_div_(ps, 1 + lr * wd)
        return
    for p, g, m, n, d, pg, f in zip(ps, gs, ms, ns, ds, pgs, fresh):
        if c is not None:
            g.mul_(c)
        diff = torch.zeros_like(g) if f else g - pg
        pg.copy_(g)
        u = (diff * b2).add_(g)
        m.mul_(b1).add_(g * (1 - b1))
        d.mul_(b2).add_(diff * (1 - b2))
        n.mul_(b3).add_((u * (1 - b3)).mul_(u))
        den = (n.sqrt() / hyper["bias3_sqrt"]).add_(hyper["eps"])
        upd = (m / hyper["bias1"]).add_((d * b2).div_(hyper["bias2"])).div_(den).mul_(lr)
        if hyper["no_prox"]:
            p.mul_(1 - lr * wd).sub_(upd)
        else:
            p.sub_(upd).div_(1 + lr * wd)


class Adan(Optimizer):
    """Adan(params, lr=1e-3, betas=(0.98, 0.92, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, no_prox=False, foreach=True) as
    in the reference, plus `fused` (module docstring).  `foreach` selects the form of the torch path.  After a step with clipping,
    `grad_norm` is the device tensor of the global gradient norm that step saw."""

    def __init__(self, params, lr=1e-3, betas=(0.98, 0.92, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, no_prox=False,
                 foreach: bool = True, fused=None):
        if not 0.0 <= max_grad_norm:
            raise ValueError("Invalid Max grad norm: {}".format(max_grad_norm))
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        for k in range(3):
            if not 0.0 <= betas[k] < 1.0:
                raise ValueError("Invalid beta parameter at index {}: {}".format(k, betas[k]))
        if fused not in (None, True, False):
            raise ValueError("fused must be None, True or False")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, no_prox=no_prox, foreach=foreach)
        super().__init__(params, defaults)
        self.fused = fused
        self.grad_norm = None
        self._norm_buffers = None

    @classmethod
    def from_cfg(cls, params, cfg, **kw):
        """The optimiser of the reference's loop-detection trainer from the `optimadan` block of config.make_cfg()."""
        o = cfg["optimadan"] if isinstance(cfg, dict) else cfg.optimadan
        get = (lambda k: o[k]) if isinstance(o, dict) else (lambda k: getattr(o, k))
        args = dict(lr=get("lr"), weight_decay=get("weight_decay"), max_grad_norm=get("max_grad_norm"), no_prox=get("no_prox"))
        if get("opt_betas") is not None:
            args["betas"] = tuple(get("opt_betas"))
        if get("opt_eps") is not None:
            args["eps"] = get("opt_eps")
        args.update(kw)
        return cls(params, **args)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("fused", None)
        self.__dict__.setdefault("grad_norm", None)
        self.__dict__.setdefault("_norm_buffers", None)
        for group in self.param_groups:
            group.setdefault("no_prox", False)

    @torch.no_grad()
    def restart_opt(self):
        """Zero the moments and the step count (the next step is a first step: pre_grad is not read)."""
        for group in self.param_groups:
            group["step"] = 0
            for p in group["params"]:
                if p.requires_grad:
                    state = self.state[p]
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                    state["exp_avg_diff"] = torch.zeros_like(p)

    def _gather(self, group):
        """The tensors of one group's step: parameters with a gradient, their state (created on first sight) and the `fresh` flags."""
        ps, fresh = [], []
        for p in group["params"]:
            if p.grad is None:
                continue
            state = self.state[p]
            if len(state) == 0:
                state["exp_avg"] = torch.zeros_like(p)
                state["exp_avg_sq"] = torch.zeros_like(p)
                state["exp_avg_diff"] = torch.zeros_like(p)
            fresh.append(1 if ("pre_grad" not in state or group["step"] == 1) else 0)
            if "pre_grad" not in state:
                state["pre_grad"] = torch.empty_like(state["exp_avg"])
            ps.append(p)
        cols = [[self.state[p][k] for p in ps] for k in _STATE]
        return ps, [p.grad for p in ps], cols[0], cols[1], cols[2], cols[3], fresh

    def _use_fused(self, tensors):
        ok = all(_fusable(t) for ts in tensors for t in ts) and len({t.device for ts in tensors for t in ts}) <= 1
        if self.fused is True and not ok:
            raise RuntimeError("Adan(fused=True): every parameter, gradient and state tensor must be a contiguous float32 CUDA tensor on "
                               "one device")
        return ok and self.fused is not False

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for group in self.param_groups:
            group["step"] = group.get("step", 0) + 1
            ps, gs, ms, ns, ds, pgs, fresh = self._gather(group)
            if ps:
                work.append((group, (ps, gs, ms, ns, ds, pgs), fresh, self._use_fused((ps, gs, ms, ns, ds, pgs))))
        if not work:
            return loss
        F = None
        if any(w[3] for w in work):
            from . import functional as F
        clip = None
        max_norm = self.defaults["max_grad_norm"]
        if max_norm > 0:
            grads = [g for w in work for g in w[1][1]]
            eps = self.param_groups[-1]["eps"]                   # like the reference: the last group's eps
            if all(w[3] for w in work) and len({g.device for g in grads}) == 1:
                dev = grads[0].device
                table = F.adan_table(None, grads, None, None, None, None, None)
                need = F.adan_ws_bytes(table)
                buf = self._norm_buffers
                if buf is None or buf[0].device != dev or buf[0].numel() < need:
                    from . import _lib
                    buf = self._norm_buffers = (_lib.workspace(need, dev), torch.empty(2, dtype=torch.float32, device=dev))
                F.adan_grad_norm(table, max_norm, eps, dev, norm_clip=buf[1], ws=buf[0])
                self.grad_norm, clip = buf[1][0], buf[1][1:2]
            else:
                dev = grads[0].device
                total = torch.zeros((), dtype=torch.float64, device=dev)
                for g in grads:
                    total = total + g.double().pow(2).sum().to(dev)
                norm = total.sqrt().float()
                self.grad_norm, clip = norm, torch.clamp(max_norm / (norm + eps), max=1.0).reshape(1)
        for group, tensors, fresh, fused in work:
            b1, b2, b3 = group["betas"]
            k = group["step"]
            hyper = dict(beta1=b1, beta2=b2, beta3=b3, bias1=1.0 - b1 ** k, bias2=1.0 - b2 ** k, bias3_sqrt=math.sqrt(1.0 - b3 ** k),
                         lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"], no_prox=1 if group["no_prox"] else 0)
            dev = tensors[0][0].device
            c = clip if clip is None or clip.device == dev else clip.to(dev)
            if fused:
                F.adan_step(F.adan_table(*tensors, fresh), F.AdanHyper(**hyper), c, dev)
                for p in tensors[0]:            # the pass wrote the parameters through raw pointers: tell torch, so that caches keyed on the
                    torch.autograd.graph.increment_version(p)      # version counter (functional.WeightStamp: transposed / split weights) are rebuilt
            else:
                _torch_step(*tensors, fresh, hyper, c, group["foreach"])
        return loss
