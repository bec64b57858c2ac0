"""fp64 NumPy restatement of the Adan step and its global-norm clipping, written from the definition in include/lcr_hip.h (lcr_adan_step,
lcr_adan_grad_norm), with planted mistakes that can be switched on, and the seeded case table shared by the golden generator
(tests/golden/make_golden_adan.py), the CPU tests and the GPU tests.

A case is a list of parameter groups over tensors of the golden sizes; step k = 1..K uses gradients (0.3 + 0.2 k) * randn and the
parameters start at 0.5 * randn, all float32 values.  `run` returns, per step, the five quantities of every tensor that has state (p,
exp_avg, exp_avg_sq, exp_avg_diff, pre_grad), the gradients as the step left them (clipped in place) and the norm / clip pair."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adan_golden.npz")
SIZES = (1, 3, 64, 65, 257)
K = 4
QUANTITIES = ("p", "exp_avg", "exp_avg_sq", "exp_avg_diff", "pre_grad")
MISTAKES = ("first_diff", "preclip", "no_b2_update", "bc3_nosqrt", "eps_inside", "no_b2_comb", "prox_swap")
BETAS2 = (0.9, 0.8, 0.95)

# name -> (constructor arguments shared by all groups, groups as (tensor indices, per-group overrides), tensors without a gradient per step)
CASES = {
    "c1": (dict(lr=1e-2), [((0, 1, 2, 3, 4), {})], {}),
    "c2": (dict(lr=5e-2, betas=BETAS2, weight_decay=0.1, no_prox=False), [((0, 1, 2, 3, 4), {})], {}),
    "c3": (dict(lr=5e-2, betas=BETAS2, weight_decay=0.1, no_prox=True, max_grad_norm=2.0), [((0, 1, 2, 3, 4), {})], {}),
    "c4": (dict(lr=5e-2, betas=BETAS2, weight_decay=0.1, max_grad_norm=2.0),
           [((0, 2, 4), {}), ((1, 3), dict(lr=1e-2, weight_decay=0.01, no_prox=True))], {}),
    "c5": (dict(lr=5e-2, betas=BETAS2, weight_decay=0.1, max_grad_norm=2.0), [((0, 1, 2, 3, 4), {})], {1: (3,), 2: (3,)}),
}
DEFAULTS = dict(lr=1e-3, betas=(0.98, 0.92, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, no_prox=False)


def case_inputs(name, sizes=SIZES, steps=K):
    """(p0: list of float32 arrays, grads: per step a list of float32 arrays or None) of a case, from its seed."""
    rng = np.random.RandomState(1000 + sorted(CASES).index(name))
    p0 = [(0.5 * rng.randn(n)).astype(np.float32) for n in sizes]
    missing = CASES[name][2]
    grads = []
    for k in range(1, steps + 1):
        gk = [((0.3 + 0.2 * k) * rng.randn(n)).astype(np.float32) for n in sizes]
        grads.append([None if i in missing.get(k, ()) else g for i, g in enumerate(gk)])
    return p0, grads


def case_groups(name):
    """[(tensor indices, the group's full settings)] and the optimiser-wide max_grad_norm of a case."""
    common, groups, _ = CASES[name]
    full = dict(DEFAULTS, **common)
    return [(idx, dict(full, **over)) for idx, over in groups], full["max_grad_norm"]


def digest(name):
    import hashlib
    h = hashlib.sha256()
    p0, grads = case_inputs(name)
    for a in p0 + [g for gk in grads for g in gk if g is not None]:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], dtype=np.uint64)[0]


def grad_norm(grads, max_grad_norm, eps):
    """(norm, clip) in fp64: clip = min(max_grad_norm / (norm + eps), 1), or 1 when max_grad_norm == 0."""
    total = sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads if g is not None)
    norm = np.sqrt(total)
    return norm, (min(max_grad_norm / (norm + eps), 1.0) if max_grad_norm > 0 else 1.0)


def new_state(p0):
    return {"tensors": [{"p": np.asarray(p, np.float64).copy()} for p in p0], "steps": {}}


def step(state, groups, max_grad_norm, grads, mistake=None):
    """One optimiser step on `state` in place.  grads: a list of arrays or None per tensor.  Returns (gradients after the step, norm, clip)."""
    grads = [None if g is None else np.asarray(g, np.float64).copy() for g in grads]
    norm, clip = grad_norm(grads, max_grad_norm, groups[-1][1]["eps"]) if max_grad_norm > 0 else (None, 1.0)
    for gi, (idx, h) in enumerate(groups):
        k = state["steps"][gi] = state["steps"].get(gi, 0) + 1
        b1, b2, b3 = h["betas"]
        lr, wd, eps = h["lr"], h["weight_decay"], h["eps"]
        bias1, bias2, bias3 = 1.0 - b1 ** k, 1.0 - b2 ** k, 1.0 - b3 ** k
        for i in idx:
            if grads[i] is None:
                continue
            s = state["tensors"][i]
            if "exp_avg" not in s:
                s["exp_avg"], s["exp_avg_sq"], s["exp_avg_diff"] = (np.zeros_like(s["p"]) for _ in range(3))
            g = grads[i]
            gc = g * clip if clip < 1 else g
            fresh = "pre_grad" not in s or k == 1
            if fresh:
                diff = gc.copy() if mistake == "first_diff" else np.zeros_like(gc)
            else:
                diff = gc - s["pre_grad"]
            s["pre_grad"] = (g if mistake == "preclip" else gc).copy()
            grads[i] = gc
            u = gc + (1.0 if mistake == "no_b2_update" else b2) * diff
            s["exp_avg"] = s["exp_avg"] * b1 + (1 - b1) * gc
            s["exp_avg_diff"] = s["exp_avg_diff"] * b2 + (1 - b2) * diff
            s["exp_avg_sq"] = s["exp_avg_sq"] * b3 + (1 - b3) * u * u
            if mistake == "bc3_nosqrt":
                den = np.sqrt(s["exp_avg_sq"]) / bias3 + eps
            elif mistake == "eps_inside":
                den = np.sqrt(s["exp_avg_sq"] / bias3 + eps)
            else:
                den = np.sqrt(s["exp_avg_sq"]) / np.sqrt(bias3) + eps
            upd = (s["exp_avg"] / bias1 + (1.0 if mistake == "no_b2_comb" else b2) * s["exp_avg_diff"] / bias2) / den
            if bool(h["no_prox"]) != (mistake == "prox_swap"):
                s["p"] = s["p"] * (1 - lr * wd) - lr * upd
            else:
                s["p"] = (s["p"] - lr * upd) / (1 + lr * wd)
    return grads, norm, clip


def snapshot(state):
    """{quantity: [array or None per tensor]} of the current state (None: the tensor has had no gradient, hence no state, yet)."""
    return {q: [s[q].copy() if "exp_avg" in s else None for s in state["tensors"]] for q in QUANTITIES}


def run_groups(groups, max_norm, p0, grads, mistake=None):
    """Any groups [(tensor indices, settings)] over any tensors: a list, per step, of snapshot() plus 'grad' (the gradients as the step
    left them), 'norm' and 'clip'."""
    state, out = new_state(p0), []
    for gk in grads:
        after, norm, clip = step(state, groups, max_norm, gk, mistake)
        snap = snapshot(state)
        snap.update(grad=after, norm=norm, clip=clip)
        out.append(snap)
    return out


def run(name, mistake=None):
    """A case of the table through its K steps (run_groups)."""
    groups, max_norm = case_groups(name)
    return run_groups(groups, max_norm, *case_inputs(name), mistake=mistake)


def family_inputs(sizes, steps, seed):
    """Parameters and gradients drawn like a case's (0.5 * randn, (0.3 + 0.2 k) * randn) for any list of sizes."""
    rng = np.random.RandomState(seed)
    p0 = [(0.5 * rng.randn(n)).astype(np.float32) for n in sizes]
    return p0, [[((0.3 + 0.2 * k) * rng.randn(n)).astype(np.float32) for n in sizes] for k in range(1, steps + 1)]


def _offsets():
    return np.concatenate([[0], np.cumsum(SIZES)])


def pack(per_step):
    """Golden layout of one quantity of one case: float32 [K, sum(SIZES)], tensor after tensor, NaN where a tensor has no state yet."""
    out = np.full((len(per_step), int(sum(SIZES))), np.nan, dtype=np.float32)
    off = _offsets()
    for k, tensors in enumerate(per_step):
        for i, a in enumerate(tensors):
            if a is not None:
                out[k, off[i]:off[i + 1]] = a
    return out


class Golden:
    """tests/golden/adan_golden.npz.  The reference's per-tensor form is stored as float32, its foreach form as the int32 difference of
    the bit patterns (a few units in the last place, so it compresses to nothing); get() undoes that."""

    def __init__(self, path=GOLDEN):
        self.z = np.load(path, allow_pickle=False)
        self._cache = {}

    def plane(self, name, form, q):
        kk = (name, form, q)
        if kk not in self._cache:
            a = self.z["%s_single_%s" % (name, q)]
            if form == "foreach":
                a = (a.view(np.int32) + self.z["%s_foreach_%s_ulps" % (name, q)]).view(np.float32)
            self._cache[kk] = a
        return self._cache[kk]

    def get(self, name, form, k, q, i):
        """Quantity q of tensor i after step k (1-based) of a case run with form 'foreach' or 'single'; None where the reference has none."""
        off = _offsets()
        a = self.plane(name, form, q)[k - 1, off[i]:off[i + 1]]
        return None if np.isnan(a).all() else a


def bound(e_ref, want):
    """The tolerance rule: 4 x the error of the reference's own fp32 module against this restatement, with a floor of 2^-20 relative to the
    largest magnitude in the tensor."""
    w = np.asarray(want, dtype=np.float64)
    big = np.abs(w).max() if w.size else 0.0
    return max(4.0 * float(e_ref), 2.0 ** -20 * big)


def err(got, want):
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    return float(np.abs(g - w).max()) if w.size else 0.0


def e_ref_table(gold):
    """{(case, quantity): e_ref}: the largest absolute error of the reference's fp32 module, in either form, at any step and in any tensor
    of the case, against the restatement.  Inputs drawn like a case's (same scales, same settings) inherit its figures."""
    tab = {}
    for name in sorted(CASES):
        r = run(name)
        for q in QUANTITIES:
            worst = 0.0
            for form in ("foreach", "single"):
                for k in range(1, K + 1):
                    for i, want in enumerate(r[k - 1][q]):
                        have = gold.get(name, form, k, q, i)
                        if want is None:
                            assert have is None, (name, form, k, q, i)
                            continue
                        worst = max(worst, err(have, want))
            tab[(name, q)] = worst
    return tab
