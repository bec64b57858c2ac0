"""fp64 restatements of the FORWARD of the 3D-RoFormer (csrc/attention.hip: k_rotary, k_attention, k_attention_seg, k_add_layernorm,
k_relu_inplace; sequenced by csrc/roformer.hip and modules/thdroformer), written from the formulas, with planted mistakes, and the seeded
named cases both test files run.  Shared by test_roformer_cpu.py and test_roformer_gpu.py.

The clean attention and rotary forwards are attention_grad_restatement's (`out` of attention_restate, `y` of rotary_restate); only their
mistaken variants, LayerNorm(a + b), one transformer layer and the whole transformer are written here.

Layouts are the library's: q [Nq, heads*32], k / v [Nk, heads*32], theta [N, heads*16] (one angle per adjacent channel pair), stacked problems
given by q_lens / k_lens; a state dict with the module tree's keys (pfx "" = ThDRoFormer.state_dict())."""
import math

import torch

from attention_grad_restatement import HEAD_DIM, _problems, attention_formula, attention_restate, bound, rotary_formula, rotary_restate  # noqa: F401

ATTENTION_MISTAKES = ("tail_unmasked", "merge_no_rescale", "scale_d_model", "neighbour_keys")
ROTARY_MISTAKES = ("sin_sign", "half_split")
LAYERNORM_MISTAKES = ("eps_outside_root", "unbiased_var", "b_dropped")
TRANSFORMER_MISTAKES = ("cross_uses_stale_cloud0",)
SPLIT = 4                                   # wavefronts of a workgroup: 32-key block j // 32 belongs to wavefront (j // 32) % 4


def owner(key):
    """the wavefront of attention_tile that walks the 32-key block of `key`"""
    return (key // 32) % SPLIT


# ---- attention ------------------------------------------------------------------------------------------------------------------------------
def attention_forward(q, k, v, heads, q_lens=None, k_lens=None, mistake=None):
    """softmax(Q K^T / sqrt(32)) V per problem and head in fp64.
    tail_unmasked: the last 32-key block is padded with copies of the last key and value row, and they are soft-maxed with the rest;
    merge_no_rescale: the 32-key blocks are dealt round-robin to four (max, sum, O) states that are added without e^{m_w - m};
    scale_d_model: 1 / sqrt(128); neighbour_keys: problem p > 0 attends the keys and values of problem p - 1."""
    if mistake is None:
        return attention_restate(q, k, v, torch.zeros_like(q), heads, q_lens, k_lens)[0]
    assert mistake in ATTENTION_MISTAKES, mistake
    q, k, v = q.double(), k.double(), v.double()
    scale = 1.0 / math.sqrt(4 * HEAD_DIM if mistake == "scale_d_model" else HEAD_DIM)
    out = torch.zeros_like(q)
    probs = _problems(q.shape[0], k.shape[0], q_lens, k_lens)
    for p, (qs, ks) in enumerate(probs):
        if mistake == "neighbour_keys" and p > 0:
            ks = probs[p - 1][1]
        for h in range(heads):
            c = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            Q, K, V = q[qs, c], k[ks, c], v[ks, c]
            if mistake == "tail_unmasked":
                pad = -K.shape[0] % 32
                K, V = torch.cat([K, K[-1:].expand(pad, -1)]), torch.cat([V, V[-1:].expand(pad, -1)])
            S = scale * Q @ K.T
            if mistake == "merge_no_rescale":
                num, den = torch.zeros_like(Q), torch.zeros(Q.shape[0], 1, dtype=torch.float64)
                for w in range(SPLIT):
                    cols = [j for j in range(K.shape[0]) if owner(j) == w]
                    if cols:
                        E = torch.exp(S[:, cols] - S[:, cols].max(1, keepdim=True)[0])
                        num, den = num + E @ V[cols], den + E.sum(1, keepdim=True)
                out[qs, c] = num / den
            else:
                E = torch.exp(S - S.max(1, keepdim=True)[0])
                out[qs, c] = (E / E.sum(1, keepdim=True)) @ V
    return out


def scores(q, k, heads):
    """[heads, Nq, Nk] fp64 scores of ONE problem, in the units the soft-max sees"""
    q, k = q.double(), k.double()
    return torch.stack([q[:, h * HEAD_DIM:(h + 1) * HEAD_DIM] @ k[:, h * HEAD_DIM:(h + 1) * HEAD_DIM].T for h in range(heads)]) / math.sqrt(HEAD_DIM)


# ---- rotary ---------------------------------------------------------------------------------------------------------------------------------
def rotary_forward(x, theta, mistake=None):
    """y = R(theta) x per adjacent channel pair in fp64.  sin_sign: R(-theta); half_split: channel i of a head is paired with i + 16."""
    if mistake is None:
        return rotary_restate(x, theta, torch.zeros_like(x))[0]
    assert mistake in ROTARY_MISTAKES, mistake
    if mistake == "sin_sign":
        return rotary_restate(x, -theta.double(), torch.zeros_like(x))[0]
    x, theta = x.double(), theta.double()
    n = x.shape[0]
    xh, th = x.reshape(n, -1, 2, HEAD_DIM // 2), theta.reshape(n, -1, HEAD_DIM // 2)
    c, s = torch.cos(th), torch.sin(th)
    return torch.stack([xh[:, :, 0] * c - xh[:, :, 1] * s, xh[:, :, 1] * c + xh[:, :, 0] * s], 2).reshape(n, -1)


# ---- LayerNorm(a + b) -----------------------------------------------------------------------------------------------------------------------
def add_layernorm_forward(a, b, gamma, beta, eps=1e-5, mistake=None):
    """y = (x - mean) / sqrt(var + eps) gamma + beta over the features of x = a + b (b optional), var the biased variance, in fp64"""
    assert mistake is None or mistake in LAYERNORM_MISTAKES, mistake
    x = a.double()
    if b is not None and mistake != "b_dropped":
        x = x + b.double()
    d = x.shape[1]
    mean = x.sum(1, keepdim=True) / d
    var = ((x - mean) ** 2).sum(1, keepdim=True) / (max(d - 1, 1) if mistake == "unbiased_var" else d)
    den = torch.sqrt(var) + eps if mistake == "eps_outside_root" else torch.sqrt(var + eps)
    return (x - mean) / den * gamma.double() + beta.double()


def add_layernorm_formula(a, b, gamma, beta, eps=1e-5):
    """the reference's op in the dtype of its arguments"""
    x = a if b is None else a + b
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


# ---- one layer and the whole transformer ----------------------------------------------------------------------------------------------------
def _lin(sd, pfx, x):
    return x @ sd[pfx + "weight"].double().T + sd[pfx + "bias"].double()


def layer_forward(sd, pfx, x, mem, heads, theta=None, x_lens=None, m_lens=None):
    """_TransformerLayer in fp64: q / k / v Linears, rotary on q and k by the SAME theta (self layers: mem is x), attention per problem,
    Linear, LayerNorm(h + x), expand with ReLU, squeeze, LayerNorm(y + z)"""
    x, mem = x.double(), mem.double()
    a = pfx + "attention.attention."
    q, k, v = _lin(sd, a + "proj_q.", x), _lin(sd, a + "proj_k.", mem), _lin(sd, a + "proj_v.", mem)
    if theta is not None:
        q, k = rotary_forward(q, theta), rotary_forward(k, theta)
    h = _lin(sd, pfx + "attention.linear.", attention_forward(q, k, v, heads, x_lens, m_lens))
    y = add_layernorm_forward(h, x, sd[pfx + "attention.norm.weight"], sd[pfx + "attention.norm.bias"])
    z = _lin(sd, pfx + "output.squeeze.", torch.clamp(_lin(sd, pfx + "output.expand.", y), min=0.0))
    return add_layernorm_forward(y, z, sd[pfx + "output.norm.weight"], sd[pfx + "output.norm.bias"])


def roformer_forward(sd, pts0, pts1, feats0, feats1, heads, num_layers, lens0=None, lens1=None, pfx="", mistake=None):
    """ThDRoFormer over stacked pairs in fp64 -> (out0, out1, theta0, theta1): pair p is rows lens0[p] of the first stack and lens1[p] of
    the second; [self, cross] x num_layers, and in a cross layer cloud 1 attends the UPDATED cloud 0 (cross_uses_stale_cloud0: the old one)"""
    assert mistake is None or mistake in TRANSFORMER_MISTAKES, mistake
    emb = lambda p: _lin(sd, pfx + "embedding.encoder2.", _lin(sd, pfx + "embedding.encoder.", p.double()))
    t0, t1 = emb(pts0), emb(pts1)
    f0, f1 = _lin(sd, pfx + "in_proj.", feats0.double()), _lin(sd, pfx + "in_proj.", feats1.double())
    for i in range(2 * num_layers):
        L = "%stransformer.layers.%d." % (pfx, i)
        if i % 2 == 0:
            f0, f1 = layer_forward(sd, L, f0, f0, heads, t0, lens0, lens0), layer_forward(sd, L, f1, f1, heads, t1, lens1, lens1)
        else:
            new0 = layer_forward(sd, L, f0, f1, heads, None, lens0, lens1)
            f1 = layer_forward(sd, L, f1, f0 if mistake == "cross_uses_stale_cloud0" else new0, heads, None, lens1, lens0)
            f0 = new0
    return _lin(sd, pfx + "out_proj.", f0), _lin(sd, pfx + "out_proj.", f1), t0, t1


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
KEY_COUNTS = (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 255, 256, 257)       # with 33 queries
QUERY_COUNTS = (1, 31, 32, 65)                                                                   # with 97 keys
GRID = [(33, nk) for nk in KEY_COUNTS] + [(nq, 97) for nq in QUERY_COUNTS]
REGIMES = ("unit", "peaked", "late_max", "early_max", "two_peaks", "shifted")
PEAK_C = {"late_max": 24.0, "early_max": 24.0, "two_peaks": 10.0}


def peak_keys(regime, nk):
    """the keys that carry the planted maxima.  two_peaks: key nk - 1 and key 0, or key 32 where nk - 1 sits in a block of wavefront 0
    (nk <= 32 has one block: both peaks are wavefront 0's)"""
    if regime == "late_max":
        return [nk - 1]
    if regime == "early_max":
        return [0]
    if regime == "two_peaks":
        return [32 if (nk > 32 and owner(nk - 1) == 0) else 0, nk - 1]
    return []


def attention_problem(regime, nq, nk, heads, seed):
    """-> (q, k, v) of one problem, fp32.  unit: standard normal.  peaked: q x 8.  late_max / early_max / two_peaks: per head the queries are
    a +-1 vector u plus 0.1 noise and the peak keys are c u plus (0.2 x) noise, so a peak scores c 32 / sqrt(32) against O(1) for the rest.
    shifted: q = u + 0.5 noise, k = noise +- 35 u (the sign alternates with the head): every score of a row carries the same shift of about
    +-200 and the spread within the row stays of order one."""
    assert regime in REGIMES, regime
    g = torch.Generator().manual_seed(seed)
    w = heads * HEAD_DIM
    q, k, v = torch.randn(nq, w, generator=g), torch.randn(nk, w, generator=g), torch.randn(nk, w, generator=g)
    u = (torch.randint(0, 2, (w,), generator=g) * 2 - 1).float()
    if regime == "peaked":
        q = q * 8.0
    elif regime in PEAK_C:
        q = u + 0.1 * q
        for j in peak_keys(regime, nk):
            k[j] = PEAK_C[regime] * u + 0.2 * k[j]
    elif regime == "shifted":
        sign = torch.tensor([1.0 if h % 2 == 0 else -1.0 for h in range(heads)]).repeat_interleave(HEAD_DIM)
        q = u + 0.5 * q
        k = k + 35.0 * sign * u
    return q, k, v


def attention_stack(regime, heads, problems=GRID, seed=0):
    """-> (q, k, v, q_lens, k_lens): the problems stacked in order, each drawn with its own seed"""
    parts = [attention_problem(regime, nq, nk, heads, 7919 * (seed + 1) + 131 * p + REGIMES.index(regime)) for p, (nq, nk) in enumerate(problems)]
    q, k, v = (torch.cat([t[i] for t in parts]) for i in range(3))
    return q, k, v, [nq for nq, _ in problems], [nk for _, nk in problems]


def attention_reference(q, k, v, heads, q_lens, k_lens):
    """-> (fp64 result, e_ref, tolerance, [(query rows, e_ref of these rows) per problem]): the suite's rule for the output tensor of one launch,
    e_ref being the error of fp32 torch through the reference's formula on the same inputs and the scale the largest |fp64| entry.  The
    per-problem e_ref is for the printed tables only: over the 128 entries of a one-row problem it is one draw of the fp32 error, not its
    size (the 1 x 97 problem of the peaked stack drew 1.0e-6 where the other twenty-one lie between 3.0e-6 and 7.6e-6)."""
    want = attention_forward(q, k, v, heads, q_lens, k_lens)
    w32 = attention_formula(q.float(), k.float(), v.float(), heads, q_lens, k_lens).double()
    rows = [(qs, (w32[qs] - want[qs]).abs().max().item() if qs.stop > qs.start else 0.0) for qs, _ in _problems(q.shape[0], k.shape[0], q_lens, k_lens)]
    e_ref = (w32 - want).abs().max().item()
    return want, e_ref, bound(e_ref, want.abs().max().item()), rows


ROTARY_SCALES = (1.0, 100.0, 1e4)


def rotary_case(n, heads, theta_scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, heads * HEAD_DIM, generator=g), torch.randn(n, heads * HEAD_DIM // 2, generator=g) * theta_scale


ROW_KINDS = ("ordinary", "constant", "tiny_spread", "large_mean")


def layernorm_case(kind, n, d, with_b, seed):
    """-> (a, b, gamma, beta).  ordinary: standard normal.  constant: every entry of a row of a (and of b) is the row's own constant.
    tiny_spread: a constant plus 1e-3 noise (variance 1e-6 < eps).  large_mean: 1e3 plus unit noise."""
    assert kind in ROW_KINDS, kind
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    row = torch.randn(n, 1, generator=g)
    if kind == "constant":
        a, b = row.expand(n, d).contiguous(), (0.37 * row + 0.1).expand(n, d).contiguous()
    elif kind == "tiny_spread":
        a, b = row + 1e-3 * a, 0.5e-3 * b
    elif kind == "large_mean":
        a, b = 1e3 + a, 0.5 * b
    gamma, beta = 1.0 + 0.3 * torch.randn(d, generator=g), torch.randn(d, generator=g)
    return a, (b if with_b else None), gamma, beta


def composite_inputs(lens0, lens1, in_dim, seed):
    """points uniform in a +-50 m box (the range real scans put through the position Linears), features 0.5 x standard normal"""
    g = torch.Generator().manual_seed(seed)
    n0, n1 = sum(lens0), sum(lens1)
    p0, p1 = torch.rand(n0, 3, generator=g) * 100.0 - 50.0, torch.rand(n1, 3, generator=g) * 100.0 - 50.0
    return p0, p1, torch.randn(n0, in_dim, generator=g) * 0.5, torch.randn(n1, in_dim, generator=g) * 0.5
