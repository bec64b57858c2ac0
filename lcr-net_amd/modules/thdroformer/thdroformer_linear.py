"""ThDRoFormer (3D-RoFormer) — module tree / parameter names of experiments/lcrnet/modules/thdroformer
(thdroformer_linear.py:12-97, rpetransformer.py:57-220, vanilla_transformer.py:13-144, Rotary3DPosEmb.py:27-38) so the
`transformer.*` checkpoint keys load unchanged; forward on the HIP kernels (lcr_gemm_f32 for every Linear,
lcr_rotary_embed, the fused MFMA attention lcr_attention_f32, lcr_add_layernorm).  One pair per call like the reference, or P
pairs per call (`lens0` / `lens1`): the rows of all first clouds are stacked in one tensor, those of all second clouds in another,
every Linear / LayerNorm runs once over the stack and the attention kernel takes the P problems in one launch
(lcr_attention_seg_f32) — per-pair results are those of P separate calls.

Differentiable: with grad mode on and an input or a parameter requiring grad, ThDRoFormer.forward takes the module tree, whose ops
(functional.linear / rotary_embed / attention / add_layernorm) return a graph with HIP backwards (csrc/attention_grad.hip); under no_grad it
makes the calls it always made.  The forward bytes do not depend on the mode.  Dense attention only: the top-k form (cfg.GAT.k) raises
NotImplementedError when a gradient is wanted."""
import torch.nn as nn

from ... import functional as F


class LinearLearnablePosEmbedding(nn.Module):
    def __init__(self, hidden_dim, reduction_a="max"):
        super().__init__()
        self.encoder = nn.Linear(3, int(hidden_dim))
        self.encoder2 = nn.Linear(int(hidden_dim), int(hidden_dim / 2))

    def forward(self, points):
        """points (N,3) -> theta (N, hidden/2); two Linears, no activation (Rotary3DPosEmb.py:34-38)."""
        return F.linear(F.linear(points, self.encoder.weight, self.encoder.bias), self.encoder2.weight, self.encoder2.bias)


class _MultiHeadAttention(nn.Module):
    """Parameters of RPEMultiHeadAttention / MultiHeadAttention (identical names; the rotary variant has no extra parameters)."""

    def __init__(self, d_model, num_heads):
        super().__init__()
        assert d_model % num_heads == 0 and d_model // num_heads == 32, "the fused attention kernel is built for head_dim 32"
        self.d_model, self.num_heads = d_model, num_heads
        self.proj_q = nn.Linear(d_model, d_model)
        self.proj_k = nn.Linear(d_model, d_model)
        self.proj_v = nn.Linear(d_model, d_model)

    def forward(self, input_q, input_k, input_v, theta_q=None, q_lens=None, k_lens=None, topk_frac=None):
        q = F.linear(input_q, self.proj_q.weight, self.proj_q.bias)
        k = F.linear(input_k, self.proj_k.weight, self.proj_k.bias)
        v = F.linear(input_v, self.proj_v.weight, self.proj_v.bias)
        if theta_q is not None:                                   # self layers: the SAME theta rotates q and k
            if F._wants_grad(q, k, theta_q):                      # training: out of place, autograd sums the two dtheta contributions
                q = F.rotary_embed(q, theta_q, self.num_heads)
                k = F.rotary_embed(k, theta_q, self.num_heads)
            else:
                F.rotary_embed_(q, theta_q, self.num_heads)
                F.rotary_embed_(k, theta_q, self.num_heads)
        if topk_frac is not None:                                 # dynamic_attention(q, k, v, self.k[layer]): k = int(n * k), n = the cloud's queries
            ql = list(q_lens) if q_lens is not None else [q.shape[0]]
            kl = list(k_lens) if k_lens is not None else [k.shape[0]]
            kks = [int(n * topk_frac) for n in ql]
            for n_k, kk in zip(kl, kks):
                if kk > n_k:                                      # torch.topk raises here too (rpetransformer.py:27-28); the kernel would clamp
                    raise RuntimeError("top-k attention: k = %d exceeds the %d keys of the cloud (selected index k out of range)" % (kk, n_k))
                if n_k > F.ATTENTION_TOPK_MAX_KEYS:               # before anything is launched (advisor r5): the scores of a row live in LDS
                    raise RuntimeError("top-k attention (cfg.GAT.k) supports at most %d keys per cloud, got %d; the dense form (k = None) has "
                                       "no such limit" % (F.ATTENTION_TOPK_MAX_KEYS, n_k))
            return F.attention_topk(q, k, v, self.num_heads, ql, kl, kks)
        return F.attention(q, k, v, self.num_heads, q_lens, k_lens)


class _AttentionLayer(nn.Module):
    def __init__(self, d_model, num_heads):
        super().__init__()
        self.attention = _MultiHeadAttention(d_model, num_heads)
        self.linear = nn.Linear(d_model, d_model)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, x, memory, theta=None, x_lens=None, m_lens=None, topk_frac=None):
        h = self.attention(x, memory, memory, theta, x_lens, m_lens, topk_frac)
        h = F.linear(h, self.linear.weight, self.linear.bias)
        return F.add_layernorm(h, x, self.norm.weight, self.norm.bias, self.norm.eps)


class _AttentionOutput(nn.Module):
    def __init__(self, d_model):
        super().__init__()
        self.expand = nn.Linear(d_model, d_model * 2)
        self.squeeze = nn.Linear(d_model * 2, d_model)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, x):
        h = F.linear(x, self.expand.weight, self.expand.bias, relu=True)
        h = F.linear(h, self.squeeze.weight, self.squeeze.bias)
        return F.add_layernorm(x, h, self.norm.weight, self.norm.bias, self.norm.eps)


class _TransformerLayer(nn.Module):
    def __init__(self, d_model, num_heads):
        super().__init__()
        self.attention = _AttentionLayer(d_model, num_heads)
        self.output = _AttentionOutput(d_model)

    def forward(self, x, memory, theta=None, x_lens=None, m_lens=None, topk_frac=None):
        return self.output(self.attention(x, memory, theta, x_lens, m_lens, topk_frac))


class RPEConditionalTransformer(nn.Module):
    def __init__(self, blocks, d_model, num_heads, parallel=False, k=None):
        super().__init__()
        self.blocks, self.parallel = list(blocks), parallel
        self.k = None if k is None else [float(x) for x in k]      # top-k fraction per SELF layer (rpetransformer.py:101-102: self.k[layer])
        if self.k is not None and len(self.k) < sum(b == "self" for b in self.blocks):
            raise ValueError("k needs one fraction per self layer")
        self.layers = nn.ModuleList([_TransformerLayer(d_model, num_heads) for _ in self.blocks])

    def forward(self, feats0, feats1, theta0, theta1, lens0=None, lens1=None):
        import torch
        n0 = feats0.shape[0]
        # self layers: ONE pass over the rows of both clouds — the module is shared (rpetransformer.py:203-206), every Linear / LayerNorm is
        # row-wise and the attention kernel takes segments, so the stacked pass gives each row exactly what two passes give it (bit for bit)
        # at half the launches (these kernels sit on their launch floors: 11 fewer per self layer)
        theta_cat = torch.cat([theta0, theta1])
        lens_cat = (list(lens0) + list(lens1)) if lens0 is not None else [n0, feats1.shape[0]]
        self_idx = 0
        for i, block in enumerate(self.blocks):
            if block == "self":
                x = torch.cat([feats0, feats1])
                x = self.layers[i](x, x, theta_cat, lens_cat, lens_cat, None if self.k is None else self.k[self_idx])
                self_idx += 1
                feats0, feats1 = x[:n0], x[n0:]
            elif self.parallel:
                feats0, feats1 = self.layers[i](feats0, feats1, None, lens0, lens1), self.layers[i](feats1, feats0, None, lens1, lens0)
            else:                                                 # sequential: cloud 1 attends to the UPDATED cloud 0 (:213-214)
                feats0 = self.layers[i](feats0, feats1, None, lens0, lens1)
                feats1 = self.layers[i](feats1, feats0, None, lens1, lens0)
        return feats0, feats1


class ThDRoFormer(nn.Module):
    def __init__(self, input_dim, output_dim, hidden_dim, num_heads, num_layers, k=None, dropout=None, activation_fn="ReLU", reduction_a="max"):
        super().__init__()
        assert dropout is None and activation_fn == "ReLU", "reference configuration: no dropout, ReLU"
        self.embedding = LinearLearnablePosEmbedding(hidden_dim, reduction_a=reduction_a)
        self.in_proj = nn.Linear(input_dim, hidden_dim)
        self.transformer = RPEConditionalTransformer(["self", "cross"] * num_layers, hidden_dim, num_heads, k=k)
        self.out_proj = nn.Linear(hidden_dim, output_dim)
        # forward through lcr_roformer_forward (one native call, csrc/roformer.hip) when the configuration allows it (dense attention);
        # LCR_NATIVE_ROFORMER=0: the module tree below (bit-identical)
        import os
        self.native = os.environ.get("LCR_NATIVE_ROFORMER", "1") != "0"

    def _apply(self, fn, *args, **kwargs):
        self.__dict__.pop("_native_table", None)        # raw device pointers: every .to() / .cuda() replaces the tensors
        return super()._apply(fn, *args, **kwargs)

    def __getstate__(self):
        d = dict(self.__dict__)
        d.pop("_native_table", None)
        return d

    def forward(self, ref_points, src_points, ref_feats, src_feats, ref_lens=None, src_lens=None, return_pos_emb=False):
        """(N,3), (M,3), (N,C), (M,C)  [a leading batch dim of 1 as in the reference is accepted] -> (N,out), (M,out).
        ref_lens / src_lens (host sequences, one entry per pair): the inputs are the stacks of P pairs' first / second clouds.
        return_pos_emb: also return the rotary angles theta of both clouds (thdroformer_linear.py:94-95).
        Inference belongs under torch.no_grad(): parameters require grad by default, so a call with grad mode on is taken for training — it
        runs the module tree instead of the native one-call path, keeps the tensors its ~50 autograd nodes save, and returns outputs that
        require grad (the same bytes)."""
        squeeze = ref_points.dim() == 3
        if squeeze:
            ref_points, src_points, ref_feats, src_feats = ref_points[0], src_points[0], ref_feats[0], src_feats[0]
        import torch
        n0 = ref_points.shape[0]
        from ... import native_roformer
        # training (grad mode on and an input or a parameter of this module requires grad): the module tree, whose ops carry a graph; its
        # forward bytes are the native call's
        wants_grad = torch.is_grad_enabled() and (any(t.requires_grad for t in (ref_points, src_points, ref_feats, src_feats))
                                                  or any(p.requires_grad for p in self.parameters()))
        if self.native and not wants_grad and native_roformer.eligible(self, ref_feats):
            lens0 = list(ref_lens) if ref_lens is not None else [n0]
            lens1 = list(src_lens) if src_lens is not None else [src_points.shape[0]]
            f, t = native_roformer.forward(self, torch.cat([ref_points, src_points]), torch.cat([ref_feats, src_feats]), lens0, lens1)
            f0, f1, t0, t1 = f[:n0], f[n0:], t[:n0], t[n0:]
            if return_pos_emb:
                return (f0[None], f1[None], t0[None], t1[None]) if squeeze else (f0, f1, t0, t1)
            return (f0[None], f1[None]) if squeeze else (f0, f1)
        t = self.embedding(torch.cat([ref_points, src_points]).contiguous())          # row-wise: both clouds in one pass
        f = F.linear(torch.cat([ref_feats, src_feats]), self.in_proj.weight, self.in_proj.bias)
        t0, t1 = t[:n0], t[n0:]
        f0, f1 = self.transformer(f[:n0], f[n0:], t0, t1, ref_lens, src_lens)
        f = F.linear(torch.cat([f0, f1]), self.out_proj.weight, self.out_proj.bias)
        f0, f1 = f[:n0], f[n0:]
        if return_pos_emb:
            return (f0[None], f1[None], t0[None], t1[None]) if squeeze else (f0, f1, t0, t1)
        return (f0[None], f1[None]) if squeeze else (f0, f1)
