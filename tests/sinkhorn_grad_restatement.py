"""The reverse pass of LearnableLogOptimalTransport restated in fp64 torch, independent of csrc/sinkhorn_grad.hip.

Forward (oracle/torch_ref.log_optimal_transport): S = padded scale * raw with dustbin row / column alpha; u_0 = v_0 = 0;
u_t = log_mu - LSE_j(S + v_{t-1}); v_t = log_nu - LSE_i(S + u_t); Z = S + u_T + v_T - norm.  Reverse, given G = dL/dZ:

    dS = G;  du = rowsum(G);  dv = colsum(G)
    for t = T..1:
        Pc = exp(S + u_t + v_t - log_nu)          dS -= Pc * dv[None, :];  du -= Pc @ dv
        Pr = exp(S + v_{t-1} + u_t - log_mu)      dS -= Pr * du[:, None];  dv = -(Pr^T @ du);  du = 0
    d_raw = scale * dS[:M, :N];  d_alpha = sum dS[M, :] + sum dS[:M, N]

Masked rows and columns are absent (G, Pc, Pr, dS zero there); a problem without a valid row or column gets dS = 0.

MISTAKES are switches that plant one error each; the tests assert that every one of them moves the result far beyond the tolerance."""
import torch

MISTAKES = ("v_same", "du_not_reset", "g_unmasked", "scale_dropped", "alpha_no_column", "one_iteration_short")


def mistake_shows(mistake, iters):
    """Whether a planted mistake can move the result at this iteration count.  Zero iterations are no transport; du is not read again
    after the last reverse step; and the mistakes in the iteration itself (the wrong v, a missing step) fade as the iteration converges —
    v_t - v_{t-1} is below fp64 rounding long before 100 steps — so they are planted where the iteration is short."""
    if mistake in ("v_same", "one_iteration_short", "du_not_reset"):
        return iters == 2 or (iters == 1 and mistake == "v_same")
    return True


def restate(raw, row_masks, col_masks, alpha, scale, G, iters, mistake=None, dtype=torch.float64):
    """-> (d_raw [B,M,N], d_alpha scalar, dS [B,M+1,N+1], d_alpha_part [B]) in `dtype`."""
    assert mistake is None or mistake in MISTAKES
    B, M, N = raw.shape
    raw, G, alpha = raw.to(dtype), G.to(dtype), torch.as_tensor(alpha).to(dtype)
    vr = torch.ones(B, M + 1, dtype=torch.bool)
    vr[:, :M] = row_masks.bool()
    vc = torch.ones(B, N + 1, dtype=torch.bool)
    vc[:, :N] = col_masks.bool()
    nr, nc = row_masks.bool().sum(1), col_masks.bool().sum(1)
    ok = (nr > 0) & (nc > 0)
    V = vr[:, :, None] & vc[:, None, :] & ok[:, None, None]
    S = torch.full((B, M + 1, N + 1), float(alpha), dtype=dtype)
    S[:, :M, :N] = raw * scale
    S = S.masked_fill(~V, float("-inf"))
    nrf, ncf = nr.clamp(min=1).to(dtype), nc.clamp(min=1).to(dtype)
    norm = -torch.log(nrf + ncf)
    log_mu = norm[:, None].expand(B, M + 1).clone()
    log_mu[:, M] = torch.log(ncf) + norm
    log_nu = norm[:, None].expand(B, N + 1).clone()
    log_nu[:, N] = torch.log(nrf) + norm
    vr, vc = vr & ok[:, None], vc & ok[:, None]
    zr, zc = torch.zeros(B, M + 1, dtype=dtype), torch.zeros(B, N + 1, dtype=dtype)
    log_mu, log_nu = torch.where(vr, log_mu, zr), torch.where(vc, log_nu, zc)
    T = iters - 1 if mistake == "one_iteration_short" else iters
    us, vs = [None], [zc]
    for _ in range(T):
        u = torch.where(vr, log_mu - torch.logsumexp(S + vs[-1][:, None, :], 2), zr)
        v = torch.where(vc, log_nu - torch.logsumexp(S + u[:, :, None], 1), zc)
        us.append(u)
        vs.append(v)
    Gm = G.clone() if mistake == "g_unmasked" else torch.where(V, G, torch.zeros_like(G))
    dS = Gm.clone()
    du, dv = Gm.sum(2), Gm.sum(1)
    for t in range(T, 0, -1):
        Pc = torch.exp(S + us[t][:, :, None] + vs[t][:, None, :] - log_nu[:, None, :])
        term = Pc * dv[:, None, :]
        dS = dS - term
        du = du - term.sum(2)
        vprev = vs[t] if mistake == "v_same" else vs[t - 1]
        Pr = torch.exp(S + vprev[:, None, :] + us[t][:, :, None] - log_mu[:, :, None])
        term = Pr * du[:, :, None]
        dS = dS - term
        dv = -term.sum(1)
        if mistake != "du_not_reset":
            du = torch.zeros_like(du)
    d_raw = dS[:, :M, :N] * (1.0 if mistake == "scale_dropped" else scale)
    part = dS[:, M, :].sum(1)
    if mistake != "alpha_no_column":
        part = part + dS[:, :M, N].sum(1)
    return d_raw, part.sum(), dS, part


def autograd_reference(raw, row_masks, col_masks, alpha, scale, G, iters, dtype):
    """(d_raw, d_alpha) by torch autograd through oracle/torch_ref.log_optimal_transport in `dtype`, on the CPU."""
    from oracle import torch_ref
    r = raw.to(dtype).clone().requires_grad_()
    a = torch.as_tensor(alpha).to(dtype).clone().requires_grad_()
    out = torch_ref.log_optimal_transport(r * scale, row_masks.bool(), col_masks.bool(), a, iters=iters)
    (out * G.to(dtype)).sum().backward()
    return r.grad, a.grad


def problem(B, M, N, seed, spread=1.0):
    """Random scores (normal * spread), row and column masks with at least one valid line each, alpha, and a random G: as drawn (G_raw) and
    zeroed on masked lines (G)."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, M, N, generator=g) * spread
    rm = torch.rand(B, M, generator=g) > 0.2
    cm = torch.rand(B, N, generator=g) > 0.15
    rm[:, 0] = cm[:, 0] = True
    G_raw = torch.randn(B, M + 1, N + 1, generator=g)
    V = torch.ones(B, M + 1, N + 1, dtype=torch.bool)
    V[:, :M, :] &= rm[:, :, None]
    V[:, :, :N] &= cm[:, None, :]
    return raw, rm, cm, torch.tensor(0.7), G_raw, torch.where(V, G_raw, torch.zeros_like(G_raw)), V


def bound(e_ref, scale):
    """the tolerance rule of the native training rows: 4 x the error of the reference's own fp32 arithmetic, floor 2^-20 of the scale"""
    return max(4.0 * e_ref, 2.0 ** -20 * scale)


def dense_transport(scores, rm, cm, alpha, iters=100, inf=1e12):
    """learnable_sinkhorn.py:20-66 in torch on the device the scores live on (oracle/torch_ref.log_optimal_transport builds its masks on
    the CPU)."""
    B, M, N = scores.shape
    prm = torch.zeros(B, M + 1, dtype=torch.bool, device=scores.device)
    prm[:, :M] = ~rm
    pcm = torch.zeros(B, N + 1, dtype=torch.bool, device=scores.device)
    pcm[:, :N] = ~cm
    S = torch.cat([torch.cat([scores, alpha.expand(B, M, 1)], -1), alpha.expand(B, 1, N + 1)], 1)
    S = S.masked_fill(prm[:, :, None] | pcm[:, None, :], -inf)
    nr, nc = rm.float().sum(1), cm.float().sum(1)
    norm = -torch.log(nr + nc)
    log_mu = norm[:, None].expand(B, M + 1).clone()
    log_mu[:, M] = torch.log(nc) + norm
    log_mu[prm] = -inf
    log_nu = norm[:, None].expand(B, N + 1).clone()
    log_nu[:, N] = torch.log(nr) + norm
    log_nu[pcm] = -inf
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(S + v[:, None, :], dim=2)
        v = log_nu - torch.logsumexp(S + u[:, :, None], dim=1)
    return S + u[:, :, None] + v[:, None, :] - norm[:, None, None]
