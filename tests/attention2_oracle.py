"""TEST-ONLY fp64 reference of the second derivative of the self-attention core and of its gated residual (ctgan_amd/attention.py:
AttentionBwdFn, AttnResidualBwdFn; csrc/attention.hip): plain torch autograd of the composite softmax(q k^T) v of tests/attention_oracle.py,
differentiated twice - no formula of DESIGN 33 is restated here.  Nothing under ctgan_amd/ imports this file."""
import torch

from tests import attention_oracle as AO


def inputs(shape, kind, seed=0):
    """(q, k, v, gout, a, b, c) of a case: the draws of tests/test_gpu_attention.py's _inputs, then the cotangents a, b, c of gq, gk, gv from
    the same generator after gout.  kind: 'normal', 'scores80' (largest |score| 80), 'equal_row' (a zero query row)."""
    n, N, dk, dv = shape
    g = torch.Generator().manual_seed(seed + 1000 * N + dk)
    q, k = torch.randn(n, N, dk, generator=g), torch.randn(n, N, dk, generator=g)
    v, gout = torch.randn(n, N, dv, generator=g), torch.randn(n, N, dv, generator=g)
    a, b = torch.randn(n, N, dk, generator=g), torch.randn(n, N, dk, generator=g)
    c = torch.randn(n, N, dv, generator=g)
    if kind == 'scores80':
        s = (q.double() @ k.double().transpose(1, 2)).abs().max().sqrt().item()
        q, k = q * (80 ** 0.5 / s), k * (80 ** 0.5 / s)
    if kind == 'equal_row':
        q[:, 5] = 0.
    return q, k, v, gout, a, b, c


def core_grads2(q, k, v, gout, a, b, c, dtype=torch.float64):
    """-> (dq, dk, dv, dgout): the gradient of <gq, a> + <gk, b> + <gv, c> with (gq, gk, gv) = the gradient of <out, gout>, by autograd on
    detached fp64 copies.  A cotangent may be None; a result that the cost does not depend on (dv with a = b = None: gv = P^T gout does not
    contain v) is zeros."""
    ins = tuple(t.detach().to(dtype).requires_grad_(True) for t in (q, k, v, gout))
    out, _ = AO.core(*ins[:3], dtype)
    firsts = torch.autograd.grad(out, ins[:3], ins[3], create_graph=True)
    cost = sum((g * ct.to(dtype)).sum() for g, ct in zip(firsts, (a, b, c)) if ct is not None)
    grads = torch.autograd.grad(cost, ins, allow_unused=True)
    return tuple(torch.zeros_like(t) if g is None else g for g, t in zip(grads, ins))


def residual_grads2(gy, o, gamma, cgo, cgg, dtype=torch.float64):
    """-> (dgy, d_o, dgamma) of <go, cgo> + ggamma cgg with (go, ggamma) = the gradient of <x + gamma o, gy> in (o, gamma); cgg may be None
    (then d_o is None)."""
    gy, o, gamma = (t.detach().to(dtype).requires_grad_(True) for t in (gy, o, gamma))
    x = torch.zeros_like(o, requires_grad=True)
    _, go, gg = torch.autograd.grad(AO.residual(x, o, gamma), (x, o, gamma), gy, create_graph=True)
    cost = (go * cgo.to(dtype)).sum()
    if cgg is not None:
        cost = cost + (gg * cgg.to(dtype)).sum()
    return torch.autograd.grad(cost, (gy, o, gamma), allow_unused=True)
