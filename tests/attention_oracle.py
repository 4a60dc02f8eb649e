"""TEST-ONLY fp64 restatement of the self-attention core and block of ctgan_amd/attention.py (csrc/attention.hip): plain torch autograd with
the [n, N, N] scores materialised.  Nothing under ctgan_amd/ imports this file."""
import torch


def core(q, k, v, dtype=torch.float64):
    """q, k [n, N, dk], v [n, N, dv] -> (out [n, N, dv], lse [n, N]): softmax over the keys of q k^T (no 1 / sqrt(dk) scale)."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    s = q @ k.transpose(1, 2)
    return torch.softmax(s, dim=2) @ v, torch.logsumexp(s, dim=2)


def core_grads(q, k, v, gout, dtype=torch.float64):
    """-> (out, lse, gq, gk, gv) by autograd on detached fp64 copies"""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    out, lse = core(q, k, v, dtype)
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), gout.to(dtype))
    return out.detach(), lse.detach(), gq, gk, gv


def residual(x, o, gamma):
    return x + gamma.reshape(()) * o


def conv1x1(x, w):
    """x logical [n, c, H, W], w the registry's HWIO filter [1, 1, c, k] -> [n, k, H, W]"""
    return torch.einsum('nchw,ck->nkhw', x, w[0, 0].to(x.dtype))


def block(x, wq, wk, wv, wo, gamma):
    """SelfAttention(name, dim, x) in x's dtype: x [n, dim, H, W], the four HWIO 1x1 filters, gamma [1] -> x + gamma Out(attention(.))"""
    n, c, h, w = x.shape

    def rows(t):
        return t.permute(0, 2, 3, 1).reshape(n, h * w, t.shape[1])

    o, _ = core(rows(conv1x1(x, wq)), rows(conv1x1(x, wk)), rows(conv1x1(x, wv)), dtype=x.dtype)
    o = o.reshape(n, h, w, -1).permute(0, 3, 1, 2)
    return residual(x, conv1x1(o, wo), gamma.to(x.dtype))
