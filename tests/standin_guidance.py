"""mpv_logits_guide restated in torch fp32 on the CPU (include/mpv.h states the contract): what the kernel must equal bit for bit.
Every arithmetic step is its own torch op on fp32 tensors -- two subtracts, a subtract, a multiply, an add -- so nothing is fused, and
the scalars are the ones ops.logits_guide hands to the library: float32(scale - 1) and float32(log(alpha)), computed in double on the
host.  The signature is ops.logits_guide's, so the function also serves as a guide_fn of generation.guided_state_fn."""
import math

import torch


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float64).to(torch.float32)


def logits_guide(cond, uncond, *, scale, alpha=0.0, ban_value=float("-inf"), vocab=None):
    """cond bf16 [rows, ld_c] (edited in place over its first `vocab` columns), uncond bf16 [rows, ld_u] (read only) -> cond"""
    assert cond.dtype == uncond.dtype == torch.bfloat16 and not cond.is_cuda and not uncond.is_cuda and cond.shape[0] == uncond.shape[0]
    V = int(vocab) if vocab is not None else min(cond.shape[1], uncond.shape[1])
    scale_m1, plaus_log = _f32(float(scale) - 1.0), _f32(math.log(alpha) if alpha > 0.0 else float("-inf"))
    ban = _f32(ban_value).to(torch.bfloat16)                                 # round to nearest even, -inf stays
    x, y = cond[:, :V].to(torch.float32), uncond[:, :V].to(torch.float32)
    m_c = x.max(dim=1, keepdim=True).values
    m_u = y.max(dim=1, keepdim=True).values
    m_c = torch.where(m_c == 0, torch.zeros_like(m_c), m_c)                  # a zero maximum counts as +0
    m_u = torch.where(m_u == 0, torch.zeros_like(m_u), m_u)
    c = torch.sub(x, m_c)
    u = torch.sub(y, m_u)
    diff = torch.sub(c, u)
    prod = torch.mul(diff, scale_m1)
    g = torch.add(c, prod)
    out = g.to(torch.bfloat16)                                               # round to nearest even
    cond[:, :V] = torch.where(c < plaus_log, ban.expand_as(out), out)
    return cond


def on_host(fn=logits_guide):
    """a guide_fn for device logits that runs the stand-in on the CPU and copies the result back (the end-to-end comparison)"""
    def guide(cond, uncond, **kw):
        host = cond.cpu()
        fn(host, uncond.cpu(), **kw)
        cond.copy_(host)
        return cond
    return guide
