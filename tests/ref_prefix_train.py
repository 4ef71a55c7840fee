"""Plain fp64 reference of the packed shared-prefix attention for training (include/mpv.h: mpv_attn_prefix_packed_fwd_lse,
mpv_attn_prefix_packed_bwd), TEST INFRASTRUCTURE ONLY.  It is composed from ref_attention.attn_fwd_ref / attn_bwd_ref, applied per
continuation to the concatenated keys [its group's prefix | its own rows] with `visible` = every prefix key plus the causal own keys and
scale_q_bf16 = 0; a group's dpk / dpv are the sums of the prefix keys' dK / dV over the group's continuations.  It looks neither at
youku_mplug_amd.ops nor at the stand-ins nor at the kernels' source.

Tensors: q / k / v / dO [rows, heads, hd], pk / pv [groups, heads, P, hd] (any strides, any device).  Every output comes with its SCALE
per element (ref_attention: the sum of the absolute terms that form it); for dpk / dpv the sum of the continuations' scales, plus
|dpk_in| when accumulating.

model=True is the ROUNDING MODEL of the kernels: P (for o and dV) and dS rounded to bf16, every output rounded once -- dpk / dpv once
for the whole group's sum (with the tensor accumulated into, if any), which is why the prefix part of the model is restated here instead
of summing attn_bwd_ref's already rounded rows."""
import torch

import ref_attention as R
from ref_attention import BF, F64, f32, rbf


def continuations(cont_len, conts_per_group):
    """[(group, first row, rows)] in packed order"""
    out, row, c = [], 0, 0
    for g, n in enumerate(conts_per_group):
        for _ in range(n):
            out.append((g, row, cont_len[c]))
            row += cont_len[c]
            c += 1
    return out


def visible_of(n, P, device):
    """bool [n, P + n]: every prefix key, and own key j of row i iff j <= i"""
    i = torch.arange(n, device=device)[:, None]
    j = torch.arange(P + n, device=device)[None, :]
    return (j < P) | (j - P <= i)


def _cat(pre, own, g, a, n, P):
    """[1, heads, P + n, hd]: group g's prefix rows in front of the continuation's own"""
    x = own[a:a + n].transpose(0, 1)
    return (x if P == 0 else torch.cat([pre[g], x], dim=1))[None]


def _prefix_model(q, K, V, o_given, lse_given, dO, vis, scale, P):
    """The prefix keys' dK / dV of one continuation with dS and P rounded to bf16 as the kernels round them and the results NOT rounded"""
    s = (q.to(F64) @ K.to(F64).transpose(-1, -2) * f32(scale)).masked_fill(~vis, float("-inf"))
    Pm = torch.exp(s - lse_given.to(F64)[..., None])
    dd = dO.to(F64)
    dS = rbf(Pm * (dd @ V.to(F64).transpose(-1, -2) - (dd * o_given.to(F64)).sum(-1)[..., None]))
    return (dS.transpose(-1, -2) @ (q.to(F64) * f32(scale)))[..., :P, :], (rbf(Pm).transpose(-1, -2) @ dd)[..., :P, :]


def reference(q, k, v, do, pk, pv, cont_len, conts_per_group, P, scale, dpk_in=None, dpv_in=None, model=False, exact_given=False):
    """-> dict of fp64 tensors: o, lse [heads, rows], dq, dk, dv [rows, heads, hd], dpk, dpv [groups, heads, P, hd], a scale_<name> for
    each, and o_given (bf16) / lse_given (fp32): what the backward is given -- the rounded forward reference, so that a backward is
    judged on its own (exact_given: the fp64 forward itself instead, for the comparison with autograd).  dpk_in / dpv_in: the tensors
    accumulated into (accumulate_prefix = 1), or None."""
    rows, heads, hd = q.shape
    G, dev = len(conts_per_group), q.device
    z = lambda *s: torch.zeros(*s, dtype=F64, device=dev)      # noqa: E731
    out = {n: z(rows, heads, hd) for n in ("o", "dq", "dk", "dv", "scale_o", "scale_dq", "scale_dk", "scale_dv")}
    out.update({n: z(heads, rows) for n in ("lse", "scale_lse")})
    out.update({n: z(G, heads, P, hd) for n in ("dpk", "dpv", "scale_dpk", "scale_dpv")})
    out["o_given"] = torch.zeros(rows, heads, hd, dtype=BF, device=dev)
    put = lambda name, a, n, x: out[name][a:a + n].copy_(x[0].transpose(0, 1))      # noqa: E731
    for g, a, n in continuations(cont_len, conts_per_group):
        vis = visible_of(n, P, dev)
        qq, dd = q[a:a + n].transpose(0, 1)[None], do[a:a + n].transpose(0, 1)[None]
        K, V = _cat(pk, k, g, a, n, P), _cat(pv, v, g, a, n, P)
        fwd = R.attn_fwd_ref(qq, K, V, False, scale, 0, visible=vis, model=model)
        exact = fwd if not model else R.attn_fwd_ref(qq, K, V, False, scale, 0, visible=vis)
        o_given, lse_given = (exact["o"], exact["lse"]) if exact_given else (rbf(exact["o"]).to(BF), exact["lse"].to(torch.float32))
        out["o_given"][a:a + n] = rbf(exact["o"])[0].transpose(0, 1).to(BF)
        bwd = R.attn_bwd_ref(qq, K, V, o_given, lse_given, dd, False, scale, 0, visible=vis, model=model)
        put("o", a, n, fwd["o"])
        put("scale_o", a, n, fwd["scale_o"])
        out["lse"][:, a:a + n] = fwd["lse"][0]
        out["scale_lse"][:, a:a + n] = fwd["scale_lse"][0]
        for name in ("dq", "scale_dq"):
            put(name, a, n, bwd[name])
        for name in ("dk", "dv", "scale_dk", "scale_dv"):
            put(name, a, n, bwd[name][..., P:, :])
        if P:
            pkm, pvm = _prefix_model(qq, K, V, o_given, lse_given, dd, vis, scale, P) if model else (bwd["dk"][..., :P, :], bwd["dv"][..., :P, :])
            out["dpk"][g] += pkm[0]
            out["dpv"][g] += pvm[0]
            out["scale_dpk"][g] += bwd["scale_dk"][0, :, :P]
            out["scale_dpv"][g] += bwd["scale_dv"][0, :, :P]
    for name, t in (("dpk", dpk_in), ("dpv", dpv_in)):
        if t is not None:
            out[name] += t.to(F64)
            out["scale_" + name] += t.to(F64).abs()
        if model:
            out[name] = rbf(out[name])
    out["lse_given"] = out["lse"].to(torch.float32)
    return out


def textbook(q, k, v, do, pk, pv, cont_len, conts_per_group, P, scale):
    """fp64 autograd of the textbook masked softmax over the materialised concatenation: the yardstick of reference() on the CPU.
    -> o, lse, dq, dk, dv, dpk, dpv"""
    rows, heads, hd = q.shape
    leaf = lambda t: t.to(F64).clone().requires_grad_(True)      # noqa: E731
    ql, kl, vl, pkl, pvl = leaf(q), leaf(k), leaf(v), leaf(pk), leaf(pv)
    o = torch.zeros(rows, heads, hd, dtype=F64, device=q.device)
    lse = torch.zeros(heads, rows, dtype=F64, device=q.device)
    outs = []
    for g, a, n in continuations(cont_len, conts_per_group):
        K = torch.cat([pkl[g], kl[a:a + n].transpose(0, 1)], dim=1)
        V = torch.cat([pvl[g], vl[a:a + n].transpose(0, 1)], dim=1)
        s = (ql[a:a + n].transpose(0, 1) @ K.transpose(-1, -2) * f32(scale)).masked_fill(~visible_of(n, P, q.device), float("-inf"))
        oc = torch.softmax(s, dim=-1) @ V
        outs.append((oc * do[a:a + n].transpose(0, 1).to(F64)).sum())
        o[a:a + n] = oc.detach().transpose(0, 1)
        lse[:, a:a + n] = torch.logsumexp(s.detach(), dim=-1)
    torch.stack(outs).sum().backward()
    return dict(o=o, lse=lse, dq=ql.grad, dk=kl.grad, dv=vl.grad, dpk=pkl.grad, dpv=pvl.grad)
