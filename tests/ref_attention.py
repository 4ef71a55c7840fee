"""Plain fp64 references of the attention family (csrc/attention.hip and its .inc files: mpv_attn_fwd / mpv_attn_bwd,
mpv_temporal_attn_fwd / _bwd and their _long forms) as include/mpv.h documents them, TEST INFRASTRUCTURE ONLY.  Every function restates
the operation in float64 torch on whatever device its inputs live on; none looks at tests/standin_ops.py or at the kernels' source.
tests/test_attention_refs_cpu.py checks them against fp64 autograd of the textbook form and a masked-einsum formulation;
tests/test_attention_kernels_gpu.py compares the HIP kernels with them element by element.

Tensors are [B, H, S, hd] (any strides).  Every output comes with its SCALE per element, the sum of the absolute terms that form it:
    o    sum_j p~_ij |v_jd|                 dV   sum_i p~_ij |dO_id|          (p~ = P keep drop_scale)
    dQ   scale sum_j |dS|+_ij |k_jd|        dK   sum_i |dS|+_ij |q''_id|      |dS|+ = P (sum_d |dO||v| keep drop_scale + sum_d |dO||o|)
    lse  the row's largest sum_d |q''_d k_jd| over its visible keys
q'' is what multiplies k in the score: q scale taken exactly (scale_q_bf16 = 0), q' = bf16(fp32(q) fp32(scale)) formed in float32 torch so
that it is the kernel's value bit for bit (1), or q itself, which is that q' already (2).

THE GATES (attention_cases.GATES, derived there) are |got - ref| <= rtol |ref| + coef x scale with rtol = 2^-8 for a bf16 output (one
rounding) and a coefficient per bf16 intermediate on the path: P for o and dV; dS and the given o inside delta for dQ and dK; plus
EPS = 2^-12 per intermediate, the fp32 allowance (accumulation order, v_exp_f32).  The functions below take model=True for the ROUNDING
MODEL: the same formulas with exactly those intermediates and the output rounded to bf16; the CPU test holds the model inside every gate."""
import torch

from ref_gemm import rbf
from ref_loss_optim import F64, close_elementwise, f32  # noqa: F401
from ref_norm import _mix32, close_scaled, drop_scale, drop_threshold  # noqa: F401

BF = torch.bfloat16
TINY = 1e-300
EPS = 2.0 ** -12
SEED_INDIRECT_BIT = 1 << 63


def visible_mask(sq, sk, causal, device="cpu"):
    """bool [sq, sk]: key j visible to query i iff not causal or j <= i + (sk - sq)   (include/mpv.h, mpv_attn_desc.causal)"""
    if not causal:
        return torch.ones(sq, sk, dtype=torch.bool, device=device)
    i = torch.arange(sq, device=device)[:, None]
    j = torch.arange(sk, device=device)[None, :]
    return j <= i + (sk - sq)


def q_eff(q, scale, scale_q_bf16):
    """-> q'' in fp64 (module text)"""
    if scale_q_bf16 == 1:
        return (q.float() * torch.tensor(scale, dtype=torch.float32, device=q.device)).to(BF).to(F64)
    if scale_q_bf16 == 2:
        return q.to(F64)
    return q.to(F64) * f32(scale)


def _scores(q, k, causal, scale, scale_q_bf16, visible):
    qq, kk = q_eff(q, scale, scale_q_bf16), k.to(F64)
    sq, sk = q.shape[-2], k.shape[-2]
    vis = visible_mask(sq, sk, causal, q.device) if visible is None else visible
    s = (qq @ kk.transpose(-1, -2)).masked_fill(~vis, float("-inf"))
    return qq, kk, s, vis


def attn_fwd_ref(q, k, v, causal, scale, scale_q_bf16, keep=None, drop_scale=1.0, visible=None, model=False):
    """-> dict(o, lse, P, scale_o, scale_lse), fp64.  Scores and softmax exact; o = (P keep drop_scale) V; lse = logsumexp of the scaled,
    masked scores, unaffected by dropout.  keep: bool [B, H, sq, sk] or None.  visible: a bool [sq, sk] mask INSTEAD of the causal rule
    (tests).  model: the rounding model -- p~ and o rounded to bf16."""
    qq, kk, s, vis = _scores(q, k, causal, scale, scale_q_bf16, visible)
    vv = v.to(F64)
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    Pt = P * float(drop_scale) if keep is None else torch.where(keep, P * float(drop_scale), torch.zeros_like(P))
    if model:
        Pt = rbf(Pt)
    o = Pt @ vv
    if model:
        o = rbf(o)
    s_lse = ((qq.abs() @ kk.abs().transpose(-1, -2)).masked_fill(~vis, 0.0)).max(dim=-1).values
    return dict(o=o, lse=lse, P=P, scale_o=Pt.abs() @ vv.abs(), scale_lse=s_lse)


def attn_bwd_ref(q, k, v, o_given, lse_given, dO, causal, scale, scale_q_bf16, keep=None, drop_scale=1.0, visible=None, model=False):
    """The backward as a formula from the values GIVEN (o_given: the bf16 output, lse_given: the fp32 statistics), fp64:
    P = exp(s - lse_given); delta = sum_d dO o_given; dP = (dO V^T) keep drop_scale; dS = P (dP - delta); dV = (P keep drop_scale)^T dO;
    dK = dS^T q''; dQ = scale dS K (with scale_q_bf16 the leaf is q' and the result is multiplied by scale: still the gradient of the
    unscaled q).  -> dict(dq, dk, dv, delta, scale_dq, scale_dk, scale_dv).  model: dS, p~ and the outputs rounded to bf16."""
    qq, kk, s, vis = _scores(q, k, causal, scale, scale_q_bf16, visible)
    vv, oo, dd = v.to(F64), o_given.to(F64), dO.to(F64)
    sc, ds = f32(scale), float(drop_scale)
    P = torch.exp(s - lse_given.to(F64)[..., None])
    km = torch.ones_like(P) * ds if keep is None else keep.to(F64) * ds
    delta = (dd * oo).sum(-1)
    dP = (dd @ vv.transpose(-1, -2)) * km
    dS = P * (dP - delta[..., None])
    Pt = P * km
    if model:
        dS, Pt = rbf(dS), rbf(Pt)
    dv = Pt.transpose(-1, -2) @ dd
    dk = dS.transpose(-1, -2) @ qq
    dq = (dS @ kk) * sc
    if model:
        dq, dk, dv = rbf(dq), rbf(dk), rbf(dv)
    dSp = P * ((dd.abs() @ vv.abs().transpose(-1, -2)) * km + (dd.abs() * oo.abs()).sum(-1)[..., None])
    return dict(dq=dq, dk=dk, dv=dv, delta=delta, scale_dq=(dSp @ kk.abs()) * sc, scale_dk=dSp.transpose(-1, -2) @ qq.abs(),
                scale_dv=Pt.abs().transpose(-1, -2) @ dd.abs())


# ------------------------------------------------------------------------------------------------------------------ dropout
def attn_keep_mask(seed, offset, B, H, sq, sk, p, device="cpu", deref=None):
    """bool [B, H, sq, sk], True where probability (b, h, row, key) is kept -- attention's own convention (include/mpv.h,
    mpv_attn_desc.dropout_p): element index = offset + ((b H + h) sq + row) sk + key; the pair's counter is the row's base index plus
    key & ~1 (pairs along the KEY axis, whatever the parity of the base), the low 16 bits of the pair's word serve the even key, the
    high 16 bits the odd key; kept iff that field >= mpv_drop_threshold(p).  ref_norm.keep_mask pairs on the global element index
    instead: the two agree only where the row base is even.  A seed with bit 63 set is the address of the 64-bit seed in device
    memory (mpv_resolve_seed): deref(address) -> its value."""
    M = 0xffffffff
    if seed & SEED_INDIRECT_BIT:
        seed = int(deref(seed & ~SEED_INDIRECT_BIT))
    ka, kb = _mix32(seed & M), _mix32(((seed >> 32) & M) ^ 0x85ebca6b)
    base = offset + torch.arange(B * H * sq, dtype=torch.int64, device=device)[:, None] * sk
    key = torch.arange(sk, dtype=torch.int64, device=device)[None, :]
    ctr = base + (key - (key & 1))
    word = _mix32((((ctr & M) + ka) & M) ^ (((ctr >> 32) + kb) & M))
    field = torch.where((key & 1) == 1, word >> 16, word & 0xffff)
    return (field >= drop_threshold(p)).view(B, H, sq, sk)


def attn_keep_scalar(seed, offset, b, h, row, key, H, sq, sk, p):
    """one element of attn_keep_mask in plain Python integers: attn_keep / mpv_keep / mpv_rand_pair restated (direct seeds only)"""
    M = 0xffffffff
    base = offset + ((b * H + h) * sq + row) * sk
    ctr = (base + (key & ~1)) & 0xffffffffffffffff
    ka, kb = _mix32(seed & M), _mix32(((seed >> 32) & M) ^ 0x85ebca6b)
    r = _mix32((((ctr & M) + ka) & M) ^ (((ctr >> 32) + kb) & M))
    return ((r >> 16) if key & 1 else (r & 0xffff)) >= drop_threshold(p)


# ------------------------------------------------------------------------------------------------------------------ needles
def needle_pairs(sq, sk, causal):
    """The (row, key) pairs of the `needle` input class, each row and each key used once: the causal diagonal of the first and of the last
    row (for sk > sq the first is key sk - sq of row 0), key 0, the last key, the first key of the last 32-key tile."""
    sh = sk - sq if causal else sk - 1
    want = []
    if causal:
        want += [(0, sk - sq), (sq - 1, sk - 1)]
    else:
        want += [(sq - 1, sk - 1)]
    tile0 = 32 * ((sk - 1) // 32)
    for key in (0, tile0, sk - 1):
        lo = max(0, key - sh) if causal else 0
        for row in (max(lo, sq // 2), max(lo, sq // 2 + 1), max(lo, sq // 2 + 2), lo):
            if row < sq and all(row != r and key != c for r, c in want):
                want.append((row, key))
                break
    out = []
    for r, c in want:
        if all(r != a and c != b for a, b in out):
            out.append((r, c))
    return out


def plant_needles(q, k, v, pairs, scale, bump=16.0):
    """In place on bf16 [B, H, S, hd] q / k / v: k_j += c q_i / |q_i| with c = bump / (scale |q_i|), so that the scaled score of (i, j)
    rises by `bump` over a field of unit-variance scores (p_ij > 0.9), and v_j becomes a distinctive row."""
    hd = q.shape[-1]
    mark = (4.0 * (1 - 2 * (torch.arange(hd, device=v.device) % 2)) + torch.arange(hd, device=v.device) / 16.0)
    for n, (i, j) in enumerate(pairs):
        qi = q[:, :, i, :].float()
        nrm = qi.norm(dim=-1, keepdim=True).clamp_min(1e-3)
        k[:, :, j, :] = (k[:, :, j, :].float() + qi / nrm * (bump / (scale * nrm))).to(BF)
        v[:, :, j, :] = (mark * (1.0 + 0.25 * n)).to(BF)


# ------------------------------------------------------------------------------------------------------------------ temporal
def temporal_split(qkv, B, N, T, heads, hd):
    """qkv [B*T*(N+1), 3D] in the layout of test_temporal_attention (sequence (b, n) has token t at row b*T*N1 + 1 + n + t*N1; row
    b*T*N1 + t*N1 is a cls row no problem owns) -> q, k, v as [B, N, heads, T, hd] views"""
    x = qkv.view(B, T, N + 1, 3, heads, hd)[:, :, 1:]
    return tuple(x[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))


def temporal_rows(x, B, N, T, heads, hd):
    """[B*T*(N+1), D] -> [B, N, heads, T, hd] view of the rows the problems own"""
    return x.view(B, T, N + 1, heads, hd)[:, :, 1:].permute(0, 2, 3, 1, 4)


def temporal_ref(qkv, dout, B, N, T, heads, hd, scale, model=False):
    """Both temporal entry points (mpv_temporal_attn_fwd / _bwd and _long_fwd / _long_bwd: include/mpv.h): q' = bf16(q scale) (every
    instance rounds it, as the model being replaced does); P = softmax(q' k^T) exact; out = P V; and the textbook backward from dout:
    dP = dO V^T, dS = P (dP - sum_j P dP), dq = scale dS K, dk = dS^T q', dv = P^T dO.  -> dict of [B, N, heads, T, hd] fp64 tensors
    out, dq, dk, dv and scale_* (sums of absolute terms; |dS|+ = P (sum_d |dO||v| + sum_j P sum_d |dO||v|)).  model: P (forward and
    dv), dS and the outputs rounded to bf16 -- the matrix-core instances; the VALU instances keep P and dS of the backward in fp32."""
    q, k, v = temporal_split(qkv, B, N, T, heads, hd)
    qq, kk, vv = q_eff(q, scale, 1), k.to(F64), v.to(F64)
    P = torch.softmax(qq @ kk.transpose(-1, -2), dim=-1)
    Pm = rbf(P) if model else P
    out = Pm @ vv
    res = dict(out=rbf(out) if model else out, scale_out=Pm @ vv.abs())
    if dout is None:
        return res
    dd = temporal_rows(dout, B, N, T, heads, hd).to(F64)
    sc = f32(scale)
    dP = dd @ vv.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    aP = dd.abs() @ vv.abs().transpose(-1, -2)
    dSp = P * (aP + (P * aP).sum(-1, keepdim=True))
    if model:
        dS = rbf(dS)
    dq, dk, dv = (dS @ kk) * sc, dS.transpose(-1, -2) @ qq, Pm.transpose(-1, -2) @ dd
    if model:
        dq, dk, dv = rbf(dq), rbf(dk), rbf(dv)
    res.update(dq=dq, dk=dk, dv=dv, scale_dq=(dSp @ kk.abs()) * sc, scale_dk=dSp.transpose(-1, -2) @ qq.abs(),
               scale_dv=Pm.transpose(-1, -2) @ dd.abs())
    return res


# ------------------------------------------------------------------------------------------------------------------ comparison
def close_gated(got, ref, scale, gate, what):
    """|got - ref| <= rtol |ref| + coef x scale for every element of tensors of any rank, the scale per element: both sides are divided by
    the scale and go through close_elementwise, whose printed residual is then the measured coefficient and whose failure names the
    element."""
    rtol, coef = gate
    s = scale.to(F64).clamp_min(TINY)
    assert tuple(got.shape) == tuple(ref.shape) == tuple(s.shape), f"{what}: shapes {tuple(got.shape)} / {tuple(ref.shape)} / {tuple(s.shape)}"
    close_elementwise(got.detach().to(F64) / s, ref.to(F64) / s, rtol, coef, what)


def residual(got, ref, scale, rtol):
    """the largest |got - ref| - rtol |ref| in units of the element's scale: what close_gated compares with coef"""
    s = scale.to(F64).clamp_min(TINY)
    g, r = got.detach().to(F64), ref.to(F64)
    return float((((g - r).abs() - rtol * r.abs()) / s).max().item())
