"""Plain fp64 references of the embedding fronts and the glue kernels (csrc/elementwise.hip, csrc/glue.hip), TEST INFRASTRUCTURE
ONLY.  Each function restates the operation from its definition (the comments of the .hip files and include/mpv.h give the rounding
order) with indexing and loops in float64 torch, on whatever device its inputs live on; none of them looks at tests/standin_ops.py.
tests/test_embed_glue_refs_cpu.py checks them against implementations they share nothing with (F.unfold, F.embedding, autograd of a
plain torch forward, torch.log_softmax + a stable sort); tests/test_embed_glue_kernels_gpu.py compares the HIP kernels with them
element by element.

A reference of a SUM also returns, per output element, the sum of the absolute values of its terms and the number of terms n: the
gate of such an output is rtol |ref| + n 2^-24 sum|terms| (tests/embed_glue_cases.py)."""
import numpy as np
import torch

from ref_loss_optim import F64, close_elementwise, worst  # noqa: F401  (re-exported: the one comparison of every suite)
from ref_norm import close_scaled, drop_scale, keep_mask  # noqa: F401

BF = torch.bfloat16


def r16(x):
    """fp64 -> the nearest bf16 (ties to even), back in fp64.  Through fp32 first, then repaired: the detour's own rounding can park a
    value ON a bf16 tie it was only close to, and the strictly nearer neighbour is taken instead (a true tie is an fp32 number and
    comes through the detour right)."""
    m = x.to(torch.float32).to(BF).to(F64)
    for up in (True, False):
        c = bf16_step(m, torch.full_like(m, up, dtype=torch.bool))
        m = torch.where((x - c).abs() < (x - m).abs(), c, m)
    return m


def bf16_step(m, up):
    """the bf16 neighbour of m (fp64 holding bf16 values) above (up) or below it; a zero stays (no case puts a mean there)"""
    i = m.to(BF).contiguous().view(torch.int16).to(torch.int32)
    away = (m > 0) == up                      # moving away from zero adds one to the magnitude bits
    j = torch.where(away, i + 1, i - 1).to(torch.int16)
    return torch.where(m == 0, m, j.view(BF).to(F64))


def r16_both(x, bound):
    """-> (bf16(x), the other bf16 neighbour where x lies within `bound` of the tie between the two, else bf16(x) again).  An fp32
    sum that differs from x by at most `bound` may round either way there; everywhere else the rounding is decided."""
    m = r16(x)
    other = bf16_step(m, x > m)
    near = ((x - (m + other) / 2).abs() <= bound) & (other != m)
    return m, torch.where(near, other, m)


# ------------------------------------------------------------------------------------------------------------------ im2col
def im2col_ref(video, B, C, T, H, W, P, kpad):
    """video [B, C, T, H, W] -> cols [B*T*(H/P)*(W/P), kpad] of the SAME dtype (a move): row (b, t, ph, pw), column c*P*P + i*P + j
    holds video[b, c, t, ph*P + i, pw*P + j]; columns from C*P*P on are +0."""
    v = video.reshape(B, C, T, H, W)
    out = torch.zeros((B * T * (H // P) * (W // P), kpad), dtype=video.dtype, device=video.device)
    for c in range(C):
        for i in range(P):
            for j in range(P):
                out[:, c * P * P + i * P + j] = v[:, c, :, i::P, j::P].reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------------------------ ViT token assembly
def assemble_fwd_ref(patch, cls, pos, temporal, B, T, N, D):
    """x[b, t, 0] = cls + pos[0] (no temporal term); x[b, t, 1 + n] = patch[b, t, n] + bf16(pos[1 + n] + temporal[t]) -> [B*T*(N+1), D]"""
    p, c, ps, tm = patch.to(F64).reshape(B, T, N, D), cls.to(F64).reshape(D), pos.to(F64).reshape(N + 1, D), temporal.to(F64).reshape(-1, D)
    x = torch.empty((B, T, N + 1, D), dtype=F64, device=patch.device)
    for t in range(T):
        x[:, t, 0] = c + ps[0]
        x[:, t, 1:] = p[:, t] + r16(ps[1:] + tm[t])[None]
    return x.reshape(-1, D)


def assemble_bwd_ref(dx, B, T, N, D):
    """-> dpatch (a move, dx's dtype), (dpos, sum|terms|, n), (dtemporal, sum|terms|, n); dcls is dpos[0]"""
    d = dx.to(F64).reshape(B, T, N + 1, D)
    dpatch = dx.reshape(B, T, N + 1, D)[:, :, 1:].reshape(B * T * N, D)
    dpos, apos = torch.zeros((N + 1, D), dtype=F64, device=dx.device), torch.zeros((N + 1, D), dtype=F64, device=dx.device)
    for b in range(B):
        for t in range(T):
            dpos += d[b, t]
            apos += d[b, t].abs()
    dtem, atem = torch.zeros((T, D), dtype=F64, device=dx.device), torch.zeros((T, D), dtype=F64, device=dx.device)
    for t in range(T):
        for b in range(B):
            dtem[t] += d[b, t, 1:].sum(0)
            atem[t] += d[b, t, 1:].abs().sum(0)
    return dpatch, (dpos, apos, B * T), (dtem, atem, B * N)


# ------------------------------------------------------------------------------------------------------------------ cls merge
def cls_mean_ref(a_cls, T):
    """a_cls [B, T, D] -> (mean over t, sum|terms| of that mean, n): T terms a / T, plus the rounding of 1 / T and of the product"""
    s, sa = torch.zeros_like(a_cls[:, 0], dtype=F64), torch.zeros_like(a_cls[:, 0], dtype=F64)
    for t in range(T):
        s += a_cls[:, t].to(F64)
        sa += a_cls[:, t].to(F64).abs()
    return s / T, sa / T, T + 2


def cls_merge_fwd_ref(xt, a, B, T, N1, D):
    """y = xt + a on the token rows; y[b, t, 0] = xt[b, t, 0] + bf16(mean_t' a[b, t', 0]).  -> (y, y_alt): y_alt differs from y only
    in cls elements whose mean lies within the fp32 sum's error bound of a bf16 tie, where it holds the other rounding."""
    x, av = xt.to(F64).reshape(B, T, N1, D), a.to(F64).reshape(B, T, N1, D)
    y = x + av
    mean, sa, n = cls_mean_ref(av[:, :, 0], T)
    m, m_alt = r16_both(mean, n * 2.0 ** -24 * sa)
    y_alt = y.clone()
    for t in range(T):
        y[:, t, 0] = x[:, t, 0] + m
        y_alt[:, t, 0] = x[:, t, 0] + m_alt
    return y.reshape(-1, D), y_alt.reshape(-1, D)


def cls_merge_bwd_ref(dy, B, T, N1, D):
    """da = dy on the token rows (a move); da[b, t, 0] = mean_t' dy[b, t', 0] for every t -> (mean [B, D], sum|terms|, n)"""
    return cls_mean_ref(dy.reshape(B, T, N1, D)[:, :, 0], T)


# ------------------------------------------------------------------------------------------------------------------ colsum / add
def colsum_ref(x, out0=None):
    """x [rows, cols] (the mapped rows, gathered) -> (sum over rows (+ out0), sum|terms|, n)"""
    s, sa = torch.zeros(x.shape[1], dtype=F64, device=x.device), torch.zeros(x.shape[1], dtype=F64, device=x.device)
    for lo in range(0, x.shape[0], 256):
        blk = x[lo:lo + 256].to(F64)
        s += blk.sum(0)
        sa += blk.abs().sum(0)
    n = x.shape[0]
    if out0 is not None:
        s, sa, n = s + out0.to(F64), sa + out0.to(F64).abs(), n + 1
    return s, sa, n


def add_ref(a, b):
    return a.to(F64) + b.to(F64)


# ------------------------------------------------------------------------------------------------------------------ GPT embedding front
def gpt_embed_fwd_ref(query, ids, wte, wpe, B, Q, L, H, keep=None, scale=1.0):
    """h[b, s] = (query[b, s] if s < Q else wte[ids[b, s - Q]]) + wpe[s]; with dropout (keep given): bf16(h) * scale where kept, 0
    elsewhere (the sum is rounded to bf16 BEFORE the mask scales it).  -> [B*(Q+L), H]"""
    S = Q + L
    h = torch.empty((B, S, H), dtype=F64, device=wte.device)
    for b in range(B):
        for s in range(S):
            src = query.reshape(B, Q, H)[b, s] if s < Q else wte[int(ids[b, s - Q])]
            h[b, s] = src.to(F64) + wpe[s].to(F64)
    h = h.reshape(B * S, H)
    if keep is not None:
        h = torch.where(keep, r16(h) * scale, torch.zeros_like(h))
    return h


def gpt_embed_bwd_full_ref(dh, keep=None, scale=1.0):
    """d[r] = dh[r] * scale where kept, 0 elsewhere (every row); the query rows of it are mpv_gpt_embed_bwd's result"""
    d = dh.to(F64)
    return d if keep is None else torch.where(keep, d * scale, torch.zeros_like(d))


def gpt_embed_rows_ref(ids, pos, wte, wpe):
    """out[r] = wte[ids[r]] + wpe[min(max(pos[r], 0), max_positions - 1)]"""
    out = torch.empty((len(ids), wte.shape[1]), dtype=F64, device=wte.device)
    for r in range(len(ids)):
        out[r] = wte[int(ids[r])].to(F64) + wpe[min(max(int(pos[r]), 0), wpe.shape[0] - 1)].to(F64)
    return out


# ------------------------------------------------------------------------------------------------------------------ log-prob top-k
def logprob_topk_ref(logits, k, add=None):
    """logits [rows, V] (the bf16 values) -> (values fp64 [rows, k], indices int64 [rows, k], logsumexp fp64 [rows]): the k first entries
    of every row in (logit descending, index ascending) order -- an order of the LOGITS, whatever `add` holds -- and
    logit - logsumexp(row) + add[row].  add = -inf gives -inf values."""
    x = logits.to(F64).cpu()
    rows, V = x.shape
    idx = torch.empty((rows, k), dtype=torch.int64)
    val = torch.empty((rows, k), dtype=F64)
    lses = torch.empty(rows, dtype=F64)
    for r in range(rows):
        v = x[r].numpy()
        order = np.lexsort((np.arange(V), -v))[:k]          # last key first: by -value, then by index
        mx = v.max()
        lse = mx + np.log(np.exp(v - mx).sum())
        a = 0.0 if add is None else float(add[r])
        idx[r] = torch.from_numpy(order.astype(np.int64))
        val[r] = torch.from_numpy(v[order] - lse + a) if a != float("-inf") else float("-inf")
        lses[r] = float(lse)
    return val, idx, lses


# ------------------------------------------------------------------------------------------------------------------ fp32 window
def f32_to_bf16_ref(src):
    """round-to-nearest-even on the bit pattern (finite values and infinities; no case holds a NaN): add 0x7fff + the lowest kept
    bit, drop 16 bits.  Subnormals round like everything else; a carry out of the mantissa moves to the next binade, at the top to inf."""
    b = src.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    out = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    out = torch.where(out >= 0x8000, out - 0x10000, out)      # as a signed 16-bit pattern
    return out.to(torch.int16).view(BF)


def accum_f32_ref(gs):
    """the window sum as the kernel forms it: fp32, acc = g0, then one fp32 addition per call in call order (exact to reproduce)"""
    acc = gs[0].float().clone()
    for g in gs[1:]:
        acc = acc + g.float()
    return acc


# ------------------------------------------------------------------------------------------------------------------ composed projection
def compose_finish_ref(P, dbc, bp, wf, D):
    """-> dwf [D, D] = P + dbc[i] bp[j]; (dbp [D] = sum_i wf[i][j] dbc[i], sum|terms|, n)"""
    Pm, d, b, w = P.to(F64).reshape(D, D), dbc.to(F64).reshape(D), bp.to(F64).reshape(D), wf.to(F64).reshape(D, D)
    dwf = torch.empty((D, D), dtype=F64, device=P.device)
    dbp, adbp = torch.zeros(D, dtype=F64, device=P.device), torch.zeros(D, dtype=F64, device=P.device)
    for i in range(D):
        dwf[i] = Pm[i] + d[i] * b
        dbp += w[i] * d[i]
        adbp += (w[i] * d[i]).abs()
    return dwf, (dbp, adbp, D)


def compose_bias_ref(wf, bp, bf, D):
    """bc[r] = sum_j wf[r][j] bp[j] + bf[r] -> (bc, sum|terms|, n)"""
    w, b, f = wf.to(F64).reshape(D, D), bp.to(F64).reshape(D), bf.to(F64).reshape(D)
    bc, abc = f.clone(), f.abs()
    for j in range(D):
        bc += w[:, j] * b[j]
        abc += (w[:, j] * b[j]).abs()
    return bc, abc, D + 1


# ------------------------------------------------------------------------------------------------------------------ caption targets
def caption_targets_ref(ids, mask, plen=None):
    """label[b][l] = ids[b][l + 1] (l < L - 1), ids[b][1] (l = L - 1), 0 when L = 1; weight[b][l] = mask[b][l + 1] / total for
    l < L - 1 and l >= plen[b], 0 elsewhere; total = the sum of the counted mask entries.  -> (labels int64 [B*L], weights fp64 [B*L])"""
    ids, mask = ids.cpu().tolist(), mask.cpu().tolist()
    pl = None if plen is None else plen.cpu().tolist()
    B, L = len(ids), len(ids[0])
    labels, w = [], []
    for b in range(B):
        for l in range(L):
            labels.append(0 if L == 1 else ids[b][l + 1 if l < L - 1 else 1])
            w.append(float(mask[b][l + 1]) if l < L - 1 and not (pl is not None and l < pl[b]) else 0.0)
    total = sum(w)
    return torch.tensor(labels, dtype=torch.int64), torch.tensor([v / total if v else 0.0 for v in w], dtype=F64)
