"""Case tables, input builders and gates of the LoRA kernel parity tests (tests/test_lora_kernels_gpu.py on the HIP kernels,
tests/test_lora_refs_cpu.py on the stand-ins of tests/standin_lora.py through the same runners), TEST INFRASTRUCTURE ONLY.

GATE.  |got - ref| <= RTOL_BF16 |ref| + coef x scale per element, ref and scale from tests/ref_lora.py.  RTOL_BF16 = 2^-8 is the half
step of the ONE bf16 rounding every output makes; coef covers the fp32 accumulation and starts from the project's cap COEF_CAP = 2^-12 (a
sixteenth of a bf16 ulp of the element's scale -- a condition, not a measurement).  profiles/lora_kernel_errors.md records the worst
measured residual / scale of each output; the coefficient is twice that, never above the cap.

SHAPES.  The smallest that reach every branch of csrc/lora.hip: down works on 32-row tiles and 4 x 64-column chunks (R = 1, 63, 129, 300;
C = 64: one wave has work, 72: a ragged chunk, 256: every wave); up_add on 128-row x 64-column tiles (N = 64, 200 ragged, 768);
wgrad on 64-column groups and row slices of 256 (R = 1, 64, 257: two slices, 1000: four; C = 64, 200 ragged).  All four ranks
(8 is half an MFMA step, 16 one, 32 two, 64 two rank tiles), both layouts of w / g, every leading dimension pitched, scale 1 and 1.5.
Inputs: guard rows and pitch columns of every INPUT hold NaN (a read outside the operand poisons the output), those of every OUTPUT a
sentinel that must come back untouched.  Each kernel is fed the bits its predecessor produced: up_add and wgrad take t from the down
entry under test, so every output is one rounding away from its reference."""
import itertools

import torch

import ref_lora as R_

BF = torch.bfloat16
RTOL_BF16 = 2.0 ** -8
COEF_CAP = 2.0 ** -12
SENT = -99.0
NAN = float("nan")
RANKS = (8, 16, 32, 64)
PAD = 8          # pitch columns (leading dimensions stay multiples of 8)
GUARD = 2        # guard rows behind every buffer

GATES = {                                 # twice the measured worst residual / scale (profiles/lora_kernel_errors.md), below COEF_CAP
    "down": (RTOL_BF16, 2.2e-09),         # measured 1.075e-09: R300-C64-r64-outmajor-s1.5
    "up_add": (RTOL_BF16, 2.0e-08),       # measured 9.691e-09: R300-C768-r64-rankmajor-s1.0
    "wgrad": (RTOL_BF16, 8.7e-09),        # measured 4.322e-09: R64-C200-r64-rankmajor-s1.0
}
assert all(c <= COEF_CAP for _, c in GATES.values())


def _cases(rows, cols):
    out = []
    for n, (R, C, r, rm) in enumerate(itertools.product(rows, cols, RANKS, (True, False))):
        out.append((R, C, r, rm, 1.5 if n % 2 else 1.0))
    return out


DOWN = _cases((1, 63, 129, 300), (64, 72, 256))
UP_ADD = _cases((1, 129, 300), (64, 200, 768))
WGRAD = _cases((1, 64, 257, 1000), (64, 200))


def case_id(c):
    R, C, r, rm, s = c
    return f"R{R}-C{C}-r{r}-{'rankmajor' if rm else 'outmajor'}-s{s}"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def padded(rows, cols, fill, device, values=None):
    """bf16 [rows + GUARD, cols + PAD] filled with `fill`, its [rows, cols] corner with `values` -> (buffer, the [rows, cols] view)"""
    buf = torch.full((rows + GUARD, cols + PAD), fill, dtype=BF)
    if values is not None:
        buf[:rows, :cols] = values.to(BF)
    buf = buf.to(device)
    return buf, buf[:rows, :cols]


def untouched(buf, rows, cols, what):
    """the guard rows and pitch columns of an output buffer still hold the sentinel"""
    b = buf.float().cpu()
    assert torch.equal(b[rows:], torch.full_like(b[rows:], SENT)), f"{what}: rows >= {rows} were written"
    assert torch.equal(b[:rows, cols:], torch.full_like(b[:rows, cols:], SENT)), f"{what}: columns >= {cols} were written"


def weight(n, r, rank_major, g, device, std=0.5):
    """the w operand over n in/out features: [r, n] rank-major or [n, r], pitched, NaN guards"""
    shape = (r, n) if rank_major else (n, r)
    return padded(*shape, NAN, device, torch.randn(shape, generator=g) * std)


def run_down(impl, c, device, seed=0):
    """-> measured coefficient inputs: runs the entry, checks guards, parity and row independence"""
    R, C, r, rm, scale = c
    g = _gen(1000 + seed)
    xb, x = padded(R, C, NAN, device, torch.randn((R, C), generator=g))
    wb, w = weight(C, r, rm, g, device)
    tb, t = padded(R, r, SENT, device)
    impl.lora_down(x, w, R, C, r, w_rank_major=rm, scale=scale, out=t)
    untouched(tb, R, r, f"down {case_id(c)}")
    ref, sc = R_.down_ref(xb.cpu(), wb.cpu(), R, C, r, rm, scale)
    R_.close_scaled(t, ref, sc, GATES["down"], f"down {case_id(c)}")
    for i in sorted({0, R // 2, R - 1}):          # row i of the R-row call has the bits of a one-row call on that row
        ob, o = padded(1, r, SENT, device)
        impl.lora_down(x[i:i + 1], w, 1, C, r, w_rank_major=rm, scale=scale, out=o)
        assert torch.equal(o.cpu(), t[i:i + 1].cpu()), f"down {case_id(c)}: row {i} depends on R"
    return t


def _t_from_down(impl, R, r, g, device):
    """t [R, r] as the down entry under test produces it (pitched, NaN guards behind it)"""
    x = (torch.randn((R, 64), generator=g)).to(BF).to(device)
    a = (torch.randn((r, 64), generator=g) * 0.25).to(BF).to(device)
    tb, t = padded(R, r, NAN, device)
    impl.lora_down(x, a, R, 64, r, w_rank_major=True, scale=1.0, out=t)
    return tb, t


def run_up_add(impl, c, device, seed=0):
    R, N, r, rm, scale = c
    g = _gen(2000 + seed)
    tb, t = _t_from_down(impl, R, r, g, device)
    wb, w = weight(N, r, rm, g, device)
    yb, y = padded(R, N, SENT, device, torch.randn((R, N), generator=g) * 2.0)
    y_old = yb.cpu().clone()
    impl.lora_up_add(t, w, y, R, N, r, w_rank_major=rm, scale=scale)
    untouched(yb, R, N, f"up_add {case_id(c)}")
    ref, sc = R_.up_add_ref(tb.cpu(), wb.cpu(), y_old, R, N, r, rm, scale)
    R_.close_scaled(y, ref, sc, GATES["up_add"], f"up_add {case_id(c)}")
    for i in sorted({0, R // 2, R - 1}):
        ob, o = padded(1, N, SENT, device, y_old[i:i + 1, :N])
        impl.lora_up_add(t[i:i + 1], w, o, 1, N, r, w_rank_major=rm, scale=scale)
        assert torch.equal(o.cpu(), y[i:i + 1].cpu()), f"up_add {case_id(c)}: row {i} depends on R"
    return y


def run_wgrad(impl, c, device, seed=0):
    R, C, r, rm, scale = c
    g = _gen(3000 + seed)
    tb, t = _t_from_down(impl, R, r, g, device)
    xb, x = padded(R, C, NAN, device, torch.randn((R, C), generator=g))
    shape = (r, C) if rm else (C, r)
    gb, gv = padded(*shape, SENT, device)
    impl.lora_wgrad(t, x, R, C, r, g_rank_major=rm, scale=scale, out=gv)
    untouched(gb, *shape, f"wgrad {case_id(c)}")
    ref, sc = R_.wgrad_ref(tb.cpu(), xb.cpu(), R, C, r, scale)
    got = gv.t() if rm else gv
    R_.close_scaled(got, ref, sc, GATES["wgrad"], f"wgrad {case_id(c)}")
    g2b, g2 = padded(*shape, SENT, device)
    impl.lora_wgrad(t, x, R, C, r, g_rank_major=rm, scale=scale, out=g2)
    assert torch.equal(g2b.cpu().float(), gb.cpu().float()), f"wgrad {case_id(c)}: two calls differ"
    return gv
