"""Operands and shapes of the FP8 decoder-weight tests (include/mpv.h, "FP8 decoder weights"): shared by tests/test_w8_cpu.py, which
checks the constructions themselves on the host, and tests/test_w8_gpu.py, which runs the kernels on them."""
import math

import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn

# the value of every e4m3fn code (the two NaN codes 0x7f / 0xff are nan)
CODE_VALUE = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(F8).float()

QUANT_SHAPES = [(8, 16, 0), (24, 80, 0), (256, 256, 24), (1024, 2048, 0)]           # (N, K, ldw - K)
SWEEP_M = [1, 5, 16, 17, 33, 160, 512]
SWEEP_NK = [(8, 16), (16, 64), (24, 80), (256, 1024)]
LARGE = [(5, 2048, 8192), (160, 2048, 8192), (5, 6144, 2048), (160, 6144, 2048)]    # (M, N, K): both K splits, at 5 and 160 rows
EXACT_M = [1, 17, 40]
GATE = 1e-2                                                                         # test_gemm_forward_nt's: max-abs error over max-abs reference


def deq(codes, scale):
    """fp32 deq(code) * scale"""
    return codes.view(F8).float() * scale[:, None]


def exponent_of(amax: float) -> int:
    """the contract's scale exponent, in Python: the smallest e with amax <= 448 * 2^e (0 for a zero row)"""
    if amax == 0.0:
        return 0
    f, x = math.frexp(amax)
    return max(x - 9 if f <= 0.875 else x - 8, -126)


def quantiser_rows(K=64, seed=0):
    """bf16 rows [7, K]: std 0.02, 1 and 1e-5, a zero row, a row whose amax is exactly 448 * 2^-3, one just above it (the next bf16
    number: the exponent moves up), and one holding -0.0 and a single tiny value"""
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(7, K)
    w[0] = torch.randn(K, generator=g) * 0.02
    w[1] = torch.randn(K, generator=g)
    w[2] = torch.randn(K, generator=g) * 1e-5
    w[4] = torch.randn(K, generator=g).clamp(-3, 3) * 10
    w[4, 5] = -56.0                                                                 # 448 * 2^-3
    w[5] = w[4]
    w[5, 5] = -56.25                                                                # the next bf16 number above 56
    w[6, 1], w[6, 2] = -0.0, 3e-3
    return w.to(BF)


def random_operands(M, N, K, seed, dev, w_std=0.02):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(BF).to(dev)
    w = (torch.randn(N, K, generator=g) * w_std).to(BF).to(dev)
    return a, w


def all_codes_case():
    """N = 256, K = 64, scale 1: row n holds code n at column n % 64 and zeros elsewhere (the NaN codes replaced by 0); A has a row of
    ones and a row of -0.5 -> (a bf16 [2, 64], codes uint8 [256, 64], scale [256], expected fp32 [2, 256])"""
    codes = torch.zeros(256, 64, dtype=torch.uint8)
    n = torch.arange(256)
    byte = n.clone()
    byte[(n & 0x7f) == 0x7f] = 0
    codes[n, n % 64] = byte.to(torch.uint8)
    a = torch.stack([torch.ones(64), torch.full((64,), -0.5)]).to(BF)
    val = CODE_VALUE[byte]
    return a, codes, torch.ones(256), torch.stack([val, -0.5 * val])


def exact_case(M, N=64, K=8192, seed=0):
    """Operands whose product is exact in fp32 in ANY summation order: A integers in [-2, 2], codes 0 or |value| in [0.25, 15] (multiples
    of 2^-5, so every product is a multiple of 2^-5 below 30 and every partial sum of 8192 of them stays below 2^18 in magnitude: at most
    23 significant bits), per-row scales 2^-7 .. 2^3 -> (a bf16 [M, K], codes uint8 [N, K], scale fp32 [N], expected fp64 [M, N])"""
    g = torch.Generator().manual_seed(seed)
    ok = torch.nonzero((CODE_VALUE == 0) | ((CODE_VALUE.abs() >= 0.25) & (CODE_VALUE.abs() <= 15))).view(-1)
    codes = ok[torch.randint(0, len(ok), (N, K), generator=g)].to(torch.uint8)
    a = torch.randint(-2, 3, (M, K), generator=g).to(BF)
    scale = torch.ldexp(torch.ones(N), torch.randint(-7, 4, (N,), generator=g)).float()
    want = (a.double() @ codes.view(F8).float().double().t()) * scale.double()[None]
    return a, codes, scale, want
