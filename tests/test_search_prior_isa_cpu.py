"""Build-time guard on the search kernels with per-row priors and the bank pass (csrc/search_common.h ScPrior, csrc/search_bank.hip),
read from the code objects inside libmpv_hip.so as tests/test_isa_cpu.py does: the instances exist, none uses scratch, and every
prior stream / target instance has its twin's LDS and sits within its twin's occupancy tier (128 / 168 / 256 / 512 unified registers
= 4 / 3 / 2 / 1 waves per SIMD).  Resource figures only."""
import re

from test_isa_cpu import kernels  # noqa: F401  (the module-scoped fixture)

TWINS = {"17pri_stream_kernelILi0ELi4EE": "17sim_stream_kernelILi0ELi4EE", "17pri_stream_kernelILi0ELi16EE": "17sim_stream_kernelILi0ELi16EE",
         "17pri_stream_kernelILi0ELi32EE": "17sim_stream_kernelILi0ELi32EE", "17pri_stream_kernelILi1ELi1EE": "17sim_stream_kernelILi1ELi1EE",
         "17pri_target_kernel": "17sim_target_kernel",
         "18pri8_stream_kernelILi0ELi4EE": "16q8_stream_kernelILi0ELi4EE", "18pri8_stream_kernelILi0ELi16EE": "16q8_stream_kernelILi0ELi16EE",
         "18pri8_stream_kernelILi0ELi32EE": "16q8_stream_kernelILi0ELi32EE", "18pri8_stream_kernelILi1ELi1EE": "16q8_stream_kernelILi1ELi1EE",
         "18pri8_target_kernel": "16q8_target_kernel"}
BANK = ("15bank_lse_kernel", "16bank8_lse_kernel")


def _tier(v):
    return next(t for t in (128, 168, 256, 512) if v <= t)


def test_prior_instances_exist_without_scratch_in_their_twins_tier(kernels):  # noqa: F811
    ks, _ = kernels
    mine = {n: k for n, k in ks.items() if re.search(r"\d+pri8?_(stream|target)_kernel", n)}
    assert len(mine) == len(TWINS), sorted(mine)
    for frag, twin in TWINS.items():
        (name, k), = [(n, v) for n, v in mine.items() if frag in n]
        (_, t), = [(n, v) for n, v in ks.items() if twin in n]
        assert k["scratch"] == 0 and t["scratch"] == 0, (name, k)
        assert k["lds"] == t["lds"], (name, k, t)                      # the stage and the resident tile are the twin's (dynamic LDS)
        assert _tier(k["vgpr"]) <= _tier(t["vgpr"]), (name, k["vgpr"], t["vgpr"])


def test_bank_kernels_exist_without_scratch_at_four_waves(kernels):  # noqa: F811
    """the bank pass keeps no list: 4 waves per SIMD, like the rank stream it is modelled on"""
    ks, _ = kernels
    for frag in BANK:
        (name, k), = [(n, v) for n, v in ks.items() if frag in n]
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (name, k)
