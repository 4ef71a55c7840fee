"""Build-time guard on the search kernels' instances over e4m3 codes (csrc/search_common.h, ScCodeStage), read from the code
objects inside libmpv_hip.so as tests/test_isa_cpu.py does: the ten instances exist, none uses scratch, and their unified register
counts stand where DESIGN section 33 reports them relative to their bf16 twins -- the code stage is 16 registers smaller than the
bf16 stage, the finish of a tile reads 16 scales."""
import re

from test_isa_cpu import kernels  # noqa: F401  (the module-scoped fixture)

TWINS = {"16q8_stream_kernelILi0ELi4EE": "17sim_stream_kernelILi0ELi4EE", "16q8_stream_kernelILi0ELi16EE": "17sim_stream_kernelILi0ELi16EE",
         "16q8_stream_kernelILi0ELi32EE": "17sim_stream_kernelILi0ELi32EE", "16q8_stream_kernelILi1ELi1EE": "17sim_stream_kernelILi1ELi1EE",
         "16q8_target_kernel": "17sim_target_kernel", "17q8_gallery_kernelILi0ELi4EE": "18mxs_gallery_kernelILi0ELi4EE",
         "17q8_gallery_kernelILi0ELi16EE": "18mxs_gallery_kernelILi0ELi16EE", "17q8_gallery_kernelILi0ELi32EE": "18mxs_gallery_kernelILi0ELi32EE",
         "17q8_gallery_kernelILi1ELi1EE": "18mxs_gallery_kernelILi1ELi1EE", "14q8_item_kernel": "15mxs_item_kernelILi3EE"}


def test_code_instances_exist_without_scratch_beside_their_twins(kernels):  # noqa: F811
    ks, _ = kernels
    mine = {n: k for n, k in ks.items() if re.search(r"\d+q8_(stream|target|gallery|item)_kernel", n)}
    assert len(mine) == len(TWINS), sorted(mine)
    for frag, twin in TWINS.items():
        (name, k), = [(n, v) for n, v in mine.items() if frag in n]
        (_, t), = [(n, v) for n, v in ks.items() if twin in n]
        assert k["scratch"] == 0 and t["scratch"] == 0, (name, k)
        assert k["lds"] == t["lds"], (name, k, t)                      # the stage and the resident tile are the twin's (dynamic LDS)
        # the streams that walk rows (sim) shed the stage's 16 registers; the segmented max of the gallery kernel keeps 32 row
        # scores live while the scales are read, so it may sit a few registers over its twin, never a tier of 64 over it
        slack = 8 if "gallery" in frag else 0
        assert k["vgpr"] <= t["vgpr"] + slack, (name, k["vgpr"], t["vgpr"])
