"""The LoRA kernels of csrc/lora.hip against the fp64 reference, element by element (tests/lora_cases.py: cases, runners, gates):
every rank, both layouts of w / g, pitched leading dimensions, scale 1 and 1.5, sentinel guards, the row independence of down and
up_add, and wgrad twice for the same bits."""
import pytest
import torch

import lora_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(dev):
    from youku_mplug_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("c", LC.DOWN, ids=LC.case_id)
def test_down(ops, dev, c):
    LC.run_down(ops, c, dev)


@pytest.mark.parametrize("c", LC.UP_ADD, ids=LC.case_id)
def test_up_add(ops, dev, c):
    LC.run_up_add(ops, c, dev)


@pytest.mark.parametrize("c", LC.WGRAD, ids=LC.case_id)
def test_wgrad(ops, dev, c):
    LC.run_wgrad(ops, c, dev)


def test_refusals(ops, dev):
    from youku_mplug_amd._lib import MpvError
    x = torch.zeros((8, 64), dtype=torch.bfloat16, device=dev)
    w = torch.zeros((64, 64), dtype=torch.bfloat16, device=dev)
    with pytest.raises(MpvError):
        ops.lora_down(x, w, 8, 64, 12, w_rank_major=True)             # rank
    with pytest.raises(MpvError):
        ops.lora_down(x, w, 8, 60, 8, w_rank_major=True)              # C % 8
    with pytest.raises(MpvError):
        ops.lora_down(x[:, 4:], w, 8, 56, 8, w_rank_major=True)       # alignment
