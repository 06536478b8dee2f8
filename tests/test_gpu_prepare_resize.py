"""scsfm_hip.prepare.resize_u8 on the GPU equals PIL's Image.resize(BILINEAR) byte for byte, launch after launch."""
import numpy as np
import pytest
import torch

from _prepare_data_check import RESIZE_CASES, pil_resize, resize_inputs
from scsfm_hip import prepare

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(RESIZE_CASES))
def test_resize_equals_pil(name):
    images, h, w, keep = resize_inputs(name)
    staged = torch.from_numpy(images).cuda()
    first = prepare.resize_u8(staged, h, w, keep)
    second = prepare.resize_u8(staged, h, w, keep)
    torch.cuda.synchronize()
    assert first.shape == (len(images), keep or h, w, images.shape[3]) and first.dtype == torch.uint8
    assert np.array_equal(first.cpu().numpy(), pil_resize(images, h, w, keep))
    assert torch.equal(first, second)


def test_host_tensors_are_refused():
    with pytest.raises(RuntimeError):
        prepare.resize_u8(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 2, 2)
