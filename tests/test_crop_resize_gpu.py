"""onepose_crop_resize on the GPU against the all-integer oracle
(tests/detector_oracle.py crop_resize): the crop must equal it exactly, crop_f32 must be
crop_u8 / 255 exactly, K_crop within 1e-12 relative (the same float64 operations; the oracle
multiplies 3x3 matrices, whose zero terms may be fused differently)."""
import numpy as np
import pytest
import torch

import detector_oracle as D
from detector_cases import ramp
from onepose_amd import detector

pytestmark = pytest.mark.gpu

BOXES = {
    "inside": (8, 4, 24, 20),
    "over_left": (-5, 3, 11, 19),
    "over_top": (4, -6, 20, 10),
    "over_right": (45, 10, 65, 30),
    "over_bottom": (10, 30, 30, 50),
    "over_all": (-3, -2, 70, 66),
    "outside": (100, 100, 120, 130),
    "wide": (5, 5, 25, 15),
    "tall": (5, 5, 15, 35),
    "one_column": (7, 3, 8, 20),
    "no_width": (5, 5, 5, 9),
    "no_height": (5, 9, 8, 9),
    "inverted": (9, 5, 3, 8),
    "far": (-40000, 3, 20, 19),          # outside warpAffine's short maps: status 2
    "far_x1": (3, 3, 32768, 19),
}
STATUS = {"no_width": 1, "no_height": 1, "inverted": 1, "far": 2, "far_x1": 2}
K = np.array([[500.0, 0.25, 28.5], [0, 510.0, 20.25], [0, 0, 1]])


@pytest.mark.parametrize("crop_size", [16, 512])
@pytest.mark.parametrize("hw", [(40, 56), (64, 64)])
def test_crop_equals_the_oracle(device, hw, crop_size):
    img = ramp(*hw)
    img_d = torch.from_numpy(img).to(device)
    K_d = torch.from_numpy(K).to(device)
    for name, box in BOXES.items():
        ref_u8, ref_K, ref_st = D.crop_resize(img, box, K, crop_size)
        out = detector.crop_resize(img_d, torch.tensor(box, dtype=torch.int32, device=device), K_d,
                                   crop_size)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert int(got["crop_status"][0]) == ref_st == STATUS.get(name, 0), name
        assert np.array_equal(got["crop_u8"], ref_u8), name
        assert np.array_equal(got["crop_f32"], ref_u8.astype(np.float32) / 255), name
        np.testing.assert_allclose(got["K_crop"], ref_K, rtol=1e-12, atol=0, err_msg=name)
        if name == "outside" or ref_st:
            assert not got["crop_u8"].any(), name
        elif name != "one_column":
            assert got["crop_u8"].any(), name
    # without K: no K_crop, the same image
    out = detector.crop_resize(img_d, torch.tensor(BOXES["wide"], dtype=torch.int32,
                                                   device=device), None, crop_size)
    assert "K_crop" not in out
    assert np.array_equal(out["crop_u8"].cpu().numpy(), D.crop_resize(img, BOXES["wide"], None,
                                                                      crop_size)[0])
