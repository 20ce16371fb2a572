"""GPU (-m gpu): every stage of ``EdgeDetection.canny(plane, return_stages=True)`` against the OpenCV 4.x restatements of
tests/edge_reference.py, each fed the GPU's own previous stage: CLAHE and the bilateral filter equal away from half-integers, the
integer thresholds, the NMS map and the hysteresis edge map equal."""
import numpy as np
import pytest

import edge_reference as E
from test_oracle_edge_reference import PARAMS, SHAPES

pytestmark = pytest.mark.gpu

_KW = ("canny_low_ratio", "canny_high_ratio", "clahe_clip_limit", "bilateral_sigma_color", "bilateral_sigma_space", "use_L2_gradient")


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def run(A, plane, params):
    kw = dict(zip(_KW, params))
    kw["use_L2_gradient"] = bool(kw["use_L2_gradient"])
    e, st, thr = A.EdgeDetection.canny(plane, return_stages=True, **kw)
    return e, st, thr


@pytest.mark.parametrize("shape", list(SHAPES) + ["4k_2160x3840"], ids=list(SHAPES) + ["4k_2160x3840"])
def test_edge_stages_shapes(A, shape):
    H, W = SHAPES.get(shape, (2160, 3840))
    plane = E.test_plane(H, W, H * 7 + W)
    e, st, thr = run(A, plane, PARAMS["default-L2"])
    assert np.array_equal(st[0], (plane * np.float32(255)).astype(np.uint8))
    E.check_stages(st, e, thr, PARAMS["default-L2"], label=shape)


@pytest.mark.parametrize("name", list(PARAMS), ids=list(PARAMS))
def test_edge_stages_hyper_parameters(A, name):
    plane = E.test_plane(203, 333, 11)
    e, st, thr = run(A, plane, PARAMS[name])
    E.check_stages(st, e, thr, PARAMS[name], label=name)
    assert (st[4] == 2).any() and e.sum() > 0
