"""CPU: the oracle's CLAHE, bilateral filter, Canny NMS and hysteresis against the independent restatements of
tests/edge_reference.py (written from OpenCV 4.x clahe.cpp, bilateral_filter.dispatch.cpp and canny.cpp), each stage fed the
oracle's previous stage.  Integer stages must be equal; CLAHE and bilateral equal except within 1e-3 of a half-integer."""
import numpy as np
import pytest

import edge_reference as E

DEFAULT = (0.10, 0.30, 0.75, 75.0, 75.0, 1)
# test_canny_hyper_parameters' sets, in aej_canny_params order
PARAMS = {
    "default-L2": DEFAULT,
    "ratios": (0.20, 0.55, 0.75, 75.0, 75.0, 1),
    "clip2": (0.10, 0.30, 2.0, 75.0, 75.0, 1), "clip40": (0.10, 0.30, 40.0, 75.0, 75.0, 1), "noclip": (0.10, 0.30, 0.0, 75.0, 75.0, 1),
    "sigmas": (0.10, 0.30, 0.75, 20.0, 3.5, 1),
    "L1": (0.10, 0.30, 0.75, 75.0, 75.0, 0),
    "L1-lo_gt_hi-sigma0": (0.6, 0.4, 1.5, 150.0, 0.0, 0),
}
# (H, W): H % 4 == 0 with W ragged and the reverse (the one-sided padding in each orientation), both ragged, below 4 on a side,
# tall and wide strips
SHAPES = {"pad_cols_only_96x131": (96, 131), "pad_rows_only_97x132": (97, 132), "pad_both_97x131": (97, 131), "exact_64x64": (64, 64),
          "below4_3x50": (3, 50), "tiny_2x2": (2, 2), "tall_400x7": (400, 7), "wide_6x500": (6, 500)}


@pytest.mark.parametrize("shape", list(SHAPES), ids=list(SHAPES))
def test_oracle_edge_stages_shapes(oracle, shape):
    H, W = SHAPES[shape]
    plane = E.test_plane(H, W, H * 7 + W)
    edge, stages, pct = oracle.edge_pipeline(plane, return_stages=True)
    E.check_stages(stages, edge, None, DEFAULT, label=shape)
    assert pct == E.percentile_thresholds(stages[3])
    _, nms = oracle.canny(stages[3], *pct, return_nms=True)
    assert np.array_equal(nms, E.canny_nms(stages[3], *E.canny_thresholds(*pct)))


@pytest.mark.parametrize("name", list(PARAMS), ids=list(PARAMS))
def test_oracle_edge_stages_hyper_parameters(oracle, name):
    plane = E.test_plane(203, 333, 11)
    edge, stages, _ = oracle.edge_pipeline(plane, return_stages=True, params=PARAMS[name])
    E.check_stages(stages, edge, None, PARAMS[name], label=name)


def test_clahe_redistribution_residual_step():
    """the test plane's plateau tile clips and leaves a residual whose step 256 / residual exceeds 1"""
    src = (E.test_plane(96, 131, 3) * 255).astype(np.uint8)
    H, W = src.shape
    ys, xs = E.reflect101(np.arange(H + 4 - H % 4 if H % 4 else H + 4), H), E.reflect101(np.arange(W + 4 - W % 4), W)
    ext = src[ys[:, None], xs[None, :]]
    th, tw = ext.shape[0] // 4, ext.shape[1] // 4
    clip = max(int(0.75 * th * tw / 256), 1)
    tile = ext[:th, :tw]
    clipped = np.maximum(np.bincount(tile.ravel(), minlength=256) - clip, 0).sum()
    assert 0 < clipped % 256 < 128


def test_canny_on_crafted_bytes(oracle):
    """NMS and hysteresis on bytes fed straight to the oracle's Canny: plateaus and ramps (the strict / non-strict ties), ramps at
    22 and 68 degrees, weak chains joined only diagonally with one strong end, chains that touch the border"""
    H, W = 120, 150
    y, x = np.mgrid[0:H, 0:W]
    img = np.full((H, W), 60, np.int64)
    img[10:40, 10:60] = 160                                  # plateau: equal magnitudes along its edges
    img += np.where(x > 100, (x - 100) * 2, 0)               # ramp: equal magnitudes across
    for ang, c in ((22.0, 30), (68.0, 90)):
        t = x * np.cos(np.deg2rad(ang)) + y * np.sin(np.deg2rad(ang))
        img += 25 * ((t // 1) % 40 < 3) * (y > c)
    for k in range(40):                                      # diagonal staircase of faint steps, one strong end
        img[60 + k, 20 + k] += 18
    img[60, 20] += 120
    img[:, 0] += 70
    img[0, :] += 70
    img = np.clip(img, 0, 255).astype(np.uint8)
    for lo, hi in ((20.0, 60.0), (60.0, 20.0), (5.0, 300.0)):
        edge, nms = oracle.canny(img, lo, hi, return_nms=True)
        ref = E.canny_nms(img, *E.canny_thresholds(lo, hi))
        assert np.array_equal(nms, ref), (lo, hi, np.argwhere(nms != ref)[:5].tolist())
        assert np.array_equal(edge == 255, E.hysteresis(ref) == 1)
        assert (ref == 2).any() and (ref == 0).any()
