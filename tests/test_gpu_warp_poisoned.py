"""GPU (-m gpu): transform_many, rotate_many and transpose_many on poisoned workspace, output and staging memory
(tests/poisoned_memory.py), as test_gpu_window_filter_poisoned.py does for the window filters: a handful of rows of test_gpu_warp.py,
each run under the byte patterns 0x00 (control), 0x01 and 0xFF and compared with the NumPy model -- never with an unpoisoned run of the
library.  An outside pixel must come from the fill and never from what the allocation held.  Every call goes through `Poison.call`,
which arms the harness and asserts that the call really drew poisoned memory."""
import functools

import numpy as np
import pytest

import poisoned_memory as PM
import warp_reference as M

pytestmark = pytest.mark.gpu
PATTERN_IDS = [f"0x{b:02X}" for b in PM.PATTERNS]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as A
    from adaptive_edge_aware_jpeg_amd import _lib
    return A, _lib.get_context()


@functools.lru_cache(maxsize=None)
def _rows(kind):
    import test_gpu_warp as TW
    if kind == "mixed":
        cases = TW._mixed(12)
    elif kind == "outside":                    # mostly outside pixels, with and without a fill colour, every path
        a = M.image(9, 6, 3, 1)
        cases = [TW.tf(a, (40, 33), m, d, f, fill) for f in TW.FILTERS for fill in (None, (3, 141, 59))
                 for m, d in ((M.AFFINE, (1.0, 0.2, -12.0, -0.2, 1.0, -9.0)), (M.AFFINE, (0.5, 0, -4.0, 0, 0.5, -4.0)),
                              (M.PERSPECTIVE, (1, 0, -1.5, 0, 1, -0.5, 0, -2)), (M.QUAD, (-9.0, -9.0, -8.0, 20.0, 17.0, 19.0, 18.0, -7.0)))]
    else:
        cases = [c for c in M.catalogue() if c[0] == kind and min(c[1].shape[:2]) < 12]
    return cases, [M.model(c) for c in cases]


@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("kind", ["transform", "rotate", "transpose", "outside", "mixed"])
def test_row(env, kind, byte):
    import test_gpu_warp as TW
    A, ctx = env
    cases, want = _rows(kind)
    assert len(cases) >= 12
    fn = {"rotate": A.rotate_many, "transpose": A.transpose_many}.get(kind, A.transform_many)
    with PM.poisoned(ctx, byte) as p:
        def call(images, **kw):
            return p.call(fn, images, _draws=("workspace_fills", "empties", "pinned_fills"), **kw)
        got = TW.run(type("Through", (), {"transform_many": staticmethod(call), "rotate_many": staticmethod(call), "transpose_many": staticmethod(call)}), cases)
        for c, g, w in zip(cases, got, want):
            assert np.array_equal(g.cpu().numpy(), w), (c[1].shape, c[2])
        assert p.calls >= 1 and p.bytes > 0
