"""GPU (-m gpu): filter_many with Color3DLUT tables on poisoned workspace, output and staging memory (tests/poisoned_memory.py), as
test_gpu_window_filter_poisoned.py does for the window filters: one row of the small catalogue cases, one of the ramps, and a mixed row
in which the blurs' entry, the window entry and the tables' entry write one output, each run under the byte patterns 0x00 (control),
0x01 and 0xFF and compared with the NumPy models -- never with an unpoisoned run of the library.  Every call goes through
`Poison.call`, which arms the harness and asserts that the call really drew poisoned memory."""
import functools

import numpy as np
import pytest

import lut3d_reference as M
import poisoned_memory as PM

pytestmark = pytest.mark.gpu
PATTERN_IDS = [f"0x{b:02X}" for b in PM.PATTERNS]
SMALL = M.SHAPES                             # up to (17, 13): every tail of a lane's run, bases of every alignment


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as A
    from adaptive_edge_aware_jpeg_amd import _lib
    return A, _lib.get_context()


@functools.lru_cache(maxsize=None)
def _cases(kind):
    cases = [(a, f) for a, f in M.catalogue() if (a.shape[:2] in SMALL) == (kind == "small")]
    return cases, [M.model(a, f) for a, f in cases]


@functools.lru_cache(maxsize=None)
def _mixed():
    import test_gpu_lut3d as TL
    cases = TL._mixed(15)
    return cases, [TL._mixed_model(a, f) for a, f in cases]


def _run(A, p, cases, want):
    import test_gpu_lut3d as TL
    got = p.call(A.filter_many, [a for a, _ in cases], TL._mixed_filters(A, cases), _draws=("workspace_fills", "empties", "pinned_fills"))
    for (a, f), g, w in zip(cases, got, want):
        assert g.shape == w.shape and np.array_equal(g.cpu().numpy(), w), (a.shape, f)


@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("kind", ["small", "ramps", "mixed"])
def test_row(env, kind, byte):
    A, ctx = env
    cases, want = _mixed() if kind == "mixed" else _cases(kind)
    assert len(cases) >= 11 and (kind != "mixed" or {isinstance(f, M.Lut) for _, f in cases} == {True, False})
    assert kind == "mixed" or {(a.shape[2], f.channels, f.bands(a.shape[2])) for a, f in cases} == set(M.COMBOS)
    with PM.poisoned(ctx, byte) as p:
        _run(A, p, cases, want)
        assert p.calls >= 1 and p.bytes > 0
