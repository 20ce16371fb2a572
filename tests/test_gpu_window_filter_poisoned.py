"""GPU (-m gpu): filter_many with the window filters on poisoned workspace, output and staging memory (tests/poisoned_memory.py), as
test_gpu_poisoned_memory.py does for the other entries: one row per kind at the smallest catalogue cases, and a mixed row in which the
blurs' entry and the window entry write one output, each run under the byte patterns 0x00 (control), 0x01 and 0xFF and compared with
the NumPy models -- never with an unpoisoned run of the library.  Every call goes through `Poison.call`, which arms the harness and
asserts that the call really drew poisoned memory."""
import functools

import numpy as np
import pytest

import filter_reference as B
import poisoned_memory as PM
import window_filter_reference as M

pytestmark = pytest.mark.gpu
PATTERN_IDS = [f"0x{b:02X}" for b in PM.PATTERNS]
SMALL = M.SHAPES[:10]                        # up to (6, 5): every border case of every kind


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as A
    from adaptive_edge_aware_jpeg_amd import _lib
    return A, _lib.get_context()


@functools.lru_cache(maxsize=None)
def _cases(kind):
    pick = {"Kernel": lambda f: hasattr(f, "filterargs"), "Rank": lambda f: hasattr(f, "rank"), "Mode": lambda f: f.name == "Mode"}[kind]
    cases = [(a, f) for a, f in M.catalogue() if a.shape[:2] in SMALL and pick(f)]
    return cases, [M.model(a, f) for a, f in cases]


@functools.lru_cache(maxsize=None)
def _mixed():
    import test_gpu_window_filter as TW
    cases = TW._mixed(12)
    return cases, [TW._model(a, f) for a, f in cases]


def _run(A, p, cases, want):
    got = p.call(A.filter_many, [a for a, _ in cases], [f for _, f in cases], _draws=("workspace_fills", "empties", "pinned_fills"))
    for (a, f), g, w in zip(cases, got, want):
        assert np.array_equal(g.cpu().numpy(), w), (a.shape, f)


@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("kind", ["Kernel", "Rank", "Mode", "mixed"])
def test_row(env, kind, byte):
    A, ctx = env
    cases, want = _mixed() if kind == "mixed" else _cases(kind)
    assert len(cases) >= 12 and (kind != "mixed" or {getattr(f, "name", "") in B.PASSES for _, f in cases} == {True, False})
    with PM.poisoned(ctx, byte) as p:
        _run(A, p, cases, want)
        assert p.calls >= 1 and p.bytes > 0
