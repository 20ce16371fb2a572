"""GPU (-m gpu): adjust_many and histogram_many on poisoned workspace, output and staging memory (tests/poisoned_memory.py), as
test_gpu_warp_poisoned.py does for the warps: a handful of rows of the catalogue, each run under the byte patterns 0x00 (control), 0x01
and 0xFF and compared with the NumPy model -- never with an unpoisoned run of the library.  The histograms, the tables and the
intermediate planes all live in the workspace: a histogram that the call did not zero, a table byte that nothing wrote or an
intermediate pixel read beyond what was written fails here.  Every call goes through `Poison.call`, which arms the harness and asserts
that the call really drew poisoned memory."""
import functools

import numpy as np
import pytest

import adjust_reference as M
import poisoned_memory as PM

pytestmark = pytest.mark.gpu
PATTERN_IDS = [f"0x{b:02X}" for b in PM.PATTERNS]
DRAWS = ("workspace_fills", "empties", "pinned_fills")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as A
    from adaptive_edge_aware_jpeg_amd import _lib
    return A, _lib.get_context()


def _names(case):
    return tuple(op[0] for op in M.chain_of(case[1]))


@functools.lru_cache(maxsize=None)
def _rows(kind):
    cat = M.catalogue()
    if kind == "statistics":                    # one statistics op
        cases = [c for c in cat if len(_names(c)) == 1 and _names(c)[0] in M.STATISTICS][::5]
    elif kind == "two_statistics":              # two histogram passes in one segment
        cases = [c for c in cat if sum(n in M.STATISTICS for n in _names(c)) >= 2 and "sharpness" not in _names(c)]
    elif kind == "sharpness_cut":               # a Sharpness that is not first: an intermediate plane in the workspace
        cases = [c for c in cat if "sharpness" in _names(c)[1:]]
    else:
        cases = cat[::40]
    return cases, [M.histogram(c[0]) if kind == "histogram" else M.model(c) for c in cases]


@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("kind", ["statistics", "two_statistics", "sharpness_cut", "histogram"])
def test_row(env, kind, byte):
    A, ctx = env
    cases, want = _rows(kind)
    assert len(cases) >= 4
    with PM.poisoned(ctx, byte) as p:
        if kind == "histogram":
            got = p.call(A.histogram_many, [c[0] for c in cases], _draws=DRAWS)
        else:
            got = p.call(A.adjust_many, [c[0] for c in cases], [M.library_ops(A, c[1]) for c in cases], _draws=DRAWS)
        for c, g, w in zip(cases, got, want):
            assert np.array_equal(g.cpu().numpy(), w), (c[0].shape, str(c[1])[:100])
        assert p.calls == 1 and p.bytes > 0
