"""GPU (-m gpu): the compose calls on poisoned workspace, output and staging memory (tests/poisoned_memory.py), as
test_gpu_adjust_poisoned.py does for adjust_many: a handful of rows of the catalogue, each run under the byte patterns 0x00 (control),
0x01 and 0xFF and compared with the NumPy model -- never with an unpoisoned run of the library.  The entries live in the workspace and
the output is drawn poisoned: an output byte that no lane wrote -- outside the region, or of an element whose region lies wholly outside
its base -- or an entry field that nothing set fails here.  Every call goes through `Poison.call`, which arms the harness and asserts
that the call really drew poisoned memory."""
import functools

import numpy as np
import pytest

import compose_reference as M
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


@functools.lru_cache(maxsize=None)
def _rows(kind):
    cat = M.catalogue()
    if kind == "outside":                       # the region lies wholly outside the base: the output is still written everywhere
        cases = [c for c in cat if c["kind"] == "paste" and str(c["geometry"]).startswith("outside")]
    elif kind == "paste":
        cases = [c for c in cat if c["kind"] == "paste" and not str(c["geometry"]).startswith("outside")][::9]
    else:
        cases = [c for c in cat if c["kind"] == kind]
        cases = cases[::max(1, len(cases) // 6)]
    return cases, [M.model(c) for c in cases]


@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("kind", ["outside", "paste", "alpha_composite", "blend", "composite", "chop"])
def test_row(env, kind, byte):
    A, ctx = env
    cases, want = _rows(kind)
    assert len(cases) >= 4
    if kind == "outside":
        assert all(np.array_equal(w, c["base"]) for c, w in zip(cases, want))
    with PM.poisoned(ctx, byte) as p:
        got = p.call(M.call, A, cases, _draws=DRAWS)
        for c, g, w in zip(cases, got, want):
            assert np.array_equal(g.cpu().numpy(), w), (M.signature(c), c["geometry"])
        assert p.calls == 1 and p.bytes > 0
