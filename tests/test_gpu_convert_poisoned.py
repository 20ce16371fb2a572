"""GPU (-m gpu): convert_many, hue_many and colorize_many on poisoned workspace, output and staging memory (tests/poisoned_memory.py),
as test_gpu_compose_poisoned.py does for the compose calls: a handful of catalogue rows per kind, each run under the byte patterns 0x00
(control), 0x01 and 0xFF and compared with the NumPy model -- never with an unpoisoned run of the library.  The entries and tables live
in the workspace and the output is drawn poisoned: an output byte that no lane wrote or an entry field that nothing set fails here.
Every call goes through `Poison.call`, which arms the harness and asserts that the call really drew poisoned memory."""
import functools

import numpy as np
import pytest

import convert_reference as M
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
    """-> (the call on A, the model's images): host sources, so that the staging buffer is drawn too"""
    rng = np.random.default_rng(31)
    if kind == "mode":
        cases = M.mode_cases()[::6]                             # one- and two-step routes of every source, 1 x 1 included
        images, targets, sources = [c[0] for c in cases], [c[2] for c in cases], [c[1] for c in cases]
        return (lambda A: A.convert_many(images, targets, source_mode=sources)), [M.convert(a, t, s) for a, s, t in cases]
    if kind == "matrix":
        images = [M.random_image(rng, h, w, 3) for h, w in M.SIZES]
        ms = [m for t, m in M.MATRICES if t == "RGB"]
        return (lambda A: A.convert_many(images, "RGB", matrix=list(ms))), [M.convert_matrix(a, "RGB", m) for a, m in zip(images, ms)]
    if kind == "hue":
        images = [M.random_image(rng, h, w, c) for (h, w), c in zip(M.SIZES + M.SIZES[1:3], (3, 4, 1, 3, 2, 4))]
        fs = list(M.HUE_FACTORS)
        return (lambda A: A.hue_many(images, fs)), [M.hue(a, f) for a, f in zip(images, fs)]
    images = [M.random_image(rng, h, w, 1) for h, w in M.SIZES]
    kw = M.COLORIZE[4]
    return (lambda A: A.colorize_many(images, **kw)), [M.colorize(a, **kw) for a in images]


@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
@pytest.mark.parametrize("kind", ["mode", "matrix", "hue", "colorize"])
def test_row(env, kind, byte):
    A, ctx = env
    run, want = _rows(kind)
    assert len(want) >= 4
    with PM.poisoned(ctx, byte) as p:
        got = p.call(run, A, _draws=DRAWS)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g.cpu().numpy(), w), (kind, k)
        assert p.calls == 1 and p.bytes > 0
