"""GPU (-m gpu): png_decode_many(interlaced=True, depth16=True) on poisoned workspace, output and staging memory
(tests/poisoned_memory.py), as test_gpu_warp_poisoned.py does for the warps: the mixed call and the call of all 81 sizes of
test_gpu_png_adam7.py, each under the byte patterns 0x00 (control), 0x01 and 0xFF and compared with the reference -- never with an
unpoisoned run of the library.  The pass images and the per-pass status words in the workspace are the places a stale byte could leak
from: a pass without pixels writes neither and must not be read.  Every call goes through `Poison.call`, which arms the harness and
asserts that the call really drew poisoned memory."""
import numpy as np
import pytest

import png_adam7_reference as Z
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


def _calls():
    names, modes = Z.mixed()
    yield "mixed", names, modes
    for ct, depth in Z.SMALL_KINDS:
        names = [f"s{w}x{h}_ct{ct}d{depth}_i" for h in range(1, 10) for w in range(1, 10)]
        yield f"sizes ct{ct}d{depth}", names, [("RGB", "auto")[i % 2] for i in range(len(names))]


@pytest.mark.parametrize("byte", PM.PATTERNS, ids=PATTERN_IDS)
def test_mixed_and_all_sizes(env, byte):
    A, ctx = env
    with PM.poisoned(ctx, byte) as p:
        for what, names, modes in _calls():
            files = [Z.lookup(n) for n in names]
            for inflate in ("gpu", "host"):
                got = p.call(A.png_decode_many, files, mode=modes, inflate=inflate, interlaced=True, depth16=True, _draws=DRAWS)
                for n, m, g in zip(names, modes, got):
                    want = Z.lookup_expected(n, m)
                    g = g.cpu().numpy()
                    assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want), (what, inflate, n, m)
        assert p.calls == 10 and p.bytes > 0
