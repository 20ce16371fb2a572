"""CPU: tests/poisoned_memory.py itself -- fill_bytes on host tensors of every width at odd sizes, and the counters and the arm rule of
poisoned() on a stand-in context (no GPU, no library)."""
import numpy as np
import pytest
import torch

import poisoned_memory as PM

DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32, torch.float64]


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
@pytest.mark.parametrize("n", [0, 1, 3, 7, 13, 1001])
@pytest.mark.parametrize("byte", PM.PATTERNS)
def test_fill_bytes_sets_every_byte(dtype, n, byte):
    t = torch.arange(n, dtype=torch.float64).to(dtype) + 5
    assert PM.fill_bytes(t, byte) is t
    raw = t.numpy().view(np.uint8)
    assert raw.size == n * t.element_size() and (raw == byte).all()
    if n and byte == 0x01:
        want = {torch.uint8: 1, torch.int32: 0x01010101, torch.int64: 0x0101010101010101}.get(dtype)
        if want is not None:
            assert int(t[0]) == want
        else:
            assert 0 < float(t[0]) < 1e-30                    # a tiny positive float, not a NaN
    if n and byte == 0xFF:
        assert bool(torch.isnan(t[0])) if dtype.is_floating_point else int(t[0]) == (255 if dtype == torch.uint8 else -1)


def test_fill_bytes_shapes_slices_and_refusals():
    t = torch.zeros((3, 5, 7), dtype=torch.int32)
    PM.fill_bytes(t[1], 0xFF)                                 # a contiguous slice: only its own bytes
    assert (t[1] == -1).all() and (t[0] == 0).all() and (t[2] == 0).all()
    odd = torch.zeros(13, dtype=torch.uint8)
    PM.fill_bytes(odd[1:12], 0x01)                            # 11 bytes at an odd offset: no 4-byte shortcut may round it
    assert odd.tolist() == [0] + [1] * 11 + [0]
    with pytest.raises(ValueError):
        PM.fill_bytes(torch.zeros((4, 4))[:, 1], 1)           # strided: it does not own the bytes between its elements
    with pytest.raises(ValueError):
        PM.fill_bytes(odd, 256)


class _Ctx:
    """what poisoned() needs of a Context: empty / workspace / pinned with the reuse rule of _lib.Context"""

    def __init__(self):
        self._ws = None
        self._pinned = None

    def empty(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype)

    def workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.zeros(int(nbytes), dtype=torch.uint8)
        return self._ws

    def pinned(self, nbytes):
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.zeros(int(nbytes), dtype=torch.uint8)
        return self._pinned


def test_counters_arming_and_restore():
    ctx = _Ctx()
    plain = (ctx.empty.__func__, ctx.workspace.__func__, ctx.pinned.__func__)
    with PM.poisoned(ctx, 0x01) as p:
        e = ctx.empty((5,), torch.int32)
        assert (e == 0x01010101).all() and p.snapshot() == dict(empties=1, workspace_fills=0, pinned_fills=0, bytes=20)
        w = ctx.workspace(100)                                # first allocation: filled although nobody armed
        assert (w == 1).all() and p.workspace_fills == 1 and p.bytes == 120
        w[:50] = 9
        assert ctx.workspace(64) is w and (w[:50] == 9).all() and p.workspace_fills == 1      # not armed: state kept in mid-operation
        p.arm()
        assert (ctx.workspace(64) == 1).all() and p.workspace_fills == 2 and p.bytes == 220   # armed: the WHOLE buffer, not the 64 asked for
        w[:] = 9
        assert ctx.workspace(10) is w and (w == 9).all()      # one fill per arm
        w2 = ctx.workspace(300)                               # reallocation: filled over its whole length
        assert w2 is not w and w2.numel() == 300 and (w2 == 1).all() and p.workspace_fills == 3
        p.arm()
        h = ctx.pinned(40)
        assert (h == 1).all() and p.pinned_fills == 1
        assert (ctx.workspace(1) == 1).all() and p.workspace_fills == 4                       # pinned() does not use up the workspace's arm
        before = p.snapshot()
        with p.suspended():                                   # the plain methods for a while: nothing filled, counted or disarmed
            p.arm()
            w2[:] = 9
            assert ctx.workspace(8) is w2 and (w2 == 9).all() and (ctx.empty((3,), torch.int32) == 0).all() and (ctx.pinned(8)[:8] == 1).all()
            assert ctx.workspace(400).numel() == 400 and (ctx.workspace(400) == 0).all()      # a reallocation inside the block stays as it came
        assert p.snapshot() == before and p._armed_ws and p._armed_pinned
        got = p.call(lambda: (ctx.workspace(8), ctx.empty((1,), torch.uint8)))
        assert p.calls == 1 and (got[0] == 1).all()
        with pytest.raises(AssertionError, match="workspace_fills"):
            p.call(lambda: ctx.empty((1,), torch.uint8))      # an entry that never asks for the workspace is found out
    assert (ctx.empty.__func__, ctx.workspace.__func__, ctx.pinned.__func__) == plain and "empty" not in vars(ctx)
    assert (ctx.empty((2,), torch.int32) == 0).all()


def test_restored_after_an_exception():
    ctx = _Ctx()
    with pytest.raises(RuntimeError):
        with PM.poisoned(ctx, 0xFF):
            raise RuntimeError("the call under test failed")
    assert "workspace" not in vars(ctx) and (ctx.workspace(4) == 0).all()
