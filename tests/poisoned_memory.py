"""Poisoned device memory for the library's Python layer: control what every byte held BEFORE a call.

Every device byte the Python layer hands to a kernel comes from `Context.empty()` (outputs, status words, histograms, staging) or
from `Context.workspace()` (one buffer per context, reused by every subsystem); `Context.pinned()` is the reused host staging buffer.
`poisoned(ctx, byte)` replaces those three methods on ONE context instance so that what they return is filled with `byte`:

  * `empty`      every tensor it returns;
  * `workspace`  the whole reused buffer on the first call after `arm()`, and whenever it had to reallocate;
  * `pinned`     the same rule as `workspace`.

The test calls `arm()` before each public call.  Arming once per public call is deliberate: begin/end pairs and the sweep ask for
the workspace again in mid-operation and legitimately keep state there.  The counters say whether the entry under test drew poisoned
memory at all, so a path that bypasses the helpers fails its test instead of passing untested.

Patterns: 0x00 is the control (the harness itself changes nothing); 0x01 makes every int32 counter 16843009 and every float about
2.4e-38 (expected symptom: a wrong answer, not a wild address); 0xFF makes ints -1, floats NaN and flags set.
"""
import contextlib

import torch

PATTERNS = (0x00, 0x01, 0xFF)


def fill_bytes(tensor, byte):
    """Set every byte of `tensor` (any dtype, any size, device or pinned host; contiguous) to `byte`.  Returns the tensor."""
    if not 0 <= int(byte) <= 255:
        raise ValueError(f"byte {byte!r} outside 0..255")
    if not tensor.is_contiguous():
        raise ValueError("fill_bytes needs a contiguous tensor: a strided view does not own every byte between its elements")
    if tensor.numel():
        tensor.view(-1).view(torch.uint8).fill_(int(byte))
    return tensor


class Poison:
    """Counters and the arm switch of one `poisoned()` block."""

    def __init__(self, byte):
        self.byte = int(byte)
        self.empties = 0                 # tensors from ctx.empty() that were filled
        self.workspace_fills = 0         # whole-buffer fills of ctx.workspace()
        self.pinned_fills = 0            # whole-buffer fills of ctx.pinned()
        self.bytes = 0                   # bytes filled, all three together
        self.calls = 0                   # public calls made through call()
        self._armed_ws = False
        self._armed_pinned = False
        self._suspended = False

    @contextlib.contextmanager
    def suspended(self):
        """Inside this block the three methods hand out memory as the plain Context does: nothing is filled, counted or disarmed.
        For the one call a test needs WITHOUT the harness (what an entry says on clean memory) while the harness stays installed."""
        was, self._suspended = self._suspended, True
        try:
            yield self
        finally:
            self._suspended = was

    def arm(self):
        """Before each public call: its first workspace() and its first pinned() poison the whole reused buffer."""
        self._armed_ws = True
        self._armed_pinned = True

    def snapshot(self):
        return {"empties": self.empties, "workspace_fills": self.workspace_fills, "pinned_fills": self.pinned_fills, "bytes": self.bytes}

    def call(self, fn, *args, _draws=("workspace_fills", "empties"), **kwargs):
        """One public call: arm, call, and require that it drew poisoned memory from every source named in `_draws` -- an entry that
        bypasses the helpers fails here instead of passing untested."""
        self.arm()
        before = self.snapshot()
        out = fn(*args, **kwargs)
        after = self.snapshot()
        for k in _draws:
            assert after[k] > before[k], f"{getattr(fn, '__qualname__', fn)}: no poisoned memory drawn through {k} ({before} -> {after})"
        assert after["bytes"] > before["bytes"]
        self.calls += 1
        return out

    def _fill(self, t):
        fill_bytes(t, self.byte)
        self.bytes += t.numel() * t.element_size()
        return t


@contextlib.contextmanager
def poisoned(ctx, byte):
    """Replace empty / workspace / pinned on this one Context instance; restored on exit.  Yields the `Poison` (arm(), counters)."""
    p = Poison(byte)
    real_empty, real_workspace, real_pinned = ctx.empty, ctx.workspace, ctx.pinned
    had = {name: name in vars(ctx) for name in ("empty", "workspace", "pinned")}

    def empty(shape, dtype):
        t = real_empty(shape, dtype)
        if p._suspended:
            return t
        p.empties += 1
        return p._fill(t)

    def workspace(nbytes):
        before = getattr(ctx, "_ws", None)
        t = real_workspace(nbytes)
        if not p._suspended and (p._armed_ws or t is not before):
            p._armed_ws = False
            p.workspace_fills += 1
            p._fill(t)
        return t

    def pinned(nbytes):
        before = getattr(ctx, "_pinned", None)
        t = real_pinned(nbytes)
        if not p._suspended and (p._armed_pinned or t is not before):
            p._armed_pinned = False
            p.pinned_fills += 1
            # the previous call's device-to-host copies into this buffer must be over before the host writes it
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            p._fill(t)
        return t

    ctx.empty, ctx.workspace, ctx.pinned = empty, workspace, pinned
    try:
        yield p
    finally:
        for name, real in (("empty", real_empty), ("workspace", real_workspace), ("pinned", real_pinned)):
            if had[name]:
                setattr(ctx, name, real)
            else:
                delattr(ctx, name)
