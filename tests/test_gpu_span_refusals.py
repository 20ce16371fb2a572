"""GPU: the C entries aej_filter_batch, aej_window_batch and aej_resample_batch themselves, on one 4 x 3 RGB image each: a correct call
writes exactly the image's bytes, and every refusal of the shared span check (csrc/aej_spans.h, tests/test_spans_host.py has its
arithmetic) comes with its code and its whole text before any kernel runs, the output untouched.  aej_warp_batch, aej_adjust_batch
and aej_compose_batch have the same test beside their own (test_gpu_warp.py, test_gpu_adjust.py, test_gpu_compose.py)."""
import ctypes

import numpy as np
import pytest

import filter_reference as F
import resample_reference as R
import window_filter_reference as W

pytestmark = pytest.mark.gpu
GUARD = 16


def _filter(L):
    d = (L.FilterDesc * 1)()
    d[0].kind, d[0].xradius, d[0].yradius = 0, 1.0, 1.0      # AEJ_FILTER_BOX, radius 1
    d[0].width, d[0].height, d[0].channels = 4, 3, 3
    return d, (0,), lambda a: F.model(a, F.Spec("BoxBlur", 1))      # (0: AEJ_FILTER_AUTO)


def _window(L):
    d = (L.WindowDesc * 1)()
    d[0].kind, d[0].size, d[0].rank = 1, 3, 4                 # AEJ_WINDOW_RANK: the median of 3 x 3
    d[0].width, d[0].height, d[0].channels = 4, 3, 3
    return d, (), lambda a: W.model(a, W.Rank(3, 4))


def _resample(L):
    d = (L.ResampleDesc * 1)()
    d[0].src_w, d[0].src_h, d[0].dst_w, d[0].dst_h = 4, 3, 2, 2
    d[0].box[:] = (0, 0, 4, 3)
    d[0].filter, d[0].reduce_x, d[0].reduce_y = 2, 1, 1       # bilinear, no reduce
    return d, (), lambda a: R.resize(a, (2, 2), "bilinear")


@pytest.mark.parametrize("entry,make", [("filter", _filter), ("window", _window), ("resample", _resample)])
def test_c_entry_refusals_and_untouched_bytes(entry, make):
    import torch
    assert torch.cuda.is_available()
    from adaptive_edge_aware_jpeg_amd import _lib as L
    ctx = L.get_context(0)
    lib = ctx.lib
    fn = f"aej_{entry}_batch"
    a = np.random.default_rng(5).integers(0, 256, (3, 4, 3), dtype=np.uint8)
    d, mid, model = make(L)
    want = model(a)
    n, m = a.size, want.size
    buf = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")      # the source, and room behind it for an output that meets it
    buf[:n] = torch.from_numpy(a).cuda().reshape(-1)
    d[0].src_offset, d[0].dst_offset = 0, GUARD
    dst = torch.full((m + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    nws = int(getattr(lib, f"aej_{entry}_workspace_bytes")(ctx.handle, ctypes.addressof(d), 1, *mid))
    assert nws > 0
    ws = ctx.workspace(max(nws, 256))

    def call(count, src_ptr, sb, dst_ptr, db, wsb):
        rc = getattr(lib, fn)(ctx.handle, ctypes.addressof(d), count, *mid, src_ptr, ctypes.c_uint64(sb), dst_ptr, ctypes.c_uint64(db), ws.data_ptr(),
                              ctypes.c_uint64(wsb))
        return rc, lib.aej_last_error(ctx.handle)

    rc, _ = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 2 * GUARD, ws.numel())
    assert rc == 0
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out[GUARD:GUARD + m].reshape(want.shape), want)
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + m:] == 0xA5).all()

    dst.fill_(0xA5)
    before = buf.cpu().numpy().copy()

    def untouched():
        torch.cuda.synchronize()
        return (dst.cpu().numpy() == 0xA5).all() and np.array_equal(buf.cpu().numpy(), before)

    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), m + 2 * GUARD, nws - 1)
    assert rc == -4 and msg == f"workspace too small: need {nws} bytes, got {nws - 1}".encode() and untouched()      # AEJ_ERR_CAPACITY, as every entry's
    rc, msg = call(1, buf.data_ptr(), n - 1, dst.data_ptr(), m + 2 * GUARD, ws.numel())
    assert rc == -1 and msg == f"{fn}: image 0: source outside the input".encode() and untouched()
    rc, msg = call(1, buf.data_ptr(), n, dst.data_ptr(), GUARD + m - 1, ws.numel())
    assert rc == -1 and msg == f"{fn}: image 0: image outside the output".encode() and untouched()
    # the output begins at the source's last byte: refused on the host, so neither the source nor the bytes behind it change
    rc, msg = call(1, buf.data_ptr(), n, buf.data_ptr() + n - 1, m + 2 * GUARD, ws.numel())
    assert rc == -1 and msg == f"{fn}: image 0: source inside the output".encode() and untouched()
    for count in (0, -1):
        rc, msg = call(count, buf.data_ptr(), n, dst.data_ptr(), m + 2 * GUARD, ws.numel())
        assert rc == -1 and msg == f"{fn}: no images".encode() and untouched()
    # an output that ends where its source begins is taken: the ranges are half-open (both lie inside buf)
    rc, _ = call(1, buf.data_ptr() + 2048, n, buf.data_ptr() + 2048 - (m + 2 * GUARD), m + 2 * GUARD, ws.numel())
    assert rc == 0
    torch.cuda.synchronize()
