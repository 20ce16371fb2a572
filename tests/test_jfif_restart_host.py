"""Restart markers on the host side (no GPU needed): the markers the host writers produce against Pillow's own header bytes, the index
rules of csrc/jfif_restart_core.h (aej_jfif_restart_map_host) against their restatement in tests/jfif_restart_reference.py and against
the DRI segments of Pillow's files, libjpeg's 16-bit clamp, the argument checks of the four calls and the ABI's new symbols."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jfif_restart_reference as RR  # noqa: E402

import adaptive_edge_aware_jpeg_amd as A  # noqa: E402
from adaptive_edge_aware_jpeg_amd import standard_jpeg as S  # noqa: E402
from adaptive_edge_aware_jpeg_amd._lib import SIGNATURES, load_library  # noqa: E402

LAYOUTS = ("4:4:4", "4:2:2", "4:2:0")
KINDS = [(s, 3) for s in LAYOUTS] + [("4:4:4", 1)]                       # (subsampling, components)
OPTIONS = [dict(restart_marker_rows=1), dict(restart_marker_blocks=5), dict(restart_marker_blocks=1), dict(restart_marker_blocks=2),
           dict(restart_marker_blocks=100), dict(restart_marker_rows=5), dict(restart_marker_rows=1, restart_marker_blocks=3)]
SIZES = [(40, 56), (64, 64), (8, 8), (9, 200), (32, 48)]                 # (H, W): the GPU tests' list
AEJ_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return load_library()


def _image(h, w, seed=3):
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5)[:, :, None] % 256
    return ((rng.integers(0, 256, (h, w, 3)) + ramp) // 2).astype(np.uint8)


def _pil(x, ss, nc, q=75, **kw):
    from PIL import Image
    buf = io.BytesIO()
    if nc == 1:
        Image.fromarray(x[:, :, 0]).save(buf, "JPEG", quality=q, **kw)
    else:
        Image.fromarray(x).save(buf, "JPEG", quality=q, subsampling=ss, **kw)
    return buf.getvalue()


def _rst(opt):
    return opt.get("restart_marker_blocks", 0), opt.get("restart_marker_rows", 0)


def _headers(lib, q, h, w, ss, nc, blocks, rows):
    out = (ctypes.c_uint8 * 1024)()
    n = lib.aej_jfif_headers_rst_host(q, h, w, LAYOUTS.index(ss), nc, blocks, rows, ctypes.addressof(out), 1024)
    assert n > 0, n
    return bytes(out[:n])


def _map(lib, h, w, ss, nc, blocks, rows, prog):
    r, dri, counts = (ctypes.c_int32 * 10)(), (ctypes.c_int32 * 10)(), (ctypes.c_int64 * 2)()
    args = (h, w, LAYOUTS.index(ss), nc, blocks, rows, int(prog), ctypes.addressof(r), ctypes.addressof(dri))
    ns = lib.aej_jfif_restart_map_host(*args, None, None, 0, None, 0, ctypes.addressof(counts))
    assert ns > 0, ns
    nblk, niv = counts[0], counts[1]
    iv, rs, mk = np.full(nblk + 1, -7, np.int32), np.full(nblk + 1, 77, np.uint8), np.full(niv + 1, 77, np.uint8)      # one guard entry behind each
    assert lib.aej_jfif_restart_map_host(*args, iv.ctypes.data, rs.ctypes.data, nblk, mk.ctypes.data, niv, None) == ns
    assert iv[nblk] == -7 and rs[nblk] == 77 and mk[niv] == 77
    return [(r[i], bool(dri[i])) for i in range(ns)], iv[:nblk].tolist(), rs[:nblk].astype(bool).tolist(), mk[:niv].tolist()


@pytest.mark.parametrize("opt", OPTIONS[:2], ids=str)
@pytest.mark.parametrize("ss,nc", KINDS)
def test_header_bytes_equal_pillows(lib, ss, nc, opt):
    h, w = 40, 56
    x = _image(h, w)
    blocks, rows = _rst(opt)
    ours = _headers(lib, 75, h, w, ss, nc, blocks, rows)
    scans, _, _, _ = _map(lib, h, w, ss, nc, blocks, rows, False)
    # baseline: every byte up to the SOS, the DRI between the last DHT and the SOS
    pil = _pil(x, ss, nc, **opt)
    assert RR.header_until_sos(pil) == ours[:len(ours) - (10 if nc == 1 else 14)]
    assert RR.dri_sequence(pil) == [scans[0][0]] and scans[0][1]
    dri = bytes([0xFF, 0xDD, 0, 4, scans[0][0] >> 8, scans[0][0] & 255])
    assert ours[-(16 if nc == 1 else 20):].startswith(dri)
    # optimised: the DHT segments depend on the pixels; everything else, the DRI's place and value included, is the same
    pil = _pil(x, ss, nc, optimize=True, **opt)
    assert RR.header_until_sos(pil, drop_dht=True) == RR.header_until_sos(ours + b"\xff\xd9", drop_dht=True)
    # progressive: SOF2, and the DRI of every scan whose interval differs from the one before
    pil = _pil(x, ss, nc, progressive=True, **opt)
    sof = ours.index(b"\xff\xc0")
    assert RR.header_until_sos(pil, drop_dht=True) == RR.header_until_sos(ours[:sof] + b"\xff\xc2" + ours[sof + 2:] + b"\xff\xd9", drop_dht=True)
    scans, _, _, _ = _map(lib, h, w, ss, nc, blocks, rows, True)
    assert len(scans) == (6 if nc == 1 else 10)
    assert RR.dri_sequence(pil) == [r if d else None for r, d in scans]


def test_the_issues_dri_example(lib):
    """40 x 56 (H x W) 4:2:0, progressive, rows = 1: DRI 4, 7, 4, -, 7, -, 4, -, -, 7; baseline 4; grey 7"""
    scans, _, _, _ = _map(lib, 40, 56, "4:2:0", 3, 0, 1, True)
    assert [r if d else None for r, d in scans] == [4, 7, 4, None, 7, None, 4, None, None, 7]
    assert _map(lib, 40, 56, "4:2:0", 3, 0, 1, False)[0] == [(4, True)]
    assert _map(lib, 40, 56, "4:2:0", 1, 0, 1, False)[0] == [(7, True)]
    assert _map(lib, 40, 56, "4:2:0", 3, 0, 0, True)[0] == [(0, False)] * 10


@pytest.mark.parametrize("opt", OPTIONS, ids=str)
@pytest.mark.parametrize("ss,nc", KINDS)
def test_restart_map_equals_the_python_rules(lib, ss, nc, opt):
    blocks, rows = _rst(opt)
    for h, w in SIZES:
        for prog in (False, True):
            scans, iv, rs, mk = _map(lib, h, w, ss, nc, blocks, rows, prog)
            assert scans == RR.scan_intervals(h, w, ss, nc, blocks, rows, prog), (h, w, prog)
            want = RR.block_map(h, w, ss, nc, scans[0][0])
            assert (iv, rs, mk) == want, (h, w, prog)


def test_marker_numbers_wrap(lib):
    _, iv, rs, mk = _map(lib, 64, 64, "4:4:4", 3, 1, 0, False)
    assert mk[:11] == [0, 0xD0, 0xD1, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD0, 0xD1] and len(mk) == 64
    assert iv == [m for m in range(64) for _ in range(3)] and all(rs)


def test_rows_are_clamped_as_libjpeg_does(lib):
    """a 24 x 8 (W x H) 4:4:4 image has 3 MCUs per row: 30000 rows would be 90000 MCUs"""
    dri = bytes.fromhex("ffdd0004ffff")
    for blocks, rows in ((0, 30000), (65535, 0)):
        assert dri in _headers(lib, 75, 8, 24, "4:4:4", 3, blocks, rows)
        assert _map(lib, 8, 24, "4:4:4", 3, blocks, rows, True)[0][0] == (65535, True)
    x = _image(8, 24)
    assert dri in _pil(x, "4:4:4", 3, restart_marker_rows=30000) and dri in _pil(x, "4:4:4", 3, restart_marker_blocks=65535)


@pytest.fixture()
def no_context(monkeypatch):
    """any attempt to reach a device context, or the library, fails the test"""
    def boom(*a, **k):
        raise AssertionError("the device or the library was asked for before the arguments were checked")
    monkeypatch.setattr(S, "get_context", boom)
    from adaptive_edge_aware_jpeg_amd import _lib
    monkeypatch.setattr(_lib, "load_library", boom)              # (the calls import it from there when they parse a file)


def _calls():
    x = np.zeros((8, 8, 3), np.uint8)
    jpg = _pil(_image(16, 16), "4:2:0", 3)
    return [lambda **kw: A.standard_jpeg_encode_many([x], **kw),
            lambda **kw: A.standard_jpeg_thumbnail_jpeg_many([jpg], (8, 8), **kw),
            lambda **kw: A.standard_jpeg_transcode_many([jpg], **kw),
            lambda **kw: A.standard_jpeg_transform_many([jpg], "flip_h", **kw)]


def test_restart_arguments_are_checked_before_the_library_is_touched(no_context):
    for call in _calls():
        for name in ("restart_marker_blocks", "restart_marker_rows"):
            for bad in (True, False, 1.5, 2.0, "1", None):
                with pytest.raises(TypeError, match=name):
                    call(**{name: bad})
            for bad in (-1, 65536):
                with pytest.raises(ValueError, match=name):
                    call(**{name: bad})


class _Recorder:
    """stands in for the library: notes every entry called with its arguments and answers 0 (a workspace the library refuses)"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, tuple(a.value if hasattr(a, "value") else a for a in args)))
            return 0
        return entry


class _HostContext:
    """a context without a device: CPU tensors, the recorder as its library"""
    def __init__(self):
        import torch
        self.torch, self.lib, self.handle, self.device = torch, _Recorder(), None, torch.device("cpu")

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype)

    def pinned(self, n):
        return self.torch.empty((n,), dtype=self.torch.uint8)

    def workspace(self, n):
        raise AssertionError("no workspace is made for a size of 0")


def test_zero_zero_reaches_the_wide_entries_with_neutral_arguments(monkeypatch):
    """The package binds the widest entry of each operation ("What the JPEG file calls share"): the defaults and an explicit
    (0, 0) are one and the same call, whose restart arguments are 0, 0 -- by include/aej.h the entry without them -- and a setting
    changes those two arguments and nothing else.  tests/test_gpu_jpeg_wide_entries.py holds the library to that equivalence."""
    ctx = _HostContext()
    monkeypatch.setattr(S, "get_context", lambda device=0: ctx)
    x = _image(32, 48)                                                # whole MCUs: rot180 is allowed
    jpg = _pil(x, "4:2:0", 3)

    def entry(call, **kw):
        ctx.lib.calls.clear()
        with pytest.raises(ValueError, match="refuses"):
            call(**kw)
        assert len(ctx.lib.calls) == 1
        return ctx.lib.calls[0]

    enc = lambda **kw: A.standard_jpeg_encode_many([x], **kw)  # noqa: E731
    tra = lambda **kw: A.standard_jpeg_transcode_many([jpg], **kw)  # noqa: E731
    tfm = lambda **kw: A.standard_jpeg_transform_many([jpg], "rot180", **kw)  # noqa: E731
    ADDR = "an address"                                               # of host arrays, new with every call; NULL stays None

    def shape(args, blocks, rows):
        return tuple(ADDR if isinstance(a, int) and a > 65535 else a for a in args) == tuple(blocks if a == "blocks" else rows if a == "rows" else a
                                                                                            for a in want)

    many = ("aej_jfif_many_workspace_bytes_rst", (None, ADDR, 1, 2, 0, 0, "blocks", "rows"))      # ctx, descs, n, 4:2:0, optimize, progressive
    # ctx, descs, n_base, frames, scans, n_prog, progressive, transforms, trim, restart_blocks, restart_rows, layout_440, boxes, drop_chroma
    cut = "aej_jfif_transform_workspace_bytes_cut"
    for call, (name, want) in ((enc, many), (tra, (cut, (None, ADDR, 1, ADDR, ADDR, 0, 0, None, 0, "blocks", "rows", 0, None, 0))),
                               (tfm, (cut, (None, ADDR, 1, ADDR, ADDR, 0, 0, ADDR, 0, "blocks", "rows", 0, None, 0)))):
        assert len(want) == len(SIGNATURES[name][1])
        for kw, blocks, rows in (({}, 0, 0), (dict(restart_marker_blocks=0, restart_marker_rows=0), 0, 0),
                                 (dict(restart_marker_blocks=3, restart_marker_rows=2), 3, 2), (dict(restart_marker_rows=1), 0, 1)):
            got = entry(call, **kw)
            assert got[0] == name and shape(got[1], blocks, rows), (name, kw, got)


def test_abi_symbols_and_refusals(lib):
    assert lib.aej_abi_version() == 3
    old = ("aej_jfif_many_workspace_bytes", "aej_jfif_many_encode", "aej_jfif_transcode_workspace_bytes", "aej_jfif_transcode_batch",
           "aej_jfif_transform_workspace_bytes", "aej_jfif_transform_batch")
    for name in old + tuple(n + "_rst" for n in old) + ("aej_jfif_headers_rst_host", "aej_jfif_restart_map_host", "aej_jfif_headers_host_opt"):
        assert name in SIGNATURES and hasattr(lib, name), name
    from adaptive_edge_aware_jpeg_amd._lib import JfifManyDesc
    d = (JfifManyDesc * 2)(JfifManyDesc(0, 56, 40, 75, 0), JfifManyDesc(56 * 40 * 3, 56, 40, 75, 1))

    def size(opt, prog, blocks, rows):
        return lib.aej_jfif_many_workspace_bytes_rst(None, ctypes.addressof(d), 2, 2, opt, prog, blocks, rows)

    for opt, prog in ((0, 0), (1, 0), (0, 1)):
        base = lib.aej_jfif_many_workspace_bytes(None, ctypes.addressof(d), 2, 2, opt, prog)
        assert base > 0 and size(opt, prog, 0, 0) == base
        assert size(opt, prog, 1, 0) > base and size(opt, prog, 0, 1) > base     # the intervals' starts
        for blocks, rows in ((-1, 0), (65536, 0), (0, -1), (0, 65536)):
            assert size(opt, prog, blocks, rows) == 0
    out = (ctypes.c_uint8 * 1024)()
    assert lib.aej_jfif_headers_rst_host(75, 40, 56, 2, 3, 65536, 0, ctypes.addressof(out), 1024) == AEJ_ERR_ARG
    assert lib.aej_jfif_headers_rst_host(75, 40, 56, 2, 2, 1, 0, ctypes.addressof(out), 1024) == AEJ_ERR_ARG
    assert lib.aej_jfif_headers_rst_host(75, 40, 56, 2, 3, 1, 0, ctypes.addressof(out), 10) == -4
    # with 0, 0 the new writer gives the old writers' bytes
    old_hdr = (ctypes.c_uint8 * 1024)()
    n = lib.aej_jfif_headers_host_opt(75, 40, 56, 2, ctypes.addressof(old_hdr), 1024)
    assert n > 0 and lib.aej_jfif_headers_rst_host(75, 40, 56, 2, 3, 0, 0, ctypes.addressof(out), 1024) == n and bytes(out[:n]) == bytes(old_hdr[:n])
    r, dri = (ctypes.c_int32 * 10)(), (ctypes.c_int32 * 10)()
    assert lib.aej_jfif_restart_map_host(40, 56, 2, 3, 1, 0, 0, None, ctypes.addressof(dri), None, None, 0, None, 0, None) == AEJ_ERR_ARG
    iv = (ctypes.c_int32 * 4)()
    assert lib.aej_jfif_restart_map_host(40, 56, 2, 3, 1, 0, 0, ctypes.addressof(r), ctypes.addressof(dri), ctypes.addressof(iv), None, 4, None, 0, None) == -4
    # without a context the device entries refuse at once, as every entry does
    assert lib.aej_jfif_many_encode_rst(None, ctypes.addressof(d), 2, None, 0, 2, 0, 0, 1, 0, None, 0, None, None, None, None, None, 0) == AEJ_ERR_ARG
