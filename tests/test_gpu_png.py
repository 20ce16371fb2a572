"""GPU: png_decode_many (csrc/inflate.hip as it is, csrc/png.hip: the scanline un-filter and the layout conversion).  Every comparison is
exact equality against tests/png_reference.py's reader, which live Pillow has confirmed on the same bytes (``R.expected``).  The files
come from the helper's writer, which filters each row with the filter type the test asks for; samples are seeded."""
import ctypes

import numpy as np
import pytest

import png_reference as R

pytestmark = pytest.mark.gpu
MODES = ("RGB", "auto")


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _check(A, names, modes=MODES, **kw):
    """one call per mode over the named files of the suite; every tensor equal to the reference"""
    S = R.suite()
    for mode in modes:
        got = A.png_decode_many([S[n] for n in names], mode=mode, **kw)
        assert len(got) == len(names)
        for n, g in zip(names, got):
            want = R.expected(n, mode)
            g = g.cpu().numpy()
            assert g.dtype == np.uint8 and g.shape == want.shape, (n, mode, g.shape, want.shape)
            assert np.array_equal(g, want), (n, mode, np.argwhere(g != want)[:4].tolist())


@pytest.mark.parametrize("pattern", sorted(R.PATTERNS))
def test_every_kind_13x7(A, pattern):
    """row r with filter r % 5, with (4 - r) % 5 (every filter on row 0, where "up" is zero), and one filter for all rows; width 13 at
    depths 1, 2 and 4 leaves the last byte partial"""
    _check(A, [f"f13x7_{pattern}_ct{ct}d{d}" for ct, d in R.KINDS])


@pytest.mark.parametrize("w", (1, 2, 3))
def test_narrow(A, w):
    _check(A, [f"w{w}_ct{ct}d{d}" for ct, d in R.KINDS])


def test_band_boundaries(A):
    """heights around one and two bands of rows, all Paeth and all Average: the last row of a band is carried to the next"""
    _check(A, [f"h{h}_all{f}" for h in R.HEIGHTS for f in (4, 3)])


def test_rows_wider_than_a_tile(A):
    """700 x 9 RGBA (2800 bytes a row), and wide rows over more than one band at every unit size: the carry across tiles"""
    _check(A, ["wide_rgba", "wide_rgb", "wide_grey", "wide_ga", "wide_bits", "wide_pal4"])


def test_streams(A):
    """stored, fixed / short dynamic and dynamic blocks; IDAT in 1-byte chunks, in 7-byte chunks with empty ones between; a Pillow-written
    file with Up and Paeth rows and several dynamic blocks"""
    _check(A, ["level0", "level1", "level9", "idat_1", "idat_7_empty", "lena"])
    S = R.suite()
    assert np.array_equal(R.expected("level0", "RGB"), R.expected("idat_1", "RGB"))
    assert R.read_png(S["lena"])[1].shape == (512, 1536) and len(S["level0"]) > len(S["level9"])


def test_layouts(A):
    """a palette of 10 entries with indices up to 255 (black); tRNS on palette, grey and RGB files (ignored); grey + alpha and RGBA in
    both modes; unknown ancillary chunks"""
    _check(A, ["short_palette", "trns_palette", "trns_grey", "trns_rgb", "ga", "rgba", "ancillary"])
    assert not R.expected("short_palette", "RGB")[0, 0].any() and not R.expected("short_palette", "RGB")[0, 1].any()
    S = R.suite()
    ga, rgba = (x.cpu().numpy() for x in A.png_decode_many([S["ga"], S["rgba"]], mode="auto"))
    assert ga.shape == (33, 45, 2) and rgba.shape == (33, 45, 4)
    ga3, rgb = (x.cpu().numpy() for x in A.png_decode_many([S["ga"], S["rgba"]]))
    assert np.array_equal(ga3, np.repeat(ga[:, :, :1], 3, 2)) and np.array_equal(rgb, rgba[:, :, :3])      # alpha dropped, not composited


def _mixed():
    names = [n for n in sorted(R.suite()) if n.startswith(("f13x7_cycle", "w2_", "wide_", "h65", "h130", "level", "idat_7", "ga", "rgba", "short", "trns"))]
    names.append("lena")
    order = np.random.default_rng(5).permutation(len(names))
    names = [names[i] for i in order]
    modes = [MODES[(i * 7 + 3) % 5 % 2] for i in range(len(names))]
    return names, modes


def test_mixed_call_with_a_mode_per_file(A):
    """every kind and several sizes in one call, shuffled, each file with its own mode"""
    names, modes = _mixed()
    assert {m for m in modes} == set(MODES) and len(names) > 40
    S = R.suite()
    got = A.png_decode_many([S[n] for n in names], mode=modes)
    for n, m, g in zip(names, modes, got):
        assert np.array_equal(g.cpu().numpy(), R.expected(n, m)) and g.shape == R.expected(n, m).shape, (n, m)


def test_more_files_than_one_launch_takes(A):
    """the un-filter kernel takes 64 files a launch (their table travels in its arguments): 77 files are two launches"""
    names = [f"f13x7_{p}_ct{ct}d{d}" for p in sorted(R.PATTERNS) for ct, d in R.KINDS]
    assert len(names) > 64
    _check(A, names)


def test_host_inflate_equals_gpu_inflate(A):
    import torch
    names, modes = _mixed()
    S = R.suite()
    files = [S[n] for n in names]
    gpu = A.png_decode_many(files, mode=modes, inflate="gpu")
    host = A.png_decode_many(files, mode=modes, inflate="host", workers=4)
    assert len(gpu) == len(host) == len(files)
    for n, a, b in zip(names, gpu, host):
        assert a.shape == b.shape and torch.equal(a, b), n
    _check(A, ["wide_rgb", "idat_1"], inflate="host")


@pytest.mark.parametrize("inflate", ("gpu", "host"))
def test_data_errors_name_the_file_and_leave_the_context_good(A, inflate):
    """a flipped byte in the compressed data, a truncated IDAT, one row too few and a filter byte 5 are data errors, not faults: in a call
    of three files only the bad one is named, and the same call without it then decodes correctly"""
    S = R.suite()
    for what, bad in R.corrupt_files().items():
        with pytest.raises(ValueError, match=r"^file 1: ") as e:
            A.png_decode_many([S["level9"], bad, S["ga"]], inflate=inflate)
        assert not isinstance(e.value, NotImplementedError)
        text = {"flipped": "inflate", "truncated": "inflate", "short": "size", "filter5": "filter byte"}[what]
        assert text in str(e.value), (what, str(e.value))
        with pytest.raises(ValueError, match=r"^file 0: "):
            A.png_decode_many([bad], inflate=inflate)
        _check(A, ["level9", "ga"], inflate=inflate)


def test_c_entry(A):
    """aej_inflate_batch + aej_png_unfilter_batch through ctypes on two files, the status array read back: the ABI without the Python layer"""
    import torch
    from adaptive_edge_aware_jpeg_amd._lib import PngDesc, get_context
    ctx = get_context(0)
    lib = ctx.lib
    S = R.suite()
    names, layouts = ["short_palette", "wide_ga"], np.array([0, 1], np.int32)
    descs, streams = (PngDesc * 2)(), []
    for i, n in enumerate(names):
        data = S[n]
        buf = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
        spans = np.zeros((4, 2), np.int64)
        assert lib.aej_png_parse_host(ctypes.addressof(buf), len(data), ctypes.addressof(descs[i]), spans.ctypes.data, 4, None, 0) == 0
        streams.append(b"".join(data[o:o + k] for o, k in spans[:descs[i].n_idat].tolist()))
    sizes = [d.height * (1 + d.row_bytes) for d in descs]
    in_off = np.array([0, (sizes[0] + 3) // 4 * 4], np.int64)
    src_off = [0, (len(streams[0]) + 3) // 4 * 4]
    src = np.zeros(src_off[1] + len(streams[1]) + 3, np.uint8)
    for o, z in zip(src_off, streams):
        src[o:o + len(z)] = np.frombuffer(z, np.uint8)
    table = np.array([[src_off[i], len(streams[i]), in_off[i], sizes[i]] for i in range(2)], np.int64)
    pal = np.stack([np.frombuffer(bytes(d.palette), np.uint8) for d in descs])
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    d_src, d_table, d_pal = dev(src), dev(table), dev(pal)
    # what the two entries write (scanlines, inflated sizes) and their scratch start as 0xA5 bytes, not as zeros they could lean on
    raw = torch.full((int(in_off[1]) + (sizes[1] + 3) // 4 * 4,), 0xA5, dtype=torch.uint8, device="cuda")
    inflated = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda").view(torch.int64)
    ist = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    want = [R.expected(names[0], "RGB"), R.expected(names[1], "auto")]
    out_off = np.array([8, 8 + want[0].size + 5], np.int64)              # unaligned images with guard bytes around them
    out = torch.full((int(out_off[1]) + want[1].size + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.check(lib.aej_inflate_batch(ctx.handle, d_src.data_ptr(), d_table.data_ptr(), 2, raw.data_ptr(), ctypes.c_uint64(raw.numel()),
                                    inflated.data_ptr(), ist.data_ptr()))
    nws = int(lib.aej_png_workspace_bytes(ctx.handle, ctypes.addressof(descs), 2))
    assert nws > 0 and nws % 256 == 0
    ws = torch.full((nws,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.check(lib.aej_png_unfilter_batch(ctx.handle, ctypes.addressof(descs), 2, raw.data_ptr(), ctypes.c_uint64(raw.numel()), in_off.ctypes.data,
                                         inflated.data_ptr(), ist.data_ptr(), d_pal.data_ptr(), layouts.ctypes.data, out.data_ptr(),
                                         ctypes.c_uint64(out.numel()), out_off.ctypes.data, status.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nws)))
    assert status.cpu().tolist() == [0, 0] and ist.cpu().tolist() == [0, 0] and inflated.cpu().tolist() == sizes
    o = out.cpu().numpy()
    for i in range(2):
        a = int(out_off[i])
        assert np.array_equal(o[a:a + want[i].size].reshape(want[i].shape), want[i]), names[i]
    used = np.zeros(o.size, bool)
    for i in range(2):
        used[int(out_off[i]):int(out_off[i]) + want[i].size] = True
    assert (o[~used] == 0xAB).all()                                      # no write leaves a file's image
    # what the entry refuses on the host: a workspace too small, an image outside the output, a misaligned scanline offset
    args = lambda **k: (ctx.handle, ctypes.addressof(descs), 2, raw.data_ptr(), ctypes.c_uint64(raw.numel()), k.get("in_off", in_off).ctypes.data,  # noqa: E731
                        inflated.data_ptr(), ist.data_ptr(), d_pal.data_ptr(), layouts.ctypes.data, out.data_ptr(),
                        ctypes.c_uint64(k.get("out_bytes", out.numel())), out_off.ctypes.data, status.data_ptr(), ws.data_ptr(),
                        ctypes.c_uint64(k.get("nws", nws)))
    assert lib.aej_png_unfilter_batch(*args(nws=nws - 256)) == -4
    assert lib.aej_png_unfilter_batch(*args(out_bytes=out.numel() - 9)) == -1
    assert lib.aej_png_unfilter_batch(*args(in_off=in_off + 2)) == -1
