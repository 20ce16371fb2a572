"""Restart markers (DRI / RSTn) as libjpeg's encoders place them, restated in plain Python for the tests: a scan's interval, every
block's interval and predictor reset, the marker numbers, the DRI sequence of a file -- and a small marker walker that reads the same
facts back from a finished file (Pillow's or this library's).  The scan scripts are jfif_progressive_reference's."""
from jfif_options_reference import FACTORS
from jfif_progressive_reference import SCRIPT

GREY_SCRIPT = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
MAX_INTERVAL = 65535


def ceil_div(a, b):
    return -(-a // b)


def grid(H, W, subsampling, components=3):
    """-> (hs, vs, mcux, mcuy, ybx, yby): luma sampling factors, the MCU grid, the real luma blocks per row / column"""
    hs, vs = (1, 1) if components == 1 else FACTORS[subsampling]
    return hs, vs, ceil_div(W, 8 * hs), ceil_div(H, 8 * vs), ceil_div(W, 8), ceil_div(H, 8)


def interval(blocks, rows, per_row):
    """R of a scan with per_row MCUs in a row: rows > 0 overrides blocks and is clamped to 16 bits"""
    return min(rows * per_row, MAX_INTERVAL) if rows > 0 else blocks


def scan_mcus(H, W, subsampling, components, comps):
    """-> (MCUs per row, MCUs) of a scan over the components `comps` (indices into Y, Cb, Cr)"""
    hs, vs, mcux, mcuy, ybx, yby = grid(H, W, subsampling, components)
    if len(comps) > 1 or components == 1:
        return mcux, mcux * mcuy
    return (ybx, ybx * yby) if comps[0] == 0 else (mcux, mcux * mcuy)


def scan_intervals(H, W, subsampling, components, blocks, rows, progressive):
    """-> [(R, DRI written before this scan)] for every scan of the file"""
    if progressive:
        script = [s[0] for s in (GREY_SCRIPT if components == 1 else SCRIPT)]
    else:
        script = [(0,) if components == 1 else (0, 1, 2)]
    out, written = [], 0
    for comps in script:
        r = interval(blocks, rows, scan_mcus(H, W, subsampling, components, comps)[0])
        out.append((r, r != written))
        written = r
    return out


def block_map(H, W, subsampling, components, R):
    """The interleaved (baseline) scan, blocks in MCU order, dummies included -> (interval of every block, whether its DC predictor is
    0, the second byte of the marker before every interval -- 0 for the first)"""
    hs, vs, mcux, mcuy, _, _ = grid(H, W, subsampling, components)
    bpm = hs * vs + (0 if components == 1 else 2)
    n_mcu = mcux * mcuy
    ivs, resets = [], []
    for m in range(n_mcu):
        opens = m == 0 or (R > 0 and m % R == 0)
        for k in range(bpm):
            ivs.append(m // R if R else 0)
            first_of_component = k == 0 or k >= hs * vs      # the component's first block of this MCU: its predecessor is in MCU m - 1
            resets.append(opens and first_of_component)
    niv = ceil_div(n_mcu, R) if R else 1
    return ivs, resets, [0] + [0xD0 + ((k - 1) & 7) for k in range(1, niv)]


# ---- reading a file back ---------------------------------------------------------------------------------------------------------------
def walk(data):
    """-> [(marker, offset, end)] of the segments SOI .. EOI; an SOS entry's end is the end of its entropy-coded data"""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    out, i = [(0xD8, 0, 2)], 2
    while i < len(data):
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m == 0xD9:
            out.append((m, i, i + 2))
            break
        n = int.from_bytes(data[i + 2:i + 4], "big")
        j = i + 2 + n
        if m == 0xDA:
            while not (data[j] == 0xFF and data[j + 1] != 0 and not 0xD0 <= data[j + 1] <= 0xD7):
                j += 1
        out.append((m, i, j))
        i = j
    return out


def dri_sequence(data):
    """-> per scan, the interval its own DRI sets, or None when no DRI directly precedes its SOS"""
    out, last = [], None
    for m, a, b in walk(data):
        if m == 0xDA:
            out.append(last)
            last = None
        elif m == 0xDD:
            assert data[a + 2:a + 4] == b"\x00\x04"
            last = int.from_bytes(data[a + 4:a + 6], "big")
        else:
            last = None
    return out


def markers(data):
    """-> per scan, the list of RSTn second bytes in its data (a stuffed FF 00 is data)"""
    data, out = bytes(data), []
    for m, a, b in walk(data):
        if m != 0xDA:
            continue
        i = a + 2 + int.from_bytes(data[a + 2:a + 4], "big")
        found = []
        while i < b - 1:
            if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7:
                found.append(data[i + 1])
                i += 2
            elif data[i] == 0xFF:
                i += 2
            else:
                i += 1
        out.append(found)
    return out


def header_until_sos(data, drop_dht=False):
    """the bytes before the first SOS, optionally without the DHT segments (optimised tables depend on the pixels)"""
    data, out = bytes(data), b""
    for m, a, b in walk(data):
        if m == 0xDA:
            return out
        if not (drop_dht and m == 0xC4):
            out += data[a:b]
    raise AssertionError("no SOS")


# ---- the inputs and Pillow calls the GPU tests share --------------------------------------------------------------------------------------
def noise():
    import numpy as np
    return np.random.default_rng(0).integers(0, 256, (64, 64, 3), dtype=np.uint8)


def flat():
    import numpy as np
    return np.full((64, 64, 3), 137, np.uint8)


def spike():
    """value 137 with one 8 x 8 noise block: long end-of-band runs that every restart cuts"""
    import numpy as np
    x = flat()
    x[24:32, 40:48] = np.random.default_rng(5).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    return x


def gradient(h, w, seed=3):
    """a gradient plus noise"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5)[:, :, None] % 256
    return ((rng.integers(0, 256, (h, w, 3)) + ramp) // 2).astype(np.uint8)


def pil_save(x, q=75, **kw):
    """Pillow's file of an [H, W, 3] or [H, W] array (a larger ImageFile.MAXBLOCK lets optimised scans of noise through and does not
    change the bytes)"""
    import io
    from PIL import Image, ImageFile
    im = x if isinstance(x, Image.Image) else Image.fromarray(x)
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * im.size[0] * im.size[1] + 4096)
    try:
        im.save(buf, "JPEG", quality=q, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def pil_pixels(data):
    import io
    import numpy as np
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def same_files_and_pixels(A, ours, want, progressive=False):
    """every file equals Pillow's byte for byte, and this library's decoder gives the pixels Pillow decodes from it"""
    import numpy as np
    assert len(ours) == len(want)
    for i, (a, b) in enumerate(zip(ours, want)):
        assert a == b, (i, len(a), len(b), next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), None))
    for i, (t, f) in enumerate(zip(A.standard_jpeg_decode_many(ours, progressive=progressive), ours)):
        assert np.array_equal(t.cpu().numpy(), pil_pixels(f)), i
