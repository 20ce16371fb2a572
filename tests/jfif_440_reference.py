"""4:4:0 JPEG files that do not depend on the code under test, shared by the host and the GPU tests of layout_440=.

Pillow cannot write the layout (subsampling="4:4:0" raises), but a Pillow 4:2:2 file becomes a valid 4:4:0 file when the sampling byte
of its frame header goes from 0x21 to 0x12 and its height and width fields are swapped: both layouts have Y, Y, Cb, Cr per MCU, the same
number of MCUs (ceil(W / 16) x ceil(H / 8) becomes ceil(H / 8) x ceil(W / 16)) and the same number of real blocks per component in the
non-interleaved scans of a progressive file, so every scan -- its restart intervals too -- decodes to the end.  The picture is another
one, which does not matter: Pillow's decode of the patched file is the reference.

There is no up-sampling rule here.  The NumPy model of the layout's reconstruction -- libjpeg's h1v2 "fancy" filter, replication at scale
8 -- is tests/scaled_decode_reference.upsample_h1v2 and the 4:4:0 branch of its decode(), checked against pil_decode-style Pillow
decodes of written 4:4:0 files at every scale (tests/test_jpeg_streams_host.py)."""
import io
import struct

import numpy as np

# source sizes (H, W) of the 4:2:2 file; the patched file is W x H
SIZES = ((16, 16), (24, 40), (9, 17), (1, 1), (8, 16), (33, 50))
# what Pillow's save takes: every way the entropy-coded data can be laid out
OPTIONS = {"baseline": dict(), "optimize": dict(optimize=True), "progressive": dict(progressive=True),
           "restart_rows": dict(restart_marker_rows=1), "progressive_restart_blocks": dict(progressive=True, restart_marker_blocks=2)}


def noise(H, W, seed=0):
    return np.random.default_rng(H * 1000 + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth(H, W):
    """a picture with structure in both directions and saturated colours: chroma edges are where an up-sampling rule shows"""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 37 + y * 11) % 256, (y * 53 + x * 5) % 256, ((x // 3 + y // 2) % 2) * 255], -1)
    return np.ascontiguousarray(img.astype(np.uint8))


def pil_422(x, quality=75, **opts):
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4 * x.shape[0] * x.shape[1] + (1 << 17))
    try:
        Image.fromarray(x).save(buf, "JPEG", quality=quality, subsampling="4:2:2", **opts)
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


def sof_at(data):
    """offset of the FF of the SOF0 / SOF1 / SOF2 marker of a file, by a marker walk of its own"""
    i = 2
    while True:
        assert data[i] == 0xFF, i
        m = data[i + 1]
        if m in (0xC0, 0xC1, 0xC2):
            return i
        assert m != 0xDA, "no frame header before the first scan"
        i += 2 + struct.unpack(">H", data[i + 2:i + 4])[0]


def frame(data):
    """(height, width, [(id, h, v, tq)]) of the frame header"""
    a = sof_at(data)
    h, w, n = struct.unpack(">HHB", data[a + 5:a + 10])
    return h, w, [(data[a + 10 + 3 * k], data[a + 11 + 3 * k] >> 4, data[a + 11 + 3 * k] & 15, data[a + 12 + 3 * k]) for k in range(n)]


def patch_440(data):
    """a three-component 4:2:2 file -> the 4:4:0 file of the docstring above"""
    a = sof_at(data)
    h, w, comps = frame(data)
    assert len(comps) == 3 and comps[0][1:3] == (2, 1) and comps[1][1:3] == comps[2][1:3] == (1, 1), comps
    out = bytearray(data)
    out[a + 5:a + 9] = struct.pack(">HH", w, h)
    out[a + 11] = 0x12
    return bytes(out)


def make_440(H, W, option="baseline", quality=75, image=None):
    """the patched file of an H x W source; its own size is W x H"""
    return patch_440(pil_422(noise(H, W) if image is None else image, quality, **OPTIONS[option]))


def pil_decode(data, scale=1):
    """Pillow's RGB pixels of a file, after draft("RGB", (W // scale, H // scale)) has chosen `scale` when that is not 1 -> (pixels,
    im.layer of the first component).  draft() cannot ask for a size of 0, so for a file with min(W, H) < scale the three things it
    sets (JpegImageFile.draft: the tile's extent, the size, decoderconfig) are set here: libjpeg then decodes at 1 / scale all the same."""
    from PIL import Image, ImageFile
    im = Image.open(io.BytesIO(data))
    if scale != 1:
        w, h = im.size
        if min(w, h) >= scale:
            im.draft("RGB", (w // scale, h // scale))
        else:
            d, e, o, a = im.tile[0]
            im._size = (-(-w // scale), -(-h // scale))
            im.tile = [ImageFile._Tile(d, (e[0], e[1], e[0] + im._size[0], e[1] + im._size[1]), o, a)]
            im.decoderconfig = (scale, 0)
        assert im.decoderconfig == (scale, 0), (im.size, scale, im.decoderconfig)
    layer = tuple(im.layer[0])
    return np.asarray(im.convert("RGB")), layer
