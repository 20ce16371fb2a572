"""Pillow references for the mode-"L" output of the JPEG decoders and thumbnails (tests/test_gpu_jpeg_luma.py, tests/test_jpeg_luma_host.py,
tests/golden/jpeg_luma/make_jpeg_luma_golden.py).  Everything here is Pillow itself: ``im.draft("L", ...)`` makes libjpeg set
out_color_space = JCS_GRAYSCALE, so a colour file decodes to its luma plane alone; a one-component file is mode "L" already."""
import io

import numpy as np

FILTERS = {"box": 4, "bilinear": 2, "hamming": 5, "bicubic": 3, "lanczos": 1}


def _force(im, mode, scale):
    """what JpegImageFile.draft sets (mode, the tile's extent and arguments, the size, decoderconfig), set by hand: draft() cannot ask for a
    size of 0, which (W // scale, H // scale) is for a file with min(W, H) < scale.  libjpeg decodes at 1 / scale all the same."""
    from PIL import ImageFile
    d, e, o, a = im.tile[0]
    if a[0] == "RGB" and mode in ("L", "YCbCr"):
        im._mode = mode
        a = mode, ""
    w, h = im.size
    im._size = (-(-w // scale), -(-h // scale))
    im.tile = [ImageFile._Tile(d, (e[0], e[1], e[0] + im._size[0], e[1] + im._size[1]), o, a)]
    im.decoderconfig = (scale, 0)


def draft(data, mode, scale=1):
    """the opened file after its one draft() call has asked for `mode` ("L", "YCbCr" or None) at `scale`"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    w, h = im.size
    if min(w, h) >= scale:
        im.draft(mode, (w // scale, h // scale))
    else:
        _force(im, mode, scale)
    assert im.decoderconfig == (scale, 0), (im.size, scale, im.decoderconfig)
    return im


def draft_l(data, scale=1):
    """uint8 [ceil(H / scale), ceil(W / scale)]: a grey file's samples, a colour file's luma plane"""
    im = draft(data, "L", scale)
    assert im.mode == "L"
    return np.asarray(im)


def convert_l(data):
    """the OTHER meaning of "L": ITU-R 601 weights over the decoded RGB pixels"""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB").convert("L"))


def auto(data):
    """the file in Pillow's own mode: [H, W] for a one-component file, [H, W, 3] for a colour one"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    return np.asarray(im if im.mode == "L" else im.convert("RGB"))


def thumbnail_image(data, size, resample, gap, mode, thumbnail_plan):
    """The PIL image of standard_jpeg_thumbnail_many's element under `mode` ("L" or "auto").  A one-component file, and a colour file
    under "auto", is ``im.thumbnail(size, F, reducing_gap=gap)``.  A colour file under "L" is the thumbnail Pillow makes when its one
    draft() call asks for mode "L" (thumbnail()'s own draft() is a no-op after a first one): thumbnail_plan (the library's host
    function, itself tested against Pillow's thumbnail()) gives the final size; the draft and the resize are Pillow's."""
    from PIL import Image
    F = FILTERS[resample] if isinstance(resample, str) else resample
    im = Image.open(io.BytesIO(data))
    if im.mode == "L" or mode == "auto":
        im.thumbnail(size, F, reducing_gap=gap)
        return im if im.mode == "L" else im.convert("RGB")
    W, H = im.size
    plan = thumbnail_plan(W, H, size, gap)
    if plan is None:
        im.draft("L", None)
        assert im.mode == "L"
        return im
    res = im.draft("L", (int(size[0] * gap), int(size[1] * gap))) if gap is not None else im.draft("L", None)
    assert im.mode == "L" and im.decoderconfig[0] == plan[0]
    if im.size != tuple(plan[2]):
        im = im.resize(tuple(plan[2]), F, box=res[1], reducing_gap=gap)
    return im


def thumbnail(data, size, resample, gap, mode, thumbnail_plan):
    return np.asarray(thumbnail_image(data, size, resample, gap, mode, thumbnail_plan))


def sampling(data):
    """"grey", "4:4:4", "4:2:2", "4:2:0" or "4:4:0" from the frame header, as Pillow's im.layer has it"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if len(im.layer) == 1:
        return "grey"
    return {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0", (1, 2): "4:4:0"}[(im.layer[0][1], im.layer[0][2])]
