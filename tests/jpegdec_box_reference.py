"""What the tests of box= (standard_jpeg_decode_many) share, none of it the code under test: the brute-force MCU window written from the
up-sampling rule, the test picture, the files Pillow makes of it in every layout, and the boxes."""
import io

import numpy as np

import jfif_440_reference as F440

# (name, hs, vs, ncomp)
LAYOUTS = (("444", 1, 1, 3), ("422", 2, 1, 3), ("420", 2, 2, 3), ("440", 1, 2, 3), ("grey", 1, 1, 1))
NARROW = tuple((w, 20) for w in range(1, 6))


def chroma_samples(W, H, hs, vs, y, x):
    """the (row, column) chroma samples libjpeg's up-sampling reads for pixel (y, x) of a W x H file whose luma is sampled hs x vs:
    the co-sited one and one neighbour per up-sampled direction, after the edge rules of the file's chroma plane"""
    wc, hc = -(-W // hs), -(-H // vs)
    if hs == 1 and vs == 1:
        return [(y, x)]
    if hs == 1:                                              # h1v2: rows, at any width
        cy = y >> 1
        far = min(cy + 1, hc - 1) if y & 1 else max(cy - 1, 0)
        return [(cy, x), (far, x)]
    j = x >> 1
    if wc <= 2:                                              # replication: the co-sited sample alone
        return [((y >> 1) if vs == 2 else y, j)]
    cols = [j]
    if x & 1 == 0 and j > 0:
        cols.append(j - 1)
    if x & 1 == 1 and j < wc - 1:
        cols.append(j + 1)
    if vs == 1:                                              # h2v1: columns
        return [(y, c) for c in cols]
    cy = y >> 1                                              # h2v2: the far row and columns j +- 1
    far = min(cy + 1, hc - 1) if y & 1 else max(cy - 1, 0)
    return [(r, c) for r in (cy, far) for c in cols]


def pixel_mcus(W, H, hs, vs, ncomp, luma=False):
    """int arrays [H, W] x0, x1, y0, y1: the first and last MCU column and row that pixel (y, x) reads a sample of"""
    if ncomp == 1:
        hs = vs = 1
    x0, x1, y0, y1 = (np.zeros((H, W), np.int64) for _ in range(4))
    for y in range(H):
        for x in range(W):
            mcus = [(y // (8 * vs), x // (8 * hs))]          # the luma sample is the pixel's own
            if ncomp == 3 and not luma:
                mcus += [(r // 8, c // 8) for r, c in chroma_samples(W, H, hs, vs, y, x)]      # chroma is 8 x 8 samples per MCU
            x0[y, x], x1[y, x] = min(m[1] for m in mcus), max(m[1] for m in mcus)
            y0[y, x], y1[y, x] = min(m[0] for m in mcus), max(m[0] for m in mcus)
    return x0, x1, y0, y1


def brute_window(pm, box):
    """the half-open MCU rectangle over the pixels of box, from pixel_mcus' arrays"""
    l, t, r, b = box
    x0, x1, y0, y1 = (a[t:b, l:r] for a in pm)
    return int(x0.min()), int(y0.min()), int(x1.max()) + 1, int(y1.max()) + 1


def all_boxes(W, H):
    return [(l, t, r, b) for l in range(W) for r in range(l + 1, W + 1) for t in range(H) for b in range(t + 1, H + 1)]


def random_boxes(W, H, count, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        l, t = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((l, t, int(rng.integers(l + 1, W + 1)), int(rng.integers(t + 1, H + 1))))
    return out


def forced_boxes(W=83, H=61):
    """the boxes every layout must get right at 83 x 61: the whole image, single pixels, edges on and beside an MCU boundary, strips"""
    out = [(0, 0, W, H)]
    out += [(x, y, x + 1, y + 1) for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (33, 27), (34, 28))]
    for e in (15, 16, 17, 31, 32, 33):                       # 16 and 32: MCU boundaries of every layout
        out += [(e, 3, W - 2, H - 3), (2, e, W - 3, H - 2), (1, 2, e, H - 1), (3, 1, W - 1, e)]
    out += [(0, y, W, y + 1) for y in (0, 15, 16, 17, 60)]
    out += [(x, 0, x + 1, H) for x in (0, 15, 16, 17, 82)]
    return out


def picture(H, W, seed=3):
    """saturated colours under noise (the luma tests' picture): chroma edges everywhere, so a wrong neighbour shows"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.stack([(x * 37) % 256, (y * 53 + x * 11) % 256, 255 - (x * 29 + y * 5) % 256], -1) + rng.integers(-60, 61, (H, W, 3)), 0, 255).astype(np.uint8)


def save(a, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", **kw)
    return buf.getvalue()


def make_file(layout, W, H, progressive=False, quality=90, seed=3):
    """a W x H file of `layout` ("444", "422", "420", "440", "grey") that Pillow wrote (4:4:0: a patched 4:2:2 file, jfif_440_reference)"""
    kw = dict(quality=quality, progressive=progressive)
    if layout == "grey":
        return save(picture(H, W, seed)[..., 1].copy(), **kw)
    if layout == "440":
        return F440.patch_440(save(picture(W, H, seed), subsampling="4:2:2", **kw))      # a H x W source: the patched file is W x H
    return save(picture(H, W, seed), subsampling={"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}[layout], **kw)


def pil_rgb(data):
    from PIL import Image
    return Image.open(io.BytesIO(data)).convert("RGB")


def pil_l(data):
    """the draft("L", None) image: libjpeg's grey output, the luma plane of a colour file"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("L", None)
    im.load()
    assert im.mode == "L"
    return im
