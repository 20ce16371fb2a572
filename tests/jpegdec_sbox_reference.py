"""What the tests of scaled_box= (standard_jpeg_decode_many) and of standard_jpeg_resized_crop_many share, none of it the code under
test: the brute-force MCU window of a box of the SCALED image, written per pixel from libjpeg's up-sampling rules at scale 2, 4 and 8;
the boxes; Pillow's drafted images; and the scale rule of the resized crop, worked by hand."""
import numpy as np

import jpeg_luma_reference as LR
import jpegdec_box_reference as R

LAYOUTS = R.LAYOUTS
SCALES = (2, 4, 8)


def scaled_size(W, H, s):
    return -(-W // s), -(-H // s)


def pixel_mcus(W, H, hs, vs, ncomp, s, luma=False):
    """int arrays [oh, ow] x0, x1, y0, y1: the first and last MCU column and row that pixel (y, x) of the image decoded at scale s
    reads a sample of.  With m = 8 // s luma samples per block side an MCU covers hs m x vs m scaled pixels.  libjpeg at that scale:
    4:4:4, one component, 4:2:0: the chroma IDCT gives the chroma at luma resolution, so the pixel reads its own MCU alone;
    4:2:2: m chroma columns per MCU, sample x >> 1; h2v1 fancy at scales 2 and 4 when the scaled chroma width (ow + 1) >> 1 exceeds 2:
        an even x also reads column j - 1 (unless j == 0), an odd x column j + 1 (unless j is the last); replication otherwise;
    4:4:0: m chroma rows per MCU, sample y >> 1; h1v2 fancy at scales 2 and 4, at any width: an even y also reads the row above
        (clamped to row 0), an odd y the row below (clamped to the last); replication at scale 8."""
    if ncomp == 1:
        hs = vs = 1
    m = 8 // s
    ow, oh = scaled_size(W, H, s)
    wc, hc = (ow + 1) >> 1, (oh + 1) >> 1
    x0, x1, y0, y1 = (np.zeros((oh, ow), np.int64) for _ in range(4))
    for y in range(oh):
        for x in range(ow):
            mcus = [(y // (vs * m), x // (hs * m))]
            if ncomp == 3 and not luma and (hs, vs) == (2, 1):
                j = x >> 1
                cols = [j]
                if s in (2, 4) and wc > 2:
                    if x % 2 == 0 and j > 0:
                        cols.append(j - 1)
                    if x % 2 == 1 and j < wc - 1:
                        cols.append(j + 1)
                mcus += [(y // m, c // m) for c in cols]
            if ncomp == 3 and not luma and (hs, vs) == (1, 2):
                cy = y >> 1
                rows = [cy]
                if s in (2, 4):
                    rows.append(min(cy + 1, hc - 1) if y % 2 else max(cy - 1, 0))
                mcus += [(r // m, x // m) for r in rows]
            x0[y, x], x1[y, x] = min(q[1] for q in mcus), max(q[1] for q in mcus)
            y0[y, x], y1[y, x] = min(q[0] for q in mcus), max(q[0] for q in mcus)
    return x0, x1, y0, y1


brute_window = R.brute_window
all_boxes = R.all_boxes


def forced_boxes(ow, oh, mw, mh):
    """the boxes every layout must get right in an ow x oh scaled image whose MCUs are mw x mh scaled pixels: the whole image, single
    pixels at the four corners and inside, an edge on and beside every MCU boundary (left / top edges, then right / bottom ones), and
    one-pixel strips"""
    out = [(0, 0, ow, oh)]
    out += [(x, y, x + 1, y + 1) for x, y in ((0, 0), (ow - 1, 0), (0, oh - 1), (ow - 1, oh - 1), (ow // 2, oh // 2), (ow // 2 + 1, oh // 2 - 1))]
    ex = sorted({e for b in range(mw, ow, mw) for e in (b - 1, b, b + 1) if 1 <= e <= ow - 1})
    ey = sorted({e for b in range(mh, oh, mh) for e in (b - 1, b, b + 1) if 1 <= e <= oh - 1})
    for k in range(max(len(ex), len(ey))):
        x, y = ex[k % len(ex)], ey[k % len(ey)]
        out += [(x, y, ow, oh), (0, 0, x, y)]
    out += [(0, y, ow, y + 1) for y in (0, oh // 2, oh - 1)]
    out += [(x, 0, x + 1, oh) for x in (0, ow // 2, ow - 1)]
    return out


def boxes_for(ow, oh, mw, mh, count, seed):
    forced = forced_boxes(ow, oh, mw, mh)
    assert len(forced) <= count, (len(forced), count)
    return forced + R.random_boxes(ow, oh, count - len(forced), seed)


def pil_drafted(data, mode, s):
    """Pillow's image after draft() has chosen scale s: RGB (a grey file converted), or for mode "L" the draft("L") image"""
    if mode == "L":
        return LR.draft(data, "L", s)
    return LR.draft(data, None, s).convert("RGB")


def crop_scale(box, size, gap):
    """the scale of a resized crop by its stated rule, worked by hand: 1 without a reducing_gap, else the largest of 8, 4, 2, 1 not
    above min(int(r - l) // int(w g), int(b - t) // int(h g)), 1 when a divisor is 0"""
    if gap is None:
        return 1
    l, t, r, b = box
    dw, dh = int(size[0] * gap), int(size[1] * gap)
    if dw == 0 or dh == 0:
        return 1
    ratio = min(int(r - l) // dw, int(b - t) // dh)
    for s in (8, 4, 2):
        if s <= ratio:
            return s
    return 1
