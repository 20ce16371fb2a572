"""NumPy model of Pillow's two-image operations -- Image.paste with every mask, Image.alpha_composite (the in-place form with dest and
source), Image.blend, Image.composite and ImageChops -- for uint8 images of 1 to 4 channels (L, LA, RGB, RGBA), and the catalogue of
cases and the exhaustive inputs the host and GPU tests share.  Nothing here calls PIL: test_compose_host.py pins the model to live
Pillow, the GPU tests pin the library to the model.

A case is a dict with "kind" and that call's arguments for ONE element:
    paste            base, overlay (an image, an int or a tuple), at, mask (None, "alpha", a bool array, a uint8 image)
    alpha_composite  base, overlay, dest, source
    blend            im1, im2, alpha
    composite        im1, im2, mask
    chop             im1, im2, op (a name, or (name, scale, offset) for add and subtract)

The wrong variant `split_division` of the masked paste (each product divided by 255 on its own), which test_compose_host.py shows to
differ from Pillow."""
import numpy as np

CHOPS = ("add", "subtract", "add_modulo", "subtract_modulo", "multiply", "screen", "lighter", "darker", "difference", "soft_light",
         "hard_light", "overlay")
PASTE_PAIRS = ((1, 1), (2, 2), (3, 3), (4, 4), (3, 4), (1, 2))          # (base channels, overlay channels) that are built
MASKS = ("none", "bit", "L", "LA", "RGBA", "alpha")


# ---- pieces ----------------------------------------------------------------------------------------------------------------------------
def _bands(a):
    return a[..., None] if a.ndim == 2 else a


def _like(r, a):
    return r[..., 0] if a.ndim == 2 else r


def div255(t):
    return ((t >> 8) + t) >> 8


def region(W, H, x, y, ow, oh, box=None):
    """the pixels of a W x H output that an ow x oh overlay with its pixel (0, 0) at (x, y) reaches through `box` (in the overlay's
    coordinates): -> (left, top, right, bottom), or None"""
    l, t, r, b = box if box is not None else (0, 0, ow, oh)
    x0, x1 = max(0, x + max(l, 0)), min(W, x + min(r, ow))
    y0, y1 = max(0, y + max(t, 0)), min(H, y + min(b, oh))
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else None


def mix(d, s, m, split_division=False):
    """Pillow's masked paste of int arrays: ONE division of the sum"""
    if split_division:
        return div255(d * (255 - m) + 128) + div255(s * m + 128)
    return div255(d * (255 - m) + s * m + 128)


def mask_kind(mask):
    if mask is None:
        return "none"
    if isinstance(mask, str):
        return "alpha"
    if mask.dtype == np.bool_:
        return "bit"
    return {2: "L", 3: {2: "LA", 4: "RGBA"}.get(mask.shape[-1])}[mask.ndim]


def paste(base, overlay, at=(0, 0), mask=None, split_division=False):
    out = _bands(base).astype(np.int64)
    H, W, C = out.shape
    if isinstance(overlay, np.ndarray):
        ov = _bands(overlay).astype(np.int64)
        oh, ow = ov.shape[:2]
    else:
        ov = None
        colour = np.array([overlay] if isinstance(overlay, int) else list(overlay), np.int64)
        if isinstance(mask, np.ndarray):
            oh, ow = mask.shape[:2]
        else:
            ow, oh = at[2] - at[0], at[3] - at[1]
    if len(at) == 4:
        assert (at[2] - at[0], at[3] - at[1]) == (ow, oh)
    x, y = at[0], at[1]
    reg = region(W, H, x, y, ow, oh)
    if reg is not None:
        x0, y0, x1, y1 = reg
        sy, sx = slice(y0 - y, y1 - y), slice(x0 - x, x1 - x)
        d = out[y0:y1, x0:x1]
        s = ov[sy, sx, :C] if ov is not None else np.broadcast_to(colour, d.shape)
        kind = mask_kind(mask)
        if kind == "none":
            r = s
        elif kind == "bit":
            r = np.where(mask[sy, sx, None], s, d)
        else:
            m = (ov if kind == "alpha" else _bands(mask).astype(np.int64))[sy, sx, -1:]
            if ov is None and kind == "L" and C in (2, 4):    # Pillow's fill_mask_L: a transparent base pixel takes the colour whole
                m = np.concatenate([np.where((m != 0) & (d[..., -1:] == 0), 255, m)] * (C - 1) + [m], axis=-1)
            r = mix(d, s, m, split_division)
        out[y0:y1, x0:x1] = r
    return _like(out.astype(np.uint8), base)


def alpha_pixels(d, s):
    """Image.alpha_composite of int arrays [..., C], C 2 or 4: the last band is alpha"""
    sa, da = s[..., -1:], d[..., -1:]
    outa = sa * 255 + da * (255 - sa)
    c1 = sa * 255 * 255 * 128 // np.maximum(outa, 1)
    c2 = 255 * 128 - c1
    colour = div255(s[..., :-1] * c1 + d[..., :-1] * c2 + (0x80 << 7)) >> 7
    r = np.concatenate([colour, div255(outa + 0x80)], axis=-1)
    return np.where(sa == 0, d, r)


def alpha_composite(base, overlay, dest=(0, 0), source=(0, 0)):
    out = base.astype(np.int64)
    H, W, C = out.shape
    ov = overlay.astype(np.int64)
    oh, ow = ov.shape[:2]
    box = tuple(source) + ((ow, oh) if len(source) == 2 else ())
    x, y = dest[0] - box[0], dest[1] - box[1]
    reg = region(W, H, x, y, ow, oh, box)
    if reg is not None:
        x0, y0, x1, y1 = reg
        out[y0:y1, x0:x1] = alpha_pixels(out[y0:y1, x0:x1], ov[y0 - y:y1 - y, x0 - x:x1 - x])
    return out.astype(np.uint8)


def blend(im1, im2, alpha):
    """Image.blend: float32 throughout, the product and the sum rounded separately, every band"""
    d, s = im1.astype(np.int32), im2.astype(np.int32)
    a = np.float32(alpha)
    t = d.astype(np.float32) + a * (s - d).astype(np.float32)
    if 0 <= a <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def composite(im1, im2, mask):
    return paste(im2, im1, (0, 0), mask)


def chop(im1, im2, op):
    name, scale, offset = (op if isinstance(op, tuple) else (op, 1.0, 0))
    h, w = min(im1.shape[0], im2.shape[0]), min(im1.shape[1], im2.shape[1])
    a, b = im1[:h, :w].astype(np.int64), im2[:h, :w].astype(np.int64)
    q = lambda n, k: np.where(n >= 0, n // k, -((-n) // k))      # noqa: E731  (C's division truncates)
    if name in ("add", "subtract"):
        t = ((a + b if name == "add" else a - b).astype(np.float32) / np.float32(scale) + np.float32(offset)).astype(np.int32)
        return np.clip(t, 0, 255).astype(np.uint8)
    r = {"multiply": lambda: a * b // 255, "screen": lambda: 255 - (255 - a) * (255 - b) // 255, "lighter": lambda: np.maximum(a, b),
         "darker": lambda: np.minimum(a, b), "difference": lambda: np.abs(a - b), "add_modulo": lambda: a + b, "subtract_modulo": lambda: a - b,
         "hard_light": lambda: np.where(b < 128, a * b // 127, 255 - q((255 - b) * (255 - a), 127)),
         "overlay": lambda: np.where(a < 128, a * b // 127, 255 - q((255 - a) * (255 - b), 127)),
         "soft_light": lambda: ((255 - a) * (a * b)) // 65536 + (a * (255 - (255 - a) * (255 - b) // 255)) // 255}[name]()
    return (r & 255).astype(np.uint8)


def model(case, **switch):
    k = case["kind"]
    if k == "paste":
        return paste(case["base"], case["overlay"], case["at"], case["mask"], **switch)
    if k == "alpha_composite":
        return alpha_composite(case["base"], case["overlay"], case["dest"], case["source"])
    if k == "blend":
        return blend(case["im1"], case["im2"], case["alpha"])
    if k == "composite":
        return composite(case["im1"], case["im2"], case["mask"])
    return chop(case["im1"], case["im2"], case["op"])


def signature(case):
    """(kind, base channels, overlay channels (0: a colour), mask kind or chop name): what BUILT lists"""
    ch = lambda a: 1 if a.ndim == 2 else a.shape[2]      # noqa: E731
    k = case["kind"]
    if k == "paste":
        ov = case["overlay"]
        return (k, ch(case["base"]), ch(ov) if isinstance(ov, np.ndarray) else 0, mask_kind(case["mask"]))
    if k == "alpha_composite":
        return (k, ch(case["base"]), ch(case["overlay"]), "none")
    if k == "blend":
        return (k, ch(case["im1"]), ch(case["im2"]), "none")
    if k == "composite":
        return (k, ch(case["im2"]), ch(case["im1"]), mask_kind(case["mask"]))
    return (k, ch(case["im1"]), ch(case["im2"]), case["op"][0] if isinstance(case["op"], tuple) else case["op"])


def built():
    """every combination the library builds"""
    rows = []
    for c, oc in PASTE_PAIRS + tuple((c, 0) for c in (1, 2, 3, 4)):
        rows += [("paste", c, oc, m) for m in MASKS if (m != "alpha" or oc in (2, 4)) and (m != "LA" or oc)]      # (Pillow refuses a colour through an LA mask)
    rows += [("composite", c, c, m) for c in (1, 2, 3, 4) for m in ("bit", "L", "LA", "RGBA")]
    rows += [("alpha_composite", c, c, "none") for c in (2, 4)] + [("blend", c, c, "none") for c in (1, 2, 3, 4)]
    rows += [("chop", c, c, op) for c in (1, 2, 3, 4) for op in CHOPS]
    return rows


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------------
def image(h, w, c, seed=0):
    """random uint8 [h, w] or [h, w, c]; an alpha band holds 0, 255 and values between"""
    rng = np.random.default_rng(1000 * seed + 100 * c + 7 * h + w)
    a = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if c in (2, 4):
        al = a[..., -1].reshape(-1)
        al[::5], al[1::7] = 0, 255
    return a[..., 0].copy() if c == 1 else a


def make_mask(kind, h, w, seed=0):
    if kind in ("none", "alpha"):
        return None if kind == "none" else "alpha"
    if kind == "bit":
        return np.random.default_rng(seed + 3 * h + w).integers(0, 2, (h, w)).astype(np.bool_)
    return image(h, w, {"L": 1, "LA": 2, "RGBA": 4}[kind], seed + 50)


# (name, base (h, w), overlay (h, w), at): where the region falls
GEOMETRIES = (
    ("inside", (20, 31), (5, 7), (4, 6)), ("left", (20, 31), (5, 7), (-3, 6)), ("top", (20, 31), (5, 7), (4, -2)),
    ("right", (20, 31), (5, 7), (27, 6)), ("bottom", (20, 31), (5, 7), (4, 17)), ("left and top", (20, 31), (5, 7), (-3, -2)),
    ("right and bottom", (20, 31), (5, 7), (27, 17)), ("outside right", (20, 31), (5, 7), (40, 3)), ("outside left", (20, 31), (5, 7), (-7, 0)),
    ("outside below", (20, 31), (5, 7), (3, 20)), ("1 x 1 overlay", (20, 31), (1, 1), (30, 19)), ("larger than the base", (9, 13), (30, 40), (-5, -8)),
    ("width 1", (6, 1), (3, 1), (0, 2)), ("width 3", (5, 3), (2, 2), (1, 1)), ("width 17", (7, 17), (3, 5), (13, 2)),
    ("width 61", (4, 61), (3, 17), (50, 1)), ("whole groups inside", (3, 64), (2, 33), (16, 0)), ("4-tuple", (20, 31), (5, 7), (4, 6, 11, 11)),
    ("same size", (16, 17), (16, 17), (0, 0)),
)
EVERY_GEOMETRY = (("paste", 3, 4, "alpha"), ("paste", 4, 4, "L"), ("paste", 1, 1, "none"), ("paste", 2, 2, "bit"), ("paste", 4, 0, "L"),
                  ("alpha_composite", 4, 4, "none"), ("alpha_composite", 2, 2, "none"))


def _colour(c, seed):
    v = [int(x) for x in np.random.default_rng(seed).integers(0, 256, c)]
    return v[0] if c == 1 else tuple(v)


def _paste_case(c, oc, m, geom, seed):
    name, (bh, bw), (oh, ow), at = geom
    return dict(kind="paste", base=image(bh, bw, c, seed), overlay=image(oh, ow, oc, seed + 1) if oc else _colour(c, seed),
                at=at if (oc or m != "none" or len(at) == 4) else tuple(at) + (at[0] + ow, at[1] + oh), mask=make_mask(m, oh, ow, seed), geometry=name)


def catalogue():
    cases, seed = [], 0
    for row in built():
        kind, c, oc, m = row
        geoms = GEOMETRIES if row in EVERY_GEOMETRY else (GEOMETRIES[seed % len(GEOMETRIES)],)
        for g in geoms:
            seed += 1
            name, (bh, bw), (oh, ow), at = g
            if kind == "paste":
                cases.append(_paste_case(c, oc, m, g, seed))
            elif kind == "composite":
                cases.append(dict(kind=kind, im1=image(bh, bw, c, seed), im2=image(bh, bw, c, seed + 1), mask=make_mask(m, bh, bw, seed), geometry=name))
            elif kind == "alpha_composite":
                source = (0, 0) if seed % 3 else (1, 0, ow + 2, oh) if seed % 2 else (min(2, ow - 1), min(1, oh - 1))
                cases.append(dict(kind=kind, base=image(bh, bw, c, seed), overlay=image(oh, ow, c, seed + 1), dest=tuple(at[:2]), source=source,
                                  geometry=name))
            elif kind == "blend":
                for alpha in (0.3, -0.7, 1.7):
                    cases.append(dict(kind=kind, im1=image(bh, bw, c, seed), im2=image(bh, bw, c, seed + 1), alpha=alpha, geometry=name))
            else:
                op = (m, 1.5, -20) if m in ("add", "subtract") and seed % 2 else m
                cases.append(dict(kind=kind, im1=image(bh, bw, c, seed), im2=image(oh, ow, c, seed + 1) if seed % 3 == 0 else image(bh, bw, c, seed + 1),
                                  op=op, geometry=name))
    cases.append(dict(kind="chop", im1=image(7, 5, 3, 1), im2=image(3, 9, 3, 2), op="add", geometry="5 x 7 and 9 x 3"))
    return cases


# ---- the exhaustive inputs -------------------------------------------------------------------------------------------------------------
CHOP_PARAMETERS = ((1.0, 0), (2.0, 0), (0.5, -10), (1.5, 7), (3.0, -100), (-2.0, 300))
BLEND_ALPHAS = (0, 1, 0.3, -0.7, 1.7, 1e-30)


def exhaustive_paste():
    """all 2^24 (d, s, m) triples in one 4096 x 4096 L paste"""
    y, x = np.mgrid[0:4096, 0:4096]
    return dict(kind="paste", base=(x & 255).astype(np.uint8), overlay=(y & 255).astype(np.uint8), at=(0, 0),
                mask=((x >> 8) | ((y >> 8) << 4)).astype(np.uint8))


def exhaustive_pair():
    """the 256 x 256 images of all (a, b)"""
    a, b = np.mgrid[0:256, 0:256]
    return a.astype(np.uint8), b.astype(np.uint8)


def exhaustive_chops():
    a, b = exhaustive_pair()
    ops = [op for op in CHOPS if op not in ("add", "subtract")] + [(n, s, o) for n in ("add", "subtract") for s, o in CHOP_PARAMETERS]
    return [dict(kind="chop", im1=a, im2=b, op=op) for op in ops]


def exhaustive_blends():
    a, b = exhaustive_pair()
    return [dict(kind="blend", im1=a, im2=b, alpha=alpha) for alpha in BLEND_ALPHAS]


def colour_pairs():
    """64 (overlay, base) colour pairs: all of 0, 1, 127, 128, 254, 255 against each other, and 28 random ones"""
    edge = (0, 1, 127, 128, 254, 255)
    rng = np.random.default_rng(11)
    return [(s, d) for s in edge for d in edge] + [tuple(int(v) for v in rng.integers(0, 256, 2)) for _ in range(28)]


def exhaustive_alpha(c):
    """all 65536 (sa, da) pairs, tiled over the 64 colour pairs (band k takes pair j + 7 k): a 256 x 16384 element of c channels"""
    pairs = colour_pairs()
    sa, da = np.mgrid[0:256, 0:256]
    base, over = np.zeros((256, 256 * 64, c), np.uint8), np.zeros((256, 256 * 64, c), np.uint8)
    for j in range(64):
        cols = slice(256 * j, 256 * j + 256)
        for k in range(c - 1):
            over[:, cols, k], base[:, cols, k] = pairs[(j + 7 * k) % 64]
        over[:, cols, -1], base[:, cols, -1] = sa, da
    return dict(kind="alpha_composite", base=base, overlay=over, dest=(0, 0), source=(0, 0))


# ---- the library's call for a list of cases of ONE kind ------------------------------------------------------------------------------------
def library_op(A, op):
    if isinstance(op, tuple):
        return (A.ChopAdd if op[0] == "add" else A.ChopSubtract)(op[1], op[2])
    return op


def call(A, cases, wrap=lambda a: a):
    """the library call for cases of one kind, one entry per image.  `wrap` is applied to every array"""
    w = lambda v: wrap(v) if isinstance(v, np.ndarray) else v      # noqa: E731
    k = cases[0]["kind"]
    assert all(c["kind"] == k for c in cases)
    if k == "paste":
        return A.paste_many([w(c["base"]) for c in cases], [w(c["overlay"]) for c in cases], [c["at"] for c in cases], [w(c["mask"]) for c in cases])
    if k == "alpha_composite":
        return A.alpha_composite_many([w(c["base"]) for c in cases], [w(c["overlay"]) for c in cases], [c["dest"] for c in cases],
                                      [c["source"] for c in cases])
    if k == "blend":
        return A.blend_many([w(c["im1"]) for c in cases], [w(c["im2"]) for c in cases], [c["alpha"] for c in cases])
    if k == "composite":
        return A.composite_many([w(c["im1"]) for c in cases], [w(c["im2"]) for c in cases], [w(c["mask"]) for c in cases])
    return A.chop_many([w(c["im1"]) for c in cases], [w(c["im2"]) for c in cases], [library_op(A, c["op"]) for c in cases])
