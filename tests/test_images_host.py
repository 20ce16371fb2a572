"""Host: the intake the image-list calls share (adaptive_edge_aware_jpeg_amd/_images.py) -- the predicates, one_or_each and the layout
of the staging buffer.  No device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from adaptive_edge_aware_jpeg_amd import _images as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#                 value              number  int
PREDICATES = [(True,              False, False),
              (np.bool_(1),       False, False),
              (3,                 True,  True),
              (np.int32(3),       True,  True),
              (2.5,               True,  False),
              (np.float32(2.5),   True,  False),
              ("3",               False, False),
              (None,              False, False)]


@pytest.mark.parametrize("v,number,integer", PREDICATES, ids=[repr(p[0]) + type(p[0]).__name__ for p in PREDICATES])
def test_predicates(v, number, integer):
    assert I.is_number(v) is number
    assert I.is_int(v) is integer
    assert I.is_tensor(v) is False


def test_is_tensor_is_false_for_arrays_and_lists():
    assert I.is_tensor(np.zeros((2, 2), np.uint8)) is False
    assert I.is_tensor([1, 2]) is False and I.is_tensor((1, 2)) is False and I.is_tensor([np.zeros(3)]) is False


def test_import_needs_no_torch():
    """in a fresh interpreter: importing _images (and so the package) leaves torch unimported"""
    code = "import sys; import adaptive_edge_aware_jpeg_amd._images as I; assert I.is_tensor([]) is False; print('torch' in sys.modules)"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    assert r.stdout.strip().splitlines()[-1] == "False"


def test_one_or_each():
    seen = []

    def check(v, who):
        seen.append((v, who))
        return v * 2

    assert I.one_or_each(7, 3, check, "thing", "image") == [14, 14, 14]
    assert seen == [(7, "every image")]
    del seen[:]
    assert I.one_or_each([1, 2, 3], 3, check, "thing", "image") == [2, 4, 6]
    assert seen == [(1, "image 0"), (2, "image 1"), (3, "image 2")]
    del seen[:]
    assert I.one_or_each((5, 6), 2, check, "thing", "file") == [10, 12]
    assert seen == [(5, "file 0"), (6, "file 1")]
    for wrong in ([1, 2], (1, 2, 3, 4), []):
        with pytest.raises(ValueError) as e:
            I.one_or_each(wrong, 3, check, "thing", "image")
        assert str(e.value) == f"thing: {len(wrong)} entries for 3 images"
    with pytest.raises(ValueError) as e:
        I.one_or_each([1], 2, check, "resample", "file")
    assert str(e.value) == "resample: 1 entries for 2 files"

    def refuse(v, who):
        raise TypeError(f"{who}: no")

    with pytest.raises(TypeError, match="^every image: no$"):
        I.one_or_each(1, 2, refuse, "thing", "image")
    with pytest.raises(TypeError, match="^image 0: no$"):
        I.one_or_each([1, 2], 2, refuse, "thing", "image")


LAYOUTS = {"sizes 1 3 4 5, all on the host": ([1, 3, 4, 5], [True] * 4),
           "no items": ([], []),
           "one item": ([5], [True]),
           "an item of no bytes": ([1, 0, 3], [True] * 3),
           "all on the device": ([1, 3, 4, 5], [False] * 4),
           "interleaved, host first": ([1, 3, 4, 5, 7], [True, False, True, False, True]),
           "interleaved, device first": ([1, 3, 4, 5, 7], [False, True, False, True, True]),
           "host items between device items": ([5, 1, 3, 4], [False, True, True, False])}


@pytest.mark.parametrize("align", [1, 4])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_stage_layout(name, align):
    nbytes, on_host = LAYOUTS[name]
    before = (list(nbytes), list(on_host))
    offsets, total = I.stage_layout(nbytes, on_host, align)
    assert (nbytes, on_host) == before and len(offsets) == len(nbytes)
    assert all(o is None for o, h in zip(offsets, on_host) if not h)
    host = [(o, nb) for o, nb, h in zip(offsets, nbytes, on_host) if h]
    assert all(isinstance(o, int) and o >= 0 and o % align == 0 for o, _ in host)
    end = 0
    for o, nb in host:                       # input order, no overlap, no more than the alignment between two items
        assert end <= o < end + align
        end = o + nb
    assert end <= total < end + align and total % align == 0
    if not host:
        assert total == 0
    if align == 1:
        assert [o for o, _ in host] == [int(v) for v in np.cumsum([0] + [nb for _, nb in host])[:-1]]


def test_stage_layout_values():
    assert I.stage_layout([1, 3, 4, 5], [True] * 4) == ([0, 1, 4, 8], 13)
    assert I.stage_layout([1, 3, 4, 5], [True] * 4, 4) == ([0, 4, 8, 12], 20)
    assert I.stage_layout([1, 3, 4, 5], [True, False, True, True], align=4) == ([0, None, 4, 8], 16)


# ---- the refusals of the packed-image calls' intake ------------------------------------------------------------------------------------
# Every call, every place an image goes (the list, and for the two-image calls the second image and the mask), every fault below; the
# other arguments are good.  All of them are refused on the host, before a context exists.
def _view(shape, dtype=np.uint8):
    return np.broadcast_to(np.zeros((), dtype), shape)      # costs no memory


FAULTS = {"shape (4,)": lambda limit: _view((4,)),
          "shape (4, 5, 1)": lambda limit: _view((4, 5, 1)),
          "shape (4, 5, 5)": lambda limit: _view((4, 5, 5)),
          "shape (2, 2, 3, 1)": lambda limit: _view((2, 2, 3, 1)),
          "shape (0, 5, 3)": lambda limit: _view((0, 5, 3)),
          "shape (4, 0)": lambda limit: _view((4, 0)),
          "int16": lambda limit: _view((4, 5, 3), np.int16),
          "float32": lambda limit: _view((4, 5, 3), np.float32),
          "bool": lambda limit: _view((4, 5, 3), np.bool_),
          "a side above the limit": lambda limit: _view((1, limit + 1))}


def _calls():
    """name -> (call(images, second, mask), side limit, channels of a good image, the places besides the list)"""
    import adaptive_edge_aware_jpeg_amd as A
    from adaptive_edge_aware_jpeg_amd import adjust, compose, filters, geometry
    return {"filter_many": (lambda im, s, m: filters.filter_many(im, filters.MedianFilter(3)), 65535, 3, ()),
            "transform_many": (lambda im, s, m: geometry.transform_many(im, (3, 2), "affine", (1, 0, 0, 0, 1, 0)), 32767, 3, ()),
            "rotate_many": (lambda im, s, m: geometry.rotate_many(im, 30), 32767, 3, ()),
            "transpose_many": (lambda im, s, m: geometry.transpose_many(im, "rotate_90"), 32767, 3, ()),
            "adjust_many": (lambda im, s, m: adjust.adjust_many(im, adjust.Brightness(1.2)), 32767, 3, ()),
            "histogram_many": (lambda im, s, m: adjust.histogram_many(im), 32767, 3, ()),
            "paste_many": (lambda im, s, m: compose.paste_many(im, s, (0, 0), m), 32767, 3, ("second", "mask")),
            "alpha_composite_many": (lambda im, s, m: compose.alpha_composite_many(im, s), 32767, 4, ("second",)),
            "blend_many": (lambda im, s, m: compose.blend_many(im, s, 0.5), 32767, 3, ("second",)),
            "composite_many": (lambda im, s, m: compose.composite_many(im, s, m), 32767, 3, ("second", "mask")),
            "chop_many": (lambda im, s, m: compose.chop_many(im, s, "add"), 32767, 3, ("second",))}


def _refusal(call, *args):
    try:
        call(*args)
    except Exception as e:      # noqa: BLE001 (the table says which)
        return type(e).__name__, str(e)
    return None


def intake_refusals():
    """-> {"call / place / fault": (exception type name, message) or None}, in the table's order"""
    got = {}
    for name, (call, limit, channels, places) in _calls().items():
        good, good_mask = _view((4, 5, channels)), _view((4, 5))
        got[f"{name} / images / an empty list"] = _refusal(call, [], good, good_mask)
        for fault, make in FAULTS.items():
            got[f"{name} / images / {fault}"] = _refusal(call, [good, make(limit)], good, good_mask)
            if "second" in places:
                got[f"{name} / second / {fault}"] = _refusal(call, [good, good], [good, make(limit)], good_mask)
            if "mask" in places:
                got[f"{name} / mask / {fault}"] = _refusal(call, [good, good], good, [good_mask, make(limit)])
    return got


# recorded at the commit before _images.py took the intake over: the exception type and the whole message of every row
INTAKE_REFUSALS = {
    'filter_many / images / an empty list': ('ValueError', 'filter_many needs at least one image'),
    'filter_many / images / shape (4,)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'filter_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'filter_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'filter_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'filter_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'filter_many / images / shape (4, 0)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'filter_many / images / int16': ('TypeError', 'image 1: uint8 required, got int16'),
    'filter_many / images / float32': ('TypeError', 'image 1: uint8 required, got float32'),
    'filter_many / images / bool': ('TypeError', 'image 1: uint8 required, got bool'),
    'filter_many / images / a side above the limit': ('ValueError', 'image 1: sizes up to 65535 a side'),
    'transform_many / images / an empty list': ('ValueError', 'transform_many needs at least one image'),
    'transform_many / images / shape (4,)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'transform_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'transform_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'transform_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'transform_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'transform_many / images / shape (4, 0)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'transform_many / images / int16': ('TypeError', 'image 1: uint8 required, got int16'),
    'transform_many / images / float32': ('TypeError', 'image 1: uint8 required, got float32'),
    'transform_many / images / bool': ('TypeError', 'image 1: uint8 required, got bool'),
    'transform_many / images / a side above the limit': ('ValueError', 'image 1: sizes up to 32767 a side'),
    'rotate_many / images / an empty list': ('ValueError', 'rotate_many needs at least one image'),
    'rotate_many / images / shape (4,)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'rotate_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'rotate_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'rotate_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'rotate_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'rotate_many / images / shape (4, 0)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'rotate_many / images / int16': ('TypeError', 'image 1: uint8 required, got int16'),
    'rotate_many / images / float32': ('TypeError', 'image 1: uint8 required, got float32'),
    'rotate_many / images / bool': ('TypeError', 'image 1: uint8 required, got bool'),
    'rotate_many / images / a side above the limit': ('ValueError', 'image 1: sizes up to 32767 a side'),
    'transpose_many / images / an empty list': ('ValueError', 'transpose_many needs at least one image'),
    'transpose_many / images / shape (4,)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'transpose_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'transpose_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'transpose_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'transpose_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'transpose_many / images / shape (4, 0)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'transpose_many / images / int16': ('TypeError', 'image 1: uint8 required, got int16'),
    'transpose_many / images / float32': ('TypeError', 'image 1: uint8 required, got float32'),
    'transpose_many / images / bool': ('TypeError', 'image 1: uint8 required, got bool'),
    'transpose_many / images / a side above the limit': ('ValueError', 'image 1: sizes up to 32767 a side'),
    'adjust_many / images / an empty list': ('ValueError', 'adjust_many needs at least one image'),
    'adjust_many / images / shape (4,)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'adjust_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'adjust_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'adjust_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'adjust_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'adjust_many / images / shape (4, 0)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'adjust_many / images / int16': ('TypeError', 'image 1: uint8 required, got int16'),
    'adjust_many / images / float32': ('TypeError', 'image 1: uint8 required, got float32'),
    'adjust_many / images / bool': ('NotImplementedError', "image 1: images of mode '1' (bool) are not built"),
    'adjust_many / images / a side above the limit': ('ValueError', 'image 1: sizes up to 32767 a side'),
    'histogram_many / images / an empty list': ('ValueError', 'histogram_many needs at least one image'),
    'histogram_many / images / shape (4,)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'histogram_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'histogram_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'histogram_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'histogram_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'histogram_many / images / shape (4, 0)': ('ValueError', 'image 1: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'histogram_many / images / int16': ('TypeError', 'image 1: uint8 required, got int16'),
    'histogram_many / images / float32': ('TypeError', 'image 1: uint8 required, got float32'),
    'histogram_many / images / bool': ('NotImplementedError', "image 1: images of mode '1' (bool) are not built"),
    'histogram_many / images / a side above the limit': ('ValueError', 'image 1: sizes up to 32767 a side'),
    'paste_many / images / an empty list': ('ValueError', 'paste_many needs at least one image'),
    'paste_many / images / shape (4,)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'paste_many / second / shape (4,)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'paste_many / mask / shape (4,)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'paste_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'paste_many / second / shape (4, 5, 1)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'paste_many / mask / shape (4, 5, 1)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'paste_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'paste_many / second / shape (4, 5, 5)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'paste_many / mask / shape (4, 5, 5)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'paste_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'paste_many / second / shape (2, 2, 3, 1)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'paste_many / mask / shape (2, 2, 3, 1)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'paste_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'paste_many / second / shape (0, 5, 3)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'paste_many / mask / shape (0, 5, 3)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'paste_many / images / shape (4, 0)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'paste_many / second / shape (4, 0)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'paste_many / mask / shape (4, 0)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'paste_many / images / int16': ('TypeError', 'image 1: image: uint8 required, got int16'),
    'paste_many / second / int16': ('TypeError', 'image 1: overlay: uint8 required, got int16'),
    'paste_many / mask / int16': ('TypeError', 'image 1: mask: uint8 required, got int16'),
    'paste_many / images / float32': ('TypeError', 'image 1: image: uint8 required, got float32'),
    'paste_many / second / float32': ('TypeError', 'image 1: overlay: uint8 required, got float32'),
    'paste_many / mask / float32': ('TypeError', 'image 1: mask: uint8 required, got float32'),
    'paste_many / images / bool': ('NotImplementedError', "image 1: images of mode '1' (bool) are not built"),
    'paste_many / second / bool': ('NotImplementedError', "image 1: overlays of mode '1' (bool) are not built"),
    'paste_many / mask / bool': ('ValueError', 'image 1: mask: a bool mask is [h, w] with sizes from 1 to 32767, got shape (4, 5, 3)'),
    'paste_many / images / a side above the limit': ('ValueError', 'image 1: image: sizes up to 32767 a side'),
    'paste_many / second / a side above the limit': ('ValueError', 'image 1: overlay: sizes up to 32767 a side'),
    'paste_many / mask / a side above the limit': ('ValueError', 'image 1: mask: sizes up to 32767 a side'),
    'alpha_composite_many / images / an empty list': ('ValueError', 'alpha_composite_many needs at least one image'),
    'alpha_composite_many / images / shape (4,)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'alpha_composite_many / second / shape (4,)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'alpha_composite_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'alpha_composite_many / second / shape (4, 5, 1)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'alpha_composite_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'alpha_composite_many / second / shape (4, 5, 5)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'alpha_composite_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'alpha_composite_many / second / shape (2, 2, 3, 1)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'alpha_composite_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'alpha_composite_many / second / shape (0, 5, 3)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'alpha_composite_many / images / shape (4, 0)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'alpha_composite_many / second / shape (4, 0)': ('ValueError', 'image 1: overlay: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'alpha_composite_many / images / int16': ('TypeError', 'image 1: image: uint8 required, got int16'),
    'alpha_composite_many / second / int16': ('TypeError', 'image 1: overlay: uint8 required, got int16'),
    'alpha_composite_many / images / float32': ('TypeError', 'image 1: image: uint8 required, got float32'),
    'alpha_composite_many / second / float32': ('TypeError', 'image 1: overlay: uint8 required, got float32'),
    'alpha_composite_many / images / bool': ('NotImplementedError', "image 1: images of mode '1' (bool) are not built"),
    'alpha_composite_many / second / bool': ('NotImplementedError', "image 1: overlays of mode '1' (bool) are not built"),
    'alpha_composite_many / images / a side above the limit': ('ValueError', 'image 1: image: sizes up to 32767 a side'),
    'alpha_composite_many / second / a side above the limit': ('ValueError', 'image 1: overlay: sizes up to 32767 a side'),
    'blend_many / images / an empty list': ('ValueError', 'blend_many needs at least one image'),
    'blend_many / images / shape (4,)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'blend_many / second / shape (4,)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'blend_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'blend_many / second / shape (4, 5, 1)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'blend_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'blend_many / second / shape (4, 5, 5)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'blend_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'blend_many / second / shape (2, 2, 3, 1)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'blend_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'blend_many / second / shape (0, 5, 3)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'blend_many / images / shape (4, 0)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'blend_many / second / shape (4, 0)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'blend_many / images / int16': ('TypeError', 'image 1: image: uint8 required, got int16'),
    'blend_many / second / int16': ('TypeError', 'image 1: second image: uint8 required, got int16'),
    'blend_many / images / float32': ('TypeError', 'image 1: image: uint8 required, got float32'),
    'blend_many / second / float32': ('TypeError', 'image 1: second image: uint8 required, got float32'),
    'blend_many / images / bool': ('NotImplementedError', "image 1: images of mode '1' (bool) are not built"),
    'blend_many / second / bool': ('NotImplementedError', "image 1: second images of mode '1' (bool) are not built"),
    'blend_many / images / a side above the limit': ('ValueError', 'image 1: image: sizes up to 32767 a side'),
    'blend_many / second / a side above the limit': ('ValueError', 'image 1: second image: sizes up to 32767 a side'),
    'composite_many / images / an empty list': ('ValueError', 'composite_many needs at least one image'),
    'composite_many / images / shape (4,)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'composite_many / second / shape (4,)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'composite_many / mask / shape (4,)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'composite_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'composite_many / second / shape (4, 5, 1)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'composite_many / mask / shape (4, 5, 1)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'composite_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'composite_many / second / shape (4, 5, 5)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'composite_many / mask / shape (4, 5, 5)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'composite_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'composite_many / second / shape (2, 2, 3, 1)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'composite_many / mask / shape (2, 2, 3, 1)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'composite_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'composite_many / second / shape (0, 5, 3)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'composite_many / mask / shape (0, 5, 3)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'composite_many / images / shape (4, 0)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'composite_many / second / shape (4, 0)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'composite_many / mask / shape (4, 0)': ('ValueError', 'image 1: mask: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'composite_many / images / int16': ('TypeError', 'image 1: image: uint8 required, got int16'),
    'composite_many / second / int16': ('TypeError', 'image 1: second image: uint8 required, got int16'),
    'composite_many / mask / int16': ('TypeError', 'image 1: mask: uint8 required, got int16'),
    'composite_many / images / float32': ('TypeError', 'image 1: image: uint8 required, got float32'),
    'composite_many / second / float32': ('TypeError', 'image 1: second image: uint8 required, got float32'),
    'composite_many / mask / float32': ('TypeError', 'image 1: mask: uint8 required, got float32'),
    'composite_many / images / bool': ('NotImplementedError', "image 1: images of mode '1' (bool) are not built"),
    'composite_many / second / bool': ('NotImplementedError', "image 1: second images of mode '1' (bool) are not built"),
    'composite_many / mask / bool': ('ValueError', 'image 1: mask: a bool mask is [h, w] with sizes from 1 to 32767, got shape (4, 5, 3)'),
    'composite_many / images / a side above the limit': ('ValueError', 'image 1: image: sizes up to 32767 a side'),
    'composite_many / second / a side above the limit': ('ValueError', 'image 1: second image: sizes up to 32767 a side'),
    'composite_many / mask / a side above the limit': ('ValueError', 'image 1: mask: sizes up to 32767 a side'),
    'chop_many / images / an empty list': ('ValueError', 'chop_many needs at least one image'),
    'chop_many / images / shape (4,)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'chop_many / second / shape (4,)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4,)'),
    'chop_many / images / shape (4, 5, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'chop_many / second / shape (4, 5, 1)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 1)'),
    'chop_many / images / shape (4, 5, 5)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'chop_many / second / shape (4, 5, 5)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 5, 5)'),
    'chop_many / images / shape (2, 2, 3, 1)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'chop_many / second / shape (2, 2, 3, 1)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (2, 2, 3, 1)'),
    'chop_many / images / shape (0, 5, 3)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'chop_many / second / shape (0, 5, 3)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (0, 5, 3)'),
    'chop_many / images / shape (4, 0)': ('ValueError', 'image 1: image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'chop_many / second / shape (4, 0)': ('ValueError', 'image 1: second image: uint8 [H, W], [H, W, 2], [H, W, 3] or [H, W, 4] with at least one pixel required, got shape (4, 0)'),
    'chop_many / images / int16': ('TypeError', 'image 1: image: uint8 required, got int16'),
    'chop_many / second / int16': ('TypeError', 'image 1: second image: uint8 required, got int16'),
    'chop_many / images / float32': ('TypeError', 'image 1: image: uint8 required, got float32'),
    'chop_many / second / float32': ('TypeError', 'image 1: second image: uint8 required, got float32'),
    'chop_many / images / bool': ('NotImplementedError', "image 1: images of mode '1' (bool) are not built"),
    'chop_many / second / bool': ('NotImplementedError', "image 1: second images of mode '1' (bool) are not built"),
    'chop_many / images / a side above the limit': ('ValueError', 'image 1: image: sizes up to 32767 a side'),
    'chop_many / second / a side above the limit': ('ValueError', 'image 1: second image: sizes up to 32767 a side'),
}


def test_intake_refusals_are_the_recorded_ones():
    got = intake_refusals()
    assert list(got) == list(INTAKE_REFUSALS)
    wrong = {k: (got[k], INTAKE_REFUSALS[k]) for k in got if got[k] != INTAKE_REFUSALS[k]}
    assert not wrong, wrong
