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
