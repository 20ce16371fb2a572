"""CPU: the span check of the packed-image entries (csrc/aej_spans.h -- aej_filter_batch, aej_window_batch, aej_resample_batch*,
aej_warp_batch, aej_adjust_batch / aej_histogram_batch and aej_compose_batch all refuse through it), compiled alone from the header the
library compiles (tests/native/spans_check.cpp prints its answers as a table) and compared with the rule as include/aej.h states it:

  * image by image, in the caller's order: first that image's sources outside the input ("source outside the input"), then its image
    outside the output ("image outside the output"), then its sources meeting the output ("source inside the output");
  * every range is half-open: a source may end where the output begins and begin where it ends;
  * the output's bounds are counted in its own elements (8 bytes for aej_histogram_batch), an overlap in bytes;
  * an image may have several sources (compose: base, overlay, mask): any of them trips the check."""
import os
import shutil
import subprocess

import pytest
from conftest import ROOT

FINE, SOURCE_OUTSIDE, IMAGE_OUTSIDE, SOURCE_INSIDE = 0, 1, 2, 3

# name -> (fault, image): worked out by hand from the rule
NAMED = {"source ends at src_bytes": (FINE, -1),
         "source one byte past src_bytes": (SOURCE_OUTSIDE, 0),
         "image ends at the output's end": (FINE, -1),
         "image one element past the output": (IMAGE_OUTSIDE, 0),
         "source ends at the output's first byte": (FINE, -1),
         "source begins after the output's last byte": (FINE, -1),
         "one byte of overlap, the source below": (SOURCE_INSIDE, 0),
         "one byte of overlap, the source above": (SOURCE_INSIDE, 0),
         "source wholly inside a larger output": (SOURCE_INSIDE, 0),
         "output inside the source span, meeting no image": (FINE, -1),
         "8-byte elements, source at the output + 2": (SOURCE_INSIDE, 0),       # a count in elements would end the output at + 2 and pass it
         "8-byte elements, source at the output + 15": (SOURCE_INSIDE, 0),
         "8-byte elements, source at the output + 16": (FINE, -1),
         "8-byte elements, source ends at the output": (FINE, -1),
         "8-byte elements, source ends one byte inside": (SOURCE_INSIDE, 0),
         "8-byte elements, third element": (IMAGE_OUTSIDE, 0),
         "image 0 outside the output, image 1 outside the input": (IMAGE_OUTSIDE, 0),       # the lower image's, whatever its kind
         "image 0 inside the output, image 1 outside the input": (SOURCE_INSIDE, 0),
         "image 0 fine, image 1 outside the output": (IMAGE_OUTSIDE, 1),
         "outside the input and outside the output": (SOURCE_OUTSIDE, 0),                    # the stated order within an image
         "outside the output and inside it": (IMAGE_OUTSIDE, 0),
         "outside the input and inside the output": (SOURCE_OUTSIDE, 0),
         "three reads, all fine": (FINE, -1),
         "three reads, the last outside the input": (SOURCE_OUTSIDE, 0),
         "three reads, the second outside the input": (SOURCE_OUTSIDE, 0),
         "three reads, the last inside the output": (SOURCE_INSIDE, 0),
         "three reads, the first inside the output": (SOURCE_INSIDE, 0),
         "two images of two reads, image 1's second outside": (SOURCE_OUTSIDE, 1),
         "image 0's second read inside, image 1's first outside": (SOURCE_INSIDE, 0)}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    """the program's table, compiled and run once: [(name, (src, src_bytes, dst, dst_elements, unit), reads, writes, (fault, image))]"""
    exe = str(tmp_path_factory.mktemp("spans") / "spans_check")
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), "g++")      # any host C++ compiler
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "spans_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = []
    for line in out.stdout.splitlines():
        call, answer = line.split(" -> ")
        name, buffers, reads, writes = call.split(" |")
        spans = [[tuple(int(v) for v in s.split(":")) for s in part.split()] for part in (reads, writes)]
        rows.append((name, tuple(int(v) for v in buffers.split()), spans[0], spans[1], tuple(int(v) for v in answer.split())))
    return rows


def rule(src, src_bytes, dst, dst_elements, unit, reads, writes):
    """the rule, from its statement"""
    for image, offset, elements in writes:
        mine = [(o, nb) for i, o, nb in reads if i == image]
        if any(o + nb > src_bytes for o, nb in mine):
            return SOURCE_OUTSIDE, image
        if offset + elements > dst_elements:
            return IMAGE_OUTSIDE, image
        out = range(dst, dst + dst_elements * unit)
        if any(set(range(src + o, src + o + nb)) & set(out) for o, nb in mine):
            return SOURCE_INSIDE, image
    return FINE, -1


def test_every_row_follows_the_rule(rows):
    assert len(rows) == len(NAMED) + 29 + 10
    for name, buffers, reads, writes, answer in rows:
        assert answer == rule(*buffers, reads, writes), (name, buffers, reads, writes)


def test_named_cases(rows):
    assert {name: answer for name, _, _, _, answer in rows if not name.startswith("sweep")} == NAMED


def test_sweeps(rows):
    about = [(b[0] - b[2], answer) for name, b, _, _, answer in rows if name == "sweep: the source about the output"]
    assert [at for at, _ in about] == list(range(-14, 15))
    assert all(answer == ((SOURCE_INSIDE, 0) if -12 < at < 12 else (FINE, -1)) for at, answer in about), about      # half-open on both sides
    sizes = {name: [(b[1] if "src" in name else b[3], answer) for n, b, _, _, answer in rows if n == name] for name in ("sweep: src_bytes", "sweep: dst_elements")}
    assert sizes["sweep: src_bytes"] == [(s, (SOURCE_OUTSIDE, 0) if s < 12 else (FINE, -1)) for s in range(10, 15)]
    assert sizes["sweep: dst_elements"] == [(s, (IMAGE_OUTSIDE, 0) if s < 12 else (FINE, -1)) for s in range(10, 15)]
