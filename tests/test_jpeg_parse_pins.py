"""CPU: the two JPEG marker parsers (aej_jpegdec_parse_host, aej_jpegprog_parse_host) against results recorded before they were
joined into one marker walk (tools/record_jpeg_parse_pins.py -> tests/golden/jpegparse/pins.json): return code, message text,
descriptor bytes and scan count of every case of a corpus of valid, cut, corrupted and hand-made files, through both parsers."""
import hashlib
import json

import pytest

from tools import record_jpeg_parse_pins as P


@pytest.fixture(scope="module")
def pins():
    with open(P.PINS) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases():
    return P.corpus()


def test_corpus_is_the_recorded_one(pins, cases):
    assert (pins["seed"], pins["mutations_per_file"]) == (P.SEED, P.MUTATIONS)
    assert len(cases) == pins["n_cases"] == len(pins["cases"])
    for (name, data), row in zip(cases, pins["cases"]):
        assert hashlib.sha256(data).hexdigest()[:12] == row[0], f"{name}: the case's bytes are not the recorded ones"


def test_every_recorded_message_has_a_case(pins):
    strings = pins["strings"]
    seen = {strings[row[k]] for row in pins["cases"] for k in (2, 5, 8) if row[k] is not None and strings[row[k]]}
    assert sorted(seen) == pins["messages"] and len(seen) == pins["n_messages"] > 40


def test_parsers_answer_as_recorded(pins, cases):
    from adaptive_edge_aware_jpeg_amd import _lib as L
    lib = L.load_library()
    strings = pins["strings"]
    fields = ("baseline rc", "baseline message", "baseline descriptor", "progressive query rc", "progressive query message",
              "progressive query frame", "progressive rc", "progressive message", "progressive frame and scans", "n_scans")
    for (name, data), row in zip(cases, pins["cases"]):
        want = [strings[v] if k in (1, 2, 4, 5, 7, 8) and v is not None else v for k, v in enumerate(row[1:])]
        got = P.parse_case(lib, L, data)
        for field, g, w in zip(fields, got, want):
            assert g == w, f"{name}: {field}: {g!r}, recorded {w!r}"
