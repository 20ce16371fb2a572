"""CPU: the deflate stream catalogue (tests/deflate_stream_catalogue.py) against ``zlib.decompress`` and the plain reader
(tests/inflate_reference.py), and the coverage the catalogue claims, asserted from the reader's traces.  No GPU and no part of the package:
this is the check of the inputs and of the reference that tests/test_gpu_inflate_streams.py then holds csrc/inflate.hip against."""
import functools
import zlib

import pytest

import deflate_stream_catalogue as C
import deflate_stream_writer as W
import inflate_reference as R


@functools.lru_cache(maxsize=None)
def traced(name):
    return R.inflate_traced(C.by_name(name).data)


def traces(prefix=""):
    return [(c.name, traced(c.name)[2]) for c in C.catalogue() if c.name.startswith(prefix)]


def union(attr, prefix=""):
    out = set()
    for _, t in traces(prefix):
        out |= set(getattr(t, attr))
    return out


def test_every_valid_case_is_what_zlib_and_the_reference_read():
    for c in C.catalogue():
        got, status, _ = traced(c.name)
        assert status == R.OK, (c.name, status)
        assert zlib.decompress(c.data) == got, c.name
        assert got == c.payload, c.name


def test_every_malformed_case_is_refused_with_its_status():
    for b in C.malformed():
        with pytest.raises(zlib.error):
            zlib.decompress(b.data)
        assert R.inflate(b.data)[1] == b.status, b.name
    assert sorted({b.status for b in C.malformed()}) == [3, 4, 5, 6]
    assert len(C.malformed()) >= 16


def test_the_writer_writes_what_zlib_writes_where_both_can():
    """the writer's own Adler-32 and header against zlib's, and a stored stream against zlib level 0"""
    data = bytes(range(256)) * 37
    assert W.adler32(data) == zlib.adler32(data) and W.adler32(b"") == 1
    assert W.write([W.stored(data)], cinfo=7, flevel=0)[0] == zlib.compress(data, 0)


def test_every_strict_prefix_is_truncated():
    lengths = set()
    kinds = set()
    for name in C.PREFIX_CASES:
        c = C.by_name(name)
        assert 0 < len(c.data) < 200, (name, len(c.data))
        kinds |= set(traced(name)[2].blocks)
        for n in range(len(c.data)):
            with pytest.raises(zlib.error):
                zlib.decompress(c.data[:n])
            got, status = R.inflate(c.data[:n])
            assert status == R.TRUNCATED, (name, n, status)
            assert c.payload.startswith(got), (name, n)
            lengths.add(n)
    assert kinds == {"stored", "fixed", "dynamic"}
    assert {6, 7} <= lengths                                          # the stream lengths below the shortest valid stream
    assert max(max(t) for t in traced("prefix/dynamic_long")[2].lit_lengths) == 15
    assert min(traced("prefix/dynamic_long")[2].lit_code_bits) >= 11


def test_size_caps():
    total = 0
    for c in C.catalogue():
        assert len(c.payload) <= C.MAX_STREAM_OUT, c.name
        total += len(c.payload)
    assert total <= C.MAX_TOTAL_OUT, total


# ---------------------------------------------------------------------------------------------------------------- coverage, from traces
def test_coverage_header():
    seen = {(t.cinfo, t.flevel) for _, t in traces("header/")}
    assert seen == {(c, f) for c in range(8) for f in range(4)}
    for _, t in traces("header/"):
        assert max(d for d, _, _ in t.matches) == 256 << t.cinfo       # the whole declared window, and nothing beyond it


def test_coverage_symbols():
    for group in ("symbols/fixed_all", "symbols/dynamic_all"):
        t = traced(group)[2]
        assert t.len_pairs >= {(c, e) for c in range(257, 286) for e in (0, (1 << W.LEN_EXTRA[c - 257]) - 1)}, group
        assert t.dist_pairs >= {(d, e) for d in range(30) for e in (0, (1 << W.DIST_EXTRA[d]) - 1)}, group
        assert {(285, 0), (284, 31)} <= t.len_pairs
        assert any(d == 32768 for d, _, _ in t.matches)
    assert any(d == p for d, _, p in traced("symbols/distance_equals_position")[2].matches)
    assert any(d == p == 32768 for _, t in traces() for d, _, p in t.matches)
    assert (284, 31) in traced("restream/alt258")[2].len_pairs and (285, 0) not in traced("restream/alt258")[2].len_pairs


def test_coverage_code_lengths():
    lit = {l for _, t in traces() for code in t.lit_lengths for l in code}
    dist = {l for _, t in traces() for code in t.dist_lengths for l in code}
    assert lit >= set(range(1, 16)) and dist >= set(range(1, 16))
    assert union("lit_code_bits") >= set(range(1, 16)) and union("dist_code_bits") >= set(range(1, 16))      # and codes of each length are read
    t = traced("litcode/ladder_1_to_15")[2]
    assert sorted(l for l in t.lit_lengths[0] if l) == list(range(1, 15)) + [15, 15] and t.lit_code_bits >= set(range(1, 16))
    t = traced("litcode/all_slow")[2]
    assert min(t.lit_code_bits) == 11 and max(t.lit_code_bits) == 15 and t.lit_code_bits == t.dist_code_bits == {11, 12, 13, 14, 15}
    assert traced("litcode/ten_and_eleven")[2].lit_code_bits == {10, 11}
    for name in ("litcode/eob_only", "blocks/empty_dynamic_final"):
        t = traced(name)[2]
        assert [l for l in t.lit_lengths[-1] if l] == [1] and t.lit_lengths[-1][256] == 1 and t.dist_lengths[-1] == [0]
    assert [l for l in traced("litcode/two_symbols")[2].lit_lengths[0] if l] == [1, 1]
    assert len(traced("litcode/hlit257")[2].lit_lengths[0]) == 257 and len(traced("litcode/hlit286")[2].lit_lengths[0]) == 286
    assert traced("litcode/hlit286")[2].lit_lengths[0][285] and (285, 0) in traced("litcode/hlit286")[2].len_pairs
    # distance codes
    t = traced("distcode/empty")[2]
    assert t.dist_lengths == [[0]] and not t.matches
    t = traced("distcode/one_code_0")[2]
    assert t.dist_lengths == [[1]] and {d for d, _, _ in t.matches} == {1} and {n for _, n, _ in t.matches} >= {3, 258}
    t = traced("distcode/one_code_29")[2]
    assert t.dist_lengths == [[0] * 29 + [1]] and {d for d, _ in t.dist_pairs} == {29} and (29, 8191) in t.dist_pairs
    t = traced("distcode/thirty_15bit")[2]
    assert sorted(t.dist_lengths[0]) == sorted(C.DIST30) and max(C.DIST30) == 15 and W.kraft(C.DIST30) == 1 << 15
    assert {d for d, _ in t.dist_pairs} == set(range(30)) and t.dist_code_bits == set(C.DIST30)
    assert len(traced("distcode/hdist30")[2].dist_lengths[0]) == 30
    assert traced("restream/one_code_distance")[2].dist_lengths == [[1]] and traced("restream/one_code_distance")[2].matches
    assert traced("restream/literal_only")[2].dist_lengths == [[0]]
    assert 15 in traced("restream/long_literal_codes")[2].lit_code_bits and 15 in traced("restream/long_distance_codes")[2].dist_code_bits


def test_coverage_code_length_code():
    reps = [x for _, t in traces() for x in t.repeats]
    counts = {(s, n) for s, n, _, _, _ in reps}
    assert counts >= {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)}
    assert traced("clcode/repeat_extremes")[2].repeats and {(s, n) for s, n, _, _, _ in traced("clcode/repeat_extremes")[2].repeats} >= \
        {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)}
    assert traced("clcode/cross_16")[2].crossing() == {16}
    assert traced("clcode/cross_17")[2].crossing() == {17}
    assert traced("clcode/cross_18")[2].crossing() == {18}
    after = {(s, last) for s, _, _, _, last in traced("clcode/cross_17")[2].repeats}
    assert {(16, 17), (16, 18)} <= after                               # a 16 right after a 17 and after an 18: it repeats a zero
    assert traced("clcode/cross_17")[2].lit_lengths[0][:23] == [0] * 23
    t = traced("clcode/sixteen_first_distance")[2]
    assert any(s == 16 and at == hlit for s, _, at, hlit, _ in t.repeats) and t.dist_lengths[0] == [2] * 4 and t.lit_lengths[0][-1] == 2
    hclen = {h for _, t in traces() for h, _ in t.cl_lengths}
    assert 5 in hclen and 19 in hclen and 4 not in hclen
    assert traced("clcode/hclen5")[2].cl_lengths[0][0] == 5 and traced("clcode/hclen19")[2].cl_lengths[0][0] == 19
    h, cl = traced("clcode/seven_bit")[2].cl_lengths[0]
    assert sorted(l for l in cl if l) == [1, 2, 3, 4, 5, 6, 7, 7] and cl[16] == 7 and cl[10] == 7
    t = traced("clcode/seven_bit")[2]
    assert any(s == 16 for s, _, _, _, _ in t.repeats) and 10 in t.lit_lengths[0]      # both 7-bit members are read
    assert max(traced("restream/cl_repeats")[2].cl_lengths[0][1]) == 7


def test_coverage_stored():
    st = [x for _, t in traces() for x in t.stored]
    assert {n for n, _, _, _ in st} >= set(C.STORED_LENS)
    for b in range(8):
        t = traced(f"stored/after_fixed_{b}")[2]
        assert t.blocks == ["fixed", "stored"] and t.stored[0][1] == (2 + b) % 8, (b, t.stored)
    assert {t.stored[0][1] for _, t in traces("stored/after_fixed_")} == set(range(8))
    t = traced("stored/empty_x300")[2]
    assert t.blocks == ["fixed"] + ["stored"] * 300 and all(n == 0 for n, _, _, _ in t.stored)
    t = traced("stored/across_32768")[2]
    assert any(p < 32768 < p + n for n, _, _, p in t.stored) and t.matches[0] == (32768, 258, 33000)
    assert {traced(f"stored/in_pos_{k}")[2].stored[-1][2] & 3 for k in range(4)} == {0, 1, 2, 3}
    assert all(traced(f"stored/in_pos_{k}")[2].stored[-1][0] > 64 for k in range(4))


def test_coverage_blocks():
    assert traced("blocks/empty_fixed_final")[2].blocks == ["fixed", "fixed"] and traced("blocks/empty_fixed_first")[2].blocks == ["fixed"] * 3
    assert traced("blocks/empty_dynamic_final")[2].blocks == ["fixed", "dynamic"]
    assert traced("blocks/empty_dynamic_first")[2].blocks == ["dynamic", "dynamic", "fixed"]
    assert traced("blocks/empty_only")[0] == b"" and len(traced("blocks/empty_only")[2].blocks) == 4
    t = traced("blocks/forty_mixed")[2]
    assert len(t.blocks) == 40 and set(t.blocks) == {"stored", "fixed", "dynamic"}
    assert len(traced("blocks/forty_mixed")[0]) < 40 * 13 and sum(1 for d, _, p in t.matches if d > 13) >= 10      # matches that leave their block
    assert len(set(traced("restream/block_mix")[2].blocks)) == 3 and len(traced("restream/block_mix")[2].blocks) > 20


def test_coverage_overlap():
    grid = {(d, n) for _, t in traces("overlap/") for d, n, _ in t.matches}
    assert grid >= {(d, n) for d in C.OVERLAP_DISTANCES for n in C.OVERLAP_LENGTHS}
    assert len(C.OVERLAP_DISTANCES) == 67 and set(range(1, 66)) | {127, 128} == set(C.OVERLAP_DISTANCES)
    # the source of every match has no period of half its length or less: a copy in the wrong phase gives other bytes
    for c in C.catalogue():
        if c.name.startswith("overlap/"):
            for d, n, p in traced(c.name)[2].matches:
                src = c.payload[p - d:p]
                assert not any(src[q:] == src[:-q] for q in range(1, d // 2 + 1)), (c.name, d)
    assert any(n > d for d, n, _ in traced("restream/overlap")[2].matches)


def test_coverage_boundaries():
    starts = {p for _, t in traces() for _, _, p in t.matches}
    assert {p % 256 for p in starts} >= {0, 1, 255}
    assert {p % 32768 for p in starts if p >= 32767} >= {32767, 0, 1}
    assert set(C.MATCH_STARTS) <= starts
    for p in C.MATCH_STARTS:
        for n in (258, 64, 129):
            assert traced(f"boundary/start{p}_len{n}")[2].matches[0][1:] == (n, p)
    sizes = {len(c.payload) for c in C.catalogue()}
    assert sizes >= set(C.OUTPUT_SIZES)
    for n in C.OUTPUT_SIZES:
        assert len(C.by_name(f"boundary/size{n}").payload) == n


def test_coverage_input():
    assert {len(C.by_name(f"input/bytes{n}").data) for n in range(8, 17)} == set(range(8, 17))
    assert {len(C.by_name(f"input/stored_bytes{n}").data) for n in range(11, 17)} == set(range(11, 17))
    assert {len(c.data) & 3 for c in C.catalogue() if c.name.startswith("input/")} == {0, 1, 2, 3}
    for n in (1, 3, 9):
        assert C.by_name(f"input/tail{n}").data.endswith(b"\xff" * n)
        body = C.by_name(f"input/tail{n}").data[:-n]
        assert zlib.decompress(body) == C.by_name(f"input/tail{n}").payload and R.inflate(body)[1] == R.OK


def test_restream_styles_carry_any_payload():
    for payload in (b"", b"a", bytes(300), bytes(range(256)) * 3 + b"abcabcabcabc" * 30):
        for style in C.STYLES:
            data = C.restream(payload, style)
            assert zlib.decompress(data) == payload and R.inflate(data) == (payload, R.OK), style
