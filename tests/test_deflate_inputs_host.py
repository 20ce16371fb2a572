"""CPU: the input catalogue of the GPU deflate's tests (tests/deflate_input_catalogue.py) reaches what it claims -- every claim is checked by
a plain search that shares nothing with the generators -- and the stream analysis (tests/deflate_stream_analysis.py) gives back the tokens
and the exact sizes of streams written by two independent writers."""
import zlib

import numpy as np
import pytest

import deflate_input_catalogue as C
import deflate_reference as DT
import deflate_stream_analysis as SA
import deflate_stream_writer as W
import inflate_reference as R


@pytest.fixture(scope="module")
def entries():
    return C.catalogue()


def run_length(u, pos, q, start, end):
    """how many coefficients from pos + start on equal those from q + start on, not reading at or beyond `end`"""
    k = start
    while pos + k < end and u[pos + k] == u[q + k]:
        k += 1
    return k - start


def search(u, pos, lo, end):
    """every source q in lo .. pos - 1, nearest first -> (best A: (coefficients, d), best B: (coefficients behind the literal, d)) by length,
    the nearer source at equal length; B needs equal upper three bytes and counts from the next coefficient"""
    best_a, best_b = (0, 0), (-1, 0)
    for q in range(pos - 1, lo - 1, -1):
        if u[q] >> 8 != u[pos] >> 8:
            continue
        if u[q] == u[pos]:
            n = run_length(u, pos, q, 0, end)
            if n > best_a[0]:
                best_a = (n, pos - q)
        n = run_length(u, pos, q, 1, end)
        if n > best_b[0]:
            best_b = (n, pos - q)
    return best_a, best_b


def test_catalogue_has_every_group_and_is_seeded(entries):
    names = [e.name for e in entries]
    assert len(set(names)) == len(names)
    assert {n.split("/")[0] for n in names} == set(C.GROUPS)
    again = C.catalogue()
    assert all(np.array_equal(a.array, b.array) and a.array.dtype == np.int32 for a, b in zip(entries, again))
    sizes = {g: sum(1 for n in names if n.startswith(g + "/")) for g in C.GROUPS}
    print(sizes)
    assert sizes == dict(lengths=4, distances=2, literals=4, runs=12, ends=80, adler=10, borders=2)
    for kind in ("zeros", "ones", "random", "nomatch"):
        for n in C.SIZES + (65536, 61440):
            assert any(e.name.startswith(f"ends/{kind}_") and len(e.array) == n for e in entries), (kind, n)


def test_planted_matches_exist_and_nothing_longer_does(entries):
    """each plant, by a search over every source in its chunk: the planted length at the planted distance is the longest there is, of
    its own shape and of the other one, clipped to the sub-block -- and unclipped too unless the entry claims a longer window match"""
    n_plants = 0
    for e in entries:
        u = e.array.view(np.uint32).tolist()
        for p in e.claims.get("plants", ()):
            n_plants += 1
            lo, sub_end = p.pos // C.CHUNK * C.CHUNK, min(len(u), (p.pos // C.SUB + 1) * C.SUB)
            assert p.pos - p.d >= lo, (e.name, p)
            ends = [sub_end] if "window" in e.claims else [sub_end, len(u)]
            for end in ends:
                (la, da), (lb, db) = search(u, p.pos, lo, end)
                if p.kind == "A":
                    assert (la, da) == (p.L, p.d), (e.name, p, la, da)
                    assert 3 + 4 * lb <= 4 * la, (e.name, p, lb)
                else:
                    assert (lb, db) == (p.L, p.d) and la == 0, (e.name, p, la, lb, db)
                    assert (u[p.pos] ^ u[p.pos - p.d]) & 0xFF, (e.name, p)
            if p.kind == "A" and p.taken:
                assert 64 * p.L > C.dist_cost(4 * p.d), (e.name, p)      # (the parser's threshold for an A candidate)
            if not p.taken:
                assert p.why
        if "window" in e.claims:
            pos, L, d = e.claims["window"]
            (la, da), _ = search(u, pos, max(0, pos - C.CHUNK + 1), len(u))
            assert (la, da) == (L, d), (e.name, la, da)
    assert n_plants > 300


def test_distinct_and_byte_range_claims(entries):
    for e in entries:
        a = e.array
        if "bytes" in e.claims:
            b = a.view(np.uint8)
            assert b.min() >= e.claims["bytes"][0] and b.max() <= e.claims["bytes"][1], e.name
        if e.claims.get("no_match"):
            assert not e.claims.get("plants") and e.claims.get("distinct")
        if e.claims.get("distinct"):
            keep = np.ones(len(a), bool)
            for p in e.claims.get("plants", ()):
                keep[p.pos:p.pos + p.L + (p.kind == "B")] = False
            if "window" in e.claims:
                keep[e.claims["window"][0]:e.claims["window"][0] + e.claims["window"][1]] = False
            upper = a.view(np.uint32)[keep] >> 8
            assert len(np.unique(upper)) == len(upper), e.name
        if "constant" in e.claims:
            assert np.all(a == np.int32(e.claims["constant"]))
        if "period" in e.claims:
            p = e.claims["period"]
            assert np.array_equal(a[p:], a[:-p]) and len(np.unique(a[:p])) == p and all(not np.array_equal(a[k:], a[:-k]) for k in range(1, p))
        if "zeros" in e.claims:
            lo, hi = e.claims["zeros"]
            assert not a[lo:hi].any() and (lo == 0 or a[lo - 1]) and (hi == len(a) or a[hi])
        if "capacity" in e.claims:
            assert len(a) == e.claims["capacity"]
    lanes = next(e for e in entries if e.name == "literals/every_byte_every_lane").array.view(np.uint8).reshape(-1, 4)
    assert all(sorted(lanes[:, k].tolist()) == list(range(256)) for k in range(4))
    n = 2 * C.CHUNK + 65
    assert C.literal_only_size(n) == 74028 and len(next(e for e in entries if e.name == "literals/high").array) == n


def test_reachable_symbols_follow_from_the_rfc_tables(entries):
    lens, dists = SA.reachable_symbols()
    assert sorted(lens) == [257, 258, 261, 262, 265, 267] + list(range(269, 285)) and len(lens) == 22
    assert sorted(set(range(257, 286)) - set(lens)) == [259, 260, 263, 264, 266, 268, 285]
    assert sorted(dists) == [3] + list(range(5, 30))
    assert C.DIST_BASE == W.DIST_BASE
    # the distance grid holds both ends of every reachable symbol, up to d = 8190: 8191 is planted apart (distances/d8191)
    grid = C.distance_grid()
    for s, (lo, hi) in dists.items():
        d_lo, d_hi = (W.DIST_BASE[s] + lo) // 4, min((W.DIST_BASE[s] + hi) // 4, C.CHUNK - 2)
        assert d_lo in grid and d_hi in grid, (s, d_lo, d_hi)
    assert 9 in grid and any((4 * d - 16385) & 4096 for d in grid if 16385 <= 4 * d < 24577) and any((4 * d - 24577) & 4096 for d in grid if 4 * d >= 24577)
    planted = {p.d for e in entries if e.name.startswith("distances/") for p in e.claims["plants"]}
    assert set(grid) | {C.CHUNK - 1} <= planted
    # lengths/: every L of both shapes near, and far wherever the hash can see it
    for kind, Ls in (("A", range(1, 65)), ("B", range(0, 64))):
        for far in (False, True):
            e = next(x for x in entries if x.name == f"lengths/{kind}_{'far' if far else 'near'}")
            assert [p.L for p in e.claims["plants"]] == list(Ls)
            assert all((p.d > C.NEAR) == far and p.d <= 100 for p in e.claims["plants"])
            assert [p.L for p in e.claims["plants"] if not p.taken] == ([] if not far else [1] if kind == "A" else [0])


def some_payloads():
    rng = np.random.default_rng(3)
    return [b"", b"a", bytes(300), rng.integers(-3, 4, 700).astype(np.int32).tobytes(), bytes(range(256)) * 3 + bytes(600),
            C.filling("nomatch", 200).tobytes()]


def test_analysis_gives_back_tokens_and_sizes():
    """streams from deflate_reference.encode_tokens (fixed and adaptive tables) and from the stream writer (fixed blocks): tokens in =
    tokens out, computed bits = stream length, counts = the histogram of the tokens; `zlib.decompress` agrees on every stream"""
    for data in some_payloads():
        tokens = DT.greedy_tokens(data, window=600)
        hist = DT.histogram_of(tokens)
        tables = [("fixed", DT.fixed_table()), ("exact", DT.adaptive_table(hist[:286], hist[286:316], cover_all=False)),
                  ("cover", DT.adaptive_table(hist[:286], hist[286:316], cover_all=True))]
        for name, table in tables:
            stream = DT.encode_tokens(data, tokens, table)
            assert zlib.decompress(stream) == data
            out, status, tr = R.inflate_traced(stream)
            assert status == R.OK and out == data
            assert SA.tokens_of(tr, out) == tokens, name
            bits = SA.fixed_bits(tokens) if name == "fixed" else SA.table_bits(tokens, table)
            assert len(stream) == SA.stream_bytes(bits), (name, len(data))
            assert np.array_equal(SA.symbol_counts(tr), hist), name
            assert tr.blocks == (["fixed"] if name == "fixed" else ["dynamic"])
        wt = [W.lit(t[1]) if t[0] == "lit" else W.match_value(t[1], t[2]) for t in tokens]
        stream, payload = W.write([W.fixed(wt)])
        out, status, tr = R.inflate_traced(stream)
        assert payload == data and status == R.OK and SA.tokens_of(tr, out) == tokens
        assert len(stream) == SA.stream_bytes(SA.fixed_bits(tokens))
        assert SA.expected_kind(tokens, None) == ("fixed", len(stream))
    # a missing code is reported, not costed as free
    t = DT.adaptive_table(DT.histogram_of([("lit", 0)])[:286], np.zeros(30, np.int64), cover_all=False)
    assert SA.table_bits([("lit", 1)], t) is None and SA.table_bits([("match", 4, 4)], t) is None and SA.table_bits([("lit", 0)], t) is not None
    t[256] = 0
    assert SA.table_bits([("lit", 0)], t) is None
    # length 258 is symbol 285 (8 bits, no extra), 257 is symbol 284 with extra 30
    assert SA.fixed_bits([("match", 258, 1)]) == 10 + 8 + 5 and SA.fixed_bits([("match", 257, 1)]) == 10 + 8 + 5 + 5


def test_foreign_tables_are_what_they_are_named():
    cases = C.tables_catalogue(DT.adaptive_table)
    by = {c[0]: c for c in cases}
    nocode = lambda t: [s for s in range(316) if int(t[s]) >> 16 == 0]
    assert len(cases) == 12
    assert nocode(by["tables/no_length_284_on_zeros"][2]) == [284] and nocode(by["tables/no_distance_3_on_zeros"][2]) == [286 + 3]
    assert nocode(by["tables/no_length_270"][2]) == [270]
    assert nocode(by["tables/no_distance_10"][2]) == [286 + 10]
    assert nocode(by["tables/no_end_of_block"][2]) == [256]
    assert max(int(by["tables/literals_15_bits"][2][s]) >> 16 for s in range(256)) == 15
    assert nocode(by["tables/complete_from_other_array"][2]) == []
    # every table's header opens a block zlib accepts (the blanked end-of-block entry is still declared in the header)
    for name, arr, table, _ in cases:
        t = np.array(table).copy()
        if name == "tables/no_end_of_block":
            t[256] = DT.adaptive_table(np.ones(286, np.int64), np.ones(30, np.int64), cover_all=False)[256]
        usable = [s for s in range(256) if int(t[s]) >> 16]
        data = bytes(usable[:5])
        assert zlib.decompress(DT.encode_tokens(data, [("lit", b) for b in data], t)) == data, name
    # the tie: literal-only arrays, one bit either side of equality
    want = {"below": -1, "equal": 0, "above": 1}
    for k, d in want.items():
        name, arr, table, expect = by[f"tables/tie_{k}"]
        tokens = [("lit", b) for b in arr.tobytes()]
        assert SA.table_bits(tokens, table) - SA.fixed_bits(tokens) == d, name
        assert SA.expected_kind(tokens, table)[0] == expect == ("dynamic" if d < 0 else "fixed")
        upper = arr.view(np.uint32) >> 8
        assert len(np.unique(upper)) == len(upper)
