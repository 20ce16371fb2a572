"""GPU: csrc/deflate.hip (k_lz_parse, k_lz_sizes, k_lz_scan, k_lz_emit) on coefficient arrays the codec never produces
(tests/deflate_input_catalogue.py, whose claims tests/test_deflate_inputs_host.py checks by brute force).  aej_deflate_histogram and
aej_deflate_batch are driven through ctypes on the test's own coefficient, counts and stream buffers; the stream buffer is pre-filled.
Every stream is read by ``zlib.decompress`` and by the plain reader tests/inflate_reference.py, whose trace gives the tokens the GPU
chose; from them the stream's size under either code is recomputed bit by bit (tests/deflate_stream_analysis.py) and compared."""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_input_catalogue as C
import deflate_reference as DT
import deflate_stream_analysis as SA
import inflate_reference as R

pytestmark = pytest.mark.gpu
GARBAGE = 0x5A5A5A5A                  # what the coefficient buffer holds beyond every count


class Env:
    def __init__(self, A):
        self.A = A
        self.codec = A.Jpeg(A.JpegCompressionSettings("YCbCr", (40, 80), (4, 64)))
        self.ctx = self.codec._bind()
        self.torch = self.ctx.torch

    def caps(self, H, W):
        p = self.ctx.plan(1, H, W)
        return [int((p.coeff_off[l + 1] if l < 2 else p.coeff_stride) - p.coeff_off[l]) for l in range(3)]

    def bound(self, raw_bytes):
        return int(self.ctx.lib.aej_deflate_stream_bound(ctypes.c_uint64(raw_bytes)))

    def run(self, slots, H=256, W=256, tables=None, adaptive=False, fill=0xA5, parse_first=False):
        """One aej_deflate_batch call over len(slots) / 3 images; slots[3 b + l] is the array of image b's layer l, or None (count 0).
        tables: [3][448] uint32 foreign tables; adaptive: aej_deflate_histogram, the library's tables from it, then the batch call on the
        parse it left (reuse_parse = 1); parse_first: the histogram call runs first although `tables` are given, and the batch call
        reuses its parse.  -> dict(streams, rows, sizes, hist, tables)"""
        ctx, t = self.ctx, self.torch
        assert len(slots) % 3 == 0
        B = len(slots) // 3
        p = ctx.plan(B, H, W)
        caps = self.caps(H, W)
        host = np.full(B * p.coeff_stride, GARBAGE, np.uint32).view(np.int32)
        counts = np.zeros((B, 3, 4), np.int64)
        for s, a in enumerate(slots):
            if a is None:
                continue
            b, l = divmod(s, 3)
            assert a.dtype == np.int32 and len(a) <= caps[l], (s, len(a), caps[l])
            o = b * p.coeff_stride + p.coeff_off[l]
            host[o:o + len(a)] = a
            counts[b, l, 0] = len(a)
        coeffs, d_counts = t.from_numpy(host).to(ctx.device), t.from_numpy(counts).to(ctx.device)
        nbytes = int(ctx.lib.aej_deflate_workspace_bytes(ctx.handle, B, H, W))
        ws = ctx.workspace(nbytes)
        hist = None
        reuse = 0
        if adaptive or parse_first:
            d_hist = t.full((3, DT.HIST_BINS), -7, dtype=t.int32, device=ctx.device)
            ctx.check(ctx.lib.aej_deflate_histogram(ctx.handle, coeffs.data_ptr(), d_counts.data_ptr(), B, H, W, d_hist.data_ptr(), ws.data_ptr(),
                                                    ctypes.c_uint64(nbytes)))
            hist = d_hist.cpu().numpy()
            reuse = 1
        if adaptive:
            h = np.ascontiguousarray(hist, dtype=np.int32)
            cover = np.zeros(3, np.int32)
            tables = np.empty((3, DT.TABLE_WORDS), np.uint32)
            assert ctx.lib.aej_deflate_build_tables(h.ctypes.data, cover.ctypes.data, tables.ctypes.data) == 0
        d_tables = None
        if tables is not None:
            tables = np.ascontiguousarray(tables, dtype=np.uint32)
            assert tables.shape == (3, DT.TABLE_WORDS)
            d_tables = t.from_numpy(tables.view(np.int32)).to(ctx.device)
        stride = (self.bound(4 * max(caps)) + 255) // 256 * 256
        d_streams = t.full((3 * B, stride), fill, dtype=t.uint8, device=ctx.device)
        d_sizes = t.full((3 * B,), -1, dtype=t.int64, device=ctx.device)
        ctx.check(ctx.lib.aej_deflate_batch(ctx.handle, coeffs.data_ptr(), d_counts.data_ptr(), B, H, W, d_tables.data_ptr() if d_tables is not None else None,
                                            reuse, d_streams.data_ptr(), ctypes.c_uint64(stride), d_sizes.data_ptr(), ws.data_ptr(), ctypes.c_uint64(nbytes)))
        rows, sizes = d_streams.cpu().numpy(), d_sizes.cpu().numpy()
        streams = [rows[s, :sizes[s]].tobytes() for s in range(3 * B)]
        for s in range(3 * B):                  # nothing beyond the stream's last word is touched
            assert 6 <= sizes[s] <= stride and np.all(rows[s, (sizes[s] + 3) // 4 * 4:] == fill), (s, int(sizes[s]))
        return dict(streams=streams, rows=rows, sizes=sizes, hist=hist, tables=tables)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as A
    return Env(A)


@pytest.fixture(scope="module")
def entries():
    return C.catalogue()


def pack(arrays, caps):
    """-> (images, slot of every array): each array in a layer slot that holds it, the larger arrays first"""
    free, where, B = [], [None] * len(arrays), 0
    for i in sorted(range(len(arrays)), key=lambda i: -len(arrays[i])):
        n = len(arrays[i])
        assert n <= max(caps)
        if not any(c >= n for c, _ in free):
            free += [(caps[l], 3 * B + l) for l in range(3)]
            B += 1
        k = min((k for k in range(len(free)) if free[k][0] >= n), key=lambda k: free[k][0])
        where[i] = free.pop(k)[1]
    return B, where


def in_slots(arrays, caps):
    B, where = pack(arrays, caps)
    slots = [None] * (3 * B)
    for i, s in enumerate(where):
        slots[s] = arrays[i]
    return slots, where


def block_kind(stream):
    """from the first bits: CMF / FLG valid with CINFO = 7, then BFINAL = 1 and the block type"""
    assert stream[0] == 0x78 and (stream[0] * 256 + stream[1]) % 31 == 0 and not stream[1] & 0x20
    assert stream[2] & 1, "the stream is one final block"
    return {1: "fixed", 2: "dynamic"}[(stream[2] >> 1) & 3]


def check_stream(env, name, arr, stream, table, traced=True):
    """assertions 1, 2, 3 and 8 of the module's contract on one stream -> (trace, tokens, kind); trace and tokens None if not traced"""
    raw = arr.tobytes() if arr is not None else b""
    try:
        back = zlib.decompress(stream)
    except zlib.error as err:
        pytest.fail(f"{name}: zlib refuses the stream of {len(stream)} bytes: {err}")
    assert back == raw, name
    assert len(stream) <= env.bound(len(raw)), (name, len(stream))
    kind = block_kind(stream)
    if table is None:
        assert kind == "fixed", name
    if not traced:
        return None, None, kind
    out, status, tr = R.inflate_traced(stream)
    assert status == R.OK and len(out) == len(raw) and out == raw, (name, status)
    assert tr.cinfo == 7 and tr.blocks == [kind], (name, tr.cinfo, tr.blocks)
    tokens = SA.tokens_of(tr, out)
    want_kind, want_size = SA.expected_kind(tokens, table)
    print(f"{name}: {len(raw)} -> {len(stream)} bytes {kind}; fixed {SA.fixed_bits(tokens)} bits, table {SA.table_bits(tokens, table) if table is not None else None}")
    assert (kind, len(stream)) == (want_kind, want_size), (name, kind, len(stream), want_kind, want_size)
    return tr, tokens, kind


def check_plants(entry, tr):
    """every plant the parser is expected to take is in the stream as exactly that match"""
    got = set(tr.matches)                     # (distance, length, output position)
    missing = []
    for p in entry.claims.get("plants", ()):
        length, distance, at = C.token_bytes(p)
        if p.taken and (distance, length, at) not in got:
            missing.append(p)
    assert not missing, (entry.name, missing[:5], len(missing))


def check_coverage(group, traces):
    """assertion 5: what the union of the group's streams reached"""
    lens, dists = SA.reachable_symbols(d_max=C.CHUNK - 2)      # (d = 8191 cannot be written: deflate_input_catalogue._distances)
    if group == "lengths":
        got = set().union(*(tr.len_pairs for tr in traces.values()))
        want = {(s, x) for s, (lo, hi) in lens.items() for x in (lo, hi)}
        assert want <= got, sorted(want - got)
        assert {s for s, _ in got} == set(lens), "a length symbol the token shapes cannot give"
        for name, lengths in (("lengths/A_near", (256, 252)), ("lengths/B_near", (255, 251)), ("lengths/A_far", (256, 252)), ("lengths/B_far", (255, 251))):
            assert set(lengths) <= {m[1] for m in traces[name].matches}, name
    if group == "distances":
        got = set().union(*(tr.dist_pairs for tr in traces.values()))
        want = {(s, x) for s, (lo, hi) in dists.items() for x in (lo, hi)}
        assert want <= got, sorted(want - got)
        assert {s for s, _ in got} <= set(dists)
        assert any(s == 29 and x & 4096 for s, x in got) and any(s == 28 and x & 4096 for s, x in got), "bit 12 of the 13-bit extras"
        assert (36, 64) in {m[:2] for m in traces["distances/grid"].matches}, "d = 9, the first distance beyond the near ones"
        # the chunk's last coefficient cannot be the destination of a far match (the chain is not walked for one coefficient)
        assert traces["distances/d8191"].matches == []
    if group == "literals":
        assert {8, 9} <= set().union(*(tr.lit_code_bits for tr in traces.values()))


def small(entries, group):
    return [e for e in entries if e.name.startswith(group + "/") and not e.claims.get("large")]


@pytest.mark.parametrize("group", C.GROUPS)
def test_fixed_code_catalogue(env, entries, group):
    """no table: every stream one final fixed block that reads back exactly, whose size is the size of its own tokens; the planted
    matches are taken and the group's coverage is reached; the whole group in ONE call"""
    es = small(entries, group)
    slots, where = in_slots([e.array for e in es], env.caps(256, 256))
    got = env.run(slots)
    traces = {}
    for e, s in zip(es, where):
        tr, tokens, kind = check_stream(env, e.name, e.array, got["streams"][s], None)
        check_plants(e, tr)
        traces[e.name] = tr
        if e.claims.get("no_match"):
            assert tr.matches == [] and len(got["streams"][s]) == SA.stream_bytes(SA.fixed_bits([("lit", b) for b in e.array.tobytes()])), e.name
        if e.name == "literals/high":
            assert len(got["streams"][s]) == C.literal_only_size(len(e.array)) == 74028
    for s in set(range(len(slots))) - set(where):
        check_stream(env, f"empty slot {s}", None, got["streams"][s], None)
    check_coverage(group, traces)


@pytest.mark.parametrize("group", C.GROUPS)
def test_adaptive_catalogue(env, entries, group):
    """aej_deflate_histogram, the library's tables from it, aej_deflate_batch on the same parse -- one image a call, so every stream has
    the table counted on itself: the histogram equals the stream's own symbol counts in every bin, the code is the cheaper one, and the
    streams of lengths/, distances/ and runs/ are dynamic"""
    es = small(entries, group)
    slots, where = in_slots([e.array for e in es], env.caps(256, 256))
    name_of = {s: e for e, s in zip(es, where)}
    traces = {}
    for b in range(len(slots) // 3):
        got = env.run(slots[3 * b:3 * b + 3], adaptive=True)
        assert np.all(got["hist"][:, 316:] == 0)
        for l in range(3):
            e = name_of.get(3 * b + l)
            name = e.name if e else f"empty slot {3 * b + l}"
            tr, tokens, kind = check_stream(env, name, e.array if e else None, got["streams"][l], got["tables"][l])
            counts = SA.symbol_counts(tr)
            if e is None or len(e.array) == 0:
                assert counts[256] == 1 and counts.sum() == 1
                counts[256] = 0                        # the histogram counts an end of block where a stream has a last chunk
            assert np.array_equal(got["hist"][l], counts), (name, np.nonzero(got["hist"][l] != counts)[0][:8])
            if e is not None:
                check_plants(e, tr)
                traces[e.name] = tr
                if group in ("lengths", "distances", "runs") and len(e.array):
                    assert kind == "dynamic", name
    check_coverage(group, traces)


@pytest.mark.parametrize("H,W,cap", ((256, 256, 65536), (192, 320, 61440)))
def test_layers_filled_to_capacity(env, entries, H, W, cap):
    """a whole number of chunks and seven and a half: read back by zlib alone (the plain reader would take minutes), within the bound,
    the incompressible high-byte array at exactly nine bits a byte, and never larger with its own table than without"""
    caps = env.caps(H, W)
    assert caps[0] == cap
    es = [e for e in entries if e.claims.get("large") and len(e.array) == cap]
    assert len(es) == (7 if cap == 65536 else 6)
    slots = [x for e in es for x in (e.array, None, None)]
    fixed = env.run(slots, H, W)
    for k, e in enumerate(es):
        check_stream(env, e.name, e.array, fixed["streams"][3 * k], None, traced=False)
        if e.name == "literals/high_capacity":
            assert len(fixed["streams"][3 * k]) == C.literal_only_size(cap)
        if e.claims.get("no_match"):
            assert len(fixed["streams"][3 * k]) == SA.stream_bytes(SA.fixed_bits([("lit", b) for b in e.array.tobytes()])), e.name
        own = env.run(slots[3 * k:3 * k + 3], H, W, adaptive=True)
        check_stream(env, e.name, e.array, own["streams"][0], own["tables"][0], traced=False)
        assert len(own["streams"][0]) <= len(fixed["streams"][3 * k]), e.name
        n_lit = int(own["hist"][0, :256].sum())
        assert own["hist"][0, 256] == 1 and (n_lit == 4 * cap if e.claims.get("no_match") else n_lit < 4 * cap)


def test_foreign_tables(env):
    """tables counted elsewhere: a stream that needs a symbol the table lacks (one length, one distance, end of block) is written with
    the fixed code, 15-bit literal codes lose on incompressible data, a tie goes to the fixed code and one bit less to the table"""
    for name, arr, table, expect in C.tables_catalogue(DT.adaptive_table):
        for reuse in (False, True):
            got = env.run([arr, None, None], tables=np.stack([table] * 3), parse_first=reuse)
            tr, tokens, kind = check_stream(env, name, arr, got["streams"][0], table)
            if expect is not None:
                assert kind == expect, (name, kind)
            need = {"tables/no_length_270": 270, "tables/no_distance_10": 286 + 10, "tables/no_length_284_on_zeros": 284,
                    "tables/no_distance_3_on_zeros": 286 + 3}.get(name)
            if need is not None:               # the stream does need the one symbol the table lacks
                assert SA.symbol_counts(tr)[need] > 0 and SA.table_bits(tokens, table) is None, name
            if name == "tables/no_length_270_unneeded":
                assert kind == "dynamic"
            for l in (1, 2):
                check_stream(env, f"{name}: empty layer {l}", None, got["streams"][l], table)


def subset(entries, cap, n=24):
    """a mixed subset that fits the smallest layer: some of every group"""
    names = ["lengths/A_near", "lengths/B_near", "lengths/A_far", "lengths/B_far", "distances/grid", "literals/every_byte_every_lane", "runs/constant_00000000",
             "runs/constant_80000000", "runs/period_7", "runs/period_65", "runs/trailing_zeros", "ends/zeros_0", "ends/random_1", "ends/nomatch_3",
             "ends/ones_63", "ends/random_65", "ends/nomatch_128", "ends/random_8191", "ends/nomatch_8193", "ends/ones_8256", "ends/random_8257",
             "adler/top5_8193", "borders/chunk", "borders/sub_block", "ends/zeros_64", "ends/nomatch_127", "runs/period_2"]
    by = {e.name: e for e in entries}
    out = [by[k] for k in names if len(by[k].array) <= cap][:n]
    return out


def test_bytes_do_not_depend_on_what_the_buffer_held(env, entries):
    """assertion 6: the same bytes into a buffer of 0x00, 0xFF and 0xA5, under the fixed code and under a common complete table"""
    caps = env.caps(256, 256)
    es = subset(entries, min(caps))
    slots = [e.array for e in es] + [None] * (-len(es) % 3)
    other = C.filling("random", 5000, 9)
    table = DT.adaptive_table(np.bincount(other.view(np.uint8), minlength=286)[:286], np.ones(30, np.int64), cover_all=True)
    for tables in (None, np.stack([table] * 3)):
        ref = env.run(slots, tables=tables, fill=0x00)
        for k, e in enumerate(es):
            assert zlib.decompress(ref["streams"][k]) == e.array.tobytes(), e.name
        for fill in (0xFF, 0xA5):
            got = env.run(slots, tables=tables, fill=fill)
            assert got["streams"] == ref["streams"], [e.name for e, a, b in zip(es, got["streams"], ref["streams"]) if a != b]
        if tables is not None:
            assert "dynamic" in {block_kind(s) for s in ref["streams"]} and "fixed" in {block_kind(s) for s in ref["streams"]}


def test_bytes_do_not_depend_on_the_call(env, entries):
    """assertion 7: twice the same call; the parse reused after a histogram call and made anew; an array alone and in a shuffled call
    of 24 streams; in layer 0, 1 and 2; in the first image and the last -- under the fixed code and a common complete table"""
    caps = env.caps(256, 256)
    es = subset(entries, min(caps))
    assert len(es) == 24
    other = C.filling("random", 5000, 9)
    table = DT.adaptive_table(np.bincount(other.view(np.uint8), minlength=286)[:286], np.ones(30, np.int64), cover_all=True)
    order = np.random.default_rng(1).permutation(24)
    for tables in (None, np.stack([table] * 3)):
        slots = [e.array for e in es]
        ref = env.run(slots, tables=tables)["streams"]
        assert env.run(slots, tables=tables)["streams"] == ref
        assert env.run(slots, tables=tables, parse_first=True)["streams"] == ref
        shuffled = env.run([slots[i] for i in order], tables=tables)["streams"]
        assert [shuffled[int(np.nonzero(order == i)[0][0])] for i in range(24)] == ref      # (every array moved to another layer and image)
        for k in (0, 4, 17, 23):
            for l in range(3):
                alone = env.run([slots[k] if j == l else None for j in range(3)], tables=tables)["streams"]
                assert alone[l] == ref[k], (es[k].name, l)
        first_last = env.run([slots[5], None, None] + [None] * 9 + [None, None, slots[5]], tables=tables)["streams"]
        assert first_last[0] == first_last[-1] == ref[5]


def test_package_entry_gives_the_same_bytes(env, entries):
    """assertion 9: Jpeg.deflate_batch on an EncodedBatch whose tensors hold a mixed subset, against the C entry"""
    t = env.torch
    caps = env.caps(256, 256)
    es = subset(entries, min(caps), 6)
    enc = env.codec.compress_batch(np.full((2, 256, 256, 3), 0.5, np.float32))
    p = enc.plan
    host = np.full(2 * p.coeff_stride, GARBAGE, np.uint32).view(np.int32)
    counts = enc.counts.cpu().numpy().copy()
    for s, e in enumerate(es):
        b, l = divmod(s, 3)
        o = b * p.coeff_stride + p.coeff_off[l]
        host[o:o + len(e.array)] = e.array
        counts[b, l, 0] = len(e.array)
    enc.coeffs.copy_(t.from_numpy(host).to(enc.coeffs.device))
    enc.counts.copy_(t.from_numpy(counts).to(enc.counts.device))
    enc._counts_host = None
    slots = [e.array for e in es]
    other = C.filling("random", 5000, 9)
    table = np.stack([DT.adaptive_table(np.bincount(other.view(np.uint8), minlength=286)[:286], np.ones(30, np.int64), cover_all=True)] * 3)
    for kw, mine in ((dict(adaptive=False), dict()), (dict(adaptive=True), dict(adaptive=True)), (dict(tables=table), dict(tables=table))):
        pkg = env.codec.deflate_batch(enc, **kw)
        got = env.run(slots, **mine)["streams"]
        assert [bytes(x) for im in pkg for x in im] == got, kw
        for e, s in zip(es, got):
            assert zlib.decompress(s) == e.array.tobytes()
