"""GPU: the JPEG decoders (csrc/jpegdec.hip, csrc/jpegprog.hip) on conforming streams that no libjpeg encoder writes -- the catalogue of
tests/jpeg_stream_catalogue.py, every case of which tests/test_jpeg_streams_host.py holds against live Pillow.  Every file is built at
run time from seeds, decoded in one mixed call beside two ordinary Pillow files (nothing may leak between files), and compared exactly
with tests/scaled_decode_reference.decode: at the smallest subsequence length and at the default one, at every scale, as the luma plane,
through a box that cuts MCUs, and through the lossless transcoder."""
import io

import numpy as np
import pytest

import jpeg_stream_catalogue as C
import jpeg_stream_writer as Wr
from jpeg_adobe_reference import picture

pytestmark = pytest.mark.gpu
CASES = C.catalogue()
GROUPS = sorted({c.name.split("/")[0] for c in CASES})
SYNC_BATCH = 4                                         # kJdSyncBatch: rounds launched between two looks at the "changed" word


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _set_s(bits):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    get_context(0).set_option("jpegdec_subseq_bits", bits)


def _pil_save(x, **opts):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, "JPEG", **opts)
    return buf.getvalue()


def _pillow(data, scale=1, mode="RGB"):
    import jpeg_luma_reference as LR
    im = LR.draft(data, "L" if mode == "L" else None, scale)
    return np.asarray(im if mode == "L" else im.convert("RGB"))


@pytest.fixture(scope="module")
def ordinary():
    """two files as Pillow writes them, which travel in every call"""
    return [_pil_save(picture(37, 53, 3, seed=3), quality=85), _pil_save(picture(40, 33, 3, seed=4), quality=70, subsampling=0, progressive=True)]


def _decode(A, files, **kw):
    return [t.cpu().numpy() for t in A.standard_jpeg_decode_many(files, progressive=True, layout_440=True, **kw)]


def _mixed(cases, ordinary):
    """the cases' files with the two ordinary ones among them -> (files, index of each case's file, indices of the ordinary ones)"""
    files = [c.data for c in cases]
    files.insert(1, ordinary[0])
    files.append(ordinary[1])
    at = [0] + list(range(2, len(cases) + 1))
    return files, at, (1, len(files) - 1)


# Which slot kernels a call runs is decided per call (jpegdec.hip, jd_four): the plain ones (k_jd_init, k_jd_sync, k_jd_scan_slots,
# k_jd_write) unless one of its baseline files has three components under one table pair -- then the kFour ones, for every file of the
# call.  So every test here makes its calls per family: "plain" calls hold no such file, "uniform" calls hold nothing else from the
# catalogue (the two ordinary files ride along in both).  _family() asserts it from the descriptors the library's own parser writes.
FAMILIES = ("plain", "uniform")


def _of_family(cases, family):
    return [c for c in cases if ("uniform" in c.tags) == (family == "uniform")]


def _lib_uniform(A, data):
    try:
        d = A.standard_jpeg.parse_header(data, layout_440=True)
    except NotImplementedError:                                    # a progressive file: another decoder
        return False
    return d.ncomp == 3 and all(bytes(t[c]) == bytes(t[0]) for t in (d.dc, d.ac) for c in (1, 2))


def _family(A, files, family):
    assert any(_lib_uniform(A, f) for f in files) == (family == "uniform"), family


def _per_file(values, cases, at, n, other):
    out = [other] * n
    for c, i in zip(cases, at):
        out[i] = values(c) if callable(values) else values
    return out


GROUP_CALLS = [(g, f) for g in GROUPS for f in FAMILIES if _of_family([c for c in CASES if c.name.split("/")[0] == g], f)]


def test_both_kernel_families_meet_the_catalogue():
    """the plain kernels meet every group but the one made for the others, with every code shape, selector and restart interval in it"""
    plain = {g for g, f in GROUP_CALLS if f == "plain"}
    assert plain == set(GROUPS) - {"uniform"} and {g for g, f in GROUP_CALLS if f == "uniform"} >= {"uniform", "never", "segments", "selectors"}
    for group, least in (("shapes", 28), ("selectors", 10), ("segments", 20), ("never", 8)):
        assert sum(c.name.startswith(group + "/") and not c.progressive and "uniform" not in c.tags for c in CASES) >= least, group
    assert sum(c.name.startswith("shapes/") and c.layout != "grey" and not c.progressive and "uniform" not in c.tags for c in CASES) >= 28


@pytest.mark.parametrize("S", [32, 2048])
@pytest.mark.parametrize("group,family", GROUP_CALLS)
def test_catalogue_equals_the_reference(A, ordinary, group, family, S):
    cases = _of_family([c for c in CASES if c.name.split("/")[0] == group], family)
    files, at, pil = _mixed(cases, ordinary)
    _family(A, files, family)
    try:
        _set_s(S)
        got = _decode(A, files)
    finally:
        _set_s(2048)
    for c, i in zip(cases, at):
        ref = C.reference(c.data)
        assert got[i].dtype == np.uint8 and got[i].shape == ref.shape and np.array_equal(got[i], ref), (c.name, S)
    for k, i in enumerate(pil):
        assert np.array_equal(got[i], _pillow(ordinary[k])), ("ordinary", k, S)


def _rotation(stride, offset, family):
    """plain: every case with a 16-bit table or of the coefficient-reach class, and every stride-th of the rest; uniform: all of that family"""
    if family == "uniform":
        return _of_family(CASES, family)
    return _of_family([c for k, c in enumerate(CASES) if "large" not in c.tags and ("pq1" in c.tags or "reach" in c.tags or k % stride == offset)], family)


@pytest.mark.parametrize("S", [32, 2048])
@pytest.mark.parametrize("family", FAMILIES)
def test_scales(A, ordinary, family, S):
    cases = _rotation(5, 1, family)
    files, at, pil = _mixed(cases, ordinary)
    _family(A, files, family)
    try:
        _set_s(S)
        for turn in range(3):                                      # every file meets every scale
            scales = _per_file(lambda c: (2, 4, 8)[(len(c.name) + turn) % 3], cases, at, len(files), (2, 4, 8)[turn])
            got = _decode(A, files, scale=scales)
            for c, i in zip(cases, at):
                ref = C.reference(c.data, scales[i])
                assert got[i].shape == ref.shape and np.array_equal(got[i], ref), (c.name, scales[i], S)
            for k, i in enumerate(pil):
                assert np.array_equal(got[i], _pillow(ordinary[k], scales[i])), ("ordinary", k, scales[i])
    finally:
        _set_s(2048)


@pytest.mark.parametrize("family", FAMILIES)
def test_luma_mode(A, ordinary, family):
    cases = _rotation(5, 2, family)
    files, at, pil = _mixed(cases, ordinary)
    _family(A, files, family)
    scales = _per_file(lambda c: (1, 2, 4, 8)[len(c.name) % 4], cases, at, len(files), 1)
    got = _decode(A, files, scale=scales, mode="L")
    for c, i in zip(cases, at):
        ref = C.reference(c.data, scales[i], "L")
        assert got[i].shape == ref.shape and np.array_equal(got[i], ref), (c.name, scales[i])
    for k, i in enumerate(pil):
        assert np.array_equal(got[i], _pillow(ordinary[k], 1, "L"))


@pytest.mark.parametrize("S", [32, 2048])
@pytest.mark.parametrize("family", FAMILIES)
def test_box_that_cuts_mcus(A, ordinary, family, S):
    cases = [c for c in _rotation(5, 3, family) if C.reference(c.data).shape[0] >= 24]
    files, at, pil = _mixed(cases, ordinary)
    _family(A, files, family)

    def box(shape):
        h, w = shape[:2]
        return (3, 5, w - 7, h - 2)                                # no edge on a block boundary; skips the first and the last MCU row's top / bottom
    boxes = _per_file(lambda c: box(C.reference(c.data).shape), cases, at, len(files), None)
    for k, i in enumerate(pil):
        boxes[i] = box(_pillow(ordinary[k]).shape)
    try:
        _set_s(S)
        got = _decode(A, files, box=boxes)
    finally:
        _set_s(2048)
    for c, i in zip(cases, at):
        l, t, r, b = boxes[i]
        assert np.array_equal(got[i], C.reference(c.data)[t:b, l:r]), (c.name, S)
    for k, i in enumerate(pil):
        l, t, r, b = boxes[i]
        assert np.array_equal(got[i], _pillow(ordinary[k])[t:b, l:r])


@pytest.fixture(scope="module")
def never_rounds(A):
    """{name: sync rounds at S = 32} of the never-synchronising files, each decoded alone (and compared with the reference)"""
    rounds = {}
    try:
        _set_s(32)
        for c in CASES:
            if c.name.split("/")[0] == "never":
                (got,) = _decode(A, [c.data])                      # must not raise "did not settle"
                rounds[c.name] = A.standard_jpeg.decode_sync_rounds()
                assert np.array_equal(got, C.reference(c.data)), c.name
    finally:
        _set_s(2048)
    for name, r in sorted(rounds.items()):
        print("sync rounds at S = 32:", name, r)
    return rounds


def _segment_bits(A, data):
    d = A.standard_jpeg.parse_header(data)
    return (d.scan_length - 2 - 2 * (d.n_segments - 1)) * 8 // d.n_segments


def test_never_synchronising_files_settle(A, never_rounds):
    """A flat picture under a one-code AC table: after the first block every block is '00', so a guessed entry state never meets the true
    one by itself.  When the first block has an odd number of bits every guess sits in mid-block and the decode needs one sync round per
    subsequence of the (longest) segment; the twin with an even first block starts every guess on a block boundary and settles at once
    -- the 4:2:0 one too, whose guesses are still wrong in the block slot (12 bits per MCU against 32 per subsequence): its components
    share one table pair, so it goes through the kernels that take the slot from the block counts (JdFile::uniform).  Neither may raise
    "did not settle".  Measured on an MI355X at S = 32, odd / even: grey 96 x 80 8 / 1, grey 264 x 200 52 / 1, 4:2:0 96 x 80 12 / 1,
    4:2:0 264 x 200 84 / 1; with one restart segment per MCU row 0 / 0 (one subsequence per segment), 3 / 1, 3 / 1 and 7 / 1."""
    for c in CASES:
        if c.name.split("/")[0] != "never" or "odd" not in c.tags:
            continue
        bits = _segment_bits(A, c.data)
        assert never_rounds[c.name] >= bits // 32 - SYNC_BATCH, (c.name, never_rounds[c.name], bits)
        even = never_rounds[c.name.replace("/odd", "/even")]
        assert even < never_rounds[c.name] or (bits <= 32 and even == never_rounds[c.name] == 0), c.name      # one subsequence: no round at all


def test_transcode_reads_the_same_streams(A, ordinary):
    """the lossless transcoder decodes with the same entropy stages: its output, decoded by Pillow, is Pillow's decode of its input"""
    # not the 16-bit tables, which the transcoder's parser refuses, nor the chunk-boundary files, whose DC of 2047 no 8-bit encoder takes
    cases = [c for c in CASES if "pq1" not in c.tags and "large" not in c.tags and "chunk" not in c.tags]
    for family in FAMILIES:
        for progressive in (False, True):
            part = _of_family(cases, family)[progressive::2]
            files, at, pil = _mixed(part, ordinary)
            _family(A, files, family)
            out = A.standard_jpeg_transcode_many(files, progressive=progressive, grey=True, layout_440=True)
            assert len(out) == len(files)
            for c, i in zip(part, at):
                assert np.array_equal(_pillow(bytes(out[i])), C.reference(c.data)), (c.name, progressive)
            for k, i in enumerate(pil):
                assert np.array_equal(_pillow(bytes(out[i])), _pillow(ordinary[k]))


# ---- outside Pillow's reach ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 2, 4, 8])
def test_extreme_blocks_follow_the_c_arithmetic(A, ordinary, scale):
    """Coefficients of +-1023 under a 16-bit quantisation table of 65535 everywhere: dequantised terms of +-2^26, far outside what
    samples give and outside what Pillow shares with libjpeg's C code (its SIMD inverse DCTs wrap at 16 bits and saturate; see
    DESIGN.md).  So the reference here is the C arithmetic alone, in unbounded integers: tests/jfif_reference.idct and the int64
    idct_reduced with the masked range limit.  This is the test of the argument that jd_idct4_block and jd_idct2_block may keep pass 1
    modulo 2^32; it pins the present behaviour past the documented boundary."""
    rng = np.random.default_rng(1023)
    files = []
    for W, H in ((52, 40), (8, 8)):
        for q in (65535, 40000):
            files.append(Wr.write(W, H, Wr.extreme(rng, W, H, 1023), qtables=[(np.full(64, q), 1)], selectors=[(0, 0, 0)],
                                  dc_tables={0: Wr.chain(Wr.DC_SYMBOLS)}, ac_tables={0: Wr.spread(Wr.AC_SYMBOLS)}))
    got = _decode(A, files + ordinary, scale=scale)
    for k, f in enumerate(files):
        assert np.array_equal(got[k], C.reference(f, scale)), (k, scale)
    (luma,) = _decode(A, files[:1], scale=scale, mode="L")
    assert np.array_equal(luma, C.reference(files[0], scale, "L"))
    for k in range(2):
        assert np.array_equal(got[len(files) + k], _pillow(ordinary[k], scale))


def test_refusals_leave_the_other_files_alone(A, ordinary):
    """What the decoders do not take is refused before or without any fault, naming the file; the good files of the same call decode
    afterwards.  A DC difference of category 12 (Pillow decodes it: libjpeg takes up to 15): refused by the kernel when the file uses
    it.  A DC table that lists symbol 16, and a table whose last 16-bit code is all ones: refused by the parser, as libjpeg refuses both."""
    bad = C.refusal_files()
    good = [CASES[0].data, ordinary[0]]
    for name in ("dc12", "dc16", "all-ones"):
        with pytest.raises(ValueError, match="file 1"):
            _decode(A, [good[0], bad[name][0], good[1]])
        got = _decode(A, good)
        assert np.array_equal(got[0], C.reference(good[0])) and np.array_equal(got[1], _pillow(good[1])), name
    try:
        _set_s(32)
        with pytest.raises(ValueError, match="file 1"):
            _decode(A, [good[0], bad["dc12"][0], good[1]])
    finally:
        _set_s(2048)
