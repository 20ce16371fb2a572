"""GPU: what the JPEG C entries refuse, and in which words (csrc/api_jpeg.hip).  A characterisation test: every return code and every
aej_last_error text below was recorded from the library before the entries' option checks were folded into one routine, and pins
that routine to them -- the entry's own name in every message, the fault that wins when a call has two, the size query that answers
0 for the same options and leaves the context's last error alone, and the output and status buffers that no refusal touches.  No
case launches a kernel but the one accepted _sbox call per family, which is compared with the Python call."""
import ctypes

import numpy as np
import pytest

import jpeg_adobe_reference as AR
import jpegdec_box_reference as R

pytestmark = pytest.mark.gpu
WHOLE, EMPTY = (0, 0, 24, 16), (8, 8, 8, 9)
OUT_EACH = 24 * 16 * 4                                       # room for one image of any file here, four channels included
WS_BYTES = 1 << 20
ENTRIES = {"": 0, "_scaled": 1, "_mode": 2, "_box": 3, "_sbox": 3, "_adobe": 4}      # entry -> how many of (scales, comps, boxes, adobe) it takes
SENTINEL = "aej_jpegdec_batch: no files, or a descriptor aej_jpegdec_parse_host did not write"


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available()
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


def _arr(ctype, values):
    """(the ctypes array kept alive by the caller, its address) or (None, None)"""
    if values is None:
        return None, None
    flat = [int(v) for v in np.asarray(values).reshape(-1)]
    a = (ctype * len(flat))(*flat)
    return a, ctypes.addressof(a)


class _Base:
    def _setup(self):
        from adaptive_edge_aware_jpeg_amd._lib import get_context
        self.ctx = get_context(0)
        self.lib = self.ctx.lib

    def last_error(self):
        return self.lib.aej_last_error(self.ctx.handle).decode()

    def sentinel(self):
        """a failing call of another entry: the text a size query has to leave in place"""
        assert self.lib.aej_jpegdec_batch(self.ctx.handle, None, 0, None, 0, None, None, 0, None, None, None, 0) == -1
        assert self.last_error() == SENTINEL


class _Decoder(_Base):
    """n files of one decoder family staged for its C entries; out and status hold patterns"""

    def __init__(self, A, family, files):
        import torch
        from adaptive_edge_aware_jpeg_amd._lib import JpegAdobe, JpegDecDesc, JpegProgFrame, JpegProgScan
        self._setup()
        self.family, self.n = family, len(files)
        n = self.n
        if family == "jpegdec":
            self.frames = [A.standard_jpeg.parse_header(f, adobe=True) for f in files]
            descs = (JpegDecDesc * n)(*self.frames)
            self.keep = (descs,)
            self.head = (self.ctx.handle, ctypes.addressof(descs), n)
            pieces = [f[d.scan_offset:d.scan_offset + d.scan_length] for f, d in zip(files, self.frames)]
        else:
            parsed = [A.standard_jpeg.parse_scans(f, adobe=True) for f in files]
            self.frames = [p[0] for p in parsed]
            frames = (JpegProgFrame * n)(*self.frames)
            flat = [(f, s) for f, p in zip(files, parsed) for s in p[1]]
            scans = (JpegProgScan * len(flat))(*[s for _, s in flat])
            self.keep = (frames, scans)
            self.head = (self.ctx.handle, ctypes.addressof(frames), ctypes.addressof(scans), n)
            pieces = [f[s.data_offset:s.data_offset + s.data_length] for f, s in flat]
        self.xs = (JpegAdobe * n)(*[f.adobe for f in self.frames])
        self.data = torch.frombuffer(bytearray(b"".join(pieces)), dtype=torch.uint8).cuda()
        self.data_off = [int(v) for v in np.cumsum([0] + [len(p) for p in pieces[:-1]])]
        self.out_off = [i * OUT_EACH for i in range(n)]
        self.out_pattern = (torch.arange(n * OUT_EACH, device="cuda") % 251).to(torch.uint8)
        self.status_pattern = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.out, self.status = self.out_pattern.clone(), self.status_pattern.clone()
        self.ws = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")

    def _options(self, entry, scales, comps, boxes):
        s, c, b = _arr(ctypes.c_int, scales), _arr(ctypes.c_int, comps), _arr(ctypes.c_int32, boxes)
        return (s[0], c[0], b[0]), (s[1], c[1], b[1], ctypes.addressof(self.xs))[:ENTRIES[entry]]

    def query(self, entry, scales=None, comps=None, boxes=None):
        keep, opts = self._options(entry, scales, comps, boxes)
        return int(getattr(self.lib, f"aej_{self.family}_workspace_bytes{entry}")(*self.head, *opts))

    def call(self, entry, scales=None, comps=None, boxes=None, out=True, status=True, data_off=None, out_off=None, ws_bytes=WS_BYTES):
        keep, opts = self._options(entry, scales, comps, boxes)
        so, so_at = _arr(ctypes.c_int64, self.data_off if data_off is None else data_off)
        oo, oo_at = _arr(ctypes.c_int64, self.out_off if out_off is None else out_off)
        return getattr(self.lib, f"aej_{self.family}_batch{entry}")(
            *self.head, *opts, self.data.data_ptr(), ctypes.c_uint64(self.data.numel()), so_at, self.out.data_ptr() if out else None,
            ctypes.c_uint64(self.out.numel()), oo_at, self.status.data_ptr() if status else None, self.ws.data_ptr(), ctypes.c_uint64(ws_bytes))

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.equal(self.out, self.out_pattern) and torch.equal(self.status, self.status_pattern))


# name -> (the entries it goes through, the call's keywords, whether the options alone are refused: the size query then answers 0)
PAIR_CASES = {
    "scale 3": ("_scaled _mode _box _sbox _adobe", dict(scales=[1, 3]), True),
    "2 components": ("_mode _box _sbox _adobe", dict(comps=[3, 2]), True),
    "4 components of a three-component file": ("_mode _box _sbox _adobe", dict(comps=[3, 4]), True),
    "box leaves the image": ("_box _sbox _adobe", dict(boxes=[WHOLE, (0, 0, 25, 16)]), True),
    "empty box": ("_box _sbox _adobe", dict(boxes=[WHOLE, EMPTY]), True),
    "box at scale 2": ("_box _adobe", dict(scales=[1, 2], boxes=[WHOLE, (0, 0, 8, 8)]), True),
    "sbox leaves the scaled image": ("_sbox", dict(scales=[1, 2], boxes=[WHOLE, (0, 0, 13, 8)]), True),
    "scale 3 on file 1, 2 components on file 0": ("_mode _box _sbox _adobe", dict(scales=[1, 3], comps=[2, 3]), True),
    "scale 3 and an empty box": ("_box _sbox _adobe", dict(scales=[1, 3], boxes=[EMPTY, WHOLE]), True),
    "empty box and a short workspace": ("_box _sbox _adobe", dict(boxes=[WHOLE, EMPTY], ws_bytes=1), True),
    "NULL output and scale 3": ("_scaled _mode _box _sbox _adobe", dict(scales=[1, 3], out=False), True),
    "NULL status and scale 3": ("_scaled _mode _box _sbox _adobe", dict(scales=[1, 3], status=False), True),
    "scan outside the buffer": (" _scaled _mode _box _sbox _adobe", dict(scales=[1, 1], data_off="last past the end"), False),
    "image outside the output": (" _scaled _mode _box _sbox _adobe", dict(scales=[1, 1], out_off=[0, 2 * OUT_EACH - 1]), False),
    "workspace one byte short": (" _scaled _mode _box _sbox _adobe", dict(scales=[1, 1], ws_bytes="one short"), False),
}
CMYK_CASES = {                                               # file 0: the 4:2:0 file, file 1: the CMYK file
    "luma of a CMYK file": ("_adobe", dict(comps=[3, 1]), True),
    "scale 2 of a CMYK file": ("_adobe", dict(scales=[1, 2]), True),
    "box of a CMYK file": ("_adobe", dict(boxes=[WHOLE, (0, 0, 8, 8)]), True),
}
SBOX = dict(scales=[1, 2], boxes=[WHOLE, (2, 1, 10, 7)])    # accepted through _sbox: 8 x 6 pixels of file 1's 12 x 8 image


def _entries(spec):
    return spec.split(" ") if spec.startswith(" ") else spec.split()


def _observe_decoders(A, files, cmyk):
    seen = {}
    for family in ("jpegdec", "jpegprog"):
        for d, cases in ((_Decoder(A, family, [files[family]] * 2), PAIR_CASES), (_Decoder(A, family, [files[family], cmyk[family]]), CMYK_CASES)):
            for name, (spec, case_kw, options) in cases.items():
                for entry in _entries(spec):
                    kw = dict(case_kw)
                    opts = {k: kw[k] for k in ("scales", "comps", "boxes") if k in kw}
                    if kw.get("data_off") == "last past the end":
                        kw["data_off"] = d.data_off[:-1] + [d.data.numel()]
                    if kw.get("ws_bytes") == "one short":
                        kw["ws_bytes"] = d.query(entry, **opts) - 1
                        assert 0 < kw["ws_bytes"] < WS_BYTES
                    rc = d.call(entry, **kw)
                    rec = dict(rc=rc, msg=d.last_error(), untouched=d.untouched())
                    if options:
                        d.sentinel()
                        rec.update(query=d.query(entry, **opts), after_query=d.last_error())
                    seen[f"aej_{family}_batch{entry}: {name}"] = rec
    return seen


class _Transform(_Base):
    """two baseline files (4:2:0, 4:2:2) and a progressive one staged for the aej_jfif_transform_* entries"""

    def __init__(self, A, base_files, prog_files):
        import torch
        from adaptive_edge_aware_jpeg_amd._lib import JpegDecDesc, JpegProgFrame, JpegProgScan
        self._setup()
        ds = [A.standard_jpeg.parse_header(f) for f in base_files]
        parsed = [A.standard_jpeg.parse_scans(f) for f in prog_files]
        nb, npg = len(ds), len(parsed)
        self.n = nb + npg
        descs, frames = (JpegDecDesc * nb)(*ds), (JpegProgFrame * npg)(*[p[0] for p in parsed])
        flat = [(f, s) for f, p in zip(prog_files, parsed) for s in p[1]]
        pscans = (JpegProgScan * len(flat))(*[s for _, s in flat])
        pieces = [f[d.scan_offset:d.scan_offset + d.scan_length] for f, d in zip(base_files, ds)] + [f[s.data_offset:s.data_offset + s.data_length] for f, s in flat]
        off = [int(v) for v in np.cumsum([0] + [len(p) for p in pieces[:-1]])]
        self.data = torch.frombuffer(bytearray(b"".join(pieces)), dtype=torch.uint8).cuda()
        so, do = (ctypes.c_int64 * nb)(*off[:nb]), (ctypes.c_int64 * len(flat))(*off[nb:])
        self.keep = (descs, frames, pscans, so, do)
        self.sizes = (self.ctx.handle, ctypes.addressof(descs), nb, ctypes.addressof(frames), ctypes.addressof(pscans), npg, 0)
        self.head = (self.ctx.handle, ctypes.addressof(descs), nb, self.data.data_ptr(), ctypes.c_uint64(self.data.numel()), ctypes.addressof(so),
                     ctypes.addressof(frames), ctypes.addressof(pscans), npg, self.data.data_ptr(), ctypes.c_uint64(self.data.numel()), ctypes.addressof(do),
                     None, 0)
        self.pattern = (torch.arange(8192, device="cuda") % 251).to(torch.uint8)
        self.out = self.pattern.clone()
        self.words_pattern = torch.full((3 * self.n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")      # offsets, lengths, status
        self.words = self.words_pattern.clone()
        self.ws = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")

    def _middle(self, entry, xf, trim, rb, rr, l440, boxes, drop):
        x, b = _arr(ctypes.c_int32, xf), _arr(ctypes.c_int32, boxes)
        return (x[0], b[0]), (x[1], trim, rb, rr, l440, b[1], drop)[:{"": 2, "_rst": 4, "_440": 5, "_cut": 7}[entry]]

    def query(self, entry, xf=(0, 0, 0), trim=0, rb=0, rr=0, l440=0, boxes=None, drop=0):
        keep, mid = self._middle(entry, xf, trim, rb, rr, l440, boxes, drop)
        return int(getattr(self.lib, f"aej_jfif_transform_workspace_bytes{entry}")(*self.sizes, *mid))

    def call(self, entry, xf=(0, 0, 0), trim=0, rb=0, rr=0, l440=0, boxes=None, drop=0):
        keep, mid = self._middle(entry, xf, trim, rb, rr, l440, boxes, drop)
        self.total, self.groups = ctypes.c_uint64(12345), ctypes.c_int32(12345)
        w, n = self.words.data_ptr(), self.n
        return getattr(self.lib, f"aej_jfif_transform_batch{entry}")(
            *self.head, *mid, self.out.data_ptr(), ctypes.c_uint64(self.out.numel()), w, w + 8 * n, ctypes.addressof(self.total), w + 16 * n,
            ctypes.addressof(self.groups), self.ws.data_ptr(), ctypes.c_uint64(WS_BYTES))

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return bool(torch.equal(self.out, self.pattern) and torch.equal(self.words, self.words_pattern) and self.total.value == 12345 and
                    self.groups.value == 12345)


TRANSPOSE = 3
TRANSFORM_CASES = {                                          # files: 4:2:0, 4:2:2 (both baseline), 4:2:0 progressive
    "layout_440 2": ("_440 _cut", dict(l440=2)),
    "drop_chroma 2": ("_cut", dict(drop=2)),
    "trim 2": (" _rst _440 _cut", dict(trim=2)),
    "restart interval 65536": ("_rst _440 _cut", dict(rb=65536)),
    "crop box outside the transformed image": ("_cut", dict(boxes=[(0, 0, 0, 0), (0, 0, 40, 16), (0, 0, 0, 0)])),
    "transpose of a 4:2:2 file without layout_440": (" _rst _440 _cut", dict(xf=(0, TRANSPOSE, 0))),
    "NULL transforms": (" _rst", dict(xf=None)),
}


def _observe_transforms(A, files):
    t = _Transform(A, [files["jpegdec"], files["422"]], [files["jpegprog"]])
    seen = {}
    for name, (spec, kw) in TRANSFORM_CASES.items():
        for entry in _entries(spec):
            rc = t.call(entry, **kw)
            rec = dict(rc=rc, msg=t.last_error(), untouched=t.untouched())
            t.sentinel()
            rec.update(query=t.query(entry, **kw), after_query=t.last_error())
            seen[f"aej_jfif_transform_batch{entry}: {name}"] = rec
    return seen


def _files():
    files = {"jpegdec": R.make_file("420", 24, 16), "jpegprog": R.make_file("420", 24, 16, progressive=True), "422": R.make_file("422", 24, 16)}
    cmyk = {"jpegdec": AR.make_file("cmyk", "2x2", 16, 16), "jpegprog": AR.make_file("cmyk", "2x2", 16, 16, progressive=True)}
    return files, cmyk


def observe(A):
    """every case run once -> {"<entry>: <case>": dict(rc, msg, untouched[, query, after_query])}"""
    files, cmyk = _files()
    seen = _observe_decoders(A, files, cmyk)
    seen.update(_observe_transforms(A, files))
    return seen


@pytest.fixture(scope="module")
def seen(A):
    return observe(A)


# (case, return code, aej_last_error with the entry's name as {fn}, the entries that answer so), as the library gave them before the fold
PINS = [
    ('2 components', -1, '{fn}: file 1: 2 output components (3: RGB, 1: luma)',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox'),
    ('4 components of a three-component file', -1, '{fn}: file 1: 4 output components (3: RGB, 1: luma)',
     'aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox'),
    ('4 components of a three-component file', -1, '{fn}: file 1: 4 output components for a file that does not have four',
     'aej_jpegdec_batch_adobe aej_jpegprog_batch_adobe'),
    ('NULL output and scale 3', -1, '{fn}: NULL buffer',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegdec_batch_scaled aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox aej_jpegprog_batch_scaled'),
    ('NULL status and scale 3', -1, '{fn}: NULL buffer',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegdec_batch_scaled'),
    ('NULL status and scale 3', -1, '{fn}: file 1: scale 3 (1, 2, 4 or 8)',
     'aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox aej_jpegprog_batch_scaled'),
    ('NULL transforms', -1, '{fn}: NULL buffer',
     'aej_jfif_transform_batch aej_jfif_transform_batch_rst'),
    ('box at scale 2', -5, '{fn}: file 1: a box at scale 2, 4 or 8 is not built',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegprog_batch_adobe aej_jpegprog_batch_box'),
    ('box leaves the image', -1, '{fn}: file 1: box (0, 0, 25, 16) is empty or leaves the 24 x 16 image',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_sbox aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_sbox'),
    ('box of a CMYK file', -5, '{fn}: file 1: a box of a four-component / RGB-coded file is not built',
     'aej_jpegdec_batch_adobe aej_jpegprog_batch_adobe'),
    ('crop box outside the transformed image', -1, '{fn}: file 1: crop box (0, 0, 40, 16) does not lie inside the transformed image',
     'aej_jfif_transform_batch_cut'),
    ('drop_chroma 2', -1, '{fn}: drop_chroma 2 (0 or 1)',
     'aej_jfif_transform_batch_cut'),
    ('empty box', -1, '{fn}: file 1: box (8, 8, 8, 9) is empty or leaves the 24 x 16 image',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_sbox aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_sbox'),
    ('empty box and a short workspace', -1, '{fn}: file 1: box (8, 8, 8, 9) is empty or leaves the 24 x 16 image',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_sbox aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_sbox'),
    ('image outside the output', -1, '{fn}: file 1: image outside the output',
     'aej_jpegdec_batch aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegdec_batch_scaled aej_jpegprog_batch aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox aej_jpegprog_batch_scaled'),
    ('layout_440 2', -1, '{fn}: layout_440 2 (0 or 1)',
     'aej_jfif_transform_batch_440 aej_jfif_transform_batch_cut'),
    ('luma of a CMYK file', -5, '{fn}: file 1: luma output of a four-component / RGB-coded file is not built',
     'aej_jpegdec_batch_adobe aej_jpegprog_batch_adobe'),
    ('restart interval 65536', -1, '{fn}: restart_blocks 65536, restart_rows 0 (0 .. 65535)',
     'aej_jfif_transform_batch_440 aej_jfif_transform_batch_cut aej_jfif_transform_batch_rst'),
    ('sbox leaves the scaled image', -1, '{fn}: file 1: box (0, 0, 13, 8) is empty or leaves the 12 x 8 image',
     'aej_jpegdec_batch_sbox aej_jpegprog_batch_sbox'),
    ('scale 2 of a CMYK file', -5, '{fn}: file 1: a scale other than 1 of a four-component / RGB-coded file is not built',
     'aej_jpegdec_batch_adobe aej_jpegprog_batch_adobe'),
    ('scale 3', -1, '{fn}: file 1: scale 3 (1, 2, 4 or 8)',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegdec_batch_scaled aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox aej_jpegprog_batch_scaled'),
    ('scale 3 and an empty box', -1, '{fn}: file 1: scale 3 (1, 2, 4 or 8)',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_sbox aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_sbox'),
    ('scale 3 on file 1, 2 components on file 0', -1, '{fn}: file 1: scale 3 (1, 2, 4 or 8)',
     'aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox'),
    ('scan outside the buffer', -1, '{fn}: file 1: scan outside the scans buffer',
     'aej_jpegdec_batch aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegdec_batch_scaled'),
    ('scan outside the buffer', -1, '{fn}: scan 19: bytes outside the data buffer',
     'aej_jpegprog_batch aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox aej_jpegprog_batch_scaled'),
    ('transpose of a 4:2:2 file without layout_440', -5, '{fn}: file 1: a transposing transform of a 4:2:2 file would be a 4:4:0 file, which is not built',
     'aej_jfif_transform_batch aej_jfif_transform_batch_440 aej_jfif_transform_batch_cut aej_jfif_transform_batch_rst'),
    ('trim 2', -1, '{fn}: trim 2 (0 or 1)',
     'aej_jfif_transform_batch aej_jfif_transform_batch_440 aej_jfif_transform_batch_cut aej_jfif_transform_batch_rst'),
    ('workspace one byte short', -4, 'workspace too small: need 216576 bytes, got 216575',
     'aej_jpegprog_batch aej_jpegprog_batch_adobe aej_jpegprog_batch_box aej_jpegprog_batch_mode aej_jpegprog_batch_sbox aej_jpegprog_batch_scaled'),
    ('workspace one byte short', -4, 'workspace too small: need 26880 bytes, got 26879',
     'aej_jpegdec_batch aej_jpegdec_batch_adobe aej_jpegdec_batch_box aej_jpegdec_batch_mode aej_jpegdec_batch_sbox aej_jpegdec_batch_scaled'),
]
EXPECTED = {f"{fn}: {case}": (rc, text.format(fn=fn)) for case, rc, text, fns in PINS for fn in fns.split()}


def test_every_case_is_pinned(seen):
    assert sorted(seen) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_refusal(seen, case):
    got = seen[case]
    assert (got["rc"], got["msg"]) == EXPECTED[case]
    assert got["rc"] < 0 and got["untouched"], "a refusal wrote to the output or the status words"
    if "query" in got:                                       # the options alone are refused: the size query agrees, silently
        assert got["query"] == 0 and got["after_query"] == SENTINEL


@pytest.mark.parametrize("family", ["jpegdec", "jpegprog"])
def test_sbox_entry_takes_the_box_at_scale_2(A, family):
    """the box that _box refuses at scale 2 (above), through _sbox: the Python call's pixels, and nothing beside them"""
    import torch
    files, _ = _files()
    d = _Decoder(A, family, [files[family]] * 2)
    need = d.query("_sbox", **SBOX)
    assert 0 < need <= WS_BYTES
    d.status.fill_(-0x5A5A5A5B)                              # 0xA5 bytes: the entry clears its status words itself
    assert d.call("_sbox", ws_bytes=need, **SBOX) == 0
    torch.cuda.synchronize()
    assert not d.status.any()
    want = A.standard_jpeg_decode_many([files[family]] * 2, progressive=True, scale=SBOX["scales"], scaled_box=[None, SBOX["boxes"][1]])
    assert [tuple(w.shape) for w in want] == [(16, 24, 3), (6, 8, 3)]
    for i, w in enumerate(want):
        assert torch.equal(d.out[i * OUT_EACH:i * OUT_EACH + w.numel()], w.reshape(-1)), i
    for lo, hi in ((24 * 16 * 3, OUT_EACH), (OUT_EACH + 8 * 6 * 3, 2 * OUT_EACH)):
        assert torch.equal(d.out[lo:hi], d.out_pattern[lo:hi])
