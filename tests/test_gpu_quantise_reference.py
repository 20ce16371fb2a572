"""GPU (-m gpu): every kernel copy of the quantiser (csrc/dct.hip epilogues, csrc/requant.hip) against tests/quantise_reference.py on
the cases that reach its ties, near-ties, range guards, float64 fallbacks, zero-skip thresholds and, for 64 x 64 leaves, the values past
zigzag position 1 024 -- with quantiser tables up to 2^31 - 1, a different one per layer and block size.  Y comes from the oracle's DCT
(bit-identical to the kernels) or from the kernels' own dct_f32 output; the coefficients must equal
reference(Y, Q) exactly.  Every test prints what its cases reached (quantise_reference.classify)."""
import ctypes

import numpy as np
import pytest

import quantise_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import adaptive_edge_aware_jpeg_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def ctx(A):
    from adaptive_edge_aware_jpeg_amd._lib import get_context
    return get_context()


@pytest.fixture
def options(ctx):
    """aej_set_option for one test, restored to the previous values afterwards"""
    saved = {}

    def set_(name, value):
        saved.setdefault(name, ctx.get_option(name))
        ctx.set_option(name, value)
    yield set_
    for k, v in saved.items():
        ctx.set_option(k, v)


def report(label, Y, Q, zpos=None):
    c = R.classify(Y, Q, zpos)
    print(f"\n{label}: " + ", ".join(f"{k} {v}" for k, v in c.items()))
    return c


# ------------------------------------------------------------------ a. stage entry, every block size
def stage_cases(s):
    """(label, plane, table kind of layer 0) for block size s; layer 2 runs the same plane under another table"""
    n = lambda per: max(1, min(64, per // (s * s))) if s >= 256 else max(1, per // (s * s))      # noqa: E731
    cases = [("large", R.large_plane(s, n(1 << 16), s, spill=0.1), "ones"),
             ("large", R.large_plane(s, n(1 << 16), s + 1, spill=0.1), "odd"),
             ("huge", R.large_plane(s, n(1 << 15), s + 2, lo=2.0 ** 17, hi=2.0 ** 21), "odd"),
             ("vast", R.large_plane(s, n(1 << 14), s + 3, lo=2.0 ** 24, hi=2.0 ** 27), "big"),
             ("band", R.large_plane(s, n(1 << 15), s + 4), "band"),
             ("vast", R.large_plane(s, n(1 << 14), s + 5, lo=2.0 ** 25, hi=2.0 ** 27), "held")]
    if s in (32, 64, 128):
        cases.append(("vote", R.vote_plane(s, 4, s + 9), "vote"))
    if s in R.POW2_ALPHA_SIZES:
        vals = R.tie_constants(s)
        cases.append(("const", R.constant_plane(s, vals if s <= 256 else vals[2:4]), "dc=16777217"))
        cases.append(("const", R.constant_plane(s, vals if s <= 256 else vals[2:4]), "dc=16777216"))
    if s == 64:
        cases.append(("basis", R.basis_plane(64, 16, 7, 2.0 ** 28), "odd"))
    if s >= 512:
        cases = [c for c in cases if c[2] in ("ones", "held", "big") or c[0] == "const"]
    return cases


OTHER = {"vote": "pow2", "held": "odd", "ones": "pow2", "odd": "big", "big": "odd", "band": "outlier", "dc=16777217": "outlier", "dc=16777216": "pow2"}


def run_stage(ctx, plane, s, layer, want_dct):
    import torch
    H, W = plane.shape
    n = W // s
    leaves = R.leaves_row(s, n)
    offs = (np.arange(n, dtype=np.int64) * s * s).astype(np.int32)
    lv4 = np.concatenate([leaves, offs[:, None]], 1).astype(np.int32)
    d_l, d_n = ctx.to_device(lv4, torch.int32), ctx.to_device(plane, torch.float32)
    d_c = ctx.empty((n * s * s,), torch.int32)
    d_d = ctx.empty((n * s * s,), torch.float32) if want_dct else None
    ctx.check(ctx.lib.aej_dct_quant_zigzag(ctx.handle, d_n.data_ptr(), H, W, layer, d_l.data_ptr(), ctypes.c_int64(n), d_c.data_ptr(),
                                           d_d.data_ptr() if want_dct else None))
    return d_c.cpu().numpy(), (d_d.cpu().numpy() if want_dct else None)


@pytest.mark.parametrize("s", R.ALL_SIZES)
def test_stage_entry_quantiser(A, ctx, oracle, options, s):
    if s <= 16:
        options("dct_small_workgroups", 1)        # one workgroup walks every leaf: the tables it keeps must stay right
    dct64 = (1, 4) if s == 64 else (0,)
    failures = []
    for label, plane, kind in stage_cases(s):
        if kind == "held":          # a table searched for this plane: quantisers above 2^24 that a float32 does not hold, at its large values
            t0 = R.searched_table(oracle, plane, s, kind)
            assert (t0 > (1 << 24)).sum() > 0
        elif kind == "vote":        # searched: one lane of every vote unit of the large-leaf kernels in the zero-skip window
            t0 = R.searched_table(oracle, plane, s, kind)
            assert t0.max() <= (1 << 22)
        else:
            t0 = R.table(kind, s, 10 * s + 1)
        tabs = {0: t0, 1: R.table("ones", s, 2), 2: R.table(OTHER[kind], s, 10 * s + 3)}
        ctx.set_settings("YCbCr", s, s, np.concatenate([tabs[l] for l in range(3)]))
        for layer in (0, 2):
            Yo, Yz, co, Qz, zpos, _, _ = R.oracle_case(oracle, plane, s, tabs[layer])
            assert np.array_equal(co, R.reference(Yz, Qz))
            report(f"s={s} {label} layer {layer} table {kind if layer == 0 else OTHER[kind]}", Yz, Qz, zpos if s == 64 else None)
            if kind == "held" and layer == 0:
                assert (R.m_float_held_q(Yz, Qz) != co).any()      # the case separates the float-held quantiser
            if kind == "vote" and layer == 0:
                Yr, nl = Yo.reshape(-1, s * s), plane.shape[1] // s
                for unit in ("mfma", "wave64") if s == 64 else ("mfma",):
                    hit = R.vote_units_in_window(Yr, t0, s, unit)
                    print(f"s={s} vote units ({unit}) that a 0.501 threshold would skip wrongly: {hit}")
                    assert hit >= nl * ((s // 8) * (s // 32) - 1) * 3 // 4
            for k64 in dct64:
                if s == 64:
                    options("dct64_kernel", k64)
                for want_dct in (True, False):
                    got_c, got_d = run_stage(ctx, plane, s, layer, want_dct)
                    if want_dct:
                        assert np.array_equal(got_d, Yo), f"s={s} {label} layer {layer}: DCT floats differ from the oracle"
                    bad = np.flatnonzero(got_c != co)
                    if bad.size:
                        failures.append(f"s={s} {label} layer {layer} table {kind if layer == 0 else OTHER[kind]} dct64_kernel={k64} "
                                        f"dct_f32={want_dct}: {bad.size} coefficients differ, first zigzag {zpos[bad[0]]} Y={Yz[bad[0]]!r} "
                                        f"Q={Qz[bad[0]]} got {got_c[bad[0]]} want {co[bad[0]]}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ b. whole path: compress_batch with adversarial tables
def make_codec(A, space, br, kinds, seed):
    class Adversarial(A.Jpeg):
        def _qmats_blob(self):
            return np.concatenate([R.table(kinds[l], s, seed + 31 * l + s) for l in range(3) for s in self._block_sizes]).astype(np.int32)
    return Adversarial(A.JpegCompressionSettings(space, (40, 80), br))


def check_whole_path(codec, imgs, label):
    enc_d = codec.compress_batch(imgs, want_dct=True)
    enc = codec.compress_batch(imgs)
    blob = codec._qmats_blob()
    sizes = codec._block_sizes
    base, k = {}, 0
    for l in range(3):
        for s in sizes:
            base[l, s] = k
            k += s * s
    Ys, Qs, zs = [], [], []
    big = 0
    for b in range(imgs.shape[0]):
        for l in range(3):
            ld, ln = enc_d.layer(b, l, want_dct=True), enc.layer(b, l)
            assert np.array_equal(ld["leaves"], ln["leaves"]) and np.array_equal(ld["states"], ln["states"])
            assert np.array_equal(ld["coeffs"], ln["coeffs"]), f"{label} b={b} L{l}: want_dct=False coefficients differ from want_dct=True"
            Y, co = ld["dct"], ld["coeffs"]
            for s in sizes:
                sel = np.flatnonzero(ld["leaves"][:, 2] == s)
                if sel.size == 0:
                    continue
                zz = R.zigzag(s)
                idx = (ld["leaf_coeff_offsets"][sel].astype(np.int64)[:, None] + np.arange(s * s)[None, :]).ravel()
                raster = (ld["leaf_coeff_offsets"][sel].astype(np.int64)[:, None] + zz[None, :]).ravel()
                q = np.tile(blob[base[l, s]:base[l, s] + s * s].astype(np.int64)[zz], sel.size)
                want = R.reference(Y[raster], q)
                bad = np.flatnonzero(co[idx] != want)
                assert bad.size == 0, (f"{label} b={b} L{l} s={s}: {bad.size} coefficients differ, first Y={Y[raster][bad[0]]!r} "
                                       f"Q={q[bad[0]]} got {co[idx][bad[0]]} want {want[bad[0]]}")
                Ys.append(Y[raster]), Qs.append(q), zs.append(np.tile(np.arange(s * s), sel.size) if s == 64 else np.zeros(q.size, int))
                if (np.abs(Y[raster]) >= R.TWO17).any():
                    big = max(big, s)
    c = report(label, np.concatenate(Ys), np.concatenate(Qs), np.concatenate(zs))
    c["largest_leaf_at_or_above_2^17"] = big
    print(f"{label}: leaf sizes {sorted({int(v) for b in range(imgs.shape[0]) for l in range(3) for v in enc_d.layer(b, l)['leaves'][:, 2]})}, "
          f"largest with |Y| >= 2^17: {big}")
    return c


def smooth_image(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([0.5 + 0.4 * np.sin(x / (W / (2 + c)) + y / (H / (1 + c)) + rng.uniform(0, 6)) for c in range(3)], -1)
    return (img + rng.uniform(-0.02, 0.02, img.shape)).clip(0, 1).astype(np.float32)


WHOLE = [
    # label, space, br, (B, H, W), input, layer table kinds, options.  Input: "in range" (smooth and noise images in [0, 1]); "x k" (the
    # same scaled by k: every pixel becomes an edge, so only leaves below 32 and the small kernels see |Y| >= 2^17); "+ 256" (smooth images
    # offset by 256 in every channel: in the matrix spaces the luma moves by 256 and the chroma not at all, and 255 x 256 wraps to 0 in the
    # 8-bit edge planes, so the quadtree keeps large leaves, whose |Y| is far above 2^17)
    ("in-range 2x2 multi", "YCbCr", (4, 64), (2, 720, 1280), "in range", ("ones", "pow2", "ones"), {"dct_multi": 1}),
    ("in-range 2x2 per-size", "YCbCr", (4, 64), (2, 720, 1280), "in range", ("pow2", "ones", "pow2"), {"dct_multi": 0}),
    ("in-range 1x4 row-major", "ICtCp", (2, 64), (1, 600, 808), "in range", ("ones", "pow2", "odd"), {"planes_row_major": 1}),
    ("in-range 1x4 per-size", "ICaCb", (4, 64), (1, 512, 768), "in range", ("pow2", "ones", "ones"), {"dct_multi": 0}),
    ("scaled 2x2 multi", "YCbCr", (4, 64), (2, 512, 768), "x 3000", ("odd", "big", "outlier"), {"dct_multi": 1}),
    ("scaled above 8 Mpx", "YCbCr", (4, 64), (2, 1536, 3072), "x 400", ("odd", "pow2", "big"), {"planes_row_major": 1}),
    ("offset 2x2 multi", "YCbCr", (4, 64), (2, 512, 768), "+ 256", ("odd", "big", "outlier"), {"dct_multi": 1}),
    ("offset 2x2 per-size", "YCoCg", (4, 64), (2, 512, 768), "+ 256", ("big", "odd", "pow2"), {"dct_multi": 0}),
    ("offset bmax 1024", "YCoCg", (8, 1024), (1, 2048, 2048), "+ 256", ("odd", "outlier", "big"), {}),
]


@pytest.mark.parametrize("label,space,br,shape,inp,kinds,opts", WHOLE, ids=[w[0] for w in WHOLE])
def test_whole_path_quantiser(A, ctx, options, label, space, br, shape, inp, kinds, opts):
    for k, v in opts.items():
        options(k, v)
    B, H, W = shape
    if inp.startswith("+"):
        imgs = np.stack([smooth_image(H, W, 7 * b + H) for b in range(B)]) + np.float32(inp[2:])
    else:
        imgs = np.stack([smooth_image(H, W, 7 * b + H) if b % 2 == 0 else
                         np.random.default_rng(b).random((H, W, 3), dtype=np.float32) for b in range(B)])
        if inp.startswith("x"):
            imgs = imgs * np.float32(inp[2:])
    c = check_whole_path(make_codec(A, space, br, kinds, B * H + W), imgs.astype(np.float32), label)
    if inp != "in range":
        assert c["at_or_above_2^17"] > 0 and c["q_above_2^24"] > 0
    elif "ones" in kinds[:2] and space != "ICaCb":
        assert c["ties"] > 0
    if inp.startswith("+"):                        # the large kernels see values past 2^17
        assert c["largest_leaf_at_or_above_2^17"] >= min(br[1], 128)


# ------------------------------------------------------------------ c. requantisation of crafted Y
def crafted_y(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(-(1 << 15), 1 << 15, n).astype(np.float64)
    q = rng.choice([1, 2, 3, 5, 7, 255], n).astype(np.float64)
    ties = ((k + 0.5) * q).astype(np.float32)
    big = np.float32(131072.0) * rng.choice([-1, 1], n).astype(np.float32)
    f24 = np.float32(1.5 * ((1 << 24) + 1)) * rng.choice([-1, 1], n).astype(np.float32)
    pick = rng.integers(0, 8, n)
    y = np.select([pick < 3, pick == 3, pick == 4, pick == 5, pick == 6],
                  [ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf)), big, f24],
                  default=np.nextafter(f24, np.float32(0)))
    step = rng.integers(-3, 4, n).astype(np.float32)             # around 2^17 and 1.5 (2^24 + 1): a few ulp either side
    y = np.where((pick >= 5), y + step * np.spacing(np.abs(y)), y)
    return y.astype(np.float32)


def test_requantise_crafted(A, ctx, oracle):
    import torch
    space, br = "YCbCr", (4, 64)
    sizes = [4, 8, 16, 32, 64]
    img = smooth_image(384, 512, 3)[None]
    codec = A.Jpeg(A.JpegCompressionSettings(space, (40, 80), br))
    enc = codec.compress_batch(img, want_dct=True)
    ctx = codec._bind()
    Y = crafted_y(enc.dct.numel(), 11)
    enc.dct.copy_(torch.from_numpy(Y))
    lw = sum(s * s for s in sizes)
    sets = [np.concatenate([R.table(kind, s, 5 * j + s + l) for l in range(3) for s in sizes])
            for j, kind in enumerate(("ones", "pow2", "odd", "big", "dc=16777217", "outlier"))]
    sets[3][:4] = [(1 << 24) + 1, (1 << 31) - 1, (1 << 24) + 1, (1 << 31) - 1]
    n = enc.plan.batch * enc.plan.coeff_stride
    out = torch.full((len(sets) * n,), -0x5A5A5A5B, dtype=torch.int32, device=ctx.device)
    blob = ctx.to_device(np.concatenate(sets).astype(np.int32), torch.int32)
    ctx.check(ctx.lib.aej_requantise_batch(ctx.handle, enc.dct.data_ptr(), enc.leaves.data_ptr(), enc.counts.data_ptr(), 1, 384, 512,
                                           len(sets), blob.data_ptr(), out.data_ptr(), ctypes.c_uint64(n)))
    out = out.view(len(sets), -1).cpu().numpy()
    p = enc.plan
    for j, qs in enumerate(sets):
        Ys, Qs = [], []
        for l in range(3):
            lay = enc.layer(0, l)
            o0 = p.coeff_off[l]
            for s in sizes:
                sel = np.flatnonzero(lay["leaves"][:, 2] == s)
                if sel.size == 0:
                    continue
                zz = R.zigzag(s)
                offs = lay["leaf_coeff_offsets"][sel].astype(np.int64)[:, None]
                raster, idx = (o0 + offs + zz[None, :]).ravel(), (o0 + offs + np.arange(s * s)[None, :]).ravel()
                k = sizes.index(s)
                q0 = l * lw + sum(t * t for t in sizes[:k])
                q = np.tile(qs[q0:q0 + s * s].astype(np.int64)[zz], sel.size)
                want = R.reference(Y[raster], q)
                bad = np.flatnonzero(out[j, idx] != want)
                assert bad.size == 0, (f"set {j} L{l} s={s}: {bad.size} differ, first Y={Y[raster][bad[0]]!r} Q={q[bad[0]]} "
                                       f"got {out[j, idx][bad[0]]} want {want[bad[0]]}")
                Ys.append(Y[raster]), Qs.append(q)
        report(f"requantise set {j}", np.concatenate(Ys), np.concatenate(Qs))
