"""CPU: the oracle's decode arithmetic (``blocks_decode``, ``upsample_linear``, ``decode_image``) against the float64 restatement of
tests/decode_reference.py and its elementwise float32 bound, on basis functions, highest-frequency energy, checkerboards, dense and
saturating blocks, and the layer geometries the codec accepts.  Each check also shows that the plausible wrong kernels (mutants)
fall outside the bound on the same inputs."""
import numpy as np
import pytest

import decode_reference as R

SIZES = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024]


def random_tables(sizes, seed):
    rng = np.random.default_rng(seed)
    return {s: rng.integers(1, 65, (s, s)).astype(np.int32) for s in sizes}


@pytest.mark.parametrize("s", SIZES)
def test_oracle_idct_basis_functions_and_patterns(oracle, s):
    """every basis function (k, j) for s <= 32, a random sample of them above, then a lone DC, the highest frequency, a checkerboard,
    dense and largest-magnitude blocks, laid out as a row of leaves of one size; dequantised with a random integer table"""
    if s <= 32:
        n_basis = s * s
    else:
        n_basis = {64: 24, 128: 12, 256: 6, 512: 3, 1024: 1}[s]
    qm = random_tables([s], s)
    rng = np.random.default_rng(100 + s)
    kinds = ["dc", "highest", "checker", "dense", "max"] if s < 512 else ["checker", "max"] if s == 512 else ["dense"]
    basis = [(k, j) for k in range(s) for j in range(s)] if s <= 32 else [tuple(v) for v in rng.integers(0, s, (n_basis, 2))]
    blocks = []
    for i, kj in enumerate(basis):
        Y = R.leaf_pattern("basis", s, rng, kj) * (100.0 if i % 3 else 400.0) * s / 2
        blocks.append(np.where(Y != 0, np.sign(Y) * np.maximum(np.abs(np.rint(Y / qm[s])), 1), 0))
    n = len(blocks) + len(kinds)
    leaves = np.array([[i * s, 0, s] for i in range(n)], np.int32)
    tail = R.make_coeffs(leaves[len(blocks):], qm, s, kinds=kinds)
    zz = R.zigzag(s)
    co = np.concatenate([np.concatenate([b.reshape(-1)[zz] for b in blocks]).astype(np.int32) if blocks else np.zeros(0, np.int32), tail])
    got = oracle.blocks_decode(co, leaves, qm, {s: oracle.zigzag(s)}, "YCoCg", 0, s, n * s)
    ref, bound = R.blocks_decode(co, leaves, qm, "YCoCg", 0, s, n * s)
    R.assert_within(got, ref, bound, f"s={s}")
    R.assert_mutants_caught(lambda v: R.blocks_decode(co, leaves, qm, "YCoCg", 0, s, n * s, idct_variant=v)[0], R.IDCT_MUTANTS, ref, bound,
                            f"s={s}")


@pytest.mark.parametrize("h,w,H,W", [(16, 24, 33, 49), (3, 5, 7, 21), (5, 1, 11, 5), (1, 4, 2, 17), (40, 13, 81, 52), (8, 8, 16, 16)],
                         ids=lambda v: str(v))
def test_oracle_upsample_linear(oracle, h, w, H, W):
    """cv.resize INTER_LINEAR: ragged (non-integer) scales, a source 1 sample wide or high, exact 2x"""
    rng = np.random.default_rng(h * 1000 + w)
    src = (rng.standard_normal((h, w)) * 0.3).astype(np.float32)
    got = oracle.upsample_linear(src, H, W)
    ref, bound = R.upsample(src.astype(np.float64), np.zeros((h, w)), H, W)
    R.assert_within(got, ref, bound, "upsample")
    variants = [m for m in R.UPSAMPLE_MUTANTS if not (w == 1 and H == 2 * h and m == "nearest")]
    R.assert_mutants_caught(lambda v: R.upsample(src.astype(np.float64), np.zeros((h, w)), H, W, v)[0], variants, ref, bound, "upsample")


def _oracle_case(oracle, space, H, W, qr, br, seed, zero_layers=(), amp=(100.0, 40.0, 40.0)):
    img = oracle.synth_image(H, W, seed).astype(np.float32) / np.float32(255)
    enc = oracle.encode_image(img, space, qr, br)
    _, _, qm = oracle.tables(space, qr, br)
    layers = []
    for l, L in enumerate(enc):
        L["coeffs"] = R.make_coeffs(L["leaves"], qm[l], seed + l, amp=amp[l])
        if l in zero_layers:
            L["coeffs"][:] = 0
        layers.append(dict(coeffs=L["coeffs"], leaves=L["leaves"], qm=qm[l]))
    return enc, layers, qm


CASES = [("YCbCr", 61, 97, (40, 80), (2, 16)), ("YCoCg", 130, 70, (30, 90), (4, 128)), ("YCoCg-R", 45, 200, (1, 1), (8, 32)),
         ("YCoCg", 9, 2, (40, 80), (2, 4))]


@pytest.mark.parametrize("space,H,W,qr,br", CASES, ids=lambda v: str(v))
def test_oracle_decode_image(oracle, space, H, W, qr, br):
    enc, layers, _ = _oracle_case(oracle, space, H, W, qr, br, 7)
    got = oracle.decode_image(oracle.write_ajpg(enc, H, W, space, qr, br, ".png"))
    ref, bound = R.decode(layers, space, H, W)
    R.assert_within(got, ref, bound, space)
    assert ((ref > 0.01) & (ref < 0.99)).mean() > 0.3 and ((ref == 0) | (ref == 1)).any()      # in range mostly, and the clip is hit
    R.assert_mutants_caught(lambda v: R.decode(layers, space, H, W, idct_variant=v)[0], R.IDCT_MUTANTS, ref, bound, space)
    if min(H, W) >= 4:
        R.assert_mutants_caught(lambda v: R.decode(layers, space, H, W, upsample_mode=v)[0], R.UPSAMPLE_MUTANTS, ref, bound, space)


@pytest.mark.parametrize("space,H,W", [("ICtCp", 37, 5), ("ICaCb", 50, 129)])
def test_oracle_decode_planes_ratio_1x4(oracle, space, H, W):
    """the (1, 4) layer-ratio set: its colour spaces are not linear, so the decoded planes are compared, before and after the
    upsample; W = 5 leaves a chroma layer 1 sample wide"""
    enc, layers, qm = _oracle_case(oracle, space, H, W, (40, 80), (2, 16), 3, amp=(100.0, 100.0, 100.0))
    for l, ((h, w), L) in enumerate(zip(R.layer_shapes(H, W, space), layers)):
        zz = {s: oracle.zigzag(s) for s in qm[l]}
        plane = oracle.blocks_decode(L["coeffs"], L["leaves"], qm[l], zz, space, l, h, w)
        ref, bound = R.blocks_decode(L["coeffs"], L["leaves"], qm[l], space, l, h, w)
        R.assert_within(plane, ref, bound, f"{space} layer {l} plane")
        up = oracle.upsample_linear(plane, H, W)
        ref_u, bound_u = R.upsample(ref, bound, H, W)
        R.assert_within(up, ref_u, bound_u, f"{space} layer {l} upsampled")
        if l and w >= 2:
            R.assert_mutants_caught(lambda v: R.upsample(ref, bound, H, W, v)[0], R.UPSAMPLE_MUTANTS, ref_u, bound_u, f"{space} layer {l}")


def test_oracle_stage_isolation_identities(oracle):
    """Identities the GPU tests lean on, confirmed on the oracle first.  YCoCg's inverse (R = Y + Co - Cg, G = Y + Cg,
    B = Y - Co - Cg) has unit luma weights: with both chroma planes zero, R = G = B = clip(luma plane) exactly, which isolates
    dequantise, IDCT and denormalise with no upsample in the way; with zero luma (0.5 after denormalising) and Cg zero,
    R = clip(0.5 + Co), G = 0.5, B = clip(0.5 - Co) isolate the upsampled Co plane."""
    H, W = 77, 91
    enc, layers, qm = _oracle_case(oracle, "YCoCg", H, W, (40, 80), (2, 16), 21, zero_layers=(1, 2))
    rgb = oracle.decode_image(oracle.write_ajpg(enc, H, W, "YCoCg", (40, 80), (2, 16), ".png"))
    zz = {s: oracle.zigzag(s) for s in qm[0]}
    luma = oracle.blocks_decode(enc[0]["coeffs"], enc[0]["leaves"], qm[0], zz, "YCoCg", 0, H, W)
    assert np.array_equal(rgb[..., 0], np.clip(luma, 0, 1)) and np.array_equal(rgb[..., 1], rgb[..., 0]) and np.array_equal(rgb[..., 2], rgb[..., 0])
    enc, layers, qm = _oracle_case(oracle, "YCoCg", H, W, (40, 80), (2, 16), 22, zero_layers=(0, 2), amp=(0.0, 60.0, 0.0))
    rgb = oracle.decode_image(oracle.write_ajpg(enc, H, W, "YCoCg", (40, 80), (2, 16), ".png"))
    co = oracle.upsample_linear(oracle.blocks_decode(enc[1]["coeffs"], enc[1]["leaves"], qm[1], zz, "YCoCg", 1, H // 2, W // 2), H, W)
    luma0 = np.float32(0.5)                             # denormalised zero luma
    assert np.array_equal(rgb[..., 0], np.clip(luma0 + co, 0, 1)) and np.array_equal(rgb[..., 1], np.full_like(co, luma0))
    assert np.array_equal(rgb[..., 2], np.clip(luma0 - co, 0, 1))
