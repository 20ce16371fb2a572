"""Independent restatement of the codec's quantiser, np.round(block / q).astype(np.int32) (jpeg.py:499-502), with the subtly wrong
variants a kernel copy of it could be, a classifier of the inputs that separate them, and the planes and tables the quantiser tests
draw their cases from (tests/test_oracle_quantise_reference.py on the CPU, tests/test_gpu_quantise_reference.py on the GPU).

Contract: q = rint(float64(Y) / float64(Q)), round half to even, for every Q >= 1 an int32 holds.  The float32
sequence of the kernels (csrc/aej_quant.h) is valid for Q <= 2^22 and |Y / Q| < 2^18; they guard it with |Y| < 2^17 and fall back
to the float64 division.  A case is meant to reach one of those places:
  * exact ties |Y| = (k + 1/2) Q and near-ties, where rint(Y * rcp(Q)) is one off and the remainder correction must fire;
  * |Y| on both sides of 2^17 inside one leaf, row and wave (the range guards);
  * Q above 2^22 and 2^24 (the float64 fallbacks, and a quantiser a float cannot hold);
  * |Y| in [0.499 Q, 0.501 Q] (the zero-skip thresholds);
  * for 64 x 64 leaves, non-zero values past zigzag position 1 024 (k_dct64_wave's second pass)."""
import numpy as np

TWO17 = float(1 << 17)
TWO31 = float(1 << 31)
POW2_ALPHA_SIZES = (4, 16, 64, 256, 1024)       # alpha_0 = 1 / sqrt(s) is a power of two: a constant leaf c has DC exactly c * s
IRRATIONAL_ALPHA_SIZES = (2, 8, 32, 128, 512)
ALL_SIZES = (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
BIG_Q = (1 << 22, (1 << 22) + 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 1)
ODD_Q = (3, 5, 7, 255, 4095)


# ------------------------------------------------------------------ the reference
def reference(Y, Q):
    """rint(float64(Y) / float64(Q)) as int32; refuses what the contract leaves undefined (non-finite Y, |Y / Q| >= 2^31, Q < 1)."""
    y = np.asarray(Y, np.float32).astype(np.float64)
    q = np.asarray(Q).astype(np.float64)
    if not np.isfinite(y).all():
        raise ValueError("reference: non-finite Y is out of scope")
    if (q < 1).any():
        raise ValueError("reference: quantisers must be >= 1")
    v = y / q
    if not (np.abs(v) < TWO31).all():
        raise ValueError("reference: |Y / Q| >= 2^31 is out of scope")
    return np.rint(v).astype(np.int32)


# ------------------------------------------------------------------ mutants: each a quantiser that is subtly wrong
def _f64(Y, Q):
    return np.asarray(Y, np.float32).astype(np.float64), np.asarray(Q).astype(np.float64)


def _rcp(Q):
    return (np.float32(1) / np.asarray(Q).astype(np.float32)).astype(np.float32)


def m_half_away(Y, Q):
    y, q = _f64(Y, Q)
    v = y / q
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int32)


def m_floor_half(Y, Q):
    y, q = _f64(Y, Q)
    return np.floor(y / q + 0.5).astype(np.int32)


def m_f32_product(Y, Q):
    """rint(float32(y) * float32(1 / q)) with no correction"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.asarray(Y, np.float32) * _rcp(Q)
    return np.rint(t.astype(np.float64)).astype(np.int64).astype(np.int32)


def m_f32_division(Y, Q):
    t = np.asarray(Y, np.float32) / np.asarray(Q).astype(np.float32)
    return np.rint(t.astype(np.float64)).astype(np.int64).astype(np.int32)


def m_no_tie_to_even(Y, Q):
    """the float32 product, corrected only when |r| > q / 2: a tie keeps whatever the product rounded to"""
    y, q = _f64(Y, Q)
    with np.errstate(over="ignore", invalid="ignore"):
        k = np.rint((np.asarray(Y, np.float32) * _rcp(Q)).astype(np.float64))
    r = y - k * q
    k = np.where(np.abs(r) > q / 2, k + np.sign(r), k)
    return k.astype(np.int64).astype(np.int32)


def m_float_held_q(Y, Q):
    """the float64 division with the quantiser held as a float32 (2^24 + 1 -> 2^24)"""
    y = np.asarray(Y, np.float32).astype(np.float64)
    q = np.asarray(Q).astype(np.float32).astype(np.float64)
    return np.rint(y / q).astype(np.int32)


def m_skip_0501(Y, Q):
    """zero-skip at |y| < 0.501 q instead of 0.499 q, value by value (the kernels vote per unit of lanes: m_skip_vote)"""
    y, q = _f64(Y, Q)
    qf = np.asarray(Q).astype(np.float32)
    skip = np.abs(np.asarray(Y, np.float32)) < np.float32(0.501) * qf
    return np.where(skip, 0, reference(Y, Q)).astype(np.int32)


# the zero-skip of the large-leaf kernels is a wave vote, "every lane's value quantises to 0", taken per unit of raster positions:
#   mfma    k_dct_mfma<32 / 64 / 128>: one output register = rows {R, R + 4} (R % 8 < 4) x 32 columns;
#   wave64  k_dct64_wave: one group = 8 rows x 32 columns (lane = column, 4 rows per half-wave, 0.499 x the least of their 4 quantisers);
#           the group holding the DC (rows 0-7, columns 0-31) takes no vote.
def vote_units(s, unit):
    """unit index of every raster position of an s x s leaf (s >= 32)"""
    r, c = np.divmod(np.arange(s * s), s)
    if unit == "mfma":
        return ((r // 8) * 4 + r % 4) * (s // 32) + c // 32
    if unit == "wave64":
        return (r // 8) * (s // 32) + c // 32
    raise ValueError(unit)


def m_skip_vote(Yr, Qr, s, unit, thr=0.501):
    """the kernels' vote with its threshold at `thr` instead of 0.499: Yr [n][s * s] raster values of n leaves, Qr [s * s] raster
    quantisers -> [n][s * s] raster coefficients"""
    Yr = np.asarray(Yr, np.float32).reshape(-1, s * s)
    ref = reference(Yr, np.broadcast_to(np.asarray(Qr), Yr.shape)).reshape(Yr.shape)
    u = vote_units(s, unit)
    low = np.abs(Yr) < np.float32(thr) * np.asarray(Qr).astype(np.float32)[None, :]
    nu = int(u.max()) + 1
    allow = np.stack([np.bincount(u, weights=~low[i], minlength=nu) == 0 for i in range(Yr.shape[0])])      # [n][unit]: every value below
    if unit == "wave64":
        allow[:, 0] = False
    return np.where(allow[:, u], 0, ref).astype(np.int32)


def vote_units_in_window(Yr, Qr, s, unit):
    """(leaf, unit) pairs where a vote at 0.501 q gives another result than the contract: the units that catch a wrong skip threshold"""
    Yr = np.asarray(Yr, np.float32).reshape(-1, s * s)
    ref = reference(Yr, np.broadcast_to(np.asarray(Qr), Yr.shape)).reshape(Yr.shape)
    bad = m_skip_vote(Yr, Qr, s, unit) != ref
    u = vote_units(s, unit)
    return int(sum((np.bincount(u, weights=bad[i], minlength=int(u.max()) + 1) > 0).sum() for i in range(Yr.shape[0])))


MUTANTS = {"half_away_from_zero": m_half_away, "floor_x_plus_half": m_floor_half, "f32_product_uncorrected": m_f32_product,
           "f32_division": m_f32_division, "no_tie_to_even": m_no_tie_to_even, "float_held_quantiser": m_float_held_q,
           "skip_at_0501": m_skip_0501}


# ------------------------------------------------------------------ classifier
def wrong_way_near_ties(Y, Q):
    """mask: the uncorrected float32 product rint(y * rcp) is wrong for some reciprocal within +-4 ulp of float32(1 / q) (the
    perturbation of tests/native/quantise_check.c: v_rcp_f32 is not correctly rounded)"""
    y = np.asarray(Y, np.float32)
    want = reference(Y, Q).astype(np.int64)
    rcp = _rcp(Q)
    bad = np.zeros(y.shape, bool)
    lo, hi = rcp.copy(), rcp.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(5):
            for r in (lo, hi):
                bad |= np.rint((y * r).astype(np.float64)) != want
            lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
    return bad


def classify(Y, Q, zpos=None, leaf_of=None, row_of=None):
    """counts of the edges a (Y, Q) case reaches.  Y, Q: flat arrays of the same length; zpos: zigzag position of each value
    (for the past-1024 count of 64 x 64 leaves); leaf_of / row_of: index of each value's leaf / leaf row, for the guard units.
    Values are taken in 64-lane groups of consecutive elements for the per-wave mix."""
    y = np.asarray(Y, np.float32).ravel()
    q = np.asarray(Q).astype(np.int64).ravel()
    yd, qd = y.astype(np.float64), q.astype(np.float64)
    ay = np.abs(yd)
    frac = ay / qd - np.floor(ay / qd)
    ref = reference(y, q)
    big = ay >= TWO17
    c = {
        "values": int(y.size),
        "ties": int((frac == 0.5).sum()),
        "wrong_way_near_ties": int(wrong_way_near_ties(y, q).sum()),
        "below_2^17": int((~big).sum()),
        "at_or_above_2^17": int(big.sum()),
        "q_above_2^22": int((q > (1 << 22)).sum()),
        "q_above_2^24": int((q > (1 << 24)).sum()),
        "skip_band_0499_0501": int(((ay >= 0.499 * qd) & (ay <= 0.501 * qd)).sum()),
        "nonzero": int((ref != 0).sum()),
    }
    if zpos is not None:
        c["nonzero_past_zigzag_1024"] = int(((np.asarray(zpos).ravel() >= 1024) & (ref != 0)).sum())

    def mixed(unit):
        u = np.asarray(unit).ravel()
        n = int(u.max()) + 1 if u.size else 0
        nb = np.bincount(u, weights=big, minlength=n)
        nt = np.bincount(u, minlength=n)
        return int(((nb > 0) & (nb < nt)).sum())
    c["waves_mixing_2^17"] = mixed(np.arange(y.size) // 64)
    if leaf_of is not None:
        c["leaves_mixing_2^17"] = mixed(leaf_of)
    if row_of is not None:
        c["rows_mixing_2^17"] = mixed(row_of)
    return c


# ------------------------------------------------------------------ tables
def zigzag(s):
    """raster index at each zigzag position (jpeg.py:726-766 as an anti-diagonal walk)"""
    out = np.empty(s * s, np.int64)
    i = 0
    for d in range(2 * s - 1):
        lo, hi = max(0, d - s + 1), min(d, s - 1)
        rows = range(lo, hi + 1) if d % 2 else range(hi, lo - 1, -1)
        for r in rows:
            out[i] = r * s + (d - r)
            i += 1
    return out


def table(kind, s, seed):
    """[s * s] int32 quantisers in raster order.  kinds: ones, pow2, odd, big (2^22 .. 2^31 - 1), band (near 2 |Y| of the large
    planes), outlier (a normal table with one entry 2^24 + 1), and dc=<q> (q at the DC, ones elsewhere)."""
    rng = np.random.default_rng(seed)
    n = s * s
    if kind == "ones":
        t = np.ones(n, np.int64)
    elif kind == "pow2":
        t = 1 << rng.integers(0, 3, n)
    elif kind == "odd":
        t = rng.choice(ODD_Q, n)
    elif kind == "big":
        t = rng.choice(BIG_Q, n)
    elif kind == "band":
        t = rng.integers(1 << 15, 1 << 18, n)
    elif kind == "outlier":
        t = np.clip(np.round(16 + 40 * np.add.outer(np.arange(s), np.arange(s)).ravel() / max(1, s - 1)), 1, None).astype(np.int64)
        t[rng.integers(0, n)] = (1 << 24) + 1
    elif kind.startswith("dc="):
        t = np.ones(n, np.int64)
        t[0] = int(kind[3:])
    else:
        raise ValueError(kind)
    return t.astype(np.int32)


# ------------------------------------------------------------------ planes: one row of leaves side by side, (H, W) = (s, n s)
def leaves_row(s, n):
    """(n, 3) int32 leaves x, y, s covering an s x (n s) plane"""
    return np.stack([np.arange(n) * s, np.zeros(n, np.int64), np.full(n, s)], 1).astype(np.int32)


def constant_plane(s, values):
    """leaf i constant values[i] (for s in POW2_ALPHA_SIZES its DC is exactly values[i] * s)"""
    v = np.asarray(values, np.float32)
    return np.repeat(np.repeat(v[None, :], s, 0), s, 1).astype(np.float32)


def tie_constants(s):
    """constants whose DC is an exact tie under q = 2^24, or the 2^24 + 1 case, for s with a power-of-two alpha_0: DC = (k + 1/2) 2^24
    for k = 0 .. 3 and both signs (1.5 (2^24) quantises to 1 under 2^24 + 1, to 2 under a float-held 2^24)"""
    dcs = [sg * (k + 0.5) * (1 << 24) for k in range(4) for sg in (1, -1)]
    return [np.float32(d / s) for d in dcs]


def float_held_table(Y0, limit=256):
    """[s * s] quantisers that separate the exact quantiser from a float-held one on the values Y0 of one leaf (raster order), for any
    block size: at up to `limit` positions with |y| >= 2^25, the least q > 2 |y| / 3 whose float32 image is at most 2 |y| / 3, so that
    |y| / q < 1.5 <= |y| / float32(q) (reference 1, float-held 2); 1 elsewhere"""
    t = np.ones(Y0.size, np.int64)
    for p in np.flatnonzero(np.abs(Y0.astype(np.float64)) >= 2.0 ** 25)[:limit]:
        m = 2.0 * abs(float(Y0[p])) / 3.0
        for q in range(int(np.floor(m)) + 1, int(np.floor(m)) + 16):
            if float(np.float32(q)) <= m:
                t[p] = q
                break
    return t.astype(np.int32)


def skip_vote_table(Y0, s):
    """[s * s] quantisers that put one value of every 8-row x 32-column block of a leaf (raster values Y0) in the skip window, its
    block's largest, with |y| / q in (0.5, 0.501), and every other value far below 0.499 q (q = 2^22, so the layer takes the float32
    quantiser): a vote unit of either kernel then holds one lane that must stop the skip, which a threshold of 0.501 would not"""
    t = np.full(s * s, 1 << 22, np.int64)
    a = np.abs(np.asarray(Y0, np.float64))
    u = vote_units(s, "wave64")
    for k in range(int(u.max()) + 1):
        idx = np.flatnonzero(u == k)
        p = idx[np.argmax(a[idx])]
        if not 1024.0 <= a[p] < 2.0 ** 21:
            continue
        q = int(np.ceil(2.0 * a[p])) - 1
        if 0.5 < a[p] / q < 0.501:
            t[p] = q
    return t.astype(np.int32)


def searched_table(oracle, plane, s, kind):
    """the tables searched for a plane from the oracle's Y of its first leaf: held (float_held_table), vote (skip_vote_table)"""
    Y0 = oracle_case(oracle, plane, s, table("ones", s, 0))[0][:s * s]
    return float_held_table(Y0) if kind == "held" else skip_vote_table(Y0, s)


def vote_plane(s, n, seed):
    """n leaves that are leaf 0 with alternating sign (the DCT is linear and a sign flip exact), |Y| mostly in [2^10, 2^16)"""
    X = large_plane(s, 1, seed, lo=2.0 ** 10, hi=2.0 ** 16)
    return np.concatenate([X if i % 2 == 0 else -X for i in range(n)], 1)


def large_plane(s, n, seed, lo=2.0 ** 15, hi=2.0 ** 17, spill=0.0):
    """n random leaves whose DCT values mostly lie in [lo, hi) in magnitude (orthonormal DCT: a uniform plane of amplitude a gives
    coefficients of standard deviation a / sqrt(3)); spill > 0 scales a random fraction of the leaves' rows by 4 so that the range
    guards see both sides of 2^17 inside a leaf, a row and a wave"""
    rng = np.random.default_rng(seed)
    a = np.sqrt(3.0) * np.sqrt(lo * hi)
    X = rng.uniform(-a, a, (s, n * s))
    if spill > 0:
        rows = rng.random(s) < spill
        X[rows] *= 4.0
    return X.astype(np.float32)


def basis_plane(s, n, seed, amp):
    """leaves that are one high-frequency DCT basis pattern each, of amplitude amp: a single large value far along the zigzag order
    and small residues elsewhere (for 64 x 64 leaves, a non-zero value past position 1 024 while every value before it is small)"""
    rng = np.random.default_rng(seed)
    k = np.arange(s)
    X = np.empty((s, n * s))
    for i in range(n):
        u, v = (int(x) for x in rng.integers(s // 2 + s // 4, s, 2))
        du = np.sqrt(2.0 / s) * np.cos(np.pi * (2 * k + 1) * u / (2 * s))
        dv = np.sqrt(2.0 / s) * np.cos(np.pi * (2 * k + 1) * v / (2 * s))
        X[:, i * s:(i + 1) * s] = amp * rng.uniform(0.1, 1.0) * np.outer(du, dv)
    return X.astype(np.float32)


def oracle_case(oracle, plane, s, qt):
    """-> (Y in raster order per leaf, flat; coefficients in zigzag order; Q per coefficient in zigzag order; zigzag positions;
    leaf index; leaf-row index) of the oracle's blocks_encode of a row of s x s leaves under table qt"""
    n = plane.shape[1] // s
    leaves = leaves_row(s, n)
    zz = zigzag(s)
    co, Y = oracle.blocks_encode(plane, leaves, {s: qt}, {s: zz.astype(np.int32)}, want_dct=True)
    Yz = Y.reshape(n, s * s)[:, zz].ravel()
    Qz = np.tile(qt.astype(np.int64)[zz], n)
    zpos = np.tile(np.arange(s * s), n)
    leaf = np.repeat(np.arange(n), s * s)
    row = leaf * s + np.tile(zz // s, n)
    return Y, Yz, co, Qz, zpos, leaf, row


# the families every quantiser test draws from: name -> (sizes, plane(s, seed), table kind, the mutants it must catch)
def _const(s, seed):
    return constant_plane(s, tie_constants(s))


def _large(s, seed):
    return large_plane(s, max(1, (1 << 16) // (s * s)), seed, spill=0.1)


def _huge(s, seed):
    return large_plane(s, max(1, (1 << 15) // (s * s)), seed, lo=2.0 ** 17, hi=2.0 ** 21)


def _band(s, seed):
    return large_plane(s, max(1, (1 << 16) // (s * s)), seed)


def _vast(s, seed):
    return large_plane(s, max(1, (1 << 14) // (s * s)), seed, lo=2.0 ** 24, hi=2.0 ** 27)


def _basis(s, seed):
    return basis_plane(s, 16, seed, 2.0 ** 28)


FAMILIES = {
    "const_dc_2^24": (POW2_ALPHA_SIZES[:4], _const, "dc=16777216", ("half_away_from_zero", "floor_x_plus_half")),
    "const_dc_2^24+1": (POW2_ALPHA_SIZES[:4], _const, "dc=16777217", ("float_held_quantiser",)),
    "large_ones": ((4, 8, 16, 32, 64), _large, "ones", ("half_away_from_zero", "floor_x_plus_half")),
    "large_pow2": ((2, 8, 32, 128), _large, "pow2", ("half_away_from_zero", "floor_x_plus_half")),
    "large_odd": ((4, 8, 16, 32, 64), _large, "odd", ("f32_product_uncorrected", "no_tie_to_even")),
    "huge_odd": ((8, 16, 64), _huge, "odd", ("f32_product_uncorrected", "no_tie_to_even")),
    "vast_odd": ((4, 8, 32, 64), _vast, "odd", ("f32_division", "f32_product_uncorrected", "no_tie_to_even")),
    "vast_big_q": ((4, 16, 32, 128), _vast, "big", ()),
    "band": ((8, 16, 32, 64), _band, "band", ("skip_at_0501",)),
    "basis_64_odd": ((64,), _basis, "odd", ("f32_product_uncorrected", "f32_division")),
}
