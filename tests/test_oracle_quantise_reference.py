"""CPU: the oracle's quantiser (blocks_encode) against tests/quantise_reference.py on every case family the GPU quantiser tests draw
from, every mutant of the reference shown to differ on the family meant for it, and each family's reach of its edge bounded below."""
import numpy as np
import pytest

import quantise_reference as R

# the least of each classifier count a family must reach (summed over its sizes): a generator that stops reaching its edge fails
MINIMA = {
    "const_dc_2^24": {"ties": 24, "q_above_2^22": 4},
    "const_dc_2^24+1": {"q_above_2^24": 4, "at_or_above_2^17": 16},
    "large_ones": {"ties": 1000, "leaves_mixing_2^17": 100, "rows_mixing_2^17": 1000, "waves_mixing_2^17": 1000},
    "large_pow2": {"ties": 500, "rows_mixing_2^17": 1000},
    "large_odd": {"ties": 100, "wrong_way_near_ties": 1000},
    "huge_odd": {"ties": 100, "wrong_way_near_ties": 1000, "at_or_above_2^17": 10000},
    "vast_odd": {"ties": 100, "wrong_way_near_ties": 10000},
    "vast_big_q": {"q_above_2^24": 10000, "nonzero": 10000},
    "band": {"skip_band_0499_0501": 200},
    "basis_64_odd": {"nonzero_past_zigzag_1024": 50, "at_or_above_2^17": 8},
}


def test_reference_refuses_what_the_contract_leaves_undefined():
    with pytest.raises(ValueError):
        R.reference(np.float32([np.nan]), [1])
    with pytest.raises(ValueError):
        R.reference(np.float32([2.0 ** 31]), [1])
    with pytest.raises(ValueError):
        R.reference(np.float32([1.0]), [0])
    assert R.reference(np.float32([2.5, -2.5, 3.5, 25165824.0]), [1, 1, 1, (1 << 24) + 1]).tolist() == [2, -2, 4, 1]


def test_the_float_held_quantiser_case(oracle):
    """a constant 4 x 4 leaf of 6291456 has DC 1.5 (2^24), which quantises to 1 under 2^24 + 1 and to 2 under the float32 image of that
    quantiser"""
    plane = R.constant_plane(4, [6291456.0])
    Y, Yz, co, Qz, *_ = R.oracle_case(oracle, plane, 4, R.table("dc=16777217", 4, 0))
    assert Yz[0] == np.float32(25165824.0) and co[0] == 1 and R.m_float_held_q(Yz, Qz)[0] == 2


@pytest.mark.parametrize("family", list(R.FAMILIES))
def test_oracle_equals_reference_and_mutants_differ(oracle, family):
    sizes, gen, kind, mutants = R.FAMILIES[family]
    total, diff = {}, dict.fromkeys(R.MUTANTS, 0)
    for s in sizes:
        plane = gen(s, s)
        qt = R.table(kind, s, 100 + s)
        Y, Yz, co, Qz, zpos, leaf, row = R.oracle_case(oracle, plane, s, qt)
        assert np.array_equal(co, R.reference(Yz, Qz)), f"{family} s={s}: oracle != reference"
        c = R.classify(Yz, Qz, zpos if s == 64 else None, leaf, row)
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
        for m, f in R.MUTANTS.items():
            diff[m] += int((f(Yz, Qz) != co).sum())
    print(f"\n{family}: {total}\n{family}: mutant differences {diff}")
    for m in mutants:
        assert diff[m] > 0, f"{family}: mutant {m} is not caught"
    for k, lo in MINIMA[family].items():
        assert total.get(k, 0) >= lo, f"{family}: {k} = {total.get(k, 0)} < {lo}"


def test_every_mutant_has_a_family():
    caught = {m for *_, ms in R.FAMILIES.values() for m in ms}
    assert caught == set(R.MUTANTS)


@pytest.mark.parametrize("s", R.IRRATIONAL_ALPHA_SIZES[:4])
def test_float_held_table_separates_at_irrational_alpha_sizes(oracle, s):
    """where no constant leaf has an exact DC, a table searched for the plane's large values puts them in the float-held window"""
    plane = R.large_plane(s, max(1, (1 << 14) // (s * s)), s + 5, lo=2.0 ** 25, hi=2.0 ** 27)
    t = R.searched_table(oracle, plane, s, "held")
    _, Yz, co, Qz, *_ = R.oracle_case(oracle, plane, s, t)
    assert np.array_equal(co, R.reference(Yz, Qz))
    n = int((R.m_float_held_q(Yz, Qz) != co).sum())
    print(f"\ns={s}: {int((t > (1 << 24)).sum())} quantisers above 2^24, {n} values the float-held quantiser gets wrong")
    assert n >= 1


@pytest.mark.parametrize("s,unit", [(32, "mfma"), (64, "mfma"), (64, "wave64"), (128, "mfma")])
def test_skip_vote_table_reaches_every_vote_unit_kind(oracle, s, unit):
    """the searched skip table puts values where the kernels' wave vote decides: a vote at 0.501 q instead of 0.499 q changes the result
    of many units, while the value-by-value mutant alone would say nothing about a vote"""
    plane = R.vote_plane(s, 4, s + 9)
    t = R.searched_table(oracle, plane, s, "vote")
    assert t.max() <= (1 << 22)                    # the layer stays on the float32 quantiser (no q_slow)
    Y, Yz, co, Qz, *_ = R.oracle_case(oracle, plane, s, t)
    assert np.array_equal(co, R.reference(Yz, Qz))
    n = plane.shape[1] // s
    Yr = Y.reshape(n, s * s)
    assert np.array_equal(R.m_skip_vote(Yr, t, s, unit, thr=0.499), R.reference(Yr, np.broadcast_to(t, Yr.shape)))   # the right vote is exact
    hit = R.vote_units_in_window(Yr, t, s, unit)
    blocks = (s // 8) * (s // 32) - (unit == "wave64")
    print(f"\ns={s} {unit}: {int((t < (1 << 22)).sum())} window quantisers, {hit} of {n * blocks} blocks' vote units reach the window")
    assert hit >= n * blocks * 3 // 4
