"""The table of tests/local_codes.py, checked without a GPU: every row's matrix is (3,6)-regular with n = 2m and lands on the
wave table, the bodies, the PAIRKEY and the padding the row pins (the host-only exports run the same layout search
bposd_create runs); the rows together reach every loop body of bp_local_kernel at both position counts; the window edges
are in the table; the matrix past the window is refused; and every row's q is one at which the oracle alone leaves
between 0.1 % and 60 % of the GPU test's H e syndromes unconverged."""
import numpy as np
import pytest

from bp_osd_amd import _lib
from bp_osd_amd.build import build_library
from tests.local_codes import (ALL_KEYS_ROWS, KEYS, LOCAL_CODES, MIXED, N_SPECIAL, NOT_FOUND, PAIR_KEYS, PAST_WINDOW,
                               assert_row_tables, coverage, decoder_settings, matrix_of, per_bit_probs, row_by_id,
                               syndrome_seed, syndromes, wave_tables)

IDS = [r["id"] for r in LOCAL_CODES]


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


@pytest.fixture(scope="module")
def tables(lib):
    """{row id: wave_tables(...)}: one layout search per row for the whole module"""
    return {r["id"]: wave_tables(lib, matrix_of(r)) for r in LOCAL_CODES}


def _regular_3_6(H, m):
    assert H.shape == (m, 2 * m) and H.dtype == np.uint8 and (H.data == 1).all()
    assert (np.diff(H.indptr) == 6).all() and (np.bincount(H.indices, minlength=2 * m) == 3).all()


@pytest.mark.parametrize("rid", IDS)
def test_row_matrix_and_wave_table(tables, rid):
    """(3,6)-regular with n = 2m, the rank the row states, and the wave table the row pins."""
    from bp_osd_amd.codes import gf2_rank

    row = row_by_id(rid)
    H = matrix_of(row)
    _regular_3_6(H, row["m"])
    assert (gf2_rank(H.toarray()) == row["m"]) == row["full_rank"]
    t = tables[rid]
    print(rid, "MP", t["MP"], "waves", t["waves"], "bodies", t["body"], "PAIRKEY", t["pairkey"], "generic", t["generic"],
          "checks per group", t["group_checks"])
    assert_row_tables(row, t)
    assert IDS.count(rid) == 1


def test_every_body_is_reached_at_both_sizes(tables):
    """For 1024 and for 2048 positions: each of the seven keys is run by a wave whose two groups both hold checks, and the
    generic body by such a wave of two different uniform keys.  Every pair body is reached at one size at least, and of
    the 12 (MP, pair body) combinations at most 2 are missing -- those NOT_FOUND names, no other.  A generic wave
    (k, mixed) with k != PAIRKEY is reached or named in NOT_FOUND."""
    cov = coverage(tables)
    for MP in (1024, 2048):
        print(f"MP {MP}: keyed bodies on real waves {sorted(cov['keyed'][MP])}; pair bodies {sorted(cov['pair'][MP])}; "
              f"generic body on waves of two uniform keys {sorted(cov['generic_uniform'][MP])}; "
              f"on (k, mixed) waves (k, PAIRKEY) {sorted(cov['generic_mixed'][MP])}")
        assert cov["keyed"][MP] == set(KEYS), (MP, sorted(cov["keyed"][MP]))
        assert cov["generic_uniform"][MP], MP
        assert all(a != b and MIXED not in (a, b) for a, b in cov["generic_uniform"][MP])
        assert bool(cov["generic_mixed"][MP]) != (MP in NOT_FOUND["generic_mixed"]), MP
    want = {(MP, 32 + k) for MP in (1024, 2048) for k in PAIR_KEYS}
    have = {(MP, b) for MP in (1024, 2048) for b in cov["pair"][MP]}
    missing = want - have
    print("pair bodies not reached:", sorted(missing), "-- NOT_FOUND:", NOT_FOUND)
    assert have <= want and missing == set(NOT_FOUND["pair"]) and len(missing) <= 2
    for k in PAIR_KEYS:
        assert (1024, 32 + k) in have or (2048, 32 + k) in have, k
    # every body a row says it is there for is one its table has (assert_row_tables), and no body is covered by accident
    # only: each (MP, body) of the coverage is named by some row's for_bodies
    named = {(r["MP"], b) for r in LOCAL_CODES for b in r["for_bodies"]}
    for MP in (1024, 2048):
        assert {(MP, b) for b in cov["keyed"][MP] | cov["pair"][MP]} | {(MP, -1)} <= named, MP


def test_rows_of_the_suites_own_codes_are_in_the_table():
    makes = {r["make"] for r in LOCAL_CODES}
    assert {("h1922", "hz"), ("h1922", "hx"), ("hgp_reg33", 31, 3, "hz"), ("hgp_circ", 45, (0, 2, 5), "hz")} <= makes


def test_window_edges(tables):
    """m = 64, 65, 128, 1024, 1025 and 2048: the position count, and the padding-only groups the row pins -- never more
    than the groups the checks leave empty when packed densely, none at m = 1024 and m = 2048 (every position holds a
    check), and waves made of padding only at 64, 65, 128 and 1025."""
    by_m = {r["m"]: r for r in LOCAL_CODES if r["make"][0] == "reg36"}
    for m, MP in ((64, 1024), (65, 1024), (128, 1024), (1024, 1024), (1025, 2048), (2048, 2048)):
        row = by_m[m]
        t = tables[row["id"]]
        G = MP // 64
        assert t["MP"] == row["MP"] == MP
        assert t["padding_only_groups"] == row["pad"] <= G - -(-m // 64)
        assert MP - m == sum(64 - c for c in t["group_checks"])
        padding_waves = sum(not (a or b) for a, b in t["real"])
        print(f"m {m}: MP {MP}, {MP - m} padding positions, {row['pad']} padding-only groups, {padding_waves} waves of "
              f"padding only, checks per group {t['group_checks']}")
        if m in (1024, 2048):
            assert row["pad"] == 0 and min(t["group_checks"]) == 64
        else:
            assert padding_waves >= 1
            assert any(0 < c < 64 for c in t["group_checks"])  # real and padding lanes inside one group
            for (a, b), real in zip(t["waves"], t["real"]):  # a padding-only group computes its toy graph under any
                if not (real[0] or real[1]):  # key: the host gives it key 0 and the wave runs body 0
                    assert (a, b) == (0, 0)
    assert tables["reg65_s1"]["real"].count((True, False)) >= 1  # a wave of a real and a padding-only group


def test_all_keys_rows_hold_all_seven_keys(tables):
    assert {row_by_id(r)["MP"] for r in ALL_KEYS_ROWS} == {1024, 2048}
    for rid in ALL_KEYS_ROWS:
        assert set(tables[rid]["group_key"]) == set(KEYS) and row_by_id(rid)["full_rank"]


def test_one_past_the_window_is_refused(lib):
    """m = 2050: (3,6)-regular, and the layout search's admission test refuses it (BPOSD_ERR_UNSUPPORTED).  bposd_create's
    rules (bposd_capi.hip, launch_bp_lds.hip: pick_shape) then leave no LDS shape either -- shape 8 holds two checks per
    thread on at most 1024 threads -- so BP is HBM-resident, which tests/test_gpu_local_bodies.py asserts on the GPU."""
    from bp_osd_amd.codes import gf2_rank

    H = matrix_of(PAST_WINDOW)
    m = PAST_WINDOW["m"]
    assert m > 2048
    _regular_3_6(H, m)
    assert (gf2_rank(H.toarray()) == m) == PAST_WINDOW["full_rank"]
    with pytest.raises(ValueError, match=f"status {_lib.BPOSD_ERR_UNSUPPORTED}"):
        wave_tables(lib, H)
    p2 = lambda x: 1 << max(6, (x - 1).bit_length())
    assert p2(max(-(-m // 2), -(-2 * m // 4))) > 1024  # shape_threads(h, 8) > 1024: pick_shape returns 0


@pytest.mark.parametrize("rid", IDS + [PAST_WINDOW["id"]])
def test_row_q_leaves_part_of_the_batch_unconverged(rid):
    """The oracle alone, max_iter 30, on the first 256 H e syndromes of the batch the GPU test decodes: between 0.1 % and
    60 % unconverged, under the uniform and under the per-bit channel."""
    from oracle import OracleDecoder

    row = PAST_WINDOW if rid == PAST_WINDOW["id"] else row_by_id(rid)
    H = matrix_of(row)
    syn = syndromes(H, row["q"], N_SPECIAL + 256, syndrome_seed(row))
    o = OracleDecoder(H, **decoder_settings(row["q"], 30))
    for channel in ("uniform", "per_bit"):
        if channel == "per_bit":
            o.update_channel_probs(per_bit_probs(row))
        unconverged = float((o.decode_batch(syn, want_llr=False)["converged"][N_SPECIAL:] == 0).mean())
        print(rid, "q", row["q"], channel, "unconverged", unconverged)
        assert 0.001 <= unconverged <= 0.6, (rid, channel, unconverged)
