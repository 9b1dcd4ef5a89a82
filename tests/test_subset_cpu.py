"""Fault sets of a fixed weight without a GPU: the definition ``fault_subsets`` (colexicographic unranking and Floyd's draw),
``subset_table``, ``weight_distribution``, and ``dem_decode_sim(engine="numpy", fault_weight=..., subset=...)`` and
``dem_failure_spectrum`` on the CPU oracle against the exact logical error rate of a model small enough to enumerate.
Models and references: tests/subset_cases.py."""
import itertools
import json
import math
import os
import re

import numpy as np
import pytest

from bp_osd_amd import _lib, dem_decode_sim, dem_failure_spectrum, fault_subsets, subset_table, weight_distribution
from tests import dem_cases as dc
from tests import dem_weight_cases as wc
from tests import subset_cases as sc


def test_library_declares_the_subset_call():
    hdr = open(os.path.join(dc.ROOT, "include", "bposd_mi355x.h")).read()
    assert "bposd_dem_set_subset" in _lib.EXPORTED_SYMBOLS and "int bposd_dem_set_subset(" in hdr
    for name, value in (("OFF", 0), ("ENUMERATE", 1), ("RANDOM", 2)):
        assert re.search(rf"#define BPOSD_DEM_SUBSET_{name} {value}\b", hdr), name
    assert _lib.DEM_SUBSET == {None: 0, "enumerate": 1, "random": 2}
    assert "2^-49" in hdr  # the multiply-shift bias is stated


# --------------------------------------------------------------------------------------------------- colex
def test_colex_sequence_of_seven_choose_three():
    assert fault_subsets(0, 0, 5, 7, 3, "enumerate").tolist() == [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3], [0, 1, 4]]
    assert fault_subsets(0, 34, 1, 7, 3, "enumerate").tolist() == [[4, 5, 6]]
    a = fault_subsets(0, 0, 35, 7, 3, "enumerate")
    assert a.dtype == np.int64 and a.shape == (35, 3)


@pytest.mark.parametrize("n,w", [(1, 1), (5, 2), (9, 4), (12, 6), (13, 12), (66, 2), (20, 3)])
def test_colex_ranks_are_all_the_sets_once(n, w):
    C = math.comb(n, w)
    a = fault_subsets(0, 0, C, n, w, "enumerate")
    assert (np.diff(a, axis=1) > 0).all() and a.min() >= 0 and a.max() < n
    assert len({tuple(r) for r in a.tolist()}) == C
    assert a[-1].tolist() == list(range(n - w, n))  # the last rank: the top w positions
    # colexicographic: the sets ascend when compared from their largest element down
    keys = [tuple(reversed(r)) for r in a.tolist()]
    assert keys == sorted(keys)
    # the same ranks asked for in pieces
    cut = C // 3
    assert (np.concatenate([fault_subsets(0, 0, cut, n, w, "enumerate"), fault_subsets(0, cut, C - cut, n, w, "enumerate")]) == a).all()


def test_colex_edges():
    assert fault_subsets(0, 0, 1, 9, 0, "enumerate").shape == (1, 0)  # the one empty set
    assert fault_subsets(0, 0, 1, 64, 64, "enumerate").tolist() == [list(range(64))]
    big = math.comb(1031, 4)
    assert fault_subsets(0, big - 1, 1, 1031, 4, "enumerate").tolist() == [[1027, 1028, 1029, 1030]]
    a = fault_subsets(0, 2 ** 32 + 12345, 3, 1031, 4, "enumerate")  # a rank is sum_j C(c_j, j)
    assert [sum(math.comb(c, j + 1) for j, c in enumerate(r)) for r in a.tolist()] == [2 ** 32 + 12345 + i for i in range(3)]
    with pytest.raises(ValueError, match="only 35 sets"):
        fault_subsets(0, 30, 6, 7, 3, "enumerate")
    with pytest.raises(ValueError, match="2\\^63"):
        fault_subsets(0, 0, 1, 200, 64, "enumerate")
    with pytest.raises(ValueError, match="weight"):
        fault_subsets(0, 0, 1, 5, 6, "enumerate")
    with pytest.raises(ValueError, match="weight"):
        fault_subsets(0, 0, 1, 100, 65, "random")
    with pytest.raises(ValueError, match="mode"):
        fault_subsets(0, 0, 1, 5, 2, "lex")


# --------------------------------------------------------------------------------------------------- Floyd
@pytest.mark.parametrize("n,w", [(1, 1), (8, 7), (8, 3), (128, 64), (1031, 4), (70, 0)])
def test_floyd_rows_are_sets(n, w):
    a = fault_subsets(sc.SEED, 2 ** 32 - 3, 500, n, w, "random")
    assert a.shape == (500, w) and a.dtype == np.int64
    if w:
        assert (np.diff(a, axis=1) > 0).all() and a.min() >= 0 and a.max() < n
    # independent of the batch: the same shots asked for in pieces, and another seed draws other sets
    assert (np.concatenate([fault_subsets(sc.SEED, 2 ** 32 - 3, 7, n, w, "random"), fault_subsets(sc.SEED, 2 ** 32 + 4, 493, n, w, "random")]) == a).all()
    if 0 < w < n:
        assert (fault_subsets(sc.SEED + 1, 2 ** 32 - 3, 500, n, w, "random") != a).any()


def test_floyd_by_hand_takes_j_on_a_collision():
    """The definition restated with Python ints, shot by shot; n = 8, w = 7 collides on nearly every step."""
    from bp_osd_amd.sim import philox4x32_10

    n, w, seed, first = 8, 7, 5, 2 ** 40 + 9
    a = fault_subsets(seed, first, 200, n, w, "random")
    collisions = 0
    for row, s in zip(a.tolist(), range(first, first + 200)):
        chosen = []
        for i in range(w):
            j = n - w + i
            o = [int(x) for x in philox4x32_10((s & 0xFFFFFFFF, s >> 32, i >> 1, 1), (seed & 0xFFFFFFFF, seed >> 32))]
            u = o[2 * (i & 1)] | (o[2 * (i & 1) + 1] << 32)
            t = (u * (j + 1)) >> 64
            collisions += t in chosen
            chosen.append(j if t in chosen else t)
        assert sorted(chosen) == row
    assert collisions > 200  # more than one per shot on average


def test_floyd_is_uniform_on_eight_choose_three():
    """56 000 draws: every one of the 56 subsets within 5 sigma of 1000 (sigma^2 = 1000 (1 - 1/56); at seed 5 the worst is 2.6)."""
    a = fault_subsets(5, 0, 56000, 8, 3, "random")
    index = {c: i for i, c in enumerate(itertools.combinations(range(8), 3))}
    count = np.bincount([index[tuple(r)] for r in a.tolist()], minlength=56)
    worst = np.abs(count - 1000).max() / math.sqrt(1000 * (1 - 1 / 56))
    print("worst deviation in sigma:", worst)
    assert count.sum() == 56000 and worst < 5


# --------------------------------------------------------------------------------------------------- the tables
def test_weight_distribution_against_all_rows():
    _, _, p = wc.exact_model()
    N = p.shape[0]
    f = (np.arange(2 ** N)[:, None] >> np.arange(N)) & 1
    prob = np.where(f == 1, p, 1 - p).prod(axis=1)
    brute = np.array([math.fsum(prob[f.sum(axis=1) == w]) for w in range(N + 1)])
    full = weight_distribution(p, N)
    assert full.shape == (N + 1,) and full == pytest.approx(brute, rel=1e-12)
    assert math.fsum(full) == pytest.approx(1.0, abs=1e-14)
    assert weight_distribution(p, 3) == pytest.approx(brute[:4], rel=1e-12)
    sup = [0, 2, 5, 11]
    sub = (np.arange(16)[:, None] >> np.arange(4)) & 1
    pr = np.where(sub == 1, p[sup], 1 - p[sup]).prod(axis=1)
    assert weight_distribution(p, 4, support=sup) == pytest.approx([math.fsum(pr[sub.sum(axis=1) == w]) for w in range(5)], rel=1e-12)
    # priors of 0 and 1 need no special case
    assert weight_distribution([0.0, 1.0, 0.25], 3) == pytest.approx([0.0, 0.75, 0.25, 0.0])


def test_subset_table_by_hand_and_refusals():
    p = np.array([0.25, 0.0, 0.5, 1.0, 0.01])
    incr, c0 = subset_table(p, [0, 2, 4])
    assert incr.dtype == np.int64 and incr.tolist() == [round(math.log(1 / 3) * 2 ** 32), 0, 0, 0, round(math.log(1 / 99) * 2 ** 32)]
    assert c0 == pytest.approx(math.log(0.75) + math.log(0.5) + math.log(0.99), rel=1e-15) and isinstance(c0, float)
    # P({0, 4}) = p0 (1 - p2) p4
    assert math.exp(c0 + (int(incr[0]) + int(incr[4])) / 2 ** 32) == pytest.approx(0.25 * 0.5 * 0.01, rel=2.0 ** -31)
    for bad in (1, 3):
        with pytest.raises(ValueError, match=f"fault {bad}"):
            subset_table(p, [0, bad, 4])
    for sup in ([2, 0], [0, 0], [0, 5], [-1, 2]):
        with pytest.raises(ValueError, match="ascending"):
            subset_table(p, sup)


def test_front_end_refusals():
    H, L, p = wc.exact_model()
    make = lambda **kw: dem_decode_sim(H, L, kw.pop("priors", p), engine="numpy", decoder_factory=lambda *a, **k: None, run_sim=False, **kw)
    with pytest.raises(ValueError, match="go together"):
        make(fault_weight=2)
    with pytest.raises(ValueError, match="go together"):
        make(subset="random")
    with pytest.raises(ValueError, match="exclude"):
        make(fault_weight=2, subset="random", sample_scale=2.0)
    with pytest.raises(ValueError, match="exclude"):
        make(fault_weight=2, subset="random", sample_priors=p.copy())
    with pytest.raises(ValueError, match="subset must be"):
        make(fault_weight=2, subset="lex")
    for w in (-1, 14, 2.0, True):
        with pytest.raises(ValueError, match="fault_weight"):
            make(fault_weight=w, subset="random")
    with pytest.raises(ValueError, match="only 78 sets"):
        make(fault_weight=2, subset="enumerate", target_runs=79)
    one = p.copy()
    one[6] = 1.0
    with pytest.raises(ValueError, match="fault 6"):
        make(priors=one, fault_weight=2, subset="random")
    zero = p.copy()
    zero[[1, 4]] = 0.0  # the default support leaves the faults that never fire out: n = 11
    sim = make(priors=zero, fault_weight=2, subset="enumerate")
    assert sim.stratum_size == 55 and sim.target_runs == 55 and sim._support.tolist() == [0, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12]
    assert make(fault_weight=2, subset="random").target_runs == 100 and make().target_runs == 100
    with pytest.raises(ValueError, match="support belongs"):
        make(support=[0, 1])
    with pytest.raises(ValueError, match="set_fault_weight"):
        make().set_fault_weight(1, "random")


# --------------------------------------------------------------------------------------------------- the exact answer
def test_enumerated_strata_sum_to_the_exact_rate():
    """exact_model, every stratum w = 0 .. 13 enumerated on the oracle: the failing osdw sets of weight 0 .. 3, the strata's
    sizes and masses, error bars of exactly 0.0, and sum_w osdw_failure_mass = exact_osdw_rate() within 1e-8 relative (the
    integer log-weights round by 13 * 2^-33 = 1.5e-9 at most; observed 2.2e-10)."""
    _, _, p = wc.exact_model()
    strata = sc.exact_strata()
    dist = weight_distribution(p, 13)
    for w, s in enumerate(strata):
        assert s["run_count"] == s["stratum_size"] == math.comb(13, w) and isinstance(s["stratum_size"], int)
        assert s["stratum_mass"] == dist[w]
        for key in ("bp", "osd0", "osdw"):
            assert s[f"{key}_failure_mass_eb"] == 0.0 and 0.0 <= s[f"{key}_failure_mass"] <= s["stratum_mass"] * (1 + 1e-8)
        assert s["logw"].dtype == np.int64
    assert tuple(s["run_count"] - s["osdw_success_count"] for s in strata[:4]) == sc.EXACT_FAILING
    # a stratum in which every set fails carries its whole mass: the table and the distribution agree
    full = [s for s in strata if s["osdw_success_count"] == 0]
    assert full and all(s["osdw_failure_mass"] == pytest.approx(s["stratum_mass"], rel=1e-8) for s in full)
    total, exact = math.fsum(s["osdw_failure_mass"] for s in strata), wc.exact_osdw_rate()
    print("sum of the strata", total, "exact", exact, "relative difference", abs(total - exact) / exact)
    assert abs(total - exact) <= sc.EXACT_REL * exact
    assert math.fsum(s["osdw_failure_mass"] for s in strata[:4]) > 0.998 * exact  # strata 0 .. 3 carry 99.89 % of the rate


def test_run_does_not_depend_on_the_batch_size_and_reports():
    H, L, p = wc.exact_model()
    ref = sc.exact_strata()[3]
    sim = sc.oracle_sim(H, L, p, 3, "enumerate", batch_size=97)  # 286 = 2 * 97 + 92: the last batch is clamped
    got = sc.snapshot(sim)
    for k in dc.COUNTS + ("stratum_size", "stratum_mass", "osdw_failure_mass_eb"):
        assert got[k] == ref[k], k
    assert got["osdw_failure_mass"] == pytest.approx(ref["osdw_failure_mass"], rel=1e-13)
    assert sim.last_batch("faults").shape == (92, 1)
    out = json.loads(sim.output_dict())
    assert out["fault_weight"] == 3 and out["subset"] == "enumerate" and out["stratum_size"] == 286
    assert out["osdw_failure_mass"] == sim.osdw_failure_mass and out["osdw_logical_error_rate"] == 152 / 286
    # a part of a stratum, and a drawn one, have error bars; the drawn estimate is within 5 of them of the enumerated mass
    part = sc.oracle_sim(H, L, p, 3, "enumerate", target_runs=100)
    assert part.run_count == 100 and part.osdw_failure_mass_eb > 0.0
    drawn = sc.oracle_sim(H, L, p, 3, "random", target_runs=2000)
    assert drawn.osdw_failure_mass_eb > 0.0 and abs(drawn.osdw_failure_mass - ref["osdw_failure_mass"]) < 5 * drawn.osdw_failure_mass_eb
    # every set of a drawn batch has weight 3, and its log-weight is the table's sum
    f = dc.unpack(drawn.last_batch("faults"), 13)
    assert (f.sum(axis=1) == 3).all() and (drawn.last_batch("logw") == f.astype(np.int64) @ subset_table(p, np.arange(13))[0]).all()


def test_failure_spectrum_of_the_exact_model():
    from oracle import OracleDecoder

    H, L, p = wc.exact_model()
    strata = sc.exact_strata()
    sp = dem_failure_spectrum(H, L, p, 4, 300, engine="numpy", seed=dc.RUN_SEED, decoder_factory=OracleDecoder, harvest=4, **dc.DECODER)
    assert sp["corrected_weight"] == 1 and sp["min_failing_weight"] == 2
    assert [r["mode"] for r in sp["strata"]] == ["enumerate"] * 4 + ["random"]  # C(13, 4) = 715 > 300
    assert [r["runs"] for r in sp["strata"]] == [1, 13, 78, 286, 300]
    for r, s in zip(sp["strata"][:4], strata):
        assert r["osdw_failures"] == s["run_count"] - s["osdw_success_count"] and r["osdw_failure_mass_eb"] == 0.0
        assert r["osdw_failure_mass"] == pytest.approx(s["osdw_failure_mass"], rel=1e-13) and r["stratum_mass"] == s["stratum_mass"]
    drawn = sp["strata"][4]
    assert drawn["osdw_failure_mass_eb"] > 0 and abs(drawn["osdw_failure_mass"] - strata[4]["osdw_failure_mass"]) < 5 * drawn["osdw_failure_mass_eb"]
    assert sp["logical_error_rate_lower"] == pytest.approx(math.fsum(r["osdw_failure_mass"] for r in sp["strata"]))
    assert sp["logical_error_rate_lower_eb"] == drawn["osdw_failure_mass_eb"]
    assert sp["tail_mass"] == pytest.approx(1 - math.fsum(weight_distribution(p, 4)), rel=1e-6)
    exact = wc.exact_osdw_rate()
    slack = 5 * sp["logical_error_rate_lower_eb"] + 1e-8 * exact
    assert sp["logical_error_rate_lower"] - slack <= exact <= sp["logical_error_rate_lower"] + sp["tail_mass"] + slack
    # the first failing stratum lists its malignant sets: weight-2 fault sets whose residual is a logical fault
    bad = sp["strata"][2]["failures"]
    assert bad["shot"].size == 4 and (dc.unpack(bad["faults"], 13).sum(axis=1) == 2).all() and sp["strata"][2]["min_logical_weight"] == 3
    assert sp["strata"][1]["failures"]["shot"].size == 0
    with pytest.raises(ValueError, match="max_weight"):
        dem_failure_spectrum(H, L, p, 14, 10, engine="numpy", decoder_factory=OracleDecoder)
    # a decoder that fails on the empty set corrects nothing
    always_wrong = L.copy()

    class Flipper(OracleDecoder):
        def decode_batch(self, det):
            r = super().decode_batch(det)
            r["osdw"] = np.asarray(r["osdw"], dtype=np.uint8) ^ np.asarray(always_wrong.toarray()[0], dtype=np.uint8)
            return r

    flipped = dem_failure_spectrum(H, L, p, 1, 20, engine="numpy", decoder_factory=Flipper, **dc.DECODER)
    assert flipped["corrected_weight"] == -1 and flipped["min_failing_weight"] == 0
