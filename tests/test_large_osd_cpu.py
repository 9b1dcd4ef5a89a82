"""tests/large_osd_cases.py kept honest without a GPU: the designed panel list lengths against a plain numpy elimination
under two pivot-row rules and in both elimination modes, the coverage of every panel form and threshold, the mask bits of
the apply passes, and -- on the CPU oracle -- the column order the chosen channel forces.  Run with ``-s`` to see the lines
that the comments of tests/large_osd_cases.py quote."""
import numpy as np
import pytest

from tests import large_osd_cases as lc

MODES = ("gauss", "jordan")
RULES = ("lowest", "highest")
MODE_OF = {"osd_0": "gauss", "osd_e": "gauss", "osd_cs": "jordan"}
PANEL_IDS = [c["id"] for c in lc.PANEL_CASES]
ROWS_IDS = [c["id"] for c in lc.PANEL_CASES if c["rows"]]


def _sorted_dense(case_id, perm=None):
    H, p = lc.panel_pcm(case_id)
    return np.asarray(H[:, p if perm is None else perm].todense())


_RESTATED = {}


def _restated(case_id):
    """{(mode, rule): (lengths, bits, nrank, npiv, last)} in the table's column order, once per process."""
    if case_id not in _RESTATED:
        Hs = _sorted_dense(case_id)
        _RESTATED[case_id] = {(mo, ru): lc.panel_list_lengths(Hs, min(Hs.shape), mo, ru) for mo in MODES for ru in RULES}
    return _RESTATED[case_id]


def test_table_holds_the_lists_asked_for():
    """One matrix per RPT at an exact m, with the list lengths that sit on the form boundaries."""
    want = {"rpt2_m2048": (2, 2048, (128, 129, 256, 257, 512, 513)), "rpt2_m1316": (2, 1316, (1024, 100)),
            "rpt4_m3265": (4, 3265, (1025, 2048, 64)), "rpt8_m8192": (8, 8192, (2049, 2048, 1025, 1024, 513)),
            "rpt16_m8193": (16, 8193, (2049, 2049, 1025, 129)), "rpt16_m16384": (16, 16384, (2049,) * 4 + (1024, 1025, 2048))}
    assert set(want) == set(PANEL_IDS)
    for cid, (rpt, m, lists) in want.items():
        case = lc.PANEL_BY_ID[cid]
        H, perm = lc.panel_pcm(cid)
        assert H.shape == (m, lc.case_n(case)) and lc.rpt_of(m) == rpt
        have = [b for b in case["blocks"] if b != lc.C]
        for L in set(lists):
            assert have.count(L) >= lists.count(L), (cid, L)
        assert lc.C in case["blocks"]
        assert sorted(perm) == list(range(H.shape[1]))
    methods = [r for c in lc.PANEL_CASES for r in c["runs"]]
    assert ("osd_e", 16) in methods and ("osd_cs", 17) in methods
    rows_modes = {MODE_OF[lc.PANEL_BY_ID[i]["rows"][0]] for i in ROWS_IDS}
    assert rows_modes == {"gauss", "jordan"}
    assert sum(1 for c in lc.PANEL_CASES if c["rand"]) >= 2


@pytest.mark.parametrize("case_id", PANEL_IDS)
def test_designed_lengths_equal_the_restatement(case_id):
    case = lc.PANEL_BY_ID[case_id]
    want = lc.designed_lengths(case)
    got = _restated(case_id)
    ranks = {v[2] for v in got.values()}
    assert len(ranks) == 1
    line = [f"{case_id} m {lc.case_m(case)} n {lc.case_n(case)} rank {ranks.pop()}"]
    for mo in MODES:
        for ru in RULES:
            lengths, bits, _, _, _ = got[(mo, ru)]
            # (a further entry is the tail's panel, reached only where the rank is not complete before it: not designed)
            assert lengths[:len(want)] == want, (mo, ru, lengths)
            assert len(bits) >= len(want) - 1
        a, b = (lc.passbits(got[(mo, ru)][1]) for ru in RULES)
        line.append(f"passbits {mo} " + " ".join(f"{x}/{y}" for x, y in zip(a, b)))
    print("\n  " + "   ".join(line))


@pytest.mark.parametrize("case_id", ROWS_IDS)
def test_every_per_shot_order_keeps_the_designed_lengths(case_id):
    """A channel per shot reorders whole panels (and the columns inside them): the same multiset of list lengths in another
    order, the moved panel first in shot 0 and last in shot 1, so that a form is met with any number of groups open."""
    case = lc.PANEL_BY_ID[case_id]
    porders, perms = lc.shot_orders(case_id)
    H, _ = lc.panel_pcm(case_id)
    base = lc.designed_lengths(case)
    assert len(perms) == lc.ROWS_SHOTS <= case["he"] + 1
    seen_at = set()
    for b, (order, perm) in enumerate(zip(porders, perms)):
        assert sorted(perm) == list(range(H.shape[1]))
        want = lc.designed_lengths(case, order)
        assert sorted(want) == sorted(base)
        seen_at.add(want.index(case["move"]) % lc.OSDL_K)
        Hs = _sorted_dense(case_id, perm)
        for mo in MODES:
            for ru in RULES:
                lengths, _, nrank, _, _ = lc.panel_list_lengths(Hs, min(Hs.shape), mo, ru)
                assert lengths[:len(want)] == want, (b, mo, ru, lengths)
                assert nrank == _restated(case_id)[(mo, ru)][2]
    assert lc.designed_lengths(case, porders[0])[0] == case["move"] == lc.designed_lengths(case, porders[1])[-1]
    assert seen_at == set(range(lc.OSDL_K)), "the moved panel is not met with 0 .. OSDL_K - 1 groups open"
    assert len({tuple(o) for o in porders}) == lc.ROWS_SHOTS


def test_every_form_and_threshold_is_hit_in_both_modes():
    hit = {mo: set() for mo in MODES}
    for case in lc.PANEL_CASES:
        for method, _ in case["runs"] + ((case["rows"],) if case["rows"] else ()):
            mo = MODE_OF[method]
            for ru in RULES:  # (equal under both rules, asserted above)
                hit[mo].update(_restated(case["id"])[(mo, ru)][0][:len(case["blocks"])])
    rows = []
    for mo in MODES:
        classes = {lc.form_class(x) for x in hit[mo] if x > 0}
        assert classes == set(range(len(lc.FORM_CLASSES))), (mo, classes)
        assert set(lc.THRESHOLDS) <= hit[mo], (mo, sorted(set(lc.THRESHOLDS) - hit[mo]))
        rows.append(f"{mo}: " + "  ".join(f"{lo}..{hi if hi < 1 << 30 else ''}: {sorted(x for x in hit[mo] if lo <= x <= hi)}"
                                          for lo, hi in lc.FORM_CLASSES))
    print("\n  " + "\n  ".join(rows))


def test_every_form_meets_a_panel_with_fewer_than_64_pivots():
    """Where every panel finds 64 pivots, pivot q is column q of its panel and a form that confused the two would pass.  Panels
    of every form class have columns that are sums of two others (``deficit``) and find 63 or 62, in both modes, the
    threshold lengths 129 .. 2049 among them -- and full panels stay in every class too."""
    for mo in MODES:
        short, full = {}, {}
        for case in lc.PANEL_CASES:
            P = len(case["blocks"])
            per_rule = [_restated(case["id"])[(mo, ru)] for ru in RULES]
            assert per_rule[0][3] == per_rule[1][3], "the pivots per panel do not depend on the pivot-row rule"
            lengths, _, _, npiv, _ = per_rule[0]
            for w in range(P):
                d = case.get("deficit", {}).get(w, 0)
                if case["blocks"][w] == lc.C or lengths[w] >= 100:
                    assert npiv[w] == 64 - d, (case["id"], w, npiv[w])
                (short if npiv[w] < 64 else full).setdefault(lc.form_class(lengths[w]), set()).add(lengths[w])
        assert set(short) == set(full) == set(range(len(lc.FORM_CLASSES))), (mo, short, full)
        at = set().union(*short.values())
        assert {129, 257, 513, 1024, 1025, 2048, 2049} <= at, (mo, sorted(at))
        print(f"\n  {mo}: panels with fewer than 64 pivots, by form class: {[sorted(short[k]) for k in sorted(short)]}", end="")
    print()


def test_the_rank_is_complete_in_the_middle_of_a_panel():
    """Handed the true rank, as the kernel is, the elimination stops inside the last designed panel -- column 63 there is a sum
    of two others -- in the one-wave (CR 16), the sixteen-wave and the all-rows form, and never starts the tail's panel."""
    forms = set()
    for case in lc.PANEL_CASES:
        P = len(case["blocks"])
        if not case.get("deficit", {}).get(P - 1):
            continue
        Hs = _sorted_dense(case["id"])
        for mo in MODES:
            for ru in RULES:
                rank = _restated(case["id"])[(mo, ru)][2]
                lengths, _, nrank, npiv, last = lc.panel_list_lengths(Hs, rank, mo, ru)
                assert nrank == rank and len(lengths) == P and last[0] == P - 1 and last[1] < 63, (case["id"], mo, ru, last)
        forms.add(lc.form_class(lengths[-1]))
    assert forms == {3, 4, 5}, forms


def test_passbits_reach_the_sparse_and_the_table_pass():
    """The apply pass takes its sparse form up to OSDL_SPARSE_LIST mask bits.  The bits depend on the pivot-row rule, and the
    kernel's (fewest absorbed rows) is neither of the two restated here: a factor 2 either way is the margin."""
    lo, hi = lc.OSDL_SPARSE_LIST // 2, 2 * lc.OSDL_SPARSE_LIST
    assert (lo, hi) == (3072, 12288)
    for mo in MODES:
        both = []
        sparse = table = False
        for cid in PANEL_IDS:
            a, b = (lc.passbits(_restated(cid)[(mo, ru)][1]) for ru in RULES)
            assert len(a) == len(b)
            s = [i for i, (x, y) in enumerate(zip(a, b)) if 0 < x < lo and 0 < y < lo]
            t = [i for i, (x, y) in enumerate(zip(a, b)) if x > hi and y > hi]
            sparse, table = sparse or bool(s), table or bool(t)
            if s and t:
                both.append(cid)
            print(f"\n  {mo} {cid}: sparse passes {s}, table passes {t}", end="")
        assert sparse and table, mo
        assert both, f"{mo}: no matrix holds a sparse and a table pass in one elimination"
    print()


def _check_order(llr, perm, what):
    order = np.argsort(llr, kind="stable")
    assert (order == perm).all(), f"{what}: the posterior order is not the intended one"


@pytest.mark.parametrize("case_id", PANEL_IDS)
def test_oracle_confirms_the_chosen_order(case_id):
    case = lc.PANEL_BY_ID[case_id]
    H, perm = lc.panel_pcm(case_id)
    S, c = lc.syndromes(case_id)
    dc = np.diff(H.indptr)
    dv = np.bincount(H.indices, minlength=H.shape[1])
    assert dc.min() >= 2, "a degree-1 check: the reference's min over an empty set"
    assert dc.max() <= 16 and dv.min() >= 1 and dv.max() > 8  # bp_anydeg_kernel by the bit degree alone
    probs = lc.channel_for(perm)
    prior = np.log((1 - probs) / probs)
    assert (prior > 0).all()
    gap = np.diff(np.sort(prior)).min()
    assert gap > 4 * dv.max() * lc.ALPHA * np.abs(prior).max(), (gap, dv.max())
    assert (~S.any(axis=1)).sum() == 1 and not S[c - 1].any()
    rank = _restated(case_id)[("gauss", "lowest")][2]
    assert H.shape[1] - rank >= max(o for _, o in case["runs"])
    for method, order in case["runs"]:
        ref = lc.reference(case_id, method, order)
        S, c = lc.run_syndromes(case_id, method, order)
        zero = ~S.any(axis=1)
        assert int(ref["rank"]) == rank and len(ref["osdw"]) == len(S)
        assert (ref["converged"].astype(bool) == zero).all(), "every shot but the zero one goes to OSD"
        assert not ref["bp"].any(), "all priors are positive: BP's hard decision is all-zero"
        for b in np.flatnonzero(~zero):
            _check_order(ref["llr"][b], perm, f"{method} shot {b}")
            assert np.abs(ref["llr"][b] - prior).max() < gap / 4
        syn0 = (np.asarray(H.astype(np.int32) @ ref["osd0"][:c].T.astype(np.int32)) % 2).T
        assert (syn0 == S[:c]).all()
        if order:
            assert (ref["osdw"] != ref["osd0"]).any(), f"{method} {order}: the sweep had nothing to choose"
    if case["rows"]:
        P, Srows = lc.rows_inputs(case_id)
        ref = lc.rows_reference(case_id)
        _, perms = lc.shot_orders(case_id)
        for b in range(len(Srows)):
            assert Srows[b].any() and not ref["converged"][b]
            _check_order(ref["llr"][b], perms[b], f"rows shot {b}")
        assert (ref["osdw"] != ref["osd0"]).any()
    secs = lc.ORACLE_SECONDS[case_id]
    print(f"\n  {case_id}: oracle {secs:.1f} s")
    assert secs < 10.0


@pytest.mark.parametrize("case_id", [c["id"] for c in lc.LIMIT_CASES])
def test_limit_cases_are_what_they_claim(case_id):
    case = lc.LIMIT_BY_ID[case_id]
    H = lc.limit_pcm(case_id)
    m, n = H.shape
    assert (m, n) == (case["m"], case["n"]) and m <= 16384 and n <= 32767
    dc = np.diff(H.indptr)
    dv = np.bincount(H.indices, minlength=n)
    assert lc.limit_bp_instance(H) == ("bp_anydeg_kernel", ())
    if case["kind"] == "wide":
        assert (dc == 32).all() and dv.min() >= 1  # past osdl_build_rows' 12-edge batch; no empty column
    else:
        assert (dc == 4).all() and lc.rpt_of(m) == 16
    S = lc.limit_syndromes(case_id)
    assert len(S) == case["shots"] and S.any(axis=1).all()
    for method, order in case["runs"]:
        ref = lc.limit_reference(case_id, method, order)
        assert len(ref["osdw"]) == len(lc.limit_run_syndromes(case_id, method)) == (1 if method == "osd_cs" else len(S))
        assert not ref["converged"].any(), "the elimination does not run"
        assert 0 < int(ref["rank"]) <= min(m, n)
    secs = lc.ORACLE_SECONDS[case_id]
    print(f"\n  {case_id}: rank {int(ref['rank'])}, oracle {secs:.1f} s")
    assert secs < 10.0


def test_limit_table_sits_on_the_sort_sizes_and_the_last_shapes():
    def nsort(n):  # bposd_capi.hip: the power of two that holds n keys
        return 1 << int(np.ceil(np.log2(n)))

    wide = {c["n"]: c for c in lc.LIMIT_CASES if c["kind"] == "wide"}
    assert [nsort(n) for n in sorted(wide)] == [8192, 16384, 16384, 32768, 32768]
    assert max(wide) == 32767 and wide[32767]["packed"]
    assert [c["id"] for c in lc.LIMIT_CASES if ("osd_cs", 6) in c["runs"]] == ["wide_n16385"]
    assert all(c["shots"] == 2 and c["m"] == 1100 for c in wide.values())
    assert lc.PANEL_BY_ID["rpt16_m16384"].get("packed")
