"""The higher LSD orders on the CPU: ``lsd_decode_reference`` against an independent restatement from sets and ranks that
solves every candidate by an elimination of its own, a cluster over the whole graph against the oracle's osd_cs / osd_e
rows, H x = s, the defaults against LSD-0, the refusals of ``LsdConfig``, and the coverage conditions that keep the device
table of tests/test_gpu_lsd_order.py from being trivial."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests import lsd_cases as lc
from tests import lsd_order_cases as oc


# ---------------------------------------------------------------- the restatement
def _xor_basis_insert(basis, v, tag):
    """``basis``: list of (vector, combination) with distinct leading bits.  Reduce v; independent: insert, return None;
    dependent: return the combination of earlier columns that equals v."""
    comb = tag
    for bv, bc in basis:
        if v ^ bv < v:
            v ^= bv
            comb ^= bc
    if v:
        basis.append((v, comb))
        basis.sort(key=lambda e: -e[0])
        return None
    return comb


def _express(basis, v):
    """(in span?, combination of the inserted columns that equals v)."""
    comb = 0
    for bv, bc in basis:
        if v ^ bv < v:
            v ^= bv
            comb ^= bc
    return v == 0, comb


def _restate_shot(H, s, rank, opt, cost, ebo, max_bits=None, max_checks=None):
    method, order, min_free, grow_limit = opt
    m, n = H.shape
    Hc, Hr = sp.csc_matrix(H), sp.csr_matrix(H)
    checks_of = [set(Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]].tolist()) for j in range(n)]
    bits_of = [set(Hr.indices[Hr.indptr[c]:Hr.indptr[c + 1]].tolist()) for c in range(m)]
    colvec = [sum(1 << c for c in checks_of[j]) for j in range(n)]
    clusters = [({int(c)}, set()) for c in np.flatnonzero(s)]
    taken = set()
    status, rounds = 0, 0

    def analyse(C, V):
        """(valid, greedy basis columns in bit order, free columns in bit order, xor basis)"""
        cols = sorted(V, key=lambda j: rank[j])
        basis, inb, free = [], [], []
        for q, j in enumerate(cols):
            if _xor_basis_insert(basis, colvec[j], 1 << q) is None:
                inb.append(j)
            else:
                free.append(j)
        target = sum(1 << c for c in C if s[c])
        return _express(basis, target)[0], cols, free, basis

    while True:
        picks = []
        for C, V in clusters:
            valid, _, free, _ = analyse(C, V)
            if valid and not (len(free) < min_free and len(V) < grow_limit):
                continue
            cand = set().union(*(bits_of[c] for c in C)) - taken
            if not cand:
                if not valid:
                    status = 2
                continue
            picks.append((C, V, min(cand, key=lambda j: rank[j])))
        if status == 2 or not picks:
            break
        rounds += 1
        for C, V, j in picks:
            taken.add(j)
            V.add(j)
            C |= checks_of[j]
        merged = []
        for C, V in clusters:  # clusters that share a check are one
            C, V = set(C), set(V)
            while True:
                hit = [k for k, (C2, _) in enumerate(merged) if C & C2]
                if not hit:
                    break
                for k in sorted(hit, reverse=True):
                    C |= merged[k][0]
                    V |= merged[k][1]
                    del merged[k]
            merged.append((C, V))
        clusters = merged
        if any((max_bits is not None and len(V) > max_bits) or (max_checks is not None and len(C) > max_checks) for C, V in clusters):
            status = 1
            break
    row0, row, max_free = np.zeros(n, np.uint8), np.zeros(n, np.uint8), 0
    if status == 0:
        for C, V in clusters:
            valid, cols, free, basis = analyse(C, V)
            assert valid
            kp = len(free)
            max_free = max(max_free, kp)
            w = min(order, kp)
            if method == "lsd_0":
                cands = []
            elif method == "lsd_cs":
                cands = [(t,) for t in range(kp)] + [(a, b) for a in range(w) for b in range(a + 1, w)]
            else:
                cands = [tuple((w - 1 - b) if ebo else b for b in range(w) if (pat >> b) & 1) for pat in range(1, 1 << w)]
            basis_cols = [j for j in cols if j not in free]
            target = sum(1 << c for c in C if s[c])

            def solve(T):  # an elimination of its own over the basis columns, the columns of T moved to the right-hand side
                b2, t = [], target
                for k, j in enumerate(basis_cols):
                    assert _xor_basis_insert(b2, colvec[j], 1 << k) is None
                for tt in T:
                    t ^= colvec[free[tt]]
                ok, comb = _express(b2, t)
                assert ok
                x = {j: (comb >> k) & 1 for k, j in enumerate(basis_cols)}
                x.update({j: 0 for j in free})
                x.update({free[tt]: 1 for tt in T})
                return x

            def weight(x):
                if cost is None:
                    return sum(x.values())
                wsum = 0.0
                for j in sorted(x):
                    if x[j]:
                        wsum += cost[j]
                return wsum

            x0 = solve(())
            best, bw = x0, weight(x0)
            for T in cands:
                x = solve(T)
                cw = weight(x)
                if cw < bw:
                    best, bw = x, cw
            for j in cols:
                row0[j], row[j] = x0[j], best[j]
    return dict(row=row, row0=row0, status=status, rounds=rounds, clusters=len(clusters),
                max_bits=max((len(V) for _, V in clusters), default=0), max_free=max_free, improved=int((row != row0).any()))


def _channel_cost(n, seed):
    """A non-uniform channel's log(1/p): fp64 weights."""
    p = np.random.default_rng(seed).uniform(0.01, 0.3, n)
    return np.array([math.log(1 / float(v)) for v in p])


@pytest.mark.parametrize("min_free", [0, 4, 8])
@pytest.mark.parametrize("method,order", [("lsd_cs", 4), ("lsd_e", 3)])
@pytest.mark.parametrize("tie", [0, 1])
@pytest.mark.parametrize("case_id", ["surface13", "hgp_rep5"])
def test_reference_against_restatement(case_id, tie, method, order, min_free):
    from bp_osd_amd import lsd_decode_reference
    from bp_osd_amd.lsd import lsd_bit_rank

    H = oc.matrix(case_id)
    _, S, llr = oc.open_shots(case_id, tie)
    S, llr = S[:40], llr[:40]
    order_kw = oc.order_kw(method, order, min_free, 20)
    cfg = oc.config_of(order_kw)
    for cost in (None, _channel_cost(H.shape[1], 3)):
        ref = lsd_decode_reference(H, S, llr, cfg, tie, cost=cost, e_bit_order=tie)
        for b in range(len(S)):
            want = _restate_shot(H, S[b], lsd_bit_rank(llr[b], tie), cfg._order_fields(), cost, tie, 256, 256)
            for k, v in want.items():
                assert (np.asarray(ref[k][b]) == v).all(), (b, k)
    if min_free == 8:
        assert ref["max_free"].max() >= 4 and ref["improved"].any()


@pytest.mark.parametrize("ebo", [0, 1])
@pytest.mark.parametrize("method,order", [("cs", 5), ("e", 4)])
def test_whole_graph_cluster_equals_the_oracle(method, order, ebo):
    """Grown for more free bits than there are, the clusters of a connected graph end as one cluster with every bit: the rows
    are the oracle's OSD rows, under a uniform, a two-valued and a general channel."""
    from bp_osd_amd import lsd_decode_reference
    from oracle import OracleDecoder

    case = lc.CASE_BY_ID["hgp_rep5"]
    H, S = oc.matrix("hgp_rep5"), oc.syndromes("hgp_rep5")
    n = H.shape[1]
    rng = np.random.default_rng(11)
    cfg = oc.config_of(oc.order_kw("lsd_" + method, order, 64, 256))
    for probs in (None, np.where(rng.random(n) < 0.5, 0.02, 0.2), rng.uniform(0.01, 0.3, n)):
        kw = dict(lc.settings(case, (0, 0, "osd_" + method, order, ebo)), osd_e_bit_order=ebo)
        cost = None
        if probs is not None:
            del kw["error_rate"]
            kw["channel_probs"] = probs
            cost = np.array([math.log(1 / float(p)) for p in probs])
        r = OracleDecoder(H, **kw).decode_batch(S)
        open_ = np.flatnonzero(r["converged"] == 0)
        assert open_.size > 50
        ref = lsd_decode_reference(H, S[open_], r["llr"][open_], cfg, ebo, cost=cost, e_bit_order=ebo)
        assert (ref["status"] == 0).all() and (ref["clusters"] == 1).all() and (ref["max_bits"] == n).all()
        assert (ref["row0"] == r["osd0"][open_]).all()
        assert (ref["row"] == r["osdw"][open_]).all()
        assert ref["improved"].any()


@pytest.mark.parametrize("row", range(len(oc.TABLE)), ids=[oc.row_id(r) for r in oc.TABLE])
def test_coverage_and_parity_checks(row):
    """H x = s for both rows of every solved shot, and what the row of the table is there for."""
    case_id, order = oc.TABLE[row]
    exp = oc.EXPECT.get(row, {})
    H = oc.matrix(case_id)
    Hd = np.asarray(H.todense()).astype(np.int64)
    for tie in (0, 1):
        _, S, _ = oc.open_shots(case_id, tie)
        ref = oc.uncapped(case_id, order, tie)
        ok = ref["status"] == 0
        for k in ("row", "row0"):
            assert ((ref[k][ok].astype(np.int64) @ Hd.T) % 2 == S[ok]).all(), k
        assert (ref["improved"] == (ref["row"] != ref["row0"]).any(axis=1)).all()
        assert not ref["improved"][~ok].any() and not ref["max_free"][~ok].any()
        exact = tie == 0 or exp.get("exact", False)
        if "open" in exp and tie == 0:
            assert len(S) == exp["open"]
        if "improved" in exp and (tie == 0 or not exp.get("tie0_only")):
            got = int(ref["improved"].sum())
            assert got == exp["improved"] if exact else (got >= 1) == (exp["improved"] >= 1), (tie, got)
        if "max_free" in exp:
            assert ref["max_free"].max() == exp["max_free"] if exact else ref["max_free"].max() >= min(exp["max_free"], 4), tie
        if "max_free_at_most" in exp:
            assert ref["max_free"].max() <= exp["max_free_at_most"]
        if "max_bits" in exp:
            assert ref["max_bits"].max() == exp["max_bits"]
        if "status" in exp:
            assert (ref["status"] == exp["status"]).all()
        if "status1" in exp:
            got = int((ref["status"] == 1).sum())
            assert got == exp["status1"] if exact else got >= 3, (tie, got)
        if "w0" in exp:
            assert int(ref["row0"][0].sum()) == exp["w0"] and int(ref["row"][0].sum()) == exp["ww"]
        if "four_words" in exp and tie == 0:  # the shot that differs holds a cluster of four words per row (more than 192 bits)
            assert ref["max_bits"][ref["improved"] == 1].max() > 192 and ref["max_bits"].max() == 252


def test_candidates_of_the_chain_with_copies():
    """chaindup_156: 100 free columns, 100 + 21 candidates -- a second round of lanes."""
    ref = oc.uncapped("chaindup_156", oc.order_kw("lsd_cs", 7, 0))
    kp, w = int(ref["max_free"][0]), 7
    assert kp == 100 and kp + w * (w - 1) // 2 == 121


def test_defaults_are_lsd0():
    from bp_osd_amd import LsdConfig, lsd_decode_reference

    for case_id in ("hgp_rep5", "dense_dc20_dv9"):
        for tie in (0, 1):
            U = lc.uncapped(case_id, tie)
            _, S, llr = oc.open_shots(case_id, tie)
            ref = lsd_decode_reference(oc.matrix(case_id), S, llr, LsdConfig(), tie)
            assert (ref["row"] == U["row"]).all() and (ref["row0"] == U["row"]).all()
            assert not ref["improved"].any()
            for k in ("status", "rounds", "clusters", "max_bits"):
                assert (ref[k] == U[k]).all(), k
    assert repr(LsdConfig(7, 9)) == "LsdConfig(max_cluster_bits=7, max_cluster_checks=9)"
    assert "lsd_cs" in repr(LsdConfig(method="lsd_cs", order=3))
    assert LsdConfig() == LsdConfig(method="lsd_0", order=0, min_free_bits=0, grow_bits_limit=256)
    assert LsdConfig() != LsdConfig(min_free_bits=1) and LsdConfig() != LsdConfig(grow_bits_limit=255)
    assert LsdConfig(method="lsd_cs", order=2) != LsdConfig(method="lsd_e", order=2)
    assert LsdConfig(method="lsd_cs", order=2) != LsdConfig(method="lsd_cs", order=3)


@pytest.mark.parametrize("kw,field", [
    (dict(method="lsd_x"), "method"), (dict(method="lsd_0", order=1), "order"), (dict(method="lsd_cs", order=0), "order"),
    (dict(method="lsd_cs", order=65), "order"), (dict(method="lsd_e", order=11), "order"), (dict(method="lsd_e", order=2.5), "order"),
    (dict(min_free_bits=-1), "min_free_bits"), (dict(min_free_bits=65), "min_free_bits"), (dict(min_free_bits=True), "min_free_bits"),
    (dict(grow_bits_limit=0), "grow_bits_limit"), (dict(grow_bits_limit=257), "grow_bits_limit"),
])
def test_refusals(kw, field):
    from bp_osd_amd import LsdConfig

    with pytest.raises(ValueError, match=field):
        LsdConfig(**kw)
    with pytest.raises(TypeError):
        LsdConfig(256, 256, "lsd_cs")  # the new settings are keyword arguments


def test_fp64_cases_differ_from_hamming():
    """On some shot of each fp64 case the sweep chooses another row than Hamming weights would."""
    from bp_osd_amd import lsd_decode_reference

    for which, c in (("two_valued", oc.TWO_VALUED), ("rows", oc.ROWS)):
        want, P = oc.per_shot_reference(which)
        op = np.flatnonzero(want["status"] == 0)
        H, S = oc.matrix(c["case"]), oc.syndromes(c["case"])
        cost = np.array([[math.log(1 / float(p)) for p in r] for r in P[op]])
        a = lsd_decode_reference(H, S[op], want["llr"][op], oc.config_of(c["order"]), 0, cost=cost)
        b = lsd_decode_reference(H, S[op], want["llr"][op], oc.config_of(c["order"]), 0, cost=None)
        assert (a["row"] == want["osdw"][op]).all() and (a["row0"] == want["osd0"][op]).all()
        assert (a["row"] != b["row"]).any(), which
        assert (want["improved"][op] == a["improved"]).all()


def test_c_abi_is_declared():
    import os

    from bp_osd_amd import _lib

    lib = _lib.load()
    inc = os.path.join(os.path.dirname(_lib.__file__), "..", "include")
    public, debug = open(os.path.join(inc, "bposd_mi355x.h")).read(), open(os.path.join(inc, "bposd_mi355x_debug.h")).read()
    for name, header in (("bposd_set_lsd_order", public), ("bposd_lsd_order_stats", public), ("bposd_debug_lsd_launches", debug)):
        assert name in _lib.EXPORTED_SYMBOLS + _lib.DEBUG_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header, name
    assert "not offered" not in public
