"""The LSD definition on the CPU: ``lsd_decode_reference`` (bp_osd_amd/lsd.py) against a scalar restatement from sets and
ranks that shares no code with it, the properties the definition promises, and the conditions on tests/lsd_cases.py that
keep tests/test_gpu_lsd.py from passing empty."""
import numpy as np
import pytest

from bp_osd_amd import LsdConfig, LsdReferenceDecoder, lsd_decode_reference
from bp_osd_amd.codes import gf2_rank
from tests import lsd_cases as lc


def _restated(H, s, llr, max_bits=None, max_checks=None, tie=0):
    """The definition once more, from its text: clusters are (set of checks, set of bits), validity and the solution are
    statements about ranks.  Returns (row, status, rounds, clusters, max_bits, a valid cluster was swallowed)."""
    H = np.asarray(H, dtype=np.uint8)
    m, n = H.shape

    def before(a, b):
        return llr[a] < llr[b] or (llr[a] == llr[b] and (a > b if tie else a < b))

    def sub(checks, bits):
        return H[np.ix_(sorted(checks), list(bits))]

    def valid(cl):
        rows = sorted(cl[0])
        A = sub(cl[0], sorted(cl[1]))
        return gf2_rank(np.concatenate([A, s[rows][:, None]], axis=1)) == gf2_rank(A)

    clusters = [[{int(c)}, set()] for c in np.flatnonzero(s)]
    status = rounds = 0
    swallowed = False
    while True:
        invalid = [cl for cl in clusters if not valid(cl)]
        if not invalid:
            break
        free = set(range(n)) - set().union(*[cl[1] for cl in clusters])
        picks = set()
        for cl in invalid:
            cand = [j for j in free if any(H[c, j] for c in cl[0])]
            if not cand:
                status = 2
                break
            first = cand[0]
            for j in cand[1:]:
                if before(j, first):
                    first = j
            picks.add(first)
        if status:
            break
        rounds += 1
        was_valid = [cl for cl in clusters if cl not in invalid]
        groups = [[set(cl[0]), set(cl[1]), [cl]] for cl in clusters] + [[set(map(int, np.flatnonzero(H[:, j]))), {j}, []] for j in picks]
        merged = True
        while merged:  # groups that share a check are one cluster
            merged = False
            for a in range(len(groups)):
                for b in range(a + 1, len(groups)):
                    if groups[a][0] & groups[b][0]:
                        groups[a] = [groups[a][0] | groups[b][0], groups[a][1] | groups[b][1], groups[a][2] + groups[b][2]]
                        del groups[b]
                        merged = True
                        break
                if merged:
                    break
        swallowed |= any(len(g[2]) > 1 and any(cl in was_valid for cl in g[2]) for g in groups)
        clusters = [[g[0], g[1]] for g in groups]
        if any((max_bits is not None and len(cl[1]) > max_bits) or (max_checks is not None and len(cl[0]) > max_checks) for cl in clusters):
            status = 1
            break
    row = np.zeros(n, np.uint8)
    if status == 0:
        for checks, bits in clusters:
            order = []
            for j in sorted(bits):  # insertion by the order's own comparison
                k = 0
                while k < len(order) and before(order[k], j):
                    k += 1
                order.insert(k, j)
            basis = []
            for j in order:
                if gf2_rank(sub(checks, basis + [j])) > len(basis):
                    basis.append(j)
            rows = sorted(checks)
            for j in basis:  # x_j = 0 iff s is in the span of the other basis columns
                rest = [b for b in basis if b != j]
                A = sub(checks, rest)
                if gf2_rank(np.concatenate([A, s[rows][:, None]], axis=1)) > len(rest):
                    row[j] = 1
    return row, status, rounds, len(clusters), max([len(cl[1]) for cl in clusters], default=0), swallowed


SMALL = ("surface13", "hgp_rep5")


@pytest.mark.parametrize("tie", (0, 1))
@pytest.mark.parametrize("caps", ((None, None), (4, None), (None, 4)))
@pytest.mark.parametrize("case_id", SMALL)
def test_reference_against_the_restatement(case_id, caps, tie):
    case = lc.CASE_BY_ID[case_id]
    H = lc.matrix(case["code"]).toarray()
    u = lc.uncapped(case_id, tie)
    S = lc.syndromes(case_id)[u["open"]][:60]
    cfg = None if caps == (None, None) else LsdConfig(caps[0] or 256, caps[1] or 256)
    ref = lsd_decode_reference(H, S, u["llr"][:60], cfg, tie)
    for b in range(len(S)):
        row, status, rounds, ncl, maxb, _ = _restated(H, S[b], u["llr"][b], caps[0], caps[1], tie)
        assert (status, rounds, ncl, maxb) == tuple(int(ref[k][b]) for k in ("status", "rounds", "clusters", "max_bits")), b
        assert (row == ref["row"][b]).all(), b


@pytest.mark.parametrize("case", lc.CASES, ids=[c["id"] for c in lc.CASES])
def test_solved_shots_satisfy_the_syndrome(case):
    H, S = lc.matrix(case["code"]), lc.syndromes(case["id"])
    for run in lc.RUNS[:2]:
        ref = lc.reference(case["id"], run)
        ok = ref["status"] == 0
        assert ok.any() or case["id"] in lc.CHAIN_OVERFLOWS
        assert (((H.astype(np.int32) @ ref["osdw"][ok].T.astype(np.int32)) % 2).T == S[ok]).all()
        assert (ref["osdw"][ok] == ref["osd0"][ok]).all()
        conv = ref["status"] == -1
        assert (ref["osdw"][conv] == ref["bp"][conv]).all() and (ref["converged"][conv] == 1).all()


def test_one_cluster_over_the_whole_graph_is_osd0():
    """Growth that exhausts the graph: one cluster holds every check and bit, and its solution is the oracle's OSD-0."""
    from oracle import OracleDecoder

    H = np.array([[1, 1, 0, 0], [0, 1, 1, 0], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.uint8)  # a chain: only bit 0 solves s = e_0
    s = np.array([1, 0, 0, 0], dtype=np.uint8)
    for tie in (0, 1):
        llr = np.array([5.0, 1.0, 2.0, 2.0])  # ... and it comes last: bits 1, 2, 3 join first, each with the next check
        r = lsd_decode_reference(H, s, llr, None, tie)
        assert (r["status"][0], r["rounds"][0], r["clusters"][0], r["max_bits"][0], r["max_checks"][0]) == (0, 4, 1, 4, 4)
        o = OracleDecoder(H, error_rate=0.1, osd_method="osd0", sort_tie_policy=tie).osd(s, llr)
        assert (r["row"][0] == o["osd0"]).all() and r["row"][0].any()


def test_status_2_outside_the_column_space():
    H = np.array([[1, 1, 0], [1, 1, 0], [0, 0, 1]], dtype=np.uint8)  # rank 2: rows 0 and 1 are equal
    s = np.array([1, 0, 0], dtype=np.uint8)
    r = lsd_decode_reference(H, s, np.array([1.0, 2.0, 3.0]), LsdConfig())
    assert r["status"][0] == 2 and not r["row"].any()
    assert _restated(H, s, np.array([1.0, 2.0, 3.0]))[1] == 2
    d = lc.reference_decoder(H, lsd=LsdConfig(), error_rate=0.1, max_iter=2, bp_method="ms", osd_method="osd_off")
    out = d.decode_batch(s)
    assert out["status"][0] == 2 and (out["osdw"] == out["bp"]).all()  # osd_off: BP's decision


def test_initial_cluster_ids_do_not_matter():
    case = lc.CASE_BY_ID["hgp_rep5"]
    H, u = lc.matrix(case["code"]), lc.uncapped("hgp_rep5")
    S = lc.syndromes("hgp_rep5")[u["open"]]
    rng = np.random.default_rng(3)
    seen = 0
    for b in np.flatnonzero(u["clusters"] >= 2)[:25]:
        w = int(S[b].sum())
        for ids in (rng.permutation(w), 100 - rng.permutation(w)):
            r = lsd_decode_reference(H, S[b], u["llr"][b], None, cluster_ids=ids)
            assert all(r[k][0] == u[k][b] for k in ("status", "rounds", "clusters", "max_bits")) and (r["row"][0] == u["row"][b]).all()
            seen += 1
    assert seen >= 20


def test_the_table_is_not_trivial():
    """What the GPU tests rely on, over the whole table."""
    refs = {(c["id"], r): lc.reference(c["id"], r) for c in lc.CASES for r in lc.RUNS}
    generous = [v for (cid, r), v in refs.items() if r[:2] == (lc.LSD_MAX, lc.LSD_MAX)]
    assert any((v["status"] == -1).any() for v in generous), "no converged shot"
    assert any(((v["status"] == 0) & (v["clusters"] >= 3)).any() for v in generous), "no solved shot with three clusters"
    assert any((v["rounds"] >= 5).any() for v in generous), "no shot of five rounds"
    by_bits = [v for (cid, r), v in refs.items() if r[0] == 4]
    by_checks = [v for (cid, r), v in refs.items() if r[1] == 4]
    assert any((v["status"] == 1).any() and (v["status"] == 0).any() for v in by_bits), "no overflow by bits"
    assert any((v["status"] == 1).any() and (v["status"] == 0).any() for v in by_checks), "no overflow by checks"
    # an overflow under (4, 256) is one by bits and one under (256, 4) one by checks: the other cap is out of reach
    assert all(v["max_bits"].max() <= lc.LSD_MAX for v in by_checks)
    # OSD rows behind the clusters: some shot of status 1 gets a row that is not BP's
    assert any(((v["status"] == 1) & (v["osdw"] != v["bp"]).any(axis=1)).any() for (cid, r), v in refs.items() if r[2] == "osd_cs")


def test_ties_matter_under_both_policies():
    """Equal LLRs among the bits a cluster chooses from: the two tie policies select different bits somewhere."""
    case = lc.CASE_BY_ID["hgp_rep5"]
    a, b = lc.uncapped("hgp_rep5", 0), lc.uncapped("hgp_rep5", 1)
    assert (a["llr"].view(np.uint64) == b["llr"].view(np.uint64)).all()
    tied = [len(np.unique(l)) < len(l) for l in a["llr"]]
    assert any(tied)
    assert (a["row"] != b["row"]).any() and (a["status"] == 0).all() and (b["status"] == 0).all()
    assert case["p"] == 0.08  # (uniform priors: min-sum leaves exact ties)


def test_a_merge_swallows_a_valid_cluster():
    case = lc.CASE_BY_ID["hgp_rep5"]
    H, u = lc.matrix(case["code"]).toarray(), lc.uncapped("hgp_rep5")
    S = lc.syndromes("hgp_rep5")[u["open"]]
    hits = sum(_restated(H, S[b], u["llr"][b])[5] for b in np.flatnonzero(u["clusters"] + u["rounds"] >= 5)[:40])
    assert hits >= 1


def test_edge_runs_meet_their_caps():
    """Every EDGE_RUNS row: some cluster meets the cap exactly and its shot is solved, another holds one more when its shot
    ends with status 1.  On these sampled shots the largest solved cluster at the ceilings has 254 checks (and one of 257
    overflows); exactly 256 bits and 256 checks are the chains' part (test_chains_land_on_the_ceilings)."""
    for edge in lc.EDGE_RUNS:
        cid, bits, checks = edge
        case, base = lc.CASE_BY_ID[cid], lc.sizes_at_the_ceilings(cid)
        S = lc.syndromes(cid)[base["open"]]
        llr = lc.reference(cid, (lc.LSD_MAX, lc.LSD_MAX, "osd_off", 0, 0))["llr"][base["open"]]
        u = lsd_decode_reference(lc.matrix(case["code"]), S, llr, LsdConfig(bits, checks), 0)
        assert (u["status"] == lc.reference(cid, lc.edge_run(edge))["status"][base["open"]]).all()
        if bits < lc.LSD_MAX:
            at, past = u["max_bits"] == bits, u["max_bits"] == bits + 1
        elif checks < lc.LSD_MAX:
            at, past = u["max_checks"] == checks, u["max_checks"] == checks + 1
        else:
            at, past = u["max_checks"] == 254, u["max_checks"] == 257
        assert (at & (u["status"] == 0)).any(), (edge, "no cluster at the cap")
        assert (past & (u["status"] == 1)).any(), (edge, "no cluster one past the cap")


@pytest.mark.parametrize("tie", (0, 1))
def test_chains_land_on_the_ceilings(tie):
    """The deterministic cases: one cluster of exactly N bits and N checks at 128, 129, 192, 193 and 256 (status 0, the row
    satisfies the syndrome and is the oracle's OSD-0 wherever the cluster holds the whole chain), 257 checks with 256 bits
    and 257 bits on 157 checks (status 1)."""
    run = (lc.LSD_MAX, lc.LSD_MAX, "osd_off", 0, tie)
    for case in lc.CASES:
        if "chain" not in case:
            continue
        N, H, S, ref = case["chain"], lc.matrix(case["code"]), lc.syndromes(case["id"]), lc.reference(case["id"], run)
        u = lsd_decode_reference(H, S[:1], ref["llr"][:1], LsdConfig(), tie)
        copies = case.get("copies", 0)
        want_status = 1 if case["id"] in lc.CHAIN_OVERFLOWS else 0
        assert ref["converged"][0] == 0 and ref["status"][0] == u["status"][0] == want_status, case["id"]
        assert (u["clusters"][0], u["max_checks"][0]) == (1, N), case["id"]
        assert u["max_bits"][0] == (N - 1 if case["id"] == "chain_257" else N + copies), case["id"]
        if want_status == 0:
            assert (((H.astype(np.int32) @ ref["osdw"][:1].T.astype(np.int32)) % 2).T == S[:1]).all()
            assert ref["osdw"][0].sum() == N  # bits 1 .. N - 1 and one spare bit: the only solution without bit 0


def test_config_and_window_refusals():
    for bad in (dict(max_cluster_bits=0), dict(max_cluster_bits=257), dict(max_cluster_checks=0), dict(max_cluster_checks=257),
                dict(max_cluster_bits=2.5), dict(max_cluster_bits=True)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            LsdConfig(**bad)
    assert LsdConfig() == LsdConfig(256, 256) and LsdConfig(3, 4) != LsdConfig(4, 3)
    with pytest.raises(ValueError, match="LsdConfig"):
        LsdReferenceDecoder(np.eye(3, dtype=np.uint8), lsd=(4, 4), error_rate=0.1)
    from bp_osd_amd import WindowedDemDecoder, windowed_dem_decode_sim
    from bp_osd_amd.codes import surface13
    from bp_osd_amd.dem import phenomenological_dem, phenomenological_detector_times

    cd = surface13()
    H, L, priors = phenomenological_dem(cd.hz, cd.lz, 4, 0.02, 0.02)
    times = phenomenological_detector_times(cd.hz.shape[0], 4)
    for cls, kw in ((windowed_dem_decode_sim, dict(run_sim=False, engine="numpy")), (WindowedDemDecoder, {})):
        with pytest.raises(ValueError, match="no lsd= argument"):
            cls(H, L, priors, times, (2, 1), lsd=LsdConfig(), **kw)


def test_c_abi_is_declared():
    import os

    from bp_osd_amd import _lib

    lib = _lib.load()
    public = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "bposd_mi355x.h")).read()
    for name in ("bposd_set_lsd", "bposd_lsd_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in public, name
