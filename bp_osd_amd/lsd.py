"""BP+LSD: localized statistics decoding of order 0 (Hillmann et al., 2024, "Localized statistics decoding: a parallel
decoding algorithm for quantum low-density parity-check codes"), as a mode of :class:`bp_osd_amd.BpOsdDecoder`.

``BpOsdDecoder(..., lsd=LsdConfig())`` (or ``set_lsd``) puts ``lsd_kernel`` between the BP stage and the OSD stage of every
decode call of that decoder: it consumes the list of shots BP left open, solves each from clusters grown around the
unsatisfied checks, and hands only the shots it does not finish on to the OSD kernels.  DESIGN.md §4.19 and the comment at
``bposd_set_lsd`` in include/bposd_mi355x.h hold the definition.  This module holds the configuration object and the
definition restated in numpy (:func:`lsd_decode_reference`), which is what the device results are compared with bit for bit.

The definition is synchronous: every invalid cluster selects one bit per round and all selected bits join at once, so the
result depends neither on the order clusters are visited in nor on how a cluster is eliminated.  It is not upstream
``ldpc.BpLsdDecoder``'s growth order, and no bit-for-bit parity with it is claimed.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

__all__ = ["LsdConfig", "lsd_bit_rank", "lsd_decode_reference", "LsdReferenceDecoder", "LSD_MAX_CLUSTER_BITS", "LSD_MAX_CLUSTER_CHECKS"]

# What one elimination of lsd_kernel holds (csrc/lsd_kernel.hip.h: LSD_RPL rows per lane of a 64-lane wave, LSD_WPR 64-bit
# words per row).  The defaults are the ceilings: see DESIGN.md §4.19.
LSD_MAX_CLUSTER_BITS = 256
LSD_MAX_CLUSTER_CHECKS = 256


LSD_METHODS = ("lsd_0", "lsd_cs", "lsd_e")
LSD_MAX_ORDER = {"lsd_0": 0, "lsd_cs": 64, "lsd_e": 10}
LSD_MAX_MIN_FREE_BITS = 64


class LsdConfig:
    """The LSD mode of a decoder: a cluster that holds more than ``max_cluster_bits`` bits or ``max_cluster_checks`` checks
    after a round ends the shot with status 1 (it goes on to the OSD stage).  Both are integers in [1, 256]; the defaults are
    the ceilings of the kernel.

    ``method`` ``"lsd_cs"`` / ``"lsd_e"`` with ``order`` in [1, 64] / [1, 10] sweeps the candidates of the OSD stage's
    combination sweep / exhaustive search inside every final cluster (``"lsd_0"`` with order 0: none).  ``min_free_bits`` in
    [0, 64] keeps a valid cluster growing, one bit a round, until it holds that many free columns or ``grow_bits_limit``
    (in [1, 256]) bits.  ValueError names what is wrong."""

    def __init__(self, max_cluster_bits=LSD_MAX_CLUSTER_BITS, max_cluster_checks=LSD_MAX_CLUSTER_CHECKS, *, method="lsd_0", order=0,
                 min_free_bits=0, grow_bits_limit=LSD_MAX_CLUSTER_BITS):
        if method not in LSD_METHODS:
            raise ValueError(f"method = {method!r} must be one of {LSD_METHODS}")
        lo = 0 if method == "lsd_0" else 1
        for name, v, low, top, what in (("max_cluster_bits", max_cluster_bits, 1, LSD_MAX_CLUSTER_BITS, "the ceiling of lsd_kernel"),
                                        ("max_cluster_checks", max_cluster_checks, 1, LSD_MAX_CLUSTER_CHECKS, "the ceiling of lsd_kernel"),
                                        ("order", order, lo, LSD_MAX_ORDER[method], f"method {method}"),
                                        ("min_free_bits", min_free_bits, 0, LSD_MAX_MIN_FREE_BITS, "the free columns a sweep can use"),
                                        ("grow_bits_limit", grow_bits_limit, 1, LSD_MAX_CLUSTER_BITS, "the ceiling of lsd_kernel")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer, float)) or int(v) != v or not low <= int(v) <= top:
                raise ValueError(f"{name} = {v} must be an integer in [{low}, {top}] ({what})")
        self.max_cluster_bits = int(max_cluster_bits)
        self.max_cluster_checks = int(max_cluster_checks)
        self.method = method
        self.order = int(order)
        self.min_free_bits = int(min_free_bits)
        self.grow_bits_limit = int(grow_bits_limit)

    def _order_fields(self):
        return (self.method, self.order, self.min_free_bits, self.grow_bits_limit)

    @property
    def higher_order(self):
        """Does the configuration need the second kernel instance (a sweep, or growth for free bits)?"""
        return self.method != "lsd_0" or self.min_free_bits > 0

    def __repr__(self):
        base = f"max_cluster_bits={self.max_cluster_bits}, max_cluster_checks={self.max_cluster_checks}"
        if self._order_fields() != ("lsd_0", 0, 0, LSD_MAX_CLUSTER_BITS):
            base += (f", method={self.method!r}, order={self.order}, min_free_bits={self.min_free_bits}, "
                     f"grow_bits_limit={self.grow_bits_limit}")
        return f"LsdConfig({base})"

    def __eq__(self, other):
        return (isinstance(other, LsdConfig) and self.max_cluster_bits == other.max_cluster_bits
                and self.max_cluster_checks == other.max_cluster_checks and self._order_fields() == other._order_fields())

    __hash__ = None


def lsd_bit_rank(llr, tie_policy=0):
    """rank[j] = position of bit j in the order the OSD stage sorts columns by: ascending LLR, ties by ascending index
    (``tie_policy`` 0) or descending index (1).  Bit a comes before bit b iff rank[a] < rank[b]."""
    llr = np.asarray(llr, dtype=np.float64)
    n = llr.shape[0]
    start = np.arange(n)[::-1] if tie_policy == 1 else np.arange(n)
    order = start[np.argsort(llr[start], kind="stable")]
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    return rank


def _reduce_in_order(A, s):
    """A uint8 [r, c] with its columns already in bit order, s uint8 [r]: (valid, A', s', piv_row) after Gauss-Jordan over the
    columns in order -- a column is a basis column iff it is independent of the columns before it, piv_row[j] is its pivot
    row (-1: a free column)."""
    A = A.copy()
    s = s.copy()
    r, c = A.shape
    used = np.zeros(r, bool)
    piv_row = np.full(c, -1)
    for j in range(c):
        rows = np.flatnonzero(A[:, j].astype(bool) & ~used)
        if rows.size == 0:
            continue
        p = rows[0]
        used[p] = True
        piv_row[j] = p
        others = np.flatnonzero(A[:, j])
        others = others[others != p]
        A[others] ^= A[p]
        s[others] ^= s[p]
    return not s[~used].any(), A, s, piv_row


def _solve_in_order(A, s):
    """(valid, x) with x the solution of A x = s supported on the greedy column basis."""
    ok, _, s, piv_row = _reduce_in_order(A, s)
    if not ok:
        return False, None
    x = np.zeros(A.shape[1], np.uint8)
    has = piv_row >= 0
    x[has] = s[piv_row[has]]
    return True, x


def _weight(x, cols_by_index, cost):
    """The OSD stage's weight of x (over the cluster's columns, ``cols_by_index`` = their positions by ascending bit index):
    the number of set bits, or the fp64 sum of ``cost`` over them in ascending bit index, started at 0.0."""
    if cost is None:
        return int(x.sum())
    w = 0.0
    for q in cols_by_index:
        if x[q]:
            w += cost[q]
    return w


def _sweep(A, s, piv_row, cols, cost, method, order, e_bit_order):
    """The candidates of ``method`` / ``order`` over the reduced system of a final cluster (columns ``cols`` in bit order):
    (x0, the lightest candidate, free columns)."""
    c = A.shape[1]
    basis = np.flatnonzero(piv_row >= 0)
    free = np.flatnonzero(piv_row < 0)
    kp = free.size
    w = min(order, kp)
    x0 = np.zeros(c, np.uint8)
    x0[basis] = s[piv_row[basis]]
    if method == "lsd_0" or kp == 0:
        return x0, x0, kp
    flips = np.zeros((kp, c), np.uint8)  # what setting free column t does to the solution
    flips[:, basis] = A[piv_row[basis]][:, free].T
    flips[np.arange(kp), free] = 1
    if method == "lsd_cs":
        cands = [(t,) for t in range(kp)] + [(a, b) for a in range(w) for b in range(a + 1, w)]
    else:
        cands = [tuple((w - 1 - b) if e_bit_order else b for b in range(w) if (pat >> b) & 1) for pat in range(1, 1 << w)]
    by_index = np.argsort(np.asarray(cols))
    cc = None if cost is None else np.asarray(cost, np.float64)[np.asarray(cols)]
    best, bw = x0, _weight(x0, by_index, cc)
    for T in cands:
        x = x0.copy()
        for t in T:
            x ^= flips[t]
        cw = _weight(x, by_index, cc)
        if cw < bw:  # strictly lighter: the first found wins ties
            best, bw = x, cw
    return x0, best, kp


def _lsd_one(rp, ci, cp, cr, s, rank, max_bits, max_checks, ids, opt=("lsd_0", 0, 0, LSD_MAX_CLUSTER_BITS), cost=None, e_bit_order=0):
    method, order, min_free, grow_limit = opt
    m, n = len(rp) - 1, len(cp) - 1
    seeds = np.flatnonzero(s)
    if ids is None:
        ids = np.arange(seeds.size)
    owner = np.full(m, -1, np.int64)  # cluster id per check
    taken = np.zeros(n, bool)
    # id -> [set of checks, set of bits, valid, reduced system (A, s, piv_row, cols) of a valid one, free columns, finished]
    clusters = {}
    for c, k in zip(seeds, ids):
        clusters[int(k)] = [{int(c)}, set(), False, None, 0, False]
        owner[c] = int(k)
    rounds, status = 0, 0
    while True:
        picks = {}
        for k in sorted(clusters):
            cl = clusters[k]
            if cl[2] and (cl[4] >= min_free or len(cl[1]) >= grow_limit or cl[5]):
                continue  # finished
            best = -1
            for c in cl[0]:
                for j in ci[rp[c]:rp[c + 1]]:
                    if not taken[j] and (best < 0 or rank[j] < rank[best]):
                        best = int(j)
            if best < 0:
                if cl[2]:
                    cl[5] = True  # a valid cluster with nothing to select is finished until a merge changes it
                else:
                    status = 2
                continue
            picks[k] = best
        if status == 2 or not picks:
            break
        rounds += 1
        # all selected bits join at once; clusters connected through a joined bit merge (union-find over cluster ids)
        parent = {k: k for k in clusters}

        def find(k):
            while parent[k] != k:
                parent[k] = parent[parent[k]]
                k = parent[k]
            return k

        for k, j in picks.items():
            taken[j] = True
            for c in cr[cp[j]:cp[j + 1]]:
                if owner[c] < 0:  # a check no cluster holds yet comes with the bit (two joining bits may share it)
                    owner[c] = k
                else:
                    a, b = find(k), find(int(owner[c]))
                    if a != b:
                        parent[max(a, b)] = min(a, b)
        changed = set()
        for k, j in picks.items():
            root = find(k)
            changed.add(root)
            clusters[root][1].add(j)
        for k in list(clusters):
            root = find(k)
            if root != k:
                clusters[root][1] |= clusters[k][1]
                del clusters[k]
        for c in np.flatnonzero(owner >= 0):
            owner[c] = find(int(owner[c]))
            clusters[int(owner[c])][0].add(int(c))
        for k in changed:
            cl = clusters[k]
            checks, bits = cl[0], cl[1]
            cl[5] = False
            if (max_bits is not None and len(bits) > max_bits) or (max_checks is not None and len(checks) > max_checks):
                status = 1
                continue
            rows = sorted(checks)
            cols = sorted(bits, key=lambda j: rank[j])
            pos = {c: i for i, c in enumerate(rows)}
            A = np.zeros((len(rows), len(cols)), np.uint8)
            for q, j in enumerate(cols):
                for c in cr[cp[j]:cp[j + 1]]:
                    A[pos[int(c)], q] = 1
            ok, Ar, sr, piv_row = _reduce_in_order(A, s[rows])
            cl[2] = ok
            cl[3] = (Ar, sr, piv_row, cols) if ok else None
            cl[4] = int((piv_row < 0).sum())
        if status == 1:
            break
    row0 = np.zeros(n, np.uint8)
    row = np.zeros(n, np.uint8)
    max_free = 0
    if status == 0:
        for cl in clusters.values():
            Ar, sr, piv_row, cols = cl[3]
            x0, xw, kp = _sweep(Ar, sr, piv_row, cols, cost, method, order, e_bit_order)
            max_free = max(max_free, kp)
            row0[cols] = x0
            row[cols] = xw
    return (row, status, rounds, len(clusters), max((len(cl[1]) for cl in clusters.values()), default=0),
            max((len(cl[0]) for cl in clusters.values()), default=0), row0, max_free, int((row != row0).any()))


def lsd_decode_reference(H, syndrome, llr, cfg, tie_policy=0, cluster_ids=None, cost=None, e_bit_order=0):
    """LSD of ``syndrome`` (uint8 [m] or [B, m]) with the soft output ``llr`` (float64 [n] or [B, n]) on the check matrix
    ``H``: dict(row, row0 uint8 [B, n], status, rounds, clusters, max_bits, max_free, improved int32 [B]).

    Bit a comes before bit b iff it does in the OSD stage's column order (:func:`lsd_bit_rank`).  Every unsatisfied check
    starts as a cluster of its own without bits.  A cluster is valid iff the syndrome on its checks is in the column span of
    H[checks, bits].  In a round every cluster that is invalid at its start selects the first bit in bit order among the
    bits that are adjacent to one of its checks and in no cluster; all selected bits join at once, each with all its checks,
    clusters connected through a joined bit merge, and the validity of every cluster that grew or merged is evaluated
    afresh.  Rounds repeat until every cluster is valid; per cluster the row holds the solution of H[checks, bits] x =
    s[checks] supported on the greedy column basis with the bits in bit order (OSD-0 restricted to the cluster).

    status 0: solved.  1: after some round a cluster holds more than ``cfg.max_cluster_bits`` bits or
    ``cfg.max_cluster_checks`` checks.  2: at the start of a round an invalid cluster has no bit to select.  Statuses 1 and
    2 leave an all-zero row.  ``rounds`` counts the rounds in which bits joined, ``clusters`` and ``max_bits`` are the number
    of clusters and the most bits in one of them when the shot ended (``max_checks``, the most checks, is not among the
    words the device keeps).  ``cfg`` None: no caps.  ``cluster_ids``: distinct
    integers, the initial id of the cluster of every unsatisfied check in ascending check order (one shot only) -- the
    result does not depend on them.

    Higher orders (``cfg.method``, ``cfg.order``, ``cfg.min_free_bits``, ``cfg.grow_bits_limit``; ``cfg`` None: LSD-0, no
    growth).  free = bits - rank of a cluster; its free columns are the columns, in bit order, outside the greedy column
    basis.  A cluster is unfinished at the start of a round if it is invalid, or valid with free < min_free_bits and fewer
    than grow_bits_limit bits; every unfinished cluster selects as above, a valid one with nothing to select is finished until
    a merge changes it, and rounds repeat while some cluster selects.  ``row0`` holds, per final cluster, the solution on the
    greedy column basis (LSD-0 on the possibly larger clusters); ``row`` the lightest candidate of the sweep over the
    cluster's reduced system: with kp free columns and w = min(order, kp), ``lsd_cs`` tries the kp single free columns in
    column order and then the pairs a < b < w (a outer), ``lsd_e`` the patterns 1 .. 2^w - 1 (bit b of a pattern is free
    column b, or w - 1 - b with ``e_bit_order`` 1); a candidate sets its free columns, clears the others and solves the basis
    bits.  Its weight is the number of set bits (``cost`` None) or the fp64 sum, from 0.0, of ``cost`` (float64 [n] or
    [B, n]: log(1/p)) over its set bits in ascending bit index; a strictly lighter candidate replaces the best, so the first
    found wins ties (the OSD stage's sweep, inside a cluster).  ``max_free`` is the most free columns in one final
    cluster, ``improved`` 1 iff ``row`` differs from ``row0``; both are 0 unless status is 0."""
    Hc = sp.csr_matrix(H)
    Hc.sort_indices()
    m, n = Hc.shape
    Ht = sp.csc_matrix(Hc)
    Ht.sort_indices()
    rp, ci, cp, cr = Hc.indptr, Hc.indices, Ht.indptr, Ht.indices
    S = np.atleast_2d(np.asarray(syndrome, dtype=np.uint8) & 1)
    L = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    if S.shape[1] != m or L.shape[1] != n or L.shape[0] not in (1, S.shape[0]):
        raise ValueError(f"syndromes {S.shape} and LLRs {L.shape} do not fit a {m} x {n} matrix")
    if cluster_ids is not None and S.shape[0] != 1:
        raise ValueError("cluster_ids belongs to a single shot")
    B = S.shape[0]
    mb = None if cfg is None else cfg.max_cluster_bits
    mc = None if cfg is None else cfg.max_cluster_checks
    out = {"row": np.zeros((B, n), np.uint8), "row0": np.zeros((B, n), np.uint8)}
    for k in ("status", "rounds", "clusters", "max_bits", "max_checks", "max_free", "improved"):
        out[k] = np.zeros(B, np.int32)
    opt = ("lsd_0", 0, 0, LSD_MAX_CLUSTER_BITS) if cfg is None else cfg._order_fields()
    C = None if cost is None else np.atleast_2d(np.asarray(cost, dtype=np.float64))
    if C is not None and (C.shape[1] != n or C.shape[0] not in (1, B)):
        raise ValueError(f"cost {C.shape} does not fit {B} shots of {n} bits")
    for b in range(B):
        lb = L[b if L.shape[0] > 1 else 0]
        ids = None if cluster_ids is None else [int(v) for v in cluster_ids]
        cb = None if C is None else C[b if C.shape[0] > 1 else 0]
        r = _lsd_one(rp, ci, cp, cr, S[b], lsd_bit_rank(lb, tie_policy), mb, mc, ids, opt, cb, int(e_bit_order))
        out["row"][b], out["row0"][b] = r[0], r[6]
        out["status"][b], out["rounds"][b], out["clusters"][b], out["max_bits"][b], out["max_checks"][b] = r[1:6]
        out["max_free"][b], out["improved"][b] = r[7:]
    return out


class _PlainDecoder:
    """The default per-shot decoder of :class:`LsdReferenceDecoder`: this package's ``BpOsdDecoder`` without the mode, its
    outputs as the dict the reference works on."""

    def __init__(self, pcm, **kw):
        from .decoder import BpOsdDecoder

        self.dec = BpOsdDecoder(pcm, **kw)

    def update_channel_probs(self, channel_probs):
        self.dec.update_channel_probs(channel_probs)

    def decode_batch(self, syndromes):
        d = self.dec
        osdw = d.decode_batch(syndromes, want_osd0=True, want_bp=True, want_llr=True)
        return {"osdw": osdw, "osd0": d.batch_osd0, "bp": d.batch_bp, "converged": d.batch_converge, "iters": d.batch_iter, "llr": d.batch_llr}


class LsdReferenceDecoder:
    """BP from a per-shot decoder, :func:`lsd_decode_reference` on the shots it leaves open, that decoder's OSD rows on the
    shots LSD does not solve: usable as ``decoder_factory=LsdReferenceDecoder`` with ``lsd=cfg`` among the decoder keyword
    arguments (``engine="numpy"``).  ``base_factory(pcm, **kw)`` makes the per-shot decoder -- by default this package's
    ``BpOsdDecoder`` without the mode; the tests bind a CPU oracle -- whose ``decode_batch`` returns a dict with ``bp``,
    ``converged``, ``iters``, ``llr``, ``osdw`` and ``osd0``.  Shots BP converged on keep BP's decision and have status -1
    and zeros; status-0 shots get the LSD rows (``row`` in ``osdw``, ``row0`` in ``osd0``); the others keep the configured
    OSD's rows (BP's decision with ``osd_off``).  Candidates are weighed as the OSD stage weighs them: by set bits under a
    uniform channel (0 < p < 1) or ``weight_fn=1``, else by log(1/p) of the channel in force."""

    def __init__(self, pcm, lsd=None, base_factory=None, sort_tie_policy=0, weight_fn=0, osd_e_bit_order=0, **kw):
        if not isinstance(lsd, LsdConfig):
            raise ValueError("lsd= must be an LsdConfig")
        self._H = sp.csr_matrix(pcm)
        self.m, self.n = self._H.shape
        self._cfg = lsd
        self._tie = int(sort_tie_policy)
        self._weight_fn, self._e_bit_order = int(weight_fn), int(osd_e_bit_order)
        self.base = (base_factory or _PlainDecoder)(pcm, sort_tie_policy=sort_tie_policy, weight_fn=weight_fn, osd_e_bit_order=osd_e_bit_order, **kw)
        self.last = None
        cp = kw.get("channel_probs")
        self._set_cost(cp if cp is not None else np.full(self.n, float(kw.get("error_rate", 0.0) or 0.0)))

    def _set_cost(self, probs):
        p = np.asarray(probs, dtype=np.float64).reshape(-1)
        if self._weight_fn != 0 or ((p == p[0]).all() and 0.0 < p[0] < 1.0):
            self._cost = None  # the OSD stage counts bits
        else:
            with np.errstate(divide="ignore"):
                self._cost = np.array([math.log(1 / v) if v > 0 else math.inf for v in p.tolist()])

    def update_channel_probs(self, channel_probs):
        self.base.update_channel_probs(channel_probs)
        self._set_cost(channel_probs)

    def decode_batch(self, syndromes, **kw):
        other = sorted(k for k in kw if not k.startswith("want_"))
        if other:
            raise ValueError(f"LsdReferenceDecoder.decode_batch does not take {other}")
        S = np.atleast_2d(np.asarray(syndromes, dtype=np.uint8) & 1)
        r = self.base.decode_batch(S)
        out = {k: np.array(r[k]) for k in ("osdw", "osd0", "bp", "converged", "iters", "llr")}
        B = S.shape[0]
        out["status"] = np.full(B, -1, np.int32)
        for k in ("rounds", "clusters", "max_bits", "max_free", "improved"):
            out[k] = np.zeros(B, np.int32)
        open_ = np.flatnonzero(out["converged"] == 0)
        if open_.size:
            ref = lsd_decode_reference(self._H, S[open_], out["llr"][open_], self._cfg, self._tie, cost=self._cost, e_bit_order=self._e_bit_order)
            for k in ("status", "rounds", "clusters", "max_bits", "max_free", "improved"):
                out[k][open_] = ref[k]
            ok = open_[ref["status"] == 0]
            out["osdw"][ok] = ref["row"][ref["status"] == 0]
            out["osd0"][ok] = ref["row0"][ref["status"] == 0]
        self.last = out
        return out
