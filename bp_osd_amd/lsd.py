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

import numpy as np
import scipy.sparse as sp

__all__ = ["LsdConfig", "lsd_bit_rank", "lsd_decode_reference", "LsdReferenceDecoder", "LSD_MAX_CLUSTER_BITS", "LSD_MAX_CLUSTER_CHECKS"]

# What one elimination of lsd_kernel holds (csrc/lsd_kernel.hip.h: LSD_RPL rows per lane of a 64-lane wave, LSD_WPR 64-bit
# words per row).  The defaults are the ceilings: see DESIGN.md §4.19.
LSD_MAX_CLUSTER_BITS = 256
LSD_MAX_CLUSTER_CHECKS = 256


class LsdConfig:
    """The LSD mode of a decoder: a cluster that holds more than ``max_cluster_bits`` bits or ``max_cluster_checks`` checks
    after a round ends the shot with status 1 (it goes on to the OSD stage).  Both are integers in [1, 256]; the defaults are
    the ceilings of the kernel.  ValueError names what is wrong."""

    def __init__(self, max_cluster_bits=LSD_MAX_CLUSTER_BITS, max_cluster_checks=LSD_MAX_CLUSTER_CHECKS):
        for name, v, top in (("max_cluster_bits", max_cluster_bits, LSD_MAX_CLUSTER_BITS),
                             ("max_cluster_checks", max_cluster_checks, LSD_MAX_CLUSTER_CHECKS)):
            if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= top:
                raise ValueError(f"{name} = {v} must be an integer in [1, {top}] (the ceiling of lsd_kernel)")
        self.max_cluster_bits = int(max_cluster_bits)
        self.max_cluster_checks = int(max_cluster_checks)

    def __repr__(self):
        return f"LsdConfig(max_cluster_bits={self.max_cluster_bits}, max_cluster_checks={self.max_cluster_checks})"

    def __eq__(self, other):
        return (isinstance(other, LsdConfig) and self.max_cluster_bits == other.max_cluster_bits
                and self.max_cluster_checks == other.max_cluster_checks)

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


def _solve_in_order(A, s):
    """A uint8 [r, c] with its columns already in bit order, s uint8 [r]: (valid, x) with x the solution of A x = s supported
    on the greedy column basis (a column is a basis column iff it is independent of the columns before it)."""
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
    if s[~used].any():
        return False, None
    x = np.zeros(c, np.uint8)
    has = piv_row >= 0
    x[has] = s[piv_row[has]]
    return True, x


def _lsd_one(rp, ci, cp, cr, s, rank, max_bits, max_checks, ids):
    m, n = len(rp) - 1, len(cp) - 1
    seeds = np.flatnonzero(s)
    if ids is None:
        ids = np.arange(seeds.size)
    owner = np.full(m, -1, np.int64)  # cluster id per check
    taken = np.zeros(n, bool)
    clusters = {}  # id -> [set of checks, set of bits, valid, solution {bit: value}]
    for c, k in zip(seeds, ids):
        clusters[int(k)] = [{int(c)}, set(), False, {}]
        owner[c] = int(k)
    rounds, status = 0, 0
    while True:
        invalid = sorted(k for k, cl in clusters.items() if not cl[2])
        if not invalid:
            break
        picks = {}
        for k in invalid:
            best = -1
            for c in clusters[k][0]:
                for j in ci[rp[c]:rp[c + 1]]:
                    if not taken[j] and (best < 0 or rank[j] < rank[best]):
                        best = int(j)
            if best < 0:
                status = 2
            picks[k] = best
        if status == 2:
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
            checks, bits = clusters[k][0], clusters[k][1]
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
            ok, x = _solve_in_order(A, s[rows])
            clusters[k][2] = ok
            clusters[k][3] = dict(zip(cols, x)) if ok else {}
        if status == 1:
            break
    row = np.zeros(n, np.uint8)
    if status == 0:
        for cl in clusters.values():
            for j, v in cl[3].items():
                row[j] = v
    return (row, status, rounds, len(clusters), max((len(cl[1]) for cl in clusters.values()), default=0),
            max((len(cl[0]) for cl in clusters.values()), default=0))


def lsd_decode_reference(H, syndrome, llr, cfg, tie_policy=0, cluster_ids=None):
    """LSD-0 of ``syndrome`` (uint8 [m] or [B, m]) with the soft output ``llr`` (float64 [n] or [B, n]) on the check matrix
    ``H``: dict(row uint8 [B, n], status, rounds, clusters, max_bits int32 [B]).

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
    result does not depend on them."""
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
    out = {"row": np.zeros((B, n), np.uint8)}
    for k in ("status", "rounds", "clusters", "max_bits", "max_checks"):
        out[k] = np.zeros(B, np.int32)
    for b in range(B):
        lb = L[b if L.shape[0] > 1 else 0]
        ids = None if cluster_ids is None else [int(v) for v in cluster_ids]
        r = _lsd_one(rp, ci, cp, cr, S[b], lsd_bit_rank(lb, tie_policy), mb, mc, ids)
        out["row"][b] = r[0]
        out["status"][b], out["rounds"][b], out["clusters"][b], out["max_bits"][b], out["max_checks"][b] = r[1:]
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
    and zeros; status-0 shots get the LSD row in ``osdw`` and ``osd0``; the others keep the configured OSD's rows (BP's
    decision with ``osd_off``)."""

    def __init__(self, pcm, lsd=None, base_factory=None, sort_tie_policy=0, **kw):
        if not isinstance(lsd, LsdConfig):
            raise ValueError("lsd= must be an LsdConfig")
        self._H = sp.csr_matrix(pcm)
        self.m, self.n = self._H.shape
        self._cfg = lsd
        self._tie = int(sort_tie_policy)
        self.base = (base_factory or _PlainDecoder)(pcm, sort_tie_policy=sort_tie_policy, **kw)
        self.last = None

    def update_channel_probs(self, channel_probs):
        self.base.update_channel_probs(channel_probs)

    def decode_batch(self, syndromes, **kw):
        other = sorted(k for k in kw if not k.startswith("want_"))
        if other:
            raise ValueError(f"LsdReferenceDecoder.decode_batch does not take {other}")
        S = np.atleast_2d(np.asarray(syndromes, dtype=np.uint8) & 1)
        r = self.base.decode_batch(S)
        out = {k: np.array(r[k]) for k in ("osdw", "osd0", "bp", "converged", "iters", "llr")}
        B = S.shape[0]
        out["status"] = np.full(B, -1, np.int32)
        for k in ("rounds", "clusters", "max_bits"):
            out[k] = np.zeros(B, np.int32)
        open_ = np.flatnonzero(out["converged"] == 0)
        if open_.size:
            ref = lsd_decode_reference(self._H, S[open_], out["llr"][open_], self._cfg, self._tie)
            for k in ("status", "rounds", "clusters", "max_bits"):
                out[k][open_] = ref[k]
            ok = open_[ref["status"] == 0]
            out["osdw"][ok] = out["osd0"][ok] = ref["row"][ref["status"] == 0]
        self.last = out
        return out
