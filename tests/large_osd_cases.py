"""Matrices that put osd_large_kernel<RPT> on a chosen panel form, and matrices at the limits of its shape window.

The panel phase of osd_large_kernel.hip.h picks its form from ``nnz``, the number of rows that are not yet pivot rows and
have a non-zero word in the 64-column panel once the open groups are applied: one wave on a list of 2 / 4 / 8 / 16 entries
per lane (nnz <= 128 / 256 / 512 / 1024), all sixteen waves (1025 .. 2048 = OSDL_E2C_CAP), the all-rows register window
beyond.  Which form runs depends on the data -- on the column order OSD sorts the matrix into -- so these cases FIX that
order through the public API: min-sum, ``max_iter = 1``, ``ms_scaling_factor = 2**-20`` and a per-bit channel whose
priors are strictly monotone along the intended order (``probs[perm] = geomspace(0.3, 0.003, n)``).  One iteration moves an
LLR by at most ``dv_max * 2**-20 * max|prior|``, far less than the gap between neighbouring priors, so the posterior order
is the prior order; every prior is positive, so BP's hard decision is all-zero and every non-zero syndrome reaches OSD.
No check may have degree 1 (the reference's min over an empty set sends ``alpha * DBL_MAX``).

With the order in hand the sorted matrix ``H' = H[:, perm]`` is designed (``panel_pcm``): a sequence of 64-column panels
and a short tail.  A LIST block of L rows has ones in its own panel only (2 or 3 per row): rows of other blocks are zero
there and stay zero, so the panel's list holds exactly these L rows in both elimination modes, whichever rows became pivots
before.  A COUPLING block has 64 rows whose restriction to its panel is unit lower-triangular (non-singular: all 64 become
pivot rows and are never listed again) and which carry two more ones in later panels: work for the Jordan fix-up
(Gauss-Jordan, osd_cs) and for the back-substitution (Gaussian, osd_0 / osd_e).  Some list panels hold columns that are sums
of two others (``deficit``): they find fewer than 64 pivots, so that a pivot's ordinal is not its column, in every form.  The
tail's columns are sums of three panel columns, plus two ones per row of the last coupling block (which has no later panel
for them): over the rows that are not pivot rows they stay sums of panel columns, so the tail finds no pivot, k' > 0 and the
rank is complete before the tail's panel -- which is not designed (its word also holds the syndrome bit) and never starts.
Rows are permuted at random, columns scattered by ``perm``.

``panel_list_lengths`` restates the elimination in numpy and returns the list length of every panel and the mask bits of
every pivot group; tests/test_large_osd_cpu.py holds the table to it (and prints what is copied below),
tests/test_gpu_large_osd_forms.py runs the table and ``LIMIT_CASES`` on the device.
"""
from __future__ import annotations

import functools
import time

import numpy as np
import scipy.sparse as sp

OSDL_K = 4  # open pivot groups per apply pass
OSDL_SPARSE_LIST = 6144  # a pass with at most this many mask bits takes the sparse form
OSDL_E2C_CAP = 2048
ALPHA = 2.0 ** -20
FORM_CLASSES = ((1, 128), (129, 256), (257, 512), (513, 1024), (1025, 2048), (2049, 1 << 30))
THRESHOLDS = (128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049)
C = "c"  # a coupling block


def rpt_of(m):
    """launch_osd_large.hip: rows per thread of the instance that holds m rows."""
    return next(r for r in (2, 4, 8, 16) if m <= 1024 * r)


# ------------------------------------------------------------------------------------------------ the panel table
# Keys: id; blocks (in sorted-column order: an int L is a list block of L rows, C a coupling block; m is their sum, 64 per
# coupling block); tail (columns); seed; runs ((method, order) of the plain decodes); he (syndromes H e; every run also
# decodes the all-zero syndrome); rand (uniformly random syndromes, checked by the contract of tests/gpu_contract.py);
# few ({run: k}: that run decodes the first k syndromes H e and the all-zero one only -- the oracle weighs 2^16 candidates per
# shot for osd_e 16);
# rows ((method, order) of the decode with a channel -- a column order -- of its own per shot, or None); move (rows cases:
# the list length of the panel that the per-shot orders put first in shot 0 and last in shot 1).
#
# Measured by tests/test_large_osd_cpu.py (it prints these lines).  lengths: the designed list lengths, which the
# restatement finds under both pivot-row rules in both modes.  passbits: mask bits of each apply pass (OSDL_K groups; the
# last may hold fewer) as lowest-row / highest-row rule, Gaussian then Gauss-Jordan.  oracle: seconds for all references of
# the case on one core of the development machine.
#   rpt2_m2048   m  2048 n 616 rank 572   gauss 1911/2159 14877/15303 7379/6603       jordan 4339/4873 18399/19108 8301/7333        oracle 0.1 s
#   rpt2_m1316   m  1316 n 360 rank 317   gauss 515/471 13906/13948                   jordan 6275/6157 17030/16808                  oracle 5.4 s
#   rpt4_m3265   m  3265 n 360 rank 315   gauss 46637/43853 0/0                       jordan 51215/48072 601/617                    oracle 0.3 s
#   rpt8_m8192   m  8192 n 616 rank 573   gauss 80505/82709 42693/44972 0/0           jordan 83043/85619 45517/47956 1604/1594      oracle 0.8 s
#   rpt16_m8193  m  8193 n 488 rank 443   gauss 79868/85662 47539/42120               jordan 83633/89969 52392/46037                oracle 0.6 s
#   rpt16_m16384 m 16384 n 744 rank 700   gauss 88493/98443 91574/93377 62355/55577   jordan 90941/101217 96708/98024 66344/59192   oracle 2.8 s
# Sparse passes (more than 0 and fewer than OSDL_SPARSE_LIST / 2 = 3072 bits under both rules): Gaussian rpt2_m2048 pass 0 and
# rpt2_m1316 pass 0; Gauss-Jordan rpt4_m3265 pass 1 and rpt8_m8192 pass 2 (Gauss-Jordan also counts the pivot rows' own masks and
# the fix-up masks, so its passes are heavier).  Table passes (above 2 * OSDL_SPARSE_LIST = 12288 under both rules): every
# matrix.  Both kinds in one elimination: rpt2_m2048 and rpt2_m1316 (Gaussian), rpt4_m3265 and rpt8_m8192 (Gauss-Jordan).
# rpt2_m1316's 5.4 s are the four shots of osd_e 16 (65536 candidates each).
# deficit ({panel: d}): d columns of that list panel are sums of two others over the block's rows, so the panel finds 64 - d
# pivots and pivot q is not column q.  Panels with fewer than 64 pivots, by form: 64 (random blocks of 64 rows come out short
# on their own) | 129 | 257 | 513, 1024 | 1025, 1914, 2048 | 2049, 2813; every form also keeps full panels.  Where the last
# panel has a deficit (513, 1024, 1914, 2813) its column 63 is a dependent one: the rank is complete, and the elimination
# stops, in the middle of that panel.
PANEL_CASES = [
    dict(id="rpt2_m2048", blocks=(C, 128, 129, C, 256, 257, 125, 512, 513), tail=40, seed=1,
         runs=(("osd_0", 0), ("osd_e", 6), ("osd_cs", 6)), he=8, rand=3, rows=("osd_cs", 6), move=513,
         deficit={2: 1, 5: 2, 8: 1}),
    dict(id="rpt2_m1316", blocks=(C, 100, C, 64, 1024), tail=40, seed=2, runs=(("osd_0", 0), ("osd_e", 16), ("osd_cs", 6)), he=8,
         rand=0, rows=None, few={("osd_e", 16): 4}, deficit={4: 1}),
    dict(id="rpt4_m3265", blocks=(1025, C, 2048, 64, C), tail=40, seed=3, runs=(("osd_0", 0), ("osd_e", 6), ("osd_cs", 17)),
         he=8, rand=3, rows=None, deficit={0: 1, 2: 2}),
    dict(id="rpt8_m8192", blocks=(2049, C, 2048, 1025, 1024, C, 513, 1341, C), tail=40, seed=4,
         runs=(("osd_0", 0), ("osd_e", 6), ("osd_cs", 6)), he=6, rand=0, rows=("osd_e", 6), move=2049,
         deficit={0: 1, 4: 1, 6: 1}),
    dict(id="rpt16_m8193", blocks=(2049, C, 2049, 1025, 129, C, 2813), tail=40, seed=5,
         runs=(("osd_0", 0), ("osd_e", 6), ("osd_cs", 6)), he=6, rand=0, rows=None, deficit={2: 2, 3: 1, 4: 1, 6: 1}),
    dict(id="rpt16_m16384", blocks=(2049, 2049, C, 2049, 2049, 1024, 1025, 2048, 2049, C, 1914), tail=40, seed=6,
         runs=(("osd_0", 0), ("osd_e", 6), ("osd_cs", 6)), he=6, rand=0, rows=None, packed=True,
         deficit={0: 1, 6: 1, 7: 1, 10: 1}),
]
PANEL_BY_ID = {c["id"]: c for c in PANEL_CASES}
ROWS_SHOTS = 6


def case_m(case):
    return sum(64 if b == C else b for b in case["blocks"])


def case_n(case):
    return 64 * len(case["blocks"]) + case["tail"]


def designed_lengths(case, order=None):
    """The list length of every panel in elimination order (``order``: a permutation of the panels; default: the table's)."""
    L = [64 if b == C else b for b in case["blocks"]]
    return [L[p] for p in (order if order is not None else range(len(L)))]


@functools.lru_cache(maxsize=None)
def panel_pcm(case_id):
    """(H, perm): the case's parity-check matrix (scipy CSR, uint8, sorted indices) and the intended column order -- sorted
    position j holds column perm[j], so ``H[:, perm]`` is the designed matrix H' with its rows permuted."""
    case = PANEL_BY_ID[case_id]
    rng = np.random.default_rng(100 + case["seed"])
    blocks = case["blocks"]
    P, T = len(blocks), case["tail"]
    m, n = case_m(case), case_n(case)
    A = np.zeros((m, n), dtype=np.uint8)
    coupling = [p for p, b in enumerate(blocks) if b == C]
    tail_ones = []
    r0 = 0
    for p, b in enumerate(blocks):
        c0 = 64 * p
        if b == C:
            for i in range(64):
                A[r0 + i, c0 + i] = 1
                if i:
                    A[r0 + i, c0 + rng.choice(i, size=min(i, int(rng.integers(0, 3))), replace=False)] = 1
            # two more ones to the right: in later coupling panels where the case reorders its panels per shot (list panels
            # move freely there, coupling panels keep their relative order), in any later panel otherwise
            later = [q for q in coupling if q > p] if case["rows"] else list(range(p + 1, P))
            for i in range(64):
                for q in rng.choice(later, size=min(2, len(later)), replace=False):
                    A[r0 + i, 64 * q + rng.integers(64)] = 1
            if len(later) < 2:  # (the last coupling block: ones in the tail instead, set once the tail is built)
                tail_ones += [(r0 + i, int(t)) for i in range(64) for t in rng.choice(T, size=2, replace=False)]
            # (the panel's own columns are shuffled below, with every other panel's)
            r0 += 64
        else:
            assert b >= 64, "a list block shorter than its panel leaves empty columns"
            # ``deficit`` columns of the panel are sums of two others over the block's rows: they find no pivot (the panel has
            # fewer than 64, pivot q is no longer column q); in the last panel column 63 is one of them, so that the rank is
            # complete -- and the elimination stops -- in the middle of a panel
            d = case.get("deficit", {}).get(p, 0)
            dep = ([63] if d and p == P - 1 else []) + [int(x) for x in rng.permutation(63)]
            dep, free = dep[:d], np.array(sorted(set(range(64)) - set(dep[:d])))
            for i in range(b):
                A[r0 + i, c0 + rng.choice(free, size=int(rng.integers(2, 4)), replace=False)] = 1
            for c in free[A[r0:r0 + b, c0 + free].sum(axis=0) == 0]:  # no empty column
                two = np.where(A[r0:r0 + b, c0:c0 + 64].sum(axis=1) == 2)[0]
                A[r0 + rng.choice(two), c0 + c] = 1
            for c in dep:
                a2 = rng.choice(free, size=2, replace=False)
                A[r0:r0 + b, c0 + c] = A[r0:r0 + b, c0 + a2[0]] ^ A[r0:r0 + b, c0 + a2[1]]
            r0 += b
    assert r0 == m
    for p in coupling:  # a coupling panel's columns in random order (the block stays non-singular)
        A[:, 64 * p:64 * p + 64] = A[:, 64 * p + rng.permutation(64)]
    # the tail: sums of three columns of the lighter panels (a tail column is three times as heavy as its sources, and the
    # bound on what BP moves grows with the heaviest column)
    light = np.concatenate([64 * p + np.arange(64) for p, b in enumerate(blocks) if b == C or b <= 1100])
    for t in range(T):
        src = rng.choice(light, size=3, replace=False)
        A[:, 64 * P + t] = A[:, src[0]] ^ A[:, src[1]] ^ A[:, src[2]]
    for r, t in tail_ones:
        A[r, 64 * P + t] = 1
    A = A[rng.permutation(m)]
    perm = rng.permutation(n)
    H = np.zeros_like(A)
    H[:, perm] = A
    H = sp.csr_matrix(H)
    H.sort_indices()
    perm.setflags(write=False)
    return H, perm


def channel_for(perm):
    """Per-bit probabilities that sort the columns into ``perm``: the least reliable bit (highest probability) first."""
    probs = np.empty(len(perm))
    probs[perm] = np.geomspace(0.3, 0.003, len(perm))
    return probs


@functools.lru_cache(maxsize=None)
def shot_orders(case_id):
    """(panel orders [B][P], column orders perm_b [B][n]) of a rows case: every shot reorders whole panels -- list panels
    anywhere, coupling panels in their relative order, because a coupling block's extra ones sit in later coupling panels --
    and the columns inside each panel; the tail stays last.  Shot 0 starts with the ``move`` panel, shot 1 ends with it."""
    case = PANEL_BY_ID[case_id]
    _, perm = panel_pcm(case_id)
    rng = np.random.default_rng(200 + case["seed"])
    blocks = case["blocks"]
    P, n = len(blocks), case_n(case)
    coupling = [p for p, b in enumerate(blocks) if b == C]
    mv = blocks.index(case["move"])
    porders, perms = [], []
    for b in range(ROWS_SHOTS):
        order = [int(p) for p in rng.permutation(P) if p != mv]
        order = [mv] + order if b == 0 else (order + [mv] if b == 1 else order[:b] + [mv] + order[b:])
        slots = [i for i, p in enumerate(order) if p in coupling]
        for i, p in zip(slots, coupling):
            order[i] = p
        cols = np.concatenate([64 * p + rng.permutation(64) for p in order] + [64 * P + rng.permutation(case["tail"])])
        porders.append(order)
        perms.append(perm[cols])
    return porders, np.array(perms)


def settings(case, method, order, perm=None):
    kw = dict(bp_method="ms", max_iter=1, ms_scaling_factor=ALPHA, osd_method=method, osd_order=order)
    kw["channel_probs"] = channel_for(panel_pcm(case["id"])[1] if perm is None else perm)
    return kw


@functools.lru_cache(maxsize=None)
def syndromes(case_id):
    """(S, c): ``he`` syndromes H e and the all-zero one -- the first c rows, in the column space -- then ``rand`` uniformly
    random ones (outside it: the matrices are tall and rank-deficient)."""
    case = PANEL_BY_ID[case_id]
    H, _ = panel_pcm(case_id)
    m, n = H.shape
    rng = np.random.default_rng(300 + case["seed"])
    e = (rng.random((case["he"], n)) < 0.05).astype(np.int32)
    he = (np.asarray(H.astype(np.int32) @ e.T) % 2).T
    S = np.concatenate([he, np.zeros((1, m), np.int64), rng.integers(0, 2, size=(case["rand"], m))]).astype(np.uint8)
    S = np.ascontiguousarray(S)
    S.setflags(write=False)
    return S, case["he"] + 1


def run_syndromes(case_id, method, order):
    """(S, c) of one run: syndromes(case_id), or the few of them the table keeps for a run with a slow reference."""
    S, c = syndromes(case_id)
    k = PANEL_BY_ID[case_id].get("few", {}).get((method, order))
    if k is None:
        return S, c
    S = np.ascontiguousarray(np.concatenate([S[:k], S[c - 1:c]]))
    S.setflags(write=False)
    return S, k + 1


@functools.lru_cache(maxsize=None)
def rows_inputs(case_id):
    """(P [B, n], S [B, m]) of a rows case: shot b's channel sorts the columns into shot_orders()[1][b]."""
    H, _ = panel_pcm(case_id)
    _, perms = shot_orders(case_id)
    P = np.array([channel_for(p) for p in perms])
    S = np.array(syndromes(case_id)[0][:ROWS_SHOTS])
    P.setflags(write=False)
    S.setflags(write=False)
    return P, S


ORACLE_SECONDS = {}  # case id -> seconds spent in the oracle (what the table's comment quotes)


def _freeze(ref):
    for v in ref.values():
        if v is not None:
            v.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(case_id, method, order):
    """The oracle's decode of syndromes(case_id) in the table's column order: computed once per process, read-only."""
    from oracle import OracleDecoder

    case = PANEL_BY_ID[case_id]
    H, _ = panel_pcm(case_id)
    S, _ = run_syndromes(case_id, method, order)
    t0 = time.perf_counter()
    o = OracleDecoder(H, **settings(case, method, order))
    ref = o.decode_batch(S)
    ref["rank"] = np.array(o.rank)
    ORACLE_SECONDS[case_id] = ORACLE_SECONDS.get(case_id, 0.0) + time.perf_counter() - t0
    return _freeze(ref)


@functools.lru_cache(maxsize=None)
def rows_reference(case_id):
    """The oracle, shot by shot, each with its own channel: update_channel_probs(P[b]), then decode S[b]."""
    from oracle import OracleDecoder

    case = PANEL_BY_ID[case_id]
    H, _ = panel_pcm(case_id)
    P, S = rows_inputs(case_id)
    t0 = time.perf_counter()
    o = OracleDecoder(H, **settings(case, *case["rows"]))
    outs = []
    for b in range(len(S)):
        o.update_channel_probs(P[b])
        outs.append(o.decode_batch(S[b:b + 1]))
    ORACLE_SECONDS[case_id] = ORACLE_SECONDS.get(case_id, 0.0) + time.perf_counter() - t0
    return _freeze({k: np.concatenate([r[k] for r in outs]) for k in outs[0]})


# ------------------------------------------------------------------------------------------------ the restatement
def _popcount(a):
    return int(np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).sum())


def panel_list_lengths(Hsorted, rank, mode, pick):
    """A plain elimination of ``Hsorted`` (dense 0/1, columns in OSD's order), left to right in panels of 64 columns, until
    ``rank`` pivots are found -- as osd_large_kernel.hip.h walks it.  ``mode``: "gauss" (osd_0 / osd_e: a pivot row is final
    when chosen, only rows that are not pivot rows are reduced) or "jordan" (osd_cs: every row is).  ``pick``: "lowest" or
    "highest" -- which of a column's candidate rows becomes its pivot row.

    Returns (lengths, bits, nrank, npiv, last).  npiv[w]: the pivots found in panel w; last: (panel, column inside it) of the
    last pivot.  lengths[w]: the rows that are not pivot rows before panel w and have a one in it after
    all earlier reductions (the kernel's nnz).  bits[g]: the mask bits of pivot group g as the kernel counts them for
    ``passbits`` -- a row's mask names the pivot rows of the panel, at the panel's start, that it absorbed; the Gaussian
    list forms leave the new pivot rows' own masks out, Gauss-Jordan counts the earlier pivot rows' fix-up masks in."""
    A = np.asarray(Hsorted, dtype=np.uint8)
    m, n = A.shape
    W = (n + 63) // 64
    pad = np.zeros((m, 64 * W), np.uint8)
    pad[:, :n] = A
    M = np.packbits(pad, axis=1, bitorder="little").view("<u8").copy()
    used = np.zeros(m, bool)
    lengths, bits, npiv = [], [], []
    nrank, last = 0, None
    for w in range(W):
        if nrank >= rank:
            break
        nnz = int((~used & (M[:, w] != 0)).sum())
        lengths.append(nnz)
        T = np.zeros(m, np.uint64)
        pivots = []
        for c in range(min(64, n - 64 * w)):
            if nrank >= rank:
                break
            bit = ((M[:, w] >> np.uint64(c)) & np.uint64(1)).astype(bool)
            cand = np.flatnonzero(bit & ~used)
            if cand.size == 0:
                continue
            p = int(cand[0] if pick == "lowest" else cand[-1])
            if mode == "gauss":
                bit &= ~used
            bit[p] = False
            rows = np.flatnonzero(bit)
            M[rows] ^= M[p]
            T[rows] ^= T[p] ^ (np.uint64(1) << np.uint64(len(pivots)))
            used[p] = True
            pivots.append(p)
            nrank += 1
            last = (w, c)
        npiv.append(len(pivots))
        if pivots:
            b = _popcount(T)
            if mode == "gauss" and nnz <= OSDL_E2C_CAP:
                b -= _popcount(T[pivots])
            bits.append(b)
    return lengths, bits, nrank, npiv, last


def passbits(bits):
    """Mask bits per apply pass: OSDL_K groups each, the last pass what is left."""
    return [int(sum(bits[i:i + OSDL_K])) for i in range(0, len(bits), OSDL_K)]


def form_class(nnz):
    return next(i for i, (lo, hi) in enumerate(FORM_CLASSES) if lo <= nnz <= hi)


# ------------------------------------------------------------------------------------------------ the shape limits
# Keys: id, m, n, kind ("wide": check degree 32 -- one pass over a permutation of the columns, so that every column has a
# check, the rest at random; "rows4": four random columns per row), runs, shots, packed (also through the packed host API).
# Ordinary channel (error_rate 0.05, min-sum 0.625, two iterations).  The sort size nsort is 16384 from n = 8193 and 32768
# from n = 16385: with n = 8192 / 8193 and 16384 / 16385 both sides of either switch; n = 32767 and m = 16384 are the last
# sizes the library takes.  Oracle seconds per case on one core of the development machine (tests/test_large_osd_cpu.py
# prints them): wide_n8192 0.1, wide_n8193 0.1, wide_n16384 0.1, wide_n16385 3.9 (osd_cs: one shot), wide_n32767 0.1,
# rows4_m8193 0.6 (rank 8097).
_WIDE_RUNS = (("osd_0", 0), ("osd_e", 6))
LIMIT_CASES = [dict(id=f"wide_n{n_}", kind="wide", m=1100, n=n_, seed=n_, shots=2,
                    runs=_WIDE_RUNS + ((("osd_cs", 6),) if n_ == 16385 else ()), packed=n_ == 32767)
               for n_ in (8192, 8193, 16384, 16385, 32767)]
LIMIT_CASES.append(dict(id="rows4_m8193", kind="rows4", m=8193, n=8300, seed=7, shots=1, runs=(("osd_e", 4),), packed=False))
LIMIT_BY_ID = {c["id"]: c for c in LIMIT_CASES}
LIMIT_SETTINGS = dict(error_rate=0.05, bp_method="ms", max_iter=2, ms_scaling_factor=0.625)


@functools.lru_cache(maxsize=None)
def limit_pcm(case_id):
    case = LIMIT_BY_ID[case_id]
    m, n = case["m"], case["n"]
    rng = np.random.default_rng(400 + case["seed"])
    if case["kind"] == "wide":
        dc = 32
        assert m * dc >= n
        rows = [list(r) for r in np.array_split(rng.permutation(n), m)]
        for r in rows:
            have = set(int(x) for x in r)
            while len(have) < dc:
                have.add(int(rng.integers(n)))
            r[:] = sorted(have)
    else:
        rows = [sorted(int(x) for x in rng.choice(n, size=4, replace=False)) for _ in range(m)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    H = sp.csr_matrix((np.ones(indptr[-1], np.uint8), np.concatenate(rows), indptr), shape=(m, n))
    H.sort_indices()
    return H


def limit_bp_instance(H):
    """bposd_capi.hip: degrees beyond the compiled pairs (check degree 16, bit degree 8) run on bp_anydeg_kernel."""
    dc = int(np.diff(H.indptr).max())
    dv = int(np.bincount(H.indices, minlength=H.shape[1]).max())
    assert dc > 16 or dv > 8, "the limit cases are written for the any-degree BP kernel"
    return ("bp_anydeg_kernel", ())


@functools.lru_cache(maxsize=None)
def limit_syndromes(case_id):
    case = LIMIT_BY_ID[case_id]
    H = limit_pcm(case_id)
    rng = np.random.default_rng(500 + case["seed"])
    e = (rng.random((case["shots"], H.shape[1])) < 0.05).astype(np.int32)
    S = np.ascontiguousarray((np.asarray(H.astype(np.int32) @ e.T) % 2).T.astype(np.uint8))
    S.setflags(write=False)
    return S


def limit_run_syndromes(case_id, method):
    """The shots of one run: osd_cs takes the first one only (the oracle weighs all n - rank single candidates: 5.5 s per
    shot at 1100 x 16385)."""
    S = limit_syndromes(case_id)
    return S[:1] if method == "osd_cs" else S


@functools.lru_cache(maxsize=None)
def limit_reference(case_id, method, order):
    from oracle import OracleDecoder

    t0 = time.perf_counter()
    o = OracleDecoder(limit_pcm(case_id), osd_method=method, osd_order=order, **LIMIT_SETTINGS)
    ref = o.decode_batch(limit_run_syndromes(case_id, method))
    ref["rank"] = np.array(o.rank)
    ORACLE_SECONDS[case_id] = ORACLE_SECONDS.get(case_id, 0.0) + time.perf_counter() - t0
    return _freeze(ref)
