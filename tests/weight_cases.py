"""The fp64 candidate sweep of osd_kernel<W> and osd_large_kernel<RPT> (the `if (P.cost)` branch of either kernel) at every
instance edge, with channels whose candidate weights tie: the table, the inputs, the oracle references and a numpy
restatement of the sweep alone.

The sweep weighs every OSD candidate with the sum of log(1 / p_i) over its set bits, added in ascending original bit
index, and keeps the first candidate of the enumeration that attains the strict minimum.  With a continuous channel
(``uniform(0.03, 0.15)``) no two candidate weights are ever equal and no pair of them is close enough for the order of the
additions to decide, so such a run notices neither a re-ordered sum nor a changed tie rule.  A two-valued channel makes
both decide: many candidates hold the same multiset of costs (equal up to the rounding of the order they are added in, or
exactly equal).  ``WEIGHT_EDGES`` has one row per (instance, edge) the sweep must reach, each on the matrix of an ``EDGES``
row (tests/edge_codes.py); ``sweep_restatement`` restates the sweep with the two mutants (sum in descending index order, keep
the last lightest candidate) that tests/test_weight_cpu.py counts per row, so that the inputs provably tell them apart.
tests/test_gpu_weight_edges.py runs the table on the device.
"""
from __future__ import annotations

import functools
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.sparse as sp

from tests.edge_codes import EDGE_BY_ID, osd_words, pcm_for

# the two-valued channels: (share of the bits on the first value, the first value, the other value)
MIXES = {"half": (0.5, 0.11, 0.04), "sparse": (0.15, 1.0 / 3.0, 0.0172)}
KINDS = ("vector", "select", "rows", "flat-rows", "continuous")
WEIGHT_EDGES = []


def _w(edge, method, order, mix="half", **kw):
    e = EDGE_BY_ID[edge]
    hbm = e["osd"][0] == "osd_large_kernel"
    kw.setdefault("osd", e["osd"])
    kw.setdefault("shots", 11 if hbm else (48 if e["n"] <= 1023 else 24))
    kw.setdefault("seed", 5)
    kw.setdefault("max_iter", 2)
    kw.setdefault("continuous", hbm)
    kw.setdefault("err", 0.12 if hbm else (0.1 if e["n"] < 400 else 0.07))
    WEIGHT_EDGES.append(dict(id=f"{edge}-{method}{order}", edge=edge, method=method, order=order, mix=mix, hbm=hbm,
                             osd_variant=e["osd_variant"], **kw))


# Keys: id, edge (the EDGES row whose matrix the row reuses), method, order, mix (MIXES), osd (the instance last_instance()
# must report), osd_variant (as the EDGES row sets it), shots (the all-zero syndrome included), seed, max_iter, err (the rate the
# errors e of the syndromes H e are drawn at; 0.1 for n < 400, else 0.07, and 0.12 on the HBM path, unless the row says otherwise), bit_order
# (osd_e_bit_order), continuous (the row also runs the continuous kind), hbm.
#
# Measured on the oracle and the restatement (tests/test_weight_cpu.py prints them and asserts the minima): shots in OSD /
# of them order-sensitive (the sum_descending mutant changes osdw) / tie-rule-sensitive (the last_wins mutant changes osdw),
# for the vector kind:
#   osd_kernel_W1_n63 cs6          47 /  6 / 14      osd_kernel_rows_m513_n1023 e8   47 / 24 / 44
#   osd_kernel_W2_n64 e5           46 /  3 / 24      kprime5_osd_cs_osd_kernel cs5   95 /  4 / 21
#   osd_kernel_W4_n255 cs64        47 /  6 / 21      kprime_osd_e_osd_kernel e18     47 /  2 / 12
#   osd_kernel_W8_n511 e12         47 /  4 / 40      osd_wave_5x10_corner cs6        47 /  3 / 11
#   osd_kernel_W16_n1023 cs20      47 /  3 / 10      osd_mw_shape1_m512_n959 cs6     47 /  4 /  7
#   osd_kernel_W24_n1535 e10       23 / 14 / 23      large_m1025_n2040 cs6           10 /  0 /  1
#   osd_kernel_W31_n1983 cs42      23 /  2 /  2      large_rpt4_m2049 cs16, cs17     10 /  2 /  5
#   osd_kernel_W32_n2047 cs64      23 /  2 /  8      large_rpt8_m4097 cs64           21 /  2 / 14
#   osd_kernel_W32_n2047 e12       23 / 15 / 23      large_n4095 e12                 10 /  3 / 10
#   osd_kernel_rows_m129_n255 cs10 47 /  2 / 23      large_n4097 e12                 10 /  4 / 10
#   osd_kernel_rows_m641_n1535 cs20 23 / 3 /  3      kprime_osd_e_large e16          21 /  3 /  9
#                                                    kprime64_osd_cs_large cs64      21 /  8 / 10
# order-sensitive shots together: 97 on the small path, 24 on the HBM path (counted for the vector kind
# only).  Where a row departs from the defaults (another mix or seed, a higher error
# rate, one BP iteration, up to twice the shots) the defaults left one of the conditions of tests/test_weight_cpu.py unmet:
# nearly full-rank matrices (k' = 5, 16, 18, 64 and the HBM shapes) rarely leave OSD-0 unless BP is cut short on heavy errors.
# osd_kernel<W>: one row per width, the last n of the width (W = 2: the first)
_w("osd_kernel_W1_n63", "osd_cs", 6, mix="sparse")
_w("osd_kernel_W2_n64", "osd_e", 5, mix="sparse")
_w("osd_kernel_W4_n255", "osd_cs", 64)  # 2016 pairs: all of pairw
_w("osd_kernel_W8_n511", "osd_e", 12, mix="sparse", bit_order=1)
_w("osd_kernel_W16_n1023", "osd_cs", 20)
_w("osd_kernel_W24_n1535", "osd_e", 10)
_w("osd_kernel_W31_n1983", "osd_cs", 42)
_w("osd_kernel_W32_n2047", "osd_cs", 64, mix="sparse", seed=6, continuous=True)  # m = 1024, row 1023, the largest LDS carve-up
_w("osd_kernel_W32_n2047", "osd_e", 12, continuous=True)
# the row shapes of osd_kernel: two waves, six waves, the row buffer in a region of its own
_w("osd_kernel_rows_m129_n255", "osd_cs", 10)
_w("osd_kernel_rows_m641_n1535", "osd_cs", 20)
_w("osd_kernel_rows_m513_n1023", "osd_e", 8)
# order equal to k'
_w("kprime5_osd_cs_osd_kernel", "osd_cs", 5, max_iter=1, err=0.15, seed=6, shots=96)
_w("kprime_osd_e_osd_kernel", "osd_e", 18, max_iter=1, err=0.2)
# dispatch: a request for the wave kernels with a weighted call lands on osd_kernel (launch_osd.hip: P.cost != nullptr)
_w("osd_wave_5x10_corner_m320_n639", "osd_cs", 6, osd=("osd_kernel", (osd_words(639),)))
_w("osd_mw_shape1_m512_n959_v2", "osd_cs", 6, osd=("osd_kernel", (osd_words(959),)))
# osd_large_kernel<RPT>
_w("large_m1025_n2040", "osd_cs", 6)  # RPT 2
_w("large_rpt4_m2049", "osd_cs", 16)  # the 16-bit form of the row masks
_w("large_rpt4_m2049", "osd_cs", 17)  # the 64-bit form
_w("large_rpt8_m4097", "osd_cs", 64, mix="sparse", shots=22)
_w("large_n4095", "osd_e", 12)
_w("large_n4097", "osd_e", 12)
_w("kprime_osd_e_large", "osd_e", 16, max_iter=1, err=0.45, shots=22)  # wd filled to its last entry
_w("kprime64_osd_cs_large", "osd_cs", 64, shots=22)  # span equal to k'

ROW_BY_ID = {r["id"]: r for r in WEIGHT_EDGES}
UPDATE_ROWS = ("osd_kernel_W16_n1023-osd_cs20", "large_rpt4_m2049-osd_cs17")  # uniform -> two-valued -> uniform on one handle
EXTREME_ROW = "osd_kernel_W4_n255-osd_cs64"  # the vector kind once more with entries of exactly 1.0 and exactly 0.0


def row_kinds(row):
    return KINDS if row["continuous"] else KINDS[:4]


@functools.lru_cache(maxsize=None)
def matrix(edge):
    H = sp.csr_matrix(pcm_for(EDGE_BY_ID[edge]), dtype=np.uint8)
    H.sort_indices()
    return H


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def inputs(row_id):
    """Everything a row decodes, drawn once and read-only: S [B, m] (H e for random e, the all-zero syndrome last -- all in
    the column space), q (the ctor's uniform channel: the mix's second value), vec [n] (the two-valued vector), sel [B, n] and
    alt [n] (the per-shot two-valued channel: alt where sel, q elsewhere), rows [B, n] (the same as channel rows), flat [B, n]
    (rows all equal to q), cont [n] (uniform(0.03, 0.15))."""
    row = ROW_BY_ID[row_id]
    H = matrix(row["edge"])
    m, n = H.shape
    B = row["shots"]
    rng = np.random.default_rng(row["seed"])
    e = rng.random((B - 1, n)) < row["err"]
    S = np.zeros((B, m), np.uint8)
    S[:B - 1] = (np.asarray(sp.csr_matrix(H, dtype=np.int32) @ e.T.astype(np.int32)) % 2).T
    share, hi, lo = MIXES[row["mix"]]
    vec = np.where(rng.random(n) < share, hi, lo)
    sel = (rng.random((B, n)) < share).astype(np.uint8)
    alt = np.full(n, hi)
    rows = np.where(sel != 0, alt, lo)
    flat = np.full((B, n), lo)
    cont = rng.uniform(0.03, 0.15, size=n)
    _frozen(S, vec, sel, alt, rows, flat, cont)
    return dict(S=S, q=lo, vec=vec, sel=sel, alt=alt, rows=rows, flat=flat, cont=cont)


def settings(row):
    """Decoder keywords of a row without its channel: min-sum 0.625, BP cut after max_iter iterations."""
    kw = dict(max_iter=row["max_iter"], bp_method="ms", ms_scaling_factor=0.625, osd_method=row["method"], osd_order=row["order"])
    if row.get("bit_order") is not None:
        kw["osd_e_bit_order"] = row["bit_order"]
    return kw


def expected_osd(row):
    return row["osd"] + (False,)


@functools.lru_cache(maxsize=None)
def extreme_vector(row_id=EXTREME_ROW):
    """The row's two-valued vector with three entries of exactly 1.0 (cost 0, prior LLR -inf) and three of exactly 0.0 (cost
    and prior LLR +inf), on six bits that pairwise share no check -- so no check sees two infinite messages, and no bit an
    infinite message (inf - inf is the one way to a NaN)."""
    H = matrix(ROW_BY_ID[row_id]["edge"])
    A = (H.T.astype(np.int32) @ H.astype(np.int32)).tocsr()  # bits i, j share a check where A[i, j] != 0
    rng = np.random.default_rng(17)
    picked = []
    for i in rng.permutation(H.shape[1]):
        if all(A[i, j] == 0 for j in picked):
            picked.append(int(i))
        if len(picked) == 6:
            break
    if len(picked) < 6:
        raise ValueError("no six bits that pairwise share no check")
    vec = np.array(inputs(row_id)["vec"])
    vec[picked[:3]] = 1.0
    vec[picked[3:]] = 0.0
    vec.setflags(write=False)
    return vec, tuple(picked)


def cost_of(p):
    """log(1 / p) as the oracle and the library evaluate it (the host's libm; +inf at p = 0)."""
    p = np.asarray(p, dtype=np.float64)
    return np.array([math.log(1 / x) if x > 0 else math.inf for x in p.ravel()]).reshape(p.shape)


# ------------------------------------------------------------------------------------------------ the oracle references
def oracle_run(H, kw, S, steps):
    """The oracle used the documented way, shot by shot.  ``kw`` holds the ctor's channel (error_rate or channel_probs).  Every
    step is a dict with ``channel`` ([n]: update_channel_probs before the step, or None) and ``rows`` ([B, n]:
    update_channel_probs(rows[b]) before shot b, or None); all steps run on the same handles, in order.  The shots are spread
    over threads in contiguous slices, one oracle handle per thread: per shot the computation is the same function of the same
    inputs, whichever thread runs it.  Returns one result dict per step."""
    import oracle.oracle as oo

    B = len(S)
    k = max(1, min(int(oo.DEFAULT_THREADS), B))
    cuts = [B * j // k for j in range(k + 1)]

    def run(j):
        o = oo.OracleDecoder(H, **kw)
        outs = []
        for step in steps:
            if step.get("channel") is not None:
                o.update_channel_probs(step["channel"])
            res = []
            for b in range(cuts[j], cuts[j + 1]):
                if step.get("rows") is not None:
                    o.update_channel_probs(step["rows"][b])
                res.append(o.decode_batch(S[b:b + 1], want_llr=True))
            outs.append(res)
        return outs

    with ThreadPoolExecutor(max_workers=k) as ex:
        parts = list(ex.map(run, range(k)))
    refs = []
    for i in range(len(steps)):
        shots = [r for part in parts for r in part[i]]
        ref = {key: np.concatenate([r[key] for r in shots]) for key in ("osdw", "osd0", "bp", "converged", "iters", "llr")}
        _frozen(*ref.values())
        refs.append(ref)
    return refs


@functools.lru_cache(maxsize=None)
def reference(row_id, kind):
    """The oracle's decode of one kind of a row, computed once per process and never written to.  "rows" is the same oracle
    computation as "select" (update_channel_probs(where(sel[b], alt, q)) before shot b) and "flat-rows" the same as "uniform":
    the rows of either are, entry for entry, the channel the other sets."""
    row, inp = ROW_BY_ID[row_id], inputs(row_id)
    H, kw, S = matrix(row["edge"]), settings(row), inp["S"]
    if kind in ("rows", "select"):
        return oracle_run(H, dict(kw, error_rate=inp["q"]), S, [dict(rows=inp["rows"])])[0]
    if kind in ("flat-rows", "uniform"):
        return oracle_run(H, dict(kw, error_rate=inp["q"]), S, [{}])[0]
    probs = {"vector": inp["vec"], "continuous": inp["cont"], "extreme": extreme_vector(row_id)[0] if kind == "extreme" else None}[kind]
    return oracle_run(H, dict(kw, channel_probs=probs), S, [{}])[0]


def update_channels(row_id):
    """The channels of the update run: the ctor's uniform q, then update_channel_probs(two-valued), then back to uniform."""
    inp = inputs(row_id)
    return [None, inp["vec"], np.full(len(inp["vec"]), inp["q"])]


@functools.lru_cache(maxsize=None)
def update_references(row_id):
    row, inp = ROW_BY_ID[row_id], inputs(row_id)
    return tuple(oracle_run(matrix(row["edge"]), dict(settings(row), error_rate=inp["q"]), inp["S"],
                            [dict(channel=c) for c in update_channels(row_id)]))


def kind_cost(row_id, kind, b):
    """The weights shot b of a kind is ranked with."""
    inp = inputs(row_id)
    if kind in ("select", "rows"):
        return cost_of(inp["rows"][b])
    if kind in ("flat-rows", "uniform"):
        return cost_of(inp["flat"][b])
    return cost_of({"vector": inp["vec"], "continuous": inp["cont"]}[kind] if kind != "extreme" else extreme_vector(row_id)[0])


# ------------------------------------------------------------------------------------------- the sweep, restated in numpy
@functools.lru_cache(maxsize=2)
def dense(edge):
    """The row's matrix as a dense array, for ``Sweep`` (which permutes its columns per shot)."""
    return np.ascontiguousarray(matrix(edge).toarray(), dtype=np.uint8)


def _gauss_jordan(U, m, n):
    """Reduced row echelon form, in place, of bit-packed rows (uint64 words, bit j of word w = column 64 w + j) over columns
    0 .. n - 1, pivots taken greedily from the left; columns from n on (the syndrome) ride along.  Returns the pivot columns."""
    piv = []
    r = 0
    for j in range(n):
        if r == m:
            break
        col = (U[:, j >> 6] >> np.uint64(j & 63)) & np.uint64(1)
        below = np.flatnonzero(col[r:])
        if below.size == 0:
            continue
        p = r + int(below[0])
        if p != r:
            U[[r, p]] = U[[p, r]]
            col[p] = col[r]
        col[r] = 0
        rows = np.flatnonzero(col)
        if rows.size:
            U[rows] ^= U[r]
        piv.append(j)
        r += 1
    return piv


class Sweep:
    """The candidates of one shot's OSD search: stable sort of the LLRs, Gauss-Jordan on the bit-packed rows of H in that
    column order with the syndrome as the last column, then the candidates in the oracle's enumeration order -- index 0 is
    OSD-0, then for osd_cs the singles over all k' non-pivot columns and the pairs (a < b < order, a outer) over the first
    ``order`` of them, for osd_e the patterns 1 .. 2^order - 1 (bit b of the pattern switches non-pivot b, or order - 1 - b
    with ``bit_order`` 1).  The syndrome must lie in the column space of H."""

    def __init__(self, H, syndrome, llr, method, order, bit_order=0):
        Hd = np.asarray(H.toarray() if sp.issparse(H) else H, dtype=np.uint8)
        m, n = Hd.shape
        self.n = n
        self.perm = np.argsort(np.asarray(llr, dtype=np.float64), kind="stable")  # sorted position -> original bit
        words = (n + 1 + 63) // 64
        A = np.zeros((m, words * 64), np.uint8)
        A[:, :n] = Hd[:, self.perm]
        A[:, n] = np.asarray(syndrome, dtype=np.uint8) & 1
        U = np.packbits(A, axis=1, bitorder="little").view("<u8").astype(np.uint64)
        self.piv = np.array(_gauss_jordan(U, m, n), dtype=np.int64)
        rank = len(self.piv)
        D = np.unpackbits(U.astype("<u8").view(np.uint8), axis=1, bitorder="little")
        assert not D[rank:, n].any(), "the syndrome is outside the column space"
        ispiv = np.zeros(n, bool)
        ispiv[self.piv] = True
        self.nonpiv = np.flatnonzero(~ispiv)
        self.y = D[:rank, n].copy()
        kp = len(self.nonpiv)
        assert 0 < order <= kp
        if method == "osd_cs":
            self.R = np.ascontiguousarray(D[:rank, self.nonpiv].T)  # [k', rank]: the reduced non-pivot columns
            a, b = np.triu_indices(order, 1)
            none = np.full(1, -1)
            self.ta = np.concatenate([none, np.arange(kp), a])
            self.tb = np.concatenate([none, np.full(kp, -1), b])
            self.bits = None
        elif method == "osd_e":
            self.R = np.ascontiguousarray(D[:rank, self.nonpiv[:order]].T)  # [order, rank]
            self.w = order
            self.bit_order = bit_order
            self.ta = self.tb = None
        else:
            raise ValueError(method)
        self.count = len(self.ta) if self.ta is not None else 1 << order

    def candidates(self, lo, hi):
        """Candidates lo .. hi - 1 as rows of bits in ORIGINAL bit order."""
        c = hi - lo
        Xs = np.zeros((c, self.n), np.uint8)
        if self.ta is not None:
            ta, tb = self.ta[lo:hi], self.tb[lo:hi]
            pp = np.broadcast_to(self.y, (c, len(self.y))).copy()
            ia, ib = np.flatnonzero(ta >= 0), np.flatnonzero(tb >= 0)
            pp[ia] ^= self.R[ta[ia]]
            pp[ib] ^= self.R[tb[ib]]
            Xs[:, self.piv] = pp
            Xs[ia, self.nonpiv[ta[ia]]] = 1
            Xs[ib, self.nonpiv[tb[ib]]] = 1
        else:
            pats = np.arange(lo, hi, dtype=np.int64)
            bits = ((pats[:, None] >> np.arange(self.w)) & 1).astype(np.uint8)  # column b: bit b of the pattern
            if self.bit_order:
                bits = bits[:, ::-1]  # non-pivot t is switched by bit order - 1 - t
            flips = (bits.astype(np.int32) @ self.R.astype(np.int32)) & 1  # what the pattern flips on the pivots
            Xs[:, self.piv] = self.y ^ flips.astype(np.uint8)
            Xs[:, self.nonpiv[:self.w]] = bits
        Xo = np.empty_like(Xs)
        Xo[:, self.perm] = Xs
        return Xo

    def weights(self, specs):
        """One weight array (all candidates) per spec (cost [n], descending): the sum of cost over the set bits, added strictly
        left to right in ascending -- or, for the mutant, descending -- original bit index.  An unset bit adds 0.0, which leaves
        every bit of the running sum alone.  The additions are those of ``np.cumsum(np.where(x, cost, 0.0), axis=1)[:, -1]``
        (``cumsum`` adds in sequence, ``np.sum`` does not; ``weights_by_cumsum`` is that line, and tests/test_weight_cpu.py holds
        the two together), made bit by bit over all candidates at once so that the running sums stay in the cache: the 2^18
        candidates of osd_e 18 would otherwise stream a gigabyte per shot.  ``where``, not ``x * cost``: 0 * inf is NaN, and a
        cost may be +inf."""
        if self.ta is None:
            return self._pattern_weights(specs)
        out = [np.empty(self.count) for _ in specs]
        step = max(1, 16_000_000 // self.n)
        for lo in range(0, self.count, step):
            hi = min(self.count, lo + step)
            XT = np.ascontiguousarray(self.candidates(lo, hi).T) != 0  # [n, candidates]
            live = np.flatnonzero(XT.any(axis=1))  # (a bit no candidate holds adds 0.0 to every sum)
            for (cost, descending), w in zip(specs, out):
                acc = np.zeros(hi - lo)
                for i in (live[::-1] if descending else live):
                    acc += np.where(XT[i], cost[i], 0.0)
                w[lo:hi] = acc
        return out

    def _pattern_weights(self, specs):
        """``weights`` for osd_e without the candidate matrix: over all patterns at once, pivot k holds y[k] xor the parity of
        (pattern and the pivot row's entries in the switched columns) -- row k of FT, built by doubling: pattern p | 2^b flips
        what p flips, and what bit b's column holds -- and switched column t holds its bit of the pattern."""
        w, count, rank = self.w, self.count, len(self.y)
        FT = np.zeros((rank, count), np.uint8)
        for b in range(w):
            FT[:, 1 << b:2 << b] = FT[:, :1 << b] ^ self.R[w - 1 - b if self.bit_order else b][:, None]
        pats = np.arange(count)
        rows = {int(self.perm[self.piv[k]]): FT[k] != self.y[k] for k in range(rank) if self.y[k] or FT[k].any()}
        for t in range(w):
            rows[int(self.perm[self.nonpiv[t]])] = ((pats >> (w - 1 - t if self.bit_order else t)) & 1) != 0
        live = sorted(rows)
        out = []
        for cost, descending in specs:
            acc = np.zeros(count)
            for i in (live[::-1] if descending else live):
                acc += np.where(rows[i], cost[i], 0.0)
            out.append(acc)
        return out

    def weights_by_cumsum(self, cost, descending=False):
        """``weights`` for one spec as the one line it restates (every candidate at once: small shapes only)."""
        X = self.candidates(0, self.count) != 0
        terms = np.where(X[:, ::-1], cost[::-1], 0.0) if descending else np.where(X, cost, 0.0)
        return np.cumsum(terms, axis=1)[:, -1]

    def pick(self, w, last_wins=False):
        """The index of the candidate that wins: the first strict minimum in enumeration order (the mutant: the last candidate
        attaining the minimum).  Two candidates differ in the non-pivot columns they switch, so another index is another row."""
        return int(np.argmin(w)) if not last_wins else len(w) - 1 - int(np.argmin(w[::-1]))

    def candidate(self, i):
        return self.candidates(i, i + 1)[0]


def sweep_restatement(H, syndrome, llr, cost, method, order, bit_order=0, sum_descending=False, last_wins=False):
    """(osd0, osdw) of one shot that reached OSD, from the LLRs BP left and the per-bit weights log(1 / p_i).  The two flags are
    the mutants tests/test_weight_cpu.py counts: weights added in descending bit index, and the last lightest candidate kept
    instead of the first.  tests/ref_numpy.osd_decode states the same in plain Python, for matrices up to n of about 255."""
    sw = Sweep(H, syndrome, llr, method, order, bit_order)
    (w,) = sw.weights([(np.asarray(cost, dtype=np.float64), sum_descending)])
    return sw.candidate(0), sw.candidate(sw.pick(w, last_wins))
