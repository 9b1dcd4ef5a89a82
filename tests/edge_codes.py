"""Parity-check matrices that sit on the edges of the kernel instances' size windows, and the table of those edges.

Behind one decode call the library picks one of about forty compiled kernel instances, each with a size window fixed at
compile time (launch_osd.hip, launch_osd_large.hip, launch_bp_*.hip).  ``edge_pcm`` builds a matrix of an exact shape with
exact maximum check / bit degrees (so that the intended ``<DC, DV>`` instance or degree class is the one chosen) and an
exact rank deficit (rows appended as sums of two rows), so that noisy syndromes leave ones on rows without a pivot.
``EDGES`` lists every case of tests/test_gpu_edges.py with the instance it must land on; tests/test_edge_codes_cpu.py
checks the matrices without a GPU.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

# bp_kernel degree pairs (bposd_capi.hip kPairs) and bp_class_kernel degree classes (kClassShapes: dclo, dc, dvlo, dvhi)
BP_PAIRS = ((4, 2), (6, 3), (8, 4), (12, 6), (16, 8))
CLASS_SHAPES = ((7, 7, 3, 4), (6, 6, 3, 3), (4, 4, 2, 2), (8, 8, 4, 4), (3, 4, 1, 2))
LDS_PER_CU = 160 * 1024  # MI355X: LDS of one CU


def bp_lds_bytes(dc, mp):
    """bp_kernel.hip.h bp_lds_bytes: messages + mismatch bitmap + control words of one workgroup."""
    return (dc * mp + 2) * 8 + (mp // 32 + 2) * 4 + 8 * 4


def osd_words(n):
    """launch_osd.hip osd_words: the osd_kernel<W> instance that holds n columns and the syndrome bit."""
    need = (n + 1 + 63) // 64
    return next((w for w in (1, 2, 4, 8, 16, 24, 31, 32) if w >= need), 0)


def _deg_pair(dc, dv):
    return next(((a, b) for a, b in BP_PAIRS if a >= dc and b >= dv), None)


def class_shape(H):
    """bposd_capi.hip class_shape_for: the first degree class covering the matrix's degrees, or None."""
    H = sp.csr_matrix(H)
    r, c = np.diff(H.indptr), np.bincount(H.indices, minlength=H.shape[1])
    for s in CLASS_SHAPES:
        if s[0] <= r.min() and r.max() <= s[1] and s[2] <= c.min() and c.max() <= s[3]:
            return s
    return None


def edge_pcm(m, n, dc_max, dv_max, rank_deficit=1, seed=0, dc_min=1, dv_min=1):
    """An m x n parity-check matrix (scipy CSR, uint8) with

    - no empty row, every column of degree dv_min .. dv_max, every row of degree dc_min .. dc_max;
    - maximum check degree exactly ``dc_max`` and maximum bit degree exactly ``dv_max``;
    - rank exactly m - ``rank_deficit``: m - rank_deficit independent rows (row i holds a pivot column that no earlier row
      holds) and ``rank_deficit`` rows appended as sums of two of them, so n - rank = n - m + rank_deficit.

    With the defaults (dc_min = 1) some row has degree <= 2, so no bp_class_kernel degree class covers the matrix and
    the library takes the generic kernels; dc_min = 3, dc_max = 4, dv_max = 2 gives the surface-code class.  Raises
    ValueError where the degrees cannot hold the shape."""
    m0 = m - rank_deficit
    if not (0 < m0 <= n and rank_deficit <= m0 and 1 <= dv_min <= dv_max and 1 <= dc_min <= dc_max):
        raise ValueError("shape / degrees / rank deficit do not fit")
    rng = np.random.default_rng(seed)
    A = np.zeros((m0, n), dtype=np.uint8)
    rdeg = np.zeros(m0, dtype=np.int64)
    cdeg = np.zeros(n, dtype=np.int64)
    piv = rng.permutation(n)[:m0]  # pivot column of row i: row i is its first row
    lo = np.zeros(n, dtype=np.int64)  # rows a column may take: lo[c] .. m0 - 1
    lo[piv] = np.arange(m0)
    A[np.arange(m0), piv] = 1
    rdeg[:] = 1
    cdeg[piv] = 1
    # degree targets: room for the appended sums (they add one to the columns they hold) on most columns
    cap_v = dv_max - 1 if dv_max >= 3 else dv_max
    tgt = rng.integers(dv_min, max(dv_min, cap_v) + 1, size=n)
    emax = int(0.75 * m0 * dc_max) if dc_min < 3 else int(m0 * (dc_min + 0.25))
    emin = m0 * max(dc_min, 2) if dc_min >= 3 else 0
    while tgt.sum() > max(emax, n * dv_min):
        j = rng.integers(n)
        if tgt[j] > max(dv_min, 1):
            tgt[j] -= 1
    while tgt.sum() < emin:
        j = rng.integers(n)
        if tgt[j] < dv_max:
            tgt[j] += 1
    for c in rng.permutation(n):
        want = int(tgt[c] - cdeg[c])
        if want <= 0:
            continue
        rows = np.arange(lo[c], m0)
        rows = rows[(rdeg[rows] < dc_max) & (A[rows, c] == 0)]
        if rows.size == 0:
            continue
        w = (dc_max - rdeg[rows]).astype(np.float64) ** 2
        take = rng.choice(rows, size=min(want, rows.size), replace=False, p=w / w.sum())
        A[take, c] = 1
        rdeg[take] += 1
        cdeg[c] += take.size

    def add_to_row(r, limit):  # columns r may take (pivot rule) that still have room
        cand = np.where((lo <= r) & (A[r] == 0) & (cdeg < limit))[0]
        if cand.size == 0:
            return False
        c = int(rng.choice(cand))
        A[r, c] = 1
        rdeg[r] += 1
        cdeg[c] += 1
        return True

    for r in np.where(rdeg < dc_min)[0]:
        while rdeg[r] < dc_min:
            if not add_to_row(r, cap_v) and not add_to_row(r, dv_max):
                raise ValueError("row degree floor not reachable")
    for c in np.where(cdeg < dv_min)[0]:
        while cdeg[c] < dv_min:
            rows = np.where((np.arange(m0) >= lo[c]) & (A[:, c] == 0) & (rdeg < dc_max))[0]
            if rows.size == 0:
                raise ValueError("column degree floor not reachable")
            r = int(rng.choice(rows))
            A[r, c] = 1
            rdeg[r] += 1
            cdeg[c] += 1
    # exact maxima: a full row grows to dc_max (rows may take the pivot columns of rows at or above them only), the
    # fullest column to dv_max
    if rdeg.max() < dc_max:
        room = np.array([np.count_nonzero((lo <= r) & (A[r] == 0) & (cdeg < dv_max)) for r in range(m0)])
        ok = np.where((room >= dc_max - rdeg) & (rdeg > 2))[0]
        if ok.size == 0:
            raise ValueError("check degree dc_max not reachable")
        r = int(ok[np.argmax(rdeg[ok])])
        while rdeg[r] < dc_max:
            add_to_row(r, dv_max)
    c = int(max(np.where(cdeg < dv_max)[0], key=lambda j: (cdeg[j], -lo[j]), default=-1)) if cdeg.max() < dv_max else -1
    if c >= 0:
        while cdeg[c] < dv_max:
            rows = np.where((np.arange(m0) >= lo[c]) & (A[:, c] == 0) & (rdeg < dc_max))[0]
            if rows.size == 0:
                raise ValueError("bit degree dv_max not reachable")
            rr = int(rng.choice(rows))
            A[rr, c] = 1
            rdeg[rr] += 1
            cdeg[c] += 1
    # a row of degree <= 2 keeps every bp_class_kernel degree class out (unless the caller asks for dc_min >= 3)
    if dc_min <= 2 and rdeg.min() > 2:
        r = int(np.argmin(rdeg))
        for c in rng.permutation(np.where(A[r])[0]):
            if rdeg[r] > 2 and c != piv[r] and dv_min < cdeg[c] < dv_max:
                A[r, c] = 0
                rdeg[r] -= 1
                cdeg[c] -= 1
        if rdeg[r] > 2:
            raise ValueError("no row of degree <= 2")
    # appended rows: sums of two rows -- first pairs that share a column (the sum drops it), then any pair -- within the
    # degree bounds, no pair twice
    H = np.zeros((m, n), dtype=np.uint8)
    H[:m0] = A
    pairs = set()

    def pair_candidates():
        for c in rng.permutation(np.where(cdeg >= 2)[0]):
            rows = np.where(A[:, c])[0]
            if rows.size >= 2:
                yield tuple(sorted(int(x) for x in rng.choice(rows, size=2, replace=False)))
        for _ in range(20 * m0):
            yield tuple(sorted(int(x) for x in rng.choice(m0, size=2, replace=False)))

    for k in range(rank_deficit):
        for a, b in pair_candidates():
            s = A[a] ^ A[b]
            d = int(s.sum())
            if (a, b) in pairs or not (dc_min <= d <= dc_max) or (cdeg[s.astype(bool)] >= dv_max).any():
                continue
            H[m0 + k] = s
            cdeg += s
            pairs.add((a, b))
            break
        else:
            raise ValueError("no pair of rows sums within the degree bounds")
    perm = rng.permutation(m)  # the appended rows anywhere, not only at the bottom
    out = sp.csr_matrix(H[perm])
    out.sort_indices()
    return out


def class_pcm(m, n, rank_deficit=1, seed=0):
    """Surface-code degree class of bp_class_kernel: check degrees 3..4, bit degrees 1..2 (kClassShapes (3, 4, 1, 2))."""
    return edge_pcm(m, n, 4, 2, rank_deficit, seed, dc_min=3)


def pcm_for(case):
    """The matrix of one EDGES row."""
    if case.get("family") == "class":
        return class_pcm(case["m"], case["n"], case["deficit"], case["seed"])
    return edge_pcm(case["m"], case["n"], case["dc"], case["dv"], case["deficit"], case["seed"])


# ------------------------------------------------------------------------------------------------ the edge table
# One row per (instance, edge).  Keys: id, m, n, dc, dv (maximum degrees), deficit (rank deficit), seed, method, order
# ("kprime": the number of non-pivot columns n - rank, which is n - m + deficit), osd_variant (bposd_set_osd_variant),
# bp / osd (the instance last_instance() must report: name and template integers), and optionally family ("class"),
# shots ((H e, uniformly random) syndrome counts; every case also decodes the all-zero and the all-ones syndrome; default
# (95, 32), fewer where the oracle takes seconds per shot: the HBM path, osd_e 20), batch (a large batch for auto
# selection: the H e count grows to fill it), probs ("channel": per-bit probabilities, fp64 candidate weights), bit_order
# (osd_e_bit_order), schedule, bp_variant (bposd_set_bp_variant), packed (also decode through the packed host API and
# compare).
def _bpk(dc, dv, shape=1):
    return ("bp_kernel", (dc, dv) + {1: (1, 1024), 2: (2, 512), 8: (2, 1024)}[shape])


def _m_for(n):  # rows of the osd_kernel width cases: a rate-1/2-ish code, at most 1024 checks
    return min(1024, max(24, (n + 1) // 2))


EDGES = []


def _add(**kw):
    kw.setdefault("deficit", 3)
    kw.setdefault("seed", len(EDGES) + 1)
    kw.setdefault("dc", 8)
    kw.setdefault("dv", 4)
    kw.setdefault("method", "osd_cs")
    kw.setdefault("order", 6)
    kw.setdefault("osd_variant", 1)
    EDGES.append(kw)


# osd_kernel<W> (variant 1): the last n of each width (n = 64 W - 1, the syndrome bit right next to the last column) and
# the first n of the next one
for n_ in (63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 1535, 1536, 1983, 1984, 2047):
    W_ = osd_words(n_)
    last = n_ == 64 * W_ - 1
    _add(id=f"osd_kernel_W{W_}_n{n_}", m=_m_for(n_), n=n_, bp=_bpk(8, 4), osd=("osd_kernel", (W_,)),
         method="osd_cs" if n_ % 2 else "osd_e", order=6 if n_ % 2 else 5, packed=last)
# osd_kernel rows: one vs two waves, five vs six waves, eight waves with row 1023; the panel row buffer over the sort keys
# (rows <= nsort / 2) or in an LDS region of its own (osd_rowbuf_extra)
for m_, n_ in ((128, 255), (129, 255), (640, 1535), (641, 1535), (1024, 2047), (256, 511), (257, 511), (512, 1023), (513, 1023)):
    _add(id=f"osd_kernel_rows_m{m_}_n{n_}", m=m_, n=n_, bp=_bpk(8, 4), osd=("osd_kernel", (osd_words(n_),)),
         method="osd_e", order=4, deficit=5)
# osd_wave_kernel (variant 2): each corner, one past it in m and in n
_WAVE = ((64, 127, (1, 2)), (128, 255, (2, 4)), (192, 447, (3, 7)), (320, 639, (5, 10)))
for i_, (m_, n_, t_) in enumerate(_WAVE):
    _add(id=f"osd_wave_{t_[0]}x{t_[1]}_corner_m{m_}_n{n_}", m=m_, n=n_, bp=_bpk(8, 4), osd=("osd_wave_kernel", t_),
         osd_variant=2, packed=True)
    nxt_m = _WAVE[i_ + 1][2] if i_ + 1 < len(_WAVE) else None
    for dm, dn in ((1, 0), (0, 1)):
        m2, n2 = m_ + dm, n_ + dn
        if nxt_m and m2 <= _WAVE[i_ + 1][0] and n2 + 1 <= _WAVE[i_ + 1][1] + 1:
            want = ("osd_wave_kernel", nxt_m)
        else:
            want = ("osd_mw_kernel", (2, 4, 15, 3))  # past the last corner: the mw kernel's shape 1
        _add(id=f"osd_wave_{t_[0]}x{t_[1]}_past_m{m2}_n{n2}", m=m2, n=n2, bp=_bpk(8, 4), osd=want, osd_variant=2)
# osd_mw_kernel: shape 1 (auto with a large batch, and variant 2), shapes 2 and 3 at their corners (variant 2)
_add(id="osd_mw_shape1_m321_n700", m=321, n=700, bp=_bpk(8, 4), osd=("osd_mw_kernel", (2, 4, 15, 3)), osd_variant=2)
_add(id="osd_mw_shape1_m512_n959_auto", m=512, n=959, bp=_bpk(8, 4), osd=("osd_mw_kernel", (2, 4, 15, 3)),
     osd_variant=0, batch=2048)
_add(id="osd_mw_shape1_m512_n959_v2", m=512, n=959, bp=_bpk(8, 4), osd=("osd_mw_kernel", (2, 4, 15, 3)),
     osd_variant=2, packed=True)
_add(id="osd_mw_shape2_m768_n1279", m=768, n=1279, bp=_bpk(8, 4), osd=("osd_mw_kernel", (4, 3, 20, 2)), osd_variant=2,
     packed=True)
_add(id="osd_mw_shape3_m1024_n1983", m=1024, n=1983, bp=_bpk(8, 4), osd=("osd_mw_kernel", (8, 2, 31, 2)), osd_variant=2,
     packed=True)
# HBM path (osd_large_kernel<RPT>): m just past 1024, n just past 2047 with BP in LDS, the RPT switches, the W edge at
# n = 4095 / 4096 / 4097 (sort size 4096 -> 8192)
_FEW = dict(shots=(7, 2))
_add(id="large_m1025_n2040", m=1025, n=2040, bp=_bpk(8, 4, 8), osd=("osd_large_kernel", (2,)), order=6, **_FEW)
_add(id="large_n2048_m1000", m=1000, n=2048, bp=_bpk(8, 4), osd=("osd_large_kernel", (2,)), method="osd_e", order=5,
     packed=True, **_FEW)
_add(id="large_rpt2_m2048", m=2048, n=2200, bp=_bpk(8, 4, 8), osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="large_rpt4_m2049", m=2049, n=2200, bp=("bp_large_kernel", (12, 6, 2)), osd=("osd_large_kernel", (4,)), **_FEW)
_add(id="large_rpt4_m4096", m=4096, n=4200, bp=("bp_large_kernel", (12, 6, 2)), osd=("osd_large_kernel", (4,)),
     packed=True, **_FEW)
_add(id="large_rpt8_m4097", m=4097, n=4200, bp=("bp_large_kernel", (12, 6, 2)), osd=("osd_large_kernel", (8,)),
     packed=True, **_FEW)
for n_ in (4095, 4096, 4097):
    _add(id=f"large_n{n_}", m=1800, n=n_, bp=_bpk(8, 4, 8) if n_ <= 4096 else ("bp_large_kernel", (12, 6, 2)),
         osd=("osd_large_kernel", (2,)), method="osd_e", order=4, packed=n_ == 4097, **_FEW)
# BP: every bp_kernel pair at its top degrees; beyond them bp_anydeg_kernel
for dc_, dv_ in BP_PAIRS:
    _add(id=f"bp_pair_{dc_}_{dv_}", m=300, n=620, dc=dc_, dv=dv_, bp=_bpk(dc_, dv_), osd=("osd_kernel", (16,)))
_add(id="bp_anydeg_dc17", m=300, n=620, dc=17, dv=8, bp=("bp_anydeg_kernel", ()), osd=("osd_kernel", (16,)))
_add(id="bp_anydeg_dv9", m=300, n=620, dc=16, dv=9, bp=("bp_anydeg_kernel", ()), osd=("osd_kernel", (16,)))
# BP shapes: 1 up to 1024 checks / 2048 bits, 8 beyond (2 checks per thread, stride MP = 2048) where the messages fit one
# CU's LDS -- bp_lds_bytes(8, 2048) fits, bp_lds_bytes(12, 2048) does not: the check degree edge of shape 8 is 8 / 9
_add(id="bp_shape1_m1024_n2048_dc16", m=1024, n=2048, dc=16, dv=8, bp=_bpk(16, 8), osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_shape8_m1024_n2049_dc6", m=1024, n=2049, dc=6, dv=3, bp=_bpk(6, 3, 8), osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_hbm_m1024_n2049_dc16", m=1024, n=2049, dc=16, dv=8, bp=("bp_large_kernel", (16, 8, 2)),
     osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_shape8_m1025_dc6", m=1025, n=2000, dc=6, dv=3, bp=_bpk(6, 3, 8), osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_shape8_m1025_dc8", m=1025, n=2000, dc=8, dv=4, bp=_bpk(8, 4, 8), osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_hbm_m1025_dc9", m=1025, n=2000, dc=9, dv=4, bp=("bp_large_kernel", (12, 6, 2)),
     osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_shape8_m2048_dc6", m=2048, n=2400, dc=6, dv=3, bp=_bpk(6, 3, 8), osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_hbm_m2049_dv6", m=2049, n=2400, dc=12, dv=6, bp=("bp_large_kernel", (12, 6, 2)),
     osd=("osd_large_kernel", (4,)), **_FEW)
_add(id="bp_hbm_m2049_dv7", m=2049, n=2400, dc=12, dv=7, bp=("bp_large_kernel", (16, 8, 2)),
     osd=("osd_large_kernel", (4,)), **_FEW)
# bp_class_kernel, surface-code class: one case per LDS stride 256 / 512 / 1024.  The stride is the first of 256, 512,
# 1024 for which class_layout::build's annealing search places every check and bit; that search, not a capacity formula,
# decides where the stride changes, and it is no monotone function of m -- so these cases pin one matrix per stride
# (tests/test_edge_codes_cpu.py asserts the stride bposd_debug_class_layout finds for each), not a window edge
for m_, mp_ in ((170, 256), (180, 512), (400, 1024)):
    _add(id=f"bp_class_mp{mp_}_m{m_}", family="class", m=m_, n=int(m_ * 2.6), dc=4, dv=2, seed=1,
         bp=("bp_class_kernel", (3, 4, 2, mp_)), osd=("osd_kernel", (osd_words(int(m_ * 2.6)),)))
# bp_kernel shape 2 (two checks per thread, at most 512 threads) is taken by (6,3)-regular codes or on request
# (bposd_set_bp_variant(2)): its last m and n, and one bit past them, where the request falls back to shape 8
_add(id="bp_shape2_m1024_n2048_variant2", m=1024, n=2048, dc=8, dv=4, bp_variant=2, bp=_bpk(8, 4, 2),
     osd=("osd_large_kernel", (2,)), **_FEW)
_add(id="bp_shape2_past_n2049_variant2", m=1024, n=2049, dc=8, dv=4, bp_variant=2, bp=_bpk(8, 4, 8),
     osd=("osd_large_kernel", (2,)), **_FEW)
# bp_serial_kernel at its highest bit degree (BPS_MAXDV = 8)
_add(id="bp_serial_dv8", m=300, n=620, dc=16, dv=8, schedule="serial", bp=("bp_serial_kernel", ()),
     osd=("osd_kernel", (16,)))
# orders: osd_e 13 / 16 / 20 on osd_kernel (integer and fp64 candidate weights, both enumeration bit orders)
for e_ in (13, 16, 20):
    for probs_ in ("uniform", "channel"):
        for bo_ in (0, 1):
            _add(id=f"osd_e{e_}_{probs_}_bitorder{bo_}", m=120, n=250, bp=_bpk(8, 4), osd=("osd_kernel", (4,)),
                 method="osd_e", order=e_, probs=probs_, bit_order=bo_, shots=(29, 2) if e_ == 20 else None)
# osd_e 12 stays on the wave kernel under variant 2, 13 goes to osd_kernel
_add(id="osd_e12_wave", m=100, n=200, bp=_bpk(8, 4), osd=("osd_wave_kernel", (2, 4)), method="osd_e", order=12,
     osd_variant=2)
_add(id="osd_e13_variant2_osd_kernel", m=100, n=200, bp=_bpk(8, 4), osd=("osd_kernel", (4,)), method="osd_e", order=13,
     osd_variant=2)
# osd_order == k' (the candidate span reaches the last non-pivot column), both methods, on every OSD family
_add(id="kprime_osd_e_osd_kernel", m=200, n=215, bp=_bpk(8, 4), osd=("osd_kernel", (4,)), method="osd_e",
     order="kprime", deficit=3, shots=(63, 8))  # k' = 18
_add(id="kprime_osd_e_wave", m=120, n=130, bp=_bpk(8, 4), osd=("osd_wave_kernel", (2, 4)), method="osd_e",
     order="kprime", deficit=2, osd_variant=2)  # k' = 12 (the wave kernels stop at 12)
_add(id="kprime_osd_e_mw", m=500, n=508, bp=_bpk(8, 4), osd=("osd_mw_kernel", (2, 4, 15, 3)), method="osd_e",
     order="kprime", deficit=4, osd_variant=2)  # k' = 12
_add(id="kprime_osd_e_large", m=1100, n=1113, bp=_bpk(8, 4, 8), osd=("osd_large_kernel", (2,)), method="osd_e",
     order="kprime", deficit=3, shots=(29, 2))  # k' = 16 (33 shots: the oracle's threads share them)
_add(id="kprime64_osd_cs_osd_kernel", m=400, n=460, bp=_bpk(8, 4), osd=("osd_kernel", (8,)), method="osd_cs",
     order="kprime", deficit=4)  # k' = 64
_add(id="kprime5_osd_cs_osd_kernel", m=300, n=302, bp=_bpk(8, 4), osd=("osd_kernel", (8,)), method="osd_cs",
     order="kprime", deficit=3)  # k' = 5
_add(id="kprime64_osd_cs_wave", m=250, n=310, bp=_bpk(8, 4), osd=("osd_wave_kernel", (5, 10)), method="osd_cs",
     order="kprime", deficit=4, osd_variant=2)  # k' = 64
_add(id="kprime5_osd_cs_wave", m=60, n=63, bp=_bpk(8, 4), osd=("osd_wave_kernel", (1, 2)), method="osd_cs",
     order="kprime", deficit=2, osd_variant=2)  # k' = 5
_add(id="kprime64_osd_cs_mw", m=700, n=760, bp=_bpk(8, 4), osd=("osd_mw_kernel", (4, 3, 20, 2)), method="osd_cs",
     order="kprime", deficit=4, osd_variant=2)  # k' = 64
_add(id="kprime5_osd_cs_mw", m=480, n=482, bp=_bpk(8, 4), osd=("osd_mw_kernel", (2, 4, 15, 3)), method="osd_cs",
     order="kprime", deficit=3, osd_variant=2)  # k' = 5
_add(id="kprime64_osd_cs_large", m=1100, n=1160, bp=_bpk(8, 4, 8), osd=("osd_large_kernel", (2,)), method="osd_cs",
     order="kprime", deficit=4, **_FEW)  # k' = 64
_add(id="kprime5_osd_cs_large", m=1100, n=1102, bp=_bpk(8, 4, 8), osd=("osd_large_kernel", (2,)), method="osd_cs",
     order="kprime", deficit=3, **_FEW)  # k' = 5


def kprime(case):
    return case["n"] - case["m"] + case["deficit"]


def order_of(case):
    return kprime(case) if case["order"] == "kprime" else case["order"]


# ----------------------------------------------------------------------------------- the product-sum table (PS_EDGES)
# Every BP kernel family is compiled three times per instance (METHOD 1 min-sum, 2 product-sum in the reference's operation
# order, 0 product-sum with two divisions per edge) or switches on ps_form at run time; EDGES runs min-sum only.  One row
# here per BP instance that product-sum must reach (tests/test_gpu_ps_edges.py; tests/test_ps_edges_cpu.py keeps the table
# honest without a GPU).  Keys: id; edge (the id of the EDGES row whose matrix and expected instance the row reuses) or code
# (a construction of PS_CODES); bp (the instance last_instance() must report; bp_large_kernel runs its METHOD 0 for either
# product-sum form); bp_variant / schedule; seed and shots as in EDGES (48 syndromes by default, 11 where m > 1024 or the
# EDGES row has as few); deg1 / deg2 (the number of checks of degree 1 and 2: a degree-1 check sends log(2 / 0) = +-inf
# without a clip); sat12 (the unclipped max_iter = 12 runs must saturate at least one shot to +-inf: every generic matrix);
# extras (the further runs of the row: "channel" per-bit probabilities, "select" the per-shot two-valued channel, "packed"
# the packed host API); stride (class rows: the LDS stride the layout search settles on).
EDGE_BY_ID = {c["id"]: c for c in EDGES}
PS_SHOTS = (38, 8)  # + the all-zero and the all-ones syndrome: 48
PS_ERROR_RATE = 0.08
PS_EXCLUDED_CAP = 1.0 / 8.0  # share of a case's shots whose LLRs may mix numbers and NaN (no defined OSD order)
PS_EDGES = []


def _ps(id=None, edge=None, **kw):
    if edge is not None:
        e = EDGE_BY_ID[edge]
        kw.setdefault("bp", e["bp"] if e["bp"][0] != "bp_large_kernel" else ("bp_large_kernel", e["bp"][1][:2] + (0,)))
        kw.setdefault("seed", e["seed"])
        kw.setdefault("shots", e.get("shots") or PS_SHOTS)
        for k in ("bp_variant", "schedule"):
            if k in e:
                kw.setdefault(k, e[k])
        kw.setdefault("sat12", True)
    kw.setdefault("seed", len(PS_EDGES) + 1)
    kw.setdefault("shots", PS_SHOTS)
    kw.setdefault("sat12", False)
    kw.setdefault("extras", ())
    kw.setdefault("deg1", 0)
    kw.setdefault("deg2", 0)
    PS_EDGES.append(dict(id=id or edge, edge=edge, **kw))


def _golden(name):
    import os

    return np.loadtxt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)).astype(np.uint8)


def _code(name):
    from bp_osd_amd.codes import h1922, hgp, regular_ldpc_seed, ring_code

    if name == "h1922_hz":  # (3,6)-regular, 961 x 1922: the REG instances of bp_kernel
        return h1922(compute_logicals=False).hz
    if name == "hgp400_hz":  # the reference's example code: check degree 7, bit degrees 3..4
        return hgp(_golden("mkmn_16_4_6.txt"), compute_logicals=False).hz
    if name == "reg36_m120":  # (3,6)-regular, small: the (6; 3) class below stride 1024
        return sp.csr_matrix(regular_ldpc_seed(120, 240, 3, 6, seed=11))
    if name == "toric12_hx":  # (4; 2)
        return hgp(ring_code(12), compute_logicals=False).hx
    if name == "reg44_hx":  # (8; 4)
        return hgp(regular_ldpc_seed(12, 12, 4, 4, seed=3), compute_logicals=False).hx
    raise KeyError(name)


def ps_pcm(row):
    """The matrix of one PS_EDGES row (scipy CSR, uint8, sorted indices)."""
    H = pcm_for(EDGE_BY_ID[row["edge"]]) if row["edge"] else _code(row["code"])
    H = sp.csr_matrix(H, dtype=np.uint8)
    H.sort_indices()
    return H


# bp_kernel shape 1: every degree pair, and the largest matrix of the shape
_ps(edge="bp_pair_4_2", deg1=1, deg2=57, extras=("channel",))
_ps(edge="bp_pair_6_3", deg1=16, deg2=74)
_ps(edge="bp_pair_8_4", deg2=15, extras=("channel", "select", "packed"))
_ps(edge="bp_pair_12_6", deg2=3)
_ps(edge="bp_pair_16_8", deg2=1)
_ps(edge="bp_shape1_m1024_n2048_dc16", deg2=1)
# shape 2 (on request) and shape 8
_ps(edge="bp_shape2_m1024_n2048_variant2", deg1=12, deg2=95)
_ps(edge="bp_shape8_m1025_dc6", deg1=59, deg2=284)
_ps(edge="bp_shape8_m1025_dc8", deg1=22, deg2=97, extras=("channel", "packed"))
_ps(edge="bp_shape8_m2048_dc6", deg1=917, deg2=780)
# bp_kernel<6, 3, REG> at shapes 1, 2 and 4: product-sum on a (3,6)-regular code of stride 1024 stays on bp_kernel
for v_, t_ in ((1, (1, 1024)), (0, (2, 512)), (4, (4, 256))):
    _ps(id=f"bp_reg63_h1922_variant{v_}", code="h1922_hz", bp=("bp_kernel", (6, 3) + t_), bp_variant=v_, seed=20 + v_,
        shots=(20, 2), sat12=True, extras=("channel", "select", "packed") if v_ == 0 else ())
# bp_class_kernel: the surface-code class at its three strides, then one code per other degree class
_ps(edge="bp_class_mp256_m170", stride=256, sat12=False)
_ps(edge="bp_class_mp512_m180", stride=512, sat12=False, extras=("channel", "select", "packed"))
_ps(edge="bp_class_mp1024_m400", stride=1024, sat12=False)
_ps(id="bp_class_7_hgp400", code="hgp400_hz", bp=("bp_class_kernel", (7, 7, 4, 256)), stride=256, seed=31, sat12=True, extras=("channel",))
_ps(id="bp_class_6_reg36_m120", code="reg36_m120", bp=("bp_class_kernel", (6, 6, 3, 256)), stride=256, seed=32)
_ps(id="bp_class_4_toric12", code="toric12_hx", bp=("bp_class_kernel", (4, 4, 2, 256)), stride=256, seed=33)
_ps(id="bp_class_8_reg44", code="reg44_hx", bp=("bp_class_kernel", (8, 8, 4, 256)), stride=256, seed=34, sat12=True)
# bp_large_kernel<12, 6, 0> and <16, 8, 0>
_ps(edge="bp_hbm_m1025_dc9", deg1=20, deg2=132, extras=("channel", "select", "packed"))
_ps(edge="bp_hbm_m2049_dv6", deg1=292, deg2=436)
_ps(edge="bp_hbm_m1024_n2049_dc16", deg1=1, deg2=1)
_ps(edge="bp_hbm_m2049_dv7", deg1=201, deg2=379, extras=("channel", "packed"))
# the kernels that switch on ps_form at run time
_ps(edge="bp_serial_dv8", deg2=1, extras=("channel", "select"))
_ps(edge="bp_anydeg_dc17", deg2=1, extras=("channel", "select"))
_ps(edge="bp_anydeg_dv9", deg2=1)


def ps_cases(row):
    """The runs of one row: dicts with form (ps_math_form; the oracle's ps_math is 2 - form), clip, max_iter, kind ("uniform",
    "channel", "select", "packed").  Uniform channel: both forms x {no clip, one finite clip} x {a short max_iter, so that
    most shots reach OSD; 12, so that saturation shows}.  The extras: both forms at (clip, 12) and (no clip, short)."""
    clip = (8.0, 20.0, 37.0)[row["seed"] % 3]
    short = 1 + row["seed"] % 3
    out = [dict(form=f, clip=c, max_iter=it, kind="uniform") for f in (0, 1) for c in (0.0, clip) for it in (short, 12)]
    for kind in row["extras"]:
        out += [dict(form=f, clip=c, max_iter=it, kind=kind) for f in (0, 1) for c, it in ((clip, 12), (0.0, short))]
    return out


def ps_case_id(case):
    return f"{case['kind']}-form{case['form']}-clip{case['clip']:g}-it{case['max_iter']}"


def ps_settings(row, case, n):
    """Decoder keywords of one run (without ps_math_form / ps_math, which differ between the library and the oracle) and the
    per-shot channel (select, alt) of a "select" run, else (None, None)."""
    kw = dict(max_iter=case["max_iter"], bp_method="ps", ps_clip=case["clip"], osd_method="osd_cs", osd_order=6)
    rng = np.random.default_rng(7000 + row["seed"])
    if case["kind"] == "channel":
        kw["channel_probs"] = rng.uniform(0.03, 0.15, size=n)
    else:
        kw["error_rate"] = PS_ERROR_RATE
    if row.get("schedule"):
        kw["schedule"] = row["schedule"]
    return kw


def ps_select(row, B, n):
    """The per-shot two-valued channel of a "select" run: (prior_select [B, n], alt_channel_probs [n])."""
    rng = np.random.default_rng(8000 + row["seed"])
    return (rng.random((B, n)) < 0.2).astype(np.uint8), rng.uniform(0.02, 0.3, size=n)


def ps_oracle_select(o, syn, sel, alt):
    """The oracle with a per-shot two-valued channel: update_channel_probs, then decode, shot by shot (what the reference
    harness does, css_decode_sim.py:207-248)."""
    base = o._probs.copy()
    outs = []
    for b in range(len(syn)):
        o.update_channel_probs(np.where(sel[b] != 0, alt, base))
        outs.append(o.decode_batch(syn[b:b + 1]))
    o.update_channel_probs(base)
    return {k: np.concatenate([r[k] for r in outs]) for k in outs[0]}


def ps_oracle_conditions(row, case, ref, syn):
    """What the ORACLE's output of one run must show for the run to test anything (asserted with and without a GPU, so a
    drift of the inputs fails here): the share of shots whose LLRs mix numbers and NaN stays within PS_EXCLUDED_CAP (none
    with a clip); with a clip every LLR is finite; without one, a matrix with a degree-1 check has +-inf in every shot BP
    ran on and the max_iter = 12 runs of the generic matrices in at least one; a short max_iter leaves more than half the
    shots unconverged.  Returns the mask of the excluded shots."""
    llr = ref["llr"]
    nan = np.isnan(llr)
    mixed = nan.any(axis=1) & ~nan.all(axis=1)
    assert mixed.mean() <= PS_EXCLUDED_CAP, f"{mixed.sum()} of {len(mixed)} shots mix numbers and NaN"
    if case["clip"] > 0:
        assert not mixed.any() and np.isfinite(llr).all(), "a clipped run is not finite"
    else:
        inf = np.isinf(llr).any(axis=1)
        ran = syn.any(axis=1)  # (BP does not run on the zero syndrome)
        if row["deg1"]:
            assert inf[ran].all(), "a degree-1 check did not saturate every shot"
        if row["sat12"] and case["max_iter"] == 12:
            assert inf.any(), "no shot saturated"
    if case["max_iter"] < 12:
        assert (np.asarray(ref["converged"]) == 0).mean() > 0.5, "most shots converged"
    return mixed
