"""Circuit-level noise: a detector error model from a Clifford circuit.

A ``Circuit`` is a list of Clifford ops with measurements, detector / observable annotations over the measurements, and
independent elementary Pauli faults at positions between the ops.  Every fault is propagated on its own through the rest
of the circuit as a Pauli frame; the detectors and observables it flips are its column of ``H`` and ``L``.  ``circuit_dem``
reduces the columns to a model ``(H, L, priors, detector_time, origin)`` that goes straight into ``dem_decode_sim``,
``windowed_dem_decode_sim``, ``dem_failure_spectrum`` and ``fit_sample_priors``.

The frame rule is the definition, and both engines follow it bit for bit.  A frame is one ``(x, z)`` bit pair per qubit,
all zero at the start:

    H    swap x, z                          S    z ^= x
    CX   x[b] ^= x[a];  z[a] ^= z[b]        CZ   z[a] ^= x[b];  z[b] ^= x[a]
    R, RX   clear both bits                 M / MX   record the flip x[a] / z[a], frame unchanged
    MR, MRX record the flip as M / MX, then clear

``engine="native"`` runs the propagation in libbposd_mi355x.so (bposd_frame_* of include/bposd_mi355x.h): 64 faults to a
machine word, one GPU thread per word.  ``engine="numpy"`` is the same propagation on the host with bit-packed uint64
arrays and one vectorised update per op; it is what the device is held to.  The reduction runs on the host and is the same
for both.

``css_memory_circuit`` builds the memory experiment of any CSS code, so the whole path starts from ``bp_osd_amd.codes``.
No file format is parsed; ``dem_text`` writes a model in the text format INTEGRATION.md describes.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import numpy as np
import scipy.sparse as sp

__all__ = ["OPCODES", "Circuit", "Faults", "make_faults", "FramePropagator", "fault_columns", "circuit_dem", "check_annotations", "css_memory_circuit",
           "dem_text", "greedy_edge_colouring"]

OPCODES = {"R": 0, "RX": 1, "M": 2, "MX": 3, "MR": 4, "MRX": 5, "H": 6, "S": 7, "CX": 8, "CZ": 9}
_R, _RX, _M, _MX, _MR, _MRX, _H, _S, _CX, _CZ = range(10)
_MEASURES = (_M, _MX, _MR, _MRX)
_TWO_QUBIT = (_CX, _CZ)
PAULI_X, PAULI_Z, PAULI_Y = 1, 2, 3


class Faults(NamedTuple):
    """Elementary faults, sorted by ``pos``: fault i is Pauli ``pa[i]`` on qubit ``qa[i]`` (and ``pb[i]`` on ``qb[i]`` unless
    that is -1) in front of op ``pos[i]``, with probability ``prob[i]``."""
    pos: np.ndarray
    qa: np.ndarray
    pa: np.ndarray
    qb: np.ndarray
    pb: np.ndarray
    prob: np.ndarray

    def __len__(self):  # (a NamedTuple's own len would be 6)
        return int(self.pos.shape[0])


def _faults(pos, qa, pa, qb, pb, prob):
    return Faults(np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(qa, np.int32), np.ascontiguousarray(pa, np.uint8),
                  np.ascontiguousarray(qb, np.int32), np.ascontiguousarray(pb, np.uint8), np.ascontiguousarray(prob, np.float64))


def make_faults(pos, qa, pa, qb=None, pb=None, prob=None):
    """``Faults`` from arrays in any order: sorted by ``pos``, ties in the order given."""
    pos = np.asarray(pos, np.int64)
    n = pos.shape[0]
    qb = np.full(n, -1) if qb is None else np.asarray(qb)
    pb = np.zeros(n) if pb is None else np.asarray(pb)
    prob = np.zeros(n) if prob is None else np.asarray(prob)
    order = np.argsort(pos, kind="stable")
    return _faults(pos[order], np.asarray(qa)[order], np.asarray(pa)[order], qb[order], pb[order], prob[order])


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    for i, r in enumerate(rows):
        indptr[i + 1] = indptr[i] + len(r)
    indices = np.fromiter((v for r in rows for v in r), np.int64, int(indptr[-1]))
    return indptr, indices


class Circuit:
    """Plain arrays and nothing clever.  Ops are appended in order; a noise channel appended after an op sits in front of
    the next one.  Qubits never reset are |0> at the start."""

    def __init__(self, num_qubits):
        self.Q = int(num_qubits)
        if self.Q < 1:
            raise ValueError("a circuit needs at least one qubit")
        self._ops = []
        self._n_meas = 0
        self._detectors, self._observables, self._detector_time = [], [], []
        self._faults = []  # (pos, qa, pa, qb, pb, prob) in insertion order
        self._sorted = None

    # ------------------------------------------------------------------------------------------------------------ ops
    def _qubit(self, q):
        q = int(q)
        if not 0 <= q < self.Q:
            raise ValueError(f"qubit {q} is outside [0, {self.Q})")
        return q

    def append(self, name, a, b=0):
        """Append op ``name`` (a key of OPCODES); returns the measurement's index for M, MX, MR, MRX."""
        op = OPCODES[name]
        a = self._qubit(a)
        if op in _TWO_QUBIT:
            b = self._qubit(b)
            if a == b:
                raise ValueError(f"{name} needs two different qubits, not {a} twice")
        else:
            b = 0
        self._ops.append((op, a, b))
        if op in _MEASURES:
            self._n_meas += 1
            return self._n_meas - 1
        return None

    def r(self, q): self.append("R", q)
    def rx(self, q): self.append("RX", q)
    def m(self, q): return self.append("M", q)
    def mx(self, q): return self.append("MX", q)
    def mr(self, q): return self.append("MR", q)
    def mrx(self, q): return self.append("MRX", q)
    def h(self, q): self.append("H", q)
    def s(self, q): self.append("S", q)
    def cx(self, control, target): self.append("CX", control, target)
    def cz(self, a, b): self.append("CZ", a, b)

    # ---------------------------------------------------------------------------------------------------- annotations
    def _meas_list(self, measurements):
        out = [int(v) for v in measurements]
        for v in out:
            if not 0 <= v < self._n_meas:
                raise ValueError(f"measurement {v} is outside [0, {self._n_meas}): annotate after the measurement")
        return out

    def detector(self, measurements, time=0):
        self._detectors.append(self._meas_list(measurements))
        self._detector_time.append(int(time))
        return len(self._detectors) - 1

    def observable(self, measurements):
        self._observables.append(self._meas_list(measurements))
        return len(self._observables) - 1

    # --------------------------------------------------------------------------------------------------------- faults
    def fault(self, prob, qa, pa, qb=-1, pb=0, pos=None):
        """One elementary fault in front of op ``pos`` (default: in front of the next op appended).  An identity factor
        of a pair is dropped, so that ``pa`` is never 0."""
        pos = len(self._ops) if pos is None else int(pos)
        pa, pb = int(pa), int(pb)
        if not 0 <= pa <= 3 or not 0 <= pb <= 3:
            raise ValueError("a Pauli code is 0 .. 3 (bit 0 the X part, bit 1 the Z part)")
        qa = self._qubit(qa)
        qb = -1 if int(qb) == -1 else self._qubit(qb)
        if qb == qa:
            raise ValueError(f"a two-qubit fault needs two different qubits, not {qa} twice")
        if qb >= 0 and pa == 0:
            qa, pa, qb, pb = qb, pb, -1, 0
        if qb == -1 or pb == 0:
            qb, pb = -1, 0
        if pa == 0:
            raise ValueError("the identity is no fault")
        if pos < 0:
            raise ValueError("pos must not be negative")
        prob = float(prob)
        if not 0.0 <= prob <= 1.0:
            raise ValueError(f"probability {prob} is outside [0, 1]")
        self._faults.append((pos, qa, pa, qb, pb, prob))
        self._sorted = None

    def x_error(self, p, q):
        if p > 0:
            self.fault(p, q, PAULI_X)

    def z_error(self, p, q):
        if p > 0:
            self.fault(p, q, PAULI_Z)

    def depolarize1(self, p, q):
        """X, Y, Z as three independent mechanisms whose composition gives each of them net probability p / 3."""
        if p > 0.75:
            raise ValueError(f"depolarize1: p = {p} is above 3/4")
        if p > 0:
            e = depolarize1_mechanism(p)
            for pauli in (1, 2, 3):
                self.fault(e, q, pauli)

    def depolarize2(self, p, a, b):
        """The 15 non-identity pairs as independent mechanisms whose composition gives each of them net probability p / 15."""
        if p > 15.0 / 16.0:
            raise ValueError(f"depolarize2: p = {p} is above 15/16")
        if p > 0:
            e = depolarize2_mechanism(p)
            for code in range(1, 16):
                self.fault(e, a, code & 3, b, code >> 2)

    # ----------------------------------------------------------------------------------------------------- the arrays
    @property
    def T(self):
        return len(self._ops)

    @property
    def ops(self):
        return np.asarray(self._ops, np.int32).reshape(len(self._ops), 3)

    @property
    def num_measurements(self):
        return self._n_meas

    @property
    def num_detectors(self):
        return len(self._detectors)

    @property
    def num_observables(self):
        return len(self._observables)

    @property
    def detectors(self):
        """CSR over measurement indices, one row per detector: (indptr, indices)."""
        return _csr(self._detectors)

    @property
    def observables(self):
        return _csr(self._observables)

    @property
    def detector_time(self):
        return np.asarray(self._detector_time, np.int64)

    @property
    def faults(self):
        """The faults sorted by (pos, insertion order); that order is the fault index everywhere."""
        if self._sorted is None:
            T = self.T
            for f in self._faults:
                if f[0] > T:
                    raise ValueError(f"a fault sits at pos {f[0]}, behind T = {T}")
            a = self._faults
            order = sorted(range(len(a)), key=lambda i: a[i][0])  # (stable)
            cols = list(zip(*[a[i] for i in order])) if a else [[]] * 6
            self._sorted = _faults(*cols)
        return self._sorted

    def measurement_tables(self):
        """The annotations inverted: CSR over measurements, row i the detectors (the observables) that hold measurement i
        an odd number of times, ascending.  ``(md_indptr, md_indices, mo_indptr, mo_indices)``, int32."""
        out = []
        for rows in (self._detectors, self._observables):
            per = [[] for _ in range(self._n_meas)]
            for d, row in enumerate(rows):
                for v in row:
                    if per[v] and per[v][-1] == d:
                        per[v].pop()  # twice in one row: the flips cancel
                    else:
                        per[v].append(d)
            indptr, indices = _csr(per)
            out += [indptr.astype(np.int32), indices.astype(np.int32)]
        return tuple(out)

    def gauge_faults(self):
        """Faults that act trivially on the state where they sit: Z directly after every R, M, MR, X directly after every RX,
        MX, MRX, and Z at pos 0 on every qubit (the implicit |0> start).  A sound annotation gives each an empty column."""
        rows = [(0, q, PAULI_Z) for q in range(self.Q)]
        for t, (op, a, _) in enumerate(self._ops):
            if op in (_R, _M, _MR):
                rows.append((t + 1, a, PAULI_Z))
            elif op in (_RX, _MX, _MRX):
                rows.append((t + 1, a, PAULI_X))
        rows.sort(key=lambda r: r[0])
        n = len(rows)
        pos, qa, pa = zip(*rows)
        return _faults(pos, qa, pa, np.full(n, -1), np.zeros(n), np.zeros(n))


def depolarize1_mechanism(p):
    return 0.5 - 0.5 * math.sqrt(1.0 - 4.0 * p / 3.0)


def depolarize2_mechanism(p):
    return 0.5 - 0.5 * (1.0 - 16.0 * p / 15.0) ** 0.125


# ------------------------------------------------------------------------------------------------------------- engines
def _columns_from_rows(rows, f_lo, n_faults):
    """Rows [n][nw] uint64 of a chunk whose first fault is f_lo -> (counts [n_faults], indices) of the chunk's columns, each
    column ascending.  Only the non-zero words are looked at."""
    r, w = np.nonzero(rows)
    if r.size == 0:
        return np.zeros(n_faults, np.int64), np.zeros(0, np.int32)
    words = np.ascontiguousarray(rows[r, w], "<u8")
    bits = np.unpackbits(words.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
    i, j = np.nonzero(bits)
    fault = 64 * w[i] + j
    row = r[i]
    if fault.size and int(fault.max()) >= n_faults:
        raise AssertionError("a padding bit of the last word is set")
    order = np.lexsort((row, fault))
    return np.bincount(fault, minlength=n_faults).astype(np.int64), row[order].astype(np.int32)


def _columns_numpy(circuit, fa, max_words=0):
    """The frame rule on bit-packed uint64 arrays, one vectorised update per op: the definition of the device engine."""
    ops, T, Q = circuit.ops, circuit.T, circuit.Q
    M, k = circuit.num_detectors, circuit.num_observables
    md_ptr, md_idx, mo_ptr, mo_idx = circuit.measurement_tables()
    F = len(fa)
    W = (F + 63) // 64
    wc = max(1, min(W, (1 << 28) // (8 * (2 * Q + M + k))))
    if max_words:
        wc = max(1, min(wc, int(max_words)))
    meas_before = np.concatenate([[0], np.cumsum(np.isin(ops[:, 0], _MEASURES))]).astype(np.int64) if T else np.zeros(1, np.int64)
    h_cnt, l_cnt, h_idx, l_idx = [], [], [], []
    one = np.uint64(1)
    for w0 in range(0, W, wc):
        nw = min(wc, W - w0)
        f_lo, f_hi = 64 * w0, min(F, 64 * (w0 + nw))
        n = f_hi - f_lo
        pos = fa.pos[f_lo:f_hi]
        first = np.searchsorted(pos, np.arange(T + 2), side="left")  # faults in front of op t: [first[t], first[t + 1])
        local = np.arange(n)
        word, bit = local >> 6, one << (local & 63).astype(np.uint64)
        x, z = np.zeros((Q, nw), np.uint64), np.zeros((Q, nw), np.uint64)
        D, O = np.zeros((M, nw), np.uint64), np.zeros((k, nw), np.uint64)
        t0 = int(pos[0])
        mi = int(meas_before[min(t0, T)])
        for t in range(t0, T):
            lo, hi = int(first[t]), int(first[t + 1])
            if hi > lo:
                s = slice(lo, hi)
                for arr, q, p, mask in ((x, fa.qa, fa.pa, 1), (z, fa.qa, fa.pa, 2), (x, fa.qb, fa.pb, 1), (z, fa.qb, fa.pb, 2)):
                    sel = ((p[f_lo:f_hi][s] & mask) != 0) & (q[f_lo:f_hi][s] >= 0)
                    if sel.any():
                        np.bitwise_xor.at(arr, (q[f_lo:f_hi][s][sel], word[s][sel]), bit[s][sel])
            wh = (hi + 63) >> 6  # the words behind are still zero
            op, a, b = int(ops[t, 0]), int(ops[t, 1]), int(ops[t, 2])
            if op == _H:
                tmp = x[a, :wh].copy()
                x[a, :wh] = z[a, :wh]
                z[a, :wh] = tmp
            elif op == _S:
                z[a, :wh] ^= x[a, :wh]
            elif op == _CX:
                x[b, :wh] ^= x[a, :wh]
                z[a, :wh] ^= z[b, :wh]
            elif op == _CZ:
                xa = x[a, :wh].copy()
                z[a, :wh] ^= x[b, :wh]
                z[b, :wh] ^= xa
            elif op in (_R, _RX):
                x[a, :wh] = 0
                z[a, :wh] = 0
            else:
                flip = x[a, :wh] if op in (_M, _MR) else z[a, :wh]
                if flip.any():
                    for d in md_idx[md_ptr[mi]:md_ptr[mi + 1]]:
                        D[d, :wh] ^= flip
                    for o in mo_idx[mo_ptr[mi]:mo_ptr[mi + 1]]:
                        O[o, :wh] ^= flip
                mi += 1
                if op in (_MR, _MRX):
                    x[a, :wh] = 0
                    z[a, :wh] = 0
        for rows, cnts, idxs in ((D, h_cnt, h_idx), (O, l_cnt, l_idx)):
            c, i = _columns_from_rows(rows, f_lo, n)
            cnts.append(c)
            idxs.append(i)

    def csc(cnts, idxs):
        cnt = np.concatenate(cnts) if cnts else np.zeros(0, np.int64)
        return (np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), np.concatenate(idxs).astype(np.int32) if idxs else np.zeros(0, np.int32))

    return csc(h_cnt, h_idx) + csc(l_cnt, l_idx)


class FramePropagator:
    """A bposd_frame handle for one circuit: ``columns(faults)`` propagates a fault list on the GPU.  ``max_words`` caps the
    words (of 64 faults) of a chunk; by default a chunk fills ``workspace_bytes`` (0: 1 GiB).  ``layered`` False walks the ops one
    at a time; True (and None, the library's default) takes up to four ops on disjoint qubits per memory round trip."""

    def __init__(self, circuit, max_words=0, workspace_bytes=0, device=0, layered=None):
        from . import _lib

        self._libmod, self.lib, self._h = _lib, _lib.load(), None
        self.M, self.k = circuit.num_detectors, circuit.num_observables
        ops = np.ascontiguousarray(circuit.ops, np.int32)
        tabs = [np.ascontiguousarray(t, np.int32) for t in circuit.measurement_tables()]
        cfg = _lib.BposdFrameConfig(device=int(device), layered=_lib.FRAME_LAYERED[layered], max_words=int(max_words), workspace_bytes=int(workspace_bytes))
        h = C.c_void_p()
        rc = self.lib.bposd_frame_create(C.byref(cfg), ops.ctypes.data, circuit.T, circuit.Q, circuit.num_measurements, tabs[0].ctypes.data,
                                         tabs[1].ctypes.data, tabs[2].ctypes.data, tabs[3].ctypes.data, self.M, self.k, C.byref(h))
        _lib.check_frame(self.lib, None, rc)
        self._h = h

    def columns(self, fa, prefill=None):
        """``(h_indptr, h_indices, l_indptr, l_indices)``: CSC of H and of L over the faults ``fa``.  ``prefill``: a value the
        arrays hold before the library writes them (for tests that want to see every slot written)."""
        F = len(fa)
        pauli = np.ascontiguousarray(fa.pa | (fa.pb << 2), np.uint8)
        nnz = np.zeros(2, np.int64)
        rc = self.lib.bposd_frame_columns(self._h, fa.pos.ctypes.data, fa.qa.ctypes.data, fa.qb.ctypes.data, pauli.ctypes.data, F, nnz.ctypes.data)
        self._libmod.check_frame(self.lib, self._h, rc)
        out = [np.empty(F + 1, np.int64), np.empty(int(nnz[0]), np.int32), np.empty(F + 1, np.int64), np.empty(int(nnz[1]), np.int32)]
        if prefill is not None:
            for a in out:
                a.fill(prefill)
        rc = self.lib.bposd_frame_fetch(self._h, *[a.ctypes.data for a in out])
        self._libmod.check_frame(self.lib, self._h, rc)
        return tuple(out)

    def timing(self):
        """``(propagate_ms, count_ms, fill_ms, chunks, launches)`` of the last ``columns`` (HIP events, summed over chunks)."""
        ms, info = np.zeros(3, np.float64), np.zeros(2, np.int64)
        self._libmod.check_frame(self.lib, self._h, self.lib.bposd_debug_frame_timing(self._h, ms.ctypes.data, info.ctypes.data))
        return float(ms[0]), float(ms[1]), float(ms[2]), int(info[0]), int(info[1])

    def launches(self):
        info = np.zeros(2, np.int64)
        self._libmod.check_frame(self.lib, self._h, self.lib.bposd_debug_frame_timing(self._h, None, info.ctypes.data))
        return int(info[1])

    def device_bytes(self):
        return int(self.lib.bposd_frame_device_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.bposd_frame_destroy(self._h)
            self._h = None

    __del__ = close


def fault_columns(circuit, faults=None, engine="native", max_words=0):
    """CSC of H (detectors) and of L (observables) over the elementary faults (default: the circuit's own), before any
    reduction: ``(h_indptr, h_indices, l_indptr, l_indices)``, every column ascending."""
    fa = circuit.faults if faults is None else faults
    if engine == "numpy":
        return _columns_numpy(circuit, fa, max_words)
    if engine != "native":
        raise ValueError("engine must be 'native' or 'numpy'")
    prop = FramePropagator(circuit, max_words=max_words)
    try:
        return prop.columns(fa)
    finally:
        prop.close()


def check_annotations(circuit, engine="native"):
    """Propagate ``circuit.gauge_faults()`` and raise, naming the first detector or observable that one of them flips: such
    a detector is not deterministic in the noiseless circuit."""
    g = circuit.gauge_faults()
    hp, hi, lp, li = fault_columns(circuit, g, engine)
    for name, ptr, idx in (("detector", hp, hi), ("observable", lp, li)):
        if idx.size:
            f = int(np.searchsorted(ptr, 0, side="right")) - 1  # the first fault with an entry
            pauli = "XZ"[int(g.pa[f]) - 1] if g.pa[f] in (1, 2) else "Y"
            raise ValueError(f"{name} {int(idx[0])} is not deterministic: it is flipped by the gauge fault {pauli} on qubit {int(g.qa[f])} in front of op "
                             f"{int(g.pos[f])}, which acts trivially on the state there")


# ----------------------------------------------------------------------------------------------------------- reduction
def _fold(p1, p2):
    return p1 * (1.0 - p2) + p2 * (1.0 - p1)


def _gather_columns(ptr, idx, cols):
    """(new column, row) of every entry of the CSC columns ``cols``, in that order."""
    n = np.diff(ptr)[cols]
    start = np.concatenate([[0], np.cumsum(n)[:-1]]) if cols.size else np.zeros(0, np.int64)
    within = np.arange(int(n.sum())) - np.repeat(start, n)
    return np.repeat(np.arange(cols.size), n), idx[np.repeat(ptr[cols], n) + within].astype(np.int64)


def _reduce(hp, hi, lp, li, prob, M, k, merge):
    """Columns over the elementary faults -> (H, L, priors, origin_indptr, origin_indices)."""
    F = prob.shape[0]
    hc, lc = np.diff(hp), np.diff(lp)
    cnt = hc + lc
    # the stacked column of fault i: its detectors, then M + its observables
    sp_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    stacked = np.empty(int(sp_ptr[-1]), np.int64)
    h_at = np.repeat(sp_ptr[:-1], hc) + (np.arange(hi.size) - np.repeat(hp[:-1], hc))
    l_at = np.repeat(sp_ptr[:-1] + hc, lc) + (np.arange(li.size) - np.repeat(lp[:-1], lc))
    stacked[h_at] = hi
    stacked[l_at] = li.astype(np.int64) + M
    keep = np.nonzero(cnt > 0)[0]  # observable-only columns stay: undetectable logical faults must count
    if not merge or keep.size == 0:
        rep, groups = keep, [keep, np.arange(keep.size + 1, dtype=np.int64)]
        priors = prob[keep].copy()
    else:
        # group equal columns: two 64-bit sums of per-row random words find the candidates, an entry-wise comparison confirms them
        rng = np.random.default_rng(0x0DE7EC7)
        h1 = rng.integers(0, 2 ** 63, M + k, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        h2 = rng.integers(0, 2 ** 63, M + k, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        with np.errstate(over="ignore"):
            c1 = np.concatenate([[np.uint64(0)], np.cumsum(h1[stacked], dtype=np.uint64)])
            c2 = np.concatenate([[np.uint64(0)], np.cumsum(h2[stacked], dtype=np.uint64)])
            k1 = (c1[sp_ptr[1:]] - c1[sp_ptr[:-1]])[keep]
            k2 = (c2[sp_ptr[1:]] - c2[sp_ptr[:-1]])[keep]
        order = np.lexsort((keep, cnt[keep], k2, k1))  # equal keys adjacent, ascending fault index inside
        ks = np.stack([k1[order], k2[order], cnt[keep][order].astype(np.uint64)])
        new = np.concatenate([[True], (ks[:, 1:] != ks[:, :-1]).any(axis=0)])
        gid_sorted = np.cumsum(new) - 1
        first_sorted = keep[order][new]  # the lowest fault of every group
        rep_of = np.empty(keep.size, np.int64)
        rep_of[order] = first_sorted[gid_sorted]
        # confirm: every member's entries equal its representative's
        n_e = cnt[keep]
        offs = np.arange(int(n_e.sum())) - np.repeat(np.concatenate([[0], np.cumsum(n_e)[:-1]]), n_e)
        mine = stacked[np.repeat(sp_ptr[keep], n_e) + offs]
        reps = stacked[np.repeat(sp_ptr[rep_of], n_e) + offs]
        if not np.array_equal(mine, reps):
            raise RuntimeError("two different columns share a 128-bit key")  # (never seen; the comparison is what makes merging exact)
        # mechanisms in the order of their first fault
        rank = np.argsort(first_sorted, kind="stable")
        new_id = np.empty(rank.size, np.int64)
        new_id[rank] = np.arange(rank.size)
        gid = np.empty(keep.size, np.int64)
        gid[order] = new_id[gid_sorted]
        rep = first_sorted[rank]
        member_order = np.lexsort((keep, gid))
        members, g_sorted = keep[member_order], gid[member_order]
        sizes = np.bincount(g_sorted, minlength=rep.size)
        o_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        groups = [members, o_ptr]
        # fold every group's probabilities in ascending fault index: step j takes the j-th member of every group that has one
        priors = prob[members[o_ptr[:-1]]].copy()
        for j in range(1, int(sizes.max())):
            g = np.nonzero(sizes > j)[0]
            priors[g] = _fold(priors[g], prob[members[o_ptr[g] + j]])
    n_mech = rep.size
    col_h, row_h = _gather_columns(hp, hi, rep)
    col_l, row_l = _gather_columns(lp, li, rep)
    H = sp.csr_matrix((np.ones(col_h.size, np.uint8), (row_h, col_h)), shape=(M, n_mech), dtype=np.uint8)
    L = sp.csr_matrix((np.ones(col_l.size, np.uint8), (row_l, col_l)), shape=(k, n_mech), dtype=np.uint8)
    H.sort_indices()
    L.sort_indices()
    return H, L, priors, (groups[1], groups[0].astype(np.int64))


def circuit_dem(circuit, engine="native", merge=True, max_words=0):
    """``(H, L, priors, detector_time, origin)`` of a circuit's faults.

    Columns empty in both H and L are dropped; columns with observables only are kept.  With ``merge``, columns equal in H
    and L become one mechanism with ``p <- p1 (1 - p2) + p2 (1 - p1)``, folded in ascending fault index.  Mechanisms are
    ordered by their first elementary fault; ``origin = (indptr, indices)`` is a CSR from mechanism to elementary fault
    indices (``circuit.faults`` order).  H and L are scipy CSR uint8."""
    fa = circuit.faults
    hp, hi, lp, li = fault_columns(circuit, fa, engine, max_words)
    H, L, priors, origin = _reduce(hp, hi, lp, li, fa.prob, circuit.num_detectors, circuit.num_observables, merge)
    return H, L, priors, circuit.detector_time, origin


def dem_text(H, L, priors, detector_time=None):
    """The model as ``error(p) D... L...`` lines, one per mechanism, and ``detector(t) Dd`` lines (the format INTEGRATION.md
    describes).  Probabilities are written with ``repr``, so they read back to the last bit.  A writer only."""
    Hc, Lc = sp.csc_matrix(H), sp.csc_matrix(L)
    Hc.sort_indices()
    Lc.sort_indices()
    lines = []
    for i, p in enumerate(np.asarray(priors, np.float64)):
        targets = [f"D{d}" for d in Hc.indices[Hc.indptr[i]:Hc.indptr[i + 1]]] + [f"L{o}" for o in Lc.indices[Lc.indptr[i]:Lc.indptr[i + 1]]]
        lines.append(f"error({float(p)!r}) " + " ".join(targets))
    if detector_time is not None:
        lines += [f"detector({int(t)}) D{d}" for d, t in enumerate(detector_time)]
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------------------------------------------------- builder
def greedy_edge_colouring(h):
    """Layers of the Tanner graph of ``h``: the edges (check, bit) in ascending order, each given the lowest colour free at
    its check and at its bit.  Returns a list of layers, each a list of (check, bit) on disjoint qubits."""
    h = sp.csr_matrix(h)
    h.sort_indices()
    used_c = [set() for _ in range(h.shape[0])]
    used_b = [set() for _ in range(h.shape[1])]
    layers = []
    for c in range(h.shape[0]):
        for b in h.indices[h.indptr[c]:h.indptr[c + 1]]:
            colour = 0
            while colour in used_c[c] or colour in used_b[b]:
                colour += 1
            used_c[c].add(colour)
            used_b[b].add(colour)
            while len(layers) <= colour:
                layers.append([])
            layers[colour].append((c, int(b)))
    return layers


NOISE_KEYS = ("cx", "h", "reset", "meas", "idle", "data")


def css_memory_circuit(hx, hz, lx, lz, rounds, basis="z", noise=None):
    """The memory experiment of the CSS code (hx, hz): ``rounds`` noisy rounds of syndrome extraction, then a transversal
    data measurement in ``basis``.

    Qubits: the n data qubits, then one ancilla per row of hz, then one per row of hx.  A round measures the Z checks (data ->
    ancilla CX layers from ``greedy_edge_colouring(hz)``, then MR), then the X checks (H, ancilla -> data CX layers, H, MR).
    Detectors cover the checks of ``basis``: round 0 is the outcome alone, round t is outcome(t) xor outcome(t - 1), the
    last is the parity of the final data measurements on the check's support xor outcome(rounds - 1); ``detector_time`` is
    the round, and detector (t, c) is row t m + c.  Observables are the rows of lz (lx for basis "x") on the final data
    measurements.  ``noise`` maps "cx" (depolarize2 after each CX), "h" (depolarize1 after each H), "reset" (flip after
    each reset), "meas" (flip before each measurement), "idle" (depolarize1 on every data qubit at the start of each round
    and before the final measurement) and "data" (x_error, z_error for basis "x", at the same places) to probabilities."""
    if basis not in ("z", "x"):
        raise ValueError("basis must be 'z' or 'x'")
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError("rounds must be >= 1")
    noise = dict(noise or {})
    for key in noise:
        if key not in NOISE_KEYS:
            raise ValueError(f"unknown noise term {key!r}: one of {NOISE_KEYS}")
    p = {key: float(noise.get(key, 0.0)) for key in NOISE_KEYS}
    hx, hz = sp.csr_matrix(hx), sp.csr_matrix(hz)
    hx.sort_indices()
    hz.sort_indices()
    n = hz.shape[1]
    if hx.shape[1] != n:
        raise ValueError(f"hx has {hx.shape[1]} columns, hz {n}")
    mz, mx = hz.shape[0], hx.shape[0]
    anc_z = lambda c: n + c
    anc_x = lambda c: n + mz + c
    z_layers, x_layers = greedy_edge_colouring(hz), greedy_edge_colouring(hx)
    circ = Circuit(n + mz + mx)
    zb = basis == "z"

    def reset(q, x_basis=False):
        (circ.rx if x_basis else circ.r)(q)
        (circ.z_error if x_basis else circ.x_error)(p["reset"], q)

    def data_noise():
        for q in range(n):
            circ.depolarize1(p["idle"], q)
            (circ.x_error if zb else circ.z_error)(p["data"], q)

    for q in range(n):
        reset(q, x_basis=not zb)
    for q in range(n, n + mz + mx):
        reset(q)
    out_z, out_x = [], []  # [round][check] -> measurement index
    for _ in range(rounds):
        data_noise()
        for layer in z_layers:
            for c, b in layer:
                circ.cx(b, anc_z(c))
                circ.depolarize2(p["cx"], b, anc_z(c))
        row = []
        for c in range(mz):
            circ.x_error(p["meas"], anc_z(c))
            row.append(circ.mr(anc_z(c)))
            circ.x_error(p["reset"], anc_z(c))
        out_z.append(row)
        for c in range(mx):
            circ.h(anc_x(c))
            circ.depolarize1(p["h"], anc_x(c))
        for layer in x_layers:
            for c, b in layer:
                circ.cx(anc_x(c), b)
                circ.depolarize2(p["cx"], anc_x(c), b)
        for c in range(mx):
            circ.h(anc_x(c))
            circ.depolarize1(p["h"], anc_x(c))
        row = []
        for c in range(mx):
            circ.x_error(p["meas"], anc_x(c))
            row.append(circ.mr(anc_x(c)))
            circ.x_error(p["reset"], anc_x(c))
        out_x.append(row)
    data_noise()
    final = []
    for q in range(n):
        (circ.x_error if zb else circ.z_error)(p["meas"], q)
        final.append(circ.m(q) if zb else circ.mx(q))
    checks, outcome = (hz, out_z) if zb else (hx, out_x)
    for t in range(rounds):
        for c in range(checks.shape[0]):
            circ.detector([outcome[t][c]] + ([outcome[t - 1][c]] if t else []), time=t)
    for c in range(checks.shape[0]):
        support = checks.indices[checks.indptr[c]:checks.indptr[c + 1]]
        circ.detector([final[b] for b in support] + [outcome[rounds - 1][c]], time=rounds)
    logicals = sp.csr_matrix(lz if zb else lx)
    logicals.sort_indices()
    if logicals.shape[1] != n:
        raise ValueError(f"the logicals have {logicals.shape[1]} columns, the code {n}")
    for j in range(logicals.shape[0]):
        circ.observable([final[b] for b in logicals.indices[logicals.indptr[j]:logicals.indptr[j + 1]]])
    return circ
