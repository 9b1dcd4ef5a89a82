"""Circuits, fault lists and the independent reference of tests/test_circuit_cpu.py and tests/test_gpu_circuit.py.

``reference_columns`` is the frame rule of the issue's table on unpacked bool arrays, one fault at a time.  It takes a
circuit's public arrays and shares no code with bp_osd_amd/circuit.py."""
import functools

import numpy as np

from bp_osd_amd import codes
from bp_osd_amd.circuit import Circuit, css_memory_circuit, make_faults

FULL_NOISE = {key: 1e-3 for key in ("cx", "h", "reset", "meas", "idle", "data")}


# ----------------------------------------------------------------------------------------------- the independent reference
def reference_columns(circuit, faults=None):
    """[(detectors, observables)] per fault, each an ascending tuple: one frame per fault, straight from the table."""
    ops = [tuple(int(v) for v in row) for row in circuit.ops]
    T, Q = len(ops), circuit.Q
    dp, di = circuit.detectors
    op_, oi = circuit.observables
    fa = circuit.faults if faults is None else faults
    out = []
    for pos, qa, pa, qb, pb in zip(fa.pos.tolist(), fa.qa.tolist(), fa.pa.tolist(), fa.qb.tolist(), fa.pb.tolist()):
        x, z = np.zeros(Q, bool), np.zeros(Q, bool)
        flips = []
        for t in range(T + 1):
            if t == pos:
                x[qa] ^= bool(pa & 1)
                z[qa] ^= bool(pa & 2)
                if qb != -1:
                    x[qb] ^= bool(pb & 1)
                    z[qb] ^= bool(pb & 2)
            if t == T:
                break
            op, a, b = ops[t]
            if op == 6:  # H
                x[a], z[a] = z[a], x[a]
            elif op == 7:  # S
                z[a] ^= x[a]
            elif op == 8:  # CX
                x[b] ^= x[a]
                z[a] ^= z[b]
            elif op == 9:  # CZ
                za, zb = z[a] ^ x[b], z[b] ^ x[a]
                z[a], z[b] = za, zb
            elif op in (0, 1):  # R, RX
                x[a] = z[a] = False
            elif op in (2, 4):  # M, MR
                flips.append(bool(x[a]))
                if op == 4:
                    x[a] = z[a] = False
            elif op in (3, 5):  # MX, MRX
                flips.append(bool(z[a]))
                if op == 5:
                    x[a] = z[a] = False
            else:
                raise AssertionError(op)
        rows = []
        for ptr, idx in ((dp, di), (op_, oi)):
            vals = [sum(flips[m] for m in idx[ptr[r]:ptr[r + 1]]) % 2 for r in range(len(ptr) - 1)]
            rows.append(tuple(r for r, v in enumerate(vals) if v))
        out.append(tuple(rows))
    return out


def csc_columns(ptr, idx):
    return [tuple(int(v) for v in idx[ptr[i]:ptr[i + 1]]) for i in range(len(ptr) - 1)]


def engine_columns(result):
    """(h_indptr, h_indices, l_indptr, l_indices) -> the form of reference_columns."""
    hp, hi, lp, li = result
    return list(zip(csc_columns(hp, hi), csc_columns(lp, li)))


# ------------------------------------------------------------------------------------------------------------- circuits
def opcode_circuit():
    """Five qubits, every opcode, 13 measurements, 5 detectors and 2 observables (annotated for coverage, not for
    determinism: the kernels do not care)."""
    c = Circuit(5)
    c.r(0); c.rx(1); c.h(2); c.s(2); c.cx(0, 1); c.cz(1, 2); c.cx(2, 3); c.s(3); c.h(3); c.cz(3, 4); c.cx(4, 0)
    m = [c.mr(0), c.mrx(1)]
    c.h(0); c.cx(0, 2); c.cz(1, 4); c.s(4); c.h(4); c.cx(3, 1); c.s(1)
    m += [c.m(2), c.mx(3), c.m(4), c.mx(0), c.m(1)]
    c.r(2); c.rx(3); c.cx(2, 3); c.cz(0, 3); c.h(1); c.cx(1, 4)
    m += [c.mx(2), c.m(3), c.mr(4), c.mrx(0), c.m(1), c.mx(4)]
    c.detector([m[0]], 0)
    c.detector([m[1], m[3]], 0)
    c.detector([m[2], m[4], m[7]], 1)
    c.detector([m[0], m[5], m[6], m[8], m[12]], 1)
    c.detector([m[9], m[10], m[11]], 2)
    c.observable([m[4], m[9]])
    c.observable([m[2], m[3], m[11], m[12]])
    return c


def random_circuit(Q, T, seed):
    """T random ops on Q qubits (two-qubit ops only where there are two qubits); the caller annotates."""
    rng = np.random.default_rng(seed)
    names = ["R", "RX", "M", "MX", "MR", "MRX", "H", "S"] + (["CX", "CZ"] * 3 if Q > 1 else [])
    c = Circuit(Q)
    meas = []
    for _ in range(T):
        name = names[int(rng.integers(len(names)))]
        a = int(rng.integers(Q))
        b = int((a + 1 + rng.integers(Q - 1)) % Q) if Q > 1 else 0
        r = c.append(name, a, b)
        if r is not None:
            meas.append(r)
    return c, meas


def random_faults(circuit, F, seed, positions=None):
    """F faults: positions drawn from ``positions`` (default 0 .. T), one- and two-qubit ones mixed, the two-qubit ones
    cycling through all 15 Pauli pairs (an identity on the first qubit becomes a one-qubit fault of the second)."""
    rng = np.random.default_rng(seed)
    T, Q = circuit.T, circuit.Q
    pos = rng.integers(0, T + 1, F) if positions is None else np.asarray(positions)[rng.integers(0, len(positions), F)]
    qa = rng.integers(0, Q, F)
    pa, qb, pb = np.zeros(F, np.int64), np.full(F, -1), np.zeros(F, np.int64)
    for i in range(F):
        code = 1 + i % 15
        a, b = code & 3, code >> 2
        if Q > 1 and a and b:
            pa[i], pb[i], qb[i] = a, b, (qa[i] + 1 + rng.integers(Q - 1)) % Q
        else:
            pa[i] = a or b
    return make_faults(pos, qa, pa, qb, pb, rng.uniform(1e-4, 1e-2, F))


FAULT_COUNTS = (1, 63, 64, 65, 128, 129, 64 * 256 - 1, 64 * 256 + 1)


def annotation_circuit(kind):
    """The annotation shapes of the GPU issue list; each returns (circuit, F)."""
    if kind == "q1":
        c, meas = random_circuit(1, 40, 5)
        c.detector(meas[:3], 0)
        c.detector(meas[2:], 1)
        c.observable(meas[::2])
        return c, 200
    c, meas = random_circuit(5, 240, 7)
    assert len(meas) >= 41
    if kind == "unused_measurement":
        c.detector(meas[1:4], 0)
        c.detector(meas[5:9], 1)
        c.observable(meas[1:6])  # measurement 0 and the ones from 9 on are in nothing
    elif kind == "shared_measurement":
        c.detector(meas[:3], 0)
        c.detector(meas[2:6], 1)
        c.observable([meas[2], meas[7]])  # measurement 2: two detectors and an observable
    elif kind == "wide_detector":
        c.detector(meas[:40], 0)
        c.detector(meas[39:41], 1)
        c.observable(meas[::3])
    elif kind == "m1_k0":
        c.detector(meas[:7], 0)
    elif kind == "k65":
        c.detector(meas[:5], 0)
        for j in range(65):
            c.observable([meas[j % len(meas)], meas[(3 * j + 1) % len(meas)], meas[(7 * j + 2) % len(meas)]])
    else:
        raise KeyError(kind)
    return c, 300


ANNOTATION_KINDS = ("unused_measurement", "shared_measurement", "wide_detector", "m1_k0", "k65", "q1")


# ------------------------------------------------------------------------------------------------------ builder circuits
def ring_css(d):
    """The ring code as a CSS code with Z checks only: hz the d x d ring, no X checks, logical Z on bit 0 (any Z product is
    deterministic on |0...0>), logical X the all-ones row."""
    hz = codes.ring_code(d)
    return np.zeros((0, d), np.uint8), hz, np.ones((1, d), np.uint8), np.eye(1, d, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def builder_code(name):
    if name == "surface13":
        c = codes.surface13()
    elif name == "hgp23":
        c = codes.hgp(codes.rep_code(2), codes.rep_code(3))
    elif name == "ring4":
        return ring_css(4)
    else:
        raise KeyError(name)
    return c.hx, c.hz, c.lx, c.lz


# (code, basis): the ring code has Z checks only; both bases for the surface code
BUILDER_CASES = [("surface13", "z"), ("surface13", "x"), ("hgp23", "z"), ("ring4", "z")]
BUILDER_ROUNDS = (1, 2, 4)


def builder_circuit(name, basis, rounds, noise):
    hx, hz, lx, lz = builder_code(name)
    return css_memory_circuit(hx, hz, lx, lz, rounds, basis, noise)
