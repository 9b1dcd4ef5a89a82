"""Times of the circuit-to-model path (bp_osd_amd/circuit.py, bposd_frame_*) on one MI355X.

Circuit: ``css_memory_circuit`` of ``--code`` (default h1922, the [[1922,50]] hypergraph product) at ``--rounds`` rounds, basis
z, every noise term at ``--p``.  After one warm-up per leg, ``--repeats`` rounds alternate the legs:

  native groups    FramePropagator(layered=True).columns: frame_propagate_layered_kernel, count, fill
  native op by op  FramePropagator(layered=False).columns: frame_propagate_kernel, count, fill
  numpy            fault_columns(engine="numpy") on the same circuit (``--numpy-rounds`` rounds instead, if given: said in the line)
  circuit_dem      the whole call, native and numpy: propagation, fetch and the host reduction to (H, L, priors)

Per native leg: the host time of the call and the propagate / count / fill times by the HIP events the library records, the
chunks and the device bytes.  The columns of all legs are compared before anything is timed.  Prints one line per figure;
``--out FILE`` appends them there (profiles/circuit_dem_rates.txt)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = sorted(v)
    return f"median {v[len(v) // 2]:.2f} (min {v[0]:.2f}, max {v[-1]:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", default="h1922", choices=["h1922", "surface13"])
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--numpy-rounds", type=int, default=0)
    ap.add_argument("--p", type=float, default=1e-3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from bp_osd_amd import codes
    from bp_osd_amd.circuit import FramePropagator, circuit_dem, css_memory_circuit, fault_columns

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    code = getattr(codes, a.code)()
    noise = {key: a.p for key in ("cx", "h", "reset", "meas", "idle", "data")}
    t = time.perf_counter()
    circ = css_memory_circuit(code.hx, code.hz, code.lx, code.lz, a.rounds, "z", noise)
    fa = circ.faults
    build_s = time.perf_counter() - t
    small = css_memory_circuit(code.hx, code.hz, code.lx, code.lz, a.numpy_rounds, "z", noise) if a.numpy_rounds else circ
    say(f"# tools/circuit_probe.py on one MI355X: css_memory_circuit({a.code}, rounds {a.rounds}, basis z, every noise term {a.p}): "
        f"F = {len(fa)} faults, T = {circ.T} ops, Q = {circ.Q} qubits, M = {circ.num_detectors} detectors, k = {circ.num_observables}; "
        f"built on the host in {build_s:.1f} s; warm-up, then {a.repeats} rounds alternating the legs")
    if small is not circ:
        say(f"# the numpy legs run {a.numpy_rounds} rounds: F = {len(small.faults)}, T = {small.T}")

    props = {"groups": FramePropagator(circ, layered=True), "op by op": FramePropagator(circ, layered=False)}
    cols = {name: p.columns(fa) for name, p in props.items()}  # (warm-up)
    ref = fault_columns(small, engine="numpy")
    same = all(np.array_equal(x, y) for x, y in zip(cols["groups"], cols["op by op"]))
    if small is circ:
        same = same and all(np.array_equal(x, y) for x, y in zip(cols["groups"], ref))
    say(f"columns: {int(cols['groups'][0][-1])} entries of H, {int(cols['groups'][2][-1])} of L; the legs' columns are {'identical' if same else 'DIFFERENT'}")
    if not same:
        raise SystemExit(1)
    circuit_dem(circ, engine="native")

    host = {name: [] for name in list(props) + ["numpy", "circuit_dem native", "circuit_dem numpy"]}
    events = {name: [] for name in props}
    for _ in range(a.repeats):
        for name, p in props.items():
            t = time.perf_counter()
            p.columns(fa)
            host[name].append(1e3 * (time.perf_counter() - t))
            events[name].append(p.timing())
        t = time.perf_counter()
        fault_columns(small, engine="numpy")
        host["numpy"].append(1e3 * (time.perf_counter() - t))
        for engine, c in (("native", circ), ("numpy", small)):
            t = time.perf_counter()
            H, L, priors, _, _ = circuit_dem(c, engine=engine)
            host[f"circuit_dem {engine}"].append(1e3 * (time.perf_counter() - t))
            if engine == "native":
                shape = (H.shape, L.shape[0], int(np.diff(H.tocsc().indptr).max()))
    for name, p in props.items():
        ev = np.array([e[:3] for e in events[name]])
        say(f"native {name}: bposd_frame_columns + fetch {spread(host[name])} ms; propagate {spread(ev[:, 0])} ms, count {spread(ev[:, 1])} ms, "
            f"fill {spread(ev[:, 2])} ms (HIP events, summed over {events[name][0][3]} chunks); device bytes {p.device_bytes()}")
    say(f"numpy: fault_columns {spread(host['numpy'])} ms" + (f" ({a.numpy_rounds} rounds)" if small is not circ else ""))
    say(f"circuit_dem native: {spread(host['circuit_dem native'])} ms -> H {shape[0][0]} x {shape[0][1]}, k = {shape[1]}, heaviest column {shape[2]}")
    say(f"circuit_dem numpy: {spread(host['circuit_dem numpy'])} ms" + (f" ({a.numpy_rounds} rounds)" if small is not circ else ""))
    for p in props.values():
        p.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
