"""The plain benchmark line and --dump-outputs, in a FRESH child process: the line carries the headline fields and nothing of
--full, and the dumped arrays are what the last timed step computed -- every sampled correction reproduces its syndrome and
equals the CPU oracle's decode of the same seeded input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    import bench
    from bp_osd_amd.codes import h1922
    from oracle import OracleDecoder

    B, steps, warmup = 8192, 3, 1
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--batch", str(B), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "syndromes decoded/sec (whole node) + logical error rate, HGP [[1922,50]] p=0.05"
    assert d["unit"] == "syndromes/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == steps and d["warmup"] == warmup and d["config"]["per_gpu_batch"] == B
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(B * 1e3 / d["ms_per_step"], rel=1e-9)
    for moved in ("configs", "cpu_baseline", "cross_kernel_check", "roofline", "logical_error_rate", "host_to_host"):
        assert moved not in d, moved

    H = h1922(compute_logicals=False).hz
    m, n = H.shape
    got = {name: np.load(out_dir / f"{name}.npy") for name in ("osdw", "osd0", "bp", "converged", "iters")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_TOTAL_BUDGET
    nrows = min(bench.DUMP_MAX_ROWS, B)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(B, size=nrows, replace=False))
    assert got["osdw"].shape == got["osd0"].shape == got["bp"].shape == (nrows, n)
    assert got["converged"].shape == got["iters"].shape == (B,)

    # the last timed step is step warmup + steps - 1; the steps alternate over two seeded batches (seeds 0 and 1)
    _, syn = bench.make_batch(H, 0.05, B, seed=(warmup + steps - 1) % 2)
    osdw = got["osdw"].astype(np.uint8)
    assert ((H @ osdw.T.astype(np.int64)) % 2 == syn[rows].T).all()
    k = 256
    ref = OracleDecoder(H, error_rate=0.05, max_iter=0, bp_method="ms", ms_scaling_factor=0.0, osd_method="osd_cs",
                        osd_order=7).decode_batch(np.ascontiguousarray(syn[rows[:k]]))
    assert (osdw[:k] == ref["osdw"]).all()
    assert (got["osd0"][:k] == ref["osd0"]).all() and (got["bp"][:k] == ref["bp"]).all()
    assert (got["converged"][rows[:k]] == ref["converged"]).all() and (got["iters"][rows[:k]] == ref["iters"]).all()
