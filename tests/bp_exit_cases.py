"""Syndromes whose BP iteration counts the oracle fixes beforehand, and the table of matrices that carry them to every BP
kernel family but bp_local_kernel (which has tests/local_codes.py).

Every BP kernel decodes shot after shot in one persistent workgroup and leaves its iteration loop at one of three places:
before the loop (the zero syndrome), at the convergence test that follows a check pass (``iters = it - 1``) and at
``it > max_iter``.  What can go wrong is an exit one iteration early or late, or state a shot leaves for the next one: the
mismatch bitmap and its flags, the hard decisions, the priors, the message slices of the HBM-resident kernels.  A test sees
that only if it knows at which iteration every shot must leave, and if a workgroup decodes several shots.

The plan of a matrix (``plan_for``; CPU only):
- a pool of ``N_POOL`` syndromes: the all-zero one (iters = 0), H e for one error of weight 1 that the oracle converges in
  one iteration (the first such bit in a seeded order: on a matrix with weak columns not every bit is one), and H e for
  random errors of rate q;
- the *target*: the pool row the oracle converges in the fewest iterations k >= 3 at max_iter 30;
- the pool decoded by the oracle with max_iter k + 1 (the target converges inside the loop), k (it converges in the last
  iteration: the test after the last bit pass), k - 1 (it misses by one: iters = max_iter, OSD takes it) and 1.
``CASES`` names what must occur; the plan asserts each on the oracle's results, a GPU test on the kernel's.
``batch_index`` repeats the pool in order, with the target, the zero syndrome and the one-iteration syndrome at the first
and last three indices of the batch.

``EXIT_ROWS`` is the table of tests/test_gpu_bp_exits.py; tests/test_bp_exits_cpu.py keeps it honest without a GPU.
"""
import functools

import numpy as np
import scipy.sparse as sp

N_POOL = 32
CASES = ("zero syndrome: iters 0", "one iteration, max_iter > 1", "one iteration, max_iter 1: converged in the last",
         "converged inside the loop", "converged in the last iteration", "missed by one", "missed at max_iter 1",
         "ordinary converged next to a missed one")
CASES_WITHOUT_MAX_ITER_1 = tuple(c for c in CASES if "max_iter 1" not in c)


def _occurred(res, target, k, max_iter):
    """The CASES a result (oracle's or kernel's, pool order) with this max_iter shows."""
    conv, it = np.asarray(res["converged"]).astype(bool), np.asarray(res["iters"])
    seen = set()
    if conv[0] and it[0] == 0:
        seen.add(CASES[0])
    if conv[1] and it[1] == 1:
        seen.add(CASES[1] if max_iter > 1 else CASES[2])
    t = (bool(conv[target]), int(it[target]))
    if max_iter == k + 1 and t == (True, k):
        seen.add(CASES[3])
        others = np.arange(len(it)) != target
        if (conv[2:] & (it[2:] >= 2) & others[2:]).any() and (~conv[2:] & (it[2:] == max_iter)).any():
            seen.add(CASES[7])
    if max_iter == k and t == (True, k):
        seen.add(CASES[4])
    if max_iter == k - 1 and t == (False, k - 1):
        seen.add(CASES[5])
    if max_iter == 1 and t == (False, 1):
        seen.add(CASES[6])
    return seen


def oracle_keywords(kw):
    """Decoder keywords as the oracle takes them: ``ps_math_form`` (the library's) becomes ``ps_math = 2 - form``."""
    kw = dict(kw)
    if "ps_math_form" in kw:
        kw["ps_math"] = 2 - kw.pop("ps_math_form")
    return kw


def pool_for(H, kw, q, seed, what=()):
    """uint8 [N_POOL, m]: row 0 the zero syndrome, row 1 H e for the first bit, in a seeded order, whose weight-1 error the
    oracle (keywords ``kw``, max_iter 30) converges with iters = 1, rows 2 .. H e for random errors of rate q."""
    from oracle import OracleDecoder

    H = sp.csr_matrix(H, dtype=np.int32)
    m, n = H.shape
    rng = np.random.default_rng(seed)
    err = (rng.random((N_POOL, n)) < q).astype(np.int32)
    err[0] = 0
    err[1] = 0
    order = np.concatenate([[int(rng.integers(n))], rng.permutation(n)])
    o = OracleDecoder(H, max_iter=30, **oracle_keywords(kw))
    bit = None
    for lo in range(0, len(order), 16):
        cand = order[lo:lo + 16]
        e1 = np.zeros((len(cand), n), np.int32)
        e1[np.arange(len(cand)), cand] = 1
        r = o.decode_batch((np.asarray(H @ e1.T) % 2).T.astype(np.uint8))
        hit = np.flatnonzero((r["converged"] != 0) & (r["iters"] == 1))
        if hit.size:
            bit = int(cand[hit[0]])
            break
    assert bit is not None, what + ("no weight-1 error converges in one iteration",)
    err[1, bit] = 1
    return np.ascontiguousarray((np.asarray(H @ err.T) % 2).T.astype(np.uint8))


def plan_for(H, kw, q, seed, with_max_iter_1=True, what=()):
    """dict(H, kw, q, pool, target, k, max_iters, cases, refs {max_iter: the oracle's result for the pool}) for a matrix and
    decoder keywords without max_iter; see the module docstring.  Asserts, on the oracle alone, that the pool holds a target
    and that the runs together show every one of ``cases`` (CASES, or those that need no run at max_iter 1)."""
    from oracle import OracleDecoder

    okw = oracle_keywords(kw)
    pool = pool_for(H, kw, q, seed, what)
    ref30 = OracleDecoder(H, max_iter=30, **okw).decode_batch(pool)
    ok = [i for i in range(2, N_POOL) if ref30["converged"][i] and ref30["iters"][i] >= 3]
    assert ok, what + ("no pool syndrome converges in 3 .. 30 iterations", ref30["iters"])
    target = min(ok, key=lambda i: ref30["iters"][i])
    k = int(ref30["iters"][target])
    max_iters = (k + 1, k, k - 1) + ((1,) if with_max_iter_1 else ())
    cases = CASES if with_max_iter_1 else CASES_WITHOUT_MAX_ITER_1
    refs = {mi: OracleDecoder(H, max_iter=mi, **okw).decode_batch(pool) for mi in max_iters}
    seen = set().union(*[_occurred(refs[mi], target, k, mi) for mi in max_iters])
    assert seen == set(cases), what + ("the oracle does not produce", sorted(set(cases) - seen))
    return dict(H=H, kw=kw, q=q, pool=pool, target=target, k=k, max_iters=max_iters, cases=cases, refs=refs)


def batch_index(B, target):
    """Pool row of every batch row: the pool in order, over and over, with the target, the zero syndrome and the
    one-iteration syndrome at both ends."""
    idx = np.arange(B) % N_POOL
    idx[:3] = (target, 0, 1)
    idx[-3:] = (1, 0, target)
    return idx


# ------------------------------------------------------------------------------------------------ the row table
def dropped_regular(m, col_w, row_w, seed):
    """regular_ldpc_seed(m, 2m, col_w, row_w) with the first entry of check 0 dropped: check degrees row_w - 1 .. row_w, bit
    degrees col_w - 1 .. col_w -- no regular code (the REG instances and the local-edge kernel leave it alone)."""
    from bp_osd_amd.codes import regular_ldpc_seed

    h = regular_ldpc_seed(m, 2 * m, col_w, row_w, seed=seed).astype(np.uint8)
    h[0, np.flatnonzero(h[0])[0]] = 0
    return h


def exit_matrix(row):
    """The matrix of one EXIT_ROWS row (scipy CSR, uint8, sorted indices)."""
    from tests.edge_codes import EDGE_BY_ID, _code, pcm_for

    kind, *a = row["matrix"]
    if kind == "edge":
        H = pcm_for(EDGE_BY_ID[a[0]])
    elif kind == "code":
        H = _code(a[0])
    else:
        assert kind == "dropped"
        H = dropped_regular(*a)
    H = sp.csr_matrix(H, dtype=np.uint8)
    H.sort_indices()
    return H


# One row per BP kernel instance.  Keys: id; family; matrix (("edge", id of an EDGES row) / ("code", a PS_CODES construction) /
# ("dropped", m, col_w, row_w, seed): dropped_regular); bp (the instance last_instance() must report, without the packed
# flag); bp_variant / schedule where the instance needs a request; probs ("uniform": error_rate q -- the scalar-prior
# instance on the class kernel --, "channel": per-bit probabilities around q); factor (ms_scaling_factor: 0.625 and 0
# alternate by row); q and seed of the min-sum plan, q56 / seed56 of the 56-iteration run and ps (dict(form, q, seed), or a
# string that says why the matrix gives no product-sum plan) -- each pair chosen so that the oracle alone yields every
# required case (tests/test_bp_exits_cpu.py); large_osd (the matrix lands on osd_large_kernel: the big batches decode with
# osd_off); stride (class rows: what the layout search settles on); batches (syndromes per decode); env (environment the
# decoders are created under).
B_GENERIC = 4101  # > 2 x the largest grid of a kernel of at least 256 threads: 2 x 256 CUs x 8 workgroups, + 5
B_CLASS = 8197  # bp_class_kernel: up to 16 workgroups per CU
B_CLASS_QUEUE = 65539  # m <= 160: (B - seen) >> queue_shift falls from 8 to 1, several shots per queue atomic
EXIT_ROWS = []


def _row(id, family, matrix, bp, q, seed=1, probs="uniform", **kw):
    kw.setdefault("factor", (0.625, 0.0)[len(EXIT_ROWS) % 2])
    kw.setdefault("q56", q)
    kw.setdefault("seed56", seed)
    kw.setdefault("ps", dict(form=len(EXIT_ROWS) % 2, q=q, seed=seed))
    kw.setdefault("large_osd", False)
    kw.setdefault("batches", (B_CLASS,) if family == "bp_class_kernel" else (B_GENERIC,))
    EXIT_ROWS.append(dict(id=id, family=family, matrix=matrix, bp=bp, q=q, seed=seed, probs=probs, **kw))


def _bpk(dc, dv, cpt=1, nt=1024):
    return ("bp_kernel", (dc, dv, cpt, nt))


_D24, _D36 = ("dropped", 150, 2, 4, 1), ("dropped", 150, 3, 6, 1)
# bp_kernel, predicated, one check per thread: every degree pair (the EDGES matrices of the pairs (4, 2) and (6, 3) converge
# within two iterations or never: regular codes with one entry dropped stand in for them), and the largest matrix of the shape
_row("bp_pair_4_2", "bp_kernel", _D24, _bpk(4, 2), q=0.03, bp_variant=1)
_row("bp_pair_6_3", "bp_kernel", _D36, _bpk(6, 3), q=0.04, probs="channel")
_row("bp_pair_8_4", "bp_kernel", ("edge", "bp_pair_8_4"), _bpk(8, 4), q=0.01)
_row("bp_pair_12_6", "bp_kernel", ("edge", "bp_pair_12_6"), _bpk(12, 6), q=0.006, probs="channel", q56=0.018, seed56=4,
     ps=dict(form=1, q=0.006, seed=3))
_row("bp_pair_16_8", "bp_kernel", ("edge", "bp_pair_16_8"), _bpk(16, 8), q=0.006, seed=2)
_row("bp_shape1_m1024_n2048_dc16", "bp_kernel", ("edge", "bp_shape1_m1024_n2048_dc16"), _bpk(16, 8), q=0.006, probs="channel",
     large_osd=True, q56=0.03, seed56=2)
# bp_kernel<6, 3, REG> at shapes 1, 2 and 4, on request
_row("bp_reg63_shape1", "bp_kernel_reg", ("code", "reg36_m120"), _bpk(6, 3, 1, 1024), q=0.05, bp_variant=1)
_row("bp_reg63_shape2", "bp_kernel_reg", ("code", "reg36_m120"), _bpk(6, 3, 2, 512), q=0.05, bp_variant=2, probs="channel")
_row("bp_reg63_shape4", "bp_kernel_reg", ("code", "reg36_m120"), _bpk(6, 3, 4, 256), q=0.05, bp_variant=4)
# shape 2 on request, shape 8 (two checks per thread, stride 2048) at two degree pairs
_row("bp_shape2_m1024_n2048_variant2", "bp_kernel", ("edge", "bp_shape2_m1024_n2048_variant2"), _bpk(8, 4, 2, 512), q=0.006,
     bp_variant=2, large_osd=True)
_row("bp_shape8_8_4", "bp_kernel", ("edge", "bp_shape8_m1025_dc8"), _bpk(8, 4, 2, 1024), q=0.006, probs="channel",
     large_osd=True, q56=0.018, seed56=3)
_row("bp_shape8_6_3", "bp_kernel", ("dropped", 1030, 3, 6, 1), _bpk(6, 3, 2, 1024), q=0.04, large_osd=True, q56=0.06,
     seed56=3)
# bp_class_kernel: the surface-code class at its three strides (m = 150 takes 8 shots per queue atomic, m = 161 one), then one
# code per other degree class.  A (3,6)-regular code with min-sum belongs to the local-edge kernel, and bposd_create then
# builds no class tables: the (6; 3) row creates its decoders with BPOSD_CLASS_ALWAYS set (tools/README.md) and asks for the
# class kernel by number -- no matrix reaches the min-sum instance of that class otherwise
_row("bp_class_mp256_m150", "bp_class_kernel", _D24, ("bp_class_kernel", (3, 4, 2, 256)), q=0.03, stride=256,
     batches=(B_CLASS, B_CLASS_QUEUE))
_row("bp_class_mp256_m161", "bp_class_kernel", ("dropped", 161, 2, 4, 1), ("bp_class_kernel", (3, 4, 2, 256)), q=0.03,
     stride=256, probs="channel", seed56=5)
_row("bp_class_mp512_m240", "bp_class_kernel", ("dropped", 240, 2, 4, 1), ("bp_class_kernel", (3, 4, 2, 512)), q=0.03,
     stride=512)
_row("bp_class_mp1024_m500", "bp_class_kernel", ("dropped", 500, 2, 4, 1), ("bp_class_kernel", (3, 4, 2, 1024)), q=0.03,
     stride=1024, probs="channel", seed56=2)
_row("bp_class_7_hgp400", "bp_class_kernel", ("code", "hgp400_hz"), ("bp_class_kernel", (7, 7, 4, 256)), q=0.03, stride=256)
_row("bp_class_6_reg36_m120", "bp_class_kernel", ("code", "reg36_m120"), ("bp_class_kernel", (6, 6, 3, 256)), q=0.05,
     stride=256, bp_variant=32, env={"BPOSD_CLASS_ALWAYS": "1"}, probs="channel")
_row("bp_class_4_toric12", "bp_class_kernel", ("code", "toric12_hx"), ("bp_class_kernel", (4, 4, 2, 256)), q=0.03, stride=256)
_row("bp_class_8_reg44", "bp_class_kernel", ("code", "reg44_hx"), ("bp_class_kernel", (8, 8, 4, 256)), q=0.03, stride=256,
     probs="channel")
# bp_large_kernel<12, 6> and <16, 8>: min-sum with the check data in LDS (form 2) and, under set_bp_variant(63), with whole
# check records in the workspace (form 1); product-sum is form 0
_row("bp_large_12_6", "bp_large_kernel", ("edge", "bp_hbm_m1025_dc9"), ("bp_large_kernel", (12, 6, 2)), q=0.006, large_osd=True)
_row("bp_large_16_8_n2049", "bp_large_kernel", ("edge", "bp_hbm_m1024_n2049_dc16"), ("bp_large_kernel", (16, 8, 2)), q=0.006,
     probs="channel", large_osd=True, q56=0.06, ps=dict(form=1, q=0.006, seed=2))
_row("bp_large_16_8_m2049", "bp_large_kernel", ("edge", "bp_hbm_m2049_dv7"), ("bp_large_kernel", (16, 8, 2)), q=0.006,
     large_osd=True)
# the kernels of any degree and of the serial schedule (bit degree 8: BPS_MAXDV)
_row("bp_anydeg_dc17", "bp_anydeg_kernel", ("edge", "bp_anydeg_dc17"), ("bp_anydeg_kernel", ()), q=0.03, probs="channel",
     q56=0.045, seed56=2)
_row("bp_anydeg_dv9", "bp_anydeg_kernel", ("edge", "bp_anydeg_dv9"), ("bp_anydeg_kernel", ()), q=0.03)
_row("bp_serial_dv8_channel", "bp_serial_kernel", ("edge", "bp_serial_dv8"), ("bp_serial_kernel", ()), q=0.03, probs="channel",
     schedule="serial", q56=0.045, seed56=4)
_row("bp_serial_dv8", "bp_serial_kernel", ("edge", "bp_serial_dv8"), ("bp_serial_kernel", ()), q=0.03, schedule="serial")
EXIT_BY_ID = {r["id"]: r for r in EXIT_ROWS}
PS_CLIPS = (8.0, 20.0, 37.0)  # the finite clips of edge_codes.ps_cases


def row_index(row):
    return next(i for i, r in enumerate(EXIT_ROWS) if r["id"] == row["id"])


def exit_keywords(row, kind, n):
    """Decoder keywords, without max_iter, of one run of a row: kind "ms" (min-sum with the row's factor), "f56" (factor 0: the
    adaptive factor 1 - 2^-it) or "ps" (product-sum in the row's form, with a finite clip).  The big batches of a row that
    lands on osd_large_kernel decode with osd_off."""
    q = {"ms": row["q"], "f56": row["q56"], "ps": row["ps"]["q"] if kind == "ps" else None}[kind]
    kw = dict(osd_method="osd_off" if row["large_osd"] else "osd0")
    if kind == "ps":
        kw.update(bp_method="ps", ps_math_form=row["ps"]["form"], ps_clip=PS_CLIPS[row_index(row) % 3])
    else:
        kw.update(bp_method="ms", ms_scaling_factor=row["factor"] if kind == "ms" else 0.0)
    if row["probs"] == "channel":
        kw["channel_probs"] = q * (0.75 + 0.5 * np.random.default_rng(5).random(n))
    else:
        kw["error_rate"] = q
    if row.get("schedule"):
        kw["schedule"] = row["schedule"]
    return kw


def has_ps(row):
    return isinstance(row["ps"], dict)


def select_reference(row, p):
    """(prior_select [N_POOL, n], alt_channel_probs [n], the oracle's result) of the per-shot-prior run of a row on the pool of
    its min-sum plan ``p`` at max_iter k: select row i belongs to pool row i (edge_codes.ps_select / ps_oracle_select).  Asserts
    that the per-shot channel shows: some pool row's BP outcome differs from the plan's at the same max_iter."""
    from oracle import OracleDecoder
    from tests.edge_codes import ps_oracle_select, ps_select

    k = p["k"]
    sel, alt = ps_select(dict(seed=row_index(row)), N_POOL, p["H"].shape[1])
    ref = ps_oracle_select(OracleDecoder(p["H"], max_iter=k, **oracle_keywords(p["kw"])), p["pool"], sel, alt)
    plain = p["refs"][k]
    changed = (ref["iters"] != plain["iters"]).any() or (ref["bp"] != plain["bp"]).any()
    assert changed, (row["id"], "the per-shot channel changes nothing")
    return sel, alt, ref


@functools.lru_cache(maxsize=None)
def exit_plan(row_id, kind):
    """The plan of one row (``plan_for``; "ps": without the run at max_iter 1); the min-sum plan of a row whose big batches
    decode with osd_off also holds ``refs_osd0``, the oracle's osd0 results for the bare pool.  kind "f56": dict(H, kw, pool,
    target, ref) of the 56-iteration run -- the target is a pool row still unconverged at 56, which the plan asserts to exist:
    its LLRs carry the factors of iteration 53 (1 - 2^-53), 54 and later (1.0)."""
    from oracle import OracleDecoder

    row = EXIT_BY_ID[row_id]
    H = exit_matrix(row)
    kw = exit_keywords(row, kind, H.shape[1])
    what = (row_id, kind)
    if kind == "f56":
        pool = pool_for(H, kw, row["q56"], row["seed56"], what)
        ref = OracleDecoder(H, max_iter=56, **kw).decode_batch(pool)
        left = np.flatnonzero(ref["converged"] == 0)
        assert left.size and (ref["iters"][left] == 56).all(), what + ("every pool row converges within 56 iterations",)
        assert ref["converged"][1] and ref["iters"][1] == 1 and ref["iters"][0] == 0, what
        return dict(H=H, kw=kw, pool=pool, target=int(left[0]), ref=ref)
    q, seed = (row["q"], row["seed"]) if kind == "ms" else (row["ps"]["q"], row["ps"]["seed"])
    p = plan_for(H, kw, q, seed, with_max_iter_1=kind == "ms", what=what)
    if row["large_osd"] and kind == "ms":
        okw = oracle_keywords(dict(kw, osd_method="osd0"))
        p["refs_osd0"] = {mi: OracleDecoder(H, max_iter=mi, **okw).decode_batch(p["pool"]) for mi in p["max_iters"]}
    return p
