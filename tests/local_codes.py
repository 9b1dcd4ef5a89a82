"""Parity-check matrices for bp_local_kernel: one table row per matrix, with the loop bodies its waves run.

bp_local_kernel takes (3,6)-regular m x 2m matrices with m <= 2048 (1024 positions up to m = 1024, 2048 above).  One
instance holds seven keyed iteration loops (group keys 0, 1, 2, 5, 6, 10 and 15 = mixed: csrc/local_keys.h), a generic
loop, a generic loop with LLR stores and -- in the PAIRKEY instances -- a pair loop 32 + k for the wave (uniform key k,
mixed group).  Which loop a wave runs is not a property of the kernel but of the matrix: the host's layout search
(csrc/local_layout.h) sorts checks into 64-position groups, pairs groups into waves and picks the instance.  A suite that
decodes a few codes covers what those codes happen to land on, and a change of the search can take a body out of the
suite without any test failing.

So ``LOCAL_CODES`` pins, for named and seeded constructions, the whole wave table the search gives: per wave the keys of
its two groups and the body it runs, PAIRKEY, the number of generic waves and of padding-only groups.  ``for_bodies``
says what a row is in the table for.  tests/test_local_codes_cpu.py reads the tables through the host-only exports
``bposd_debug_local_keys`` / ``bposd_debug_local_waves`` (``wave_tables``: no GPU) and asserts that every row still lands
on its bodies and that the rows together cover, at 1024 and at 2048 positions, all seven keys and the generic body on waves
whose two groups both hold checks, and every pair body at one of the two sizes at least (``coverage``; ``NOT_FOUND`` names
the combinations no searched matrix reaches).  tests/test_gpu_local_bodies.py decodes every row on the GPU against the LDS
kernel and the oracle, and asserts the same tables first.  A change of the layout search that drops a body therefore fails
on the CPU, in the row that was there for it, before any GPU runs.

The rows also hold the edges of the size window: m = 64, 65 and 128 (real and padding lanes inside one group, waves of
padding only), 1024 (no padding position), 1025 (1023 padding positions), 2048 (the last m), and ``PAST_WINDOW``, one
matrix past it, which the search refuses.

The search's acceptance test calls std::exp, so another libm may move a layout: a row that then fails says which seed to
replace, it does not say the kernel is wrong.

``q`` is the physical error rate of a row's ``H e`` syndromes: one for which the oracle alone, at max_iter 30 and
ms_scaling_factor 0.625, leaves between 0.1 % and 60 % of them unconverged (asserted on the CPU for the very syndromes
the GPU test decodes).
"""
import numpy as np
import scipy.sparse as sp

MIXED = 15
KEYS = (0, 1, 2, 5, 6, 10, 15)
PAIR_KEYS = (0, 1, 2, 5, 6, 10)
N_SPECIAL = 34  # rows 0 .. 33 of a batch of syndromes: all-zero, all-ones, 32 uniformly random


def csr(H):
    H = sp.csr_matrix(H, dtype=np.uint8)
    H.sort_indices()
    return H


def wave_tables(lib, H):
    """What the host's layout search decides for a matrix, read through the two host-only exports bposd_debug_local_keys
    and bposd_debug_local_waves (no GPU): a dict with

    - ``MP`` positions (1024 / 2048), ``pairkey`` (PAIRKEY of the instance auto-selection launches, -1 the plain one),
      ``generic`` (waves on the generic body), ``mode`` and ``unequal`` (waves whose groups differ in key, counted
      before a pair body is assigned: info[7] of bposd_debug_local_keys, which its header calls the waves on the generic
      body -- true of the plain instance only);
    - ``group_key`` [MP / 64] and ``group_checks`` [MP / 64] (checks a group holds: 0 for a padding-only group);
    - per wave w of the two-checks-per-thread kernels (groups w and w + MP / 128): ``waves`` [(key, key)], ``body`` (a
      group key, 32 + k for the pair body, -1 generic) and ``real`` [(bool, bool)]: whether each group holds a check;
    - ``padding_only_groups``.

    Raises ValueError with the library's status where the local-edge kernel does not take the matrix."""
    H = csr(H)
    m, n = H.shape
    ip, ix = np.ascontiguousarray(H.indptr, dtype=np.int32), np.ascontiguousarray(H.indices, dtype=np.int32)
    gk, pc, info = np.full(32, -7, np.int32), np.full(2048, -7, np.int32), np.zeros(8, np.int64)
    rc = lib.bposd_debug_local_keys(ip.ctypes.data, ix.ctypes.data, m, n, gk.ctypes.data, pc.ctypes.data, info.ctypes.data)
    if rc:
        raise ValueError(f"bposd_debug_local_keys: status {rc}")
    MP = int(info[6])
    G, W = MP // 64, MP // 128
    body, winfo = np.full(16, -7, np.int32), np.full(4, -7, np.int64)
    rc = lib.bposd_debug_local_waves(ip.ctypes.data, ix.ctypes.data, m, n, body.ctypes.data, winfo.ctypes.data)
    if rc:
        raise ValueError(f"bposd_debug_local_waves: status {rc}")
    assert int(winfo[0]) == MP
    pos_chk = pc[:MP]
    assert sorted(int(c) for c in pos_chk[pos_chk >= 0]) == list(range(m)), "pos_chk does not place every check once"
    checks = [int((pos_chk[64 * g: 64 * g + 64] >= 0).sum()) for g in range(G)]
    return dict(MP=MP, pairkey=int(winfo[1]), generic=int(winfo[2]), mode=int(winfo[3]), unequal=int(info[7]),
                group_key=[int(k) for k in gk[:G]], group_checks=checks,
                waves=[(int(gk[w]), int(gk[w + W])) for w in range(W)], body=[int(b) for b in body[:W]],
                real=[(checks[w] > 0, checks[w + W] > 0) for w in range(W)],
                padding_only_groups=sum(c == 0 for c in checks))


def matrix_of(row):
    """The matrix of one row (scipy CSR, uint8, sorted indices)."""
    from bp_osd_amd.codes import circulant, h1922, hgp, regular_ldpc_seed

    kind, *a = row["make"]
    if kind == "reg36":  # regular_ldpc_seed(m, 2m, 3, 6, seed)
        return csr(regular_ldpc_seed(a[0], 2 * a[0], 3, 6, seed=a[1]))
    if kind == "h1922":  # the [[1922,50]] product code
        return csr(getattr(h1922(compute_logicals=False), a[0]))
    if kind == "hgp_reg33":  # hypergraph product of a random (3,3)-regular a x a seed
        return csr(getattr(hgp(regular_ldpc_seed(a[0], a[0], 3, 3, seed=a[1]), compute_logicals=False), a[2]))
    if kind == "hgp_circ":  # hypergraph product of a circulant
        return csr(getattr(hgp(circulant(a[0], a[1]), compute_logicals=False), a[2]))
    raise ValueError(kind)


def expected_body(a, b, pairkey):
    """The body of a wave of groups with keys (a, b) in the instance compiled for ``pairkey`` (local_layout.h: wave_plan)."""
    if a == b:
        return a
    if b == MIXED and a == pairkey:
        return 32 + a
    return -1


def assert_row_tables(row, t):
    """A live wave table (``wave_tables``) is the one the row pins, and is consistent in itself."""
    rid = row["id"]
    assert t["MP"] == row["MP"] == (1024 if row["m"] <= 1024 else 2048), (rid, t["MP"])
    assert t["mode"] == 2, rid
    assert t["waves"] == row["waves"], (rid, "group keys by wave", t["waves"])
    assert t["body"] == row["body"], (rid, "wave bodies", t["body"])
    assert t["pairkey"] == row["pairkey"] and t["generic"] == row["generic"], (rid, t["pairkey"], t["generic"])
    assert t["padding_only_groups"] == row["pad"], (rid, "padding-only groups", t["padding_only_groups"])
    for (a, b), body in zip(t["waves"], t["body"]):
        assert a in KEYS and b in KEYS and body == expected_body(a, b, t["pairkey"]), (rid, a, b, body)
        assert not (a == MIXED and b != MIXED), rid  # the mixed group of a wave of unequal groups is its second
    assert t["generic"] == sum(b == -1 for b in t["body"]) and t["unequal"] == sum(a != b for a, b in t["waves"]), rid
    assert sum(t["group_checks"]) == row["m"], rid
    assert set(row["for_bodies"]) <= set(t["body"]), (rid, "the bodies the row is in the table for", t["body"])


def syndromes(H, q, nb, seed):
    """uint8 [nb, m]: the all-zero syndrome, the all-ones syndrome, 32 uniformly random ones, then H e for nb - 34 random e
    of rate q.  The first rows do not depend on nb (the generator fills row by row)."""
    rng = np.random.default_rng(seed)
    m, n = H.shape
    rand = rng.integers(0, 2, size=(N_SPECIAL - 2, m))
    err = (rng.random((nb - N_SPECIAL, n)) < q).astype(np.uint8)
    he = np.asarray((sp.csr_matrix(H, dtype=np.int32) @ err.T.astype(np.int32)) % 2).T
    rows = [np.zeros((1, m), np.int64), np.ones((1, m), np.int64), rand, he]
    return np.ascontiguousarray(np.concatenate(rows).astype(np.uint8))


def syndrome_seed(row):
    return 1000 + row["m"]


def per_bit_probs(row):
    """The per-bit channel of the GPU test: q scaled by 0.75 .. 1.25"""
    return row["q"] * (0.75 + 0.5 * np.random.default_rng(5).random(2 * row["m"]))


def decoder_settings(q, max_iter):
    return dict(error_rate=q, max_iter=max_iter, bp_method="ms", ms_scaling_factor=0.625, osd_method="osd0")


# ------------------------------------------------------------------------------------------------ the table
# One row per matrix.  waves: "a,b" per wave, the keys of groups w and w + MP / 128; body: per wave a group key, 32 + k
# (pair body) or -1 (generic); pad: padding-only groups; for_bodies: what the row is in the table for; full_rank: rank m
# (every syndrome is then in the column space, and OSD's outputs equal the oracle's for random syndromes too).
LOCAL_CODES = []


def _row(id, make, m, q, full_rank, waves, body, pairkey, generic, pad, for_bodies, why):
    waves = [tuple(int(k) for k in w.split(",")) for w in waves.split()]
    body = [int(b) for b in body.split()]
    assert len(waves) == len(body) == (8 if m <= 1024 else 16)
    LOCAL_CODES.append(dict(id=id, make=make, m=m, MP=1024 if m <= 1024 else 2048, q=q, full_rank=full_rank, waves=waves,
                            body=body, pairkey=pairkey, generic=generic, pad=pad, for_bodies=for_bodies, why=why))


_row("h1922_hz", ('h1922', 'hz'), m=961, q=0.04, full_rank=False,
     waves="1,1 5,5 5,5 5,5 5,5 5,5 6,6 6,15",
     body="1 5 5 5 5 5 6 38", pairkey=6, generic=0, pad=0,
     for_bodies=(38,),
     why="the headline code: one wave of unequal groups, (6, mixed), on the pair body; no generic wave")
_row("h1922_hx", ('h1922', 'hx'), m=961, q=0.04, full_rank=False,
     waves="1,1 5,5 5,5 5,5 5,5 5,5 6,6 6,15",
     body="1 5 5 5 5 5 6 38", pairkey=6, generic=0, pad=0,
     for_bodies=(38,),
     why="as hz")
_row("random31_s3_hz", ('hgp_reg33', 31, 3, 'hz'), m=961, q=0.04, full_rank=True,
     waves="0,0 1,1 2,2 2,2 6,6 10,10 1,6 5,15",
     body="0 1 2 2 6 10 -1 37", pairkey=5, generic=1, pad=0,
     for_bodies=(0, 1, 2, 6, 10, 37, -1),
     why="keys 0, 1, 2, 6 and 10 on real waves; pair body 37; a generic wave of two different uniform keys (1, 6)")
_row("random31_s0_hz", ('hgp_reg33', 31, 0, 'hz'), m=961, q=0.04, full_rank=True,
     waves="0,0 1,1 1,1 2,2 2,6 5,5 6,6 10,15",
     body="0 1 1 2 -1 5 6 42", pairkey=10, generic=1, pad=0,
     for_bodies=(42, 5, -1),
     why="pair body 42 at 1024 positions; generic wave (2, 6)")
_row("random31_s4_hz", ('hgp_reg33', 31, 4, 'hz'), m=961, q=0.04, full_rank=True,
     waves="0,0 1,1 2,2 2,2 5,6 6,6 10,10 1,15",
     body="0 1 2 2 -1 6 10 33", pairkey=1, generic=1, pad=0,
     for_bodies=(33, -1),
     why="pair body 33 at 1024 positions; generic wave (5, 6)")
_row("reg1000_s14", ('reg36', 1000, 14), m=1000, q=0.07, full_rank=True,
     waves="0,0 0,15 1,1 1,1 5,5 6,6 10,10 15,15",
     body="0 32 1 1 5 6 10 15", pairkey=0, generic=0, pad=0,
     for_bodies=(32, 15),
     why="pair body 32 at 1024 positions; a wave of two mixed groups (key 15)")
_row("reg1000_s4", ('reg36', 1000, 4), m=1000, q=0.07, full_rank=True,
     waves="0,0 0,1 1,1 5,5 6,6 10,10 2,15 15,15",
     body="0 -1 1 5 6 10 34 15", pairkey=2, generic=1, pad=0,
     for_bodies=(34, 15, -1),
     why="pair body 34 at 1024 positions; its groups hold all seven keys (the numbered-variant sweep)")
_row("reg1024_s7", ('reg36', 1024, 7), m=1024, q=0.07, full_rank=True,
     waves="0,0 0,1 1,1 5,5 6,6 6,15 10,10 15,15",
     body="0 -1 1 5 6 38 10 15", pairkey=6, generic=1, pad=0,
     for_bodies=(38, 15, -1),
     why="window edge m = 1024: no padding position at all")
_row("reg64_s1", ('reg36', 64, 1), m=64, q=0.07, full_rank=True,
     waves="15,15 0,0 0,0 0,0 0,0 0,0 0,0 0,0",
     body="15 0 0 0 0 0 0 0", pairkey=-1, generic=0, pad=14,
     for_bodies=(15, 0),
     why="window edge m = 64: real and padding lanes in the two groups of one wave, seven waves of padding only (body 0)")
_row("reg65_s1", ('reg36', 65, 1), m=65, q=0.07, full_rank=True,
     waves="1,1 15,15 0,0 0,0 0,0 0,0 0,0 0,0",
     body="1 15 0 0 0 0 0 0", pairkey=-1, generic=0, pad=13,
     for_bodies=(1, 15, 0),
     why="window edge m = 65: a wave of a real and a padding-only group")
_row("reg128_s1", ('reg36', 128, 1), m=128, q=0.07, full_rank=True,
     waves="1,1 0,0 5,5 15,15 0,0 0,0 0,0 0,0",
     body="1 0 5 15 0 0 0 0", pairkey=-1, generic=0, pad=12,
     for_bodies=(1, 0, 5, 15),
     why="window edge m = 128: four waves of a part-filled and a padding-only group")
_row("circ45_hz", ('hgp_circ', 45, (0, 2, 5), 'hz'), m=2025, q=0.03, full_rank=True,
     waves="1,1 1,15 5,5 5,5 5,5 5,5 5,5 5,5 5,5 5,5 5,5 5,5 5,5 5,5 6,6 6,6",
     body="1 33 5 5 5 5 5 5 5 5 5 5 5 5 6 6", pairkey=1, generic=0, pad=0,
     for_bodies=(33, 1, 5, 6),
     why="the 2025-check product code of the suite: pair body 33 at 2048 positions")
_row("reg1900_s3", ('reg36', 1900, 3), m=1900, q=0.07, full_rank=True,
     waves="0,0 0,0 0,0 1,1 1,1 1,1 2,2 5,5 5,5 5,6 6,6 6,6 10,10 10,10 10,1 0,15",
     body="0 0 0 1 1 1 2 5 5 -1 6 6 10 10 -1 32", pairkey=0, generic=2, pad=1,
     for_bodies=(32, 2, -1),
     why="pair body 32 at 2048 positions; generic waves (5, 6) and (10, 1); a padding-only group next to a full one")
_row("reg1900_s6", ('reg36', 1900, 6), m=1900, q=0.07, full_rank=True,
     waves="0,0 0,0 0,0 1,1 1,1 1,1 2,2 5,5 5,5 5,5 6,6 6,6 6,0 10,10 10,10 1,15",
     body="0 0 0 1 1 1 2 5 5 5 6 6 -1 10 10 33", pairkey=1, generic=1, pad=0,
     for_bodies=(33, 2, -1),
     why="key 2 on a real wave at 2048 positions; its groups hold all seven keys (the numbered-variant sweep); generic wave (6, 0)")
_row("reg2048_s2", ('reg36', 2048, 2), m=2048, q=0.07, full_rank=True,
     waves="0,0 0,0 0,0 1,1 1,1 1,1 1,2 5,5 5,5 5,15 6,6 6,6 6,6 10,10 10,10 15,15",
     body="0 0 0 1 1 1 -1 5 5 37 6 6 6 10 10 15", pairkey=5, generic=1, pad=0,
     for_bodies=(37, 15, -1),
     why="window edge m = 2048: the last m, no padding position; pair body 37; a wave of two mixed groups")
_row("reg2048_s3", ('reg36', 2048, 3), m=2048, q=0.07, full_rank=True,
     waves="0,0 0,0 0,0 1,1 1,1 1,1 1,2 5,5 5,5 5,6 6,6 6,6 10,10 10,10 10,15 15,15",
     body="0 0 0 1 1 1 -1 5 5 -1 6 6 10 10 42 15", pairkey=10, generic=2, pad=0,
     for_bodies=(42, 15, -1),
     why="pair body 42 at 2048 positions; generic waves (1, 2) and (5, 6)")
_row("reg2048_s49", ('reg36', 2048, 49), m=2048, q=0.07, full_rank=True,
     waves="0,0 0,0 0,0 1,1 1,1 1,1 1,1 2,5 5,5 5,5 6,6 6,6 6,15 10,10 10,10 15,15",
     body="0 0 0 1 1 1 1 -1 5 5 6 6 38 10 10 15", pairkey=6, generic=1, pad=0,
     for_bodies=(38, 15, -1),
     why="pair body 38 at 2048 positions")
_row("reg1025_s1", ('reg36', 1025, 1), m=1025, q=0.07, full_rank=True,
     waves="0,0 0,0 1,1 1,1 5,5 6,6 10,10 5,5 6,6 2,2 15,15 0,0 0,0 0,0 0,0 0,0",
     body="0 0 1 1 5 6 10 5 6 2 15 0 0 0 0 0", pairkey=-1, generic=0, pad=14,
     for_bodies=(0, 1, 2, 5, 6, 10, 15),
     why="window edge m = 1025: 1023 padding positions, five waves of padding only, four of a real and a padding-only group")
_row("random45_s29_hz", ('hgp_reg33', 45, 29, 'hz'), m=2025, q=0.03, full_rank=True,
     waves="0,0 0,0 0,5 1,1 1,1 1,1 2,2 2,2 2,2 2,2 6,6 6,6 6,6 10,10 10,10 2,15",
     body="0 0 -1 1 1 1 2 2 2 2 6 6 6 10 10 34", pairkey=2, generic=1, pad=0,
     for_bodies=(34, 2, -1),
     why="pair body 34 at 2048 positions")

# One matrix past the window: (3,6)-regular, m = 2050 > 2048.  local_layout_for refuses it (BPOSD_ERR_UNSUPPORTED = -2);
# no LDS shape of bp_kernel holds it either (shape 8: two checks per thread, 1024 threads), so bposd_create makes BP
# HBM-resident: bp_large_kernel <12, 6, 2> (degrees <= 12 / 6, min-sum with the check data in LDS).
PAST_WINDOW = dict(id="reg2050_s1", make=("reg36", 2050, 1), m=2050, q=0.07, full_rank=True)

# What no searched matrix reaches, with the extent of the search.  All 12 (MP, pair body) combinations are in the table.
# The extent: 886 layouts -- regular_ldpc_seed(m, 2m, 3, 6, seed) for m = 960, 1000 and 1024 with seeds 15 .. 94, m = 1600,
# 1900 and 2048 with seeds 4 .. 89, m = 1100, 1300, 1750 and 2000 with seeds 2 .. 59; hz of the product of a random
# (3,3)-regular a x a seed for a = 31 (seeds 4 .. 39, and hx for seeds 0 .. 19), 40 (0 .. 29) and 45 (0 .. 39).
NOT_FOUND = {
    "pair": (),  # (MP, 32 + k)
    # A generic wave (k, mixed) with k != PAIRKEY needs two waves of a uniform and a mixed group.  local_layout::pair_groups
    # pairs the mixed groups with each other first, so at most one is left for a uniform partner: none of the 886 layouts
    # has two such waves.  The generic body does run on a (k, mixed) wave in the plain instance, which a variant asked for
    # by number launches (tests/test_gpu_local_bodies.py: test_numbered_variants_without_llr, tests/test_gpu_local_pair.py).
    "generic_mixed": (1024, 2048),
}

# one row per MP whose groups hold all seven keys (the numbered-variant sweep of the GPU test)
ALL_KEYS_ROWS = ("reg1000_s4", "reg1900_s6")


def row_by_id(rid):
    return next(r for r in LOCAL_CODES if r["id"] == rid)


def coverage(tables):
    """From {row id: wave_tables(...)}: per MP the bodies run by a wave whose two groups both hold checks --
    ``keyed[MP]`` {key}, ``pair[MP]`` {32 + k}, ``generic_uniform[MP]`` {(a, b)} (generic waves of two different uniform
    keys), ``generic_mixed[MP]`` {(k, pairkey)} (generic waves (k, mixed), k != PAIRKEY)."""
    cov = {what: {1024: set(), 2048: set()} for what in ("keyed", "pair", "generic_uniform", "generic_mixed")}
    for t in tables.values():
        for (a, b), body, real in zip(t["waves"], t["body"], t["real"]):
            if not (real[0] and real[1]):
                continue
            if body >= 32:
                cov["pair"][t["MP"]].add(body)
            elif body >= 0:
                cov["keyed"][t["MP"]].add(body)
            elif b == MIXED:
                cov["generic_mixed"][t["MP"]].add((a, t["pairkey"]))
            else:
                cov["generic_uniform"][t["MP"]].add((a, b))
    return cov
