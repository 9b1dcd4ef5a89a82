"""bp_local_kernel's body for the wave that pairs a uniform group with the mixed one: the host's wave table, the instance it
picks, and the ISA of that instance's pair loop.  No GPU needed (the ISA test needs hipcc and is skipped where there is none)."""
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest

from bp_osd_amd import _lib
from bp_osd_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = 15


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def _keys_header():
    src = open(os.path.join(ROOT, "bp_osd_amd", "csrc", "local_keys.h")).read()
    keys = [int(k) for k in re.search(r"kKeys\[kNumKeys\] = \{([^}]*)\}", src).group(1).split(",")]
    pairs = [int(k) for k in re.search(r"kPairKeys\[kNumPairKeys\] = \{([^}]*)\}", src).group(1).split(",")]
    assert len(pairs) == int(re.search(r"kNumPairKeys = (\d+)", src).group(1))
    return keys, pairs


def _pair_key(k):
    """local_keys.h: pair_key()"""
    return 32 + k


def _code(name):
    from bp_osd_amd.codes import circulant, h1922, hgp, regular_ldpc_seed

    if name.startswith("h1922"):
        return getattr(h1922(compute_logicals=False), name[-2:])
    if name == "random31_hz":
        return hgp(regular_ldpc_seed(31, 31, 3, 3, seed=3), compute_logicals=False).hz
    return hgp(circulant(45, (0, 2, 5)), compute_logicals=False).hz  # 2025 checks: the 2048-position kernel


def _tables(lib, name):
    """(group keys by wave [(a, b)], wave bodies, PAIRKEY of the picked instance, generic waves, mode)"""
    import scipy.sparse as sp

    H = sp.csr_matrix(_code(name))
    H.sort_indices()
    m, n = H.shape
    ip, ix = np.ascontiguousarray(H.indptr, dtype=np.int32), np.ascontiguousarray(H.indices, dtype=np.int32)
    gk, pc, info = np.full(32, -7, np.int32), np.full(2048, -7, np.int32), np.zeros(8, np.int64)
    assert lib.bposd_debug_local_keys(ip.ctypes.data, ix.ctypes.data, m, n, gk.ctypes.data, pc.ctypes.data, info.ctypes.data) == 0
    MP = int(info[6])
    W = MP // 128
    body, winfo = np.full(16, -7, np.int32), np.full(4, -7, np.int64)
    assert lib.bposd_debug_local_waves(ip.ctypes.data, ix.ctypes.data, m, n, body.ctypes.data, winfo.ctypes.data) == 0
    assert int(winfo[0]) == MP
    waves = [(int(gk[w]), int(gk[w + W])) for w in range(W)]
    return waves, [int(b) for b in body[:W]], int(winfo[1]), int(winfo[2]), int(winfo[3]), int(info[7])


def test_pair_keys_are_a_table_of_their_own():
    """The seven group keys are what they were (the ISA test of the plain instance reads them); the pair keys are disjoint
    from them and are pair_key() of the six uniform keys."""
    keys, pairs = _keys_header()
    assert keys == [0, 1, 2, 5, 6, 10, 15]
    assert pairs == [_pair_key(k) for k in keys if k != MIXED]
    assert not set(pairs) & set(keys)


@pytest.mark.parametrize("name", ["h1922_hz", "h1922_hx"])
def test_h1922_mixed_group_second_and_instance_matches_partner(lib, name):
    """H1922: one wave of unequal groups, (key 6, mixed).  The mixed group is the wave's second group, the instance the host
    launches has PAIRKEY = the partner's key, that wave runs the pair body and no wave is left on the generic body.  A group's
    own key and the count of waves of unequal groups (bposd_debug_local_keys) are what they were."""
    waves, body, pairkey, generic, mode, unequal = _tables(lib, name)
    print(name, waves, body, pairkey, generic, mode)
    assert mode == 2
    diff = [w for w, (a, b) in enumerate(waves) if a != b]
    assert len(diff) == 1 and unequal == 1
    a, b = waves[diff[0]]
    assert b == MIXED and a != MIXED
    assert pairkey == a
    assert body[diff[0]] == _pair_key(a)
    for w, (x, y) in enumerate(waves):
        if x == y:
            assert body[w] == x
    assert generic == 0 and all(k >= 0 for k in body)


@pytest.mark.parametrize("name", ["random31_hz", "circulant45_hz"])
def test_uncovered_waves_stay_generic(lib, name):
    """The other (3,6) codes: a wave of equal keys runs that key's body; a wave (PAIRKEY, mixed) -- mixed second -- runs the
    pair body of the one instance the host picks; every other wave of unequal groups (two different uniform keys, a partner
    key other than the instance's) is still counted generic."""
    keys, pairs = _keys_header()
    waves, body, pairkey, generic, mode, unequal = _tables(lib, name)
    print(name, waves, body, pairkey, generic, mode)
    assert mode == 2
    n_generic = 0
    for w, (a, b) in enumerate(waves):
        assert a in keys and b in keys
        if a == b:
            assert body[w] == a
        elif b == MIXED and a == pairkey:
            assert body[w] == _pair_key(a) and body[w] in pairs
        else:
            assert body[w] == -1
            n_generic += 1
        assert not (a == MIXED and b != MIXED)  # the mixed group of a wave of unequal groups is its second
    assert n_generic == generic
    assert unequal == sum(a != b for a, b in waves)
    candidates = [a for a, b in waves if a != b and b == MIXED]
    assert (pairkey in candidates) if candidates else (pairkey == -1)
    if name == "random31_hz":
        assert generic >= 1  # its wave of two different uniform keys has no body of its own


def _isa_tool():
    spec = importlib.util.spec_from_file_location("isa_loop_count", os.path.join(ROOT, "tools", "isa_loop_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_pair_loop_of_the_picked_headline_instance(lib):
    """ISA of the instance the host picks for H1922, bp_local_kernel<2,1024,8,false,true,false,PAIRKEY>: the seven keyed loops
    and the two generic ones of the plain instance plus the pair loop, which meets the limits tests/test_local_dispatch_cpu.py
    sets for a uniform key (4 s_cbranch_execz, <= 6 other conditional branches, <= 6 s_branch, no s_cbranch_scc, SALU <= 140,
    VALU <= 242, no global store, two barriers); the instance has <= 64 VGPRs, no scratch and no private segment; every wave of
    H1922's table runs a loop other than the generic one.  (Measured when written: 12 branches = 4 + 5 + 3, 75 SALU, 238 VALU;
    61 VGPRs.)"""
    waves, body, pairkey, generic, mode, _ = _tables(lib, "h1922_hz")
    assert pairkey >= 0
    tool = _isa_tool()
    asm, remarks = tool.compile_listing(f"bp_local_kernel<2,1024,8,false,true,false,{pairkey}>")
    L = tool.loops(asm)
    keys, _ = _keys_header()
    pk = _pair_key(pairkey)
    assert set(L) == {f"key={k} llr=0" for k in keys} | {f"key={pk} llr=0", "key=-1 llr=0", "key=-1 llr=1"}, sorted(L)
    c = L[f"key={pk} llr=0"]
    print(pk, tool.fmt(c))
    flips = sum(op == "s_cbranch_execz" for op in c["ops"])
    cond = sum(op.startswith("s_cbranch") for op in c["ops"]) - flips
    jumps = sum(op == "s_branch" for op in c["ops"])
    assert flips == 4 and cond <= 6 and jumps <= 6
    assert not any(op.startswith("s_cbranch_scc") for op in c["ops"])
    assert c["salu"] <= 140
    assert c["valu_fp64"] + c["valu_other"] <= 242
    assert c.get("vmem", 0) == 0 and c["barrier"] == 2
    for b in body:  # no wave of H1922 runs the generic loop
        assert b >= 0 and f"key={b} llr=0" in L and f"key={b} llr=0" != "key=-1 llr=0"
    vgprs = int(re.search(r" VGPRs: (\d+)", remarks).group(1))
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", remarks).group(1))
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    print("VGPRs", vgprs, "scratch", scratch, "private segment", private)
    assert vgprs <= 64 and scratch == 0 and private and all(v == 0 for v in private)
