"""bp_local_kernel without a dl dispatch in its iteration loop: the host's wave pairing and the ISA of the loop bodies.
No GPU needed (the ISA test needs hipcc and is skipped where there is none)."""
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest

from bp_osd_amd import _lib
from bp_osd_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _lib.load()


def _instantiated_keys():
    """The keys bp_local_kernel has a loop body for, read from the header the kernel and the host share."""
    src = open(os.path.join(ROOT, "bp_osd_amd", "csrc", "local_keys.h")).read()
    keys = [int(k) for k in re.search(r"kKeys\[kNumKeys\] = \{([^}]*)\}", src).group(1).split(",")]
    assert len(keys) == int(re.search(r"kNumKeys = (\d+)", src).group(1))
    return set(keys)


def _code(name):
    from bp_osd_amd.codes import circulant, h1922, hgp, regular_ldpc_seed

    if name.startswith("h1922"):
        return getattr(h1922(compute_logicals=False), name[-2:])
    if name == "random31_hz":
        return hgp(regular_ldpc_seed(31, 31, 3, 3, seed=3), compute_logicals=False).hz
    return hgp(circulant(45, (0, 2, 5)), compute_logicals=False).hz  # 2025 checks: the 2048-position kernel


# modelled (read cycles, write cycles, mixed pairs) of the layout search for H1922, as the search stood before the pairing
H1922_MODEL = {"h1922_hx": (204, 398, 2), "h1922_hz": (218, 408, 2)}


@pytest.mark.parametrize("name", ["h1922_hx", "h1922_hz", "random31_hz", "circulant45_hz"])
def test_wave_pairing_keeps_the_layout_and_names_every_wave(lib, name):
    """Groups of equal key are moved into the same wave (groups w and w + MP / 128).  The move permutes whole 64-position
    groups, so the modelled LDS cycles and the mixed-pair count are what the search returned; every check keeps exactly one
    position; a wave either has one key of the instantiated set for both groups or is counted as generic.  H1922: the
    search's 218 + 408 cycles (hz) / 204 + 398 (hx), 2 mixed pairs, at most one generic wave."""
    import scipy.sparse as sp

    H = sp.csr_matrix(_code(name))
    H.sort_indices()
    m, n = H.shape
    ip, ix = np.ascontiguousarray(H.indptr, dtype=np.int32), np.ascontiguousarray(H.indices, dtype=np.int32)
    gk, pc, info = np.full(32, -7, np.int32), np.full(2048, -7, np.int32), np.zeros(8, np.int64)
    assert lib.bposd_debug_local_keys(ip.ctypes.data, ix.ctypes.data, m, n, gk.ctypes.data, pc.ctypes.data, info.ctypes.data) == 0
    MP = int(info[6])
    assert MP == (1024 if m <= 1024 else 2048)
    G, W = MP // 64, MP // 128
    print(name, "before", info[0:3], "after", info[3:6], "generic waves", info[7], "keys", gk[:G])
    assert tuple(info[3:6]) == tuple(info[0:3])
    if name in H1922_MODEL:
        assert tuple(int(v) for v in info[3:6]) == H1922_MODEL[name]
    pos = pc[:MP]
    assert sorted(pos[pos >= 0].tolist()) == list(range(m)) and (pos[pos < 0] == -1).all()
    keys = _instantiated_keys()
    generic = 0
    for w in range(W):
        a, b = int(gk[w]), int(gk[w + W])
        assert a in keys and b in keys  # (a group's own key is always one of the set: anything else is the mixed key)
        generic += a != b
    assert generic == info[7]
    if name in H1922_MODEL:
        assert generic <= 1
    # the one-check-per-thread kernel has one group per wave: every wave has a body
    assert all(int(k) in keys for k in gk[:G])


def test_pairing_is_what_the_kernel_tables_use(lib):
    """bposd_debug_local_layout (the layout the tables are built from) reports the paired layout's model: same cycles and
    mixed pairs as bposd_debug_local_keys after pairing."""
    import scipy.sparse as sp

    H = sp.csr_matrix(_code("h1922_hz"))
    H.sort_indices()
    ip, ix = np.ascontiguousarray(H.indptr, dtype=np.int32), np.ascontiguousarray(H.indices, dtype=np.int32)
    out = np.zeros(16, np.int64)
    assert lib.bposd_debug_local_layout(ip.ctypes.data, ix.ctypes.data, H.shape[0], H.shape[1], out.ctypes.data) == 0
    gk, pc, info = np.zeros(32, np.int32), np.zeros(2048, np.int32), np.zeros(8, np.int64)
    assert lib.bposd_debug_local_keys(ip.ctypes.data, ix.ctypes.data, H.shape[0], H.shape[1], gk.ctypes.data, pc.ctypes.data, info.ctypes.data) == 0
    assert (out[0], out[14], out[3]) == tuple(info[3:6])


def _isa_tool():
    spec = importlib.util.spec_from_file_location("isa_loop_count", os.path.join(ROOT, "tools", "isa_loop_count.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_specialised_bodies_hold_no_dispatch():
    """ISA of the headline instance bp_local_kernel<2,1024,8,false,true,false>: one iteration loop per key without LLR
    stores, one generic loop without and one with them.  Static counts in the loop of a specialised body, against the one loop
    of the kernel before (all dl arms: 68 branches, 188 SALU, 382 VALU):
      branches  one s_cbranch_execz per owned bit (the decision flip: 4) and nothing else on exec.  The source has three more
                conditions inside the loop -- the trip test, the convergence exit, the iteration-dependent scaling factor
                of the check pass -- and a structured CFG may test each once more where the exits join: <= 6 other
                conditional branches, and no more plain s_branch than that.  No s_cbranch_scc: the dispatch on dl was
                s_cmp + s_cbranch_scc, and nothing is compared with a dl any more (the generic body still has them).
      SALU      <= 140: the 188 before minus the 48 the per-bit dispatch was counted at.
      VALU      <= 382 - 8 - 3 * 4 * 11 = 242: one arm of the bit pass per bit instead of four, no keep_llr re-materialised.
      no global stores (the LLRs are the other body's).
    (Measured when written: 12 branches = 4 flips + 5 other conditional + 3 s_branch; 75-78 SALU; 190 VALU for the uniform
    keys, 286 for the mixed key.)
    The whole instance: <= 64 VGPRs, no scratch."""
    tool = _isa_tool()
    asm, remarks = tool.compile_listing("bp_local_kernel<2,1024,8,false,true,false>")
    L = tool.loops(asm)
    keys = _instantiated_keys()
    names = {f"key={k} llr=0" for k in keys} | {"key=-1 llr=0", "key=-1 llr=1"}
    assert set(L) == names, sorted(L)
    for k in sorted(keys):
        c = L[f"key={k} llr=0"]
        print(k, tool.fmt(c))
        flips = sum(op == "s_cbranch_execz" for op in c["ops"])
        cond = sum(op.startswith("s_cbranch") for op in c["ops"]) - flips
        jumps = sum(op == "s_branch" for op in c["ops"])
        assert flips == 4 and cond <= 6 and jumps <= 6
        assert not any(op.startswith("s_cbranch_scc") for op in c["ops"])
        assert any(op.startswith("s_cbranch_scc") for op in L["key=-1 llr=0"]["ops"])
        assert c["salu"] <= 140
        if k != 15:  # (the mixed key routes its operands with per-lane selects: 16 of them per bit)
            assert c["valu_fp64"] + c["valu_other"] <= 242
        assert c.get("vmem", 0) == 0 and c["barrier"] == 2
    assert L["key=-1 llr=1"].get("vmem", 0) > 0
    vgprs = int(re.search(r" VGPRs: (\d+)", remarks).group(1))
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", remarks).group(1))
    print("VGPRs", vgprs, "scratch", scratch)
    assert vgprs <= 64 and scratch == 0
