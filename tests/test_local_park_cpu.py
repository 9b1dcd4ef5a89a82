"""bp_local_kernel's park at drain without a GPU: the record layout and the rule of csrc/local_park.h, compiled into a
small host program (the header is plain C++; skipped where there is no compiler), and the plan of the GPU cases
(tests/local_park_cases.py), asserted on the oracle alone."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.local_park_cases import CH, MAX_ITERS, PARK_ROWS, crosses, batch_index, plan, planned_parks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or (
    "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)

PROGRAM = r"""
#include <cstdio>
#include <initializer_list>
#include "local_park.h"
using namespace bposd_local_park;
int main() {
    for (int mp : {1024, 2048}) {
        constexpr Layout a = layout(1024);
        static_assert(a.bytes % 128 == 0, "");
        const Layout l = layout(mp);
        printf("layout %d %zu %zu %zu %zu %zu %zu %zu\n", mp, l.shot, l.iter, l.msg, l.loc, l.bitmap, l.dec, l.bytes);
    }
    printf("words %d %d %d %d\n", kChunk, kParkCount, kResumeHead, kCounterBytes);
    for (int mode = 0; mode < 3; ++mode)
        for (int bits = 0; bits < 256; ++bits)
            printf("rule %d %d %d\n", mode, bits, park_rule(mode, bits & 1, bits & 2, bits & 4, bits & 8, bits & 16, bits & 32, bits & 64, bits & 128));
    return 0;
}
"""


@pytest.fixture(scope="module")
def header_says(tmp_path_factory):
    if CXX is None:
        pytest.skip("needs a C++ compiler")
    d = tmp_path_factory.mktemp("local_park")
    src = d / "p.cpp"
    src.write_text(PROGRAM)
    subprocess.run([CXX, "-std=c++17", "-x", "c++", "-I", os.path.join(ROOT, "bp_osd_amd", "csrc"), str(src), "-o", str(d / "p")], check=True)
    return subprocess.run([str(d / "p")], check=True, capture_output=True, text=True).stdout.splitlines()


@pytest.mark.parametrize("mp", [1024, 2048])
def test_record_size_and_offsets(header_says, mp):
    """The record holds, in this order and without overlap: the shot (8 bytes), the next iteration (4, padded to 8), the
    whole message region of LDS ((4 MP + 2) doubles, as bp_local_lds_bytes counts it), 2 MP local messages, the MP / 32
    bitmap words, one decision word per thread (at most MP threads); doubles are 8-byte aligned, records 128-byte."""
    got = [int(v) for v in [ln for ln in header_says if ln.startswith(f"layout {mp} ")][0].split()[2:]]
    shot, it, msg, loc, bitmap, dec, size = got
    assert (shot, it, msg) == (0, 8, 16)
    assert loc == msg + (4 * mp + 2) * 8
    assert bitmap == loc + 2 * mp * 8
    assert dec == bitmap + (mp // 32) * 4
    assert size >= dec + mp * 4 and size - (dec + mp * 4) < 128 and size % 128 == 0
    assert msg % 8 == 0 and loc % 8 == 0 and bitmap % 4 == 0 and dec % 4 == 0
    assert size == {1024: 53504, 2048: 106880}[mp]
    # every per-lane byte offset the kernel forms is a 32-bit sum far below 2^32
    assert size < 1 << 20


def test_counter_block(header_says):
    """The park words lie behind the 32 bytes that go into the call record; the chunk is what the plan assumes."""
    ch, count, head, size = [int(v) for v in [ln for ln in header_says if ln.startswith("words")][0].split()[1:]]
    assert ch == CH and count == 8 and head == 9 and size >= 4 * (head + 1) and size % 8 == 0


def test_rule(header_says):
    """park_on_dry: off unless OSD follows, no LLRs are stored per iteration, the instance is one auto-selection takes and
    the call is neither lean nor tail-gated; then force parks always, never never, and auto only for a device-pointer
    call that is not small (one check per thread: latency-bound) while another lane has work in flight."""
    got = {(int(a), int(b)): int(c) for a, b, c in (ln.split()[1:] for ln in header_says if ln.startswith("rule"))}
    assert len(got) == 3 * 256
    for mode, bits in itertools.product(range(3), range(256)):
        device, lean, tail, llr, osd, spec, busy, small = [bool(bits & (1 << i)) for i in range(8)]
        able = osd and spec and not (llr or lean or tail)
        want = 0 if (mode == 1 or not able) else (2 if mode == 2 else (1 if device and busy and not small else 0))
        assert got[(mode, bits)] == want, (mode, device, lean, tail, llr, osd, spec, busy, small)


@pytest.mark.parametrize("row_id,B", PARK_ROWS, ids=[r for r, _ in PARK_ROWS])
def test_oracle_alone_says_which_shots_cross_a_boundary(row_id, B):
    """The pool holds a shot the oracle converges in exactly CH - 1, CH and CH + 1 iterations and one it gives up on; at
    max_iter CH - 1 and CH no shot of the batch crosses a boundary (the chunk ends at max_iter: nothing may park), at every
    larger max_iter some do -- the CH and CH + 1 shots and the stuck one among them, the CH - 1 shot never."""
    p = plan(row_id)
    idx = batch_index(B)
    assert set(idx) == set(range(len(p["pool"])))
    top = p["refs"][MAX_ITERS[-1]]
    for k, i in p["edge"].items():
        assert top["converged"][i] and top["iters"][i] == k, (row_id, k)
    assert top["iters"][0] == 0 and top["converged"][0]
    for mi in MAX_ITERS:
        ref = p["refs"][mi]
        assert not ref["converged"][p["stuck"]] and ref["iters"][p["stuck"]] == mi
        c = crosses(ref["iters"], mi)
        n = planned_parks(p, B, mi)
        print(row_id, "max_iter", mi, "pool rows that cross", np.flatnonzero(c).tolist(), "of the batch", n)
        if mi <= CH:
            assert n == 0 and not c.any()
        else:
            assert n >= B // len(p["pool"]) * int(c.sum()) > 0
            assert c[p["edge"][CH]] and c[p["edge"][CH + 1]] and c[p["stuck"]] and not c[p["edge"][CH - 1]] and not c[0]
    # the edge shots at the max_iter that puts the LLR body's iteration next to the boundary
    assert p["refs"][CH]["converged"][p["edge"][CH]] and p["refs"][CH]["iters"][p["edge"][CH]] == CH  # converged in the last iteration
    assert not p["refs"][CH]["converged"][p["edge"][CH + 1]]
    assert p["refs"][CH + 1]["converged"][p["edge"][CH + 1]]  # restored straight into the LLR body, converges there
