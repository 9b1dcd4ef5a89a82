"""Static instruction counts of a BP kernel's iteration loop (the innermost loop: Depth=2 blocks of the ISA listing).
usage: python tools/isa_loop_count.py '<template instantiation>' [header] [--body 'key=5 llr=0'] [--list]
   e.g. python tools/isa_loop_count.py 'bp_kernel<6,3,2,4,512,6,true,0,1024>' bp_kernel.hip.h
        python tools/isa_loop_count.py 'bp_local_kernel<2,1024,8,false,true,false>' --body 'key=5 llr=0'
Compiles the one instantiation for gfx950 with the library's flags and prints wave-instructions per thread-iteration by
class.  The BP loops are fully unrolled inside an iteration and their branches are wave-uniform, so the static count of the
loop body is what a wave executes per iteration on the common path (rare-path blocks -- decision flips, LLR stores -- are
included: an upper bound).
bp_local_kernel holds one iteration loop per body (a key of the wave's groups, with / without LLR stores); each names itself
with a "; bpl_body key=K llr=L" comment in the listing.  Without --body the counts are summed over all loops (what the tool
printed when a kernel had one loop); --body counts the one named loop, --list prints every loop on a line of its own.
Importable: compile_listing(inst) gives the listing and the resource remarks, loops(listing) the counts per loop."""
import os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"]


def classify(op):
    if op.startswith("v_"):
        return "valu_fp64" if ("_f64" in op) else "valu_other"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "wait/nop"
    if op.startswith("s_cbranch") or op.startswith("s_branch"):
        return "branch"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("global_") or op.startswith("scratch_") or op.startswith("buffer_") or op.startswith("flat_"):
        return "vmem"
    return "other"


def default_header(inst):
    return "bp_class_kernel.hip.h" if "class" in inst else "bp_local_kernel.hip.h" if "local" in inst else "bp_kernel.hip.h"


def compile_listing(inst, hdr=None):
    """(ISA listing, resource-usage remarks) of the one instantiation."""
    hdr = hdr or default_header(inst)
    params = {"bp_kernel": "BpParams", "bp_local_kernel": "BpLocalParams", "bp_class_kernel": "BpClassParams"}[inst.split("<")[0]]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "k.hip")
        open(src, "w").write(f'#include "{ROOT}/bp_osd_amd/csrc/{hdr}"\ntemplate __global__ void bposd::{inst}(const bposd::{params});\n')
        r = subprocess.run([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + FLAGS + ["-c", src, "-o", os.path.join(d, "k.o"), "-save-temps", "-Rpass-analysis=kernel-resource-usage"],
                           cwd=d, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(r.stderr[-2000:])
        asm = open([os.path.join(d, f) for f in os.listdir(d) if f.endswith("gfx950.s")][0]).read()
    return asm, r.stderr


def loops(asm):
    """{loop name: {class: count, "ops": [mnemonics]}} for every Depth=2 loop; a loop is named by its bpl_body marker if
    it has one, else by the label of its header block."""
    depth, header, block = 0, None, None
    out, names = {}, {}
    for line in asm.split("\n"):
        mlabel = re.match(r"^(\.LBB\d+_\d+):", line)
        if mlabel or line.startswith("; %bb."):
            depth, header = 0, None
            block = mlabel.group(1) if mlabel else None
        mhead = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", line)
        if mhead:
            depth = int(mhead.group(1))
            header = block.replace(".L", "") if block else None
        minner = re.search(r"in Loop: Header=(\S+) .*Depth=(\d+)", line)
        if minner:
            depth = int(minner.group(2))
            header = minner.group(1).replace(".L", "")
        t = line.strip()
        if depth >= 2 and header:
            mname = re.match(r"; bpl_body (key=-?\d+ llr=\d)", t)
            if mname:
                names[header] = mname.group(1)
        if not t or t.startswith(";") or t.startswith(".") or depth < 2 or not header:
            continue
        op = t.split()[0]
        c = out.setdefault(header, {"ops": []})
        cls = classify(op)
        c[cls] = c.get(cls, 0) + 1
        c["ops"].append(op)
    return {names.get(h, h): c for h, c in out.items()}


def fmt(c):
    body = " ".join(f"{k}={v}" for k, v in sorted(c.items()) if k != "ops")
    return body + " valu_total=%d" % (c.get("valu_fp64", 0) + c.get("valu_other", 0))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    inst = args[0]
    body = sys.argv[sys.argv.index("--body") + 1] if "--body" in sys.argv else None
    if body in args:
        args.remove(body)
    hdr = args[1] if len(args) > 1 else None
    asm, _ = compile_listing(inst, hdr)
    L = loops(asm)
    if "--list" in sys.argv:
        for name, c in L.items():
            print(inst, "[%s]" % name, fmt(c))
    elif body:
        print(inst, "[%s]" % body, fmt(L[body]))
    else:
        tot = {}
        for c in L.values():
            for k, v in c.items():
                if k != "ops":
                    tot[k] = tot.get(k, 0) + v
        print(inst, fmt(tot))
