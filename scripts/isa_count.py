#!/usr/bin/env python3
"""Static instruction counts per kernel of HIP sources, from the gfx950 assembly the Makefile's
HIPFLAGS produce (hipcc -S --cuda-device-only).  CPU only: hipcc cross-compiles.

Per kernel: instruction counts by class, s_barrier count, the metadata's .vgpr_count,
.sgpr_spill_count, .vgpr_spill_count and LDS bytes, and the same class counts for every loop body
the compiler marks with "Inner Loop Header" (the blocks its "in Loop: Header=" comments assign to
the loop), together with what stands ahead of the loop's first instruction in the kernel.

Classes go by mnemonic prefix only: v_ = VALU (v_readlane / v_writelane included), s_ = scalar
(branches, waits, nops and scalar loads included; s_barrier is listed apart), ds_ = LDS,
global_ / buffer_ / flat_ / scratch_ = vector memory.  The counts are static: an instruction in a
loop counts once, one on a rarely taken path counts like any other.

Usage: isa_count.py [source.hip ...] [--kernels name,name] [--keep-asm out.s] [EXTRA_HIPFLAGS...]
(default sources: the corner stage files csrc/corner_{sort,pairs,arc,flags}.hip; --keep-asm takes one source)
"""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

PKG = Path(__file__).resolve().parent.parent / "event-camera-clustering-and-optical-flow-estimation_amd"
CLASSES = ("valu", "scalar", "lds", "vmem")
VMEM_PREFIXES = ("global_", "buffer_", "flat_", "scratch_")


def makefile_var(name):
    """The Makefile's own expansion of a variable (so the counts follow its flags)."""
    r = subprocess.run(["make", "-s", "--no-print-directory", "-C", str(PKG), "-f", "Makefile", "-f", "-", "_print_var"],
                       input=f"_print_var:\n\t@echo $({name})\n", capture_output=True, text=True, check=True)
    return r.stdout.split()


def classify(mn):
    if mn.startswith("v_"):
        return "valu"
    if mn == "s_barrier":
        return "barrier"
    if mn.startswith("s_"):
        return "scalar"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(VMEM_PREFIXES):
        return "vmem"
    return None


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::", "", n).split("(")[0] for n in out]


def parse_functions(asm):
    """symbol -> (instructions as (mnemonic, loop), inner-loop headers in order); `loop` is the
    header label of the loop the instruction's block belongs to (the compiler's "in Loop:
    Header=" block comments; a rotated loop keeps its latch ahead of the header), else None."""
    funcs, cur, loop = {}, None, None
    types = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M))
    lines = asm.splitlines()
    for n, line in enumerate(lines):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        s = line.strip()
        if m or s.startswith("; %bb."):  # a new basic block
            name = m.group(1) if m else None
            if name in types:
                cur = funcs.setdefault(name, ([], []))
                loop = None
                continue
            if name and name.startswith(".Lfunc_end"):
                cur = None
                continue
            if cur is None:
                continue
            note = line + " " + (lines[n + 1] if n + 1 < len(lines) and lines[n + 1].lstrip().startswith(";") else "")
            h = re.search(r"in Loop: Header=(\w+)", note)
            if name and "Loop Header" in note:
                loop = name
                if "Inner Loop Header" in note:
                    cur[1].append(name)
            else:
                loop = ".L" + h.group(1) if h else None
            continue
        if cur is None or not s or s.startswith((";", ".")):
            continue
        cur[0].append((s.split(";")[0].split(None, 1)[0], loop))
    return funcs


def count(insts):
    c = {k: 0 for k in CLASSES + ("barrier",)}
    for mn, _ in insts:
        k = classify(mn)
        if k:
            c[k] += 1
    return c


def parse_metadata(asm):
    """symbol -> {field: int} from the amdhsa.kernels metadata."""
    meta, cur = {}, None
    want = (".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".group_segment_fixed_size")
    for line in asm.splitlines():
        if re.match(r"^  - \.", line):
            cur = {}
            line = "    " + line[4:]
        if cur is None:
            continue
        m = re.match(r"^    (\.\w+):\s*(\S+)", line)
        if not m:
            continue
        if m.group(1) in want:
            cur[m.group(1)] = int(m.group(2))
        elif m.group(1) == ".symbol":
            meta[m.group(2).strip("'\"").removesuffix(".kd")] = cur
    return meta


def main():
    argv = sys.argv[1:]
    only, keep = None, None
    if "--kernels" in argv:
        i = argv.index("--kernels")
        only = argv[i + 1].split(",")
        del argv[i:i + 2]
    if "--keep-asm" in argv:
        i = argv.index("--keep-asm")
        keep = argv[i + 1]
        del argv[i:i + 2]
    srcs = [Path(a) for a in argv if a.endswith(".hip")]
    extra = [a for a in argv if not a.endswith(".hip")]
    srcs = srcs or [PKG / "csrc" / f"corner_{stage}.hip" for stage in ("sort", "pairs", "arc", "flags")]
    if keep and len(srcs) != 1:
        sys.exit("--keep-asm takes one source")
    hipcc = makefile_var("HIPCC")[0]
    flags = makefile_var("HIPFLAGS")
    for src in srcs:
        report(src, hipcc, flags, extra, only, keep)


def report(src, hipcc, flags, extra, only, keep):
    with tempfile.TemporaryDirectory() as td:
        out = Path(keep) if keep else Path(td) / "out.s"
        subprocess.run([hipcc, *flags, *extra, "-fvisibility=hidden", "-S", "--cuda-device-only", str(src), "-o", str(out)],
                       check=True)
        asm = out.read_text()
    funcs, meta = parse_functions(asm), parse_metadata(asm)
    syms = [s for s in funcs if s in meta]
    rows = [(sym, name) for sym, name in zip(syms, demangle(syms))
            if not only or name.split("<")[0].split()[-1] in only]  # a template's name: "void kernel<...>"
    if not rows:
        return
    print(f"# {src.name}: static gfx950 instruction counts (scripts/isa_count.py)")
    print(f"# flags: {' '.join(flags + extra)}")
    print(f"{'kernel':44s} {'valu':>5s} {'scal':>5s} {'lds':>4s} {'vmem':>4s} {'barr':>4s} {'vgpr':>4s} {'sspill':>6s} "
          f"{'vspill':>6s} {'lds_B':>6s}")
    for sym, name in rows:
        insts, loops = funcs[sym]
        c, m = count(insts), meta[sym]
        print(f"{name[:44]:44s} {c['valu']:5d} {c['scalar']:5d} {c['lds']:4d} {c['vmem']:4d} {c['barrier']:4d} "
              f"{m.get('.vgpr_count', 0):4d} {m.get('.sgpr_spill_count', 0):6d} {m.get('.vgpr_spill_count', 0):6d} "
              f"{m.get('.group_segment_fixed_size', 0):6d}")
        for label in loops:
            b = count([i for i in insts if i[1] == label])
            first = next(n for n, i in enumerate(insts) if i[1] == label)
            ahead = count(insts[:first])
            print(f"    loop {label:12s} {'':27s} {b['valu']:5d} {b['scalar']:5d} {b['lds']:4d} {b['vmem']:4d} {b['barrier']:4d}"
                  f"  (ahead of it: valu {ahead['valu']}, scal {ahead['scalar']})")

if __name__ == "__main__":
    main()
