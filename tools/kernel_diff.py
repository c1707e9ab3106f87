"""Are the GPU kernels of two builds the same?  Per kernel: `same`, or the first line that differs.
    python tools/kernel_diff.py OLD NEW [substring ...]
OLD / NEW are files of the same kind: device assembly (hipcc --cuda-device-only -S) or HIP objects (.o; their gfx950
code object is taken out as tools/kernel_regs.py does and disassembled).  Either side may be several files, comma-separated
(a unit that was split: gz_conv.o against gz_conv.o,gz_conv_fwd.o,...): its functions are the union over them, and a
function that two files of one side hold must be identical in both -- reported otherwise.  Compared per function: the instruction
stream -- comments, addresses and the .ident line dropped, local labels numbered per function in order of appearance so
that neither function order nor label numbering matters -- and per kernel also its descriptor: the .amdhsa_* block
(assembly) and the metadata note (register counts, scratch, LDS, kernarg bytes).  A plain text diff: it knows nothing
about particular instructions.  Exit status 1 if a name is missing on one side or a function differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin/")
META = ("agpr_count", "vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def metadata(text, out):
    """`.name:` blocks of the amdgpu metadata (the same YAML in an assembly file and in readelf's notes)."""
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            out.setdefault(name.group(1), []).extend(
                "%s %s" % (k, m.group(1)) for k in META for m in [re.search(r"\.%s:\s+(\S+)" % k, blk)] if m)


def relabel(lines):
    seen = {}
    # (a disassembled object numbers its labels through the whole code object, `<L123>:` where defined and `L123` as a
    # branch operand: both are one label)
    sub = lambda m: seen.setdefault(m.group(0).strip("<>"), ".L%d" % len(seen))      # noqa: E731
    return [re.sub(r"\.L[\w$.]+|<L\d+>|\bL\d+\b", sub, ln) for ln in lines]


def from_asm(path):
    funcs, desc, cur, body = {}, {}, None, None
    text = open(path).read()
    for raw in text.split("\n"):
        ln = re.sub(r"\s+", " ", raw.split(";")[0]).strip()
        if not ln or ln.startswith(".ident"):
            continue
        m = re.match(r"\.amdhsa_kernel (\S+)", ln)
        if m:
            cur = desc.setdefault(m.group(1), [])
        elif ln == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None:
            cur.append(ln)
        elif re.match(r"\.type \S+,@function", ln):
            body = funcs.setdefault(ln.split()[1].split(",")[0], [])
        elif re.match(r"\.Lfunc_end\d+:", ln):
            body = None
        elif body is not None and not re.match(r"\.(p2align|section|globl|protected|weak|hidden|text|type|size)\b", ln):
            body.append(ln)
    metadata(text, desc)
    return {k: relabel(v) for k, v in funcs.items()}, desc


def from_obj(path):
    d = tempfile.mkdtemp()
    run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout      # noqa: E731
    run(LLVM + "llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, d + "/fat.bin")
    run(LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + d + "/fat.bin",
        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + d + "/k.co")
    funcs, desc, body = {}, {}, None
    for raw in run(LLVM + "llvm-objdump", "-d", "--symbolize-operands", "--no-show-raw-insn", "--no-leading-addr",
                   d + "/k.co").split("\n"):
        m = re.match(r"[0-9a-f]* ?<([^>]+)>:$", raw.strip())
        ln = re.sub(r"\s+", " ", raw.split("//")[0]).strip()
        if m and not re.match(r"L\d+$", m.group(1)):
            body = funcs.setdefault(m.group(1), [])
        elif ln.startswith("s_code_end"):      # (what follows is padding up to the next function)
            body = None
        elif body is not None and ln and ln != "...":      # ("...": zero bytes objdump skips, after a file's last function)
            body.append(ln)
    metadata(run(LLVM + "llvm-readelf", "--notes", d + "/k.co"), desc)
    return {k: relabel(v) for k, v in funcs.items()}, desc


def load(paths):
    """The union over the comma-separated files of one side.  A function that several of them hold (a template two units
    instantiate) must be the same in each: returns also the names where it is not, with the first difference."""
    funcs, desc, clash = {}, {}, {}
    for path in paths.split(","):
        f, d = from_obj(path) if path.endswith(".o") else from_asm(path)
        for name in f:
            if name in funcs:
                diff = first_diff(desc.get(name, []), d.get(name, []))
                diff = "descriptor " + diff if diff else first_diff(funcs[name], f[name])
                if diff:
                    clash.setdefault(name, "differs between files of %s (%s): %s" % (paths, path, diff))
        for k, v in f.items():
            funcs.setdefault(k, v)
        for k, v in d.items():
            desc.setdefault(k, v)
    return funcs, desc, clash


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: `%s` / `%s`" % (i + 1, x, y)
    return None if len(a) == len(b) else "length %d / %d lines" % (len(a), len(b))


def main():
    old, new, pats = sys.argv[1], sys.argv[2], sys.argv[3:]
    (fo, do, co), (fn, dn, cn) = load(old), load(new)
    bad = n_same = 0
    for name in sorted(set(fo) | set(fn)):
        if pats and not all(p in name for p in pats):
            continue
        if name in co or name in cn:
            verdict = co.get(name) or cn[name]
        elif name not in fo or name not in fn:
            verdict = "only in " + (old if name in fo else new)
        else:
            d = first_diff(do.get(name, []), dn.get(name, []))
            verdict = "descriptor " + d if d else first_diff(fo[name], fn[name])
        bad += verdict is not None
        n_same += verdict is None
        print("%s  %s" % (verdict or "same", name))
    print("%d functions (%d kernels): %d same, %d not" % (n_same + bad, len(set(do) | set(dn)), n_same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
