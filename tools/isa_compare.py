#!/usr/bin/env python3
"""Device-code comparison of two source trees:  isa_compare.py PARENT_CSRC THIS_CSRC [--merged OLD=NEW ...]  (needs hipcc, no GPU).

Every *.hip of both csrc directories is compiled with its Makefile's flags for the device only and disassembled; addresses are
stripped, branch targets replaced by a placeholder, and the text is split per kernel symbol.  Kernels are paired by mangled name
across ALL objects of a tree (a kernel may move between files) and reported as identical / differing / added / lost / emitted by
more than one object.  Each file of THIS_CSRC is also compiled in full to check that every device kernel has its host-side stub
(hipcc can drop the host instantiation of a kernel template silently; the kernel is then undefined at load time).
--merged OLD=NEW (repeatable) declares that this tree folds duplicates: the identifier OLD in a kernel's name (a kernel, or a
type one is instantiated over) is now NEW.  A lost kernel whose renamed name is a kernel of this tree with the same normalised
disassembly is MERGED into it, many old names to one new one; a lost kernel without such a partner stays LOST, and an added kernel
that no lost one merges into stays ADDED.
Exit status 0: every kernel of the parent is present once and identical or merged, none is added, no stub is missing."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def flags(csrc):
    """CXXFLAGS of csrc/Makefile with its variables expanded ($(EXTRA) empty)"""
    mk = open(os.path.join(csrc, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", mk, re.M))
    out = var["CXXFLAGS"]
    for _ in range(4):
        out = re.sub(r"\$\((\w+)\)", lambda m: "" if m.group(1) == "EXTRA" else var.get(m.group(1), ""), out)
    return var.get("HIPCC", "hipcc"), out.split()


def run(cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def symbols(obj):
    return {line.split()[-1] for line in run([OBJDUMP, "-t", obj]).splitlines() if line[:1].isalnum() and len(line.split()) > 3}


def kernels_of(csrc, src, tmp, full):
    """{mangled kernel name: normalised disassembly} of one source file; with full also the kernels that lack a host stub"""
    hipcc, fl = flags(csrc)
    obj = os.path.join(tmp, src + ".dev.o")
    run([hipcc, *fl, "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj], cwd=csrc)
    # kernel symbols: the functions that have a kernel descriptor NAME.kd next to them
    names = {s[:-3] for s in symbols(obj) if s.endswith(".kd")}
    text, cur, out = run([OBJDUMP, "-d", "--no-show-raw-insn", obj]), None, {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1) if m.group(1) in names else None
            if cur:
                out[cur] = []
            continue
        if cur is None or not line.strip() or line.strip() in ("...", "s_code_end"):     # padding behind an object's last kernel
            continue
        line = re.sub(r"\s*//.*$", "", line).strip()                                  # the address comment
        line = re.sub(r"^(s_c?branch\w*|s_call\w*)\s+.*$", r"\1 <target>", line)
        out[cur].append(line)
    missing = []
    if full:
        host = os.path.join(tmp, src + ".o")
        run([hipcc, *fl, "-c", src, "-o", host], cwd=csrc)
        # the stub of kernel <len>name... is mangled <len + 15>__device_stub__name...
        unstub = lambda m: (str(int(m.group(1)) - 15) if m.group(1) else "")
        stubs = {re.sub(r"(\d+)?__device_stub__", unstub, s) for s in symbols(host) if "__device_stub__" in s}
        missing = sorted(names - stubs)
    return src, {k: "\n".join(v) for k, v in out.items()}, missing


def tree(csrc, tmp, full):
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    os.makedirs(tmp)
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(lambda f: kernels_of(csrc, f, tmp, full), srcs))
    where = {}
    for src, ks, _ in res:
        for k in ks:
            where.setdefault(k, []).append(src)
    code = {k: v for _, ks, _ in res for k, v in ks.items()}
    return code, where, [(src, k) for src, _, miss in res for k in miss]


def merged_into(lost, added, pc, tc, renames):
    """{lost kernel: the added kernel it is merged into} under the identifier renames [(old, new)]; an identifier is mangled as its
    length and its text, wherever it stands in a name (behind another digit only where that ends the unnamed namespace's own name)"""
    out = {}
    for k in lost:
        t = k
        for old, new in renames:
            t = re.sub(rf"(?:(?<!\d)|(?<=_GLOBAL__N_1)){len(old)}{re.escape(old)}", f"{len(new)}{new}", t)
        if t != k and t in added and pc[k] == tc[t]:
            out[k] = t
    return out


def main():
    parent, this = sys.argv[1], sys.argv[2]
    renames = [tuple(a.split("=", 1)) for f, a in zip(sys.argv[3::2], sys.argv[4::2]) if f == "--merged"]
    if len(sys.argv) % 2 == 0 or 2 * len(renames) != len(sys.argv) - 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        pc, pw, _ = tree(parent, os.path.join(tmp, "parent"), False)
        tc, tw, nostub = tree(this, os.path.join(tmp, "this"), True)
    same = sorted(k for k in pc if k in tc and pc[k] == tc[k])
    diff = sorted(k for k in pc if k in tc and pc[k] != tc[k])
    lost, added = sorted(set(pc) - set(tc)), sorted(set(tc) - set(pc))
    twice = sorted(k for k, w in tw.items() if len(w) > 1)
    merged = merged_into(lost, added, pc, tc, renames) if renames else {}
    lost, added = [k for k in lost if k not in merged], [k for k in added if k not in merged.values()]
    for src in sorted({s for w in tw.values() for s in w} | {s for w in pw.values() for s in w}):
        mine = [k for k in tc if src in tw[k]]
        moved = sorted({pw[k][0] for k in mine if k in pw and src not in pw[k]})
        print(f"{src}: {len(mine)} kernels ({sum(k in same for k in mine)} identical to the parent's"
              + (f", from {' '.join(moved)}" if moved else "") + f"); parent had {sum(src in w for w in pw.values())} here")
    for title, ks in (("DIFFERENT", diff), ("LOST", lost), ("ADDED", added), ("EMITTED TWICE", twice)):
        for k in ks:
            print(f"{title}: {k}  [{' '.join(pw.get(k, []))} -> {' '.join(tw.get(k, []))}]")
    for k, t in sorted(merged.items()):
        print(f"MERGED: {k}  [{' '.join(pw[k])}]\n     -> {t}  [{' '.join(tw[t])}]  same disassembly")
    for src, k in nostub:
        print(f"NO HOST STUB: {k}  [{src}]")
    print(f"total: parent {len(pc)} kernels; {len(same)} identical, {len(diff)} different, {len(merged)} merged into "
          f"{len(set(merged.values()))}, {len(lost)} lost, {len(added)} added, "
          f"{len(twice)} emitted twice, {len(nostub)} without host stub")
    return 0 if not (diff or lost or added or twice or nostub) and len(same) + len(merged) == len(pc) else 1


if __name__ == "__main__":
    sys.exit(main())
