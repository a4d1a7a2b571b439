#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files (tools/isa.sh UNIT out.s),
kernel by kernel: registers, scratch and spills from the code object's
metadata, the instruction count, and whether the instruction streams are the
same line for line (labels renumbered in order of appearance, the unit's
__hip_cuid_* symbol masked).  Prints one markdown table row per kernel of the
second file; a kernel the first file lacks is marked new.

    python tools/isa_compare.py parent.s this.s
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    except OSError:
        return {n: n for n in names}
    return dict(zip(names, out.stdout.splitlines())) if out.returncode == 0 else {n: n for n in names}


def kernels(path):
    text = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
        meta[name.group(1)] = (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"),
                               get("vgpr_spill_count"))
    body = {}
    for name in meta:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), text, re.S | re.M)
        if not m:
            continue
        lines, labels = [], {}
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith("."):
                if re.match(r"\.LBB\d+_\d+:", ln):
                    labels.setdefault(ln[:-1], "L%d" % len(labels))
                continue
            lines.append(ln)
        norm = []
        for ln in lines:
            ln = re.sub(r"\.LBB\d+_\d+", lambda t: labels.setdefault(t.group(0), "L%d" % len(labels)), ln)
            norm.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln))
        body[name] = norm
    return meta, body


def main():
    (ma, ba), (mb, bb) = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangle(sorted(mb))
    print("| kernel | VGPR | SGPR | scratch (B) | VGPR spills | instructions | stream |")
    print("|---|---|---|---|---|---|---|")
    for k in sorted(mb, key=lambda n: names[n]):
        short = re.sub(r"^void vad::(\(anonymous namespace\)::)?", "", names[k]).split("(")[0]
        if k in ma:
            cells = ["%d / %d" % (x, y) for x, y in zip(ma[k], mb[k])]
            cells.append("%d / %d" % (len(ba[k]), len(bb[k])))
            cells.append("identical" if ba[k] == bb[k] else "DIFFERENT")
        else:
            cells = ["%d" % y for y in mb[k]] + ["%d" % len(bb[k]), "new"]
        print("| `%s` | %s |" % (short, " | ".join(cells)))


if __name__ == "__main__":
    main()
