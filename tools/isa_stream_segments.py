"""The segment kernels' assembly at two builds, compared kernel by kernel: the
recipe behind profiles/stream_segments_sessions/isa.md.  No GPU is needed.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S \
        vad_amd/csrc/stream_segments_kernel.hip -o new.s      # and the same at the parent commit: parent.s
    python tools/isa_stream_segments.py parent.s new.s

Per kernel of the first file: the text between its entry label and its
.Lfunc_end label, with every line dropped whose first non-blank character is
';' (a comment) or '.' (a directive) unless it is a basic-block label (.LBB...);
"lines" is the number of lines left (instructions and block labels), and the
two builds' texts are compared as strings.  The resource figures are those of
the amdhsa.kernels metadata.  Kernels only the second file has are listed with
their figures.
"""
import re
import subprocess
import sys

FIELDS = dict(lds="group_segment_fixed_size", kernarg="kernarg_segment_size", scratch="private_segment_fixed_size",
              sgpr="sgpr_count", vgpr="vgpr_count", sgpr_spill="sgpr_spill_count", vgpr_spill="vgpr_spill_count")


def kernels(path):
    text = open(path).read()
    body = {}
    for m in re.finditer(r"^(_ZN3vad\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        keep = [ln for ln in m.group(2).split("\n")
                if not ln.strip().startswith((";", ".")) or ln.strip().startswith(".LBB")]
        body[m.group(1)] = "\n".join(keep)
    meta = {}
    for blk in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name and ".vgpr_count" in blk:
            meta[name.group(1)] = {k: int(re.search(r"\." + f + r":\s+(\d+)", blk).group(1)) for k, f in FIELDS.items()}
    return body, meta


def demangle(name):
    out = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return out.replace("void vad::(anonymous namespace)::", "").split("(")[0]


def main():
    (old, old_meta), (new, new_meta) = kernels(sys.argv[1]), kernels(sys.argv[2])
    for k in old:
        same = old[k] == new.get(k) and old_meta[k] == new_meta.get(k)
        print("old", demangle(k), len(old[k].split("\n")), "lines", "identical" if same else "DIFFERENT", old_meta[k])
    for k in new:
        if k not in old:
            print("new", demangle(k), len(new[k].split("\n")), "lines", new_meta[k])
    return 0 if all(old[k] == new.get(k) for k in old) else 1


if __name__ == "__main__":
    sys.exit(main())
