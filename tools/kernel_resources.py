"""Compare per-kernel resource use between two builds of libkth.so.

    make -C mpi-k-selection_amd clean all \
        HIPFLAGS='-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-result \
                  -Rpass-analysis=kernel-resource-usage' 2> build.log
    python tools/kernel_resources.py parent.log this.log > profiles/f32_kernel_resources.txt

Kernels are matched by their demangled names with the key-kind template
argument (the trailing `false` of the int32 instantiations, absent in a build
from before float32 keys) removed; the float32 instantiations (`true`) are
listed beside their int32 twins.  Exit status 1 when an int32 kernel's figures
differ between the two logs, a float32 kernel uses more scratch than its
int32 twin (k_finish keeps 296 bytes a lane in both builds and both kinds), or
a float32 twin of a grid-barrier kernel (k_head, k_finish: their grids must be
co-resident) has a lower occupancy than its int32 twin.

    python tools/kernel_resources.py --list k_rows16 this.log > profiles/rows16_kernel_resources.txt

lists every kernel of one log whose name starts with the prefix, one line each;
exit status 1 when one of them uses scratch.
"""
import re
import subprocess
import sys

FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ")]
# the kernels that read the input array (every instantiation of each)
WATCH = ("k_head", "k_main", "k_finish", "k_level", "k_small", "k_topk_count", "k_topk_write", "k_gather", "k_result")


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            out[cur] = {}
            continue
        for label, key in FIELDS:
            if cur and body.startswith(label + ":"):
                out[cur][key] = body.rsplit(":", 1)[1].strip()
    return out


def demangle(names):
    if not names:
        return {}
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def short(dem):
    """`void kth::k_main<0, false>(args)` -> (`k_main<0>`, kind) with kind in {None, False, True}"""
    m = re.match(r"(?:void )?kth::(\w+)(?:<(.*?)>)?\(", dem)
    if not m:
        return None, None
    name, targs = m.group(1), m.group(2)
    args = [a.strip() for a in targs.split(",")] if targs else []
    kind = None
    # The key kind is the LAST template argument of the kernels that have one.
    # The int32-only parent build has one argument fewer, so a trailing
    # true / false is taken as the key kind only at the arity given here: this
    # table repeats each kernel's template arity and must follow it when a
    # kernel gains or loses a template parameter (a mismatch shows as
    # "(not built)" rows in the output, not as a wrong comparison).
    has_kind = {"k_head": 1, "k_main": 2, "k_finish": 1, "k_level": 2, "k_small": 1, "k_topk_count": 3,
                "k_topk_write": 3, "k_gather": 2, "k_result": 1}
    if name in has_kind and len(args) == has_kind[name] and args[-1] in ("true", "false"):
        kind = args.pop() == "true"
    return name + ("<" + ", ".join(args) + ">" if args else ""), kind


def table(path):
    raw = parse(path)
    dem = demangle(list(raw))
    t = {}
    for mangled, vals in raw.items():
        key, kind = short(dem[mangled])
        if key and key.split("<")[0] in WATCH:
            t[(key, bool(kind))] = vals
    return t


def fmt(v):
    return " ".join(f"{k} {v.get(k, '?'):>5s}" for _, k in FIELDS) if v else "(not built)"


def list_kernels(prefix, path):
    """One line per kernel of `path` whose name starts with `prefix`; status 1 when one uses scratch."""
    raw = parse(path)
    dem = demangle(list(raw))
    bad = 0
    for mangled in sorted(raw, key=lambda m: dem[m]):
        m = re.match(r"(?:void )?kth::(\w+(?:<.*?>)?)\(", dem[mangled])
        if m and m.group(1).startswith(prefix):
            print(f"{m.group(1):40s} {fmt(raw[mangled])}")
            bad |= raw[mangled].get("scratch", "0") != "0"
    return bad


def main():
    if sys.argv[1] == "--list":  # kernel_resources.py --list k_rows16 this.log
        return list_kernels(sys.argv[2], sys.argv[3])
    parent, this = table(sys.argv[1]), table(sys.argv[2])
    bad = 0
    for key in sorted({k for k, _ in this} | {k for k, _ in parent}):
        p, t, f = parent.get((key, False)), this.get((key, False)), this.get((key, True))
        same = p == t
        print(f"{key}")
        print(f"  int32 parent  {fmt(p)}")
        print(f"  int32 this    {fmt(t)}   {'equal' if same else 'DIFFERENT'}")
        if f is not None:
            fs, ts = int(f.get("scratch", "0")), int((t or {}).get("scratch", "0"))
            note = "" if fs == 0 else "   scratch as its int32 twin" if fs <= ts else "   MORE SCRATCH THAN int32"
            print(f"  float32 this  {fmt(f)}{note}")
            bad |= fs > ts
            if key.split("<")[0] in ("k_head", "k_finish") and int(f.get("occ", "0")) < int((t or {}).get("occ", "0")):
                print("  float32 this  LOWER OCCUPANCY THAN int32 (cooperative grid)")
                bad = 1
        bad |= not same
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
