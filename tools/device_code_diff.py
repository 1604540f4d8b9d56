"""Compare the device code of two builds of kth_api.hip, kernel by kernel.

    cd mpi-k-selection_amd
    hipcc <the Makefile's HIPFLAGS> -I../include -Icsrc --offload-device-only -S csrc/kth_api.hip -o this.s
    (the same in a checkout of the parent, -o parent.s)
    python tools/device_code_diff.py parent.s this.s > profiles/host_refactor_device_code.txt

A change to the host code alone may reorder the kernels in the listing and
renumber their local labels, so whole-file hashes differ while no instruction
does.  Here each function symbol's text, from its `.type ...,@function` line to
its `.Lfunc_end`, is compared after dropping `;` comments and the function
number inside local labels (`.LBB12_3` -> `.LBB_3`), and so is its
`.amdhsa_kernel` block.  Exit status 1 when the two sets of symbols differ or
any symbol's text or kernel descriptor does.
"""
import hashlib
import re
import sys


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    return re.sub(r"\.LBB\d+_", ".LBB_", line)


def parse(path):
    """symbol -> [cleaned body lines, cleaned .amdhsa_kernel lines]"""
    out, body, desc = {}, None, None
    for raw in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+(\S+),@function", raw)
        if m:
            body = out.setdefault(m.group(1), [[], []])[0]
            continue
        if re.match(r"\.Lfunc_end\d+:", raw):
            body = None
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", raw)
        if m:
            desc = out.setdefault(m.group(1), [[], []])[1]
            continue
        if raw.strip() == ".end_amdhsa_kernel":
            desc = None
            continue
        dst = desc if desc is not None else body
        line = clean(raw)
        if dst is not None and line.strip():
            dst.append(line)
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:12]


def main():
    parent, this = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for name in sorted(set(parent) ^ set(this)):
        print(f"ONLY IN {'parent' if name in parent else 'this'}: {name}")
        bad = 1
    for name in sorted(set(parent) & set(this)):
        (pb, pd), (tb, td) = parent[name], this[name]
        same = pb == tb and pd == td
        bad |= not same
        what = "equal" if same else "DIFFERENT" + (" text" if pb != tb else "") + (" descriptor" if pd != td else "")
        print(f"{digest(tb)} {len(tb):6d} lines  {digest(td) if td else '(no descriptor)':>15s}  {what}  {name}")
    print(f"{len(parent)} symbols in parent, {len(this)} in this build, "
          f"{sum(1 for v in this.values() if v[1])} kernel descriptors: {'DIFFERENT' if bad else 'all equal'}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
