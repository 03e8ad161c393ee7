#!/usr/bin/env python
"""Resource report of every kernel in a device assembly file (hipcc -S --cuda-device-only), optionally against a second file:

    python tools/kernel_resources.py new.s [parent.s]

Per kernel: VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes, instructions, and a digest of the instruction stream (labels renumbered,
comments dropped).  With a second file the last column says whether the kernel's code is the same in both, differs, or is new."""
import hashlib
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        return dict(zip(names, out))
    except OSError:
        return {n: n for n in names}


def kernels(path):
    text = open(path).read()
    res = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\s*s_endpgm", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if not name.startswith("_Z"):
            continue
        labels = {}
        code = []
        for ln in body.splitlines():
            ln = ln.split(";")[0].strip()
            if not ln or ln.startswith(".") and not ln.startswith(".LBB"):
                continue
            code.append(ln)
        joined = "\n".join(code)
        for lab in re.findall(r"\.LBB\d+_\d+", joined):
            labels.setdefault(lab, f"L{len(labels)}")
        joined = re.sub(r"\.LBB\d+_\d+", lambda mm: labels[mm.group(0)], joined)
        res[name] = {"insts": sum(1 for c in code if not c.startswith(".LBB")), "digest": hashlib.sha256(joined.encode()).hexdigest()[:12]}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", text, re.S | re.M):
        if m.group(1) in res:
            for key, field in (("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size")):
                mm = re.search(rf"\.amdhsa_{field} (\d+)", m.group(2))
                res[m.group(1)][key] = int(mm.group(1)) if mm else 0
    for m in re.finditer(r"- \.agpr_count:\s+(\d+)(.*?)\.name:\s+(\w+)(.*?)\.sgpr_count:\s+(\d+)(.*?)\.vgpr_count:\s+(\d+)", text, re.S):
        if m.group(3) in res:
            res[m.group(3)].update(agpr=int(m.group(1)), sgpr=int(m.group(5)), vgpr=int(m.group(7)))
    return res


def main():
    new = kernels(sys.argv[1])
    old = kernels(sys.argv[2]) if len(sys.argv) > 2 else None
    names = demangle(sorted(new))
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>7} {'insts':>7}  {'code':12} {'vs parent':10} kernel")
    counts = {}
    for n in sorted(new):
        k = new[n]
        if old is None:
            verdict = ""
        elif n not in old:
            verdict = "new"
        elif old[n]["digest"] == k["digest"] and all(old[n].get(f) == k.get(f) for f in ("vgpr", "agpr", "sgpr", "scratch", "lds")):
            verdict = "same"
        else:
            verdict = "DIFFERS"
        counts[verdict] = counts.get(verdict, 0) + 1
        print(f"{k.get('vgpr', -1):5d} {k.get('agpr', -1):5d} {k.get('sgpr', -1):5d} {k.get('scratch', -1):8d} {k.get('lds', -1):7d} {k['insts']:7d}  "
              f"{k['digest']:12} {verdict:10} {names[n]}")
    if old is not None:
        gone = sorted(set(old) - set(new))
        print(f"# {len(new)} kernels: " + ", ".join(f"{v} {k}" for k, v in sorted(counts.items())) + f"; {len(gone)} of the parent's are gone")
        for n in gone:
            print(f"# gone: {n}")


if __name__ == "__main__":
    main()
