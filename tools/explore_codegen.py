"""Code generation of the exploring families' device code, two builds compared
(DESIGN.md §3): writes profiles/explore_unify/codegen.txt.

Each build is a directory that holds, for every unit paxos_explore{,_cover,_win}
of P = 1, 2, 3, the unit compiled with build()'s flags plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`: NAME_pP.s (the
assembly) and NAME_pP.remarks (the compiler's standard error).  Kernels are
matched by unit and role (candidate kernel of a shape, minimal, init, finish,
cursor, scatter), not by name.  Per kernel: every line of the resource remark
(SGPRs, VGPRs, AGPRs, spills, scratch, LDS, occupancy) and the number of
instructions of its body; for an equal count, whether the sequence is the same.

python tools/explore_codegen.py BASE_DIR HEAD_DIR [--out PATH]"""
import argparse
import collections
import os
import re
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ["paxos_%s_p%d" % (f, p) for f in ("explore", "explore_cover", "explore_win") for p in (1, 2, 3)]
CXXFILT = os.environ.get("CXXFILT", "c++filt")
ROLES = (("minimal_kernel", "minimal"), ("reach_init_kernel", "init"), ("reach_finish_kernel", "finish"),
         ("cursor_kernel", "cursor"), ("scatter_kernel", "scatter"))


def role_of(unit, demangled):
    """'candidate <PM, N, W, LG>' or one of ROLES' names."""
    if "_win_" in unit and "minimal_kernel" in demangled and "win_minimal" not in demangled and "ExploreWinX" not in demangled:
        return "minimal, link space (never launched by this unit)"
    for sub, role in ROLES:
        if sub in demangled:
            return role
    m = re.search(r"paxos_explore\w*_kernel<(?:[\w:]+X, )?(\d+), (\d+), (\d+), (\w+)>", demangled)
    if not m:                                          # (hipCUB's own kernels: by name)
        return "library %08x" % zlib.crc32(demangled.encode())
    return "candidate <%s, %s, %s, %s>" % m.groups()


def read_unit(d, unit):
    """{role: (resources dict, [instruction mnemonic + operands])}"""
    res, cur = {}, None
    for line in open(os.path.join(d, unit + ".remarks")):
        m = re.search(r"remark: +(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(": ")
        if k == "Function Name":
            cur = res.setdefault(v.strip(), collections.OrderedDict())
        elif cur is not None and v:
            cur[k.strip()] = v.strip()
    body, name = {}, None
    for line in open(os.path.join(d, unit + ".s")):
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in res:
            name = m.group(1)
            body[name] = []
        elif name and re.match(r"^\.Lfunc_end", line):
            name = None
        elif name and re.match(r"^\t[a-z]\w+", line):
            # (labels carry the function's index in its unit: .LBB14_7)
            body[name].append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", line.strip())))
    names = list(res)
    dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, dn in zip(names, dem):
        r = role_of(unit, dn)
        assert r not in out, (unit, r)
        out[r] = (res[n], body[n])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("head")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explore_unify", "codegen.txt"))
    a = ap.parse_args()
    lines, unequal, total = [], [], 0
    for unit in UNITS:
        b, h = read_unit(a.base, unit), read_unit(a.head, unit)
        for role in sorted(set(b) | set(h)):
            if role not in b or role not in h:
                # (a kernel of one build only: e.g. a unit that no longer emits a kernel it never launched)
                lines.append("%-22s %-28s only in %s" % (unit, role, "base" if role in b else "head"))
                continue
            total += 1
            (rb, ib), (rh, ih) = b[role], h[role]
            same_res, same_n = rb == rh, len(ib) == len(ih)
            order = "same sequence" if ib == ih else "same multiset" if sorted(ib) == sorted(ih) else "other text"
            tag = "EQUAL" if same_res and same_n else "DIFFERS"
            if tag == "DIFFERS":
                unequal.append((unit, role))
            lines.append("%-22s %-28s %-7s sgpr %s/%s vgpr %s/%s spill %s+%s/%s+%s scratch %s/%s lds %s/%s occ %s/%s "
                         "instr %d/%d (%s)" % (
                             unit, role, tag, rb.get("TotalSGPRs"), rh.get("TotalSGPRs"), rb.get("VGPRs"), rh.get("VGPRs"),
                             rb.get("SGPRs Spill"), rb.get("VGPRs Spill"), rh.get("SGPRs Spill"), rh.get("VGPRs Spill"),
                             rb.get("ScratchSize [bytes/lane]"), rh.get("ScratchSize [bytes/lane]"),
                             rb.get("LDS Size [bytes/block]"), rh.get("LDS Size [bytes/block]"),
                             rb.get("Occupancy [waves/SIMD]"), rh.get("Occupancy [waves/SIMD]"), len(ib), len(ih), order))
    head = ["# base/head per kernel; EQUAL: every resource line and the instruction count are equal",
            "# %d kernels in both builds, %d differ%s" % (total, len(unequal), "".join("\n#   %s %s" % u for u in unequal))]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    print("\n".join(head))
    return 1 if unequal else 0


if __name__ == "__main__":
    sys.exit(main())
