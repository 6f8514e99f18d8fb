#!/usr/bin/env python
"""Compare this tree's gfx950 kernels with another build's, instruction for instruction.

    python tools/code_object_diff.py OTHER_CSRC_DIR [--debug]

OTHER_CSRC_DIR is the caspr_amd/csrc directory of another checkout (say, the parent commit) that was built with the same compiler by
its own build.py.  For every object of build.SOURCES and every kernel in it, the instruction list (mnemonic and operands; addresses
and encodings stripped) and the metadata entry (register counts, scratch, LDS, spill counts, arguments) are compared.  One line per
kernel; the exit status is non-zero on any difference.  --debug compares the CASPR_BUILD_DEBUG=1 objects (*.dbg.o)."""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from caspr_amd.csrc import audit, build  # noqa: E402


def kernels(obj):
    """-> {kernel symbol: (metadata entry, instruction list)} of one object.  audit._kernel's list ends at the first s_endpgm; a kernel
    with an early return has several, so the list here runs to the next symbol."""
    notes, dis = audit._code_object(obj)
    body = {m.group(1): m.group(2) for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", dis, re.M | re.S)}
    names = re.findall(r"^\s*(?:- )?\.name:\s+(\S+)\s*$", notes, re.M)
    return {k: (audit._kernel(notes, dis, k)[0], [ln.split("//")[0].strip() for ln in body[k].splitlines() if ln.startswith("\t")])
            for k in names if k in body}   # (argument entries carry .name: lines too)


def main(argv):
    debug = "--debug" in argv
    other = [a for a in argv if not a.startswith("--")]
    if len(other) != 1:
        sys.exit(__doc__)
    suffix = ".dbg.o" if debug else ".o"
    bad = 0
    for s in build.SOURCES:
        mine, theirs = (kernels(os.path.join(d, s.replace(".hip", suffix))) for d in (build.HERE, other[0]))
        for k in sorted(set(mine) | set(theirs)):
            if k not in mine or k not in theirs:
                print("%-24s %s: only in %s" % (s, k, "this tree" if k in mine else "the other build"))
                bad += 1
                continue
            (meta, ins), (ometa, oins) = mine[k], theirs[k]
            what = []
            if ins != oins:
                n = next((i for i, (x, y) in enumerate(zip(ins, oins)) if x != y), min(len(ins), len(oins)))
                what.append("instruction %d: `%s` here, `%s` there (%d / %d instructions)" % (n, (ins + ["<end>"])[n], (oins + ["<end>"])[n], len(ins), len(oins)))
            if meta != ometa:
                what.append("metadata: " + "; ".join("%s | %s" % (x.strip(), y.strip()) for x, y in zip(meta.splitlines(), ometa.splitlines()) if x != y))
            bad += bool(what)
            print("%-24s %s: %d instructions, %s" % (s, k, len(ins), "DIFFERENT, " + " / ".join(what) if what else "identical"))
    print("%d kernel(s) differ" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
