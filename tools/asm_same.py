#!/usr/bin/env python3
"""Compares every kernel of two builds' gfx950 assembly (csrc/nb_engine.gfx950.s, `make asm`), labels aside.

    python tools/asm_same.py OLD.s NEW.s

A change that adds kernels of its own must leave the others instruction for instruction what they were: the function bodies are compared
line by line with comments dropped and the function's number taken out of its local labels (.LBB<fn>_<n>, .Lfunc_end<fn>: a kernel added
in front renumbers them).  Prints the kernels that differ, those only one side has, and a summary line; exit status 1 if a kernel both
sides have differs.
"""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^(_Z\w+|nb_\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name] = body
                name = None
                continue
            line = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line.strip())
            line = re.sub(r"\.Ltmp\d+", ".Ltmp", line)
            body.append(line)
    return out


def main():
    old, new = functions(sys.argv[1]), functions(sys.argv[2])
    differ = [k for k in old if k in new and old[k] != new[k]]
    for k in differ:
        print("DIFFERS  %s  (%d -> %d lines)" % (k, len(old[k]), len(new[k])))
    for k in sorted(set(old) - set(new)):
        print("ONLY OLD %s" % k)
    for k in sorted(set(new) - set(old)):
        print("ONLY NEW %s  (%d lines)" % (k, len(new[k])))
    print("%d kernels in both, %d identical, %d differ; %d only old, %d only new"
          % (len(set(old) & set(new)), len(set(old) & set(new)) - len(differ), len(differ), len(set(old) - set(new)), len(set(new) - set(old))))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
