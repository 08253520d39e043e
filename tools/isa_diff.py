#!/usr/bin/env python3
"""Compare two gfx950 assembly listings function by function.

    hipcc <build.py's HIP_FLAGS> --save-temps ... pcr_api.hip      # once per tree: writes pcr_api-hip-amdgcn-amd-amdhsa-gfx950.s
    tools/isa_diff.py parent.s new.s

Prints the functions that are missing, new or whose instruction stream differs (comments stripped, the function number taken out
of local labels), and every change in the per-function resource comments. Exit status 1 on any difference.
"""
import re
import sys

START = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @\1\s*$")
RESOURCES = ("NumVgprs", "NumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")
RESOURCE = re.compile(r"^; (%s): (\S+)" % "|".join(RESOURCES))
LABEL = re.compile(r"\.L(BB|JTI|func_end|func_begin|tmp)\d+")


def functions(path):
    """name -> (body lines, {resource: value}); the resource comments follow the body up to the next function."""
    out, name, in_body = {}, None, False
    for line in open(path):
        m = START.match(line)
        if m:
            name, in_body = m.group(1), True
            out[name] = ([], {})
            continue
        if name is None:
            continue
        r = RESOURCE.match(line)
        if r:
            out[name][1][r.group(1)] = r.group(2)
        if line.startswith(".Lfunc_end"):
            in_body = False
        code = LABEL.sub(r".L\1", line.split(";", 1)[0]).strip()
        if in_body and code:
            out[name][0].append(code)
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("%s: %s" % ("new" if name not in a else "missing", name)); bad += 1
            continue
        if a[name][0] != b[name][0]:
            print("differs: %s (%d -> %d lines)" % (name, len(a[name][0]), len(b[name][0]))); bad += 1
        for k in RESOURCES:
            if a[name][1].get(k) != b[name][1].get(k):
                print("%s of %s: %s -> %s" % (k, name, a[name][1].get(k), b[name][1].get(k))); bad += 1
    print("%d functions in %s, %d in %s, %d differences" % (len(a), sys.argv[1], len(b), sys.argv[2], bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
