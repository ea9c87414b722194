#!/usr/bin/env python3
"""One line per device function of libmlmcpi_hip.so: name, SHA-1 of its instructions, resource directives.

A refactor that promises to leave the generated kernels alone runs this before and after and diffs the two outputs:

    python tools/kernel_digest.py > after.txt          # (before.txt: the same script in a checkout of the parent)
    diff before.txt after.txt

Every .hip file the Makefile compiles is compiled again with the Makefile's own command line, `-c` replaced by
`--cuda-device-only -S`; nothing is linked or run, no GPU is needed.  The assembly is split by function (kernels and the
device functions that were not inlined).  Only what depends on a function's POSITION in its translation unit is
normalised: the function index in `.LBB<n>_<m>` and `.Lfunc_end<n>`, the unit-wide `.Ltmp<n>` counter (renumbered in order
of appearance inside the function), comments, and the `.file` directive.  The lines are sorted by name, so which file a
function lives in does not show.  A device function that is not inlined is emitted into the code object of every unit that
calls it; identical copies print as one line (a copy that differs in anything prints as a second line).

Columns: name  sha1  next_free_vgpr  next_free_sgpr  accum_offset  group_segment_fixed_size  private_segment_fixed_size
(`-` for a function that is not a kernel: it has no kernel descriptor).
"""
import argparse
import concurrent.futures
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlmcpathintegral_amd", "csrc")
RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def compile_commands(csrc, make_args):
    """The Makefile's compile lines for the objects of the library (make -n -B: printed, not run)."""
    out = subprocess.run(["make", "-C", csrc, "-n", "-B"] + make_args, check=True, capture_output=True, text=True).stdout
    cmds = []
    for line in out.splitlines():
        words = shlex.split(line)
        if "-c" in words and any(w.endswith(".hip") for w in words):
            cmds.append(words)
    if not cmds:
        sys.exit("kernel_digest: no compile command for a .hip file in the output of make -n")
    return cmds


def assembly(words, tmp):
    src = next(w for w in words if w.endswith(".hip"))
    dst = os.path.join(tmp, os.path.basename(src)[:-4] + ".s")
    cmd, skip = [], False
    for w in words:
        if skip:
            skip = False
        elif w == "-o":
            skip = True
        elif w == "-c":
            cmd += ["--cuda-device-only", "-S"]
        else:
            cmd.append(w)
    subprocess.run(cmd + ["-o", dst], check=True, stderr=subprocess.DEVNULL)
    with open(dst) as f:
        return f.read()


def functions(asm):
    """(name, normalised instruction text, {directive: value}) of every function of one unit's assembly."""
    lines = asm.splitlines()
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        i += 1
        if not m:
            continue
        name, body, res, tmps, in_descriptor = m.group(1), [], {}, {}, False
        while not re.match(r"\.Lfunc_end\d+:", lines[i]):
            text = lines[i].split(";", 1)[0].rstrip()   # comments
            i += 1
            if re.match(r"\s*\.section\s+\.rodata", text):   # a kernel's descriptor sits inside its function
                in_descriptor = True
            elif in_descriptor:
                d = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", text)
                if d and d.group(1) in RESOURCES:
                    res[d.group(1)] = d.group(2)
                if re.match(r"\s*\.text\b", text):
                    in_descriptor = False
            elif text.strip() and not re.match(r"\s*\.file\b", text):
                text = re.sub(r"\.LBB\d+_", ".LBB_", text)
                text = re.sub(r"\.Ltmp\d+", lambda t: tmps.setdefault(t.group(0), ".Ltmp%d" % len(tmps)), text)
                body.append(text)
        yield name, "\n".join(body), res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=CSRC, help="directory of the Makefile and the .hip files")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("make_args", nargs="*", help="passed to make, e.g. EXTRA=-DMLMCPI_STAMPS")
    args = ap.parse_args()
    cmds = compile_commands(args.csrc, args.make_args)
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        units = list(pool.map(lambda w: assembly(w, tmp), cmds))
    rows = set()
    for asm in units:
        for name, body, res in functions(asm):
            rows.add(" ".join([name, hashlib.sha1(body.encode()).hexdigest()] + [res.get(k, "-") for k in RESOURCES]))
    print("\n".join(sorted(rows)))
    kernels = sum(1 for r in rows if not r.endswith(" -"))
    print("kernel_digest: %d functions in %d units: %d kernels, %d other device functions" %
          (len(rows), len(units), kernels, len(rows) - kernels), file=sys.stderr)


if __name__ == "__main__":
    main()
