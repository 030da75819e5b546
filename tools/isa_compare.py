"""Development tool: is the device code of two builds the same, kernel by kernel?

usage: isa_compare.py DIR_A DIR_B      (csrc/_build/ as build.sh leaves it, or two STEREO_HIP_TMP directories)

Pairs the *-hip-amdgcn-amd-amdhsa-gfx950.s files of the two directories, splits each at its function symbols (kernels
and the device functions that are not inlined), drops .file / .loc / .ident and comment lines, and prints per function
`same` or the first differing line, with the SGPR / VGPR / spill / scratch / LDS figures of both sides.  Exit status 1
if anything differs or a symbol exists on one side only.  Files that exist on one side only (a source file was split
or renamed) are not an error by themselves: their functions are paired by demangled name across files.

This is how a refactor of the sweep kernel files is checked: textual sharing must leave every kernel
`same`.  Local labels (.LBB<function number>_<block>, ...) are renumbered in order of appearance: the number of a
function within its file changes when the kernels are instantiated in another order, its code does not.
"""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr

SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
DROP = re.compile(r"^\s*(\.file|\.loc|\.ident)\b|^\s*;|^\s*$")
LOCAL = re.compile(r"\.L[A-Za-z_]+[0-9_]*")


def functions(txt):
    """{symbol: [normalised lines]}: from a symbol's .type line to its .size line (kernel descriptor included), plus its
    .set lines"""
    out, cur, name = {}, None, None
    for line in txt.split("\n"):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, cur = m.group(1), []
            out[name] = cur
        if DROP.match(line):
            continue
        line = re.sub(r"\s*;.*$", "", line)
        if cur is not None:
            cur.append(line)
            if re.match(r"\s*\.size\s+%s," % re.escape(name), line):
                cur = None
        elif name is not None and re.match(r"\s*\.set\s+%s\." % re.escape(name), line):
            out[name].append(line)
    for lines in out.values():
        names = {}
        lines[:] = [LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), l) for l in lines]
    return out


def compare(where, sym_a, sym_b, fa, fb, ra, rb):
    """one function of either side; 1 if it differs.  Its own symbol is written <self>: a kernel whose argument types
    changed namespace has another mangled name and the same code."""
    name = kr.demangle(sym_a)[:140]
    fig = [kr.figures(r[s]) if s in r else "(device function)" for r, s in ((ra, sym_a), (rb, sym_b))]
    la, lb = [l.replace(sym_a, "<self>") for l in fa[sym_a]], [l.replace(sym_b, "<self>") for l in fb[sym_b]]
    if la == lb and fig[0] == fig[1]:
        print("%s: %s: same  [%s]" % (where, name, fig[0]))
        return 0
    i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
    print("%s: %s: DIFFERS at line %d of %d / %d" % (where, name, i, len(la), len(lb)))
    print("    a: %s\n    b: %s" % (la[i].strip() if i < len(la) else "(end)", lb[i].strip() if i < len(lb) else "(end)"))
    print("    a: %s\n    b: %s" % (fig[0], fig[1]))
    return 1


def plain_name(sym):
    """what pairs a symbol across files: its demangled name without the anonymous namespaces"""
    return kr.demangle(sym).replace("(anonymous namespace)::", "")


def main(dir_a, dir_b):
    files = [{os.path.basename(f) for f in glob.glob(os.path.join(d, "*" + SUFFIX))} for d in (dir_a, dir_b)]
    bad = total = 0
    for f in sorted(files[0] & files[1]):
        txt = [open(os.path.join(d, f)).read() for d in (dir_a, dir_b)]
        fa, fb = functions(txt[0]), functions(txt[1])
        ra, rb = kr.kernels(txt[0]), kr.kernels(txt[1])
        for sym in sorted(set(fa) | set(fb)):
            total += 1
            if sym not in fa or sym not in fb:
                print("%s: %s: only in %s" % (f[:-len(SUFFIX)], kr.demangle(sym)[:140], dir_a if sym in fa else dir_b))
                bad += 1
                continue
            bad += compare(f[:-len(SUFFIX)], sym, sym, fa, fb, ra, rb)
    # files of one side only (a file was split or renamed): their functions are paired by name, whatever file they are in
    loose = []
    for d, only in ((dir_a, files[0] - files[1]), (dir_b, files[1] - files[0])):
        fn, res, names = {}, {}, {}
        for f in sorted(only):
            txt = open(os.path.join(d, f)).read()
            fn.update(functions(txt)); res.update(kr.kernels(txt))
        for sym in fn:
            names[plain_name(sym)] = sym
        loose.append((fn, res, names))
    (fa, ra, na), (fb, rb, nb) = loose
    for name in sorted(set(na) | set(nb)):
        total += 1
        if name not in na or name not in nb:
            print("(by name) %s: only in %s" % (name[:140], dir_a if name in na else dir_b))
            bad += 1
            continue
        bad += compare("(by name)", na[name], nb[name], fa, fb, ra, rb)
    print("%d functions, %d differ or are missing" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
