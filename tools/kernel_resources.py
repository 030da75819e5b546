"""Development tool: register / spill / LDS / scratch figures of every kernel and device function in a saved .s file
(-save-temps).  usage: kernel_resources.py file.s [name filter]"""
import re, sys, subprocess

FIELDS = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def demangle(n):
    for tool in ("/opt/rocm/lib/llvm/bin/llvm-cxxfilt", "c++filt"):
        try: return subprocess.run([tool, n], capture_output=True, text=True).stdout.strip() or n
        except Exception: pass
    return n


def kernels(txt):
    """{mangled kernel name: {field: text}} from the amdhsa metadata of a device assembly file"""
    out = {}
    for b in re.split(r"\n  - \.agpr_count:", txt)[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, b) or [None, "?"])[1]
        out[g("name")] = {k: g(k) for k in FIELDS}
    return out


def functions(txt):
    """[(mangled name, sgprs, vgprs, scratch)] of the device functions that are not inlined: the ; NumVgprs comments"""
    return [m.groups() for m in re.finditer(
        r"\.type\s+(\S+),@function\n(?:.*\n)*?; NumSgprs: (\d+)\n; NumVgprs: (\d+)\n(?:.*\n)*?; ScratchSize: (\d+)", txt)]


def figures(r):
    return "sgpr %s spill %s | vgpr %s spill %s | scratch %s | lds %s" % tuple(r[k] for k in FIELDS)


if __name__ == "__main__":
    txt = open(sys.argv[1]).read()
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    ks = kernels(txt)
    for mangled, r in ks.items():
        name = demangle(mangled)
        if flt and flt not in name: continue
        print("%-110s %s" % (name[:110], figures(r)))
    for mangled, sgpr, vgpr, scratch in functions(txt):
        name = demangle(mangled)
        if mangled in ks or (flt and flt not in name): continue
        print("FUNC %-100s sgpr %s vgpr %s scratch %s" % (name[:100], sgpr, vgpr, scratch))
