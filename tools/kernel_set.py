"""Kernels of a gfx950 assembly listing (hipcc $(CXXFLAGS) --cuda-device-only -S -o unit.s unit.hip).  CPU only.
  python tools/kernel_set.py list unit.s           one line per kernel: codeLenInByte, VGPRs, SGPRs, scratch, demangled name; totals
  python tools/kernel_set.py diff parent.s new.s   per function, the instruction stream (and its .amdhsa_kernel block) of both listings
                                                   compared with the `;` comments stripped and the function index in .LBB<n>_,
                                                   .Lfunc_end<n> and .Ltmp<n> normalised; exit status 1 if a common function differs"""
import re, subprocess, sys


def functions(path):
    """{symbol: (normalised lines, info)}; info = the `; Kernel info:` figures, None for a function that is not a kernel"""
    out, lines = {}, open(path).read().split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^(\S+):\s+; @(\S+)$", lines[i])
        if not m or m.group(1) != m.group(2):
            i += 1; continue
        name, j = m.group(1), i + 1
        while not lines[j].startswith(".Lfunc_end"): j += 1
        body = []
        for l in lines[i + 1:j]:
            l = re.sub(r"\.(LBB|Lfunc_end|Ltmp)\d+", r".\1", l.split(";")[0].rstrip())
            if l: body.append(l)
        info = None
        if any(l.startswith("\t.amdhsa_kernel") for l in body):
            info = {}
            while "codeLenInByte" not in info or "ScratchSize" not in info:
                j += 1
                m = re.match(r"^; (codeLenInByte|TotalNumSgprs|TotalNumVgprs|ScratchSize)\s*[=:]\s*(\d+)", lines[j])
                if m: info[m.group(1)] = int(m.group(2))
        out[name] = (body, info)
        i = j
    return out


def demangle(names):
    return dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))


if sys.argv[1] == "list":
    k = {n: f[1] for n, f in functions(sys.argv[2]).items() if f[1] is not None}
    dm = demangle(sorted(k))
    print("%10s %6s %6s %8s  kernel" % ("codeLen", "VGPRs", "SGPRs", "scratch"))
    for n in sorted(k, key=lambda n: dm[n]):
        print("%10d %6d %6d %8d  %s" % (k[n]["codeLenInByte"], k[n]["TotalNumVgprs"], k[n]["TotalNumSgprs"], k[n]["ScratchSize"], dm[n]))
    print("%d kernels, %d bytes of machine code" % (len(k), sum(v["codeLenInByte"] for v in k.values())))
else:
    a, b = functions(sys.argv[2]), functions(sys.argv[3])
    common = sorted(set(a) & set(b))
    differ = [n for n in common if a[n][0] != b[n][0]]
    dm = demangle(sorted(set(a) | set(b)))
    for tag, names in (("only in " + sys.argv[2], sorted(set(a) - set(b))), ("only in " + sys.argv[3], sorted(set(b) - set(a))), ("DIFFER", differ)):
        for n in names: print("%s: %s" % (tag, dm[n]))
    print("%d functions in both listings, %d identical, %d differ; %d only in the first, %d only in the second"
          % (len(common), len(common) - len(differ), len(differ), len(set(a) - set(b)), len(set(b) - set(a))))
    sys.exit(1 if differ else 0)
