"""Is the gfx950 device code of two trees the same?  Compile every csrc/*.hip of each tree to assembly, then compare
the listings per symbol.  For a refactor that must not change a kernel, this is an exact test that needs no GPU.

  python tools/isa_identity.py emit OUTDIR [TREE] [-jN]    # TREE/moe-gan_cpsc541_amd/csrc/*.hip -> OUTDIR/<unit>.s
  python tools/isa_identity.py compare PARENT_DIR NEW_DIR  # the report, on stdout; exit status 1 if anything differs

emit uses the Makefile's CXXFLAGS plus --cuda-device-only -S, run inside csrc with relative file names, and pins
-cuid= (the compilation-unit id is otherwise a hash of the source's absolute path, and names one symbol per unit).
compare cuts each listing at its `.type <symbol>,@function` lines: one piece per function (its text, and for a kernel
the descriptor that follows it), plus what stands outside every function (header, metadata).  Pieces are compared as
bytes; nothing in them is interpreted.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUID = "isa-identity"
FUNC = re.compile(r"^\s*\.type\s+(\S+),@function\s*$")


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name} \?= (.*)$", text, re.M).group(1)
    return var("HIPCC"), var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()


def emit(outdir, tree, jobs):
    csrc = os.path.join(tree, "moe-gan_cpsc541_amd", "csrc")
    outdir = os.path.abspath(outdir)
    os.makedirs(outdir, exist_ok=True)
    hipcc, flags = makefile_flags(csrc)
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(u):
        cmd = [hipcc, *flags, "--cuda-device-only", "-S", f"-cuid={CUID}", u, "-o", os.path.join(outdir, u[:-4] + ".s")]
        r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        return u, " ".join(cmd), r.returncode, r.stderr

    bad = 0
    with ThreadPoolExecutor(jobs) as pool:
        for u, cmd, rc, err in pool.map(one, units):
            print(cmd if rc == 0 else f"FAILED ({rc}): {cmd}\n{err}", flush=True)
            bad += rc != 0
    return 1 if bad else 0


def pieces(path):
    """{symbol: bytes of its piece}, with "" for the lines outside every function."""
    out, name = {"": []}, ""
    for line in open(path, "rb").read().decode("utf-8", "replace").splitlines(True):
        m = FUNC.match(line)
        if m:
            name = m.group(1)
            out.setdefault(name, [])
        elif line.startswith("\t.amdgpu_metadata") or line.startswith("\t.section\t.AMDGPU"):
            name = ""
        out[name].append(line)
    return {k: "".join(v) for k, v in out.items()}


def compare(pdir, ndir):
    units = sorted(set(os.listdir(pdir)) | set(os.listdir(ndir)))
    units = [u for u in units if u.endswith(".s")]
    tot = dict(kernels=0, same=0, diff=0, only_p=0, only_n=0, rest_diff=0)
    lines, detail = [], []
    for u in units:
        pp, nn = os.path.join(pdir, u), os.path.join(ndir, u)
        if not (os.path.exists(pp) and os.path.exists(nn)):
            detail.append(f"{u}: present in one build only")
            tot["rest_diff"] += 1
            continue
        p, n = pieces(pp), pieces(nn)
        rest = p.pop("") == n.pop("")
        kern = lambda d: {k for k, v in d.items() if ".amdhsa_kernel" in v}
        both = set(p) & set(n)
        same = {k for k in both if p[k] == n[k]}
        only_p, only_n = set(p) - both, set(n) - both
        whole = open(pp, "rb").read() == open(nn, "rb").read()
        lines.append(f"  {u[:-2] + '.hip':22s} kernels {len(kern(n)):4d}  functions {len(n):4d}  identical {len(same):4d}  "
                     f"differing {len(both) - len(same):3d}  only parent {len(only_p):3d}  only new {len(only_n):3d}  "
                     f"outside functions {'same' if rest else 'DIFFERS'}  whole listing {'same bytes' if whole else 'DIFFERS'}")
        tot["kernels"] += len(kern(n))
        tot["same"] += len(same)
        tot["diff"] += len(both) - len(same)
        tot["only_p"] += len(only_p)
        tot["only_n"] += len(only_n)
        tot["rest_diff"] += (not rest) or (not whole)
        detail += [f"{u}: differs: {k}" for k in sorted(both - same)]
        detail += [f"{u}: only in the parent build: {k}" for k in sorted(only_p)]
        detail += [f"{u}: only in this build: {k}" for k in sorted(only_n)]
    print(f"translation units compared:       {len(units)}")
    print(f"kernels in this build:            {tot['kernels']}")
    print(f"functions present in both:        {tot['same'] + tot['diff']}")
    print(f"  identical bytes:                {tot['same']}")
    print(f"  differing:                      {tot['diff']}")
    print(f"only in the parent build:         {tot['only_p']}")
    print(f"only in this build:               {tot['only_n']}")
    print(f"units whose listing differs anywhere (functions, header or metadata): {tot['rest_diff']}")
    print("\nper translation unit:")
    print("\n".join(lines))
    if detail:
        print("\ndifferences:")
        print("\n".join(detail))
    return 1 if (tot["diff"] or tot["only_p"] or tot["only_n"] or tot["rest_diff"]) else 0


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-j")]
    jobs = next((int(a[2:]) for a in sys.argv[1:] if a.startswith("-j")), 8)
    if len(args) >= 2 and args[0] == "emit":
        return emit(args[1], args[2] if len(args) > 2 else ROOT, jobs)
    if len(args) == 3 and args[0] == "compare":
        return compare(args[1], args[2])
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
