"""Compare the device code of two builds kernel by kernel, keyed by symbol.  A side is one module or several (a source file that was split:
the union of their kernels is compared, and a symbol that several modules of a side hold must be the same kernel in each of them):
    hipcc <the Makefile's FLAGS> -save-temps=obj -c conv_f16k.hip -o <dir>/conv_f16k.o       (once per commit and source file)
    python tools/codeobj_diff.py <dirA>/conv_f16k-hip-amdgcn-amd-amdhsa-gfx950.s <dirB>/conv_f16k-hip-amdgcn-amd-amdhsa-gfx950.s
    python tools/codeobj_diff.py <dirA>/conv_f16k-hip-*.s -- <dirB>/conv_f16k-hip-*.s <dirB>/conv_a-hip-*.s <dirB>/gemm_f16k-hip-*.s <dirB>/conv3x3_resident-hip-*.s
A kernel is "identical" when its assembly from .type to .end_amdhsa_kernel (instruction stream and the .amdhsa_ kernel descriptor:
VGPRs, SGPRs, LDS, scratch, kernarg size) and its .amdgpu_metadata entry are equal after the function's index in the module is taken out
of its local labels (.LBB<n>_, .Lfunc_end<n>) and the IR block names are taken out of the labels' comments (numbered per module: they
move when another instantiation of the same template comes or goes) and the blanks between a local label and the comment after it are
collapsed (the comment is padded to a column, so the padding changes with the number of digits of the index).  The order of the kernels in
a module is free."""
import re, sys, hashlib

def norm(ls):
    out = []
    for l in ls:
        l = re.sub(r"BB\d+_", "BB_", l)              # local labels and loop comments carry the function's index in the module
        l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l)
        l = re.sub(r"\.Ltmp\d+", ".Ltmp", l)
        l = re.sub(r"\$local\d*", "$local", l)
        l = re.sub(r"^(\.LBB_\d+:|; %bb\.\d+:)\s*; %.*$", r"\1", l)      # the IR block name a label's comment repeats: numbered per module
        l = re.sub(r"^(\.LBB_\d+:)\s+;", r"\1 ;", l)                        # any other comment after a label is padded to a column: .LBB3_2: and .LBB10_2: pad differently
        out.append(l)
    return out

def metadata(path):
    txt = open(path).read()
    a = txt.index(".amdgpu_metadata")
    b = txt.index(".end_amdgpu_metadata")
    entries, cur = [], None
    for l in txt[a:b].split("\n"):
        if l.startswith("  - ."):
            cur = [l]
            entries.append(cur)
        elif cur is not None and l.startswith("    "):
            cur.append(l)
        else:
            cur = None
    out = {}
    for e in entries:
        sym = [re.search(r"\.symbol:\s+(\S+)", l) for l in e]
        sym = [m.group(1) for m in sym if m]
        if sym:
            out[sym[0][:-3] if sym[0].endswith(".kd") else sym[0]] = e
    return out

def kernels(path):
    lines = open(path).read().split("\n")
    ks, i, n = {}, 0, len(lines)
    while i < n:
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if m:
            j = i + 1
            while j < n and lines[j].strip() != ".end_amdhsa_kernel" and not re.match(r"\s*\.type\s+(\S+),@function", lines[j]):
                j += 1
            if j < n and lines[j].strip() == ".end_amdhsa_kernel":
                ks[m.group(1)] = lines[i:j + 1]
                i = j
            else:
                i = j - 1
        i += 1
    return ks

def side(paths):
    """the union of the kernels and metadata entries of a side's modules; a symbol in several of them (the common.h / conv_geom.h kernels
    every module instantiates for itself) must be the same kernel in each"""
    ks, ms, copies = {}, {}, 0
    for p in paths:
        k, m = kernels(p), metadata(p)
        for s in k:
            if s in ks:
                copies += 1
                if norm(k[s]) != norm(ks[s]) or m.get(s) != ms.get(s):
                    sys.exit(f"{s}: differs between {p} and an earlier module of the same side")
        ks.update(k)
        ms.update(m)
    return ks, ms, copies

args = sys.argv[1:]
if "--" in args:
    pa, pb = args[:args.index("--")], args[args.index("--") + 1:]
else:
    pa, pb = args[:1], args[1:]
if not pa or not pb:
    sys.exit("usage: codeobj_diff.py PARENT.s [PARENT.s ...] -- BRANCH.s [BRANCH.s ...]      (one file per side: the `--` may be left out)")
(ka, ma, ca), (kb, mb, cb) = side(pa), side(pb)
print(f"parent: {len(ka)} kernel symbols ({len(ma)} metadata entries) in {len(pa)} module(s), {ca} repeated; "
      f"branch: {len(kb)} kernel symbols ({len(mb)} metadata entries) in {len(pb)} module(s), {cb} repeated")
print("removed:", sorted(set(ka) - set(kb)))
print("added:  ", sorted(set(kb) - set(ka)))
ndiff = 0
for s in sorted(set(ka) & set(kb)):
    ta, tb = norm(ka[s]), norm(kb[s])
    same_text = ta == tb
    same_meta = ma.get(s) == mb.get(s) and s in ma
    ninstr = sum(1 for l in ta if l.startswith("\t") and not l.lstrip().startswith((".", ";")))
    verdict = "identical" if same_text and same_meta else "DIFFERENT"
    if verdict != "identical":
        ndiff += 1
        d = [(x, y) for x, y in zip(ta, tb) if x != y][:5]
        verdict += f" text={same_text} meta={same_meta} first diffs={d}"
    print(f"{verdict:10s} {ninstr:6d} lines  sha1 {hashlib.sha1(chr(10).join(ta).encode()).hexdigest()[:12]}  {s}")
print("kernels that differ:", ndiff)
