"""Compare the device code of two builds of one source file kernel by kernel, keyed by symbol:
    hipcc <the Makefile's FLAGS> -save-temps=obj -c conv_f16k.hip -o <dir>/conv_f16k.o       (once per commit)
    python tools/codeobj_diff.py <dirA>/conv_f16k-hip-amdgcn-amd-amdhsa-gfx950.s <dirB>/conv_f16k-hip-amdgcn-amd-amdhsa-gfx950.s
A kernel is "identical" when its assembly from .type to .end_amdhsa_kernel (instruction stream and the .amdhsa_ kernel descriptor:
VGPRs, SGPRs, LDS, scratch, kernarg size) and its .amdgpu_metadata entry are equal after the function's index in the module is taken out
of its local labels (.LBB<n>_, .Lfunc_end<n>) and the IR block names are taken out of the labels' comments (numbered per module: they
move when another instantiation of the same template comes or goes).  The order of the kernels in the module is free."""
import re, sys, hashlib

def norm(ls):
    out = []
    for l in ls:
        l = re.sub(r"BB\d+_", "BB_", l)              # local labels and loop comments carry the function's index in the module
        l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l)
        l = re.sub(r"\.Ltmp\d+", ".Ltmp", l)
        l = re.sub(r"\$local\d*", "$local", l)
        l = re.sub(r"^(\.LBB_\d+:|; %bb\.\d+:)\s*; %.*$", r"\1", l)      # the IR block name a label's comment repeats: numbered per module
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

pa, pb = sys.argv[1], sys.argv[2]
ka, kb, ma, mb = kernels(pa), kernels(pb), metadata(pa), metadata(pb)
print(f"parent: {len(ka)} kernel symbols ({len(ma)} metadata entries); branch: {len(kb)} kernel symbols ({len(mb)} metadata entries)")
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
