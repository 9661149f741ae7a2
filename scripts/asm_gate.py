"""The refactor gate, function by function: python scripts/asm_gate.py PARENT_DIR BRANCH_DIR [--table]

Each directory holds, per translation unit NAME.hip, the device assembly NAME.s (hipcc <HIPFLAGS> -save-temps=obj, the file
*-hip-amdgcn-amd-amdhsa-gfx950.s) and NAME.log (stderr of the same compile with -Rpass-analysis=kernel-resource-usage).
Compile both trees at the same path (NOTEBOOK.md, "One home for the BSDF table").  Every function of the branch -- kernels and
the static __noinline__ callees, of which each unit that calls one has a copy -- is compared with the parent's function of
the same name: from its label to its .Lfunc_end, without comment / .loc / .file / .ident lines and trailing comments, with
the labels that carry the function's position in its unit renumbered.  Exit status 1 if a function differs or is missing."""
import glob, hashlib, os, re, sys

DROP = re.compile(r"^\s*(;|\.loc\s|\.file\s|\.ident\s)")
POS = re.compile(r"\.L(BB|func_begin|func_end|JTI|tmp|CPI|post_getpc)(\d+)")
RES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
       "LDS Size [bytes/block]")


def functions(path):
    """{symbol: normalised text} of one assembly file"""
    lines = open(path).read().split("\n")
    out = {}
    for sym in re.findall(r"^\s*\.type\s+(\S+),@function", "\n".join(lines), re.M):
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        body, ids = [], {}
        for ln in lines[start:]:
            if DROP.match(ln):
                continue
            ln = ln.split(";")[0].rstrip()
            if not ln:
                continue
            # .LBB<n>_, .LCPI<n>_, .LJTI<n>_, .Lfunc_end<n>: the function's index in its unit; .Ltmp<n>, .Lpost_getpc<n>: counters
            # of the unit -- each kind numbered by first appearance within the function
            ln = POS.sub(lambda m: ".L%s%d" % (m.group(1), ids.setdefault(m.group(1, 2), len(ids))), ln)
            body.append(ln)
            if re.match(r"\.Lfunc_end\d+:", ln):
                break
        out[sym] = "\n".join(body)
    return out


def resources(path):
    """{symbol: {figure: value}} from the kernel-resource-usage remarks (the device pass prints each kernel once)"""
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"remark: [^ ]+ +(Function Name|[A-Za-z][A-Za-z /\[\]]*?): (\S+) \[-Rpass-analysis", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def load(d):
    fn, res = {}, {}
    for s in sorted(glob.glob(os.path.join(d, "*.s"))):
        unit = os.path.basename(s)[:-2]
        for k, v in functions(s).items():
            fn[(unit, k)] = v
        log = s[:-2] + ".log"
        if os.path.exists(log):
            for k, v in resources(log).items():
                res[(unit, k)] = v
    return fn, res


def main():
    pdir, bdir = sys.argv[1], sys.argv[2]
    pfn, pres = load(pdir)
    bfn, bres = load(bdir)
    pby = {}
    for (unit, k), v in pfn.items():
        pby.setdefault(k, []).append((unit, v))
    bad = 0
    seen = set()
    for (unit, k), v in sorted(bfn.items()):
        cands = pby.get(k, [])
        same = [u for u, t in cands if t == v]
        seen.add(k)
        h = hashlib.sha256(v.encode()).hexdigest()[:12]
        if same:
            state = "identical to parent %s" % same[0]
        elif cands:
            state = "DIFFERS from parent %s (%d vs %d lines)" % (cands[0][0], v.count("\n") + 1, cands[0][1].count("\n") + 1)
            bad += 1
        else:
            state = "NOT IN PARENT"
            bad += 1
        print("%-22s %s %s  %s" % (unit, h, k, state))
        if "--table" in sys.argv and (unit, k) in bres:
            pr = next((pres[(u, k)] for u, _ in cands if (u, k) in pres), {})
            print("    " + "  ".join("%s %s|%s" % (r.split(" [")[0], pr.get(r, "-"), bres[(unit, k)].get(r, "-")) for r in RES))
            if pr != bres[(unit, k)]:
                print("    RESOURCES DIFFER")
                bad += 1
    for k in sorted(set(pby) - seen):
        print("MISSING in branch: %s" % k)
        bad += 1
    print("%d functions compared, %d not identical" % (len(bfn), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
