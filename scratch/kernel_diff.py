"""kernel_diff.py <parent.s> <change.s> [kernel-name filter ...]: two device-only gfx950 assemblies of one source, kernel by
kernel.  Bodies are compared with comments, directives and label numbers stripped; for kernels that differ (or match a
filter) the registers, spills, scratch, LDS, the instruction total and the counts of the instructions the solver notes track."""
import collections, re, sys

COUNT = ["s_barrier", "v_fma_f64", "v_mul_f64", "v_add_f64", "v_rsq_f64", "v_mfma", "ds_read", "ds_write", "global_load", "global_store"]


def kernels(path):
    txt = open(path).read()
    meta = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
        meta[g("symbol").replace(".kd", "")] = "/".join([blk.split()[0]] + [g(k) for k in (
            "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")])
    out, name, body = {}, None, []
    for ln in txt.split("\n"):
        ln = ln.split(";")[0].strip()
        if name is None:
            if ln.endswith(":") and ln[:-1] in meta:  # the kernel's entry label
                name, body = ln[:-1], []
            continue
        if ln.startswith(".amdhsa_kernel") or ln.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif ln and not ln.startswith(".") and not ln.endswith(":"):
            body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", ln))
    return out, meta


(pa, pm), (ca, cm) = kernels(sys.argv[1]), kernels(sys.argv[2])
flt = sys.argv[3:]
print("kernel symbols:", len(pa), "/", len(ca), "same set" if set(pa) == set(ca) else "DIFFERENT SETS")
same = [k for k in pa if k in ca and pa[k] == ca[k]]
print("identical instruction text:", len(same), "of", len(pa))
for k in sorted(pa):
    if k not in ca or (pa[k] == ca[k] and not any(f in k for f in flt)):
        continue
    print(f"\n{k}: {'same text' if pa[k] == ca[k] else 'DIFFERENT text'}")
    print(f"  agpr/vgpr/sgpr/vspill/sspill/scratch/lds  {pm.get(k)} -> {cm.get(k)}")
    print(f"  instructions {len(pa[k])} -> {len(ca[k])} ({100.0 * (len(ca[k]) - len(pa[k])) / len(pa[k]):+.2f} %)")
    cp, cc = collections.Counter(), collections.Counter()
    for body, cnt in ((pa[k], cp), (ca[k], cc)):
        for ln in body:
            for c in COUNT:
                if ln.startswith(c):
                    cnt[c] += 1
    print("  " + ", ".join(f"{c} {cp[c]} -> {cc[c]}" for c in COUNT))
