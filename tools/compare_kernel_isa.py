#!/usr/bin/env python3
"""Did a refactor of csrc/ leave the generated kernels alone?  Compares the device assembly of two builds kernel by kernel (no GPU).

    for f in gnx_graph gnx_prep gnx_spmm gnx_spmm_bf16 gnx_spmm_train gnx_spmm_train_ord gnx_spmm_train_bf16 gnx_gcnii gnx_gcn gnx_ngcf \
             gnx_ngcf_wide gnx_ngcf_wide_back gnx_feature_dropout gnx_util gnx_dense gnx_dense_wgrad gnx_heads gnx_link gnx_rank gnx_halo; do
                                                       # every unit of the Makefile's SRCS (gnx_graph's kernels include rocprim's)
        hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S gnn-tf_amd/csrc/$f.hip -o $DIR/$f.s
    done                                               # once in a checkout of the old commit, once in the new one
    python tools/compare_kernel_isa.py OLD_DIR NEW_DIR > profiles/notes/<name>.txt

Units are paired by file name.  Where a change splits a unit, concatenate the new units' .s files under the old unit's name in NEW_DIR
(cat gnx_dense.s gnx_dense_wgrad.s gnx_heads.s > NEW_DIR/gnx_dense.s, and leave the parts out of NEW_DIR): kernel names are unique.

Per .amdhsa_kernel: the instruction text with symbol names, .LBB<n>_ label numbers, comments and directives stripped, and the
metadata counts .vgpr_count / .sgpr_count / .private_segment_fixed_size / .group_segment_fixed_size.  Kernels are paired by name:
first those whose full name is the same on both sides (reported under the family as it is spelled, so that k_x and k_x_bf16, or
the instantiations of one kernel over two row-storage policies, stay apart); for the rest a "_bf16" suffix and a leading row-storage
policy argument are dropped, the first two template arguments must agree and the rest of the shorter list must be a subsequence of
the longer one (the hand-copied bf16 kernels carried no U / PIPE arguments)."""
import glob
import os
import re
import subprocess
import sys

COUNTS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    txt = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in COUNTS)
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\s*\.section\s+\.rodata", txt, re.S | re.M):
        name, lines = m.group(1), []
        if name not in meta:
            continue
        for ln in m.group(2).split("\n"):
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()).replace(name, "SELF")
            if ln and (not ln.startswith(".") or ln.startswith(".LBB")):
                lines.append(ln)
        out[name] = (lines, meta[name])
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {p: out[n] for n, p in zip(names, plain)}            # by full name: no two kernels of a unit share an entry


def spelled(demangled):
    """(family, template arguments) as the source spells them"""
    fam, _, args = re.sub(r"\(anonymous namespace\)::|^void |\(.*\)$", "", demangled).partition("<")
    return fam, (args.rstrip(">"),)


def key(demangled):
    s = re.sub(r"\(anonymous namespace\)::|^void |\(.*\)$", "", demangled)
    fam, _, args = s.partition("<")
    fam = fam.replace("_drop_bf16", "_drop").replace("_bf16", "").replace("k_spmm_long_reduce_drop", "k_spmm_long_reduce")
    args = [a.strip() for a in re.sub(r"\w+Rows\w*(<\w+>)?,?", "", args.rstrip(">")).split(",") if a.strip()]
    return fam, tuple(args)


def subsequence(short, long):
    it = iter(long)
    return all(x in it for x in short)


def main(old_dir, new_dir):
    for new_s in sorted(glob.glob(os.path.join(new_dir, "*.s"))):
        unit = os.path.basename(new_s)
        old, new = kernels(os.path.join(old_dir, unit)), kernels(new_s)
        print(f"### {unit[:-2]}.hip: {len(old)} kernels before, {len(new)} after")
        same_name = sorted(set(old) & set(new))
        left, fams = {key(n): v for n, v in old.items() if n not in new}, {}
        assert len(left) + len(same_name) == len(old), "two kernels of the old build share a pairing key"
        pairs = [(spelled(n), new[n], old[n]) for n in same_name]
        for (fam, args), found in sorted((key(n), v) for n, v in new.items() if n not in old):
            match = [k for k in left if k[0] == fam and k[1][:2] == args[:2]
                     and subsequence(*sorted((k[1], args), key=len))]
            if not match:
                print(f"  no kernel before for {fam}<{', '.join(args)}>")
                continue
            pairs.append(((fam, args), found, left.pop(sorted(match, key=lambda k: abs(len(k[1]) - len(args)))[0])))
        for (fam, args), (body, counts), (obody, ocounts) in pairs:
            same = body == obody and counts == ocounts
            fams.setdefault(fam, []).append(None if same else
                f"    <{', '.join(args)}>: instructions {len(obody)} -> {len(body)}, "
                + ", ".join(f"{n} {a} -> {b}" for n, a, b in zip(("VGPR", "SGPR", "scratch", "LDS"), ocounts, counts)))
        for fam, rows in fams.items():
            print(f"- `{fam}`: {len(rows)} instantiations, {rows.count(None)} identical")
            print("\n".join(r for r in rows if r), end="\n" if any(rows) else "")
        for fam, args in sorted(left):
            print(f"  only before: {fam}<{', '.join(args)}>")


if __name__ == "__main__":
    main(*sys.argv[1:3])
