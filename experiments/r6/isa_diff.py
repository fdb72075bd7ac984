#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two assembly listings of the device code (isa_stats.py --out writes them): which kernels' instruction
streams are the same, which differ, which exist on one side only.  Kernels are matched by demangled name; local labels (.LBB85_4: the
number is the function's ordinal in the file, which moves when a kernel is added or removed) and the kernel's own symbol are normalised.
    python experiments/r6/isa_diff.py OLD.s NEW.s [--rename 'REGEX=REPLACEMENT' ...]     (--rename rewrites OLD's demangled names first)
Exit status 1 when a kernel differs or has no partner."""
import re, subprocess, sys


def kernels(path):
    """-> {demangled name with template arguments: normalised body}"""
    t = open(path).read()
    found = [(m.group(1), t[m.end():t.find(".Lfunc_end", m.end())]) for m in re.finditer(r"^(_Z\w+):\s*; @", t, re.M)]
    names = subprocess.run(["c++filt"], input="\n".join(s for s, _ in found), capture_output=True, text=True).stdout.splitlines()
    out = {}
    for (sym, body), name in zip(found, names):
        body = re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", body.replace(sym, "@SELF"))
        body = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", body)  # (long branches: numbered through the file)
        lines = [l.split(";")[0].rstrip() for l in body.splitlines()]  # (comments carry source-level names and basic-block notes)
        out[re.sub(r"\(.*", "", name).replace("void ", "")] = "\n".join(l for l in lines if l.strip())
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    renames = [args[i + 1].split("=", 1) for i, a in enumerate(args) if a == "--rename"]
    paths = [a for i, a in enumerate(args) if a != "--rename" and (i == 0 or args[i - 1] != "--rename")]
    old, new = kernels(paths[0]), kernels(paths[1])
    for pat, rep in renames:
        old = {re.sub(pat, rep, k): v for k, v in old.items()}
    same = [k for k in old if k in new and old[k] == new[k]]
    differ = [k for k in old if k in new and old[k] != new[k]]
    only_old, only_new = [k for k in old if k not in new], [k for k in new if k not in old]
    print(f"{len(old)} kernels in {paths[0]}, {len(new)} in {paths[1]}: {len(same)} identical, {len(differ)} differ, "
          f"{len(only_old)} only old, {len(only_new)} only new")
    for title, names in (("differ", differ), ("only old", only_old), ("only new", only_new)):
        for k in sorted(names):
            extra = f"  ({len(old[k].splitlines())} -> {len(new[k].splitlines())} lines)" if title == "differ" else ""
            print(f"  {title}: {k}{extra}")
    sys.exit(1 if differ or only_old or only_new else 0)
