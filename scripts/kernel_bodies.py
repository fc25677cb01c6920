#!/usr/bin/env python3
"""Compare the bodies of named kernels in two gfx950 listings, and print the register / scratch figures of a listing's
kernels from its code-object metadata.

    hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only csrc/ibh_fused2d.hip -o head.s     (same at the parent: parent.s)
    scripts/kernel_bodies.py diff parent.s head.s k_sweep_quad_euler k_sweep_euler
    scripts/kernel_bodies.py diff --rename '<(\d), true, true, false, true>=<\1, 3, false>' parent.s head.s k_sweep
    scripts/kernel_bodies.py meta head.s k_sweep_quad_euler k_update_euler

`diff`: for every kernel of the FIRST listing -- every name in its amdhsa.kernels metadata, template instantiation or not --
whose demangled name contains one of the patterns, the instructions between its label and its end label must be the same
lines in the second listing (labels are renumbered per function, so local
labels are compared by their order of appearance).  Exit status 1 on any difference, and when no kernel
matches.  `--rename OLD=NEW` (repeatable): a
regular expression substitution on the demangled names of the FIRST listing before they are looked up in the second, for a
kernel whose template parameters were renumbered between the two.  `meta`: .vgpr_count, .sgpr_count,
.private_segment_fixed_size (scratch bytes), .group_segment_fixed_size (LDS bytes) per matching kernel.
"""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def bodies(path):
    """{mangled kernel name: [instruction lines]} of a listing."""
    res, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\s*(\.Lfunc_end\d+:|\.section|\.rodata|\.amdhsa_kernel)", line):
                res[name] = cur
                cur = None
                continue
            t = line.split(";")[0].strip()
            if t and not t.startswith(".p2align"):
                cur.append(t)
    return res


def canon(lines):
    """local labels by order of appearance"""
    ids = {}
    def sub(m):
        return ids.setdefault(m.group(0), f".L{len(ids)}")
    return [re.sub(r"\.LBB\d+_\d+", sub, l) for l in lines]


def meta(path):
    """{mangled name: {key: value}} from the amdhsa.kernels metadata of a listing."""
    res, cur = {}, None
    for line in open(path):
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if line.lstrip().startswith("- .") and k in ("agpr_count", "args"):
            cur = {}
        if cur is not None:
            cur[k] = v
            if k == "name":
                res[v] = cur
    return res


def main():
    mode, args, renames = sys.argv[1], sys.argv[2:], []
    while "--rename" in args:
        i = args.index("--rename")
        renames.append(args[i + 1].split("=", 1))
        del args[i:i + 2]
    if mode == "diff":
        a, b, pats = bodies(args[0]), bodies(args[1]), args[2:]
        kernels = meta(args[0])   # (c++filt prints a return type for template instantiations only: no test on `void`)
        dm, dmb = demangle(list(a)), demangle(list(b))
        # a kernel that gained trailing template parameters with `false` defaults (and trailing arguments for them) is the
        # same kernel: matched by its name without them
        key = lambda d: re.sub(r"(, false)+>$", ">", d.replace("(anonymous namespace)::", "").split("(")[0])
        byname = {key(dmb[k]): k for k in b}

        def renamed(d):
            for old, new in renames:
                d = re.sub(old, new, d)
            return d
        bad = n = 0
        for k in sorted(a, key=lambda x: dm[x]):
            if k not in kernels or not any(p in dm[k] for p in pats):
                continue
            n += 1
            kb = byname.get(key(renamed(dm[k])))
            same = kb is not None and canon(a[k]) == canon(b[kb])
            bad += not same
            print(("identical  " if same else "DIFFERENT  " if kb else "MISSING    ") + f"{len(a[k]):6d} lines  {dm[k]}")
        print(f"{n} kernels compared, {bad} differ")
        return 1 if bad or not n else 0
    if mode == "meta":
        md, pats = meta(args[0]), args[1:]
        dm = demangle(list(md))
        for k in sorted(md, key=lambda x: dm[x]):
            if any(p in dm[k] for p in pats):
                r = md[k]
                print(f"vgpr {r.get('vgpr_count'):>4}  agpr {r.get('agpr_count'):>3}  sgpr {r.get('sgpr_count'):>4}  scratch "
                      f"{r.get('private_segment_fixed_size'):>4}  lds {r.get('group_segment_fixed_size'):>6}  {dm[k]}")
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main())
