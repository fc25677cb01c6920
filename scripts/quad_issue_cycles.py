"""Vector-instruction histogram and issue-cycle total of ONE full quad wave of the headline sweep.

    hipcc <CXXFLAGS of csrc/Makefile> -S --cuda-device-only ibh_fused2d.hip -o f.s
    python scripts/quad_issue_cycles.py f.s [KERNEL-NAME-PART]

Reads the gfx950 listing, finds k_sweep_quad<false,false,false,false> (or the kernel whose mangled name holds the given
part) and walks the path a wave with a complete quad and the compact companion rows takes:

  start   the basic block that takes the address of quad2::lane_tab (the pair-tile form takes lane_tab_half)
  s_branch, s_cbranch_execnz         followed (exec is non-zero after a restored mask)
  s_cbranch_execz, _scc*, _vcc*      fall through (divergent side blocks are counted: some lane of a wave takes them)
  s_endpgm                           end

Every `v_*` instruction on that path is priced with the issue costs measured on MI355X with four waves per SIMD
(profiles/r4_final/README.md, "Issue rates"): 4.0 cycles, except the ones in COST.  Registers and scratch come from
the kernel's metadata.
"""
import collections
import re
import sys

COST = {"v_pk_fma_f32": 5.7, "v_pk_mul_f32": 5.8, "v_pk_add_f32": 5.4, "v_med3_f32": 5.0, "v_rcp_f32": 8.7}
PLAIN = 4.0
TAB = "_ZN5quad2L8lane_tabE@"

# groups of the table in profiles/quad_issue_cycles/README.md
ARITH = ("v_sub_f32", "v_subrev_f32", "v_fma_f32", "v_fmaak_f32", "v_fmamk_f32", "v_fmac_f32", "v_mul_f32", "v_add_f32",
         "v_max_f32", "v_max3_f32", "v_med3_f32", "v_rcp_f32")
PACKED = ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32")


def mnemonic(line):
    op = line.split()[0]
    for suf in ("_e32", "_e64", "_dpp", "_sdwa"):
        if op.endswith(suf):
            if suf in ("_dpp", "_sdwa"):
                return op  # DPP and SDWA forms are their own rows
            op = op[:-len(suf)]
    return op


def kernel_body(text, part):
    m = re.search(r'^(\S*k_sweep_quad\S*%s\S*):\s*(;.*)?$' % re.escape(part), text, re.M)
    assert m, "kernel not found"
    end = re.search(r'^\.Lfunc_end\d+:', text[m.end():], re.M)
    return m.group(1), text[m.end():m.end() + end.start()].split('\n')


def walk(lines):
    label = {}
    for i, l in enumerate(lines):
        s = l.strip()
        if s.startswith('.LBB') and ':' in s:
            label[s.split(':')[0]] = i
    ref = next(i for i, l in enumerate(lines) if TAB in l)
    i = ref
    while i > 0 and not (lines[i].strip().startswith('.LBB') or 's_cbranch' in lines[i] or 's_branch' in lines[i]):
        i -= 1
    i += 1
    path, seen = [], set()
    while i < len(lines):
        assert i not in seen, "loop on the path"
        seen.add(i)
        s = lines[i].strip()
        i += 1
        if not s or s[0] in ';.' or s.endswith(':'):
            continue
        op = s.split()[0]
        if op == 's_endpgm':
            break
        if op in ('s_branch', 's_cbranch_execnz'):
            i = label[s.split()[1]]
            continue
        path.append(s)
    return path


def main():
    text = open(sys.argv[1]).read()
    part = sys.argv[2] if len(sys.argv) > 2 else "ILb0ELb0ELb0ELb0EE"
    name, lines = kernel_body(text, part)
    path = walk(lines)
    hist = collections.Counter(mnemonic(s) for s in path if s.startswith('v_'))
    n = sum(hist.values())
    cycles = sum(COST.get(o, PLAIN) * c for o, c in hist.items())
    meta = text[re.search(r'\.name:\s+' + re.escape(name), text).end():]  # the keys of a kernel's record are sorted
    vg = re.search(r'\.vgpr_count:\s+(\d+)', meta)
    sc = re.search(r'\.private_segment_fixed_size:\s+(\d+)', meta)
    arith = sum(c for o, c in hist.items() if o in ARITH)
    packed = sum(c for o, c in hist.items() if o in PACKED)
    print("kernel", name)
    print("full-quad path: instructions %d, vector %d, issue cycles %.1f" % (len(path), n, cycles))
    print("vgprs %s, scratch bytes %s" % (vg.group(1) if vg else "?", sc.group(1) if sc else "?"))
    print("arithmetic %d, packed arithmetic %d (as plain ops: %d)" % (arith, packed, arith + 2 * packed))
    for o, c in sorted(hist.items(), key=lambda t: (-t[1], t[0])):
        print("%-28s%4d  %7.1f" % (o, c, COST.get(o, PLAIN) * c))


if __name__ == "__main__":
    main()
