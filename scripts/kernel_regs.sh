#!/bin/bash
# One line per gfx950 kernel of the library: register / spill / scratch / LDS use from the code-object metadata and a hash
# of the kernel's machine code (its slice of .text by the symbol table), sorted by name.  Two checkouts have produced the
# same device code exactly when `diff` of their tables is empty.
# usage: python -m tapqir_amd.build && scripts/kernel_regs.sh [tq_cosmos ...] > table.txt     (default: every unit)
R=$(cd $(dirname $0)/.. && pwd)
L=/opt/rocm/lib/llvm/bin
[ $# -gt 0 ] || set -- $(cd $R/tapqir_amd/csrc && ls *.hip | sed 's/\.hip$//')
T=$(mktemp -d)
for tu in "$@"; do
  objcopy -O binary --only-section=.hip_fatbin $R/tapqir_amd/build/$tu.o $T/fatbin || exit 1
  $L/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$T/fatbin --output=$T/$tu.co --unbundle || exit 1
  $L/llvm-readelf --notes $T/$tu.co > $T/notes
  $L/llvm-readelf -S -s --wide $T/$tu.co > $T/syms
  python3 - $tu $T <<'EOF'
import hashlib, re, subprocess, sys
tu, T = sys.argv[1:3]
co = open(f"{T}/{tu}.co", "rb").read()
syms = open(f"{T}/syms").read()
addr, off = (int(x, 16) for x in re.search(r"\] \.text\s+PROGBITS\s+(\w+) (\w+)", syms).groups())
func = {m[3]: (int(m[1], 16), int(m[2])) for m in re.finditer(r"^\s*\d+: (\w+)\s+(\d+) FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$", syms, re.M)}
rows = []
for blk in open(f"{T}/notes").read().split("- .agpr_count")[1:]:
    g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
    value, size = func[g("name")]
    code = hashlib.sha256(co[value - addr + off:value - addr + off + size]).hexdigest()[:16]
    dn = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout.strip()
    dn = re.sub(r"\(.*", "", dn).replace("void ", "")
    rows.append(f"{tu:12s} {dn:72s} vgpr={g('vgpr_count'):>4s} sgpr={g('sgpr_count'):>4s} spill={g('vgpr_spill_count'):>4s} "
                f"scratch={g('private_segment_fixed_size'):>5s} lds={g('group_segment_fixed_size'):>6s} bytes={size:>6d} sha={code}")
print("\n".join(sorted(rows)))
EOF
done
rm -rf $T
