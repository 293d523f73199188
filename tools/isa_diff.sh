#!/bin/bash
# Are two builds' gfx950 kernels the same instruction stream?  Extracts the device code objects of build/obj/<object>.hip.o of
# both trees (clang-offload-bundler), disassembles them (llvm-objdump) and diffs the bodies of the named kernels, with
# addresses, labels, branch-target names, comments and the alignment padding behind a kernel left out.  Both trees must have
# been built with `make`.  No GPU needed.
# Usage: tools/isa_diff.sh <tree A> <tree B> <object> <mangled-name regex in A> <mangled-name regex in B>
#   e.g. tools/isa_diff.sh ../parent . vpcc_tiles '<_ZN4vpcc13k_recon_tilesILb0EEEvPKNS_8DevFrameE' \
#                                                  '<_ZN4vpcc13k_recon_tilesILb0ELj0EEEvPKNS_8DevFrameE'
set -e
B=/opt/rocm/llvm/bin
A=$1; N=$2; OBJ=$3; PA=$4; PN=$5
W=$(mktemp -d); trap 'rm -rf "$W"' EXIT
for t in A N; do
  tree=$A; [ $t = N ] && tree=$N
  $B/llvm-objcopy -O binary --only-section=.hip_fatbin "$tree/build/obj/$OBJ.hip.o" "$W/$t.fatbin"
  $B/clang-offload-bundler --unbundle --type=o --input="$W/$t.fatbin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$W/$t.co"
  $B/llvm-objdump -d --no-show-raw-insn "$W/$t.co" > "$W/$t.s"
done
body() { awk -v pat="$2" '/^[0-9a-f]+ <.*>:$/ {on = ($0 ~ pat)} on && !/^[0-9a-f]+ </ && !/^$/' "$1" |
         sed -E 's/^\s*[0-9a-f]+:?\s*//; s/<[^>]*>//g; s/\/\/.*$//; s/\s+$//; s/^\s+//' |
         awk '{ l[NR] = $0 } END { n = NR; while (n > 0 && (l[n] == "s_nop 0" || l[n] == "...")) n--; for (i = 1; i <= n; i++) print l[i] }'; }
body "$W/A.s" "$PA" > "$W/A.body"
body "$W/N.s" "$PN" > "$W/N.body"
[ -s "$W/A.body" ] && [ -s "$W/N.body" ] || { echo "kernel not found"; exit 2; }
echo "$(wc -l < "$W/A.body") / $(wc -l < "$W/N.body") instructions"
diff "$W/A.body" "$W/N.body" && echo "identical"
