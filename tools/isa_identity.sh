#!/bin/bash
# Device-code identity of the working tree against a parent revision, for refactors that must not move
# the compiler's output: every GK_PART of csrc/gjkepa_kernel.hip and the hull, broad-phase, swept broad-phase, contact-list and pose kernel files
# compiled with the Makefile's flags plus --cuda-device-only -S at both, the compilation-unit symbol
# (__hip_cuid_<hex>, a hash of the source text) masked, one sha256 pair per file.  It only diffs.
# usage: bash tools/isa_identity.sh <parent-rev> [workdir] > profiles/rNN/isa_identity.txt
# (a workdir that already holds <parent-rev>/ reuses the parent's assembly)
set -e
P=collision-detect-gjk-epa_amd
W=${2:-$(mktemp -d)}
REV=$(git rev-parse --short "$1")
F="--offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -Wall -Wno-unused-function --cuda-device-only -S"
emit() {   # emit <tree> <outdir>: masked device assembly of every kernel file of <tree>
  mkdir -p "$2"
  for p in 0 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15; do
    /opt/rocm/bin/hipcc $F -DGK_PART=$p "$1/$P/csrc/gjkepa_kernel.hip" -o "$2/gk_part$p.s" 2> /dev/null &
  done
  for k in hull broadphase sweep contacts pose; do
    /opt/rocm/bin/hipcc $F "$1/$P/csrc/${k}_kernel.hip" -o "$2/${k}_kernel.s" 2> /dev/null &
  done
  wait
  sed -i -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$2"/*.s
}
if [ ! -d "$W/$REV" ]; then
  mkdir -p "$W/src_$REV" && git archive "$REV" $P/csrc include | tar -x -C "$W/src_$REV"
  emit "$W/src_$REV" "$W/$REV.tmp" && mv "$W/$REV.tmp" "$W/$REV"
fi
rm -rf "$W/tree" && emit . "$W/tree"
echo "# masked device assembly, sha256: parent $REV, working tree, verdict (lines / differing lines when not identical)"
for f in $(cd "$W/$REV" && ls *.s | sort -V); do
  a=$(sha256sum < "$W/$REV/$f" | cut -c1-64); b=$(sha256sum < "$W/tree/$f" | cut -c1-64)
  v=identical
  [ "$a" = "$b" ] || v="DIFFERENT $(wc -l < "$W/$REV/$f") / $(wc -l < "$W/tree/$f") lines, $(diff "$W/$REV/$f" "$W/tree/$f" | grep -c '^<') differ"
  echo "$f $a $b $v"
done
