#!/bin/bash
# Checks that a change leaves the device code alone: tools/asm_identity.sh [REF]
# compiles every HIP translation unit of REF (default HEAD) and of the working tree to
# device assembly, each side with its own Makefile's FLAGS and unit list, and compares
# the texts byte for byte (-cuid=cmp fixes the one symbol that depends on the source
# path). For refactors of the shared kernel sources: identical assembly is identical
# behaviour and speed. A unit that does not compile prints its compiler output.
# EXTRA="-DBDPT_WLEAF_GROUP=1" tools/asm_identity.sh [REF] appends the flags to both sides'
# compile lines (the side libraries' and the probes' switches); a unit that then compiles
# on neither side (a flag it never takes) is reported and does not count.
set -e
cd "$(dirname "$0")/.."
PKG=bidirectional-path-tracing_amd
T=$(mktemp -d); trap 'rm -rf "$T"' EXIT
mkdir "$T/old" "$T/new"
git archive "${1:-HEAD}" $PKG include | tar -x -C "$T/old"
cp -r $PKG include "$T/new"
units() {  # the side's HIP units: the Makefile's list, or every csrc/*.hip of a tree without one
  (cd "$T/$1/$PKG" && { make -s print-HIP_TUS 2>/dev/null || ls csrc/*.hip | sed 's|csrc/||; s|\.hip$||'; })
}
rc=0
for side in old new; do
  cd "$T/$side/$PKG"
  FLAGS=$(make -s print-FLAGS 2>/dev/null || make -s -C "$T/new/$PKG" print-FLAGS)
  HIPCC=$(make -s -C "$T/new/$PKG" print-HIPCC)
  units $side | tr ' ' '\n' | grep . | xargs -P "${JOBS:-16}" -I{} sh -c \
    "$HIPCC $FLAGS $EXTRA --cuda-device-only -S -cuid=cmp -x hip csrc/{}.hip -o {}.s 2>{}.log || { echo 'FAILED $side {}:'; cat {}.log; }"
  cd - >/dev/null
done
if [ "$(units old | tr ' ' '\n' | sort | xargs)" != "$(units new | tr ' ' '\n' | sort | xargs)" ]; then
  echo "unit lists differ: old: $(units old | xargs)  new: $(units new | xargs)"; rc=1
fi
for t in $(units new); do
  if [ -s "$T/old/$PKG/$t.s" ] && cmp -s "$T/old/$PKG/$t.s" "$T/new/$PKG/$t.s"; then echo "same   $t"
  elif [ -n "$EXTRA" ] && [ ! -s "$T/old/$PKG/$t.s" ] && [ ! -s "$T/new/$PKG/$t.s" ]; then echo "neither $t"
  else echo "DIFFER $t"; rc=1; fi
done
exit $rc
