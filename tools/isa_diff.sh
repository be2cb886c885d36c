#!/bin/bash
# Are the gfx950 instructions of two revisions of the kernels the same?  Compiles what the library ships -- KERNELS of csrc/sources.mk as revB lists them, each
# revision with its own HIPFLAGS and per-file FLAGS_<name> of csrc/Makefile -- and diffs the device assembly (comments, debug labels, __hip_cuid_* dropped).
# Used to tie a late host-side / comment-only / ifdef-only commit to the GPU passes of an earlier one.
# usage: bash tools/isa_diff.sh <revA> <revB> [file.hip ...]        (no GPU needed)
set -u
A=$1; B=$2; shift 2
T=$(mktemp -d)
for r in $A $B; do mkdir -p $T/$r; git archive $r ntransformer_amd/csrc include | tar -x -C $T/$r; done
# variable $2 of revision $1's csrc/Makefile
mkvar() { make -s -C $T/$1/ntransformer_amd/csrc --eval 'isa-diff-var: ; @echo $($(V))' V=$2 isa-diff-var; }
FILES=${*:-$(mkvar $B KERNELS)}
rc=0
for f in $FILES; do
  for r in $A $B; do
    ( cd $T/$r/ntransformer_amd/csrc && [ -f $f ] && $(mkvar $r HIPCC) $(mkvar $r HIPFLAGS) $(mkvar $r FLAGS_${f%.hip}) -I$T/$r/include -I. -c $f -o $T/$r/${f%.hip}.o --save-temps 2>/dev/null
      grep -v "^\s*;\|^\s*\.\(file\|loc\|ident\)\|\.Ltmp\|\.Lfunc\|__hip_cuid_\|^\s*$" ${f%.hip}-hip-amdgcn-amd-amdhsa-gfx950.s 2>/dev/null | sed 's/;.*$//' > $T/$r/${f%.hip}.code.s ) &
  done; wait
  n=$(diff $T/$A/${f%.hip}.code.s $T/$B/${f%.hip}.code.s | wc -l)
  echo "$f: $n differing lines of $(wc -l < $T/$B/${f%.hip}.code.s)"
  [ "$n" = 0 ] && [ -s $T/$B/${f%.hip}.code.s ] || rc=1   # (an empty listing is a failed compile, not a match)
done
rm -rf $T
exit $rc
