#!/bin/bash
# Proof recipe for "this refactor does not change the machine code":  tools/text_hash.sh OUTDIR [extra hipcc flags]
# compiles every device translation unit of csrc/sources.sh for gfx950 and prints, per unit, the sha256 of the code object's
# .text section and of its kernel resource metadata (registers, scratch, LDS, kernarg size per kernel name; OUTDIR/*.meta).
# Run it on two commits (and once more with -DGNR_SPLIT16=0) and compare the lines.  Two compiles of one tree differ outside .text.
set -e
OUT=$(mkdir -p "$1" && cd "$1" && pwd); shift
cd "$(dirname "$0")/../graspnerf_amd/csrc" && . ./sources.sh
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
for f in $SRC; do
  [ "${f%.hip}" = "$f" ] && continue
  hipcc $CFLAGS --offload-device-only -c "$@" -o $OUT/$f.o $f
  $LLVM/clang-offload-bundler --unbundle --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 --input=$OUT/$f.o --output=$OUT/$f.co
  $LLVM/llvm-objcopy -O binary --only-section=.text $OUT/$f.co $OUT/$f.text
  $LLVM/llvm-readelf --notes $OUT/$f.co | grep -E '^ +-? *\.(name|[vas]gpr_count|private_segment_fixed_size|group_segment_fixed_size|kernarg_segment_size):' > $OUT/$f.meta
  echo "$f text $(sha256sum < $OUT/$f.text | cut -c1-64) meta $(sha256sum < $OUT/$f.meta | cut -c1-64)"
done
