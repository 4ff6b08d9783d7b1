#!/bin/bash
# Build a k_solo-only experiment library: mte_solo.hip with extra flags, linked with the default
# build's other objects. Usage: bash tools/solo_variant.sh <name> [extra hipcc flags...]
#   -> fluidframework_amd/_build/<name>/libmte.so  (select on the GPU box with MTE_LIB=<name>)
set -e
cd "$(dirname "$0")/../fluidframework_amd/csrc"
B=../_build
V=$1; shift
make -s -C . >/dev/null
# mte_solo.o alone into $B/$V (always recompiled: the flags differ from run to run), the default
# build's other objects, the Makefile's link rule; each extra flag stays one word
rm -f $B/$V/mte_solo.o
make -s SOLO=$B/$V SOLOFLAGS="${SOLOFLAGS--mllvm -amdgpu-sched-strategy=iterative-ilp} ${*@Q}"
echo "$B/$V/libmte.so"
