#!/bin/bash
# Build one profiling library per row-engine scope (reg_engine.hpp RG_PROF_ONLY): each times only its
# own scope, so no scope pays for the s_memtime pairs of the scopes inside it.
# Usage (here, after `make prof`): bash tools/rg_prof_only.sh [scope...]   -> fluidframework_amd/_build/rp_<name>/libmte.so
# (no scope named: all of them)
set -e
cd "$(dirname "$0")/../fluidframework_amd/csrc"
B=../_build
declare -A S=([apply]=2 [resolve]=3 [insert_slot]=4 [split]=5 [range]=6 [zamboni]=7 [scour]=8 [heap]=9 \
              [find_seg]=10 [pack]=11 [lru]=12 [split_at]=21 [op_ins]=22 [op_rem]=23 [zam_msn]=24 [zam_edit]=25 [pack_sibs]=26 [pack_fused]=27)
# (pack_fused, the fused pack, stands against pack_sibs + pack of a build without it; lone_doc.py reports
# them as scour_write, scour_chain and pack)
build() {
  # mte_solo.o alone into rp_<name>, the prof build's other objects, the Makefile's link rule
  rm -f $B/rp_$1/mte_solo.o
  make -s B=$B/prof SOLO=$B/rp_$1 \
    CXXFLAGS="-O3 -std=c++17 -fPIC -Wall -Wno-unused-function -Wno-unused-variable -DMTE_PROFILE -DRG_PROF_ONLY=$2"
}
n=0
for k in ${@:-${!S[@]}}; do
  [ -n "${S[$k]}" ] || { echo "no scope $k"; exit 1; }
  build $k ${S[$k]} &
  n=$((n+1)); if [ $((n % 4)) -eq 0 ]; then wait; fi
done
wait
ls $B | grep rp_ | tr '\n' ' '; echo
