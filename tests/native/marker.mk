# TEST INFRASTRUCTURE: the host plan of the marker queries (marker_plan.hpp) and the CPU build of their
# wave programs (marker_walk.hpp under MTE_CPU) as a stand-alone host program under ASan and UBSan
# (tests/test_markers_cpu.py), with no HIP runtime and no libmte.so in its link:
#   make -f marker.mk _build/marker_main
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build
CSRC := ../../fluidframework_amd/csrc
ROCM ?= $(abspath $(dir $(HIPCC))..)
HOSTCXX ?= $(ROCM)/bin/amdclang++
$(OUT)/marker_main: marker_main.cpp $(CSRC)/marker.h $(CSRC)/marker_plan.hpp $(CSRC)/marker_walk.hpp $(CSRC)/wave_simd.hpp $(CSRC)/jsonlite.hpp ../../include/mte.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -x c++ -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -DMTE_CPU -o $@ marker_main.cpp
