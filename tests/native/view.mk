# TEST INFRASTRUCTURE: the host plan of the view queries (view_plan.hpp) and the CPU build of their wave
# programs (view_walk.hpp under MTE_CPU) as a stand-alone host program under ASan and UBSan
# (tests/test_views_cpu.py), with no HIP runtime and no libmte.so in its link:
#   make -f view.mk _build/view_main
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build
CSRC := ../../fluidframework_amd/csrc
ROCM ?= $(abspath $(dir $(HIPCC))..)
HOSTCXX ?= $(ROCM)/bin/amdclang++
$(OUT)/view_main: view_main.cpp $(CSRC)/view.h $(CSRC)/view_plan.hpp $(CSRC)/view_walk.hpp $(CSRC)/wave_simd.hpp ../../include/mte.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -x c++ -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -DMTE_CPU -o $@ view_main.cpp
