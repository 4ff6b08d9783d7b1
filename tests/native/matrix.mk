# TEST INFRASTRUCTURE: the host plan of the SharedMatrix reads (matrix_plan.hpp) and the CPU build of their
# wave programs and table bodies (matrix_walk.hpp, matrix_table.hpp under MTE_CPU) as a stand-alone host
# program under ASan and UBSan (tests/test_matrix_reads_cpu.py), with no HIP runtime and no libmte.so in its
# link:
#   make -f matrix.mk _build/matrix_main
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build
CSRC := ../../fluidframework_amd/csrc
ROCM ?= $(abspath $(dir $(HIPCC))..)
HOSTCXX ?= $(ROCM)/bin/amdclang++
$(OUT)/matrix_main: matrix_main.cpp $(CSRC)/matrix.h $(CSRC)/matrix_plan.hpp $(CSRC)/matrix_walk.hpp $(CSRC)/matrix_table.hpp $(CSRC)/wave_simd.hpp ../../include/mte.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -x c++ -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -DMTE_CPU -o $@ matrix_main.cpp
