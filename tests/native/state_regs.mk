# TEST INFRASTRUCTURE: the statistics build of the CPU row engine as a stand-alone host program under
# ASan and UBSan (tests/test_state_regs_native.py, tests/test_reg_state_regs_cpu.py), with no HIP runtime
# in its link:
#   make -f state_regs.mk _build/state_regs_main
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build
CSRC := ../../fluidframework_amd/csrc
ROCM ?= $(abspath $(dir $(HIPCC))..)
HOSTCXX ?= $(ROCM)/bin/amdclang++
$(OUT)/state_regs_main: state_regs_main.cpp reg_cpu.cpp $(CSRC)/reg_engine.hpp $(CSRC)/reg_rows.hpp $(CSRC)/wave_simd.hpp $(CSRC)/engine_types.hpp ../../include/mte.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -x c++ -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ -o $@ state_regs_main.cpp
