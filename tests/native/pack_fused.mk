# TEST INFRASTRUCTURE: the statistics build of the CPU row engine as a stand-alone host program under
# ASan and UBSan (tests/test_pack_fused_native.py), with no HIP runtime in its link:
#   make -f pack_fused.mk _build/pack_fused_main
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build
CSRC := ../../fluidframework_amd/csrc
ROCM ?= $(abspath $(dir $(HIPCC))..)
HOSTCXX ?= $(ROCM)/bin/amdclang++
$(OUT)/pack_fused_main: pack_fused_main.cpp reg_cpu.cpp $(CSRC)/reg_engine.hpp $(CSRC)/reg_rows.hpp $(CSRC)/wave_simd.hpp $(CSRC)/engine_types.hpp ../../include/mte.h
	@mkdir -p $(OUT)
	$(HOSTCXX) -x c++ -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ -o $@ pack_fused_main.cpp
