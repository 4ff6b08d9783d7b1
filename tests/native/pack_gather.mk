# TEST INFRASTRUCTURE for the fused pack (reg_engine.hpp pack_fused; tests/test_reg_pack_gather_cpu.py,
# tests/test_pack_gather_native.py):
#   make -f pack_gather.mk _build/libregcpu_unfused.so   the statistics build with every engine on the
#                                                         sibling loop and pack_leaves (MTE_FUSED_PACK=0)
#   make -f pack_gather.mk _build/pack_gather_main       the statistics build as a stand-alone host program
#                                                         under ASan and UBSan, no HIP runtime in its link
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build
CSRC := ../../fluidframework_amd/csrc
ROCM ?= $(abspath $(dir $(HIPCC))..)
HOSTCXX ?= $(ROCM)/bin/amdclang++
DEPS := reg_cpu.cpp $(CSRC)/reg_engine.hpp $(CSRC)/reg_rows.hpp $(CSRC)/wave_simd.hpp $(CSRC)/engine_types.hpp ../../include/mte.h
$(OUT)/libregcpu_unfused.so: $(DEPS)
	@mkdir -p $(OUT)
	$(HIPCC) -O2 -std=c++17 -fPIC -shared -Wall -Wno-unused-function -Wno-unused-variable -DMTE_CPU_STATS -DMTE_FUSED_PACK=0 -o $@ reg_cpu.cpp
$(OUT)/pack_gather_main: pack_gather_main.cpp $(DEPS)
	@mkdir -p $(OUT)
	$(HOSTCXX) -x c++ -O1 -g -std=c++17 -Wall -Wno-unused-function -Wno-unused-variable -fsanitize=address,undefined \
	  -fno-sanitize-recover=undefined -I$(ROCM)/include -D__HIP_PLATFORM_AMD__ -o $@ pack_gather_main.cpp
