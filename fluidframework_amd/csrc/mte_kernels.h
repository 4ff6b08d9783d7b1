// Kernel launchers (mte_kernels.hip) used by the host side (engine_run.cpp). full: the engine level
// (0 lean, 1 FULL, 2 FULL + EXT; engine.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "engine_types.hpp"

namespace mte {
// Kernel instantiations: the generator always runs the FULL engine (its C3 kind uses properties);
// a replay runs the lean one (level 0) when the host found the batch free of the optional features,
// the EXT one (level 2) when it carries catch-up records or permutation runs, else FULL (level 1)
// (engine_load.cpp mte_load).
#define MTE_PICK(K, gen, lvl)                                                                           \
    ((gen) ? (const void*)K<true, 1> : (lvl) >= 2 ? (const void*)K<false, 2> : (lvl) == 1 ? (const void*)K<false, 1> \
                                                                               : (const void*)K<false, 0>)

hipError_t launch_lds(const Params& p, bool gen, int full, u32 n_groups, hipStream_t s);
hipError_t launch_solo(const Params& p, bool gen, int full, u32 n_solo, bool ck, hipStream_t s);
// wait (one wave, <= 20 ms) until `n_solo` solo workgroups have started: issued on the bulk's stream
hipError_t launch_solo_gate(const u32* started, u32 n_solo, hipStream_t s);
// lean replays: the bulk (doc_list[n_prio ..)) on the row engine, waves_per_cu 4 or 8 per CU
hipError_t launch_rows(const Params& p, u32 waves_per_cu, u32 n_groups, bool props, bool wide, bool ck, hipStream_t s);
hipError_t launch_hbmq(const Params& p, bool gen, int full, u32 n_waves, hipStream_t s);
// ck (option retain): the instantiation that also leaves block checkpoints (Engine::ckpt_save)
hipError_t launch_rows_cont(const Params& p, bool props, bool wide, bool ck, u32 n_slots, hipStream_t s);
extern const u64 ROWS_DUMP_BYTES;  // a slot must hold k_rows' state dump (reg_engine.hpp DUMP_BYTES)
hipError_t launch_hbm(const Params& p, bool gen, int full, u32 n_docs, hipStream_t s);
// mte_ckpt.hip, option retain: the listed documents (doc_list[0, n_docs), DocCfg::hb_* regions in p.hbm) on
// the block engine, continuing from and leaving block checkpoints; *saved counts the checkpoints written
hipError_t launch_blk_ck(const Params& p, int full, u32 n_docs, u32* saved, hipStream_t s);
// renumber the key / value ids in the map records of n kept block checkpoints (regions off[i], cap[i] words
// of ck) through key_xl / val_xl (old id -> new id)
hipError_t launch_ck_xlate(u32* ck, const u64* off, const u64* cap, u32 n, const u32* key_xl, u32 n_keys, const u32* val_xl,
                           u32 n_vals, u32 map_words, hipStream_t s);
hipError_t launch_wave_selftest(const u32* in, u32* out, u32 n_waves, hipStream_t s);
}  // namespace mte
