// HIP kernels of incremental replay on the block engine (gfx950, option retain). A unit of its own:
// the kernels of a pass without retain (mte_kernels.hip, mte_solo.hip) are compiled from the code they
// were, the same rule k_solo<.., CK> and k_rows<.., CK> follow.
//
//   k_blk_ck<LVL>: one wave per listed document -- the documents of a retained pass that the row
//               engines cannot hold (summary loads, relative positions, 64+ clients, '\n' beside
//               properties, local edits) -- on Engine<false, false, LVL> in a per-document HBM region
//               the host laid out (DocCfg::hb_*, as k_hbm's). It continues from the document's block
//               checkpoint of the previous pass when its log extends that pass's (Engine::ckpt_resume),
//               replays the rest and leaves this pass's checkpoint (Engine::ckpt_save).
//   k_blk_ck_clear: the header word of every listed document's region of this pass, so that a region
//               the pass leaves unwritten (a failed document) is not valid; the regions themselves are
//               never cleared.
#include "wave_hip.hpp"
#include "engine.hpp"
#include "mte_kernels.h"

namespace mte {

template <int LVL>
__global__ __launch_bounds__(64) void k_blk_ck(Params p, u32* saved) {
    const u32 d = p.doc_list[blockIdx.x];
    const u64 i0 = p.docs[d].op_begin;
    Engine<false, false, LVL> e(p, d);
    e.bind_hbm();
    e.init();
    u64 at = e.ckpt_resume(i0);
    at = e.replay_run(at);
    if (e.ckpt_save(at - i0) && lane_id() == 0) atomicAdd(saved, 1u);
    e.finish();
}

__global__ __launch_bounds__(64) void k_blk_ck_clear(Params p) {
    const u32 i = blockIdx.x * 64 + threadIdx.x;
    if (i >= p.n_list) return;
    const DocCfg& c = p.docs[p.doc_list[i]];
    if (c.ck_cap) p.ck_out[c.ck_out_off + BCK_VALID] = 0u;
}

// The key and value ids in the map records of kept block checkpoints, renumbered in place from the
// tables of the pass that wrote them to the tables of the batch just loaded (key_xl / val_xl: old id ->
// new id, by the interned text). One wave per listed region (off: its first word in ck, cap: its
// words); a region without a valid header, or whose records would lie outside it, is left alone (its
// resume then fails the header check or finds ids that match nothing: never out of bounds).
__global__ __launch_bounds__(64) void k_ck_xlate(u32* ck, const u64* off, const u64* cap, u32 n, const u32* key_xl, u32 n_keys,
                                                 const u32* val_xl, u32 n_vals, u32 mw) {
    if (blockIdx.x >= n) return;
    u32* base = ck + off[blockIdx.x];
    const u64 words = cap[blockIdx.x];
    if (words < BCK_HDR_WORDS || base[BCK_VALID] != BCK_MAGIC || !(base[BCK_FLAGS] & 1u) || base[BCK_MW] != mw) return;
    const u64 maps = (u64)base[BCK_MAPS_LO] | ((u64)base[BCK_MAPS_HI] << 32);
    const u32 nmap = base[BCK_NMAP];
    if (maps < BCK_HDR_WORDS || maps > words || (u64)nmap * mw > words - maps) return;
    const u32 maxp = (mw - 1) / 2;
    for (u32 r = 1 + threadIdx.x; r < nmap; r += 64) {  // (map id 0 is "undefined": no record)
        u32* m = base + maps + (u64)r * mw;
        const u32 np = m[0] < maxp ? m[0] : maxp;
        for (u32 i = 0; i < np; i++) {
            const u32 k = m[1 + 2 * i], v = m[2 + 2 * i];
            m[1 + 2 * i] = k < n_keys ? key_xl[k] : NONE;
            m[2 + 2 * i] = v < n_vals ? val_xl[v] : NONE;
        }
    }
}

hipError_t launch_ck_xlate(u32* ck, const u64* off, const u64* cap, u32 n, const u32* key_xl, u32 n_keys, const u32* val_xl,
                           u32 n_vals, u32 map_words, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_ck_xlate, dim3(n), dim3(64), 0, s, ck, off, cap, n, key_xl, n_keys, val_xl, n_vals, map_words);
    return hipGetLastError();
}

hipError_t launch_blk_ck(const Params& p, int full, u32 n_docs, u32* saved, hipStream_t s) {
    if (!n_docs) return hipSuccess;
    if (full > 1 || !p.ck_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_blk_ck_clear, dim3((n_docs + 63) / 64), dim3(64), 0, s, p);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    void* args[] = {(void*)&p, (void*)&saved};
    return hipLaunchKernel(full == 1 ? (const void*)k_blk_ck<1> : (const void*)k_blk_ck<0>, dim3(n_docs), dim3(64), args, 0, s);
}

}  // namespace mte
