// reg_engine.hpp — the row-vectorised replay engine for critical-path documents (k_solo).
//
// Same observer replay as engine.hpp (@fluidframework/merge-tree 0.31.0; paths relative to
// packages/dds/merge-tree/src), same B-tree shape and lazy zamboni schedule, restructured so that one
// op is a short run of wave-wide instructions with few dependent memory round trips:
//   * leaf blocks in DOCUMENT ORDER, 8 per "row": block k's slot s is lane 8*(k&7)+s of row k>>3.
//     A row is 64 slots = 64 lanes, held in LDS exactly where the LDS engine's SoloPlan keeps slots
//     (vis = len, seq, removedSeq, meta; aux = -, text offset, text capacity / overlap mask,
//     segment id): one ds_read_b128 per lane fetches a whole row's visibility fields. An empty slot
//     has len 0 (segments are never empty), so a block's child count is a popcount of one ballot.
//     The rows themselves -- storage, page table, pool, the one-row register cache -- are
//     reg_rows.hpp's RowStore, which this engine holds as `rows`;
//   * position resolution (insertingWalk + nodeLength, mergeTree.ts:2345-2474,1659-1699): per row
//     ONE predicate evaluation for 64 slots and ONE DPP prefix scan; the first block whose
//     cumulative end reaches pos wins (blocks win ties, :2274-2276), then the slot inside it
//     (breakTie, :2248-2277) from the same registers. No per-block summaries to maintain;
//   * edits of a block are lane-parallel on its row (DPP shifts inside the 8-lane group); a block
//     split or pack moves the blocks after it as one LDS memmove;
//   * interior B-tree levels as child-COUNT vectors in VGPRs (lane = node at that level, document
//     order): a parent is a prefix-sum lookup, a split 8 -> 4+4 a one-lane shift (mergeTree.ts:
//     2446-2489, 1876-1887), pack a redistribution of counts (:1368-1420);
//   * needsScour tri-state (mergeTree.ts:63,1279) in spare meta bits of every slot of its block, so
//     it moves with the block;
//   * the LRU heap (collections.ts:213-265) in 2 x 8 VGPRs, positions 1..511;
//   * op records prefetched 8 per VGPR, decoded with v_readlane.
// Text stays in HBM (the op payload and the merge arena), as in engine.hpp. Live segments carry
// removedSeq RSEQ_LIVE and removedClient RCL_LIVE so the visibility predicate needs no removed test.
// A document whose state outgrows this plan, or that reaches an op this engine does not implement
// (annotate, summary load records, relative positions, legacy catch-up, permutation runs), hands its
// state to the LDS engine between two ops (reg_handoff.hpp) and continues there.
// The same source also builds for the CPU: everything that differs there is behind wave_simd.hpp and
// reg_rows.hpp (MTE_CPU; in this file it only switches the profile and statistics blocks off or on,
// and gives the CPU pool's size the name the CPU harness has always set, RegEngine::pool_rows).
// The CPU suite checks it against the oracle (tests/test_reg_engine_cpu.py); the product runs the
// device build only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "engine_types.hpp"
#include "reg_rows.hpp"
#include "wave_simd.hpp"

namespace mte {

constexpr u32 RG_LEVELS = 8;              // interior levels (height <= RG_LEVELS + 1)
constexpr u32 RG_HEAP = 511;              // LRU heap positions 1..511
constexpr u32 RSEQ_LIVE = 0x7FFFFFFFu;    // removedSeq of a live segment (never <= a refSeq)
constexpr u32 RCL_LIVE = 0xFFu;           // removedClient byte of a live segment (never a client)
constexpr i32 REG_HANDOFF = 101;          // internal: continue in the LDS engine from the current op
// needsScour (mergeTree.ts:63) in meta bits 24..25 of every slot lane of a block
constexpr u32 NS_SHIFT = 24, NS_MASK = 3u << NS_SHIFT;

// Phase profile of the row engine (MTE_PROFILE device builds, `make prof`): inclusive s_memtime
// cycles and event counts accumulated in registers and written once per document by finish(), in
// the LDS engine's slot numbering (engine.hpp ProfSlot, mte.PROF_NAMES).
enum RgProf : u32 {
    RP_TOTAL, RP_FETCH, RP_APPLY, RP_RESOLVE, RP_INSERT_SLOT, RP_SPLIT, RP_RANGE, RP_ZAMBONI, RP_SCOUR,
    RP_HEAP, RP_FIND_SEG, RP_PACK, RP_LRU, RP_OPS, RP_N_RESOLVE, RP_N_SCOUR, RP_N_SCOUR_CHANGED,
    RP_N_PACK, RP_N_POP, RP_N_SPLIT_BLK, RP_N_MOVE, RP_SPLIT_AT, RP_INS, RP_REM, RP_MSN, RP_ZAM_EDIT,
    RP_PACK_SIBS,  // pack's sibling pass (zamboni's loop of scours in front of pack_leaves); reported as "scour_chain"
    RP_PACK_FUSED,  // the fused pack (pack_fused: both of the above in one pass); reported as "scour_write"
    RP_N
};
#if defined(MTE_PROFILE) && !defined(MTE_CPU)
// RG_PROF_ONLY=<slot>: time that one scope only (each s_memtime pair costs a lone wave ~100 cycles,
// which a full profile charges to the enclosing scopes); RP_TOTAL and the event counts stay on
#ifdef RG_PROF_ONLY
#define RG_ON(slot) ((slot) == RG_PROF_ONLY || (slot) == RP_TOTAL)
#else
#define RG_ON(slot) true
#endif
template <bool ON>
struct RgScope {
    u64& acc;
    u64 t0;
    __device__ __forceinline__ RgScope(u64& a) : acc(a), t0(ON ? __builtin_amdgcn_s_memtime() : 0) {}
    __device__ __forceinline__ ~RgScope() {
        if (ON) acc += __builtin_amdgcn_s_memtime() - t0;
    }
};
#define RG_PROF(slot) RgScope<RG_ON(slot)> _rg_scope_##slot(pf[slot])
#define RG_COUNT(slot, n) (pf[slot] += (u64)(n))
#elif defined(MTE_MARKERS) && !defined(MTE_CPU)
// static code inspection: row-engine scopes as assembly comments "MTE_BEGIN 100+slot"
template <u32 S>
struct RgMark {
    __device__ __forceinline__ RgMark() { asm volatile("; MTE_BEGIN %0" ::"i"(S + 100)); }
    __device__ __forceinline__ ~RgMark() { asm volatile("; MTE_END %0" ::"i"(S + 100)); }
};
#define RG_PROF(slot) RgMark<slot> _rg_mark_##slot
#define RG_COUNT(slot, n) \
    do {                  \
    } while (0)
#else
#define RG_PROF(slot) \
    do {              \
    } while (0)
#define RG_COUNT(slot, n) \
    do {                  \
    } while (0)
#endif

// Event statistics of the CPU build (MTE_CPU_STATS, tools/rg_stats.py only): what the critical
// document's ops do (rows a resolve scans, heap sizes at a pop, scour outcomes), to size the device
// code paths. Nothing in a device build.
#if defined(MTE_CPU) && defined(MTE_CPU_STATS)
enum RgStat : u32 {
    RS_OPS, RS_RESOLVE, RS_RES_ROWS, RS_RES_NROWS, RS_POP, RS_POP_BIG, RS_POP_HEAP, RS_FIND_ROWS, RS_SCOUR,
    RS_SCOUR_NOP, RS_SCOUR_SERIAL, RS_SCOUR_COPY, RS_PACK, RS_SPLIT_BLK, RS_MOVE_SLOTS, RS_SPLIT_AT,
    RS_ZAM_CALLS, RS_ZAM_POPS, RS_LRU_PUSH, RS_RANGE_ROWS, RS_DUO_HANDOVER, RS_DUO_SPEC_OK, RS_DUO_SPEC_REDO,
    RS_DUO_NO_RESOLVE, RS_DUO_W_ROWS,
    // removes (op_remove): all; p2's block in p1's row; of those, neither split split its block; the
    // rows second resolves scan (RS_RANGE_ROWS: the rows marking passes scan). Pack's sibling pass: its
    // scour calls and the ones among them that left their block as it was.
    RS_REM, RS_REM_SAMEROW, RS_REM_SAMEROW_NOSPLIT, RS_RES2_ROWS, RS_PACK_SCOUR, RS_PACK_SCOUR_NOP,
    // The shape of a pack (profiles/r10/pack_stats.json): the times the sibling pass's second scour of
    // the popped block changed it (not a no-op: it cannot be skipped); the other siblings the pass
    // changed; packs whose siblings lie in one row / in two; with a sibling on the serial
    // walk; with an arena_gc during the pass; that cascade into pack_internal; with 8 siblings; that
    // end with more blocks than siblings; the sums of siblings (m) and of resulting blocks (kk).
    RS_PACK_SELF_CHANGED, RS_PACK_SIB_CHANGED, RS_PACK_ONE_ROW, RS_PACK_TWO_ROWS, RS_PACK_SERIAL, RS_PACK_GC,
    RS_PACK_CASCADE, RS_PACK_M8, RS_PACK_GROWS, RS_PACK_M_SUM, RS_PACK_KK_SUM,
    // needsScour marks (add_lru): written as a second write of the row the edit has just written, and
    // folded into the edit's own row write
    RS_LRU_REWRITE, RS_LRU_FOLDED,
    // packs taken by pack_fused, and the ones it handed back before any side effect: a joining slot longer
    // than GRANULARITY (the serial walk), fresh chunks that do not fit the arena (arena_gc)
    RS_PACK_FUSED, RS_PACK_FUSED_FB_SERIAL, RS_PACK_FUSED_FB_GC,
    // The places round 13 looked at (tests/test_reg_state_regs_cpu.py; kHeapInPlace and kMulDiv change the heap
    // writes and the packs' divisions, the others count code that stayed as it was): resolves of documents
    // of three or more rows that hit in their first / second row buffer; block splits whose new block starts
    // the next row; heap entries written to register 1 (positions 64..127) and to registers 2..7; pops on the
    // serial sift; packs by kk (RS_PACK_KK1 + kk - 1) and the ones with T % kk != 0; pack_internal rounds;
    // ops room() refused
    RS_HIT_FIRST, RS_HIT_SECOND, RS_SPLIT_NEXT_ROW, RS_HEAP_REG1, RS_HEAP_REG2, RS_SIFT_SERIAL, RS_PACK_KK1, RS_PACK_KK2,
    RS_PACK_KK3, RS_PACK_KK4, RS_PACK_KK5, RS_PACK_KK6, RS_PACK_KK7, RS_PACK_REM, RS_PACK_INTERNAL, RS_ROOM_REFUSED, RS_N
};
inline u64 g_rg_stats[RS_N + 64];
#define RG_STAT(i, n) (g_rg_stats[i] += (u64)(n))
// What a settle half running on a second wave would meet, counted on one wave: an op
// whose settle pops the heap is a handover; W collects the rows its scours rewrote with other
// contents (and every row from a pack's first row on); the next op's first resolve, done beside that
// settle, would stand when W misses the rows it scanned and no pack ran, else it is repeated.
struct RgDuoStat {
    u64 w;
    bool popped, packed, pending;
    void settle_begin() {
        if (pending) RG_STAT(RS_DUO_NO_RESOLVE, 1);  // (the op after the handover resolved nothing)
        w = 0;
        popped = packed = pending = false;
    }
    void settle_end() {
        if (!popped) return;
        RG_STAT(RS_DUO_HANDOVER, 1);
        RG_STAT(RS_DUO_W_ROWS, __builtin_popcountll(w));
        pending = true;
    }
    void resolved(bool ok, u32 row) {  // rows [0, row] scanned (every row when nothing was found)
        if (!pending) return;
        pending = false;
        const u64 scanned = ok && row < 63 ? (2ull << row) - 1 : ~0ull;
        if (packed || (w & scanned)) RG_STAT(RS_DUO_SPEC_REDO, 1);
        else RG_STAT(RS_DUO_SPEC_OK, 1);
    }
};
inline RgDuoStat g_rg_duo;
#define RG_DUO(stmt) (g_rg_duo.stmt)
#else
#define RG_STAT(i, n) \
    do {              \
    } while (0)
#define RG_DUO(stmt) \
    do {             \
    } while (0)
#endif

#ifndef MTE_FUSED_PACK
#define MTE_FUSED_PACK 1  // RegEngine::kFusedPack
#endif
// The parts of round 13, one bit each: 1 RegEngine::kHeapInPlace, 4 RegEngine::kMulDiv.
// 0 builds neither: the A/B twin. (Bit 2 was resolve's hit taken from the buffer that hit, 8 one exit
// from the replay loop, 16 the loop's state re-homed at the head of each op: measured slower, removed.)
#ifndef MTE_STATE_REGS
#define MTE_STATE_REGS 5
#endif

struct RSeg {
    u32 len;
    i32 seq;
    u32 rseq;
    u32 meta;
    u32 toff;
    u32 cap;  // owned merge-arena capacity from toff (0 for payload text)
    u32 rm;   // removers: bit c for removedClient c and every client in removedClientOverlap
    u32 sid;
    u32 props = 0;  // property map id (PROPS engines; 0 = no properties)
    u32 rm2 = 0;    // removers 32..63 (WIDE engines)
};
struct RFound {
    bool ok;
    u32 k;     // leaf block (document order)
    u32 cnt;   // its child count
    i32 slot;  // first qualifying slot, -1 => append at the block end
    i32 r;     // pos - cumBefore(slot)
    u32 row;   // the row of block k
    u32 carry; // visible length before that row
};

// PAGED (k_rows): logical row r of the document lives in pool row ptab[r] of a pool the CU's waves
// share (rows_pool_*), taken as the document grows and given back as it shrinks or ends; a document
// the pool cannot grow is spilled (REG_HANDOFF, re-run by the host). Otherwise row r is slot row r.
// PROPS (k_rows of property-carrying batches): a ninth slot field, the segment's property map id
// (immutable maps in the document's HBM map table, SegmentPropertiesManager.addProperties), annotate
// ops, and merges that require matching properties.
// WIDE (k_solo's property-carrying instantiation): clients 32..63 too, a second removers word per slot.
template <int NR = (int)RG_ROWS, bool PAGED = false, bool PROPS = false, bool WIDE = false>
struct RegEngine {
    static constexpr bool kProps = PROPS, kWide = WIDE;
    // An edit's needsScour marks go into the row write the edit makes anyway (insert_slot, op_remove) on
    // the engines that own a whole row store: k_solo's and k_rows_cont's. On k_rows (a quarter's fixed
    // rows, the paged pool) the same code measured slower -- C3 +7 %, C5 +1.4 %, C2 +1-3 %, the 12-wave
    // builds spilling 19-25 VGPRs more at their 168-register bound -- and they keep add_lru's second
    // write of the row.
    static constexpr bool kFoldLru = !PAGED && NR == (int)RG_ROWS;
    // A pack decides all its siblings at once and gathers the kept slots by mask (pack_fused) on the same
    // engines; elsewhere zamboni keeps the sibling loop of scours and pack_leaves.
    // (MTE_FUSED_PACK=0 / 2 builds it into no / every engine: the unfused twin of the CPU suite, A/B libraries.)
    static constexpr bool kFusedPack = MTE_FUSED_PACK == 2 || (MTE_FUSED_PACK == 1 && !PAGED && NR == (int)RG_ROWS);
    // Round 13, on the lean engines among those, so that every k_rows kernel and the PROPS /
    // WIDE k_solo kernels (not timed with these parts) stay the code they were: a heap entry is written by
    // a lane compare in each register it can be in, not by a branch per register (kHeapInPlace: the
    // sixteen heap registers have one home across a push and a pop); a pack's T / kk is a multiply and a
    // shift (kMulDiv).
    static constexpr bool kOwnRows = !PAGED && NR == (int)RG_ROWS && !PROPS && !WIDE;
    static constexpr bool kHeapInPlace = kOwnRows && (MTE_STATE_REGS & 1) != 0;
    static constexpr bool kMulDiv = kOwnRows && (MTE_STATE_REGS & 4) != 0;
    static constexpr u32 MAXC = WIDE ? 64u : 32u;  // client ids below this (rm, rm2)
    typedef simd::V V;
    typedef simd::B B;
    static constexpr u32 NBLK = (u32)NR * 8;
    typedef RowStore<NR, PAGED, PROPS, WIDE> Rows;
    typedef typename Rows::Row Row;

    // ---------------------------------------------------------------- state
    simd::VA<RG_LEVELS> LV;  // LV[i] lane j: child count of node j of level i+1 (0 beyond the last)
    // Heap positions q at lane q&63 of register q>>6. Registers 0 and 1 (positions 1..127, every pop
    // of a heap that size) are plain values; 2..7 an indexed array touched only by larger heaps (one
    // 8-register array made every pop copy all eight registers at its merge points).
    struct HeapRegs {
        V r0, r1, x2, x3, x4, x5, x6, x7;  // named registers: no access is ever indexed at run time
        SD V get(u32 i) const {
            switch (i) {
                case 0: return r0;
                case 1: return r1;
                case 2: return x2;
                case 3: return x3;
                case 4: return x4;
                case 5: return x5;
                case 6: return x6;
                default: return x7;
            }
        }
        SD void set(u32 i, V v) {
            switch (i) {
                case 0: r0 = v; break;
                case 1: r1 = v; break;
                case 2: x2 = v; break;
                case 3: x3 = v; break;
                case 4: x4 = v; break;
                case 5: x5 = v; break;
                case 6: x6 = v; break;
                default: x7 = v; break;
            }
        }
        SD void zero() { r0 = r1 = x2 = x3 = x4 = x5 = x6 = x7 = simd::splat(0); }
    };
    HeapRegs HK, HS;         // heap keys (maxSeq) / segment ids
    u32 n_lb, height, heapSize, segNext, arenaTop, arenaSel;
    i32 minSeq, curSeq, heapTop, status, failSeq;
    u32 n_gc, max_lb;
    u32 n_ops, n_msgs;
    SD u32 ops_n() const { return n_ops; }
    SD u32 msgs_n() const { return n_msgs; }
    SD void set_counts(u32 o, u32 m) {
        n_ops = o;
        n_msgs = m;
    }
    SD void count_op() { n_ops++; }
    SD void count_msg() { n_msgs++; }
    u32 lb_lim;  // leaf-block limit of room() (Params::reg_lb_limit, read once)
    bool adirty;
#if defined(MTE_PROFILE) && !defined(MTE_CPU)
    u64 pf[RP_N];
#endif
    // per document
    const Params& p;
    u32 doc;
    u16* payload;
    u16* arena0;
    u32 seg_cap, arena_cap, payload_len;
    Rows rows;  // the slot rows (reg_rows.hpp): LDS on the device, arrays in the CPU build
#ifdef MTE_CPU
    u32& pool_rows = rows.at.pool_rows;  // the CPU pool's size, where tests/native/reg_cpu.cpp sets it
#endif
    // a PAGED engine's rows back to the pool, when it is done with its document
    SD void release_rows() { rows.release_rows(); }

    SD V ld_len(u32 r) const { return rows.ldf(r, 0, 0); }
    SD V ld_meta(u32 r) const { return rows.ldf(r, 0, 3); }
    SD V ld_sid(u32 r) const { return rows.ldf(r, 1, 3); }
    // Room for leaf blocks [0, nb): PAGED takes pool rows (none left: spill the document, the host
    // re-runs it); otherwise the fixed rows must hold them.
    SD bool ensure_blocks(u32 nb) {
        if constexpr (PAGED) {
            if (rows.grow_rows((nb + 7) >> 3)) return true;
            fail(REG_HANDOFF, curSeq);
        } else {
            if (nb <= NBLK) return true;
            fail(MTE_DOC_CAPACITY, curSeq);
        }
        return false;
    }

    // g: where the rows are (lean k_solo's place unless told otherwise)
    SD RegEngine(const Params& p_, u32 doc_, const RowsLds& g = RowsLds::solo_lean())
        : p(p_), doc(doc_), rows(g), res_mode(g.mode) {
        setup();
    }
    u32 res_mode;  // DocRes::mode of a document this engine finishes (4: k_solo, 5: k_rows)
    SD void setup() {
        const DocCfg& c = p.docs[doc];
        payload = p.payload + c.payload_off;
        arena0 = p.arena + c.arena_off;
        seg_cap = c.seg_cap;
        arena_cap = c.arena_cap;
        payload_len = c.payload_len;
        init();
        if constexpr (PROPS) {
            mw = p.map_words;
            maps = p.maps + c.map_off * mw;
            map_cap = c.map_cap;
            mapNext = 1;  // map id 0 == no properties
            // TextSegment.canAppend reads the last character when the text has '\n': not modelled here
            if (c.has_nl) status = REG_HANDOFF;
        }
    }

    // ---------------------------------------------------------------- property maps (PROPS, HBM)
    // A map record is [n, key 0, value 0, key 1, value 1, ...] (mw words) in the document's map
    // table, immutable once built; id 0 = no properties. Lane i holds pair i.
    u32* maps = nullptr;
    u32 map_cap = 0, mw = 0, mapNext = 1;
    // matchProperties on one value, b uniform (properties.ts:72-80): equal ids, or b an object value
    // that a's deep-equality bits name
    SD B val_match(V a, u32 b) const {
        const B eq = a == simd::splat(b);
        if (!(p.val_flags[b] & 2u)) return eq;
        const u32 j = p.val_objidx[b];
        if (j == NONE) return eq;
        const V om = simd::ld(reinterpret_cast<const u32*>(p.val_objmatch), a * 2u + (j >> 5), simd::mk_all());
        return eq | (((om >> (j & 31u)) & 1u) != 0u);
    }
    // matchProperties of two maps (properties.ts:62-93)
    SD bool match_props(u32 a, u32 b) {
        if (a == b) return true;
        if (a == 0 || b == 0 || a >= map_cap || b >= map_cap) return false;
        fence_arena();  // map records are written lane-parallel (build_map)
        const u32* ma = maps + (u64)a * mw;
        const u32* mb = maps + (u64)b * mw;
        const u32 na = ma[0], nb = mb[0];
        if (na != nb) return false;
        const B in = L() < na;
        const V Ka = simd::ld(ma + 1, L() * 2u, in), Va = simd::ld(ma + 2, L() * 2u, in);
        const V Kb = simd::ld(mb + 1, L() * 2u, in), Vb = simd::ld(mb + 2, L() * 2u, in);
        B ok = ~in;
        for (u32 q = 0; q < nb; q++) {
            const u32 kq = simd::readlane(Kb, q), vq = simd::readlane(Vb, q);
            const B hit = in & (Ka == kq);
            if (simd::ballot(hit)) ok = ok | (hit & val_match(Va, vq));
        }
        return simd::ballot(~ok) == 0;
    }
    // SegmentPropertiesManager.addProperties (segmentPropertiesManager.ts:35-111) on an immutable map:
    // a fresh map id (the LDS engine's build_map, engine.hpp, lane for lane)
    SD u32 build_map(u32 old, u32 propset, bool rewrite) {
        if (mapNext >= map_cap) {  // the load-time estimate was short: the host re-runs it with the worst case
            fail(res_mode == 4 ? DOC_SPILL : REG_HANDOFF, curSeq);  // (k_solo cannot hand over mid-op)
            return 0;
        }
        fence_arena();
        const u32 maxp = (mw - 1) / 2 < MTE_MAX_PROPS ? (mw - 1) / 2 : MTE_MAX_PROPS;
        u32 n = 0;
        V K = simd::splat(0), Vv = simd::splat(0);
        if (old && old < map_cap) {
            const u32* mo = maps + (u64)old * mw;
            n = mo[0];
            if (n > maxp) n = maxp;
            K = simd::ld(mo + 1, L() * 2u, L() < n);
            Vv = simd::ld(mo + 2, L() * 2u, L() < n);
        }
        const mte_propset ps = p.propsets[propset];
        const u32 pc = ps.count, pf = ps.first;
        if (rewrite) {  // delete keys whose new value is falsy / absent (:65-78); order kept
            B keep = simd::mk_none();
            for (u32 q = 0; q < pc; q++) {
                const u32 k = p.prop_keys[pf + q];
                const bool falsy = (p.val_flags[p.prop_vals[pf + q]] & 1u) != 0;
                const B hit = (L() < n) & (K == k);
                keep = falsy ? simd::andn(keep, hit) : (keep | hit);
            }
            keep = keep & (L() < n);
            const u64 km = simd::ballot(keep);
            const u32 nk = (u32)__builtin_popcountll(km);
            const V below = simd::rank_below(km);
            const V dst = simd::sel(keep, below, (L() - below) + nk);  // a permutation of the lanes
            K = simd::push(K, dst);
            Vv = simd::push(Vv, dst);
            n = nk;
        }
        for (u32 q = 0; q < pc; q++) {
            const u32 k = p.prop_keys[pf + q], v = p.prop_vals[pf + q];
            const u64 hm = simd::ballot((L() < n) & (K == k));
            if (v == 0) {  // null deletes (:98-100): the pairs after it move down one lane
                if (hm) {
                    const u32 at = (u32)__builtin_ctzll(hm);
                    const V nxt = (L() + 1u) & 63u;
                    const V K1 = simd::bperm(K, nxt), V1 = simd::bperm(Vv, nxt);
                    const B mvd = L() >= at;
                    K = simd::sel(mvd, K1, K);
                    Vv = simd::sel(mvd, V1, Vv);
                    n--;
                }
            } else if (hm) {
                Vv = simd::sel(L() == (u32)__builtin_ctzll(hm), v, Vv);
            } else if (n < maxp) {
                K = simd::sel(L() == n, k, K);
                Vv = simd::sel(L() == n, v, Vv);
                n++;
            } else {
                fail(MTE_DOC_UNSUPPORTED, curSeq);
                return 0;
            }
        }
        const u32 id = mapNext++;
        u32* m = maps + (u64)id * mw;
        simd::st(m + 1, L() * 2u, K, L() < n);
        simd::st(m + 2, L() * 2u, Vv, L() < n);
        simd::st(m, L(), simd::splat(n), L() == 0u);
        adirty = true;  // read back later (match_props, build_map): fence_arena first
        return id;
    }
    SD void init() {
        if constexpr (PAGED) {
            rows.reset_rows();
        } else {
            rows.zero_slots(0, NBLK * 8);  // every slot empty: rows past the last block stay zero
        }
        LV.zero();
        HK.zero();
        HS.zero();
        n_lb = 1;
        height = 1;
        heapSize = segNext = arenaTop = arenaSel = 0;
        minSeq = curSeq = heapTop = 0;
        status = 0;
        midop = false;
        failSeq = -1;
        set_counts(0, 0);
        n_gc = 0;
        max_lb = 1;
        lb_lim = p.reg_lb_limit && p.reg_lb_limit < NBLK ? p.reg_lb_limit : NBLK;
        adirty = false;
#if defined(MTE_PROFILE) && !defined(MTE_CPU)
        for (u32 i = 0; i < RP_N; i++) pf[i] = 0;
#endif
        if constexpr (PAGED)
            if (!rows.grow_rows(1)) status = REG_HANDOFF;
    }

    SD static V L() { return simd::lanes(); }
    // a REG_HANDOFF raised INSIDE an op (a pool row or a map record it could not get) leaves the op
    // half applied: only a restart from op 0 may continue such a document
    bool midop = false;
    SD void fail(i32 code, i32 seq) {
        if (status == 0) {
            status = code;
            failSeq = seq;
            midop = code == REG_HANDOFF;
        }
    }
    // Segment ids are 1-based in the rows (an empty slot holds 0), the LDS engine's id + 1: the
    // heap's segment lookup compares ids alone. finish() and the handoff write id - 1.
    SD u32 new_sid() {
        if (segNext >= seg_cap) {
            fail(MTE_DOC_CAPACITY, curSeq);
            return NONE;
        }
        return ++segNext;
    }

    // ---------------------------------------------------------------- blocks
    SD static u32 gbase(u32 k) { return (k & 7u) * 8u; }
    SD static B in_group(u32 k) { return (L() >> 3) == (k & 7u); }
    SD static u32 group_bits(u64 m, u32 k) { return (u32)((m >> gbase(k)) & 0xFFull); }
    SD static u32 count_in(const Row& w, u32 k) { return (u32)__builtin_popcount(group_bits(simd::ballot(w.len != 0u), k)); }
    // Every lane of a block's group holds the block's needsScour, empty slots included: ns_put writes
    // the whole group, insert_slot gives the new slot its block's bits, split_block, scour's compaction
    // and pack_leaves keep or clear them group-wide. ns_in reads the first lane; op_remove's marking
    // loop reads the lanes it marks.
    SD static u32 ns_in(const Row& w, u32 k) { return (simd::readlane(w.meta, gbase(k)) >> NS_SHIFT) & 3u; }
    SD static void ns_put(Row& w, u32 k, u32 sc) { w.meta = simd::sel(in_group(k), (w.meta & ~NS_MASK) | (sc << NS_SHIFT), w.meta); }
    SD u32 count(u32 k) { return count_in(rows.row(k >> 3), k); }
    SD u32 ns_get(u32 k) { return ns_in(rows.row(k >> 3), k); }
    SD void ns_set(u32 k, u32 sc) {
        ns_put(rows.rowref(k >> 3), k, sc);
        rows.writeback(k >> 3);
    }

    // nodeLength of every slot of a row for (refSeq R, client C) (mergeTree.ts:1659-1699):
    //   ins = client == C || seq <= R;  rem = removed && (removedClient == C || removedSeq <= R
    //   || C in removedClientOverlap);  visible = ins && !rem ? len : 0.
    // (live: rseq RSEQ_LIVE and rm 0; removed: bit C of rm covers removedClient and the overlap set)
    SD static V vis(const Row& w, i32 R, u32 C) {
        const B ins = simd::sle(w.seq, R) | (simd::bfe(w.meta, 0, 8) == C);
        B rem;
        if constexpr (WIDE) rem = simd::sle(w.rseq, R) | (((C < 32 ? w.rm : w.rm2) & (1u << (C & 31u))) != 0u);
        else rem = simd::sle(w.rseq, R) | ((w.rm & (1u << C)) != 0u);
        return simd::sel(simd::andn(ins, rem), w.len, 0u);
    }

    // insertingWalk's target for `pos` in the (R, C) view: the first leaf block whose cumulative
    // visible end is >= pos, then inside it the first slot with pos < its end, or a zero-length slot
    // at pos that wins breakTie (skip tombstones already seen at R, mergeTree.ts:2257-2261).
    // The scan starts at row r0 with the visible length before it, carry0 (a previous resolve of
    // the same op found its block in r0: rows before it are unchanged by the splits since).
    SD RFound resolve(i32 pos, i32 R, u32 C, u32 r0 = 0, u32 carry0 = 0) {
        RG_PROF(RP_RESOLVE);
        RFound f;
        f.ok = false;
        f.k = 0;
        f.cnt = 0;
        f.slot = -1;
        f.r = 0;
        f.row = 0;
        f.carry = 0;
        const u32 nrows = (n_lb + 7) >> 3;
        RG_STAT(RS_RESOLVE, 1);
        RG_STAT(RS_RES_NROWS, nrows);
        u32 carry = carry0;
        // Block ends are the lanes 8g+7; blocks past n_lb are empty (rows past the last block stay
        // zero), so their ends never reach pos before a real block's end does.
        const B end = (L() & 7u) == 7u;
        // the hit row: the block and slot from the registers of the scan
        auto hit_row = [&](const Row& w, u32 r, u64 hit, const V& v, const V& incl) MTE_LI {
            const u32 g = (u32)__builtin_ctzll(hit) >> 3;
            const u32 k = r * 8 + g, gb = g * 8;
            const V rr = (u32)pos - (incl - v);
            const B valid = w.len != 0u;
            const B seen = simd::sle(w.rseq, R) & (w.rseq != 0u);
            const B cand = in_group(k) & valid & (simd::slt(rr, v) | ((rr == 0u) & (v == 0u) & ~seen));
            const u64 cm = simd::ballot(cand);
            f.ok = true;
            f.k = k;
            f.cnt = (u32)__builtin_popcount(group_bits(simd::ballot(valid), k));
            f.row = r;
            f.carry = carry;
            rows.cache(r, w);
            if (cm) {
                const u32 l = (u32)__builtin_ctzll(cm);
                f.slot = (i32)(l - gb);
                f.r = (i32)simd::readlane(rr, l);
            }
        };
        const u32 last = nrows - 1;
        // two row buffers, each refilled (unconditionally: the last row again at the end, so the
        // LDS counter wait stays exact) while the other one is scanned; the loop only finds the hit
        // row (no state written in it, so no per-row register copies)
        Row a = rows.row(r0), b;
        V v, incl;
        u64 hit = 0;
        bool inb = false;
        u32 r = r0;
        for (;;) {
            b = rows.ldrow(r + 1 < last ? r + 1 : last);
            RG_COUNT(RP_N_RESOLVE, 1);
            v = vis(a, R, C);
            RG_STAT(RS_RES_ROWS, 1);
            incl = simd::scan_incl(v) + carry;
            hit = simd::ballot(end & simd::sge(incl, pos));
            if (hit) break;
            carry = simd::readlane(incl, 63);
            if (++r >= nrows) break;
            a = rows.ldrow(r + 1 < last ? r + 1 : last);
            RG_COUNT(RP_N_RESOLVE, 1);
            v = vis(b, R, C);
            RG_STAT(RS_RES_ROWS, 1);
            incl = simd::scan_incl(v) + carry;
            hit = simd::ballot(end & simd::sge(incl, pos));
            if (hit) {
                inb = true;
                break;
            }
            carry = simd::readlane(incl, 63);
            if (++r >= nrows) break;
        }
        if (!hit) {
            RG_DUO(resolved(false, 0));
            return f;
        }
        RG_STAT(inb ? RS_HIT_SECOND : RS_HIT_FIRST, nrows >= 3);
        // (hit_row called on the buffer that hit, with no copy of b onto a, measured 2 % slower: the code of
        // hit_row twice, 34 instructions more per op)
        if (inb) a = b;
        hit_row(a, r, hit, v, incl);
        RG_DUO(resolved(true, f.row));
        return f;
    }

    // ---------------------------------------------------------------- interior levels
    // Parent (node index at level lv+1) of node c at level lv, and its first child.
    SD u32 parent_of(u32 lv, u32 c, u32& first) const {
        const V cnt = LV.get(lv);
        const V incl = simd::scan_incl(cnt);
        const u64 m = simd::ballot(incl > c);
        const u32 pi = m ? (u32)__builtin_ctzll(m) : 0u;
        first = simd::readlane(incl, pi) - simd::readlane(cnt, pi);
        return pi;
    }
    // A new node was placed right after node c at level lv (its parent gains a child): split
    // parents that reach 8 children 4+4, grow the root (insertingWalk / split / updateRoot,
    // mergeTree.ts:2446-2489, 1876-1887).
    SD void insert_after(u32 c, u32 lv) {
        for (u32 guard = 0; guard <= RG_LEVELS; guard++) {
            if (lv + 1 >= height) {  // c is the root: a new root [c, new]
                if (lv >= RG_LEVELS) break;
                LV.set(lv, simd::sel(L() == 0u, 2u, simd::splat(0)));
                height++;
                return;
            }
            u32 first;
            const u32 pi = parent_of(lv, c, first);
            V P = LV.get(lv);
            const u32 nc = simd::readlane(P, pi) + 1;
            if (nc < 8) {
                LV.set(lv, simd::writelane(P, pi, nc));
                return;
            }
            // split node pi: it keeps 4 children, a new node right after it takes 4
            P = simd::sel(L() > pi, simd::wave_shr1(P), P);
            P = simd::sel((L() == pi) | (L() == pi + 1), 4u, P);
            LV.set(lv, P);
            c = pi;
            lv++;
        }
        fail(MTE_DOC_CAPACITY, curSeq);
    }

    // ---------------------------------------------------------------- block edits
    // Blocks [from, n_lb) move to [from + d, n_lb + d); the 8*d slots this opens (d > 0) are left
    // for the caller, the ones it frees at the end (d < 0) are zeroed.
    SD void shift_blocks(u32 from, i32 d) {
        if (d == 0) return;
        RG_COUNT(RP_N_MOVE, n_lb - from);
        const u32 n = (n_lb - from) * 8;
        RG_STAT(RS_MOVE_SLOTS, n);
        if (d > 0) {
            rows.mv_slots((from + (u32)d) * 8, from * 8, n);
        } else {
            rows.mv_slots((from - (u32)(-d)) * 8, from * 8, n);
            rows.zero_slots((n_lb - (u32)(-d)) * 8, (u32)(-d) * 8);
        }
    }

    // Insert `rec` at slot j of block k (child count cnt); a block reaching 8 children splits 4+4,
    // the new block right after it in document order (needsScour undefined). With `upd`, slot j-1
    // first takes (len ul, cap uc) (the left piece of a split). Returns the block holding rec.
    // `lru`: the seq addToLRUSet is due with for rec (0: none). With kFoldLru, where the block does not
    // split, the needsScour mark goes into this row write and the heap push follows it (lruFolded: add_lru is
    // done); a splitting block leaves it to the caller's add_lru on the block rec ends up in.
    bool lruFolded = false;
    SD u32 insert_slot(u32 k, u32 cnt, u32 j, const RSeg& rec, bool upd, u32 ul, u32 uc, i32 lru = 0) {
        RG_PROF(RP_INSERT_SLOT);
        lruFolded = false;
        if (cnt >= 8 || j > cnt) {
            fail(MTE_DOC_CAPACITY, curSeq);
            return NONE;
        }
        const u32 r = k >> 3, gb = gbase(k);
        Row& w = rows.rowref(r);
        const V sl = L() & 7u;
        const B ing = in_group(k);
        const B mv = ing & (sl > j);
        const B at = L() == gb + j;
        u32 ns = (simd::readlane(w.meta, gb) >> NS_SHIFT) & 3u;
        bool push = false;
        if constexpr (kFoldLru) {
            if (lru && cnt + 1 < 8) {
                lruFolded = true;
                if (ns != SC_TRUE && lru > curSeq) {
                    push = true;
                    ns = SC_TRUE;
                    ns_put(w, k, SC_TRUE);
                }
            }
        }
        if (upd) {
            const B lf = L() == gb + j - 1;
            w.len = simd::sel(lf, ul, w.len);
            w.cap = simd::sel(lf, uc, w.cap);
        }
        auto put = [&](V& x, u32 val) MTE_LI {
            x = simd::sel(mv, simd::row_shr1(x), x);
            x = simd::sel(at, val, x);
        };
        put(w.len, rec.len);
        put(w.seq, (u32)rec.seq);
        put(w.rseq, rec.rseq);
        put(w.meta, (rec.meta & ~NS_MASK) | (ns << NS_SHIFT));
        put(w.toff, rec.toff);
        put(w.cap, rec.cap);
        put(w.rm, rec.rm);
        put(w.sid, rec.sid);
        if constexpr (PROPS) put(w.props, rec.props);
        if constexpr (WIDE) put(w.rm2, rec.rm2);
        rows.writeback(r);
        if (push) {
            RG_STAT(RS_LRU_FOLDED, 1);
            heap_push(rec.sid, lru);
        }
        if (cnt + 1 < 8) return k;
        split_block(k);
        return j < 4 ? k : k + 1;
    }
    // Block k holds 8 children: a new block k+1 takes slots 4..7 (mergeTree.ts:2476-2489).
    SD void split_block(u32 k) {
        RG_PROF(RP_SPLIT);
        RG_COUNT(RP_N_SPLIT_BLK, 1);
        RG_STAT(RS_SPLIT_BLK, 1);
        if (!ensure_blocks(n_lb + 1)) return;
        shift_blocks(k + 1, 1);
        const u32 r = k >> 3, r2 = (k + 1) >> 3;
        RG_STAT(RS_SPLIT_NEXT_ROW, r2 != r);
        const V sl = L() & 7u;
        const B lo = in_group(k + 1) & (sl < 4u), hi2 = in_group(k + 1) & (sl >= 4u), hi = in_group(k) & (sl >= 4u);
        const V src = (L() + (r2 == r ? 0u : 64u) - 4u) & 63u;  // new slot s <- old slot 4+s of block k
        Row w = rows.row(r);
        const u32 nsk = simd::readlane(w.meta, gbase(k)) & NS_MASK;
        Row w2 = r2 == r ? w : rows.ldrow(r2);
        auto mv = [&](V& x, V& y, u32 keepHi) MTE_LI {  // x: row r, y: row r2
            const V moved = simd::bperm(x, src);
            if (r2 == r) {
                x = simd::sel(lo, moved, x);
                x = simd::sel(hi2, 0u, x);
                x = simd::sel(hi, keepHi, x);
            } else {
                y = simd::sel(lo, moved, simd::sel(hi2, 0u, y));
                x = simd::sel(hi, keepHi, x);
            }
        };
        mv(w.len, w2.len, 0u);
        mv(w.seq, w2.seq, 0u);
        mv(w.rseq, w2.rseq, 0u);
        mv(w.meta, w2.meta, nsk);  // block k keeps its needsScour in every lane
        mv(w.toff, w2.toff, 0u);
        mv(w.cap, w2.cap, 0u);
        mv(w.rm, w2.rm, 0u);
        mv(w.sid, w2.sid, 0u);
        if constexpr (PROPS) mv(w.props, w2.props, 0u);
        if constexpr (WIDE) mv(w.rm2, w2.rm2, 0u);
        // the new block's needsScour is undefined
        if (r2 == r) {
            w.meta = simd::sel(in_group(k + 1), w.meta & ~NS_MASK, w.meta);
            rows.putrow(r, w);
        } else {
            w2.meta = simd::sel(in_group(k + 1), w2.meta & ~NS_MASK, w2.meta);
            rows.strow(r2, w2);
            rows.putrow(r, w);
        }
        n_lb++;
        if (n_lb > max_lb) max_lb = n_lb;
        insert_after(k, 0);
    }

    // ---------------------------------------------------------------- LRU heap (collections.ts:213-265)
    // Position q lives in register q >> 6, lane q & 63. A walk unrolled by heap level names its
    // registers statically (level d <= 5: register 0; 6: 1; 7: 2..3; 8: 4..7): a VA indexed by a
    // run-time register number compiles to a v_cndmask chain over all eight registers per access.
    template <int D>
    SD static u32 hrd(const HeapRegs& A, u32 q) {
        const u32 l = q & 63u;
        if constexpr (D <= 5) {
            return simd::readlane(A.get(0), l);
        } else if constexpr (D == 6) {
            return simd::readlane(A.get(1), l);
        } else if constexpr (D == 7) {
            const u32 a = simd::readlane(A.get(2), l), b = simd::readlane(A.get(3), l);
            return (q >> 6) & 1u ? b : a;
        } else {
            const u32 a = simd::readlane(A.get(4), l), b = simd::readlane(A.get(5), l);
            const u32 c = simd::readlane(A.get(6), l), d = simd::readlane(A.get(7), l);
            const u32 r = (q >> 6) & 3u;
            return r == 0 ? a : r == 1 ? b : r == 2 ? c : d;
        }
    }
    template <int D>
    SD static void hwr(HeapRegs& A, u32 q, u32 v) {
        [[maybe_unused]] const u32 l = q & 63u;  // (the lane compares below take q itself)
        if constexpr (kHeapInPlace && D >= 7) {
            // no branch picks the register: each is rewritten where it lives, by a lane compare that holds in
            // the one register of position q (q - 64 * i names no lane elsewhere: it wraps or is >= 64)
            if constexpr (D == 7) {
                A.x2 = simd::sel(L() == q - 128u, v, A.x2);
                A.x3 = simd::sel(L() == q - 192u, v, A.x3);
            } else {
                A.x4 = simd::sel(L() == q - 256u, v, A.x4);
                A.x5 = simd::sel(L() == q - 320u, v, A.x5);
                A.x6 = simd::sel(L() == q - 384u, v, A.x6);
                A.x7 = simd::sel(L() == q - 448u, v, A.x7);
            }
        } else if constexpr (D <= 5) {
            A.set(0, simd::writelane(A.get(0), l, v));
        } else if constexpr (D == 6) {
            A.set(1, simd::writelane(A.get(1), l, v));
        } else if constexpr (D == 7) {
            if ((q >> 6) & 1u) A.set(3, simd::writelane(A.get(3), l, v));
            else A.set(2, simd::writelane(A.get(2), l, v));
        } else {
            switch ((q >> 6) & 3u) {
                case 0: A.set(4, simd::writelane(A.get(4), l, v)); break;
                case 1: A.set(5, simd::writelane(A.get(5), l, v)); break;
                case 2: A.set(6, simd::writelane(A.get(6), l, v)); break;
                default: A.set(7, simd::writelane(A.get(7), l, v)); break;
            }
        }
    }
    SD static u32 hlevel(u32 q) { return 31u - (u32)__builtin_clz(q); }
    SD u32 hkey(u32 q) const {  // any position (run-time level)
        const u32 d = hlevel(q);
        return d <= 5 ? hrd<0>(HK, q) : d == 6 ? hrd<6>(HK, q) : d == 7 ? hrd<7>(HK, q) : hrd<8>(HK, q);
    }
    SD u32 hsid(u32 q) const {
        const u32 d = hlevel(q);
        return d <= 5 ? hrd<0>(HS, q) : d == 6 ? hrd<6>(HS, q) : d == 7 ? hrd<7>(HS, q) : hrd<8>(HS, q);
    }
    SD void hset(u32 q, u32 sid, u32 key) {
        if constexpr (kHeapInPlace) {
            // registers 0 and 1 by a lane compare, both every time: no branch picks the register, so the
            // sixteen heap registers have one home across a push (q >= 128: q - 64 names no lane; q < 64
            // neither: it wraps)
            const B a0 = L() == q, a1 = L() == q - 64u;
            HK.r0 = simd::sel(a0, key, HK.r0);
            HS.r0 = simd::sel(a0, sid, HS.r0);
            HK.r1 = simd::sel(a1, key, HK.r1);
            HS.r1 = simd::sel(a1, sid, HS.r1);
            RG_STAT(RS_HEAP_REG1, q >= 64u && q < 128u);
            if (q >= 128u) {  // one plain branch, its body straight-line
                RG_STAT(RS_HEAP_REG2, 1);
                hwr<7>(HK, q, key);
                hwr<7>(HS, q, sid);
                hwr<8>(HK, q, key);
                hwr<8>(HS, q, sid);
            }
            return;
        }
        RG_STAT(RS_HEAP_REG1, q >= 64u && q < 128u);
        RG_STAT(RS_HEAP_REG2, q >= 128u);
        const u32 d = hlevel(q);
        if (d <= 5) {
            hwr<0>(HK, q, key);
            hwr<0>(HS, q, sid);
        } else if (d == 6) {
            hwr<6>(HK, q, key);
            hwr<6>(HS, q, sid);
        } else if (d == 7) {
            hwr<7>(HK, q, key);
            hwr<7>(HS, q, sid);
        } else {
            hwr<8>(HK, q, key);
            hwr<8>(HS, q, sid);
        }
    }
    // push: keys are op seqs, strictly increasing across messages, so the sift-up never moves an
    // entry (collections.ts:241-250 moves strictly larger parents only): an append
    SD void heap_push(u32 sid, i32 key) {
        if (heapSize + 1 >= RG_HEAP) {
            fail(MTE_DOC_CAPACITY, curSeq);
            return;
        }
        const u32 n = ++heapSize;
        RG_STAT(RS_LRU_PUSH, 1);
        if (n == 1) heapTop = key;
        hset(n, sid, (u32)key);
    }
    // pop: sift-down of collections.ts:252-264 (smaller child, left on ties, moves up while
    // strictly below the moved last entry (lk, ls)); node k sits at level D, m entries remain
    template <int D>
    SD void sift(u32 k, u32 m, u32 lk, u32 ls, i32& newTop) {
        if constexpr (D < 8) {
            u32 j = k << 1;
            if (j <= m) {
                u32 kj = hrd<D + 1>(HK, j);
                if (j < m) {
                    const u32 kj1 = hrd<D + 1>(HK, j + 1);
                    if ((i32)kj - (i32)kj1 > 0) {
                        j++;
                        kj = kj1;
                    }
                }
                if ((i32)lk - (i32)kj > 0) {
                    if (D == 0) newTop = (i32)kj;
                    hwr<D>(HK, k, kj);
                    hwr<D>(HS, k, hrd<D + 1>(HS, j));
                    sift<D + 1>(j, m, lk, ls, newTop);
                    return;
                }
            }
        }
        hwr<D>(HK, k, lk);
        hwr<D>(HS, k, ls);
    }
    // The same sift-down, lane-parallel while the heap fits positions 1..127 (registers 0 and 1):
    // every node k of register 0 (lane k) picks its child c(k) and whether the moved entry goes
    // below it (lk > K[c(k)]) at once; the path from the root then follows two ballots of those
    // decisions, and every node on it above the stop node takes its child's entry in one select.
    SD void pop_fast(u32 m, u32 lk, u32 ls, i32& newTop) {
        const V K0 = HK.get(0), K1 = HK.get(1), S0 = HS.get(0), S1 = HS.get(1);
        const V cl = L() * 2u, cr = cl + 1u;
        // both children's keys AND segment ids in one round of crossbar gathers (register 1 only
        // when the heap reaches it)
        V kL, kR, sL, sR;
        if (m < 64u) {
            kL = simd::bperm(K0, cl & 63u);
            kR = simd::bperm(K0, cr & 63u);
            sL = simd::bperm(S0, cl & 63u);
            sR = simd::bperm(S0, cr & 63u);
        } else {
            const B l0 = cl < 64u, r0 = cr < 64u;
            kL = simd::sel(l0, simd::bperm(K0, cl & 63u), simd::bperm(K1, cl & 63u));
            kR = simd::sel(r0, simd::bperm(K0, cr & 63u), simd::bperm(K1, cr & 63u));
            sL = simd::sel(l0, simd::bperm(S0, cl & 63u), simd::bperm(S1, cl & 63u));
            sR = simd::sel(r0, simd::bperm(S0, cr & 63u), simd::bperm(S1, cr & 63u));
        }
        const B right = (cr < m + 1u) & simd::slt(kR, kL);  // smaller child, the left one on ties
        const V c = simd::sel(right, cr, cl);
        const V kc = simd::sel(right, kR, kL);
        const V sc = simd::sel(right, sR, sL);
        const B go = (cl < m + 1u) & simd::slt(kc, (i32)lk);  // the moved entry goes below k
        u32 k = 1;
        u64 path = 0;  // nodes of register 0 that take their child's entry
        // G bit k: node k takes its chosen child's entry (the moved entry goes below k); Rt bit k:
        // that child is the right one. The path from the root follows them (one crossbar round trip
        // fewer than gathering each child's parent decision); nodes 32..63 continue into register 1.
        const u64 G = simd::ballot(go), Rt = simd::ballot(right);
        // Every lane decides for itself whether the walk reaches it, in straight-line code: E bit l
        // says node l is its parent's chosen child and the parent lets the entry pass (the root and
        // lane 0's bit are set), and the walk reaches l iff E holds for l and for each of its at most
        // five ancestors l >> j (all below 32; a shift that runs out reads bit 0 or 1, both set).
        const V Lv = L();
        const V pa = Lv >> 1u;
        const V ec = (simd::splat((u32)G) >> pa) & (((simd::splat((u32)Rt) >> pa) ^ Lv) ^ 0xFFFFFFFFu);
        const B e = ((ec & 1u) != 0u) | (Lv < 2u);
        const V Es = simd::splat((u32)simd::ballot(e) | 3u);
        const V anc = (Es >> pa) & (Es >> (Lv >> 2u)) & (Es >> (Lv >> 3u)) & (Es >> (Lv >> 4u)) & (Es >> (Lv >> 5u));
        const u64 reach = simd::ballot(e & ((anc & 1u) != 0u)) & ~1ull;
        path = reach & G;
        const u64 stop = reach & ~G;  // the node the walk ends at, when it ends in register 0
        if (stop) {
            k = (u32)__builtin_ctzll(stop);
        } else {  // through a node of the last level of register 0 into register 1
            const u32 n5 = 63u - (u32)__builtin_clzll(path);
            k = 2 * n5 + (u32)((Rt >> n5) & 1u);
        }
        const B mv = simd::ballot_mask(path);
        V N0 = simd::sel(mv, kc, K0), T0 = simd::sel(mv, sc, S0);
        if (path & 2u) newTop = (i32)simd::readlane(kc, 1);
        if constexpr (kHeapInPlace) {  // (as hset: k < 128 here)
            const B a0 = L() == k, a1 = L() == k - 64u;
            HK.r0 = simd::sel(a0, lk, N0);
            HS.r0 = simd::sel(a0, ls, T0);
            HK.r1 = simd::sel(a1, lk, K1);
            HS.r1 = simd::sel(a1, ls, S1);
            return;
        }
        if (k < 64u) {
            N0 = simd::writelane(N0, k, lk);
            T0 = simd::writelane(T0, k, ls);
        } else {
            HK.set(1, simd::writelane(K1, k & 63u, lk));
            HS.set(1, simd::writelane(S1, k & 63u, ls));
        }
        HK.set(0, N0);
        HS.set(0, T0);
    }
    SD u32 heap_pop() {
        RG_PROF(RP_HEAP);
        const u32 top = hrd<0>(HS, 1);
        heap_pop_rest();
        return top;
    }
    // everything of a pop but reading the root's segment id
    SD void heap_pop_rest() {
        RG_COUNT(RP_N_POP, 1);
        const u32 n = heapSize, m = n - 1;
        RG_STAT(RS_POP, 1);
        RG_DUO(popped = true);
        RG_STAT(RS_POP_BIG, m >= 128u);
        RG_STAT(RS_POP_HEAP, n);
#if defined(MTE_CPU) && defined(MTE_CPU_STATS)
        if (n > g_rg_stats[RS_N]) g_rg_stats[RS_N] = n;  // the largest heap at a pop
        if (n_lb > g_rg_stats[RS_N + 1]) g_rg_stats[RS_N + 1] = n_lb;
#endif
        const u32 lk = hkey(n), ls = hsid(n);
        i32 newTop = (i32)lk;
        if (m >= 1) {
            if (m < 128u) pop_fast(m, lk, ls, newTop);
            else {
                RG_STAT(RS_SIFT_SERIAL, 1);
                sift<0>(1, m, lk, ls, newTop);
            }
        }
        heapTop = newTop;
        heapSize = m;
    }
    // zamboni's pop: the popped segment's leaf block (find_seg) with it. The segment id is the heap's
    // root, known before the sift, and the search reads nothing the sift writes: the first eight
    // rows' ids are read first and arrive while the sift runs -- one LDS round trip of latency per pop
    // where heap_pop() + find_seg() wait for two. (LDS returns in order: the counter waits of the
    // sift's crossbar gathers cover these reads.)
    SD u32 heap_pop_find() {
        const u32 sid = hrd<0>(HS, 1);
        const u32 nrows = (n_lb + 7) >> 3;
        V s8[8];
        for (u32 i = 0; i < 8; i++) s8[i] = ld_sid(i < nrows ? i : 0u);
        simd::issue_here();
        {
            RG_PROF(RP_HEAP);
            heap_pop_rest();
        }
        RG_PROF(RP_FIND_SEG);
        RG_STAT(RS_FIND_ROWS, nrows);
        V hr = simd::splat(NONE);
        for (u32 i = 8; i-- > 0;) hr = simd::sel(s8[i] == sid, i, hr);  // rows past nrows re-read row 0: i = 0 wins
        const u64 m = simd::ballot(hr != NONE);
        if (m) {
            const u32 l = (u32)__builtin_ctzll(m);
            return simd::readlane(hr, l) * 8 + (l >> 3);
        }
        return nrows > 8 ? find_seg(sid, 8) : NONE;
    }
    // addToLRUSet (mergeTree.ts:1273-1283) for a segment of block k
    SD void add_lru(u32 k, u32 sid, i32 seq) {
        RG_PROF(RP_LRU);
        if (ns_get(k) != SC_TRUE && seq > curSeq) {
            RG_STAT(RS_LRU_REWRITE, 1);
            ns_set(k, SC_TRUE);
            heap_push(sid, seq);
        }
    }
    // the leaf block holding segment sid (segment.parent), NONE when unlinked. Segment ids are
    // unique, so each batch of eight rows needs one per-lane select per row and ONE ballot (no
    // branch per row): the hit lane's row index comes back with one readlane.
    SD u32 find_seg(u32 sid, u32 from = 0) {  // from: the first row to look at (a multiple of 8)
        RG_PROF(RP_FIND_SEG);
        const u32 nrows = (n_lb + 7) >> 3;
        if (!from) RG_STAT(RS_FIND_ROWS, nrows);
        for (u32 r0 = from; r0 < nrows; r0 += 8) {  // eight rows' reads in flight per round
            V s8[8];
            for (u32 i = 0; i < 8; i++) s8[i] = ld_sid(r0 + i < nrows ? r0 + i : r0);
            V hr = simd::splat(NONE);
            for (u32 i = 8; i-- > 0;) hr = simd::sel(s8[i] == sid, r0 + i, hr);  // rows past nrows re-read r0: i = 0 wins
            const u64 m = simd::ballot(hr != NONE);
            if (m) {
                const u32 l = (u32)__builtin_ctzll(m);
                return simd::readlane(hr, l) * 8 + (l >> 3);
            }
        }
        return NONE;
    }

    // ---------------------------------------------------------------- text (HBM)
    SD u16* arena_cur() const { return arena0 + (u64)arenaSel * arena_cap; }
    SD void fence_arena() {
        if (adirty) {
            simd::wave_fence();
            adirty = false;
        }
    }
    // copy n units from text offset src (payload or arena) to offset dst of dbase (lanes in parallel)
    SD void copy_text(u32 dst, u32 src, u32 n, u16* dbase) {
        const u16* sb = (src & ARENA_BIT) ? arena_cur() : payload;
        const u32 so = src & ~ARENA_BIT, d0 = dst & ~ARENA_BIT;
        for (u32 b = 0; b < n; b += 64) {
            const V i = L() + b;
            const B m = i < n;
            const V t = simd::ld(sb, i + so, m);
            simd::st(dbase, i + d0, t, m);
        }
    }
    // Semispace compaction of the merge arena: every live arena-resident text, document order.
    SD void arena_gc() {
        fence_arena();
        const u32 other = arenaSel ^ 1u;
        u16* dst = arena0 + (u64)other * arena_cap;
        u32 top = 0;
        for (u32 k = 0; k < n_lb; k++) {
            const u32 r = k >> 3, gb = gbase(k);
            Row w = rows.ldrow(r);
            const u32 cnt = (u32)__builtin_popcount(group_bits(simd::ballot(w.len != 0u), k));
            bool dirty = false;
            for (u32 s = 0; s < cnt; s++) {
                const u32 l = gb + s;
                const u32 meta = simd::readlane(w.meta, l), toff = simd::readlane(w.toff, l);
                if ((meta & F_MARKER) || !(toff & ARENA_BIT)) continue;
                const u32 len = simd::readlane(w.len, l), oc = simd::readlane(w.cap, l);
                const bool rm = simd::readlane(w.rseq, l) != RSEQ_LIVE;
                const u32 cap = (rm || oc < len) ? len : oc;
                if ((toff & ~ARENA_BIT) + len > arena_cap || top + cap > arena_cap) {
                    fail(MTE_DOC_CAPACITY, curSeq);
                    return;
                }
                copy_text(top, toff, len, dst);
                w.toff = simd::writelane(w.toff, l, top | ARENA_BIT);
                w.cap = simd::writelane(w.cap, l, cap);
                dirty = true;
                top += cap;
            }
            if (dirty) rows.putrow(r, w);
        }
        simd::wave_fence();
        arenaSel = other;
        arenaTop = top;
        n_gc++;
    }

    // ---------------------------------------------------------------- zamboni (mergeTree.ts:1289-1478)
    // scourNode on block k (cnt children): tombstones at or below the MSN are dropped and reset the
    // merge chain, settled live text appends to the chain head under TextSegment.canAppend
    // (textSegment.ts:63-85; no '\n' in these documents, no properties); kept slots are compacted.
    // Returns the new child count.
    //
    // Lane-parallel form: in the lean documents this engine replays (no properties, no '\n'), a
    // settled slot joins the run of the settled slot before it exactly when both are text (a removed
    // or unsettled slot resets the chain; a marker head or marker slot starts a new one), unless
    // TextSegment.canAppend's granularity test fails, which needs the run's accumulated length: a
    // block where a joining slot is longer than GRANULARITY takes the serial walk (scour_serial).
    // Each run becomes its head with the run's text: already contiguous (no copy), appended into the
    // head's arena chunk when it has the capacity, or else copied into a fresh chunk of
    // max(32, 2 * total) units; all copies of the block run as one flattened gather.
    bool scoured = false;  // the last scour rewrote its block's row, needsScour already false
    SD u32 scour(u32 k, u32 cnt) {
        RG_PROF(RP_SCOUR);
        scoured = false;
        RG_COUNT(RP_N_SCOUR, 1);
        if (cnt > 8) cnt = 8;
        const u32 r = k >> 3, gb = gbase(k);
        const B ing = in_group(k);
        Row w = rows.row(r);
        const B act = ing & (w.len != 0u);
        const B rem = act & (w.rseq != RSEQ_LIVE);
        const u32 mDROP = group_bits(simd::ballot(rem & simd::sle(w.rseq, minSeq)), k);
        const u32 mSET = group_bits(simd::ballot(simd::andn(act, rem) & simd::sle(w.seq, minSeq)), k);
        const u32 mTXT = group_bits(simd::ballot(act & ((w.meta & F_MARKER) == 0u)), k);
        const u32 mST = mSET & mTXT;
        u32 mJOIN = mST & (mST << 1) & 0xFFu;  // slot s joins the run of slot s-1
        if constexpr (PROPS) {  // ... when its properties match slot s-1's (matchProperties)
            const u32 mSAME = group_bits(simd::ballot(w.props == simd::row_shr1(w.props)), k);
            for (u32 c = mJOIN & ~mSAME; c; c &= c - 1) {
                const u32 sb = (u32)__builtin_ctz(c);
                if (!match_props(simd::readlane(w.props, gb + sb - 1), simd::readlane(w.props, gb + sb))) mJOIN &= ~(1u << sb);
            }
        }
        RG_STAT(RS_SCOUR, 1);
        if (!mDROP && !mJOIN) {  // nothing dropped, nothing merged
            RG_STAT(RS_SCOUR_NOP, 1);
            return cnt;
        }
        if (mJOIN & group_bits(simd::ballot(w.len > (u32)GRANULARITY), k)) {
            RG_STAT(RS_SCOUR_SERIAL, 1);
            return scour_serial(k, cnt);
        }
        RG_COUNT(RP_N_SCOUR_CHANGED, 1);
        fence_arena();
        const V sl = L() & 7u;
        V jdst = simd::splat(0), jlen = jdst, jsrc = jdst;  // per slot lane: jlen units from jsrc to jdst
        for (u32 attempt = 0; attempt < 2; attempt++) {
            // offsets inside a run: exclusive prefix sum of the block's lengths
            const V gl = simd::sel(ing, w.len, 0u);
            const V ex = simd::scan_incl(gl) - gl;
            const B cont = w.toff == simd::row_shr1(w.toff + w.len);  // text starts where slot s-1's ends
            const u32 mCONT = group_bits(simd::ballot(cont), k);
            jdst = jlen = simd::splat(0);
            u32 top = arenaTop, need = 0;
            Row nw = w;
            for (u32 heads = mST & ~mJOIN & (mJOIN >> 1); heads; heads &= heads - 1) {
                const u32 h = (u32)__builtin_ctz(heads);
                const u32 run = (u32)__builtin_ctz(~(mJOIN >> (h + 1)));  // joining slots after h
                const u32 e = h + run, rb = ((2u << e) - 1u) & ~((2u << h) - 1u);  // bits h+1..e
                const u32 lh = gb + h, le = gb + e;
                const u32 off = simd::readlane(w.toff, lh), cap = simd::readlane(w.cap, lh);
                const u32 exh = simd::readlane(ex, lh);
                const u32 total = simd::readlane(ex, le) + simd::readlane(w.len, le) - exh;
                u32 noff = off, ncap = cap, cbits = 0;
                if ((mCONT & rb) == rb) {  // the run's text is one contiguous range already
                    if (off & ARENA_BIT) ncap = simd::readlane(w.toff, le) + simd::readlane(w.cap, le) - off;
                } else if ((off & ARENA_BIT) && total <= cap) {  // append into the head's chunk
                    cbits = rb;
                } else {  // a fresh chunk
                    ncap = 2 * total < 32 ? 32u : 2 * total;
                    noff = top | ARENA_BIT;
                    top += ncap;
                    need += ncap;
                    cbits = rb | (1u << h);
                }
                if (cbits) {
                    const B cp = ing & (((simd::splat(cbits) >> sl) & 1u) != 0u);
                    jdst = simd::sel(cp, ex + (noff - exh), jdst);
                    jlen = simd::sel(cp, w.len, jlen);
                }
                nw.len = simd::writelane(nw.len, lh, total);
                nw.toff = simd::writelane(nw.toff, lh, noff);
                nw.cap = simd::writelane(nw.cap, lh, ncap);
            }
            if (arenaTop + need <= arena_cap) {
                arenaTop = top;
                jsrc = w.toff;  // the slots' text before the runs' heads move
                w = nw;
                break;
            }
            if (attempt == 1) {
                fail(MTE_DOC_CAPACITY, curSeq);
                return cnt;
            }
            arena_gc();  // moves every arena text: re-read the slots and redo the runs
            if (status) return cnt;
            w = rows.row(r);
            fence_arena();
        }
        copy_runs(jdst, jsrc, jlen);
        // compaction: kept slots (not dropped, not joined) in order at the front of the group, the
        // rest behind them; a push permutation (ds_permute) inside the group
        const u32 mKEEP = group_bits(simd::ballot(act), k) & ~mDROP & ~mJOIN;
        const u32 nkeep = (u32)__builtin_popcount(mKEEP);
        const V below = (simd::shl(simd::splat(1), sl) - 1u);
        const B kp = ((simd::splat(mKEEP) >> sl) & 1u) != 0u;
        const V dst = simd::sel(ing, simd::sel(kp, simd::bcnt(simd::splat(mKEEP) & below),
                                               simd::bcnt(simd::splat(~mKEEP & 0xFFu) & below) + nkeep) + gb,
                                L());
        const B tail = ing & (sl >= nkeep);
        auto cmp = [&](V& x, u32 keepEmpty) MTE_LI {
            const V nv = simd::push(x, dst);
            x = simd::sel(tail, nv & keepEmpty, nv);
        };
        cmp(w.len, 0u);
        cmp(w.seq, 0u);
        cmp(w.rseq, 0u);
        cmp(w.meta, NS_MASK);  // the block's needsScour stays in every lane
        cmp(w.cap, 0u);
        cmp(w.toff, 0u);
        cmp(w.rm, 0u);
        cmp(w.sid, 0u);
        if constexpr (PROPS) cmp(w.props, 0u);
        if constexpr (WIDE) cmp(w.rm2, 0u);
        ns_put(w, k, SC_FALSE);  // scourNode's caller clears needsScour (mergeTree.ts:1457): same write
        RG_DUO(w |= 1ull << r);
        rows.putrow(r, w);
        scoured = true;
        return nkeep;
    }
    // The runs' text copies of one block as one flattened gather: slot lane l copies jlen units from
    // its text src to jdst (sources are never destinations of the same scour).
    SD void copy_runs(V jdst, V jsrc, V jlen) {
        const V jinc = simd::scan_incl(jlen);
        const u32 total = simd::readlane(jinc, 63);
        if (!total) return;
        RG_STAT(RS_SCOUR_COPY, 1);
        const V jstart = jinc - jlen;
        u64 jm = simd::ballot(jlen != 0u);
        u16* ar = arena_cur();
        for (u32 base = 0; base < total; base += 64) {
            const V f = L() + base;
            V j = simd::splat(0);
            for (u64 m = jm; m; m &= m - 1) {
                const u32 q = (u32)__builtin_ctzll(m);
                j = simd::sel(f >= simd::readlane(jstart, q), q, j);
            }
            const V s0 = simd::bperm(jstart, j), d = simd::bperm(jdst, j), sr = simd::bperm(jsrc, j);
            const B m = f < total;
            const V o = f - s0;
            const B fa = (sr & ARENA_BIT) != 0u;
            const V so = (sr & ~ARENA_BIT) + o;
            const V t = simd::sel(fa, simd::ld(ar, so, m & fa), simd::ld(payload, so, simd::andn(m, fa)));
            simd::st(ar, (d & ~ARENA_BIT) + o, t, m);
        }
        adirty = true;
    }
    // The serial walk of scourNode (any lengths): the granularity test needs the run's accumulated
    // length.
    SD u32 scour_serial(u32 k, u32 cnt) {
        fence_arena();
        const u32 r = k >> 3, gb = gbase(k);
        const B ing = in_group(k);
        Row w = rows.row(r);
        const B act = ing & (w.len != 0u);
        const B rem = act & (w.rseq != RSEQ_LIVE);
        const u32 mREM = group_bits(simd::ballot(rem), k);
        const u32 mKEPT = group_bits(simd::ballot(rem & simd::sgt(w.rseq, minSeq)), k);
        const u32 mSET = group_bits(simd::ballot(simd::andn(act, rem) & simd::sle(w.seq, minSeq)), k);
        if (!(mREM & ~mKEPT) && !(mSET & (mSET << 1))) return cnt;  // nothing dropped, nothing to merge
        const u32 mTXT = group_bits(simd::ballot(act & ((w.meta & F_MARKER) == 0u)), k);
        u32 nkeep = 0, jn = 0;
        V kSrc = simd::splat(0), kLen = kSrc, kOff = kSrc, kCap = kSrc;  // lane i: kept slot i
        V jdst = kSrc, jsrc = kSrc, jlen = kSrc;                          // lane j: copy job j
        for (u32 attempt = 0; attempt < 2; attempt++) {
            nkeep = jn = 0;
            jdst = jsrc = jlen = simd::splat(0);
            u32 top = arenaTop, need = 0;
            i32 prev = -1;
            u32 pLen = 0, pOff = 0, pCap = 0, pMat = 0, pProps = 0;
            bool pText = false, pFresh = false;
            auto job = [&](u32 d, u32 s, u32 n) MTE_LI {
                if (jn < 64) {
                    jdst = simd::writelane(jdst, jn, d);
                    jsrc = simd::writelane(jsrc, jn, s);
                    jlen = simd::writelane(jlen, jn, n);
                }
                jn++;
            };
            for (u32 s = 0; s < cnt; s++) {
                const u32 bit = 1u << s;
                bool keep = true;
                if (mREM & bit) {
                    keep = (mKEPT & bit) != 0;
                    prev = -1;
                } else if (mSET & bit) {
                    const u32 ln = simd::readlane(w.len, gb + s), to = simd::readlane(w.toff, gb + s);
                    const u32 tc = simd::readlane(w.cap, gb + s);
                    u32 sp = 0;
                    if constexpr (PROPS) sp = simd::readlane(w.props, gb + s);
                    const bool ok = prev >= 0 && pText && (mTXT & bit) && (pLen <= (u32)GRANULARITY || ln <= (u32)GRANULARITY) &&
                                    (!PROPS || match_props(pProps, sp));
                    if (ok) {  // TextSegment.append
                        if ((pOff & ARENA_BIT) && pLen + ln <= pCap) {
                            job(pOff + pLen, to, ln);
                        } else if (pOff + pLen == to && pMat == pLen) {  // text already contiguous
                            if (pOff & ARENA_BIT) pCap = to + tc - pOff;
                            pMat += ln;
                        } else {
                            u32 ncap = 2 * (pLen + ln);
                            if (ncap < 32) ncap = 32;
                            const u32 dst = top | ARENA_BIT;
                            top += ncap;
                            need += ncap;
                            // pending jobs into the head's chunk follow it to the new one; the
                            // materialised prefix (none for a chunk built by this batch) is copied
                            const u32 m0 = pFresh ? 0u : pMat;
                            const B mvj = (L() < jn) & (jdst >= pOff + m0) & (jdst < pOff + pLen);
                            jdst = simd::sel(mvj, jdst - pOff + dst, jdst);
                            if (m0) job(dst, pOff, m0);
                            job(dst + pLen, to, ln);
                            pOff = dst;
                            pCap = ncap;
                            pFresh = true;
                        }
                        pLen += ln;
                        kLen = simd::writelane(kLen, (u32)prev, pLen);
                        kOff = simd::writelane(kOff, (u32)prev, pOff);
                        kCap = simd::writelane(kCap, (u32)prev, pCap);
                        keep = false;
                    } else {
                        prev = (i32)nkeep;
                        pLen = ln;
                        pMat = ln;
                        pOff = to;
                        pCap = tc;
                        pText = (mTXT & bit) != 0;
                        pFresh = false;
                        pProps = sp;
                    }
                } else {
                    prev = -1;
                }
                if (keep) {
                    kSrc = simd::writelane(kSrc, nkeep, s);
                    kLen = simd::writelane(kLen, nkeep, simd::readlane(w.len, gb + s));
                    kOff = simd::writelane(kOff, nkeep, simd::readlane(w.toff, gb + s));
                    kCap = simd::writelane(kCap, nkeep, simd::readlane(w.cap, gb + s));
                    nkeep++;
                }
            }
            if (nkeep == cnt) return cnt;
            if (arenaTop + need <= arena_cap && jn <= 64) {
                arenaTop = top;
                break;
            }
            if (attempt == 1) {
                fail(MTE_DOC_CAPACITY, curSeq);
                return cnt;
            }
            arena_gc();  // moves every arena text: re-read the slots and redo the chain
            if (status) return cnt;
            w = rows.row(r);
        }
        if (jn) run_jobs(jn, jdst, jsrc, jlen);
        // compaction: group lane gb+i takes kept slot i
        const V sl = L() & 7u;
        const B kp = ing & (sl < nkeep);
        const V src = simd::bperm(kSrc, sl) + gb;
        auto cmp = [&](V& x, const V* over, u32 keepEmpty) MTE_LI {  // empty lanes keep only `keepEmpty` bits
            const V nv = over ? simd::bperm(*over, sl) : simd::bperm(x, src);
            x = simd::sel(kp, nv, simd::sel(ing, x & keepEmpty, x));
        };
        cmp(w.len, &kLen, 0u);
        cmp(w.toff, &kOff, 0u);
        cmp(w.cap, &kCap, 0u);
        cmp(w.rm, nullptr, 0u);
        cmp(w.seq, nullptr, 0u);
        cmp(w.rseq, nullptr, 0u);
        cmp(w.meta, nullptr, NS_MASK);  // the block's needsScour stays in every lane
        cmp(w.sid, nullptr, 0u);
        if constexpr (PROPS) cmp(w.props, nullptr, 0u);
        if constexpr (WIDE) cmp(w.rm2, nullptr, 0u);
        ns_put(w, k, SC_FALSE);
        RG_DUO(w |= 1ull << r);
        rows.putrow(r, w);
        scoured = true;
        return nkeep;
    }
    // The recorded copies as one flattened gather (sources are never destinations of one scour).
    SD void run_jobs(u32 jn, V jdst, V jsrc, V jlen) {
        const V jl = simd::sel(L() < jn, jlen, 0u);
        const V jinc = simd::scan_incl(jl);
        const u32 total = simd::readlane(jinc, 63);
        const V jstart = jinc - jl;
        u16* ar = arena_cur();
        for (u32 base = 0; base < total; base += 64) {
            const V f = L() + base;
            V j = simd::splat(0);
            for (u32 q = 1; q < jn; q++) j = simd::sel(f >= simd::readlane(jstart, q), q, j);
            const V s0 = simd::bperm(jstart, j), d = simd::bperm(jdst, j), sr = simd::bperm(jsrc, j);
            const B m = f < total;
            const V o = f - s0;
            const B fa = (sr & ARENA_BIT) != 0u;
            const V so = (sr & ~ARENA_BIT) + o;
            const V t = simd::sel(fa, simd::ld(ar, so, m & fa), simd::ld(payload, so, simd::andn(m, fa)));
            simd::st(ar, (d & ~ARENA_BIT) + o, t, m);
        }
        adirty = true;
    }

    // T / kk and T % kk of a pack: kk in 1..7, T <= 64. The hardware has no integer divide (a run-time one is
    // some 25 vector instructions through a float reciprocal), so with kMulDiv the quotient is
    // (T * ceil(512 / kk)) >> 9, exact for these ranges (T * (kk * ceil(512 / kk) - 512) < 512); the seven
    // multipliers, less one, are nine bits each of one constant.
    SD static void div_mul(u32 T, u32 kk, u32& q, u32& r) {
        constexpr u64 M = 511ull | (255ull << 9) | (170ull << 18) | (127ull << 27) | (102ull << 36) | (85ull << 45) | (73ull << 54);
        const u32 mul = ((u32)(M >> (9u * (kk - 1u))) & 511u) + 1u;
        q = (T * mul) >> 9;
        r = T - q * kk;
    }
    SD static void div_small(u32 T, u32 kk, u32& q, u32& r) {
        RG_STAT(RS_PACK_KK1 + (kk - 1u), 1);
        RG_STAT(RS_PACK_REM, T % kk != 0);
        if constexpr (kMulDiv) {
            div_mul(T, kk, q, r);
        } else {
            q = T / kk;
            r = T % kk;
        }
    }
    // pack (mergeTree.ts:1368-1420), leaf level: the m children [k0, k0+m) of level-1 node pi
    // (already re-scoured; lane i of cn = child i's count) become max(1, min(7, T/4)) fresh blocks.
    SD void pack_leaves(u32 pi, u32 m, u32 k0, V cn) {
        RG_PROF(RP_PACK);
        RG_COUNT(RP_N_PACK, 1);
        RG_STAT(RS_PACK, 1);
        RG_DUO(packed = true);
        const u32 T = simd::readlane(simd::scan_incl(simd::sel(L() < m, cn, 0u)), 63);
        u32 kk = T / 4;
        if (kk > 7) kk = 7;
        if (kk < 1) kk = 1;
        u32 base, extra;
        div_small(T, kk, base, extra);
        RG_STAT(RS_PACK_KK_SUM, kk);
        RG_STAT(RS_PACK_GROWS, kk > m);
        RG_STAT(RS_PACK_CASCADE, kk < 4 && height > 2);
        if (!ensure_blocks(n_lb + kk - m)) return;
        // item t (lane t < T) of the concatenated children: block k0 + sib, slot q
        V sib = simd::splat(0), q = L();
        for (u32 i = 0; i < m; i++) {
            const u32 n = simd::readlane(cn, i);
            const B adv = (q >= n) & (sib == i);
            q = simd::sel(adv, q - n, q);
            sib = simd::sel(adv, i + 1, sib);
        }
        const V sg = (sib + k0) * 8u + q;  // source slot (global)
        const u32 r0 = k0 >> 3, r1 = r0 + 1 < (u32)NR ? r0 + 1 : r0;
        const B inr0 = (sg >> 6) == r0;
        Row a = rows.ldrow(r0), b = rows.ldrow(r1);
        auto gather = [&](const V& x0, const V& x1) MTE_LI {
            return simd::sel(inr0, simd::bperm(x0, sg & 63u), simd::bperm(x1, sg & 63u));
        };
        Row t;
        t.len = gather(a.len, b.len);
        t.seq = gather(a.seq, b.seq);
        t.rseq = gather(a.rseq, b.rseq);
        t.meta = gather(a.meta, b.meta) & ~NS_MASK;  // packed blocks: needsScour undefined
        t.toff = gather(a.toff, b.toff);
        t.cap = gather(a.cap, b.cap);
        t.rm = gather(a.rm, b.rm);
        t.sid = gather(a.sid, b.sid);
        if constexpr (PROPS) t.props = gather(a.props, b.props);
        if constexpr (WIDE) t.rm2 = gather(a.rm2, b.rm2);
        const i32 d = (i32)kk - (i32)m;
        shift_blocks(k0 + m, d);
        // destination: block k0 + dj slot dq <- item dj*base + min(dj, extra) + dq
        const u32 rA = k0 >> 3, rB = (k0 + kk - 1) >> 3;
        for (u32 rr = rA; rr <= rB; rr++) {
            const V G = L() + rr * 64;
            const V blk = G >> 3;
            const B inb = (blk >= k0) & (blk < k0 + kk);
            const V dj = blk - k0, dq = G & 7u;
            const V big = simd::sel(dj < extra, dj, simd::splat(extra));
            const V nB = simd::sel(dj < extra, base + 1, simd::splat(base));
            const B have = inb & (dq < nB);
            const V ti = (dj * base + big + dq) & 63u;
            Row w = rows.ldrow(rr);
            auto put = [&](V& x, const V& tv) MTE_LI { x = simd::sel(have, simd::bperm(tv, ti), simd::sel(inb, 0u, x)); };
            put(w.len, t.len);
            put(w.seq, t.seq);
            put(w.rseq, t.rseq);
            put(w.meta, t.meta);
            put(w.toff, t.toff);
            put(w.cap, t.cap);
            put(w.rm, t.rm);
            put(w.sid, t.sid);
            if constexpr (PROPS) put(w.props, t.props);
            if constexpr (WIDE) put(w.rm2, t.rm2);
            rows.strow(rr, w);
        }
        rows.drop_row();
        n_lb = (u32)((i32)n_lb + d);
        if (n_lb > max_lb) max_lb = n_lb;
        LV.set(0, simd::writelane(LV.get(0), pi, kk));
        if (kk < 4 && height > 2) pack_internal(pi, 1);
    }
    // pack_leaves' plan and scatter for the fused pack, below. (pack_leaves keeps its own text: with the two
    // sharing these functions, k_rows kernels that never fuse came out with other register and spill counts
    // than the parent's -- k_rows<4, PROPS, WIDE, CK> 490 spilled SGPRs for 429 with the scatter shared.)
    // What a pack of T items in m blocks makes: kk = max(1, min(7, T/4)) blocks of `base` items, the first
    // `extra` of them one more; false when there is no room for the blocks (the document has failed).
    SD bool pack_plan(u32 m, u32 T, u32& kk, u32& base, u32& extra) {
        RG_COUNT(RP_N_PACK, 1);
        RG_STAT(RS_PACK, 1);
        RG_DUO(packed = true);
        kk = T / 4;
        if (kk > 7) kk = 7;
        if (kk < 1) kk = 1;
        div_small(T, kk, base, extra);
        RG_STAT(RS_PACK_KK_SUM, kk);
        RG_STAT(RS_PACK_GROWS, kk > m);
        RG_STAT(RS_PACK_CASCADE, kk < 4 && height > 2);
        return ensure_blocks(n_lb + kk - m);
    }
    // The items of a pack (lane t of `t`: item t, needsScour bits clear) into blocks [k0, k0 + kk), the
    // blocks after the m old ones moved behind them, level 1 updated and the cascade run.
    SD void pack_place(u32 pi, u32 m, u32 k0, u32 kk, u32 base, u32 extra, const Row& t) {
        const i32 d = (i32)kk - (i32)m;
        shift_blocks(k0 + m, d);
        // destination: block k0 + dj slot dq <- item dj*base + min(dj, extra) + dq
        const u32 rA = k0 >> 3, rB = (k0 + kk - 1) >> 3;
        for (u32 rr = rA; rr <= rB; rr++) {
            const V G = L() + rr * 64;
            const V blk = G >> 3;
            const B inb = (blk >= k0) & (blk < k0 + kk);
            const V dj = blk - k0, dq = G & 7u;
            const V big = simd::sel(dj < extra, dj, simd::splat(extra));
            const V nB = simd::sel(dj < extra, base + 1, simd::splat(base));
            const B have = inb & (dq < nB);
            const V ti = (dj * base + big + dq) & 63u;
            Row w = rows.ldrow(rr);
            auto put = [&](V& x, const V& tv) MTE_LI { x = simd::sel(have, simd::bperm(tv, ti), simd::sel(inb, 0u, x)); };
            put(w.len, t.len);
            put(w.seq, t.seq);
            put(w.rseq, t.rseq);
            put(w.meta, t.meta);
            put(w.toff, t.toff);
            put(w.cap, t.cap);
            put(w.rm, t.rm);
            put(w.sid, t.sid);
            if constexpr (PROPS) put(w.props, t.props);
            if constexpr (WIDE) put(w.rm2, t.rm2);
            rows.strow(rr, w);
        }
        rows.drop_row();
        n_lb = (u32)((i32)n_lb + d);
        if (n_lb > max_lb) max_lb = n_lb;
        LV.set(0, simd::writelane(LV.get(0), pi, kk));
        if (kk < 4 && height > 2) pack_internal(pi, 1);
    }
    // ---- the fused pack (kFusedPack): the sibling pass and pack_leaves in one pass over the one or two
    // rows that hold blocks [k0, k0 + m). scour's predicates are taken row-wide, as 64-bit lane masks
    // restricted to the sibling lanes; the runs' heads take their new len / toff / cap in registers; the
    // kept slots (not dropped, not joined) are pushed straight to their item lane. No sibling is
    // compacted, stored and read again only to be taken apart. Results are scour's and pack_leaves', bit
    // for bit: the heads are walked in sibling order, then head order, so every fresh chunk has the offset
    // the sibling loop gives it.
    //
    // One row's share: scour's decisions for the sibling lanes `sib` of row w, then its runs. Out: the
    // heads' new (len, toff, cap) in nlen / ntoff / ncap (the other lanes as they were); the text copies as
    // (jdst, jlen) per slot lane (sources: w.toff); fresh chunks taken from `top` on, their sum added to
    // `need`; dst, the item lane of every kept slot (nBefore + its rank among the row's kept slots; the
    // other lanes fill the rest of the wave, so dst is a permutation), nkeep of them; chg, the lanes
    // dropped or joined; serial: a joining slot is longer than GRANULARITY. Nothing is written. (The masks
    // are done with before the next row starts: the replay loop has no scalar registers to spare.)
    SD void pack_row(const Row& w, u64 sib, u32 nBefore, V& nlen, V& ntoff, V& ncap, V& jdst, V& jlen, V& dst, u32& nkeep,
                     u64& chg, bool& serial, u32& top, u32& need) {
        const u64 act = simd::ballot(w.len != 0u) & sib;
        const u64 rem = act & simd::ballot(w.rseq != RSEQ_LIVE);
        const u64 drop = rem & simd::ballot(simd::sle(w.rseq, minSeq));
        const u64 st = act & ~rem & simd::ballot(simd::sle(w.seq, minSeq)) & simd::ballot((w.meta & F_MARKER) == 0u);
        u64 join = st & (st << 1) & ~0x0101010101010101ull;  // slot 0 has no slot before it in its block
        if constexpr (PROPS) {  // ... when its properties match slot s-1's (matchProperties)
            const u64 same = simd::ballot(w.props == simd::row_shr1(w.props));
            for (u64 c = join & ~same; c; c &= c - 1) {
                const u32 l = (u32)__builtin_ctzll(c);
                if (!match_props(simd::readlane(w.props, l - 1), simd::readlane(w.props, l))) join &= ~(1ull << l);
            }
        }
        serial = (join & simd::ballot(w.len > (u32)GRANULARITY)) != 0;
        chg = drop | join;
        const u64 keep = act & ~chg;
        nkeep = (u32)__builtin_popcountll(keep);
        const V rk = simd::rank_below(keep);
        dst = (simd::sel(simd::ballot_mask(keep), rk, (L() - rk) + nkeep) + nBefore) & 63u;
        nlen = w.len;
        ntoff = w.toff;
        ncap = w.cap;
        jdst = jlen = simd::splat(0);
        u64 heads = st & ~join & (join >> 1);
        if (!heads) return;
        const V ex = simd::scan_incl(w.len) - w.len;  // only differences inside one block are used
        const u64 mCONT = simd::ballot(w.toff == simd::row_shr1(w.toff + w.len));
        for (; heads; heads &= heads - 1) {  // sibling order, then head order: scour's order
            const u32 lh = (u32)__builtin_ctzll(heads);                    // a head is never slot 7: lh <= 62
            const u32 le = lh + (u32)__builtin_ctzll(~(join >> (lh + 1)));  // the run's last slot (same block)
            const u64 rb = ((2ull << le) - 1ull) & ~((2ull << lh) - 1ull);  // lanes lh+1..le
            const u32 off = simd::readlane(w.toff, lh), cap = simd::readlane(w.cap, lh);
            const u32 exh = simd::readlane(ex, lh);
            const u32 total = simd::readlane(ex, le) + simd::readlane(w.len, le) - exh;
            u32 noff = off, nc = cap;
            u64 cbits = 0;
            if ((mCONT & rb) == rb) {  // the run's text is one contiguous range already
                if (off & ARENA_BIT) nc = simd::readlane(w.toff, le) + simd::readlane(w.cap, le) - off;
            } else if ((off & ARENA_BIT) && total <= cap) {  // append into the head's chunk
                cbits = rb;
            } else {  // a fresh chunk
                nc = 2 * total < 32 ? 32u : 2 * total;
                noff = top | ARENA_BIT;
                top += nc;
                need += nc;
                cbits = rb | (1ull << lh);
            }
            if (cbits) {
                const B cp = simd::ballot_mask(cbits);
                jdst = simd::sel(cp, ex + (noff - exh), jdst);
                jlen = simd::sel(cp, w.len, jlen);
            }
            nlen = simd::writelane(nlen, lh, total);
            ntoff = simd::writelane(ntoff, lh, noff);
            ncap = simd::writelane(ncap, lh, nc);
        }
    }
    // Pack the m children [k0, k0 + m) of level-1 node pi; k is the popped block among them (already
    // scoured once and stored: it is decided like the rest, and joins across a tombstone that pass dropped).
    // false: nothing was done, and the pack needs the sibling loop -- a joining slot is longer than
    // GRANULARITY (scour_serial), or the fresh chunks do not fit the arena (arena_gc).
    SD bool pack_fused(u32 pi, u32 m, u32 k0, u32 k) {
        RG_PROF(RP_PACK_FUSED);
        const u32 r0 = k0 >> 3, r1 = (k0 + m - 1) >> 3, g0 = k0 & 7u;
        const bool two = r1 != r0;
        const u32 mA = two ? 8u - g0 : m;  // siblings in row r0; two rows: 1..7 in each
        const Row a = rows.row(r0);
        Row b;
        if (two) b = rows.ldrow(r1);
        V lenA, toffA, capA, jdA, jlA, dstA, lenB, toffB, capB, jdB, jlB, dstB;
        u32 top = arenaTop, need = 0, nA, nB = 0;
        u64 chgA, chgB = 0;
        bool serA, serB = false;
        pack_row(a, (mA == 8 ? ~0ull : (1ull << (mA * 8)) - 1ull) << (g0 * 8), 0, lenA, toffA, capA, jdA, jlA, dstA, nA, chgA, serA,
                 top, need);
        if (two) pack_row(b, (1ull << ((m - mA) * 8)) - 1ull, nA, lenB, toffB, capB, jdB, jlB, dstB, nB, chgB, serB, top, need);
        if (serA | serB) {
            RG_STAT(RS_PACK_FUSED_FB_SERIAL, 1);
            return false;
        }
        if (arenaTop + need > arena_cap) {
            RG_STAT(RS_PACK_FUSED_FB_GC, 1);
            return false;
        }
        RG_STAT(RS_PACK_FUSED, 1);
        RG_COUNT(RP_N_SCOUR, m);
        RG_COUNT(RP_N_SCOUR_CHANGED, changed_blocks(chgA) + changed_blocks(chgB));
#if defined(MTE_CPU) && defined(MTE_CPU_STATS)
        for (u32 idx = 0; idx < m; idx++) {  // the sibling loop's counters: siblings decided / unchanged / changed
            const u32 blk = k0 + idx;
            RG_STAT(RS_SCOUR, 1);
            RG_STAT(RS_PACK_SCOUR, 1);
            if (!group_bits((blk >> 3) == r0 ? chgA : chgB, blk)) {
                RG_STAT(RS_SCOUR_NOP, 1);
                RG_STAT(RS_PACK_SCOUR_NOP, 1);
            } else {
                RG_STAT(blk == k ? RS_PACK_SELF_CHANGED : RS_PACK_SIB_CHANGED, 1);
            }
        }
#endif
        arenaTop = top;
        if (chgA | chgB) {
            // One fence for all copies, then one gather per row. No copy reads what another one writes:
            // every destination is a fresh chunk above the old arenaTop or the free tail [off + len,
            // off + cap) of a head's own chunk, and every source is text some slot held before this pack
            // (chunks are never shared: split_at divides a chunk's capacity between the two pieces).
            fence_arena();
            if (chgA) RG_DUO(w |= 1ull << r0);
            if (chgB) RG_DUO(w |= 1ull << r1);
            copy_runs(jdA, a.toff, jlA);
            if (two) copy_runs(jdB, b.toff, jlB);
        }
        u32 kk, base, extra;
        if (!pack_plan(m, nA + nB, kk, base, extra)) return true;
        // item t of the concatenated children is the t-th kept slot: each kept lane is pushed to its rank
        Row t;
        if (two) {
            const B fromA = L() < nA;
            auto gather = [&](const V& x0, const V& x1) MTE_LI { return simd::sel(fromA, simd::push(x0, dstA), simd::push(x1, dstB)); };
            t.len = gather(lenA, lenB);
            t.seq = gather(a.seq, b.seq);
            t.rseq = gather(a.rseq, b.rseq);
            t.meta = gather(a.meta, b.meta);
            t.toff = gather(toffA, toffB);
            t.cap = gather(capA, capB);
            t.rm = gather(a.rm, b.rm);
            t.sid = gather(a.sid, b.sid);
            if constexpr (PROPS) t.props = gather(a.props, b.props);
            if constexpr (WIDE) t.rm2 = gather(a.rm2, b.rm2);
        } else {
            t.len = simd::push(lenA, dstA);
            t.seq = simd::push(a.seq, dstA);
            t.rseq = simd::push(a.rseq, dstA);
            t.meta = simd::push(a.meta, dstA);
            t.toff = simd::push(toffA, dstA);
            t.cap = simd::push(capA, dstA);
            t.rm = simd::push(a.rm, dstA);
            t.sid = simd::push(a.sid, dstA);
            if constexpr (PROPS) t.props = simd::push(a.props, dstA);
            if constexpr (WIDE) t.rm2 = simd::push(a.rm2, dstA);
        }
        t.meta = t.meta & ~NS_MASK;  // packed blocks: needsScour undefined
        pack_place(pi, m, k0, kk, base, extra, t);
        return true;
    }
    // blocks (aligned 8-lane groups) with a bit set in m
    SD static u32 changed_blocks(u64 m) {
        m |= m >> 4;
        m |= m >> 2;
        m |= m >> 1;
        return (u32)__builtin_popcountll(m & 0x0101010101010101ull);
    }
    // pack on an interior level: node pi of level lv underflowed; the children of its parent are
    // redistributed into max(1, min(7, T/4)) nodes, T their total child count.
    SD void pack_internal(u32 pi, u32 lv) {
        for (u32 guard = 0; guard < RG_LEVELS + 2; guard++) {
            u32 i0;
            const u32 qi = parent_of(lv, pi, i0);  // parent at level lv+1
            const V Q = LV.get(lv);
            const u32 m = simd::readlane(Q, qi);
            V C = LV.get(lv - 1);  // child counts of the level-lv nodes
            const u32 T = simd::readlane(simd::scan_incl(simd::sel((L() >= i0) & (L() < i0 + m), C, 0u)), 63);
            u32 kk = T / 4;
            if (kk > 7) kk = 7;
            if (kk < 1) kk = 1;
            u32 base, extra;
            div_small(T, kk, base, extra);
            RG_STAT(RS_PACK_INTERNAL, 1);
            const i32 d = (i32)kk - (i32)m;
            // lanes after the old range move by d
            const V src = L() - (u32)d;
            const V moved = simd::bperm(C, src & 63u);
            C = simd::sel(L() >= i0 + kk, simd::sel(src < 64u, moved, 0u), C);
            const V dj = L() - i0;
            C = simd::sel((L() >= i0) & (L() < i0 + kk), simd::sel(dj < extra, base + 1, simd::splat(base)), C);
            LV.set(lv - 1, C);
            LV.set(lv, simd::writelane(Q, qi, kk));
            if (kk < 4 && lv + 2 < height) {
                pi = qi;
                lv++;
                continue;
            }
            return;
        }
        fail(MTE_DOC_CAPACITY, curSeq);
    }

    // zamboniSegments (mergeTree.ts:1422-1478): up to 2 heap entries with maxSeq <= minSeq.
    SD void zamboni() {
        RG_PROF(RP_ZAMBONI);
        RG_STAT(RS_ZAM_CALLS, 1);
        for (int i = 0; i < 2 && !status; i++) {
            if (heapSize == 0 || heapTop > minSeq) break;
            RG_STAT(RS_ZAM_POPS, 1);
            const u32 k = heap_pop_find();
            if (k == NONE) continue;  // no longer linked
            if (ns_get(k) == SC_FALSE) continue;
            const u32 cnt = count(k);
            const u32 nc = scour(k, cnt);
            if (status) return;
            if (!scoured) ns_set(k, SC_FALSE);
            if (!(nc < cnt && nc < 4 && height > 1)) continue;
            u32 k0;
            const u32 pi = parent_of(0, k, k0);
            const u32 m = simd::readlane(LV.get(0), pi);
            if (m == 0 || m > 8 || k0 + m > n_lb) {
                fail(MTE_DOC_CAPACITY, curSeq);
                return;
            }
            V cn = simd::splat(0);
#if defined(MTE_CPU) && defined(MTE_CPU_STATS)
            const u64 serial0 = g_rg_stats[RS_SCOUR_SERIAL];
            const u32 gc0 = n_gc;
            RG_STAT(((k0 + m - 1) >> 3) == (k0 >> 3) ? RS_PACK_ONE_ROW : RS_PACK_TWO_ROWS, 1);
            RG_STAT(RS_PACK_M8, m == 8);
            RG_STAT(RS_PACK_M_SUM, m);
#endif
            // The popped block k is among them and is scoured a second time, as scourNode is in the
            // reference: a tombstone the first pass dropped had reset the merge chain, and the settled
            // text on its two sides, adjacent now, joins in this pass (RS_PACK_SELF_CHANGED counts it).
            if constexpr (kFusedPack) {
                if (pack_fused(pi, m, k0, k)) continue;  // (else: the serial walk or arena_gc, below)
            }
            {
                RG_PROF(RP_PACK_SIBS);
                for (u32 idx = 0; idx < m; idx++) {
                    RG_STAT(RS_PACK_SCOUR, 1);
                    const u32 c = scour(k0 + idx, count(k0 + idx));
                    if (status) return;
                    if (!scoured) RG_STAT(RS_PACK_SCOUR_NOP, 1);
                    else RG_STAT(k0 + idx == k ? RS_PACK_SELF_CHANGED : RS_PACK_SIB_CHANGED, 1);
                    cn = simd::writelane(cn, idx, c);
                }
            }
#if defined(MTE_CPU) && defined(MTE_CPU_STATS)
            RG_STAT(RS_PACK_SERIAL, g_rg_stats[RS_SCOUR_SERIAL] != serial0);
            RG_STAT(RS_PACK_GC, n_gc != gc0);
#endif
            pack_leaves(pi, m, k0, cn);
        }
    }

    // ---------------------------------------------------------------- ops
    // ensureIntervalBoundary at the resolved slot (BaseSegment.splitAt, mergeTree.ts:524-568): the
    // right piece copies everything and follows the left one. Returns the insert_slot result.
    SD u32 split_at(const RFound& f) {
        RG_PROF(RP_SPLIT_AT);
        RG_STAT(RS_SPLIT_AT, 1);
        const u32 r = f.k >> 3, l = gbase(f.k) + (u32)f.slot;
        const Row w = rows.row(r);
        RSeg t;
        t.len = simd::readlane(w.len, l);
        t.seq = (i32)simd::readlane(w.seq, l);
        t.rseq = simd::readlane(w.rseq, l);
        t.meta = simd::readlane(w.meta, l);
        t.toff = simd::readlane(w.toff, l);
        t.cap = simd::readlane(w.cap, l);
        t.rm = simd::readlane(w.rm, l);
        if constexpr (PROPS) t.props = simd::readlane(w.props, l);  // the right piece shares the map
        if constexpr (WIDE) t.rm2 = simd::readlane(w.rm2, l);
        const u32 sid = new_sid();
        if (sid == NONE) return NONE;
        const u32 rr = (u32)f.r;
        const bool ar = (t.toff & ARENA_BIT) != 0;  // arena text: cap >= len, split between the pieces
        const u32 lc = ar ? rr : 0u;
        RSeg right = t;
        right.len = t.len - rr;
        right.toff = t.toff + rr;
        right.cap = ar ? t.cap - rr : 0u;
        right.sid = sid;
        return insert_slot(f.k, f.cnt, (u32)f.slot + 1, right, true, rr, lc);
    }

    // insertSegments (mergeTree.ts:1968-1998): split at pos, then place the new segment.
    SD bool op_insert(i32 pos, i32 R, u32 C, i32 seq, RSeg rec) {
        RG_PROF(RP_INS);
        RFound f = resolve(pos, R, C);
        if (!f.ok) {
            fail(MTE_DOC_INSERT_FAILED, seq);
            return false;
        }
        u32 k = f.k, j;
        if (f.slot >= 0 && f.r > 0) {
            if (split_at(f) == NONE || status) return false;
            // the insertion point follows from the split: before the right piece, except when the
            // block split 4+4 right between the two pieces (blocks win ties: append to the left)
            const u32 s = (u32)f.slot;
            if (f.cnt + 1 < 8 || s + 1 < 4) {
                j = s + 1;
                f.cnt = f.cnt + 1 < 8 ? f.cnt + 1 : 4;
            } else if (s == 3) {
                j = 4;
                f.cnt = 4;
            } else {
                k = f.k + 1;
                j = s - 3;
                f.cnt = 4;
            }
        } else {
            j = f.slot >= 0 ? (u32)f.slot : f.cnt;
        }
        if (rec.len == 0) return false;  // blockInsert skips empty segments (:2196)
        rec.sid = new_sid();
        if (rec.sid == NONE) return false;
        const u32 b = insert_slot(k, f.cnt, j, rec, false, 0, 0, seq > minSeq ? seq : 0);
        if (status) return false;
        if (seq > minSeq && !lruFolded) add_lru(b, rec.sid, seq);
        return status == 0;
    }

    // markRangeRemoved (mergeTree.ts:2607-2719): split at p1 and p2, then mark [p1, p2) of the
    // (R, C) view before the op: first remover wins, later ones join removedClientOverlap.
    SD bool op_remove(i32 p1, i32 p2, i32 R, u32 C, i32 seq) {
        RG_PROF(RP_REM);
        // the p2 resolve and the marking start at p1's row: nothing before it moves or changes
        // visible length (a split keeps the lengths, a block split shifts only later blocks)
        u32 r1 = 0, c1 = 0;
        RG_STAT(RS_REM, 1);
        [[maybe_unused]] bool f1ok = false, bsplit = false;  // (statistics only)
        for (u32 ph = 0; ph < 2; ph++) {
            const RFound f = resolve(ph ? p2 : p1, R, C, r1, c1);
            if (ph == 0 && f.ok) {
                r1 = f.row;
                c1 = f.carry;
                f1ok = true;
            }
            const bool split = f.ok && f.slot >= 0 && f.r > 0;
            bsplit = bsplit || (split && f.cnt + 1 >= 8);
            if (ph) {
                RG_STAT(RS_RES2_ROWS, f.ok ? f.row - r1 + 1 : ((n_lb + 7) >> 3) - r1);
                RG_STAT(RS_REM_SAMEROW, f1ok && f.ok && f.row == r1);
                RG_STAT(RS_REM_SAMEROW_NOSPLIT, f1ok && f.ok && f.row == r1 && !bsplit);
            }
            if (!split) continue;
            if (split_at(f) == NONE || status) return false;
        }
        RG_PROF(RP_RANGE);
        const u32 nrows = (n_lb + 7) >> 3;
        u32 carry = c1;
        const u32 cbit = WIDE ? 1u << (C & 31u) : 1u << C;
        for (u32 r = r1; r < nrows && (i32)carry < p2; r++) {
            RG_STAT(RS_RANGE_ROWS, 1);
            Row& w = rows.rowref(r);
            const V v = vis(w, R, C);
            const V incl = simd::scan_incl(v) + carry;
            const V ex = incl - v;
            const B mark = (v != 0u) & simd::slt(ex, p2) & simd::sgt(incl, p1);
            carry = simd::readlane(incl, 63);
            const u64 mm = simd::ballot(mark);
            if (!mm) continue;
            const B was = mark & (w.rseq != RSEQ_LIVE);  // already removed: addOverlappingClient
            const B fresh = simd::andn(mark, was);
            if (WIDE && C >= 32) {
                if constexpr (WIDE) w.rm2 = simd::sel(mark, w.rm2 | cbit, w.rm2);
            } else {
                w.rm = simd::sel(mark, w.rm | cbit, w.rm);
            }
            w.meta = simd::sel(was, w.meta | F_OVL, simd::sel(fresh, (w.meta & ~0xFF00u) | (C << 8) | F_REMOVED, w.meta));
            w.rseq = simd::sel(fresh, (u32)seq, w.rseq);
            if constexpr (kFoldLru) {
                // addToLRUSet per block, document order, at the first marked slot of each block: the
                // needsScour marks go into this row write, the heap pushes follow it
                u64 pm = 0;
                if (seq > curSeq) {
                    const u64 nst = simd::ballot(((w.meta >> NS_SHIFT) & 3u) == SC_TRUE);  // (every lane of a block holds it)
                    u64 grp = 0;
                    for (u64 gm = mm & ~nst; gm;) {
                        const u32 l = (u32)__builtin_ctzll(gm);
                        const u64 g8 = 0xFFull << (l & ~7u);
                        gm &= ~g8;
                        pm |= 1ull << l;
                        grp |= g8;
                    }
                    if (grp) w.meta = simd::sel(simd::ballot_mask(grp), (w.meta & ~NS_MASK) | (SC_TRUE << NS_SHIFT), w.meta);
                }
                rows.writeback(r);
                for (; pm; pm &= pm - 1) {
                    RG_STAT(RS_LRU_FOLDED, 1);
                    heap_push(simd::readlane(w.sid, (u32)__builtin_ctzll(pm)), seq);
                    if (status) return false;
                }
            } else {
                rows.writeback(r);
                // addToLRUSet per block, document order: the first marked slot of each block
                for (u64 gm = mm; gm;) {
                    const u32 l = (u32)__builtin_ctzll(gm);
                    const u32 g = l >> 3;
                    gm &= ~(0xFFull << (g * 8));
                    add_lru(r * 8 + g, simd::readlane(w.sid, l), seq);
                    if (status) return false;
                }
            }
        }
        return status == 0;
    }

    // annotateRange (mergeTree.ts:2565-2605; PROPS): split at p1 and p2 like a remove, then every
    // segment of [p1, p2) visible in the (R, C) view takes a new map, addProperties of the op's set on
    // its old one (one map per distinct old map: the LDS engine's memo of the last one built).
    SD bool op_annotate(i32 p1, i32 p2, i32 R, u32 C, i32 seq, u32 propset, bool rewrite) {
        RG_PROF(RP_REM);
        u32 r1 = 0, c1 = 0;
        for (u32 ph = 0; ph < 2; ph++) {
            const RFound f = resolve(ph ? p2 : p1, R, C, r1, c1);
            if (ph == 0 && f.ok) {
                r1 = f.row;
                c1 = f.carry;
            }
            if (!f.ok || !(f.slot >= 0 && f.r > 0)) continue;
            if (split_at(f) == NONE || status) return false;
        }
        RG_PROF(RP_RANGE);
        const u32 nrows = (n_lb + 7) >> 3;
        u32 carry = c1, memoOld = NONE, memoNew = 0;
        for (u32 r = r1; r < nrows && (i32)carry < p2; r++) {
            Row& w = rows.rowref(r);
            const V v = vis(w, R, C);
            const V incl = simd::scan_incl(v) + carry;
            const V ex = incl - v;
            const B mark = (v != 0u) & simd::slt(ex, p2) & simd::sgt(incl, p1);
            carry = simd::readlane(incl, 63);
            const u64 mm = simd::ballot(mark);
            if (!mm) continue;
            for (u64 pending = mm; pending;) {
                const u32 old = simd::readlane(w.props, (u32)__builtin_ctzll(pending));
                u32 nid;
                if (old == memoOld) {
                    nid = memoNew;
                } else {
                    nid = build_map(old, propset, rewrite);
                    if (status) return false;
                    memoOld = old;
                    memoNew = nid;
                }
                const B same = simd::ballot_mask(pending) & (w.props == old);
                w.props = simd::sel(same, nid, w.props);
                pending &= ~simd::ballot(same);
            }
            rows.writeback(r);
            for (u64 gm = mm; gm;) {  // addToLRUSet per block, document order
                const u32 l = (u32)__builtin_ctzll(gm);
                const u32 g = l >> 3;
                gm &= ~(0xFFull << (g * 8));
                add_lru(r * 8 + g, simd::readlane(w.sid, l), seq);
                if (status) return false;
            }
        }
        return status == 0;
    }

    // Room for one more op (margins for the splits, packs and heap pushes an op can cause);
    // false => hand the document to the LDS engine before this op.
    SD bool room() {
        // level-1 nodes hold >= 1 leaf block each, so fewer than 57 blocks cannot reach lane 56 (and
        // the readlane, a VALU -> SALU round trip, is skipped)
        if constexpr (PAGED) {
            // rows are taken as blocks appear (ensure_blocks), so no block margin; pool rows past
            // the last block's row go back at once (a spare per wave, twelve per CU, had made the
            // pool run out on C2's peaks)
            const u32 keep = (n_lb + 7) >> 3;
            if (rows.n_rows > keep) rows.shrink_rows(keep);
            return n_lb + 4 <= lb_lim && heapSize + n_lb + 8 < RG_HEAP && height + 2 <= RG_LEVELS &&
                   (n_lb < 57 || simd::readlane(LV.get(0), 56) == 0u);
        }
        return n_lb + 16 <= lb_lim && heapSize + n_lb + 8 < RG_HEAP && height + 2 <= RG_LEVELS &&
               (n_lb < 57 || simd::readlane(LV.get(0), 56) == 0u);
    }

    // Client.applyMsg for one op record (client.ts:805-836) in two halves, split where the op's own
    // edit ends and the lazy clean-up begins:
    //   apply_edit:   decode, checks, room, the insert / remove / annotate with its resolves, splits
    //                 and needsScour marks (add_lru);
    //   apply_settle: the two zamboni calls with the curSeq / minSeq advance between them.
    // Nothing settle does changes what any (refSeq >= minSeq) view sees: scour drops tombstones at or
    // below minSeq and merges settled text, pack redistributes slots; it changes only WHERE things are.
    // apply() runs them back to back; every kernel and the CPU build replay through it.
    SD bool apply(const mte_op& op) {
        RG_PROF(RP_APPLY);
        bool edited = false;
        if (!apply_edit(op, edited)) return false;
        if (status) return true;
        RG_DUO(settle_begin());
        apply_settle(op.seq, op.msn, (op.flags & MTE_F_END_OF_MSG) != 0, edited);
        RG_DUO(settle_end());
        return true;
    }
    // false => not applied, hand off; `edited`: the op changed the tree (the first zamboni runs)
    SD bool apply_edit(const mte_op& op, bool& edited) {
        RG_STAT(RS_OPS, 1);
        const u32 type = op.type;
        const bool ins = type == MTE_OP_INSERT || type == MTE_OP_INSERT_MARKER;
        const bool ann = PROPS && type == MTE_OP_ANNOTATE;
        if (!(ins || ann || type == MTE_OP_REMOVE || type == MTE_OP_NOOP)) return false;
        // (MTE_F_CATCHUP only asks for delta records, which only a legacy-format replay reads: that one
        // runs the EXT kernels, so here the flag is ignored like the lean LDS kernels do)
        if ((op.flags & (MTE_F_REL | MTE_F_PERM)) || (!PROPS && op.props)) return false;
        if (type != MTE_OP_NOOP && (op.client == 0 || op.client >= MAXC)) return false;
        if (!room()) {
            RG_STAT(RS_ROOM_REFUSED, 1);
            return false;
        }
        const u32 C = op.client;
        const i32 seq = op.seq, R = op.ref_seq;
        if (type != MTE_OP_NOOP && !(curSeq < seq)) {
            fail(MTE_DOC_SEQ_ORDER, seq);
            return true;
        }
        if (ins) {
            RSeg rec;
            const bool mk = type == MTE_OP_INSERT_MARKER;
            rec.len = mk ? 1u : op.b;
            rec.seq = seq;
            rec.rseq = RSEQ_LIVE;
            rec.meta = (C & 0xFFu) | (RCL_LIVE << 8) | (mk ? F_MARKER : 0u);
            rec.toff = mk ? op.b : (u32)op.a;
            rec.cap = 0;
            rec.rm = 0;
            rec.sid = 0;
            if constexpr (PROPS) {
                rec.props = op.props ? build_map(0, op.props, false) : 0u;
                if (status) return true;
            }
            edited = op_insert(op.pos1, R, C, seq, rec);
            count_op();
        } else if (type == MTE_OP_REMOVE) {
            edited = op_remove(op.pos1, op.a, R, C, seq);
            count_op();
        } else if (ann) {
            if constexpr (PROPS) edited = op_annotate(op.pos1, op.a, R, C, seq, op.props, (op.flags & MTE_F_REWRITE) != 0);
            count_op();
        }
        return true;
    }
    // the settle half of an applied op (status 0 on entry): seq / msn of its record, eom its
    // end-of-message flag
    SD void apply_settle(i32 seq, i32 msn, bool eom, bool edited) {
        if (edited) {
            RG_PROF(RP_ZAM_EDIT);
            zamboni();
        }
        if (status) return;
        if (eom) {
            count_msg();
            if (seq < curSeq || msn > seq || msn < minSeq) {
                fail(MTE_DOC_SEQ_ORDER, seq);
                return;
            }
            curSeq = seq;
            if (msn > minSeq) {
                RG_PROF(RP_MSN);
                minSeq = msn;
                zamboni();
            }
        }
    }

    // Replay ops [i, e): returns the first op not applied (e when done or failed; earlier when the
    // document hands over to the LDS engine). Records are prefetched 8 per VGPR (lane 8*r + w holds
    // word w of record r), four chunks ahead.
    SD u64 replay(u64 i0, u64 e) {
        if (!p.docs[doc].collab) {  // local, non-collaborative edits: the LDS engine's path
            status = REG_HANDOFF;
            return i0;
        }
        RG_PROF(RP_TOTAL);
        // this document's records from one base pointer, indexed by 32-bit op numbers (a 64-bit
        // global op index in the loop held three more SGPR pairs in a kernel that spills SGPRs)
        const u32* src = (const u32*)p.ops + i0 * 8;
        const u32 n = (u32)(e - i0);
        auto load_chunk = [&](u32 c0) MTE_LI {  // records [c0, c0+8)
            const u32 left = n > c0 ? n - c0 : 0u;
            const u32 nw = left >= 8 ? 64u : left * 8u;
            return simd::ld(src + (u64)c0 * 8, L(), L() < nw);
        };
        // Two chunk registers: CUR holds the records being decoded, NXT the next eight. At a chunk's
        // first op CUR = NXT (loaded eight ops earlier), the op is decoded, and only THEN is NXT
        // refilled: the compiler waits for the whole vector-memory counter before a decode, so the
        // newest load outstanding there must be an op old. (Loading before the decode, or a
        // four-register ring indexed by a switch, made every chunk wait for a fresh HBM load.)
        V CUR = load_chunk(0), NXT = load_chunk(8);
        // wait for the first chunk here, once: CUR then enters the loop with no load outstanding, so
        // the decodes need no vector-memory wait at all (stores of the merge arena included)
        simd::wait_loaded(CUR);
        u32 k = 0;
        for (; k < n && !status; k++) {
            const u32 r = k & 7u;
            const bool first = r == 0 && k != 0;
            if (first) {
                CUR = NXT;
                simd::keep_branch();  // keep this a branch: a select would read NXT (and wait) every op
            }
            mte_op op;
            {
                RG_PROF(RP_FETCH);
                u32 w[8];
                for (u32 x = 0; x < 8; x++) w[x] = simd::readlane(CUR, r * 8 + x);
                __builtin_memcpy(&op, w, sizeof op);
            }
            if (first) NXT = load_chunk(k + 8);
            RG_COUNT(RP_OPS, 1);
            if (!apply(op)) {
                status = REG_HANDOFF;
                return i0 + k;
            }
        }
        return i0 + k;
    }

    // ---------------------------------------------------------------- results
    // The final segments in document order (walkAllSegments, mergeTree.ts:2969-2983) in the LDS
    // engine's row format (removedSeq 0 and removedClient 0 for live segments), text gathered into
    // the document's run of the output text pool, and the per-document result record.
    // the document leaves this engine unfinished (k_rows has no LDS plan to hand it to): the host
    // re-runs it HBM-resident from its first op (engine.hpp mark_spilled)
    SD void mark_spilled() {
        fence_arena();
        if (simd::lane0()) {
            DocRes& o = p.res[doc];
            o.status = DOC_SPILL;
            o.failing_seq = curSeq;
            o.n_segs = 0;
            o.max_lb = max_lb;
            o.mode = 0;
            o.spill_why = (n_lb << 8) | (heapSize << 20);
            simd::count_add(&p.counters[2], 1u);
        }
    }
    SD void finish() {
        fence_arena();
        const u32 nrows = (n_lb + 7) >> 3;
        u32 nseg = 0, ntext = 0;
        for (u32 r = 0; r < nrows; r++) {
            const V len = ld_len(r);
            const B txt = (len != 0u) & ((ld_meta(r) & F_MARKER) == 0u);
            nseg += (u32)__builtin_popcountll(simd::ballot(len != 0u));
            ntext += simd::readlane(simd::scan_incl(simd::sel(txt, len, 0u)), 63);
        }
        u32 off = 0, toff = 0;
        if (status == 0) {
            off = simd::reserve(&p.counters[1], nseg);
            toff = (u32)simd::reserve((u64*)&p.counters[6], (u64)ntext);
            if ((u64)off + nseg > p.out_cap || (u64)toff + ntext > p.out_text_cap) {
                fail(MTE_DOC_CAPACITY, curSeq);
                nseg = 0;
            }
        } else {
            nseg = 0;
        }
        if (nseg) {
            u32 run = off, trun = 0;
            u16* tdst = p.out_text + toff;
            u32* ov = (u32*)p.out_vis;
            u32* oa = (u32*)p.out_aux;
            u32* oo = (u32*)p.out_ovl;
            for (u32 r = 0; r < nrows; r++) {
                const Row w = rows.ldrow(r);
                const B have = w.len != 0u;
                const B txt = have & ((w.meta & F_MARKER) == 0u);
                const V one = simd::sel(have, 1u, simd::splat(0));
                const V at = simd::scan_incl(one) - one + run;
                const V tl = simd::sel(txt, w.len, 0u);
                const V tat = simd::scan_incl(tl) - tl + trun;
                const B live = w.rseq == RSEQ_LIVE;
                const B hasov = (w.meta & F_OVL) != 0u;
                const V m2 = simd::sel(live, w.meta & ~0xFF00u, w.meta) & ~NS_MASK;
                // removedClientOverlap = the removers but removedClient (the LDS engine's format)
                V ovm, ovh = simd::splat(0);
                if constexpr (WIDE) {  // removedClient may be 32..63: its bit is in rm2 then
                    const V rc = simd::bfe(w.meta, 8, 8);
                    const V rcb = simd::shl(simd::splat(1), rc);  // bit rc & 31
                    const B rclo = rc < 32u;
                    ovm = w.rm & (simd::sel(rclo, rcb, 0u) ^ 0xFFFFFFFFu);
                    ovh = simd::sel(hasov, w.rm2 & (simd::sel(rclo, 0u, rcb) ^ 0xFFFFFFFFu), 0u);
                } else {
                    ovm = w.rm & (simd::shl(simd::splat(1), simd::bfe(w.meta, 8, 8)) ^ 0xFFFFFFFFu);
                }
                const V ovl = simd::sel(hasov, ovm, 0u);
                const V z2 = simd::sel(live, w.cap, ovl);
                const V t4 = at * 4u;
                simd::st(ov, t4, w.len, have);
                simd::st(ov, t4 + 1u, w.seq, have);
                simd::st(ov, t4 + 2u, simd::sel(live, 0u, w.rseq), have);
                simd::st(ov, t4 + 3u, m2, have);
                V pm = simd::splat(0);
                if constexpr (PROPS) pm = w.props;
                simd::st(oa, t4, pm, have);
                if constexpr (PROPS) {  // the row's property map, indexed by row (emission reads it)
                    const B hp = have & (w.props != 0u);
                    if (p.out_maps && simd::ballot(hp)) {
                        fence_arena();
                        for (u32 q = 0; q < mw; q++)
                            simd::st(p.out_maps, at * mw + q, simd::ld(maps, w.props * mw + q, hp), hp);
                    }
                }
                simd::st(oa, t4 + 1u, simd::sel(txt, tat, w.toff), have);
                simd::st(oa, t4 + 2u, z2, have);
                simd::st(oa, t4 + 3u, w.sid - 1u, have);
                simd::st(oo, at * 2u, ovl, have);
                simd::st(oo, at * 2u + 1u, ovh, have);
                if (p.out_ovl2) {  // clients 64..127: never on the rows (their first op hands over)
                    simd::st((u32*)p.out_ovl2, at * 2u, simd::splat(0), have);
                    simd::st((u32*)p.out_ovl2, at * 2u + 1u, simd::splat(0), have);
                }
                // text, one segment at a time, 64 units per step
                for (u64 tm = simd::ballot(txt); tm; tm &= tm - 1) {
                    const u32 l = (u32)__builtin_ctzll(tm);
                    copy_text(simd::readlane(tat, l), simd::readlane(w.toff, l), simd::readlane(w.len, l), tdst);
                }
                run += (u32)__builtin_popcountll(simd::ballot(have));
                trun += simd::readlane(simd::scan_incl(tl), 63);
            }
        }
        DocRes& o = p.res[doc];
        if (simd::lane0()) {
            o.status = status;
            o.failing_seq = status ? failSeq : -1;
            o.ops = ops_n();
            o.msgs = msgs_n();
            o.min_seq = minSeq;
            o.cur_seq = curSeq;
            o.height = height;
            o.n_lb = n_lb;
            o.arena_sel = arenaSel;
            o.arena_top = arenaTop;
            o.map_next = PROPS ? mapNext : 1u;
            o.seg_next = segNext;
            o.heap_size = heapSize;
            o.n_gc = n_gc;
            o.out_off = off;
            o.n_segs = nseg;
            o.text_off = toff;
            o.max_lb = max_lb;
            o.cu_n = 0;
            o.mode = res_mode;  // row-vectorised engine: 4 on k_solo, 5 on k_rows
            o.spill_why = 0;
        }
#if defined(MTE_PROFILE) && !defined(MTE_CPU)
        if (simd::lane0()) {
            static constexpr u32 map[RP_N] = {PF_TOTAL, PF_FETCH, PF_APPLY, PF_RESOLVE, PF_INSERT_SLOT, PF_SPLIT,
                                              PF_RANGE, PF_ZAMBONI, PF_SCOUR, PF_HEAP, PF_FIND_SEG, PF_PACK,
                                              PF_LRU, PF_OPS, PN_RESOLVE, PN_SCOUR, PN_SCOUR_CHANGED, PN_PACK,
                                              PN_POP, PN_SPLIT_BLK, PN_DIRTY, PF_ALLOC, PF_OP_INS, PF_OP_REM,
                                              PF_ZAM_MSN, PF_ZAM_EDIT, PF_SCOUR_CHAIN, PF_SCOUR_WRITE};
            u64* o2 = p.prof + (u64)doc * PROF_SLOTS;
            for (u32 i = 0; i < RP_N; i++) o2[map[i]] += pf[i];
        }
#endif
    }

    // ---------------------------------------------------------------- the stored state
    // A replay state outside its engine -- a checkpoint (below), or the dump of a k_rows document that
    // continues HBM-resident in the same pass -- is made of three parts, each written down once here:
    //   a row:     its fields in Row::fields order, 64 words (one per lane) each;
    //   registers: LV, HK and HS, 8 registers of 64 words each (RG_STATE_REGS);
    //   scalars:   the ST_* list, scalar i in lane i of one V (lanes below ST_BASE are the user's).
    enum : u32 { ST_BASE = 4, ST_NLB = ST_BASE, ST_HEIGHT, ST_HEAPSIZE, ST_HEAPTOP, ST_MINSEQ, ST_CURSEQ, ST_SEGNEXT,
                 ST_ARENATOP, ST_ARENASEL, ST_MAPNEXT, ST_NOPS, ST_NMSGS, ST_NGC, ST_MAXLB, ST_END };
    static constexpr u32 NF = Row::NF;
    static_assert(3 * RG_LEVELS == RG_STATE_REGS, "LV, HK, HS");
    SD static void put_row(u32* o, const Row& w) {
        u32 i = 0;
        w.for_each_field([&](u32, const V& x) MTE_LI { simd::st(o + 64 * i++, L(), x, simd::mk_all()); });
    }
    // a row stored by an engine with (sp, sw) for (PROPS, WIDE); a field it did not have is 0
    SD static Row get_row(const u32* o, bool sp = PROPS, bool sw = WIDE) {
        Row w;
        u32 i = 0;
        w.for_each_field([&](u32 id, V& x) MTE_LI {
            const bool has = id < Row::FID_PROPS || (id == Row::FID_PROPS ? sp : sw);
            x = has ? simd::ld(o + 64 * i, L(), simd::mk_all()) : simd::splat(0);
            i += has;
        });
        return w;
    }
    SD void put_regs(u32* g) const {
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            simd::st(g + 64 * i, L(), LV.get(i), simd::mk_all());
            simd::st(g + 64 * (8 + i), L(), HK.get(i), simd::mk_all());
            simd::st(g + 64 * (16 + i), L(), HS.get(i), simd::mk_all());
        }
    }
    SD void get_regs(const u32* g) {
#pragma unroll
        for (u32 i = 0; i < 8; i++) {
            LV.set(i, simd::ld(g + 64 * i, L(), simd::mk_all()));
            HK.set(i, simd::ld(g + 64 * (8 + i), L(), simd::mk_all()));
            HS.set(i, simd::ld(g + 64 * (16 + i), L(), simd::mk_all()));
        }
    }
    SD V scalars() const {
        const u32 sv[ST_END - ST_BASE] = {n_lb, height, heapSize, (u32)heapTop, (u32)minSeq, (u32)curSeq, segNext,
                                          arenaTop, arenaSel, PROPS ? mapNext : 1u, ops_n(), msgs_n(), n_gc, max_lb};
        V h = simd::splat(0);
        for (u32 i = ST_BASE; i < ST_END; i++) h = simd::sel(L() == i, sv[i - ST_BASE], h);
        return h;
    }
    SD void set_scalars(V h) {
        auto hw = [&](u32 i) MTE_LI { return simd::readlane(h, i); };
        n_lb = hw(ST_NLB);
        height = hw(ST_HEIGHT);
        heapSize = hw(ST_HEAPSIZE);
        heapTop = (i32)hw(ST_HEAPTOP);
        minSeq = (i32)hw(ST_MINSEQ);
        curSeq = (i32)hw(ST_CURSEQ);
        segNext = hw(ST_SEGNEXT);
        arenaTop = hw(ST_ARENATOP);
        arenaSel = hw(ST_ARENASEL) & 1u;
        mapNext = hw(ST_MAPNEXT);
        set_counts(hw(ST_NOPS), hw(ST_NMSGS));
        n_gc = hw(ST_NGC);
        max_lb = hw(ST_MAXLB);
    }

    // The dump (k_rows' rows_dump -> k_rows_cont, mte_solo.hip): in the document's HBM slot logical row
    // rr at word rr * NF * 64 and the registers at the fixed word DUMP_REGS; in its queue record
    // (ROWS_CONT_WORDS words) doc, slot, op index (lo, hi), then the scalars. The merge arena and the
    // map table stay where they are: the same pass goes on using them.
    static constexpr u32 DUMP_REGS = (u32)RG_ROWS * NF * 64;
    static constexpr u64 DUMP_BYTES = (u64)(DUMP_REGS + RG_STATE_REGS * 64) * 4;
    static_assert(ST_END <= ROWS_CONT_WORDS, "rows_cont record");
    SD void state_dump(u32* base, u32* rec, u32 d, u32 slot, u64 at) const {
        const u32 nrows = (n_lb + 7) >> 3;
        for (u32 rr = 0; rr < nrows; rr++) put_row(base + (u64)rr * NF * 64, rows.ldrow(rr));
        put_regs(base + DUMP_REGS);
        V h = scalars();
        h = simd::sel(L() == 0u, d, h);
        h = simd::sel(L() == 1u, slot, h);
        h = simd::sel(L() == 2u, (u32)at, h);
        h = simd::sel(L() == 3u, (u32)(at >> 32), h);
        simd::st(rec, L(), h, L() < (u32)ST_END);
    }
    // ... into a fresh engine (every row zero); rec: the record, word i in lane i
    SD void state_restore(const u32* base, V rec) {
        set_scalars(rec);
        status = 0;
        const u32 nrows = (n_lb + 7) >> 3;
        for (u32 rr = 0; rr < nrows && rr < (u32)NR; rr++) rows.strow(rr, get_row(base + (u64)rr * NF * 64));
        rows.drop_row();
        get_regs(base + DUMP_REGS);
    }

    // ---------------------------------------------------------------- checkpoints (incremental replay)
    // Client.applyMsg is incremental (client.ts:805-836): a reader interleaves getText with messages.
    // With Params::ck_out set, a document this engine finishes also leaves its whole replay state in
    // its checkpoint region (DocCfg::ck_out_off, ck_cap words); a later pass over a log that extends
    // this one (the host checks the prefix, engine_run.cpp ck_match) starts from that state at op
    // ck_at instead of op 0. The state is the engine's own: rows, interior levels, heap, scalars, the
    // live merge-arena semispace and the property maps -- nothing the replay does depends on where it
    // started, so the continued replay is the full one, op for op.
    // Region (words): header [0, CK_HDR), rows (NF fields of 64 words each, row by row), LV / HK / HS
    // (8 registers each), the arena semispace's [0, arenaTop) units, the map records [0, mapNext).
    static constexpr u32 CK_MAGIC = 0x434B5031u, CK_HDR = CK_HDR_WORDS;
    // header words: the ST_* scalars at their own indices, around them
    enum : u32 { CK_VALID, CK_AT_LO, CK_AT_HI, CK_FLAGS, CK_MW = ST_END, CK_N };
    static_assert(CK_FLAGS < ST_BASE && CK_N <= CK_HDR, "checkpoint header");
    // words a checkpoint of a document with these capacities can take (the host sizes regions by it)
    SD static u64 ck_words(u32 arena_cap, u32 map_cap, u32 map_words) { return ck_region_words(arena_cap, map_cap, map_words); }
    SD void ckpt_save(u64 at) {
        const DocCfg& c = p.docs[doc];
        if (!p.ck_out || !c.ck_cap || status || !rows.rows_whole(n_lb)) return;
        fence_arena();
        u32* base = p.ck_out + c.ck_out_off;
        const u32 nrows = (n_lb + 7) >> 3;
        const u64 rows_end = CK_HDR + (u64)nrows * NF * 64, regs_end = rows_end + RG_STATE_REGS * 64;
        const u64 ar_end = regs_end + ((u64)arenaTop + 1) / 2;
        const u64 end = ar_end + (PROPS ? (u64)mapNext * mw : 0);
        if (end > c.ck_cap) return;  // (the region stays invalid: the next pass replays from op 0)
        const V Lv = L();
        for (u32 rr = 0; rr < nrows; rr++) put_row(base + CK_HDR + (u64)rr * NF * 64, rows.ldrow(rr));
        put_regs(base + rows_end);
        copy_text(0, ARENA_BIT, arenaTop, reinterpret_cast<u16*>(base + regs_end));
        if constexpr (PROPS)
            for (u64 q = 0; q < (u64)mapNext * mw; q += 64) {
                const V i = Lv + (u32)q;
                const B m = i < (u32)((u64)mapNext * mw);
                simd::st(base + ar_end, i, simd::ld(maps, i, m), m);
            }
        const u32 flags = (PROPS ? 1u : 0u) | (WIDE ? 2u : 0u);
        V h = scalars();
        h = simd::sel(Lv == (u32)CK_AT_LO, (u32)at, h);
        h = simd::sel(Lv == (u32)CK_AT_HI, (u32)(at >> 32), h);
        h = simd::sel(Lv == (u32)CK_FLAGS, flags, h);
        h = simd::sel(Lv == (u32)CK_MW, PROPS ? mw : 0u, h);
        simd::st(base, Lv, h, Lv < (u32)CK_N);
        // the valid word last, after every other word of the region is out
        simd::wave_fence();
        simd::st(base, Lv, simd::splat(CK_MAGIC), Lv == 0u);
    }
    // Continue from the checkpoint of the previous pass (DocCfg::ck_at ops in, region ck_in_off of
    // Params::ck_in): returns the op to go on from, or i0 (state untouched: replay from the start)
    // when there is none or it does not fit this engine.
    SD u64 ckpt_resume(u64 i0) {
        const DocCfg& c = p.docs[doc];
        if (!p.ck_in || !c.ck_at || status) return i0;
        const u32* base = p.ck_in + c.ck_in_off;
        const V Lv = L();
        const V h = simd::ld(base, Lv, Lv < (u32)CK_N);
        auto hw = [&](u32 i) MTE_LI { return simd::readlane(h, i); };
        const u64 at = (u64)hw(CK_AT_LO) | ((u64)hw(CK_AT_HI) << 32);
        const u32 flags = hw(CK_FLAGS), nlb = hw(ST_NLB);
        const bool cprops = flags & 1u, cwide = (flags & 2u) != 0;
        // (a lean checkpoint continues on a PROPS / WIDE engine -- no maps, no high removers -- not the
        // other way round; a map table narrower than the records written is refused too)
        if (hw(CK_VALID) != CK_MAGIC || at != c.ck_at || (cprops && !PROPS) || (cwide && !WIDE) || nlb == 0 ||
            nlb > NBLK || hw(ST_HEIGHT) > RG_LEVELS + 1 || hw(ST_ARENATOP) > arena_cap || hw(ST_SEGNEXT) > seg_cap ||
            (cprops && (hw(CK_MW) != mw || hw(ST_MAPNEXT) > map_cap)))
            return i0;
        const u32 nrows = (nlb + 7) >> 3;
        if constexpr (PAGED) {
            if (!rows.grow_rows(nrows)) {  // the pool is full now: k_rows restarts it or the host re-runs it
                status = REG_HANDOFF;
                return i0;
            }
        }
        const u32 cnf = Row::nf(cprops, cwide);
        for (u32 rr = 0; rr < nrows; rr++) rows.strow(rr, get_row(base + CK_HDR + (u64)rr * cnf * 64, cprops, cwide));
        rows.drop_row();
        const u64 rows_end = CK_HDR + (u64)nrows * cnf * 64, regs_end = rows_end + RG_STATE_REGS * 64;
        get_regs(base + rows_end);
        set_scalars(h);
        // the arena text into this pass's semispace arenaSel (offsets kept: the rows' toff stay valid)
        {
            const u16* src = reinterpret_cast<const u16*>(base + regs_end);
            u16* dst = arena_cur();
            for (u32 b = 0; b < arenaTop; b += 64) {
                const V i = Lv + b;
                const B m = i < arenaTop;
                simd::st(dst, i, simd::ld(src, i, m), m);
            }
        }
        if constexpr (PROPS) {
            if (!cprops) mapNext = 1u;
            const u32* src = base + regs_end + ((u64)arenaTop + 1) / 2;
            const u32 nw = cprops ? mapNext * mw : 0u;
            for (u32 q = 0; q < nw; q += 64) {
                const V i = Lv + q;
                const B m = i < nw;
                simd::st(maps, i, simd::ld(src, i, m), m);
            }
        }
        adirty = true;  // arena and map words written lane-parallel: fence before they are read
        if (simd::lane0()) {  // counters[12] / [13]: documents and op records resumed this pass
            simd::count_add(&p.counters[12], 1u);
            simd::count_add(&p.counters[13], (u32)at);
        }
        return i0 + at;
    }
};

}  // namespace mte
