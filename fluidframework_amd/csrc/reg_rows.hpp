// reg_rows.hpp — the slot rows of the row engine (reg_engine.hpp): where they live and how they move.
//
// A row is 64 slots = 64 lanes of eight to ten fields (Row). The engine sees ONE interface, RowStore:
// the page table of a PAGED engine, the pool operations, the slot accessors and the one-row register
// cache. Underneath are two backends side by side, as in wave_simd.hpp: RowMem on the device keeps the
// rows in LDS at the byte offsets of a RowsLds (uint4 vis and aux arrays, one ds_read_b128 per lane
// and array), RowMem under MTE_CPU keeps them in plain arrays of its own (test infrastructure only).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "engine_types.hpp"
#include "wave_simd.hpp"

namespace mte {

constexpr u32 RG_ROWS = 32;               // slot rows
constexpr u32 RG_BLOCKS = RG_ROWS * 8;    // leaf blocks
constexpr u32 ROWS_POOL_WORDS = 3;         // k_rows' pool row mask (RowsGeom): <= 96 rows
constexpr u32 ROWS_WAIT_TRIES = 20000;     // a wave finding the pool full retries this often (s_sleep 8)
static_assert(RG_BLOCKS <= SOLO_POOL, "the rows live in the SoloPlan's slot arrays");
static_assert(RG_ROWS <= CK_MAX_ROWS, "checkpoint regions hold the whole row plan");

// the extra slot fields of a PROPS engine's rows (the property map id) and of a WIDE one's (removers
// 32..63); absent otherwise: the lean rows stay eight registers
template <bool P, bool W>
struct RowProps {};
template <>
struct RowProps<true, false> {
    simd::V props;
};
template <>
struct RowProps<false, true> {
    simd::V rm2;
};
template <>
struct RowProps<true, true> {
    simd::V props, rm2;
};
// One row of slots: vis = (len, seq, rseq, meta), aux = (cap, toff, rm, sid). A live segment has
// rm 0, so nodeLength's removal test is one bit test of rm (no separate overlap-set lookup).
template <bool PROPS, bool WIDE>
struct Row : RowProps<PROPS, WIDE> {
    simd::V len, seq, rseq, meta, cap, toff, rm, sid;
    // fields of a row with / without the property map id and the removers 32..63
    static constexpr u32 nf(bool props, bool wide) { return 8 + (props ? 1u : 0u) + (wide ? 1u : 0u); }
    static constexpr u32 NF = nf(PROPS, WIDE);
    static_assert(NF <= ROW_FIELDS_MAX, "state regions are sized by ROW_FIELDS_MAX");
    enum : u32 { FID_PROPS = 8, FID_RM2 = 9 };
    // THE list of a row's fields, in the order every stored form of a row keeps them (checkpoints,
    // k_rows' state dump): f(field id, field). Ids 0..7 are vis.xyzw, aux.xyzw (ldf / stf's aux * 4 + c).
    template <class W, class F>
    SD static void fields(W& w, F f) {
        f(0u, w.len), f(1u, w.seq), f(2u, w.rseq), f(3u, w.meta);
        f(4u, w.cap), f(5u, w.toff), f(6u, w.rm), f(7u, w.sid);
        if constexpr (PROPS) f((u32)FID_PROPS, w.props);
        if constexpr (WIDE) f((u32)FID_RM2, w.rm2);
    }
    template <class F>
    SD void for_each_field(F f) { fields(*this, f); }
    template <class F>
    SD void for_each_field(F f) const { fields(*this, f); }
};

// LDS geometry of k_rows: 32 B per slot (vis + aux), +4 with the property map ids (PROPS), +4 with
// the removers 32..63 (WIDE). The pool (8 / 12 waves): vis array, aux array, [props array], [rm2
// array], row mask. Fixed quarters (4 waves): per wave its rows' vis, aux, [props] and [rm2] arrays.
template <bool PROPS, bool WIDE>
struct RowsGeom {
    static constexpr u32 SLOT = 32 + (PROPS ? 4 : 0) + (WIDE ? 4 : 0);  // LDS bytes per slot
    static constexpr u32 POOL = (LDS_BYTES - ROWS_POOL_WORDS * 4) / (64 * SLOT);  // 79, 71 or 63 rows
    static constexpr u32 MASK = POOL * 64 * SLOT;
    static constexpr u32 LDS = MASK + ROWS_POOL_WORDS * 4;
    static constexpr u32 FIXED_NR = LDS_BYTES / 4 / (64 * SLOT);  // 20, 17 or 16 rows per wave
    static constexpr u32 FIXED_WAVE = FIXED_NR * 64 * SLOT;
    static constexpr u32 FIXED_LDS = 4 * FIXED_WAVE;
    static constexpr u32 CONT_LDS = RG_ROWS * 64 * SLOT;  // k_rows_cont: the whole row plan, once
    static_assert(LDS <= LDS_BYTES && FIXED_LDS <= LDS_BYTES && POOL <= 32 * ROWS_POOL_WORDS, "k_rows LDS plan");
};
// Where one engine's rows are in the dynamic LDS (byte offsets) and the DocRes::mode of a document it
// finishes (4: k_solo, 5: k_rows). One named constructor per user; the CPU backend keeps the mode only.
struct RowsLds {
    u32 vis, aux, props, rm2, mask, mode;
    // n rows' arrays one after the other from byte `at`: vis, aux, [props], [rm2]
    template <bool PROPS, bool WIDE>
    static constexpr RowsLds packed(u32 at, u32 n, u32 mask_at = 0) {
        const u32 prp = at + 2 * n * 64 * 16;
        return {at, at + n * 64 * 16, prp, prp + (PROPS ? n * 64 * 4 : 0), mask_at, 5};
    }
    // k_solo: the SoloPlan's slot arrays, so the LDS engine finds the rows in place after a handoff
    static constexpr RowsLds solo_lean() { return {(u32)offsetof(SoloPlan, vis), (u32)offsetof(SoloPlan, aux), 0, 0, 0, 4}; }
    // ... FULL (PROPS + WIDE): the map ids and the high removers in arrays past the rows' slots in the
    // SoloPlan's aux array (blocks RG_BLOCKS.., unused until a handoff has read them)
    static constexpr RowsLds solo_full() {
        static_assert(RG_BLOCKS * 8 * 16 + 2 * RG_BLOCKS * 8 * 4 <= SOLO_POOL * 8 * 16, "props / rm2 arrays in the aux pool");
        const u32 ab = (u32)offsetof(SoloPlan, aux);
        return {(u32)offsetof(SoloPlan, vis), ab, ab + RG_BLOCKS * 8 * 16, ab + RG_BLOCKS * 8 * 16 + RG_BLOCKS * 8 * 4, 0, 4};
    }
    // k_rows at 4 waves: wave w's fixed quarter
    template <bool PROPS, bool WIDE>
    static constexpr RowsLds rows_fixed(u32 w) {
        typedef RowsGeom<PROPS, WIDE> G;
        return packed<PROPS, WIDE>(w * G::FIXED_WAVE, G::FIXED_NR, G::MASK);
    }
    // k_rows at 8 / 12 waves: the CU's pool and its row mask
    template <bool PROPS, bool WIDE>
    static constexpr RowsLds rows_pool() {
        typedef RowsGeom<PROPS, WIDE> G;
        return packed<PROPS, WIDE>(0, G::POOL, G::MASK);
    }
    // k_rows_cont: RG_ROWS rows from the start of its own LDS
    template <bool PROPS, bool WIDE>
    static constexpr RowsLds rows_cont() { return packed<PROPS, WIDE>(0, RG_ROWS); }
};

// What both backends build on: the page table, the backend's own data (Place: the LDS offsets, or the
// CPU arrays) and the one-row register cache (RowStore::row), which every function that moves blocks
// must drop. Performance note, not a correctness rule: the compiler allocates the engine's registers
// in member order and by inlining depth. With the cache ahead of `at`, k_rows<12, PROPS> came out 64 B
// larger; with mv_slots / zero_slots dropping the cache through a wrapper, lean k_solo 8 B larger (two
// more instructions in its slot move). Neither was timed: time C3 and C4 against the parent's build
// before changing either.
// PAGED (k_rows): logical row r of the document lives in pool row ptab[r] of a pool the CU's waves
// share, taken as the document grows and given back as it shrinks or ends. Otherwise row r is slot row r.
template <class Place, bool PAGED, bool PROPS, bool WIDE>
struct RowTable {
    typedef simd::V V;
    typedef simd::B B;
    typedef mte::Row<PROPS, WIDE> Row;
    V ptab = simd::splat(0);  // lane r: pool row of logical row r (PAGED)
    u32 n_rows = 0;           // logical rows taken from the pool (PAGED)
    Place at;                 // where the rows are
    Row cw;                   // the cached row ...
    u32 cr = NONE;            // ... and which one it is
    bool pool_full = false;   // PAGED: the last grow found the pool full (not the logical row limit)
    SD explicit RowTable(const RowsLds& g) : at(g) {}
    SD u32 prow(u32 r) const {
        if constexpr (PAGED) return simd::readlane(ptab, r);
        else return r;
    }
};

#ifndef MTE_CPU
// ------------------------------------------------------------------------------- device backend
extern __shared__ uint4 g_lds_dyn[];

template <bool PAGED, bool PROPS, bool WIDE>
struct RowMem : RowTable<RowsLds, PAGED, PROPS, WIDE> {
    typedef RowTable<RowsLds, PAGED, PROPS, WIDE> T;
    typedef simd::V V;
    typedef simd::B B;
    typedef typename T::Row Row;
    using T::at;
    using T::cr;
    using T::prow;
    using T::ptab;
    SD explicit RowMem(const RowsLds& g) : T(g) {}
    template <class X>
    SD static X* lds(u32 off) { return reinterpret_cast<X*>(reinterpret_cast<unsigned char*>(g_lds_dyn) + off); }
    SD uint4* VISP() const { return lds<uint4>(at.vis); }
    SD uint4* AUXP() const { return lds<uint4>(at.aux); }
    SD u32* PROPP() const { return lds<u32>(at.props); }  // PROPS: the slots' property map ids
    SD u32* RM2P() const { return lds<u32>(at.rm2); }     // WIDE: the slots' removers 32..63
    SD u32* pool_words() const { return lds<u32>(at.mask); }  // PAGED: the pool's row mask (ROWS_POOL_WORDS words)
    SD bool take_row(u32& row) {  // lane 0 claims a free pool row with an LDS atomic or
        u32 got = NONE;
        if (__lane_id() == 0) {
            u32* m = pool_words();
            for (u32 wd = 0; wd < ROWS_POOL_WORDS && got == NONE; wd++) {
                u32 cur = __hip_atomic_load(m + wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                while (~cur) {
                    const u32 bit = 1u << __builtin_ctz(~cur);
                    const u32 old = atomicOr(m + wd, bit);
                    if (!(old & bit)) {
                        got = wd * 32 + (u32)__builtin_ctz(bit);
                        break;
                    }
                    cur = old | bit;
                }
            }
        }
        got = simd::readlane(simd::V{got}, 0);
        row = got;
        return got != NONE;
    }
    // A full pool is usually full for a moment (the other waves' documents shrink and end all the
    // time): wait up to ~4 ms for a row before giving the document up (a bounded wait, so waves
    // that all wait cannot deadlock: they spill; ~0.4 ms still let one C2 document in five steps
    // spill into a 100 ms HBM re-run).
    SD bool claim_row(u32& row) {
        for (u32 t = 0; t < ROWS_WAIT_TRIES; t++) {
            if (take_row(row)) return true;
            __builtin_amdgcn_s_sleep(8);  // ~512 cycles
        }
        return take_row(row);
    }
    SD void give_row(u32 row) {
        if (__lane_id() == 0) atomicAnd(pool_words() + (row >> 5), ~(1u << (row & 31)));
    }
    SD void zero_prow(u32 row) {
        VISP()[row * 64 + __lane_id()] = make_uint4(0, 0, 0, 0);
        AUXP()[row * 64 + __lane_id()] = make_uint4(0, 0, 0, 0);
        if constexpr (PROPS) PROPP()[row * 64 + __lane_id()] = 0u;
        if constexpr (WIDE) RM2P()[row * 64 + __lane_id()] = 0u;
        simd::lds_order();
    }
    // physical slot of logical slot s, per lane (PAGED: a block range can cross pool rows)
    SD u32 pslot(u32 s) const {
        if constexpr (PAGED) return simd::bperm(ptab, simd::V{s >> 6}).x * 64u + (s & 63u);
        else return s;
    }
    SD Row ldrow(u32 r) const {
        const u32 i = prow(r) * 64 + __lane_id();
        const uint4 v = VISP()[i], a = AUXP()[i];
        Row w;
        w.len = V{v.x}, w.seq = V{v.y}, w.rseq = V{v.z}, w.meta = V{v.w};
        w.cap = V{a.x}, w.toff = V{a.y}, w.rm = V{a.z}, w.sid = V{a.w};
        if constexpr (PROPS) w.props = V{PROPP()[i]};
        if constexpr (WIDE) w.rm2 = V{RM2P()[i]};
        return w;
    }
    SD void strow(u32 r, const Row& w) {
        const u32 i = prow(r) * 64 + __lane_id();
        VISP()[i] = make_uint4(w.len.x, w.seq.x, w.rseq.x, w.meta.x);
        AUXP()[i] = make_uint4(w.cap.x, w.toff.x, w.rm.x, w.sid.x);
        if constexpr (PROPS) PROPP()[i] = w.props.x;
        if constexpr (WIDE) RM2P()[i] = w.rm2.x;
        simd::lds_order();
    }
    SD V ldf(u32 r, u32 aux, u32 c) const {  // one field of a row
        const u32* b = reinterpret_cast<const u32*>(aux ? AUXP() : VISP());
        return V{b[(prow(r) * 64 + __lane_id()) * 4 + c]};
    }
    SD void stf(u32 r, u32 aux, u32 c, V x, B m) {
        u32* b = reinterpret_cast<u32*>(aux ? AUXP() : VISP());
        if (simd::lane_of(m)) b[(prow(r) * 64 + __lane_id()) * 4 + c] = x.x;
        simd::lds_order();
    }
    // Overlapping slot move (slot-index memmove: blocks move as whole 8-slot groups), one 64-slot
    // chunk per LDS round trip; the lean engines overlap each chunk's writes with the next chunk's
    // reads (-0.3 % on the lone 10^6-op document, profiles/r05/r05x). (Issuing eight chunks' reads
    // before their writes measured 7 % SLOWER: 4.25 vs 3.93 us/op.)
    SD void mv_slots(u32 dst, u32 src, u32 n) {
        cr = NONE;
        uint4* V4 = VISP();
        uint4* A4 = AUXP();
        const u32 L = __lane_id();
        if constexpr (PAGED) {  // the same chunks, each lane's slots mapped through ptab
            const bool up = dst > src;
            for (u32 c = 0; c < n; c += 64) {
                const i32 i = up ? (i32)(n - c) - 64 + (i32)L : (i32)(c + L);
                const bool ok = i >= 0 && (u32)i < n;
                const u32 ii = ok ? (u32)i : 0u;
                const u32 ps = pslot(src + ii), pd = pslot(dst + ii);
                uint4 v = make_uint4(0, 0, 0, 0), a = v;
                u32 pp = 0, q2 = 0;
                if (ok) {
                    v = V4[ps];
                    a = A4[ps];
                    if constexpr (PROPS) pp = PROPP()[ps];
                    if constexpr (WIDE) q2 = RM2P()[ps];
                }
                simd::lds_order();
                if (ok) {
                    V4[pd] = v;
                    A4[pd] = a;
                    if constexpr (PROPS) PROPP()[pd] = pp;
                    if constexpr (WIDE) RM2P()[pd] = q2;
                }
                simd::lds_order();
            }
            return;
        }
        if constexpr (!PROPS && !WIDE) {
            // two stages: the next chunk's reads go out before this chunk's writes. The ranges never
            // meet: the walk runs away from the destination (down the slots when moving up, up them
            // when moving down), so every read still sees the slots before the move.
            const uint4 z = make_uint4(0, 0, 0, 0);
            if (dst > src) {
                i32 i = (i32)n - 64 + (i32)L;
                uint4 v = z, a = z;
                if (i >= 0) {
                    v = V4[src + (u32)i];
                    a = A4[src + (u32)i];
                }
                for (i32 b = (i32)n - 64; b > -64; b -= 64) {
                    const i32 j = i - 64;
                    uint4 v2 = z, a2 = z;
                    if (b - 64 > -64 && j >= 0) {
                        v2 = V4[src + (u32)j];
                        a2 = A4[src + (u32)j];
                    }
                    simd::lds_order();
                    if (i >= 0) {
                        V4[dst + (u32)i] = v;
                        A4[dst + (u32)i] = a;
                    }
                    simd::lds_order();
                    v = v2;
                    a = a2;
                    i = j;
                }
            } else {
                u32 i = L;
                uint4 v = z, a = z;
                if (i < n) {
                    v = V4[src + i];
                    a = A4[src + i];
                }
                for (u32 b = 0; b < n; b += 64) {
                    const u32 j = i + 64;
                    uint4 v2 = z, a2 = z;
                    if (b + 64 < n && j < n) {
                        v2 = V4[src + j];
                        a2 = A4[src + j];
                    }
                    simd::lds_order();
                    if (i < n) {
                        V4[dst + i] = v;
                        A4[dst + i] = a;
                    }
                    simd::lds_order();
                    v = v2;
                    a = a2;
                    i = j;
                }
            }
            return;
        }
        if (dst > src) {
            for (i32 b = (i32)n - 64; b > -64; b -= 64) {
                const i32 i = b + (i32)L;
                uint4 v = make_uint4(0, 0, 0, 0), a = v;
                u32 pp = 0, q2 = 0;
                if (i >= 0) {
                    v = V4[src + (u32)i];
                    a = A4[src + (u32)i];
                    if constexpr (PROPS) pp = PROPP()[src + (u32)i];
                    if constexpr (WIDE) q2 = RM2P()[src + (u32)i];
                }
                simd::lds_order();
                if (i >= 0) {
                    V4[dst + (u32)i] = v;
                    A4[dst + (u32)i] = a;
                    if constexpr (PROPS) PROPP()[dst + (u32)i] = pp;
                    if constexpr (WIDE) RM2P()[dst + (u32)i] = q2;
                }
                simd::lds_order();
            }
        } else {
            for (u32 b = 0; b < n; b += 64) {
                const u32 i = b + L;
                uint4 v = make_uint4(0, 0, 0, 0), a = v;
                u32 pp = 0, q2 = 0;
                if (i < n) {
                    v = V4[src + i];
                    a = A4[src + i];
                    if constexpr (PROPS) pp = PROPP()[src + i];
                    if constexpr (WIDE) q2 = RM2P()[src + i];
                }
                simd::lds_order();
                if (i < n) {
                    V4[dst + i] = v;
                    A4[dst + i] = a;
                    if constexpr (PROPS) PROPP()[dst + i] = pp;
                    if constexpr (WIDE) RM2P()[dst + i] = q2;
                }
                simd::lds_order();
            }
        }
    }
    SD void zero_slots(u32 s0, u32 n) {
        cr = NONE;
        if constexpr (!PAGED && !PROPS && !WIDE) {
            for (u32 b = __lane_id(); b < n; b += 64) {
                VISP()[s0 + b] = make_uint4(0, 0, 0, 0);
                AUXP()[s0 + b] = make_uint4(0, 0, 0, 0);
            }
            simd::lds_order();
            return;
        }
        for (u32 c = 0; c < n; c += 64) {
            const u32 b = c + __lane_id();
            const u32 ps = pslot(s0 + (b < n ? b : 0u));
            if (b < n) {
                VISP()[ps] = make_uint4(0, 0, 0, 0);
                AUXP()[ps] = make_uint4(0, 0, 0, 0);
                if constexpr (PROPS) PROPP()[ps] = 0u;
                if constexpr (WIDE) RM2P()[ps] = 0u;
            }
        }
        simd::lds_order();
    }
};

#else
// ---------------------------------------------------------------------------------- CPU backend
// One array per field id (Row::fields), RG_ROWS rows of 64 slots; a PAGED engine's pool is these rows
// of its own, handed out in a scattered order so that logical and pool rows differ.
struct RowArrays {
    u32 mem[ROW_FIELDS_MAX][RG_ROWS * 64];
    u64 pool_mask = 0;  // PAGED: pool rows in use
    u32 pool_rows = RG_ROWS, pool_takes = 0;
    explicit RowArrays(const RowsLds&) {}
};
template <bool PAGED, bool PROPS, bool WIDE>
struct RowMem : RowTable<RowArrays, PAGED, PROPS, WIDE> {
    typedef RowTable<RowArrays, PAGED, PROPS, WIDE> T;
    typedef simd::V V;
    typedef simd::B B;
    typedef typename T::Row Row;
    using T::at;
    using T::cr;
    using T::prow;
    explicit RowMem(const RowsLds& g) : T(g) {}
    SD u32 pslot(u32 s) const { return PAGED ? prow(s >> 6) * 64 + (s & 63) : s; }
    SD bool claim_row(u32& row) {  // (nobody else gives rows back: a full pool is not waited for)
        for (u32 t = 0; t < at.pool_rows; t++) {
            const u32 c = (at.pool_takes * 7 + 3 + t) % at.pool_rows;
            if (!((at.pool_mask >> c) & 1)) {
                at.pool_mask |= 1ull << c;
                at.pool_takes++;
                row = c;
                return true;
            }
        }
        return false;
    }
    SD void give_row(u32 row) { at.pool_mask &= ~(1ull << row); }
    SD void zero_prow(u32 row) {
        for (auto& f : at.mem) memset(&f[row * 64], 0, 64 * 4);
    }
    SD Row ldrow(u32 r) const {
        Row w;
        const u32 pr = prow(r);
        w.for_each_field([&](u32 id, V& x) { memcpy(x.x, &at.mem[id][pr * 64], 64 * 4); });
        return w;
    }
    SD void strow(u32 r, const Row& w) {
        const u32 pr = prow(r);
        w.for_each_field([&](u32 id, const V& x) { memcpy(&at.mem[id][pr * 64], x.x, 64 * 4); });
    }
    SD V ldf(u32 r, u32 aux, u32 c) const {  // one field of a row
        V x;
        memcpy(x.x, &at.mem[aux * 4 + c][prow(r) * 64], 64 * 4);
        return x;
    }
    SD void stf(u32 r, u32 aux, u32 c, V x, B m) {
        const u32 pr = prow(r);
        for (u32 l = 0; l < 64; l++)
            if ((m.m >> l) & 1) at.mem[aux * 4 + c][pr * 64 + l] = x.x[l];
    }
    // slot-index memmove (blocks move as whole 8-slot groups)
    SD void mv_slots(u32 dst, u32 src, u32 n) {
        cr = NONE;
        for (auto& f : at.mem) {
            if (!PAGED) {
                memmove(&f[dst], &f[src], (size_t)n * 4);
                continue;
            }
            for (u32 t = 0; t < n; t++) {  // slot by slot in the memmove's safe direction
                const u32 i = dst > src ? n - 1 - t : t;
                f[pslot(dst + i)] = f[pslot(src + i)];
            }
        }
    }
    SD void zero_slots(u32 s0, u32 n) {
        cr = NONE;
        for (auto& f : at.mem)
            for (u32 i = 0; i < n; i++) f[pslot(s0 + i)] = 0;
    }
};
#endif

// The row store of one engine: NR logical rows at most.
template <int NR, bool PAGED, bool PROPS, bool WIDE>
struct RowStore : RowMem<PAGED, PROPS, WIDE> {
    typedef RowMem<PAGED, PROPS, WIDE> M;
    typedef typename M::Row Row;
    using M::cr;
    using M::cw;
    using M::ldrow;
    using M::n_rows;
    using M::pool_full;
    using M::ptab;
    using M::strow;
    SD explicit RowStore(const RowsLds& g) : M(g) {}
    // The row an op is working on stays in registers between its steps (resolve -> split -> insert ->
    // LRU; heap pop -> scour -> needsScour): row(r) reads the rows only when r is not the cached row,
    // putrow writes through. Anything that moves blocks (mv_slots / zero_slots) drops the cache.
    SD Row row(u32 r) {
        if (r != cr) {
            cw = ldrow(r);
            cr = r;
        }
        return cw;
    }
    SD void putrow(u32 r, const Row& w) {
        strow(r, w);
        cw = w;
        cr = r;
    }
    // the cached row itself, for edits in place (no working copy of its eight registers); pair with
    // writeback(r) before anything else touches the cache
    SD Row& rowref(u32 r) {
        if (r != cr) {
            cw = ldrow(r);
            cr = r;
        }
        return cw;
    }
    SD void writeback(u32 r) { strow(r, cw); }
    SD void cache(u32 r, const Row& w) {  // w is row r as stored
        cw = w;
        cr = r;
    }
    SD void drop_row() { cr = NONE; }  // after rows were written behind the cache's back (strow)

    // PAGED: an empty table (the rows of an earlier document were given back with release_rows)
    SD void reset_rows() {
        n_rows = 0;
        ptab = simd::splat(0);
    }
    // PAGED: logical rows [n_rows, need) from the pool, zeroed (rows past the last block stay zero)
    SD bool grow_rows(u32 need) {
        while (n_rows < need) {
            u32 row;
            if (n_rows >= (u32)NR) return false;
            if (!M::claim_row(row)) {
                pool_full = true;
                return false;
            }
            M::zero_prow(row);
            ptab = simd::writelane(ptab, n_rows, row);
            n_rows++;
        }
        return true;
    }
    SD void shrink_rows(u32 keep) {
        cr = NONE;
        while (n_rows > keep) M::give_row(M::prow(--n_rows));
    }
    SD void release_rows() {
        if constexpr (PAGED) shrink_rows(0);
    }
    // every row of a state of n_lb leaf blocks is held (a PAGED engine whose first row the pool never
    // gave has none)
    SD bool rows_whole(u32 n_lb) const {
        if constexpr (PAGED) return n_rows * 8 >= n_lb;
        else return true;
    }
};

}  // namespace mte
