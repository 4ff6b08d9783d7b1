// matrix_table.hpp — the per-entry / per-slot / per-cell bodies of a matrix's cell table (matrix.hip
// k_mx_table, k_mx_table_resolve, k_mx_lookup). Each is the work of ONE lane and touches the table only
// through the three operations below, so the CPU build (MTE_CPU, tests/native/matrix_main.cpp) runs them one
// entry at a time, in any order, with plain memory operations in their place.
//
// The table is open addressing with linear probing over cap slots (a power of two), key
// (row handle << 32 | col handle); 0 is the empty slot (handle 0 is Handle.unallocated and never stored).
// An insert claims its slot with a 64-bit compare-and-swap on the key and then raises the slot's winner
// word to 1 + its order index with an atomic maximum: whichever lane or wave comes first, the slot ends
// with the highest index inserted under its key, i.e. the entry SharedMatrix applied last. Which slot of a
// chain a key lands in does depend on arrival order; what a lookup of the key finds does not.
// No lane waits for another: every loop here is bounded by cap.
#pragma once
#include "../../include/mte.h"
#include "matrix.h"

namespace mte {
namespace mxt {

#ifndef MTE_CPU
#define MXD __device__ __forceinline__
MXD uint64_t cas64(uint64_t* p, uint64_t expect, uint64_t v) {
    return atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expect, (unsigned long long)v);
}
MXD void max32(uint32_t* p, uint32_t v) { atomicMax(p, v); }
MXD void raise(uint32_t* f) { atomicOr(f, 1u); }
#else
#define MXD inline
MXD uint64_t cas64(uint64_t* p, uint64_t expect, uint64_t v) {
    const uint64_t o = *p;
    if (o == expect) *p = v;
    return o;
}
MXD void max32(uint32_t* p, uint32_t v) {
    if (*p < v) *p = v;
}
MXD void raise(uint32_t* f) { *f |= 1u; }
#endif

MXD uint64_t make_key(uint32_t rh, uint32_t ch) { return (uint64_t)rh << 32 | ch; }
// the first slot of a key's chain (murmur3's 64-bit finalizer)
MXD uint32_t slot_of(uint64_t k, uint32_t cap) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k & (cap - 1u);
}

// The key of entry i, false when the entry stores nothing: a set one of the vectors did not define
// (adjustPosition undefined: a handle of 0), or a cell index outside cell_h.
MXD bool entry_key(const MxTableParams& p, uint32_t i, uint64_t& key) {
    const MxEntry e = p.ent[i];
    uint32_t rh, ch;
    if (e.val & MXE_LOADED) {
        rh = e.a;
        ch = e.b;
    } else {
        if (!p.cell_h || e.a >= p.n_cells) return false;
        rh = p.cell_h[2 * (uint64_t)e.a];
        ch = p.cell_h[2 * (uint64_t)e.a + 1];
    }
    if (!rh || !ch) return false;
    key = make_key(rh, ch);
    return true;
}

// INSERT, lane = entry i < n_ent.
MXD void insert(const MxTableParams& p, uint32_t i) {
    uint64_t key;
    if (!entry_key(p, i, key)) return;
    const MxTable& t = p.t;
    uint32_t s = slot_of(key, t.cap);
    for (uint32_t n = 0; n < t.cap; n++, s = (s + 1u) & (t.cap - 1u)) {
        const uint64_t prev = cas64(t.key + s, 0ull, key);
        if (prev == 0ull || prev == key) {
            max32(t.win + s, i + 1u);
            return;
        }
    }
    raise(p.flag);  // every slot holds another key: the table was sized wrong
}

// RESOLVE, lane = slot s < cap, after every insert (a kernel boundary): the winner's value id, or
// MX_NONE when the cell is gone -- a set whose row or col handle was freed after it (last free seq above
// the set's), a loaded cell whose row or col handle the replay freed at all.
MXD void resolve(const MxTableParams& p, uint32_t s) {
    const MxTable& t = p.t;
    const uint64_t key = t.key[s];
    const uint32_t w = t.win[s];
    uint32_t v = MX_NONE;
    if (key != 0ull && w != 0u && w <= p.n_ent) {
        const MxEntry e = p.ent[w - 1u];
        const uint32_t rh = (uint32_t)(key >> 32), ch = (uint32_t)key;
        const uint32_t fr = rh < p.row_free_n ? p.row_free[rh] : 0u, fc = ch < p.col_free_n ? p.col_free[ch] : 0u;
        const bool gone = (e.val & MXE_LOADED) ? (fr | fc) != 0u : ((int32_t)fr > e.seq || (int32_t)fc > e.seq);
        if (!gone) v = e.val & ~MXE_LOADED;
    }
    t.val[s] = v;
}

// LOOKUP of one cell: getCell's read of the SparseArray2D. A chain that wraps the whole table without an
// empty slot ends the loop: the key is absent.
MXD uint32_t lookup(const MxTable& t, uint32_t rh, uint32_t ch) {
    if (!rh || !ch) return MX_NONE;
    const uint64_t key = make_key(rh, ch);
    uint32_t s = slot_of(key, t.cap);
    for (uint32_t n = 0; n < t.cap; n++, s = (s + 1u) & (t.cap - 1u)) {
        const uint64_t k = t.key[s];
        if (k == key) return t.val[s];
        if (k == 0ull) return MX_NONE;
    }
    return MX_NONE;
}

// ---- the LOOKUP phase, after the walk (a kernel boundary)

// Lane = planned query qi < n_queries: its result record. Every kind fills the counts; a CELL reads its two
// probes' handles and the table; a RECT only learns whether it lies inside the matrix.
MXD void finish_query(const MxParams& p, uint32_t qi) {
    const MxQuery Q = p.queries[qi];
    if (Q.out >= p.n_out || Q.grp_r >= p.n_groups || Q.grp_c >= p.n_groups) return;
    MxResult r{};
    r.status = MTE_MX_OK;
    r.row_count = p.totals[Q.grp_r];
    r.col_count = p.totals[Q.grp_c];
    r.value = MX_NONE;
    if (Q.kind == MTE_MQ_CELL) {
        if (Q.row >= r.row_count || Q.col >= r.col_count) {
            r.status = MTE_MX_OUT_OF_RANGE;
        } else if (Q.table < p.n_tables) {
            r.row_handle = p.probe_h[Q.pr];
            r.col_handle = p.probe_h[Q.pc];
            r.value = lookup(p.tables[Q.table], r.row_handle, r.col_handle);
        }
    } else if (Q.kind == MTE_MQ_RECT) {
        r.val_off = Q.val_off;
        if (Q.n_rows && Q.n_cols &&
            ((uint64_t)Q.row + Q.n_rows > r.row_count || (uint64_t)Q.col + Q.n_cols > r.col_count))
            r.status = MTE_MX_OUT_OF_RANGE;
    }
    p.out[Q.out] = r;
}

// Lane = id g < vals_n of the call's vals: the rect that owns it (the last whose val_off is at or below g),
// then cell (g - val_off) of it, row-major: consecutive lanes take consecutive cols of one row. A rect not
// wholly inside the matrix is all MX_NONE.
MXD void rect_cell(const MxParams& p, uint64_t g) {
    if (g >= p.vals_n || !p.n_rects) return;
    uint32_t lo = 0, hi = p.n_rects;  // rects[lo].val_off <= g < rects[hi].val_off
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (p.rects[mid].val_off <= g) lo = mid;
        else hi = mid;
    }
    const MxRect R = p.rects[lo];
    const uint64_t local = g - R.val_off;
    uint32_t v = MX_NONE;
    if (R.val_off <= g && local < (uint64_t)R.n_rows * R.n_cols && R.grp_r < p.n_groups && R.grp_c < p.n_groups &&
        R.table < p.n_tables && (uint64_t)R.row + R.n_rows <= p.totals[R.grp_r] &&
        (uint64_t)R.col + R.n_cols <= p.totals[R.grp_c]) {
        const uint32_t rr = (uint32_t)local / R.n_cols, cc = (uint32_t)local % R.n_cols;
        if (R.rh + rr < p.handle_n && R.ch + cc < p.handle_n) v = lookup(p.tables[R.table], p.handle[R.rh + rr], p.handle[R.ch + cc]);
    }
    p.vals[g] = v;
}

}  // namespace mxt
}  // namespace mte
