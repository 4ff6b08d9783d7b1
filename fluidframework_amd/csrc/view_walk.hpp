// view_walk.hpp — the two wave programs of the view queries (view.hip), written over wave_simd.hpp's
// whole-wave values like reg_engine.hpp: all control flow is scalar, so the same source is the HIP
// kernels' body and, with MTE_CPU, the program tests/native/view_main.cpp checks against a scalar walk.
//
//   walk_group: one wave streams one document's rows once in one view (client, ref_seq), 64 rows per
//               step (lane = row), and resolves the group's ascending probes on the way.
//   copy_job:   one wave copies the units of one TEXT query, row by row (lane = unit).
//
// The view length of a row is nodeLength (mergeTree.ts:1659-1699), the predicate of engine.hpp's
// vis_len over the output pool's rows.
#pragma once
#include "view.h"
#include "wave_simd.hpp"

namespace mte {
namespace view {
using namespace simd;

struct V4 {
    V x, y, z, w;
};
// One 16-byte row per lane (rows: 4 words each, 16-byte aligned).
#ifndef MTE_CPU
SD V4 ld4(const u32* rows, V row, B m) {
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (lane_of(m)) q = reinterpret_cast<const uint4*>(rows)[row.x];
    return {V{q.x}, V{q.y}, V{q.z}, V{q.w}};
}
#else
SD V4 ld4(const u32* rows, V row, B m) {
    const V i = row * 4u;
    return {ld(rows, i, m), ld(rows, i + 1u, m), ld(rows, i + 2u, m), ld(rows, i + 3u, m)};
}
#endif

struct RowLens {
    V view;   // the row's length in the view
    V obs;    // ... in the observer's view (getPosition, mergeTree.ts:1586-1603)
    V tview;  // ... in the view when it is a text row, else 0
    V meta;   // vis.w
};

// Rows row0 + row of the pool, lanes outside `in` counting 0 everywhere.
SD RowLens row_lens(const ViewParams& p, u32 row0, V row, B in, u32 C, i32 R, bool local) {
    const V4 q = ld4(p.out_vis + (u64)row0 * 4, row, in);
    const B removed = (q.w & VW_REMOVED) != 0u;
    RowLens r;
    r.meta = q.w;
    r.obs = sel(removed, 0u, q.x);
    if (local) {
        r.view = r.obs;
    } else {
        const B ins = ((q.w & 0xffu) == C) | sle(q.y, R);
        B hid = (bfe(q.w, 8, 8) == C) | sle(q.z, R);
        const u64* ow = C < 64 ? p.out_ovl : C < 128 ? p.out_ovl2 : nullptr;
        if (ow) {  // C among the overlapping removers: bit C & 63 of the row's word
            const V w = ld(reinterpret_cast<const u32*>(ow + row0), row * 2u + ((C & 63u) >> 5), in & removed);
            hid = hid | (((w >> (C & 31u)) & 1u) != 0u);
        }
        r.view = sel(andn(ins, hid & removed), q.x, 0u);
    }
    r.tview = sel((q.w & (VW_MARKER | VW_PERM)) == 0u, r.view, 0u);
    return r;
}

SD void put_rec(ViewProbeRec* o, u32 row, u32 offset, u32 length, u32 cur_pos, u32 flags, u32 tunits) {
    if (lane0()) *o = ViewProbeRec{row, offset, length, cur_pos, flags, tunits, 0u, 0u};
}

SD void walk_group(const ViewParams& p, u32 g) {
    const ViewGroup G = p.groups[g];
    const bool local = (G.flags & VG_LOCAL) != 0, need_total = (G.flags & VG_TOTAL) != 0;
    const V lane = lanes();
    u32 pi = G.p0;
    u32 vbase = 0, obase = 0, tbase = 0;  // view / observer / view-text units before this step's rows
    for (u32 base = 0; base < G.n_rows && (pi < G.p1 || need_total); base += 64) {
        const V row = lane + base;
        const RowLens L = row_lens(p, G.row0, row, row < G.n_rows, G.client, G.ref_seq, local);
        const V sv = scan_incl(L.view), so = scan_incl(L.obs), st = scan_incl(L.tview);
        const u32 step = readlane(sv, 63);
        const V end = sv + vbase;
        while (pi < G.p1) {
            const u32 pos = p.probe_pos[pi];  // >= vbase: the probes ascend
            if (pos - vbase >= step) break;
            // the first row whose cumulative end exceeds pos (rows of length 0 never do first)
            const u32 l = (u32)__builtin_ctzll(ballot(end > pos));
            const u32 len = readlane(L.view, l), meta = readlane(L.meta, l);
            const u32 off = pos - (vbase + readlane(sv, l) - len);
            const u32 tun = tbase + readlane(st, l) - readlane(L.tview, l) + ((meta & (VW_MARKER | VW_PERM)) ? 0u : off);
            put_rec(p.rec + pi, base + l, off, len, obase + readlane(so, l) - readlane(L.obs, l),
                    (meta & VW_REMOVED) ? VR_REMOVED : 0u, tun);
            pi++;
        }
        vbase += step;
        obase += readlane(so, 63);
        tbase += readlane(st, 63);
    }
    // probes left after the last row: at or past the view's length
    for (; pi < G.p1; pi++) put_rec(p.rec + pi, G.n_rows, 0u, vbase, obase, VR_PAST_END, tbase);
    if (lane0()) p.totals[g] = vbase;
}

SD void copy_job(const ViewParams& p, u32 j) {
    const ViewCopyJob J = p.jobs[j];
    const bool local = (J.flags & VG_LOCAL) != 0;
    const V lane = lanes();
    u32 remaining = J.n_units;
    u64 dst = J.dst_off;
    if (dst > p.text_out_units || remaining > p.text_out_units - dst) return;
    const u32* aux = p.out_aux + (u64)J.row0 * 4;
    for (u32 base = J.start_row; base < J.n_rows && remaining; base += 64) {
        const V row = lane + base;
        const B in = row < J.n_rows;
        const RowLens L = row_lens(p, J.row0, row, in, J.client, J.ref_seq, local);
        const V toff = ld(aux, row * 4u + 1u, in);
        const V skip = sel(row == J.start_row, J.start_off, splat(0u));  // the first row starts mid-row
        const V avail = sel(skip < L.tview, L.tview - skip, 0u);
        const V s = scan_incl(avail), before = s - avail;
        const V room = sel(before < remaining, remaining - before, 0u);
        const V cnt = sel(avail < room, avail, room);
        for (u64 todo = ballot(cnt != 0u); todo; todo &= todo - 1) {
            const u32 l = (u32)__builtin_ctzll(todo);
            const u32 n = readlane(cnt, l);
            const u64 src = J.src_base + readlane(toff, l) + readlane(skip, l);
            if (src > p.text_units || n > p.text_units - src) continue;
            const uint16_t* from = p.out_text + src;
            uint16_t* to = p.text_out + dst + readlane(before, l);
            for (u32 u = 0; u < n; u += 64) {  // a long row: the whole wave, 64 units a turn
                const V i = lane + u;
                const B m = i < n;
                st(to, i, ld(from, i, m), m);
            }
        }
        const u32 tot = readlane(s, 63), done = tot < remaining ? tot : remaining;
        remaining -= done;
        dst += done;
    }
}

}  // namespace view
}  // namespace mte
