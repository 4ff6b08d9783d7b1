// marker_walk.hpp — the wave programs of the marker queries (marker.hip), written over wave_simd.hpp's
// whole-wave values like view_walk.hpp: all control flow is scalar, so the same source is the HIP
// kernels' body and, with MTE_CPU, the program tests/native/marker_main.cpp checks against a scalar
// restatement.
//
//   walk_tiles:      one wave streams one document's rows, 64 per step (lane = row), and resolves the
//                    ascending findTile probes of one (label, direction) from one ballot of the step's
//                    tile rows and one inclusive scan of their local lengths.
//   walk_paragraphs: one wave walks the rows of one getTextAndMarkers range. COUNT (WRITE = false) counts
//                    the pieces and their units, tags included; WRITE walks the same rows again and writes
//                    the piece records and the text the host laid out from the counts.
//
// Everything is the observer's current view: a row's length is its local net length (0 when removed at
// all). The tile predicate is refHasTileLabel (mergeTree.ts:581-597) over the row's map record; the tag
// machine is gatherText's tagsInProgress (textSegment.ts:196-240).
#pragma once
#include "marker.h"
#include "wave_simd.hpp"

namespace mte {
namespace mark {
using namespace simd;

struct Row {
    V len;   // local net length
    V meta;  // vis.w
    V ax;    // aux.x: non-zero = the row has a map record
    V ay;    // aux.y: a text row's offset in the document's text run, a marker's refType word
};

SD Row load_row(const MarkParams& p, u32 row0, V row, B in) {
    Row r;
#ifndef MTE_CPU
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    uint2 a = make_uint2(0u, 0u);
    if (lane_of(in)) {
        q = reinterpret_cast<const uint4*>(p.out_vis)[(u64)row0 + row.x];
        a = *reinterpret_cast<const uint2*>(p.out_aux + ((u64)row0 + row.x) * 4);
    }
    r.meta = V{q.w};
    r.len = V{(q.w & MW_REMOVED) ? 0u : q.x};
    r.ax = V{a.x};
    r.ay = V{a.y};
#else
    const u32 *vis = p.out_vis + (u64)row0 * 4, *aux = p.out_aux + (u64)row0 * 4;
    const V i = row * 4u;
    r.meta = ld(vis, i + 3u, in);
    r.len = sel((r.meta & MW_REMOVED) != 0u, 0u, ld(vis, i, in));
    r.ax = ld(aux, i, in);
    r.ay = ld(aux, i + 1u, in);
#endif
    return r;
}

// The values of keys k1 and k2 (MK_NONE: not asked, or the batch has no such key) in the map records of
// the lanes in m, MK_NONE where the record has no such key. A record is [count, (key, value) ...] in
// map_words words (the narrow record or a wider one); markers and annotated rows are the lanes that read.
SD void map_find2(const MarkParams& p, u32 row0, V row, B m, u32 k1, u32 k2, V& v1, V& v2) {
    v1 = splat(MK_NONE);
    v2 = splat(MK_NONE);
    if (!p.out_maps || !ballot(m) || (k1 == MK_NONE && k2 == MK_NONE)) return;
    const u32* maps = p.out_maps + (u64)row0 * p.map_words;
    const u32 maxp = (p.map_words - 1u) / 2u;
    const V at = row * p.map_words;
    V cnt = ld(maps, at, m);
    cnt = sel(cnt < maxp, cnt, maxp);
    for (u32 i = 0; i < maxp; i++) {
        const B a = m & (cnt > i);
        if (!ballot(a)) break;
        const V k = ld(maps, at + (1u + 2u * i), a), v = ld(maps, at + (2u + 2u * i), a);
        if (k1 != MK_NONE) v1 = sel(a & (k == k1), v, v1);
        if (k2 != MK_NONE) v2 = sel(a & (k == k2), v, v2);
    }
}

// bit v of a label's bitmap ("value v contains the label"), for the lanes in m
SD B val_in_label(const MarkParams& p, const u32* bits, V v, B m) {
    const B ok = m & (v < p.n_vals) & ((v >> 5u) < p.bits_words);
    const V w = ld(bits, v >> 5u, ok);
    return ok & (((w >> (v & 31u)) & 1u) != 0u);
}
// JS truthiness of value v (val_flags bit 0 = falsy)
SD B val_truthy(const MarkParams& p, V v, B m) {
    const B ok = m & (v < p.n_vals);
    return ok & ((ld(p.val_flags, v, ok) & 1u) == 0u);
}

// The rows that are tiles for the label, visible or not: a marker with ReferenceType.Tile and a map whose
// "referenceTileLabels" value contains the label.
SD B tile_rows(const MarkParams& p, u32 row0, V row, B in, const Row& R, const u32* bits) {
    const B cand = in & ((R.meta & MW_MARKER) != 0u) & ((R.ay & 1u) != 0u) & (R.ax != 0u);
    V v, none;
    map_find2(p, row0, row, cand, p.key_tile, MK_NONE, v, none);
    return val_in_label(p, bits, v, cand);
}

SD void put_tile(MarkTileRec* o, u32 row, u32 pos, u32 flags) {
    if (lane0()) *o = MarkTileRec{row, pos, flags, 0u};
}

SD void walk_tiles(const MarkParams& p, u32 g) {
    const MarkGroup G = p.groups[g];
    const u32* bits = p.label_bits + (u64)G.label * p.bits_words;
    const bool after = (G.flags & MG_AFTER) != 0;
    const V lane = lanes();
    u32 pi = G.p0;
    u32 obase = 0;                         // visible units before this step's rows
    u32 last_row = MK_NONE, last_pos = 0;  // BEFORE: the last visible tile of the steps behind
    for (u32 base = 0; base < G.n_rows && pi < G.p1; base += 64) {
        const V row = lane + base;
        const B in = row < G.n_rows;
        const Row R = load_row(p, G.row0, row, in);
        const u64 tb = ballot(andn(tile_rows(p, G.row0, row, in, R, bits), (R.meta & MW_REMOVED) != 0u));
        const V so = scan_incl(R.len);
        const u32 step = readlane(so, 63);
        const V start = so - R.len + obase;
        if (!after) {
            const V end = so + obase;
            while (pi < G.p1) {
                const u32 pos = p.probe_pos[pi];  // >= obase: the probes ascend
                if (pos - obase >= step) break;
                // the containing row is the first whose end exceeds pos; the answer is the highest tile
                // lane at or below it, else the last tile of the steps behind
                const u32 l = (u32)__builtin_ctzll(ballot(end > pos));
                const u64 m = tb & ((2ull << l) - 1ull);
                if (m) {
                    const u32 h = 63u - (u32)__builtin_clzll(m);
                    put_tile(p.rec + pi, base + h, readlane(start, h), MR_FOUND);
                } else {
                    put_tile(p.rec + pi, last_row, last_pos, last_row != MK_NONE ? MR_FOUND : 0u);
                }
                pi++;
            }
            if (tb) {
                const u32 h = 63u - (u32)__builtin_clzll(tb);
                last_row = base + h;
                last_pos = readlane(start, h);
            }
        } else {
            while (pi < G.p1) {
                // the lowest tile lane whose position is at or above the probe; none: no later probe has one
                // in this step either
                const u64 m = tb & ballot(start >= p.probe_pos[pi]);
                if (!m) break;
                const u32 l = (u32)__builtin_ctzll(m);
                put_tile(p.rec + pi, base + l, readlane(start, l), MR_FOUND);
                pi++;
            }
        }
        obase += step;
    }
    if (pi >= G.p1) return;
    // probes left after the last row (obase is the document's length)
    if (!after) {  // at or past the length every row was passed: the last visible tile of the document
        for (; pi < G.p1; pi++) put_tile(p.rec + pi, last_row, last_pos, last_row != MK_NONE ? MR_FOUND : 0u);
        return;
    }
    // backwardSearch at pos == length: the last row is the containing leaf whatever its length, and
    // recordTileStart does not test visibility. That row alone is read (lane 0).
    u32 lflags = 0, lpos = 0;
    if (G.n_rows) {
        const V row = splat(G.n_rows - 1u);
        const B in = lane == 0u;
        const Row R = load_row(p, G.row0, row, in);
        if (ballot(tile_rows(p, G.row0, row, in, R, bits)) & 1ull) {
            lflags = MR_FOUND | ((readlane(R.meta, 0) & MW_REMOVED) ? MR_REMOVED : 0u);
            lpos = obase - readlane(R.len, 0);
        }
    }
    for (; pi < G.p1; pi++) {
        const bool hit = lflags && p.probe_pos[pi] == obase;
        put_tile(p.rec + pi, hit ? G.n_rows - 1u : MK_NONE, hit ? lpos : 0u, hit ? lflags : 0u);
    }
}

// gatherText's tag machine (textSegment.ts:196-240). tagsInProgress has five reachable states:
// 0 [], 1 [b], 2 [u], 3 [u,b], 4 [b,u]; a text row's tag list T is bit 0 = "b" (font-weight truthy),
// bit 1 = "u" (text-decoration truthy). tag_step(state, T) = next state | tag A << 3 | tag B << 6: the row
// prints endTags + beginTags = A then B before its text (1 <b>, 2 <u>, 3 </b>, 4 </u>, 0 nothing).
constexpr u32 TG_OB = 1, TG_OU = 2, TG_CB = 3, TG_CU = 4;
constexpr u64 tg_e(u32 next, u32 a, u32 b) { return (u64)(next | a << 3 | b << 6); }
constexpr u64 tg_row(u64 t0, u64 t1, u64 t2, u64 t3) { return t0 | t1 << 16 | t2 << 32 | t3 << 48; }
constexpr u64 TG_S0 = tg_row(tg_e(0, 0, 0), tg_e(1, TG_OB, 0), tg_e(2, TG_OU, 0), tg_e(3, TG_OB, TG_OU));
constexpr u64 TG_S1 = tg_row(tg_e(0, TG_CB, 0), tg_e(1, 0, 0), tg_e(2, TG_CB, TG_OU), tg_e(4, TG_OU, 0));
constexpr u64 TG_S2 = tg_row(tg_e(0, TG_CU, 0), tg_e(1, TG_CU, TG_OB), tg_e(2, 0, 0), tg_e(3, TG_OB, 0));
constexpr u64 TG_S3 = tg_row(tg_e(0, TG_CU, TG_CB), tg_e(1, TG_CU, 0), tg_e(2, TG_CB, 0), tg_e(3, 0, 0));
constexpr u64 TG_S4 = tg_row(tg_e(0, TG_CB, TG_CU), tg_e(1, TG_CU, 0), tg_e(2, TG_CB, 0), tg_e(4, 0, 0));
SD u32 tag_step(u32 state, u32 T) {
    const u64 r = state == 0 ? TG_S0 : state == 1 ? TG_S1 : state == 2 ? TG_S2 : state == 3 ? TG_S3 : TG_S4;
    return (u32)(r >> (16u * (T & 3u))) & 0xFFFFu;
}
SD u32 tag_len(u32 t) { return t == 0 ? 0u : t <= TG_OU ? 3u : 4u; }
// the units of tag t at o; returns the units written (one lane calls this)
SD u32 put_tag(uint16_t* o, u32 t) {
    if (!t) return 0;
    u32 n = 0;
    o[n++] = '<';
    if (t >= TG_CB) o[n++] = '/';
    o[n++] = (t == TG_OB || t == TG_CB) ? 'b' : 'u';
    o[n++] = '>';
    return n;
}

template <bool WRITE>
SD void walk_paragraphs(const MarkParams& p, u32 j) {
    const MarkJob J = p.jobs[j];
    const u32* bits = p.label_bits + (u64)J.label * p.bits_words;
    if (WRITE) {  // the host laid these out (marker_plan.hpp layout_jobs); nothing is written outside them
        if (!J.n_pieces || J.piece0 > p.n_pieces || J.n_pieces > p.n_pieces - J.piece0) return;
        if (J.dst_off > p.text_out_units || J.n_units > p.text_out_units - J.dst_off) return;
    }
    const V lane = lanes();
    u32 state = 0, pieces = 0, obase = 0;
    u64 total = 0, cur = 0;  // units of the finished pieces / of the piece being gathered
    for (u32 base = 0; base < J.n_rows && obase < J.end; base += 64) {
        const V row = lane + base;
        const B in = row < J.n_rows;
        const Row R = load_row(p, J.row0, row, in);
        const V so = scan_incl(R.len);
        const u32 step = readlane(so, 63);
        const V start = so - R.len + obase, end = so + obase;
        // mapRange's clip of each row to [J.start, J.end): rows of length 0 and rows outside are not visited
        const V lo = sel(start < J.start, J.start, start), hi = sel(end < J.end, end, J.end);
        const B seen = in & (lo < hi);
        const B text = seen & ((R.meta & (MW_MARKER | MW_PERM)) == 0u);
        const u64 tm = ballot(text);
        const u64 km = ballot(seen & tile_rows(p, J.row0, row, in, R, bits));
        V vb, vu;
        map_find2(p, J.row0, row, text & (R.ax != 0u), p.key_bold, p.key_under, vb, vu);
        const V tags = sel(val_truthy(p, vb, text), 1u, splat(0u)) | sel(val_truthy(p, vu, text), 2u, splat(0u));
        const V cnt = sel(text, hi - lo, 0u), skip = lo - start;
        u64 ev = tm | km;
        if (!WRITE && !km && state == 0 && !ballot(tags != 0u)) {  // no tile, no tag, none open: the step's units
            cur += readlane(scan_incl(cnt), 63);
            ev = 0;
        }
        // the step's text and tile rows in order, one at a time: the tag state and the piece boundaries
        // are a chain through them, and WRITE copies row by row anyway
        for (; ev; ev &= ev - 1) {
            const u32 l = (u32)__builtin_ctzll(ev);
            if ((tm >> l) & 1ull) {
                const u32 e = tag_step(state, readlane(tags, l));
                const u32 ta = (e >> 3) & 7u, tb = (e >> 6) & 7u, tl = tag_len(ta) + tag_len(tb);
                const u32 n = readlane(cnt, l);
                if (WRITE) {
                    if (total + cur + tl + n > J.n_units) return;  // (COUNT walked the same rows: never)
                    uint16_t* to = p.text_out + J.dst_off + total + cur;
                    if (tl && lane0()) put_tag(to + put_tag(to, ta), tb);
                    to += tl;
                    const u64 src = J.src_base + readlane(R.ay, l) + readlane(skip, l);
                    // a source range outside the pass's text (the pool's own offsets: never) reads nothing and
                    // writes zeros: the caller never gets what an earlier call left in the buffer
                    const bool inside = src <= p.text_units && n <= p.text_units - src;
                    const uint16_t* from = p.out_text + (inside ? src : 0);
                    for (u32 u = 0; u < n; u += 64) {  // the whole wave, 64 units a turn (lane = unit)
                        const V i = lane + u;
                        const B m = i < n;
                        st(to, i, inside ? ld(from, i, m) : splat(0u), m);
                    }
                }
                cur += tl + n;
                state = e & 7u;
            } else {  // a tile closes the piece: the marker and the text gathered so far; the tags stay open
                const u32 mpos = readlane(start, l);
                if (WRITE && lane0()) p.pieces[J.piece0 + pieces] = mte_mark_piece{base + l, mpos, J.dst_off + total, (u32)cur, 0u};
                total += cur;
                cur = 0;
                pieces++;
                if (WRITE && pieces == J.n_pieces) return;  // the text behind the last tile is dropped
            }
        }
        obase += step;
    }
    if (!WRITE && lane0()) p.count[j] = MarkCount{pieces, 0u, total};
}

}  // namespace mark
}  // namespace mte
