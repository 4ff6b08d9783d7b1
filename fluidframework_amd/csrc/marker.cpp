// marker.cpp — mte_markers (include/mte.h): the device side of the marker queries. marker_plan.hpp plans a
// call and turns the walks' records into results; this unit keeps what is derived from the loaded batch
// (the key ids, the labels' bitmaps over the value ids, the documents' annotate flags) and the device
// buffers (grown as calls need them, reused across calls), uploads the plan, launches the phases
// (marker.hip) on the engine's stream and downloads the records, the pieces and the text. Nothing here
// touches the whole-pool download (ensure_download): the queries read the output pool where the pass
// left it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mte.h"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "marker.h"
#include "marker_plan.hpp"

static_assert(sizeof(mte_mark_q) == 20 && sizeof(mte_mark_r) == 32 && sizeof(mte_mark_piece) == 24, "mte.h marker records");

namespace {
// room for n, half as much again when the buffer has to grow (a caller's batches vary a little)
template <class T>
hipError_t grow(DevBuf<T>& d, size_t n) {
    return (d.p && d.n >= n) ? hipSuccess : d.alloc(n + n / 2);
}
template <class T>
int put(mte_engine* e, DevBuf<T>& d, const std::vector<T>& h, hipStream_t s) {
    HIP_TRY(e, grow(d, h.size()));
    if (!h.empty()) HIP_TRY(e, hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return MTE_OK;
}

mte::markplan::Tables tables_of(const HostBatch& hb) {
    return mte::markplan::Tables{(uint32_t)hb.key_offsets.size() - 1, hb.key_offsets.data(), hb.key_text.data(),
                                 (uint32_t)hb.val_offsets.size() - 1, hb.val_offsets.data(), hb.val_text.data()};
}

void ensure_keys(mte_engine* e) {
    mte_engine::MkCache& c = e->mk;
    if (c.keys_known) return;
    const mte::markplan::Keys k = mte::markplan::find_keys(tables_of(e->hb));
    c.key_tile = k.tile;
    c.key_bold = k.bold;
    c.key_under = k.under;
    mte::markplan::propsets_with_key(e->hb.propsets.data(), (uint32_t)e->hb.propsets.size(), e->hb.prop_keys.data(), k.tile,
                                     c.set_has_tile);
    c.doc_annot.assign(e->res.size(), 0);
    c.keys_known = true;
}

// The hazard flag of document d, derived from its op records at the first TILE query and kept.
int doc_annotates(mte_engine* e, uint32_t d, bool& yes) {
    mte_engine::MkCache& c = e->mk;
    yes = false;
    if (c.key_tile == MK_NONE) return MTE_OK;  // no set of the batch names the key
    if (c.doc_annot.size() != e->res.size()) c.doc_annot.assign(e->res.size(), 0);
    if (!c.doc_annot[d]) {
        if (int rc = ensure_host_ops(e)) return rc;
        const HostBatch& hb = e->hb;
        bool a = false;
        if ((size_t)d + 1 < hb.doc_op_offsets.size())
            a = mte::markplan::doc_annotates(hb.ops.data(), hb.doc_op_offsets[d], std::min<uint64_t>(hb.doc_op_offsets[d + 1], hb.ops.size()),
                                             c.set_has_tile);
        c.doc_annot[d] = a ? 2 : 1;
    }
    yes = c.doc_annot[d] == 2;
    return MTE_OK;
}
}  // namespace

void mk_drop_cache(mte_engine* e) {
    const uint64_t built = e->mk.bitmaps_built;
    e->mk = mte_engine::MkCache{};
    e->mk.bitmaps_built = built;
}

int mte_markers(mte_engine* e, const mte_mark_q* q, size_t n, const char* const* labels, size_t n_labels, mte_mark_r* out,
                mte_mark_piece* pieces, size_t pieces_cap, size_t* n_pieces, uint16_t* text, size_t text_cap, size_t* text_len) {
    if (!e || (n && (!q || !out)) || (n_labels && !labels)) return MTE_E_ARG;
    for (size_t l = 0; l < n_labels; l++)
        if (!labels[l]) return MTE_E_ARG;
    if (!e->replayed) return set_err(e, MTE_E_STATE, "mte_markers before mte_replay");
    if (n >= (1u << 30) || n_labels >= (1u << 30)) return set_err(e, MTE_E_ARG, "too many queries or labels in one call");
    if (n_pieces) *n_pieces = 0;
    if (text_len) *text_len = 0;
    if (!n) return MTE_OK;
    int rc;
    HIP_TRY(e, hipSetDevice(e->device));
    uint32_t ctr[8];
    if ((rc = read_counters(e, ctr, 8))) return rc;
    const uint64_t rows = std::min<uint64_t>(ctr[1], e->P.out_cap);
    uint64_t units;
    memcpy(&units, ctr + 6, sizeof units);
    units = std::min<uint64_t>(units, e->P.out_text_cap);

    // the call's distinct labels and their bitmaps (built once per load and label)
    ensure_keys(e);
    mte_engine::MkCache& c = e->mk;
    const uint32_t n_vals = (uint32_t)e->val_flags.size();
    const uint32_t bits_words = (uint32_t)(((size_t)e->hb.val_offsets.size() - 1 + 31) / 32);
    std::vector<uint32_t> label_slot(n_labels), bits;
    {
        std::unordered_map<std::string, uint32_t> slot;
        for (size_t l = 0; l < n_labels; l++) {
            const std::string name(labels[l]);
            auto it = slot.find(name);
            if (it == slot.end()) {
                it = slot.emplace(name, (uint32_t)slot.size()).first;
                auto b = c.label_bits.find(name);
                if (b == c.label_bits.end()) {
                    b = c.label_bits.emplace(name, std::vector<uint32_t>()).first;
                    mte::markplan::label_bitmap(tables_of(e->hb), name, b->second);
                    c.bitmaps_built++;
                }
                bits.insert(bits.end(), b->second.begin(), b->second.end());
            }
            label_slot[l] = it->second;
        }
    }

    mte::markplan::Plan pl;
    int annot_rc = MTE_OK;
    mte::markplan::plan_markers(
        q, n, (uint32_t)e->res.size(), label_slot,
        [&](uint32_t d) {
            const DocRes& r = e->res[d];
            mte::markplan::DocInfo i;
            i.ok = r.status == 0 && (uint64_t)r.out_off + r.n_segs <= rows && (uint64_t)r.n_segs * e->map_words < (1ull << 32);
            i.row0 = r.out_off;
            i.n_rows = r.n_segs;
            i.text_off = r.text_off;
            return i;
        },
        [&](uint32_t d) {
            bool yes = false;
            if (int r = doc_annotates(e, d, yes)) annot_rc = r;
            return yes;
        },
        pl);
    if (annot_rc) return annot_rc;

    MarkParams p{};
    p.out_vis = reinterpret_cast<const uint32_t*>(e->d_out_vis.p);
    p.out_aux = reinterpret_cast<const uint32_t*>(e->d_out_aux.p);
    p.out_maps = e->P.out_maps ? e->d_out_maps.p : nullptr;
    p.map_words = e->map_words;
    p.n_vals = std::min<uint32_t>(n_vals, (uint32_t)e->hb.val_offsets.size() - 1);
    p.val_flags = e->d_val_flags.p;
    p.out_text = e->d_out_text.p;
    p.text_units = units;
    p.key_tile = c.key_tile;
    p.key_bold = c.key_bold;
    p.key_under = c.key_under;
    p.bits_words = bits_words;

    // TILE and COUNT
    std::vector<MarkTileRec> rec(pl.probe_pos.size());
    std::vector<MarkCount> count(pl.jobs.size());
    if (!pl.groups.empty() || !pl.jobs.empty()) {
        if ((rc = put(e, e->d_mk_bits, bits, e->stream))) return rc;
        p.label_bits = e->d_mk_bits.p;
    }
    if (!pl.groups.empty()) {
        if ((rc = put(e, e->d_mk_groups, pl.groups, e->stream))) return rc;
        if ((rc = put(e, e->d_mk_pos, pl.probe_pos, e->stream))) return rc;
        HIP_TRY(e, grow(e->d_mk_rec, rec.size()));
        p.groups = e->d_mk_groups.p;
        p.n_groups = (uint32_t)pl.groups.size();
        p.probe_pos = e->d_mk_pos.p;
        p.rec = e->d_mk_rec.p;
        HIP_TRY(e, launch_mark_tile(p, e->stream));
        HIP_TRY(e, hipMemcpyAsync(rec.data(), e->d_mk_rec.p, rec.size() * sizeof(MarkTileRec), hipMemcpyDeviceToHost, e->stream));
    }
    if (!pl.jobs.empty()) {
        if ((rc = put(e, e->d_mk_jobs, pl.jobs, e->stream))) return rc;
        HIP_TRY(e, grow(e->d_mk_count, count.size()));
        p.jobs = e->d_mk_jobs.p;
        p.n_jobs = (uint32_t)pl.jobs.size();
        p.count = e->d_mk_count.p;
        HIP_TRY(e, launch_mark_count(p, e->stream));
        HIP_TRY(e, hipMemcpyAsync(count.data(), e->d_mk_count.p, count.size() * sizeof(MarkCount), hipMemcpyDeviceToHost, e->stream));
    }
    if (!pl.groups.empty() || !pl.jobs.empty()) HIP_TRY(e, hipStreamSynchronize(e->stream));

    uint64_t need_pieces = 0, need_units = 0;
    mte::markplan::layout_jobs(pl, count.data(), need_pieces, need_units);
    mte::markplan::scatter_markers(pl, q, n, rec.data(), out);
    if (n_pieces) *n_pieces = (size_t)need_pieces;
    if (text_len) *text_len = (size_t)need_units;
    if (!need_pieces || !pieces || (need_units && !text)) return MTE_OK;  // a sizing call, or no PARAGRAPHS query with a tile
    if (pieces_cap < need_pieces || text_cap < need_units) return set_err(e, MTE_E_RANGE, "mte_markers: pieces or text buffer too small");

    // WRITE
    if ((rc = put(e, e->d_mk_jobs, pl.jobs, e->stream))) return rc;
    HIP_TRY(e, grow(e->d_mk_pieces, need_pieces));
    HIP_TRY(e, grow(e->d_mk_text, need_units));
    p.jobs = e->d_mk_jobs.p;
    p.pieces = e->d_mk_pieces.p;
    p.n_pieces = need_pieces;
    p.text_out = e->d_mk_text.p;
    p.text_out_units = need_units;
    HIP_TRY(e, launch_mark_write(p, e->stream));
    HIP_TRY(e, hipMemcpyAsync(pieces, e->d_mk_pieces.p, need_pieces * sizeof(mte_mark_piece), hipMemcpyDeviceToHost, e->stream));
    if (need_units)
        HIP_TRY(e, hipMemcpyAsync(text, e->d_mk_text.p, need_units * sizeof(uint16_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return MTE_OK;
}
