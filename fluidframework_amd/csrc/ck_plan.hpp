// ck_plan.hpp — the host arithmetic of incremental replay (option retain): what the engine keeps of a
// pass's checkpoints, the prefix check that offers them to the next pass, the regions of a pass and the
// block documents' admission to the checkpoint budget. Header-only and without a HIP call (the device
// half is engine_ckpt.cpp), so the CPU suite drives it on batches of the real builder
// (tests/native/ck_plan_main.cpp).
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mte.h"
#include "engine_types.hpp"
#include "host_batch.hpp"

namespace mte {
inline u64 blk_ck_region_words(const DocCfg& c, u32 map_words) {
    return blk_ck_region_words(c.hb_blk, c.hb_ord, c.hb_in, c.hb_heap, c.seg_cap, c.ovl2_off != OVL2_NONE, c.arena_cap,
                               c.map_cap, map_words);
}
}  // namespace mte

#pragma GCC visibility push(hidden)

struct CkDoc {
    uint64_t n_ops = 0, n_pay = 0, off = 0, h_ops = 0, h_pay = 0;
    uint8_t kind = 0;  // the region's format: 0 a row checkpoint, 1 a block checkpoint (k_blk_ck)
    uint8_t props = 0; // the log has an op with a property set (its map records hold key / value ids)
    uint64_t cap = 0;  // words of the region
};

// What the engine keeps between two retained passes.
struct CkState {
    int cur = -1;                 // the buffer with the last pass's checkpoints (-1: none)
    std::vector<CkDoc> prev;      // per document of the last pass: what its checkpoint covers, and where
    std::vector<CkDoc> load;      // per document of the loaded batch: its whole log's hashes
    std::vector<uint64_t> match;  // per document of the loaded batch: op records it shares with prev
    HostBatch tabs;               // the last pass's property tables (ids must keep their meaning)
    uint64_t tabs_n = 0;          // their key / value / propset counts, 0 = none kept
    uint32_t map_words = 0;

    void reset() {
        cur = -1;
        prev.clear();
        load.clear();
        match.clear();
        tabs_n = 0;
    }
    // the previous pass left document d a checkpoint (in a region of its own) that this pass's log extends
    bool have(uint32_t d) const { return cur >= 0 && d < match.size() && d < prev.size() && match[d] && prev[d].cap; }
    // t's tables are the ones the kept checkpoints' ids mean
    void keep_tabs(const HostBatch& t, uint32_t words) {
        tabs.propsets = t.propsets;
        tabs.prop_keys = t.prop_keys;
        tabs.prop_vals = t.prop_vals;
        tabs.key_offsets = t.key_offsets;
        tabs.key_text = t.key_text;
        tabs.val_offsets = t.val_offsets;
        tabs.val_text = t.val_text;
        tabs_n = 1 + (uint64_t)t.propsets.size() + t.prop_keys.size() + t.key_offsets.size() + t.val_offsets.size();
        map_words = words;
    }
};

// word-wise hash of a byte range, continuing from h (a prefix's hash continues to the whole log's)
inline uint64_t ck_hash(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, b + i, 8);
        h = (h ^ w) * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
    }
    for (; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}
// payload units one at a time: a prefix's hash continued over the rest is the whole run's hash
// whatever the prefix's length (a word-wise hash would regroup the units after an odd cut)
inline uint64_t ck_hash_units(uint64_t h, const uint16_t* y, uint64_t n) {
    for (uint64_t i = 0; i < n; i++) {
        h = (h ^ y[i]) * 0x100000001B3ull;
        h ^= h >> 31;
    }
    return h;
}
// an op record as the engine reads it: MTE_F_CATCHUP marks the ops of the messages still above
// minSeq at the END of a log (DocBuild::commit), which the row engines never read, so a prefix log
// and its extension differ there and nowhere else.
// A property-set id is hashed as the set's content (ps_hash: its keys' and values' interned texts in
// order), not as the number a builder happened to give it: a fresh builder over longer logs of several
// property-carrying documents numbers keys, values and sets in another order, and the log is the
// same log. (Cell records' props is a value id of another table walk: hashed as it is.)
inline uint64_t ck_hash_ops(uint64_t h, const mte_op* o, uint64_t n, const std::vector<uint64_t>& ps_hash, bool* props = nullptr) {
    for (uint64_t i = 0; i < n; i++) {
        mte_op x = o[i];
        x.flags &= ~MTE_F_CATCHUP;
        const bool set = x.props && x.props < ps_hash.size() && x.type != MTE_OP_CELL &&
                         !(x.type == MTE_OP_NOOP && (x.flags & MTE_F_MX_MASK));
        const uint64_t ph = set ? ps_hash[x.props] : 0;
        if (set) {
            x.props = 1;
            if (props) *props = true;
        }
        h = ck_hash(h, &x, sizeof x);
        if (set) {
            h = (h ^ ph) * 0x9E3779B97F4A7C15ull;
            h ^= h >> 29;
        }
    }
    return h;
}
// content hash of every property set of a batch's tables
inline std::vector<uint64_t> ck_ps_hashes(const HostBatch& t) {
    std::vector<uint64_t> out(t.propsets.size(), 0);
    for (size_t s = 0; s < t.propsets.size(); s++) {
        uint64_t h = 0xCBF29CE484222325ull;
        const mte_propset& ps = t.propsets[s];
        for (uint32_t q = 0; q < ps.count && (size_t)ps.first + q < t.prop_keys.size(); q++) {
            const uint32_t k = t.prop_keys[ps.first + q], v = t.prop_vals[ps.first + q];
            auto mix = [&](const std::string& text, const std::vector<uint64_t>& off, uint32_t id, unsigned char sep) {
                if ((size_t)id + 1 < off.size())
                    for (uint64_t c = off[id]; c < off[id + 1]; c++) h = (h ^ (unsigned char)text[c]) * 0x100000001B3ull;
                h = (h ^ sep) * 0x100000001B3ull;
            };
            mix(t.key_text, t.key_offsets, k, 0xFF);
            mix(t.val_text, t.val_offsets, v, 0xFE);
        }
        out[s] = h ^ ((uint64_t)ps.count << 56);
    }
    return out;
}
// the loaded tables start with the last pass's: every id the checkpointed map records hold means the
// same key / value / property set
inline bool ck_tabs_extend(const HostBatch& old, const HostBatch& nw) {
    auto pre = [](const auto& a, const auto& b) { return a.size() <= b.size() && std::equal(a.begin(), a.end(), b.begin()); };
    auto pre_ps = [](const std::vector<mte_propset>& a, const std::vector<mte_propset>& b) {
        if (a.size() > b.size()) return false;
        for (size_t i = 0; i < a.size(); i++)
            if (a[i].first != b[i].first || a[i].count != b[i].count) return false;
        return true;
    };
    return pre_ps(old.propsets, nw.propsets) && pre(old.prop_keys, nw.prop_keys) && pre(old.prop_vals, nw.prop_vals) &&
           pre(old.key_offsets, nw.key_offsets) && pre(old.key_text, nw.key_text) && pre(old.val_offsets, nw.val_offsets) &&
           pre(old.val_text, nw.val_text);
}

// The kept block checkpoints whose map records hold ids of the last pass's tables, to be renumbered in
// place to the loaded batch's (k_ck_xlate): old id -> new id of the same text, NONE where the text is gone.
struct CkRenumber {
    std::vector<uint32_t> key, val;
    std::vector<uint64_t> off, cap;  // the checkpoints' regions (words) in the last pass's buffer
};

// mte_load with retain: which documents of batch b (tables `tabs`, map records of `map_words` words)
// extend the last pass's (s.match), and the hashes of their whole logs for the next one (s.load).
// Tables that do not start with the last pass's (a fresh builder per pass over several
// property-carrying documents interns in another order) still number the same keys and values: a
// document without property sets has no id in its checkpoint and continues as it is; a block
// checkpoint's map records are renumbered, once (the CkRenumber returned), and the kept tables become
// the loaded ones. A row checkpoint with map records is not offered then.
inline CkRenumber ck_match(CkState& s, const mte_batch* b, const HostBatch& tabs, uint32_t map_words) {
    const uint32_t nd = b->n_docs;
    s.match.assign(nd, 0);
    s.load.assign(nd, CkDoc{});
    const bool kept = s.cur >= 0 && s.prev.size() == nd && s.tabs_n && s.map_words == map_words;
    const bool extend = kept && ck_tabs_extend(s.tabs, tabs);
    const std::vector<uint64_t> ps_hash = ck_ps_hashes(tabs);
    for (uint32_t d = 0; d < nd; d++) {
        const mte_op* o = b->ops + b->doc_op_offsets[d];
        const uint16_t* y = b->payload + b->doc_payload_offsets[d];
        const uint64_t n = b->doc_op_offsets[d + 1] - b->doc_op_offsets[d];
        const uint64_t np = b->doc_payload_offsets[d + 1] - b->doc_payload_offsets[d];
        CkDoc& c = s.load[d];
        c.n_ops = n;
        c.n_pay = np;
        uint64_t ho = 0xCBF29CE484222325ull, hp = 0xCBF29CE484222325ull, k = 0, kp = 0;
        bool has_props = false;
        if (kept) {
            const CkDoc& q = s.prev[d];
            if (q.n_ops && q.n_ops <= n && q.n_pay <= np) {
                ho = ck_hash_ops(ho, o, q.n_ops, ps_hash, &has_props);
                hp = ck_hash_units(hp, y, q.n_pay);
                k = q.n_ops;
                kp = q.n_pay;
                if (ho == q.h_ops && hp == q.h_pay && (extend || !q.props || q.kind == 1)) s.match[d] = q.n_ops;
            }
        }
        c.h_ops = ck_hash_ops(ho, o + k, n - k, ps_hash, &has_props);
        c.h_pay = ck_hash_units(hp, y + kp, np - kp);
        c.props = has_props;
    }
    CkRenumber r;
    if (!kept || extend) return r;
    // renumber the offered block checkpoints that hold ids; every other kept checkpoint with ids is in
    // the old numbering still and is dropped, since the kept tables become this batch's
    auto xlate = [](const std::string& ot, const std::vector<uint64_t>& oo, const std::string& nt, const std::vector<uint64_t>& no) {
        std::unordered_map<std::string, uint32_t> ids;
        for (size_t i = 0; i + 1 < no.size(); i++) ids.emplace(nt.substr(no[i], no[i + 1] - no[i]), (uint32_t)i);
        std::vector<uint32_t> x(oo.empty() ? 0 : oo.size() - 1, NONE);
        for (size_t i = 0; i + 1 < oo.size(); i++) {
            auto it = ids.find(ot.substr(oo[i], oo[i + 1] - oo[i]));
            if (it != ids.end()) x[i] = it->second;
        }
        return x;
    };
    r.key = xlate(s.tabs.key_text, s.tabs.key_offsets, tabs.key_text, tabs.key_offsets);
    r.val = xlate(s.tabs.val_text, s.tabs.val_offsets, tabs.val_text, tabs.val_offsets);
    for (uint32_t d = 0; d < nd; d++) {
        CkDoc& q = s.prev[d];
        if (!q.props) continue;
        if (s.match[d] && q.kind == 1 && q.cap) {
            r.off.push_back(q.off);
            r.cap.push_back(q.cap);
        } else {
            s.match[d] = 0;
            q.n_ops = 0;  // (never offered again)
        }
    }
    s.keep_tabs(tabs, map_words);
    return r;
}

// Block documents of a retained pass are admitted to the budget of block regions in one checkpoint
// buffer shortest first (stable: equal lengths in the order given). Marks blk_ck[doc] 1 (admitted) or
// 2 (over the budget: no checkpoint this pass); returns how many were marked 2.
struct CkCand {
    uint32_t doc;
    uint64_t words, n_ops;  // blk_ck_region_words of the document, and its op records
};
inline uint32_t ck_admit(const std::vector<CkCand>& cand, uint64_t budget_bytes, std::vector<uint8_t>& blk_ck) {
    std::vector<CkCand> by_len(cand);
    std::stable_sort(by_len.begin(), by_len.end(), [](const CkCand& a, const CkCand& b) { return a.n_ops < b.n_ops; });
    uint64_t used = 0;
    uint32_t skipped = 0;
    for (const CkCand& c : by_len) {
        const uint64_t w = (c.words + 63) & ~63ull;
        if ((used + w) * 4 <= budget_bytes) {
            used += w;
            blk_ck[c.doc] = 1;
        } else {
            blk_ck[c.doc] = 2;
            skipped++;
        }
    }
    return skipped;
}

// This pass's regions (DocCfg::ck_out_off / ck_cap) and the previous pass's ones to continue from
// (ck_at / ck_in_off): the row regions first, then the block documents' (blk_ck 1: sized from the
// capacities of the engine each runs on, cfg's hb_* and its worst-case map_cap), each rounded to 64
// words; a block document over the budget (blk_ck 2) gets none. A checkpoint of the other kind than the
// engine the document runs on this pass is offered but not used: the document replays from op 0.
struct CkRegions {
    uint64_t total = 0, row_total = 0;  // words
    uint32_t offered = 0;
};
inline CkRegions ck_assign_regions(const CkState& s, std::vector<DocCfg>& cfg, const std::vector<uint8_t>& blk_ck,
                                   uint32_t map_words) {
    CkRegions r;
    for (int blk = 0; blk < 2; blk++) {
        for (uint32_t d = 0; d < (uint32_t)cfg.size(); d++) {
            DocCfg& c = cfg[d];
            const uint8_t mark = d < blk_ck.size() ? blk_ck[d] : 0;
            const bool is_blk = mark == 1;
            if (is_blk != (blk == 1)) continue;
            c.ck_out_off = r.total;
            c.ck_cap = mark == 2 ? 0 : is_blk ? blk_ck_region_words(c, map_words) : ck_region_words(c.arena_cap, c.map_cap, map_words);
            r.total += (c.ck_cap + 63) & ~63ull;
            const bool have = s.have(d);
            const bool use = have && (s.prev[d].kind == 1) == is_blk;
            c.ck_at = use ? s.match[d] : 0;
            c.ck_in_off = use ? s.prev[d].off : 0;
            r.offered += have;
        }
        if (!blk) r.row_total = r.total;
    }
    return r;
}

// After the pass: its checkpoints are the ones the next pass continues from (the same batch replayed
// again continues every document from its end). row_now_blk[d]: document d's row region was found to
// hold a block checkpoint (it left its rows mid-pass and finished in the checkpointing k_rows_cont; it
// stays a block document from the next pass on).
inline void ck_commit(CkState& s, const std::vector<DocCfg>& cfg, const std::vector<uint64_t>& n_ops_doc,
                      const std::vector<uint8_t>& blk_ck, const std::vector<uint8_t>& row_now_blk, const HostBatch& tabs,
                      uint32_t map_words) {
    const uint32_t nd = (uint32_t)cfg.size();
    s.cur = s.cur == 0 ? 1 : 0;
    s.prev.assign(nd, CkDoc{});
    s.match.assign(nd, 0);
    for (uint32_t d = 0; d < nd; d++) {
        CkDoc& q = s.prev[d];
        if (d < s.load.size()) q = s.load[d];
        q.off = cfg[d].ck_out_off;
        q.n_ops = n_ops_doc[d];
        q.n_pay = cfg[d].payload_len;
        q.kind = (d < blk_ck.size() && blk_ck[d] == 1) || (d < row_now_blk.size() && row_now_blk[d]);
        q.cap = cfg[d].ck_cap;
        if (!q.cap) q.n_ops = 0;  // no region (over the block budget): nothing to offer
        s.match[d] = q.n_ops;
    }
    s.keep_tabs(tabs, map_words);
}

#pragma GCC visibility pop
