// TEST INFRASTRUCTURE: the host arithmetic of incremental replay (fluidframework_amd/csrc/ck_plan.hpp) as a
// stand-alone host program over batches of the real builder (builder.cpp), built with AddressSanitizer
// and UBSan and linked without the HIP runtime and without libmte.so (tests/test_ck_plan_cpu.py).
//
// Every case is a table lookup, none replays anything: a pass is stood in for by ck_commit over made-up
// regions. Expected values come from the inputs: the number of messages appended (each carries one op,
// so one record) and texts looked up by string. Prints "ok: <checks>" and exits 0, or one line per
// failed check on stderr and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fluidframework_amd/csrc/ck_plan.hpp"
#include "../../include/mte.h"

static int g_checks = 0, g_failed = 0;
#define CHECK(x)                                                            \
    do {                                                                    \
        g_checks++;                                                         \
        if (!(x)) {                                                         \
            g_failed++;                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
        }                                                                   \
    } while (0)

// ---- logs: one writer, one op per message; refSeq lags by two, so a message above minSeq is one the
// builder marks MTE_F_CATCHUP at the end of a log
struct Log {
    int seq = 0;
    std::vector<std::string> msgs;
    void add(const std::string& contents, int msn = 0, bool lag = true) {
        seq++;
        const int ref = lag && seq >= 2 ? seq - 2 : seq - 1;
        msgs.push_back("{\"clientId\":\"writer\",\"sequenceNumber\":" + std::to_string(seq) + ",\"referenceSequenceNumber\":" +
                       std::to_string(ref) + ",\"minimumSequenceNumber\":" + std::to_string(msn) +
                       ",\"type\":\"op\",\"contents\":" + contents + "}");
    }
    void ins(const std::string& text, int msn = 0, bool lag = true) { add("{\"pos1\":0,\"seg\":\"" + text + "\",\"type\":0}", msn, lag); }
    void ins_props(const std::string& text, const std::string& props) {
        add("{\"pos1\":0,\"seg\":{\"text\":\"" + text + "\",\"props\":" + props + "},\"type\":0}");
    }
    void ann(const std::string& props) { add("{\"pos1\":0,\"pos2\":1,\"props\":" + props + ",\"type\":2}"); }
    std::string json(size_t from, size_t to) const {
        std::string s = "[";
        for (size_t i = from; i < to; i++) s += (i > from ? "," : "") + msgs[i];
        return s + "]";
    }
    std::string json() const { return json(0, msgs.size()); }
};

// ---- a builder's batch, copied (the view is the builder's until its next mte_builder_batch)
struct Snap {
    std::vector<uint64_t> op_off, pay_off;
    std::vector<mte_op> ops;
    std::vector<uint16_t> pay;
    HostBatch tabs;
    uint32_t n_docs() const { return (uint32_t)op_off.size() - 1; }
    uint64_t n_ops(uint32_t d) const { return op_off[d + 1] - op_off[d]; }
    uint64_t n_pay(uint32_t d) const { return pay_off[d + 1] - pay_off[d]; }
    mte_batch view() const {
        mte_batch v;
        memset(&v, 0, sizeof v);
        v.n_docs = n_docs();
        v.doc_op_offsets = op_off.data();
        v.ops = ops.data();
        v.doc_payload_offsets = pay_off.data();
        v.payload = pay.data();
        return v;
    }
};

static Snap snap(mte_builder* b) {
    mte_batch v;
    memset(&v, 0, sizeof v);
    Snap s;
    if (int rc = mte_builder_batch(b, &v)) {
        fprintf(stderr, "mte_builder_batch: %d: %s\n", rc, mte_builder_error(b));
        exit(2);
    }
    const uint32_t n = v.n_docs;
    s.op_off.assign(v.doc_op_offsets, v.doc_op_offsets + n + 1);
    s.pay_off.assign(v.doc_payload_offsets, v.doc_payload_offsets + n + 1);
    s.ops.assign(v.ops, v.ops + s.op_off[n]);
    s.pay.assign(v.payload, v.payload + s.pay_off[n]);
    HostBatch& t = s.tabs;
    t.propsets.assign(v.propsets, v.propsets + v.n_propsets);
    size_t nkv = 0;
    for (const mte_propset& ps : t.propsets) nkv = std::max<size_t>(nkv, (size_t)ps.first + ps.count);
    t.prop_keys.assign(v.prop_keys, v.prop_keys + nkv);
    t.prop_vals.assign(v.prop_vals, v.prop_vals + nkv);
    t.key_offsets.assign(v.key_offsets, v.key_offsets + v.n_keys + 1);
    t.key_text.assign(v.key_text, v.key_offsets[v.n_keys]);
    t.val_offsets.assign(v.val_offsets, v.val_offsets + v.n_vals + 1);
    t.val_text.assign(v.val_text, v.val_offsets[v.n_vals]);
    return s;
}

struct Builder {
    mte_builder* b = nullptr;
    Builder() {
        if (mte_builder_create(&b)) exit(2);
    }
    ~Builder() { mte_builder_destroy(b); }
    void must(int rc, const char* what) {
        if (!rc) return;
        fprintf(stderr, "%s: %d: %s\n", what, rc, mte_builder_error(b));
        exit(2);
    }
    void add_doc(const Log& l) {
        const std::string j = l.json();
        must(mte_builder_add_doc(b, "observer", j.data(), j.size()), "mte_builder_add_doc");
    }
    uint32_t open_doc() {
        uint32_t d = 0;
        must(mte_builder_open_doc(b, "observer", &d), "mte_builder_open_doc");
        return d;
    }
    void append(uint32_t d, const Log& l, size_t from, size_t to) {
        const std::string j = l.json(from, to);
        must(mte_builder_append_messages(b, d, j.data(), j.size()), "mte_builder_append_messages");
    }
};

constexpr uint32_t WORDS = 16;  // map record width of every batch here (at most 7 keys)

// A pass over batch b stood in for: document d's region at word 4096 * (d + 1), 700 + d words.
static uint64_t region_off(uint32_t d) { return 4096ull * (d + 1); }
static uint64_t region_cap(uint32_t d) { return 700 + d; }
static void pass(CkState& s, const Snap& b, const std::vector<uint8_t>& blk_ck, uint32_t map_words = WORDS) {
    std::vector<DocCfg> cfg(b.n_docs(), DocCfg{});
    std::vector<uint64_t> n_ops(b.n_docs());
    for (uint32_t d = 0; d < b.n_docs(); d++) {
        cfg[d].ck_out_off = region_off(d);
        cfg[d].ck_cap = region_cap(d);
        cfg[d].payload_len = (uint32_t)b.n_pay(d);
        n_ops[d] = b.n_ops(d);
    }
    ck_commit(s, cfg, n_ops, blk_ck, {}, b.tabs, map_words);
}
static std::vector<uint64_t> match(CkState& s, const Snap& b, uint32_t map_words = WORDS, CkRenumber* r = nullptr) {
    const mte_batch v = b.view();
    CkRenumber got = ck_match(s, &v, b.tabs, map_words);
    if (r) *r = got;
    return s.match;
}

// ---- a growing open document, and the near misses of its prefix check
static void growing_document() {
    Log l;
    for (int i = 0; i < 9; i++) l.ins("abc");
    l.ins("de");  // 29 payload units: the kept prefix has an odd length
    const size_t m1 = l.msgs.size();
    l.ins("fgh", 10, false);  // minSeq passes every message of the first append
    for (int i = 0; i < 11; i++) l.ins("ijkl", 10);
    const size_t m2 = l.msgs.size();
    for (int i = 0; i < 7; i++) l.ins("m", 10);
    const size_t m3 = l.msgs.size();

    Builder b;
    const uint32_t d = b.open_doc();
    CkState s;
    b.append(d, l, 0, m1);
    const Snap b1 = snap(b.b);
    CHECK(b1.n_ops(0) == m1 && b1.n_pay(0) == 29);
    CHECK(match(s, b1) == std::vector<uint64_t>{0});  // nothing kept yet
    pass(s, b1, {});
    CHECK(s.cur == 0 && s.prev[0].n_ops == m1 && s.prev[0].n_pay == 29 && s.prev[0].props == 0);
    CHECK(match(s, b1) == std::vector<uint64_t>{m1});  // the same batch again continues from its end

    b.append(d, l, m1, m2);
    const Snap b2 = snap(b.b);
    // the kept prefix ended on a catch-up record, which the longer log no longer marks
    CHECK(b1.ops[m1 - 1].flags & MTE_F_CATCHUP);
    CHECK(!(b2.ops[m1 - 1].flags & MTE_F_CATCHUP));
    CHECK(b2.n_ops(0) == m2);
    CHECK(match(s, b2) == std::vector<uint64_t>{m1});
    const CkState kept1 = s;  // (after b1's pass, b2 matched)
    pass(s, b2, {});
    CHECK(s.cur == 1);

    b.append(d, l, m2, m3);
    const Snap b3 = snap(b.b);
    CHECK(b3.n_ops(0) == m3);
    CHECK(match(s, b3) == std::vector<uint64_t>{m2});
    // the whole log's hashes, continued from the prefix's, are those of the log hashed in one go
    CkState fresh;
    match(fresh, b3);
    CHECK(fresh.match[0] == 0);
    CHECK(s.load[0].h_ops == fresh.load[0].h_ops && s.load[0].h_pay == fresh.load[0].h_pay);
    CHECK(s.load[0].n_ops == m3 && s.load[0].n_pay == b3.n_pay(0));
    {  // ... and so after an odd cut alone (b1's 29 units kept, b3 loaded)
        CkState k = kept1;
        CHECK(match(k, b3) == std::vector<uint64_t>{m1});
        CHECK(k.load[0].h_ops == fresh.load[0].h_ops && k.load[0].h_pay == fresh.load[0].h_pay);
    }

    // near misses against the state kept after b2's pass: each alone gives no match
    const CkState kept2 = s;
    auto miss = [&](const Snap& x, uint32_t map_words = WORDS) {
        CkState k = kept2;
        return match(k, x, map_words)[0];
    };
    CHECK(miss(b3) == m2);
    {
        Snap x = b3;
        x.ops[3].pos1 ^= 1;  // one op field inside the prefix
        CHECK(miss(x) == 0);
        x = b3;
        x.ops[m2 - 1].seq += 1;
        CHECK(miss(x) == 0);
        x = b3;
        x.ops[m2].seq += 1;  // (the first record after the prefix is not the prefix's)
        CHECK(miss(x) == m2);
    }
    {
        Snap x = b3;
        x.pay[5] ^= 1;  // one payload unit
        CHECK(miss(x) == 0);
        x = b3;
        x.pay[b2.n_pay(0)] ^= 1;
        CHECK(miss(x) == m2);
    }
    CHECK(miss(b1) == 0);      // a log shorter than the kept one
    CHECK(miss(b3, 20) == 0);  // another map record width
    {
        Snap x = b3;  // MTE_F_CATCHUP alone on prefix records: the same log
        for (size_t i = 0; i < m2; i++) x.ops[i].flags ^= MTE_F_CATCHUP;
        CHECK(miss(x) == m2);
    }
}

// ---- three documents: none, a block checkpoint and a row checkpoint with property sets
struct Three {
    Log plain, blk, row;
    size_t n_plain, n_blk, n_row;  // messages of the first pass
    Three() {
        for (int i = 0; i < 12; i++) plain.ins("plain");
        for (int i = 0; i < 8; i++) blk.ins_props("blk", "{\"bold\":true}");
        blk.ann("{\"size\":12}");
        for (int i = 0; i < 6; i++) row.ins_props("row", "{\"color\":\"red\"}");
        row.ann("{\"size\":14}");
        n_plain = plain.msgs.size(), n_blk = blk.msgs.size(), n_row = row.msgs.size();
        // the second pass: the block document's new key and value come before the row document's old ones
        for (int i = 0; i < 5; i++) plain.ins("more");
        blk.ins_props("new", "{\"italic\":\"yes\"}");
        blk.ann("{\"bold\":false}");
        row.ins_props("row2", "{\"color\":\"red\"}");
    }
};
static int64_t find_text(const std::string& text, const std::vector<uint64_t>& off, const std::string& want) {
    for (size_t i = 0; i + 1 < off.size(); i++)
        if (text.substr(off[i], off[i + 1] - off[i]) == want) return (int64_t)i;
    return -1;
}
// every old id maps to the new id of the same text, NONE where the text is gone
static void check_xlate(const std::vector<uint32_t>& xl, const std::string& ot, const std::vector<uint64_t>& oo, const std::string& nt,
                        const std::vector<uint64_t>& no, bool expect_gone) {
    CHECK(xl.size() + 1 == oo.size());
    bool gone = false;
    for (size_t i = 0; i < xl.size() && i + 1 < oo.size(); i++) {
        const int64_t want = find_text(nt, no, ot.substr(oo[i], oo[i + 1] - oo[i]));
        CHECK(xl[i] == (want < 0 ? NONE : (uint32_t)want));
        gone = gone || want < 0;
    }
    CHECK(gone == expect_gone);
}
static bool same_tabs(const HostBatch& a, const HostBatch& b) {
    return a.key_text == b.key_text && a.key_offsets == b.key_offsets && a.val_text == b.val_text && a.val_offsets == b.val_offsets &&
           a.prop_keys == b.prop_keys && a.prop_vals == b.prop_vals && a.propsets.size() == b.propsets.size();
}

static void fresh_builder_per_pass() {
    const Three t;
    const std::vector<uint8_t> blk_ck{0, 1, 0};  // document 1 runs on k_blk_ck
    Log p1 = t.plain, k1 = t.blk, r1 = t.row;
    p1.msgs.resize(t.n_plain), k1.msgs.resize(t.n_blk), r1.msgs.resize(t.n_row);
    Builder a;
    a.add_doc(p1), a.add_doc(k1), a.add_doc(r1);
    const Snap b1 = snap(a.b);
    CkState s;
    CHECK(match(s, b1) == (std::vector<uint64_t>{0, 0, 0}));
    CHECK(s.load[0].props == 0 && s.load[1].props == 1 && s.load[2].props == 1);
    pass(s, b1, blk_ck);
    CHECK(s.prev[0].kind == 0 && s.prev[1].kind == 1 && s.prev[2].kind == 0);

    Builder b;
    b.add_doc(t.plain), b.add_doc(t.blk), b.add_doc(t.row);
    const Snap b2 = snap(b.b);
    CHECK(!ck_tabs_extend(b1.tabs, b2.tabs));  // (the precondition: "italic" / "yes" precede "color" / "red")
    CHECK(find_text(b1.tabs.key_text, b1.tabs.key_offsets, "\"color\"") != find_text(b2.tabs.key_text, b2.tabs.key_offsets, "\"color\""));
    CkRenumber r;
    CHECK(match(s, b2, WORDS, &r) == (std::vector<uint64_t>{t.n_plain, t.n_blk, 0}));
    CHECK(r.off == std::vector<uint64_t>{region_off(1)} && r.cap == std::vector<uint64_t>{region_cap(1)});
    check_xlate(r.key, b1.tabs.key_text, b1.tabs.key_offsets, b2.tabs.key_text, b2.tabs.key_offsets, false);
    check_xlate(r.val, b1.tabs.val_text, b1.tabs.val_offsets, b2.tabs.val_text, b2.tabs.val_offsets, false);
    CHECK(same_tabs(s.tabs, b2.tabs) && s.tabs_n);
    // loaded again before any pass: the tables extend now, the row checkpoint is still in the old numbering
    CHECK(ck_tabs_extend(s.tabs, b2.tabs));
    CHECK(match(s, b2, WORDS, &r) == (std::vector<uint64_t>{t.n_plain, t.n_blk, 0}));
    CHECK(r.off.empty() && r.key.empty() && r.val.empty());
    pass(s, b2, blk_ck);

    // a third pass whose block document is another log, without "italic" / "yes": those ids are gone
    Log other;
    for (int i = 0; i < 4; i++) other.ins_props("x", "{\"size\":12}");
    Log p3 = t.plain, r3 = t.row;
    p3.ins("tail");
    r3.ann("{\"color\":\"blue\"}");
    Builder c;
    c.add_doc(p3), c.add_doc(other), c.add_doc(r3);
    const Snap b3 = snap(c.b);
    CHECK(!ck_tabs_extend(b2.tabs, b3.tabs));
    CHECK(match(s, b3, WORDS, &r) == (std::vector<uint64_t>{t.plain.msgs.size(), 0, 0}));
    CHECK(r.off.empty());
    check_xlate(r.key, b2.tabs.key_text, b2.tabs.key_offsets, b3.tabs.key_text, b3.tabs.key_offsets, true);
    check_xlate(r.val, b2.tabs.val_text, b2.tabs.val_offsets, b3.tabs.val_text, b3.tabs.val_offsets, true);
    CHECK(same_tabs(s.tabs, b3.tabs));
}

static void one_growing_builder() {
    const Three t;
    Builder b;
    const uint32_t d0 = b.open_doc(), d1 = b.open_doc(), d2 = b.open_doc();
    b.append(d0, t.plain, 0, t.n_plain);
    b.append(d1, t.blk, 0, t.n_blk);
    b.append(d2, t.row, 0, t.n_row);
    const Snap b1 = snap(b.b);
    CkState s;
    match(s, b1);
    pass(s, b1, {0, 1, 0});
    b.append(d0, t.plain, t.n_plain, t.plain.msgs.size());
    b.append(d1, t.blk, t.n_blk, t.blk.msgs.size());
    b.append(d2, t.row, t.n_row, t.row.msgs.size());
    const Snap b2 = snap(b.b);
    CHECK(ck_tabs_extend(b1.tabs, b2.tabs) && !same_tabs(b1.tabs, b2.tabs));
    CkRenumber r;
    CHECK(match(s, b2, WORDS, &r) == (std::vector<uint64_t>{t.n_plain, t.n_blk, t.n_row}));
    CHECK(r.off.empty() && r.cap.empty() && r.key.empty() && r.val.empty());
}

// ---- regions of a pass, and what is kept after it
static void regions() {
    const uint32_t nd = 5;
    std::vector<DocCfg> cfg(nd, DocCfg{});
    for (uint32_t d = 0; d < nd; d++) {
        DocCfg& c = cfg[d];
        c.arena_cap = 1000 + 37 * d;
        c.map_cap = 10 + d;
        c.seg_cap = 300 + d;
        c.ovl2_off = d == 4 ? 0 : OVL2_NONE;
        hbm_caps(500 + 100 * d, c.hb_blk, c.hb_ord, c.hb_in, c.hb_heap);
        c.payload_len = 11 * (d + 1);
    }
    const std::vector<uint8_t> blk_ck{0, 1, 0, 2, 1};  // 1, 4: block documents; 3: one over the budget
    CkState s;
    s.cur = 1;
    s.prev.assign(nd, CkDoc{});
    s.match = {40, 41, 42, 0, 44};
    const uint8_t kind[nd] = {1, 0, 0, 0, 1};  // 0, 1: a checkpoint of the other kind than this pass's engine
    for (uint32_t d = 0; d < nd; d++) {
        s.prev[d].n_ops = s.match[d];
        s.prev[d].off = 64 * (100 + d);
        s.prev[d].cap = d == 3 ? 0 : 500;
        s.prev[d].kind = kind[d];
    }
    const CkRegions r = ck_assign_regions(s, cfg, blk_ck, WORDS);
    CHECK(r.offered == 4);
    const uint32_t order[nd] = {0, 2, 3, 1, 4};  // row regions first
    uint64_t end = 0;
    for (uint32_t q = 0; q < nd; q++) {
        const DocCfg& c = cfg[order[q]];
        CHECK(c.ck_out_off % 64 == 0 && c.ck_out_off >= end);
        end = c.ck_out_off + c.ck_cap;
        if (q == 3) CHECK(r.row_total == c.ck_out_off);
    }
    CHECK(r.total >= end && r.total % 64 == 0 && r.row_total <= r.total);
    for (uint32_t d : {0u, 2u}) CHECK(cfg[d].ck_cap == ck_region_words(cfg[d].arena_cap, cfg[d].map_cap, WORDS));
    for (uint32_t d : {1u, 4u}) {
        const DocCfg& c = cfg[d];
        CHECK(c.ck_cap == blk_ck_region_words(c.hb_blk, c.hb_ord, c.hb_in, c.hb_heap, c.seg_cap, d == 4, c.arena_cap, c.map_cap, WORDS));
        CHECK(c.ck_cap == blk_ck_region_words(c, WORDS) && c.ck_cap > 0);
    }
    CHECK(cfg[3].ck_cap == 0);
    CHECK(cfg[0].ck_at == 0 && cfg[0].ck_in_off == 0 && cfg[1].ck_at == 0 && cfg[1].ck_in_off == 0 && cfg[3].ck_at == 0);
    CHECK(cfg[2].ck_at == 42 && cfg[2].ck_in_off == 64 * 102 && cfg[4].ck_at == 44 && cfg[4].ck_in_off == 64 * 104);

    // after the pass: document 2 was found to hold a block checkpoint in its row region
    const std::vector<uint64_t> n_ops{50, 51, 52, 53, 54};
    ck_commit(s, cfg, n_ops, blk_ck, {0, 0, 1, 0, 0}, HostBatch(), WORDS);
    CHECK(s.cur == 0 && s.map_words == WORDS && s.tabs_n);
    const uint8_t kind_now[nd] = {0, 1, 1, 0, 1};
    for (uint32_t d = 0; d < nd; d++) {
        const CkDoc& q = s.prev[d];
        CHECK(q.kind == kind_now[d] && q.off == cfg[d].ck_out_off && q.cap == cfg[d].ck_cap && q.n_pay == 11 * (d + 1));
        CHECK(q.n_ops == (d == 3 ? 0 : n_ops[d]) && s.match[d] == q.n_ops);  // (no region: nothing to offer)
        CHECK(s.have(d) == (d != 3));
    }
    s.reset();
    CHECK(s.cur == -1 && s.prev.empty() && s.load.empty() && s.match.empty() && !s.tabs_n && !s.have(0));
}

static void admission() {
    // 100 words round to 128: 512 bytes a region
    const std::vector<CkCand> cand{{0, 100, 300}, {1, 100, 100}, {2, 100, 200}};
    auto admit = [&](const std::vector<CkCand>& c, uint64_t budget, uint32_t& skipped) {
        std::vector<uint8_t> m(4, 0);
        skipped = ck_admit(c, budget, m);
        return m;
    };
    uint32_t sk;
    CHECK(admit(cand, 1024, sk) == (std::vector<uint8_t>{2, 1, 1, 0}) && sk == 1);  // the two shortest
    CHECK(admit(cand, 1023, sk) == (std::vector<uint8_t>{2, 1, 2, 0}) && sk == 2);  // (regions are rounded up)
    CHECK(admit(cand, 0, sk) == (std::vector<uint8_t>{2, 2, 2, 0}) && sk == 3);
    CHECK(admit(cand, 1536, sk) == (std::vector<uint8_t>{1, 1, 1, 0}) && sk == 0);
    const std::vector<CkCand> equal{{2, 100, 70}, {0, 100, 70}, {1, 100, 70}};  // equal lengths keep their order
    CHECK(admit(equal, 1024, sk) == (std::vector<uint8_t>{1, 2, 1, 0}) && sk == 1);
}

int main() {
    growing_document();
    fresh_builder_per_pass();
    one_growing_builder();
    regions();
    admission();
    if (g_failed) {
        fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    printf("ok: %d checks\n", g_checks);
    return 0;
}
