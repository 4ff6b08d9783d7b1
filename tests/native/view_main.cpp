// TEST INFRASTRUCTURE (tests/test_views_cpu.py): the view queries without a GPU. The host plan
// (view_plan.hpp) and the two wave programs (view_walk.hpp, compiled with MTE_CPU: every lane looped
// over with the device's semantics) run the way view.cpp runs them -- plan, one walk_group per group,
// scatter, one copy_job per job -- on synthetic output pools, and every result is compared with a
// scalar walk written here from the view predicate as DESIGN §3.16 states it. Built with ASan and
// UBSan: an index outside a table is a report. stdout "ok: ...", stderr empty.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../fluidframework_amd/csrc/view_plan.hpp"
#include "../../fluidframework_amd/csrc/view_walk.hpp"

using namespace mte;
static int g_fail = 0;
static long g_checks = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        g_checks++;                                     \
        if (!(c)) {                                     \
            if (g_fail++ < 20) {                        \
                fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
                fprintf(stderr, __VA_ARGS__);           \
                fprintf(stderr, "\n");                  \
            }                                           \
        }                                               \
    } while (0)

struct Row {
    uint32_t len, kind;  // kind 0 text, 1 marker, 2 run
    int32_t seq, rseq;
    uint32_t client, rclient;
    bool removed;
    uint64_t ovl, ovl2;
    uint32_t toff;
};
struct Doc {
    std::vector<Row> rows;
    std::vector<uint16_t> text;
    bool collab = true, ok = true;
    int32_t min_seq = 0, cur_seq = 0;
};
struct Pool {
    std::vector<uint32_t> vis, aux;
    std::vector<uint64_t> ovl, ovl2;
    std::vector<uint16_t> text;
    std::vector<uint32_t> row0;
    std::vector<uint64_t> text_off;
};

// the view predicate as DESIGN §3.16 states it, one row, scalar
static uint32_t view_len(const Doc& d, const Row& r, uint32_t client, int32_t ref) {
    if (client == 0 || !d.collab) return r.removed ? 0 : r.len;
    if (!(r.client == client || r.seq <= ref)) return 0;
    if (r.removed) {
        const bool in_ovl = client < 64 ? (r.ovl >> client) & 1 : client < 128 ? (r.ovl2 >> (client - 64)) & 1 : false;
        if (r.rclient == client || in_ovl || r.rseq <= ref) return 0;
    }
    return r.len;
}

static Doc make_doc(uint32_t n, uint32_t seed, bool long_rows) {
    std::mt19937 g(seed * 7919u + n);
    Doc d;
    d.cur_seq = (int32_t)(2 * n + 10);
    static const uint32_t lens[] = {1, 31, 32, 33, 64, 65, 300};
    for (uint32_t i = 0; i < n; i++) {
        Row r{};
        r.kind = g() % 9 == 0 ? 1 : g() % 23 == 0 ? 2 : 0;
        r.len = r.kind == 1 ? 1 : long_rows ? lens[g() % 7] : 1 + g() % 5;
        r.seq = (int32_t)(g() % (uint32_t)(d.cur_seq + 1));
        static const uint32_t cl[] = {1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 127};
        r.client = cl[g() % 11];
        r.removed = g() % 4 == 0;
        // rows of length 0 in some views on both sides of every 64-row step
        if ((i >= 62 && i <= 65) || (i >= 126 && i <= 129)) r.removed = true;
        if (r.removed) {
            r.rseq = (int32_t)std::min<uint32_t>((uint32_t)d.cur_seq, (uint32_t)r.seq + g() % 20);
            r.rclient = cl[(i + g()) % 11];
            for (int k = 0; k < 3; k++)
                if (g() % 2) {
                    const uint32_t c = cl[g() % 11];
                    (c < 64 ? r.ovl : r.ovl2) |= 1ull << (c & 63);
                }
        }
        if (r.kind == 0) {
            r.toff = (uint32_t)d.text.size() + (g() % 3);  // (gaps: rows need not be packed)
            d.text.resize(r.toff + r.len);
            for (uint32_t u = 0; u < r.len; u++) d.text[r.toff + u] = (uint16_t)(0x4000u + ((i * 131u + u) & 0x3fffu));
        } else {
            r.toff = 0xFFFF0000u + i;  // a marker's / run's word is no text offset: never read as one
        }
        d.rows.push_back(r);
    }
    return d;
}

static Pool make_pool(const std::vector<Doc>& docs, bool with_ovl2) {
    Pool p;
    for (const Doc& d : docs) {
        p.row0.push_back((uint32_t)(p.vis.size() / 4));
        p.text_off.push_back(p.text.size());
        for (const Row& r : d.rows) {
            const uint32_t meta = (d.collab ? r.client | r.rclient << 8 : 0u) | (r.removed ? VW_REMOVED : 0u) |
                                  (r.kind == 1 ? VW_MARKER : r.kind == 2 ? VW_PERM : 0u);
            p.vis.insert(p.vis.end(), {r.len, (uint32_t)r.seq, (uint32_t)r.rseq, meta});
            p.aux.insert(p.aux.end(), {0u, r.toff, 0u, 0u});
            p.ovl.push_back(r.ovl);
            if (with_ovl2) p.ovl2.push_back(r.ovl2);
        }
        p.text.insert(p.text.end(), d.text.begin(), d.text.end());
    }
    return p;
}

struct Want {
    int32_t status;
    uint32_t row, offset, length, cur_pos, flags;
    std::vector<uint16_t> text;
};

static Want scalar(const std::vector<Doc>& docs, const mte_view_q& q, bool with_ovl2) {
    Want w{};
    if (q.doc >= docs.size() || (q.client >= 128 && q.client != MTE_VIEW_NO_CLIENT) || q.kind > 2 ||
        (q.kind == MTE_VQ_TEXT && q.pos2 < q.pos1)) {
        w.status = MTE_VIEW_BAD_QUERY;
        return w;
    }
    const Doc& d = docs[q.doc];
    if (!d.ok) {
        w.status = MTE_VIEW_DOC_FAILED;
        return w;
    }
    const bool local = q.client == 0 || !d.collab;
    if (!local && (q.ref_seq < d.min_seq || q.ref_seq > d.cur_seq)) {
        w.status = MTE_VIEW_OUT_OF_WINDOW;
        return w;
    }
    uint32_t L = 0;
    for (const Row& r : d.rows) {
        Row rr = r;
        if (!with_ovl2) rr.ovl2 = 0;
        L += view_len(d, rr, q.client, q.ref_seq);
    }
    if (q.kind == MTE_VQ_LENGTH) {
        w.length = L;
        return w;
    }
    uint32_t at = 0, cur = 0;
    for (uint32_t i = 0; i < d.rows.size(); i++) {
        Row rr = d.rows[i];
        if (!with_ovl2) rr.ovl2 = 0;
        const uint32_t v = view_len(d, rr, q.client, q.ref_seq), o = rr.removed ? 0 : rr.len;
        if (q.kind == MTE_VQ_LOCATE) {
            if (v && q.pos1 < at + v) {
                w.row = i;
                w.offset = q.pos1 - at;
                w.length = rr.len;
                w.cur_pos = cur;
                w.flags = rr.removed ? MTE_VIEW_F_REMOVED : 0;
                return w;
            }
        } else if (rr.kind == 0) {
            for (uint32_t u = 0; u < v; u++)
                if (at + u >= q.pos1 && at + u < q.pos2) w.text.push_back(d.text[rr.toff + u]);
        }
        at += v;
        cur += o;
    }
    if (q.kind == MTE_VQ_LOCATE) {
        w.status = MTE_VIEW_PAST_END;
        w.length = L;
    } else {
        w.length = (uint32_t)w.text.size();
    }
    return w;
}

// what view.cpp does, the kernels' waves one after the other
static void run(const std::vector<Doc>& docs, const Pool& pool, bool with_ovl2, const std::vector<mte_view_q>& q,
                std::vector<mte_view_r>& out, std::vector<uint16_t>& text, viewplan::Plan& pl) {
    viewplan::plan_views(q.data(), q.size(), (uint32_t)docs.size(), [&](uint32_t d) {
        viewplan::DocInfo i{};
        i.ok = docs[d].ok;
        i.collab = docs[d].collab;
        i.min_seq = docs[d].min_seq;
        i.cur_seq = docs[d].cur_seq;
        i.row0 = pool.row0[d];
        i.n_rows = (uint32_t)docs[d].rows.size();
        i.text_off = pool.text_off[d];
        return i;
    }, pl);
    ViewParams p{};
    p.out_vis = pool.vis.data();
    p.out_aux = pool.aux.data();
    p.out_ovl = pool.ovl.data();
    p.out_ovl2 = with_ovl2 ? pool.ovl2.data() : nullptr;
    p.out_text = pool.text.data();
    p.text_units = pool.text.size();
    std::vector<ViewProbeRec> rec(pl.probe_pos.size());
    std::vector<uint32_t> totals(pl.groups.size());
    p.groups = pl.groups.data();
    p.n_groups = (uint32_t)pl.groups.size();
    p.probe_pos = pl.probe_pos.data();
    p.rec = rec.data();
    p.totals = totals.data();
    for (uint32_t g = 0; g < p.n_groups; g++) view::walk_group(p, g);
    out.resize(q.size());
    std::vector<ViewCopyJob> jobs;
    uint64_t need = 0;
    viewplan::scatter_views(pl, q.data(), q.size(), rec.data(), totals.data(), out.data(), jobs, need);
    text.assign(need, 0xDEADu);
    p.jobs = jobs.data();
    p.n_jobs = (uint32_t)jobs.size();
    p.text_out = text.data();
    p.text_out_units = need;
    for (uint32_t j = 0; j < p.n_jobs; j++) view::copy_job(p, j);
}

static void compare(const std::vector<Doc>& docs, bool with_ovl2, const std::vector<mte_view_q>& q,
                    const std::vector<mte_view_r>& out, const std::vector<uint16_t>& text, const char* what) {
    uint64_t laid = 0;
    for (size_t i = 0; i < q.size(); i++) {
        const Want w = scalar(docs, q[i], with_ovl2);
        const mte_view_r& r = out[i];
        CHECK(r.status == w.status, "%s q%zu doc %u kind %u client %u ref %d pos %u: status %d want %d", what, i, q[i].doc,
              q[i].kind, q[i].client, q[i].ref_seq, q[i].pos1, r.status, w.status);
        if (r.status != w.status) continue;
        CHECK(r.length == w.length, "%s q%zu kind %u doc %u client %u ref %d pos %u..%u: length %u want %u", what, i,
              q[i].kind, q[i].doc, q[i].client, q[i].ref_seq, q[i].pos1, q[i].pos2, r.length, w.length);
        if (q[i].kind == MTE_VQ_LOCATE && w.status == MTE_VIEW_OK)
            CHECK(r.row == w.row && r.offset == w.offset && r.cur_pos == w.cur_pos && r.flags == w.flags,
                  "%s q%zu doc %u client %u ref %d pos %u: row %u+%u cur %u f %u want %u+%u cur %u f %u", what, i, q[i].doc,
                  q[i].client, q[i].ref_seq, q[i].pos1, r.row, r.offset, r.cur_pos, r.flags, w.row, w.offset, w.cur_pos,
                  w.flags);
        if (q[i].kind == MTE_VQ_TEXT && w.status == MTE_VIEW_OK && r.length == w.length) {
            CHECK(r.text_off == laid, "%s q%zu: text_off %llu want %llu", what, i, (unsigned long long)r.text_off,
                  (unsigned long long)laid);
            CHECK(r.text_off + r.length <= text.size(), "%s q%zu: text outside the buffer", what, i);
            if (r.text_off + r.length <= text.size())
                CHECK(std::equal(w.text.begin(), w.text.end(), text.begin() + r.text_off), "%s q%zu doc %u client %u ref %d %u..%u: text differs",
                      what, i, q[i].doc, q[i].client, q[i].ref_seq, q[i].pos1, q[i].pos2);
            laid += r.length;
        }
    }
    CHECK(laid == text.size(), "%s: %llu units laid out, buffer %zu", what, (unsigned long long)laid, text.size());
}

static const uint32_t SIZES[] = {0, 1, 63, 64, 65, 128, 129, 200};
static const uint32_t CLIENTS[] = {0, 1, 2, 31, 32, 63, 64, 65, 127, MTE_VIEW_NO_CLIENT};

static void test_walk(bool with_ovl2, bool long_rows) {
    std::vector<Doc> docs;
    for (uint32_t n : SIZES) docs.push_back(make_doc(n, with_ovl2 * 2 + long_rows, long_rows));
    docs.push_back(make_doc(70, 99, long_rows));  // a non-collaborating document: every view is the local one
    docs.back().collab = false;
    const Pool pool = make_pool(docs, with_ovl2);
    std::mt19937 g(12345 + with_ovl2);
    std::vector<mte_view_q> q;
    for (uint32_t d = 0; d < docs.size(); d++) {
        const int32_t cur = docs[d].cur_seq;
        for (uint32_t c : CLIENTS)
            for (int32_t ref : {0, cur / 2, cur}) {
                if (c == 0 && ref) continue;
                mte_view_q v{d, ref, c, MTE_VQ_LENGTH, 0, 0};
                const uint32_t L = scalar(docs, v, with_ovl2).length;
                q.push_back(v);
                const uint32_t stride = long_rows ? 1 + L / 97 : 1;
                for (uint32_t pos = 0; pos <= L; pos += stride) q.push_back(mte_view_q{d, ref, c, MTE_VQ_LOCATE, pos, 0});
                q.push_back(mte_view_q{d, ref, c, MTE_VQ_LOCATE, L, 0});
                q.push_back(mte_view_q{d, ref, c, MTE_VQ_LOCATE, L + 7, 0});
                // TEXT: whole, empty, past the end, random
                q.push_back(mte_view_q{d, ref, c, MTE_VQ_TEXT, 0, L});
                q.push_back(mte_view_q{d, ref, c, MTE_VQ_TEXT, 0, 0xFFFFFFFFu});
                q.push_back(mte_view_q{d, ref, c, MTE_VQ_TEXT, L / 2, L / 2});
                q.push_back(mte_view_q{d, ref, c, MTE_VQ_TEXT, L, L + 5});
                q.push_back(mte_view_q{d, ref, c, MTE_VQ_TEXT, L + 3, L + 5});
                for (int k = 0; k < 6; k++) {
                    const uint32_t a = g() % (L + 1), b = a + g() % (L - a + 3);
                    q.push_back(mte_view_q{d, ref, c, MTE_VQ_TEXT, a, b});
                }
            }
    }
    std::shuffle(q.begin(), q.end(), g);
    std::vector<mte_view_r> out;
    std::vector<uint16_t> text;
    viewplan::Plan pl;
    run(docs, pool, with_ovl2, q, out, text, pl);
    compare(docs, with_ovl2, q, out, text, long_rows ? "walk/long" : "walk/short");
}

static void test_plan() {
    std::vector<Doc> docs;
    docs.push_back(make_doc(130, 5, false));
    docs.push_back(make_doc(10, 6, false));
    docs.push_back(make_doc(10, 7, false));
    docs[1].ok = false;
    docs[2].min_seq = 12;
    const Pool pool = make_pool(docs, true);
    std::vector<mte_view_q> q = {
        {0, 200, 2, MTE_VQ_LOCATE, 40, 0},   {0, 200, 2, MTE_VQ_LOCATE, 3, 0},    {0, 200, 2, MTE_VQ_LOCATE, 40, 0},
        {3, 0, 0, MTE_VQ_LENGTH, 0, 0},                                      // doc out of range
        {0, 0, 128, MTE_VQ_LENGTH, 0, 0},                                    // client out of range
        {0, 0, 1, 3, 0, 0},                                                  // unknown kind
        {0, 0, 1, MTE_VQ_TEXT, 5, 4},                                        // pos2 < pos1
        {1, 0, 0, MTE_VQ_LENGTH, 0, 0},                                      // failed document
        {2, 11, 1, MTE_VQ_LENGTH, 0, 0},                                     // below minSeq
        {2, 31, 1, MTE_VQ_LENGTH, 0, 0},                                     // above currentSeq
        {2, 11, 0, MTE_VQ_LENGTH, 0, 0},                                     // the observer has no window
        {0, 200, 2, MTE_VQ_TEXT, 2, 30},     {0, 7, 0, MTE_VQ_LOCATE, 1, 0},   {0, 3, 0, MTE_VQ_LOCATE, 0, 0},
        {0, 200, MTE_VIEW_NO_CLIENT, MTE_VQ_LENGTH, 0, 0},
    };
    std::vector<mte_view_r> out;
    std::vector<uint16_t> text;
    viewplan::Plan pl;
    run(docs, pool, true, q, out, text, pl);
    const int32_t want[] = {0, 0, 0, 4, 4, 4, 4, 3, 2, 2, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < q.size(); i++) {
        CHECK(out[i].status == want[i], "plan q%zu: status %d want %d", i, out[i].status, want[i]);
        // a refused query is in no group and has no probe
        if (want[i]) CHECK(pl.group_of[i] == viewplan::NO_PROBE && pl.probe_a[i] == viewplan::NO_PROBE, "plan q%zu planned", i);
    }
    // groups: (doc 0 local) with both observer queries whatever their ref_seq, (doc 0, client 2, ref 200),
    // (doc 0, NO_CLIENT, ref 200), (doc 2 local)
    CHECK(pl.groups.size() == 4, "plan: %zu groups", pl.groups.size());
    CHECK(pl.group_of[12] == pl.group_of[13], "plan: observer views split by ref_seq");
    CHECK(pl.group_of[0] == pl.group_of[1] && pl.group_of[0] == pl.group_of[2] && pl.group_of[0] == pl.group_of[11], "plan: one view, several groups");
    CHECK(pl.probe_a[0] != pl.probe_a[2], "plan: duplicates share a probe record slot");
    size_t probes = 0;
    for (const ViewGroup& g : pl.groups) {
        CHECK(g.p0 == probes && g.p1 >= g.p0, "plan: probe ranges not back to back");
        for (uint32_t k = g.p0; k + 1 < g.p1; k++) CHECK(pl.probe_pos[k] <= pl.probe_pos[k + 1], "plan: probes not ascending");
        probes = g.p1;
    }
    CHECK(probes == pl.probe_pos.size() && probes == 7, "plan: %zu probes", probes);
    CHECK(out[0].row == out[2].row && out[0].offset == out[2].offset && out[0].cur_pos == out[2].cur_pos, "plan: duplicates differ");
    CHECK(out[11].text_off == 0 && out[11].length == text.size(), "plan: text layout");
    compare(docs, true, q, out, text, "plan");
}

// group sizes on both sides of a wave's 64 rows and far beyond, with duplicates
static void test_group_sizes() {
    std::vector<Doc> docs = {make_doc(200, 11, false)};
    const Pool pool = make_pool(docs, true);
    std::mt19937 g(77);
    for (uint32_t n : {1u, 63u, 64u, 65u, 1000u}) {
        std::vector<mte_view_q> q;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t pos = (i % 3 == 0 && i) ? q[g() % i].pos1 : (uint32_t)(g() % 400);
            q.push_back(mte_view_q{0, 200, 33, i % 5 == 4 ? (uint32_t)MTE_VQ_TEXT : (uint32_t)MTE_VQ_LOCATE, pos, pos + (uint32_t)(g() % 40)});
        }
        std::vector<mte_view_r> out;
        std::vector<uint16_t> text;
        viewplan::Plan pl;
        run(docs, pool, true, q, out, text, pl);
        CHECK(pl.groups.size() == 1, "group of %u: %zu groups", n, pl.groups.size());
        compare(docs, true, q, out, text, "group");
    }
}

int main() {
    test_plan();
    for (int o2 = 0; o2 < 2; o2++)
        for (int lr = 0; lr < 2; lr++) test_walk(o2, lr);
    test_group_sizes();
    if (g_fail) {
        fprintf(stderr, "%d of %ld checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("ok: %ld checks\n", g_checks);
    return 0;
}
