// TEST INFRASTRUCTURE (tests/test_markers_cpu.py): the marker queries without a GPU. The host plan
// (marker_plan.hpp) and the wave programs (marker_walk.hpp, compiled with MTE_CPU: every lane looped
// over with the device's semantics) run the way marker.cpp runs them -- plan, one walk_tiles per group,
// one COUNT walk per job, layout, one WRITE walk per job, scatter -- on synthetic output pools with narrow
// and wide map records, and every result is compared with a scalar restatement written here from
// the leaf walks of search / backwardSearch and gatherText's tag lists kept as lists.
// Built with ASan and UBSan: an index outside a table is a report. stdout "ok: ...", stderr empty.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../fluidframework_amd/csrc/marker_plan.hpp"
#include "../../fluidframework_amd/csrc/marker_walk.hpp"

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

// ---- the batch's interned tables: keys 0..4, values 0..N
static const char* KEYS[] = {"\"x\"", "\"referenceTileLabels\"", "\"font-weight\"", "\"markerId\"", "\"text-decoration\""};
static const uint32_t K_X = 0, K_TILE = 1, K_BOLD = 2, K_ID = 3, K_UNDER = 4;
struct Interned {
    std::vector<uint64_t> key_off{0}, val_off{0};
    std::string key_text, val_text;
    std::vector<uint32_t> val_flags;  // bit 0: falsy
    markplan::Tables tables() const {
        return markplan::Tables{(uint32_t)key_off.size() - 1, key_off.data(), key_text.data(), (uint32_t)val_off.size() - 1,
                                val_off.data(), val_text.data()};
    }
    uint32_t val(const std::string& canonical, bool falsy) {
        val_text += canonical;
        val_off.push_back(val_text.size());
        val_flags.push_back(falsy ? 1u : 0u);
        return (uint32_t)val_off.size() - 2;
    }
};

struct Row {
    uint32_t len, kind;  // kind 0 text, 1 marker, 2 run
    bool removed;
    uint32_t ref_type, toff;
    std::vector<std::pair<uint32_t, uint32_t>> props;  // (key id, value id)
    uint32_t net() const { return removed ? 0 : len; }
};
struct Doc {
    std::vector<Row> rows;
    std::vector<uint16_t> text;
    bool ok = true, annot = false;
};
struct Pool {
    std::vector<uint32_t> vis, aux, maps;
    std::vector<uint16_t> text;
    std::vector<uint32_t> row0;
    std::vector<uint64_t> text_off;
    uint32_t map_words;
};

// ---- the scalar restatement
static bool has_label(const Row& r, const std::vector<uint8_t>& contains) {
    if (r.kind != 1 || !(r.ref_type & 1)) return false;
    for (auto& kv : r.props)
        if (kv.first == K_TILE) return contains[kv.second] != 0;
    return false;
}
struct TileAns {
    bool found;
    uint32_t row, pos;
    bool removed;
};
static TileAns find_tile(const Doc& d, uint32_t pos, const std::vector<uint8_t>& contains, bool preceding) {
    int tile = -1;
    if (preceding) {
        uint64_t p = pos;
        for (size_t i = 0; i < d.rows.size(); i++) {
            const uint32_t n = d.rows[i].net();
            if (p < n) {
                if (has_label(d.rows[i], contains)) tile = (int)i;
                break;
            }
            if (n > 0 && has_label(d.rows[i], contains)) tile = (int)i;
            p -= n;
        }
    } else {
        uint64_t end = 0;
        for (auto& r : d.rows) end += r.net();
        if (pos > end) return TileAns{false, 0, 0, false};
        for (int i = (int)d.rows.size() - 1; i >= 0; i--) {
            const uint32_t n = d.rows[i].net();
            const uint64_t start = end - n;
            if (pos >= start) {
                if (has_label(d.rows[i], contains)) tile = i;
                break;
            }
            if (n > 0 && has_label(d.rows[i], contains)) tile = i;
            end = start;
        }
    }
    if (tile < 0) return TileAns{false, 0, 0, false};
    uint32_t at = 0;
    for (int i = 0; i < tile; i++) at += d.rows[i].net();
    return TileAns{true, (uint32_t)tile, at, d.rows[tile].removed};
}

// gatherText's tag block on lists (textSegment.ts:196-240): returns endTags + beginTags
static std::string gather_tags(bool bold, bool under, std::vector<char>& prog) {
    std::vector<char> tags, init, remv;
    std::string begin, end;
    auto in = [](const std::vector<char>& v, char c) { return std::find(v.begin(), v.end(), c) != v.end(); };
    if (bold) tags.push_back('b');
    if (under) tags.push_back('u');
    if (!tags.empty()) {
        for (char t : tags)
            if (!in(prog, t)) {
                begin += std::string("<") + t + ">";
                init.push_back(t);
            }
        for (char t : prog)
            if (!in(tags, t)) {
                end += std::string("</") + t + ">";
                remv.push_back(t);
            }
        std::reverse(init.begin(), init.end());
        for (char t : init) prog.push_back(t);
    } else {
        for (char t : prog) {
            end += std::string("</") + t + ">";
            remv.push_back(t);
        }
    }
    for (char t : remv) {
        auto it = std::find(prog.begin(), prog.end(), t);
        if (it != prog.end()) prog.erase(it);
    }
    return end + begin;
}
struct Piece {
    uint32_t row, pos;
    std::vector<uint16_t> units;
};
static std::vector<Piece> paragraphs(const Doc& d, const Interned& in, const std::vector<uint8_t>& contains, uint32_t start,
                                     uint32_t end) {
    std::vector<Piece> out;
    std::vector<uint16_t> text;
    std::vector<char> prog;
    uint64_t at = 0;
    for (size_t i = 0; i < d.rows.size(); i++) {
        const Row& r = d.rows[i];
        const uint64_t n = r.net(), lo = std::max<uint64_t>(at, start), hi = std::min<uint64_t>(at + n, end);
        if (lo < hi) {
            if (r.kind == 0) {
                bool bold = false, under = false;
                for (auto& kv : r.props) {
                    if (kv.first == K_BOLD) bold = !(in.val_flags[kv.second] & 1);
                    if (kv.first == K_UNDER) under = !(in.val_flags[kv.second] & 1);
                }
                for (char c : gather_tags(bold, under, prog)) text.push_back((uint16_t)c);
                for (uint64_t u = lo - at; u < hi - at; u++) text.push_back(d.text[r.toff + u]);
            } else if (r.kind == 1 && has_label(r, contains)) {
                out.push_back(Piece{(uint32_t)i, (uint32_t)at, text});
                text.clear();
            }
        }
        at += n;
    }
    return out;
}

// ---- the device's view of the documents
static Pool make_pool(const std::vector<Doc>& docs, uint32_t map_words) {
    Pool p;
    p.map_words = map_words;
    for (const Doc& d : docs) {
        p.row0.push_back((uint32_t)(p.vis.size() / 4));
        p.text_off.push_back(p.text.size());
        for (const Row& r : d.rows) {
            const uint32_t flags = (r.removed ? MW_REMOVED : 0u) | (r.kind == 1 ? MW_MARKER : 0u) | (r.kind == 2 ? MW_PERM : 0u);
            p.vis.insert(p.vis.end(), {r.len, 1u, r.removed ? 2u : 0u, 1u | flags});
            p.aux.insert(p.aux.end(), {r.props.empty() ? 0u : 7u, r.kind == 1 ? (r.ref_type | 0x50000u) : r.kind == 2 ? 9u : r.toff, 0u, 0u});
            std::vector<uint32_t> rec(map_words, 0xDEADBEEFu);  // (a row without props has no record: garbage)
            if (!r.props.empty()) {
                rec[0] = (uint32_t)r.props.size();
                for (size_t k = 0; k < r.props.size(); k++) {
                    rec[1 + 2 * k] = r.props[k].first;
                    rec[2 + 2 * k] = r.props[k].second;
                }
            }
            p.maps.insert(p.maps.end(), rec.begin(), rec.end());
        }
        p.text.insert(p.text.end(), d.text.begin(), d.text.end());
    }
    return p;
}

struct Call {
    std::vector<mte_mark_r> out;
    std::vector<mte_mark_piece> pieces;
    std::vector<uint16_t> text;
};
// marker.cpp's sequence with the wave programs on the CPU
static Call run(const std::vector<Doc>& docs, const Pool& pool, const Interned& in, const std::vector<mte_mark_q>& q,
                const std::vector<std::string>& labels) {
    const markplan::Tables t = in.tables();
    const markplan::Keys keys = markplan::find_keys(t);
    std::vector<uint32_t> slot(labels.size()), bits;
    std::vector<std::string> distinct;
    for (size_t l = 0; l < labels.size(); l++) {
        size_t s = std::find(distinct.begin(), distinct.end(), labels[l]) - distinct.begin();
        if (s == distinct.size()) {
            distinct.push_back(labels[l]);
            std::vector<uint32_t> b;
            markplan::label_bitmap(t, labels[l], b);
            bits.insert(bits.end(), b.begin(), b.end());
        }
        slot[l] = (uint32_t)s;
    }
    markplan::Plan pl;
    markplan::plan_markers(
        q.data(), q.size(), (uint32_t)docs.size(), slot,
        [&](uint32_t d) { return markplan::DocInfo{docs[d].ok, pool.row0[d], (uint32_t)docs[d].rows.size(), pool.text_off[d]}; },
        [&](uint32_t d) { return docs[d].annot; }, pl);
    MarkParams p{};
    p.out_vis = pool.vis.data();
    p.out_aux = pool.aux.data();
    p.out_maps = pool.maps.data();
    p.map_words = pool.map_words;
    p.n_vals = t.n_vals;
    p.val_flags = in.val_flags.data();
    p.out_text = pool.text.data();
    p.text_units = pool.text.size();
    p.key_tile = keys.tile;
    p.key_bold = keys.bold;
    p.key_under = keys.under;
    p.bits_words = (t.n_vals + 31) / 32;
    p.label_bits = bits.data();
    std::vector<MarkTileRec> rec(pl.probe_pos.size(), MarkTileRec{0xAAAAAAAAu, 0xAAAAAAAAu, 0xAAAAAAAAu, 0});
    std::vector<MarkCount> count(pl.jobs.size());
    p.groups = pl.groups.data();
    p.n_groups = (uint32_t)pl.groups.size();
    p.probe_pos = pl.probe_pos.data();
    p.rec = rec.data();
    for (uint32_t g = 0; g < p.n_groups; g++) mark::walk_tiles(p, g);
    p.jobs = pl.jobs.data();
    p.n_jobs = (uint32_t)pl.jobs.size();
    p.count = count.data();
    for (uint32_t j = 0; j < p.n_jobs; j++) mark::walk_paragraphs<false>(p, j);
    uint64_t np = 0, nu = 0;
    markplan::layout_jobs(pl, count.data(), np, nu);
    Call c;
    c.out.resize(q.size());
    markplan::scatter_markers(pl, q.data(), q.size(), rec.data(), c.out.data());
    c.pieces.assign(np, mte_mark_piece{0xAAAAAAAAu, 0, 0, 0, 0});
    c.text.assign(nu, 0xAAAA);  // exactly the laid-out sizes: a write past them is a sanitizer report
    p.jobs = pl.jobs.data();
    p.pieces = c.pieces.data();
    p.n_pieces = np;
    p.text_out = c.text.data();
    p.text_out_units = nu;
    for (uint32_t j = 0; j < p.n_jobs; j++) mark::walk_paragraphs<true>(p, j);
    return c;
}

static void check_call(const std::vector<Doc>& docs, const Interned& in, const std::vector<mte_mark_q>& q,
                       const std::vector<std::string>& labels, const std::vector<std::vector<uint8_t>>& contains, const Call& c,
                       const char* what) {
    uint64_t np = 0, nt = 0;
    for (size_t i = 0; i < q.size(); i++) {
        const mte_mark_q& m = q[i];
        const mte_mark_r& r = c.out[i];
        int want = MTE_MARK_OK;
        if (m.doc >= docs.size() || m.label >= labels.size() || m.kind > 2 || (m.kind == 2 && m.pos2 < m.pos1)) want = MTE_MARK_BAD_QUERY;
        else if (!docs[m.doc].ok) want = MTE_MARK_DOC_FAILED;
        else if (m.kind != 2 && docs[m.doc].annot) want = MTE_MARK_UNSUPPORTED;
        if (want != MTE_MARK_OK) {
            CHECK(r.status == want, "%s q%zu status %d want %d", what, i, r.status, want);
            continue;
        }
        const Doc& d = docs[m.doc];
        if (m.kind != 2) {
            const TileAns a = find_tile(d, m.pos1, contains[m.label], m.kind == 0);
            CHECK(r.status == (a.found ? MTE_MARK_OK : MTE_MARK_NOT_FOUND), "%s q%zu doc %u kind %u pos %u status %d", what, i, m.doc,
                  m.kind, m.pos1, r.status);
            if (a.found)
                CHECK(r.row == a.row && r.pos == a.pos && r.flags == (a.removed ? 1u : 0u), "%s q%zu doc %u kind %u pos %u: row %u pos %u flags %u want %u %u %d",
                      what, i, m.doc, m.kind, m.pos1, r.row, r.pos, r.flags, a.row, a.pos, (int)a.removed);
            continue;
        }
        const std::vector<Piece> want_p = paragraphs(d, in, contains[m.label], m.pos1, m.pos2);
        CHECK(r.status == MTE_MARK_OK && r.count == want_p.size() && r.first_piece == np, "%s q%zu doc %u [%u,%u): count %u want %zu first %llu want %llu",
              what, i, m.doc, m.pos1, m.pos2, r.count, want_p.size(), (unsigned long long)r.first_piece, (unsigned long long)np);
        if (r.count != want_p.size()) return;
        for (const Piece& w : want_p) {
            const mte_mark_piece& g = c.pieces[np++];
            CHECK(g.row == w.row && g.pos == w.pos && g.text_off == nt && g.text_len == w.units.size(),
                  "%s q%zu piece: row %u pos %u off %llu len %u want %u %u %llu %zu", what, i, g.row, g.pos, (unsigned long long)g.text_off,
                  g.text_len, w.row, w.pos, (unsigned long long)nt, w.units.size());
            if (g.text_off != nt || g.text_len != w.units.size()) return;
            CHECK(std::equal(w.units.begin(), w.units.end(), c.text.begin() + nt), "%s q%zu piece text differs", what, i);
            nt += w.units.size();
        }
    }
    CHECK(np == c.pieces.size() && nt == c.text.size(), "%s totals %llu/%zu %llu/%zu", what, (unsigned long long)np, c.pieces.size(),
          (unsigned long long)nt, c.text.size());
}

int main() {
    // ---- the plan's table helpers
    Interned in;
    for (const char* k : KEYS) {
        in.key_text += k;
        in.key_off.push_back(in.key_text.size());
    }
    const uint32_t V_NULL = in.val("null", true);
    const uint32_t V_EOP = in.val("[\"EOP\"]", false);
    const uint32_t V_THREE = in.val("[\"H1\",\"EOP\",\"Q\"]", false);
    const uint32_t V_STR = in.val("\"EQ\"", false);            // code points E, Q
    const uint32_t V_EMOJI = in.val("\"\xF0\x9F\x98\x80x\"", false);  // U+1F600, x
    const uint32_t V_NUM = in.val("7", false);
    const uint32_t V_TRUE = in.val("true", false);
    const uint32_t V_EMPTY = in.val("\"\"", true);
    const uint32_t V_ZERO = in.val("0", true);
    const uint32_t V_OBJ = in.val("{\"EOP\":1}", false);
    const uint32_t V_MIXED = in.val("[1,null,[\"EOP\"],\"H1\"]", false);
    std::vector<uint32_t> filler;
    for (int i = 0; i < 80; i++) filler.push_back(in.val("[\"L" + std::to_string(i) + "\"]", false));  // the bitmap passes one word
    const uint32_t V_LATE = in.val("[\"EOP\",\"late\"]", false);  // a value id above 64
    const markplan::Keys keys = markplan::find_keys(in.tables());
    CHECK(keys.tile == K_TILE && keys.bold == K_BOLD && keys.under == K_UNDER, "keys %u %u %u", keys.tile, keys.bold, keys.under);
    {
        Interned none;
        none.key_text = "\"referenceTileLabel\"";
        none.key_off.push_back(none.key_text.size());
        const markplan::Keys k = markplan::find_keys(none.tables());
        CHECK(k.tile == MK_NONE && k.bold == MK_NONE && k.under == MK_NONE, "absent keys");
    }
    const std::vector<std::string> labels = {"EOP", "H1", "E", "\xF0\x9F\x98\x80", "EOP", "L70", "nope"};
    std::vector<std::vector<uint8_t>> contains(labels.size(), std::vector<uint8_t>(in.val_off.size() - 1, 0));
    auto set = [&](size_t l, std::initializer_list<uint32_t> vs) {
        for (uint32_t v : vs) contains[l][v] = 1;
    };
    set(0, {V_EOP, V_THREE, V_LATE});
    set(1, {V_THREE, V_MIXED});
    set(2, {V_STR});
    set(3, {V_EMOJI});
    set(4, {V_EOP, V_THREE, V_LATE});
    set(5, {filler[70]});
    for (size_t l = 0; l < labels.size(); l++) {
        std::vector<uint32_t> b;
        markplan::label_bitmap(in.tables(), labels[l], b);
        CHECK(b.size() == (in.val_off.size() - 1 + 31) / 32 && b.size() >= 3, "bitmap words %zu", b.size());
        for (uint32_t v = 0; v + 1 < in.val_off.size(); v++)
            CHECK(((b[v >> 5] >> (v & 31)) & 1u) == contains[l][v], "label %zu value %u", l, v);
    }
    {
        const mte_propset ps[3] = {{0, 0}, {0, 2}, {2, 1}};
        const uint32_t pk[3] = {K_X, K_TILE, K_BOLD};
        std::vector<uint8_t> has;
        markplan::propsets_with_key(ps, 3, pk, K_TILE, has);
        CHECK(has == std::vector<uint8_t>({0, 1, 0}), "propsets_with_key");
        mte_op ops[4] = {};
        ops[0].type = MTE_OP_INSERT_MARKER; ops[0].props = 1;
        ops[1].type = MTE_OP_ANNOTATE; ops[1].props = 2;
        ops[2].type = MTE_OP_ANNOTATE; ops[2].props = 1;
        ops[3].type = MTE_OP_ANNOTATE; ops[3].props = 9;
        CHECK(!markplan::doc_annotates(ops, 0, 2, has) && markplan::doc_annotates(ops, 0, 3, has) && !markplan::doc_annotates(ops, 3, 4, has),
              "doc_annotates");
        markplan::propsets_with_key(ps, 3, pk, MK_NONE, has);
        CHECK(!markplan::doc_annotates(ops, 0, 4, has), "doc_annotates without the key");
    }
    // ---- the tag table against the lists: every state, every tag list
    {
        const char* names[5] = {"", "b", "u", "ub", "bu"};
        for (uint32_t s = 0; s < 5; s++)
            for (uint32_t T = 0; T < 4; T++) {
                std::vector<char> prog(names[s], names[s] + strlen(names[s]));
                const std::string want = gather_tags(T & 1, T & 2, prog);
                const uint32_t e = mark::tag_step(s, T);
                uint16_t buf[8];
                const uint32_t n = mark::put_tag(buf, (e >> 3) & 7), n2 = mark::put_tag(buf + n, (e >> 6) & 7);
                const std::string got(buf, buf + n + n2);
                CHECK(got == want && n + n2 == mark::tag_len((e >> 3) & 7) + mark::tag_len((e >> 6) & 7), "tags s%u T%u: %s want %s", s, T,
                      got.c_str(), want.c_str());
                CHECK(std::string(prog.begin(), prog.end()) == names[e & 7], "next s%u T%u: %u", s, T, e & 7);
            }
    }

    // ---- random documents
    std::mt19937 rng(12345);
    auto rnd = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const std::vector<uint32_t> tile_vals = {V_EOP, V_EOP, V_EOP, V_THREE, V_STR, V_EMOJI, V_NUM, V_TRUE, V_EMPTY, V_NULL, V_OBJ, V_MIXED, V_LATE, filler[70], V_ZERO};
    const std::vector<uint32_t> tag_vals = {V_TRUE, V_TRUE, V_NUM, V_NULL, V_ZERO, V_EMPTY, V_OBJ};
    for (int wide = 0; wide < 2; wide++) {
        std::vector<Doc> docs;
        const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 200, 300, 64, 130};
        for (uint32_t n : sizes) {
            Doc d;
            const uint32_t p_mark = 5 + rnd(40), p_rem = rnd(30);
            for (uint32_t i = 0; i < n; i++) {
                Row r{};
                const uint32_t k = rnd(100);
                r.kind = k < p_mark ? 1 : k < p_mark + 3 ? 2 : 0;
                r.removed = rnd(100) < p_rem;
                if (r.kind == 1) {
                    r.len = 1;
                    r.ref_type = rnd(8) ? 1 + 2 * rnd(2) : 2 * rnd(2);
                    if (rnd(10)) {
                        if (wide && rnd(2))
                            for (uint32_t x = 0; x < 7; x++) r.props.emplace_back(K_X + 100 + x, V_NUM);  // nine properties
                        if (rnd(3) == 0) r.props.emplace_back(K_ID, V_STR);
                        if (rnd(8)) r.props.emplace_back(K_TILE, tile_vals[rnd((uint32_t)tile_vals.size())]);
                        if (rnd(3) == 0) r.props.emplace_back(K_X, V_EOP);
                    }
                } else if (r.kind == 2) {
                    r.len = 1 + rnd(5);
                } else {
                    r.len = rnd(12) == 0 ? 60 + rnd(90) : rnd(20) == 0 ? 0 : 1 + rnd(6);
                    r.toff = (uint32_t)d.text.size();
                    for (uint32_t u = 0; u < r.len; u++) d.text.push_back((uint16_t)(0x100 + rnd(0x700)));
                    if (rnd(3) == 0) r.props.emplace_back(K_X, V_EOP);
                    if (rnd(3) == 0) r.props.emplace_back(K_BOLD, tag_vals[rnd((uint32_t)tag_vals.size())]);
                    if (rnd(3) == 0) r.props.emplace_back(K_UNDER, tag_vals[rnd((uint32_t)tag_vals.size())]);
                }
                d.rows.push_back(r);
            }
            docs.push_back(d);
        }
        // the last row: a visible tile, a removed tile, a text row
        docs[4].rows.back() = Row{1, 1, false, 1, 0, {{K_TILE, V_EOP}}};
        docs[5].rows.back() = Row{1, 1, true, 1, 0, {{K_TILE, V_EOP}}};
        docs[6].rows.back() = Row{1, 0, false, 0, 0, {}};
        docs[11].ok = false;
        docs[12].annot = true;
        const Pool pool = make_pool(docs, wide ? 24 : 16);
        std::vector<mte_mark_q> q;
        for (uint32_t d = 0; d < docs.size(); d++) {
            uint32_t L = 0;
            for (auto& r : docs[d].rows) L += r.net();
            for (uint32_t l = 0; l < labels.size(); l++) {
                const uint32_t stride = (l == 0 || L < 80) ? 1 : 7;
                for (uint32_t pos = 0; pos <= L + 2; pos += stride) {
                    q.push_back(mte_mark_q{d, MTE_MQ_TILE_BEFORE, pos, 0, l});
                    q.push_back(mte_mark_q{d, MTE_MQ_TILE_AFTER, pos, 0, l});
                }
                q.push_back(mte_mark_q{d, MTE_MQ_TILE_AFTER, L, 0, l});
                q.push_back(mte_mark_q{d, MTE_MQ_TILE_BEFORE, 0xFFFFFFFFu, 0, l});
                q.push_back(mte_mark_q{d, MTE_MQ_PARAGRAPHS, 0, 0xFFFFFFFFu, l});
                for (int k = 0; k < 6; k++) {
                    const uint32_t a = rnd(L + 2), b = a + rnd(L + 3 - a);
                    q.push_back(mte_mark_q{d, MTE_MQ_PARAGRAPHS, a, b, l});
                }
                q.push_back(mte_mark_q{d, MTE_MQ_PARAGRAPHS, L / 2, L / 2, l});
            }
        }
        q.push_back(mte_mark_q{(uint32_t)docs.size(), MTE_MQ_TILE_BEFORE, 0, 0, 0});
        q.push_back(mte_mark_q{0, MTE_MQ_TILE_BEFORE, 0, 0, (uint32_t)labels.size()});
        q.push_back(mte_mark_q{0, 3, 0, 0, 0});
        q.push_back(mte_mark_q{3, MTE_MQ_PARAGRAPHS, 5, 4, 0});
        q.push_back(mte_mark_q{3, MTE_MQ_TILE_AFTER, 5, 4, 0});  // pos2 is PARAGRAPHS' alone
        std::shuffle(q.begin(), q.end(), rng);
        const Call c = run(docs, pool, in, q, labels);
        check_call(docs, in, q, labels, contains, c, wide ? "wide" : "narrow");
        std::reverse(q.begin(), q.end());
        const Call c2 = run(docs, pool, in, q, labels);
        check_call(docs, in, q, labels, contains, c2, wide ? "wide reversed" : "narrow reversed");
    }
    if (g_fail) {
        fprintf(stderr, "%d of %ld checks failed\n", g_fail, g_checks);
        return 1;
    }
    printf("ok: %ld checks\n", g_checks);
    return 0;
}
