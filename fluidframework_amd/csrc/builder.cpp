// builder.cpp — mte_builder_*: ISequencedDocumentMessage JSON logs -> SoA op records + interned
// property sets (Client.applyMsg input, client.ts:805-836; op shapes ops.ts:29-110), summaries as
// LOAD records (SnapshotLoader, snapshotLoader.ts:38-216; snapshotV1.ts:249-270; legacy chunks,
// snapshotChunks.ts:135-176), container-level logs (clientReplayTool.ts:113-347), SharedMatrix logs
// and summaries (matrix.ts:405-640, permutationvector.ts, sparsearray2d.ts) and open documents.
// Host-only C++: no device call and no engine state; engine_types.hpp is included for its constants.
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/mte.h"
#include "engine_types.hpp"
#include "host_batch.hpp"
#include "jsonlite.hpp"

// the builder object and its documents are internal to the library
#pragma GCC visibility push(hidden)

struct DocBuild;
struct mte_builder {
    HostBatch hb;
    std::unique_ptr<Interner> in;
    std::string err;
    std::vector<std::string> paths;  // per document: channel full path (container logs), else ""
    uint32_t n_cells = 0;            // SharedMatrix cell ops so far (MTE_OP_CELL's cell index)
    // open documents (mte_builder_open_doc): logs still growing, after every committed document;
    // mte_builder_batch commits copies of them into `view`
    std::vector<std::unique_ptr<DocBuild>> open;
    HostBatch view;
    mte_builder() { in.reset(new Interner(&hb)); }
    ~mte_builder();
};

// One document under construction: its records, payload and short-id table (observer = 0).
struct DocBuild {
    std::vector<mte_op> ops;
    std::vector<uint16_t> payload;
    std::vector<std::string> names;
    std::unordered_map<std::string, uint32_t> ids;
    bool collab = false;
    bool perm = false;  // a SharedMatrix row / col vector: PermutationSegment specs
    std::string err;
    // marker ids for relative positions (include/mte.h MTE_OP_RELPOS): id -> tag of the marker the
    // reference maps it to; ids tied to two markers, and every id after an annotate that sets a
    // "markerId" property, are ambiguous (blockUpdate re-maps live markers, mergeTree.ts:2748-2768)
    std::unordered_map<std::u16string, uint32_t> mk_tag;
    std::unordered_set<std::u16string> mk_amb;
    bool mk_annot = false;
    uint32_t n_tags = 0;
    // mapIdToSegment (mergeTree.ts:1185-1187) for a marker record: its tag into bits 16..31 of the
    // refType word *w
    void map_marker(const std::u16string& id, uint32_t* w) {
        if (mk_tag.count(id)) mk_amb.insert(id);
        if (n_tags >= 0xFFFFu) {
            mk_amb.insert(id);
            return;
        }
        mk_tag[id] = ++n_tags;
        *w = (*w & 0xFFFFu) | (n_tags << 16);
    }
    // posFromRelativePos's marker lookup (mergeTree.ts:1949-1951) -> tag, offset, before
    uint32_t rel_tag(const json::Value& rp, int32_t* off, bool* before) const {
        *off = 0;
        *before = false;
        if (rp.kind != json::Value::Object) return MTE_REL_UNMAPPED;
        const json::Value* id = rp.get(u"id");
        const json::Value* bf = rp.get(u"before");
        *before = bf && json::truthy(bf);
        num_field(rp, u"offset", off);
        if (!id || id->kind != json::Value::String || id->str.empty() || mk_annot || mk_amb.count(id->str))
            return MTE_REL_UNMAPPED;
        auto it = mk_tag.find(id->str);
        return it == mk_tag.end() ? MTE_REL_UNMAPPED : it->second;
    }
    // Windowed short ids: the engine's client field has MTE_MAX_CLIENTS values, the reference's
    // short-id map grows without bound (client.ts:644-668; a container log gets a new clientId per
    // reconnect). A client's id matters only while one of its ops is above minSeq: nodeLength
    // (mergeTree.ts:1659-1699) compares client ids only for segments whose seq / removedSeq is above
    // the op's refSeq >= minSeq (msn is the least refSeq of the quorum), and SnapshotV1 names clients
    // only above minSeq. So a slot whose client's last op is at or below minSeq is reused; `names`
    // holds each slot's last owner (the name every output above minSeq refers to). Concurrent
    // overlapping removers are all above minSeq while their removal matters. An op whose refSeq is
    // below minSeq after a reuse is reported unsupported (slot 255), as is a client with no free slot.
    // messagesSinceMSNChange (sequence.ts:597-650): op messages above the running minSeq, as
    // JSON.stringify(JSON.parse(message)), with the index of their first op record; the ones left at
    // commit are the legacy summary's catch-up messages
    struct Msg {
        int32_t seq;
        bool rewrite;  // refSeq != seq - 1: the legacy summary rewrites it from its delta ranges
        uint64_t first_op;
        std::string text;
    };
    std::deque<Msg> stash;
    void trim_stash() {
        while (!stash.empty() && stash.front().seq <= cur_min) stash.pop_front();
    }
    std::vector<int32_t> last_use;  // slot -> highest seq its owner used
    int32_t cur_min = 0;            // minSeq as the engine will have it at the next record
    bool loading = false;           // summary records: no reuse before LOAD_END
    bool reused = false;
    explicit DocBuild(const char* observer_name) {
        const std::string observer = observer_name ? observer_name : "";
        names.push_back(observer);
        last_use.push_back(INT32_MAX);  // the observer keeps slot 0
        ids[observer] = 0;
        collab = !observer.empty();
    }
    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
    // getOrAddShortClientId (client.ts:644-668), windowed (above); `use` = the seq the id is used at
    int short_id(const std::string& name, uint32_t* out, int32_t use = 0) {
        auto it = ids.find(name);
        if (it != ids.end()) {
            *out = it->second;
            if (use > last_use[*out]) last_use[*out] = use;
            return MTE_OK;
        }
        uint32_t slot = NONE;
        if (names.size() < MTE_MAX_CLIENTS) {
            slot = (uint32_t)names.size();
            names.push_back(name);
            last_use.push_back(use);
        } else if (!loading) {
            for (uint32_t q = 1; q < MTE_MAX_CLIENTS && slot == NONE; q++)
                if (last_use[q] <= cur_min) slot = q;
            if (slot != NONE) {
                ids.erase(names[slot]);
                names[slot] = name;
                last_use[slot] = use;
                reused = true;
            }
        }
        // no slot free: the engine reports the document MTE_DOC_UNSUPPORTED at the first record
        // naming this client (255), the rest of the batch replays normally
        *out = slot == NONE ? 255u : slot;
        if (slot != NONE) ids[name] = slot;
        return MTE_OK;
    }
    void commit(HostBatch& hb) {
        trim_stash();
        for (size_t i = 0; i < stash.size(); i++) {
            const uint64_t end = i + 1 < stash.size() ? stash[i + 1].first_op : ops.size();
            if (stash[i].rewrite)
                for (uint64_t q = stash[i].first_op; q < end && q < ops.size(); q++)
                    if (ops[q].type <= MTE_OP_INSERT_MARKER) ops[q].flags |= MTE_F_CATCHUP;
            hb.msg_first_op.push_back(stash[i].first_op);
            hb.msg_text += stash[i].text;
            hb.msg_text_offsets.push_back(hb.msg_text.size());
        }
        hb.doc_msg_offsets.push_back(hb.msg_first_op.size());
        hb.ops.insert(hb.ops.end(), ops.begin(), ops.end());
        hb.doc_op_offsets.push_back(hb.ops.size());
        hb.payload.insert(hb.payload.end(), payload.begin(), payload.end());
        hb.doc_payload_offsets.push_back(hb.payload.size());
        for (auto& nm : names) {
            hb.client_names += nm;
            hb.client_name_offsets.push_back(hb.client_names.size());
        }
        hb.doc_client_offsets.push_back(hb.doc_client_offsets.back() + (uint32_t)names.size());
    }
};

#pragma GCC visibility pop

extern "C" {

// ------------------------------------------------------------------------------------------------
// Builder: ISequencedDocumentMessage JSON -> op records (client.ts:776-836; ops.ts:29-110)
int mte_builder_create(mte_builder** out) {
    if (!out) return MTE_E_ARG;
    *out = new mte_builder();
    return MTE_OK;
}
void mte_builder_destroy(mte_builder* b) { delete b; }
const char* mte_builder_error(const mte_builder* b) { return b ? b->err.c_str() : "null builder"; }

// A JSON array of ISequencedDocumentMessage -> op records appended to `db`.
static int add_messages(mte_builder* b, const json::Value& doc, DocBuild& db) {
    std::vector<mte_op>& ops = db.ops;
    std::vector<uint16_t>& payload = db.payload;
    const bool collab = db.collab;
    auto fail = [&](int code, const std::string& m) { return db.fail(code, m); };
    if (doc.kind != json::Value::Array) return fail(MTE_E_PARSE, "op log must be a JSON array of messages");
    for (const json::Value& m : doc.items) {
        if (m.kind != json::Value::Object) return fail(MTE_E_PARSE, "message is not an object");
        mte_op base{};
        num_field(m, u"sequenceNumber", &base.seq);
        num_field(m, u"referenceSequenceNumber", &base.ref_seq);
        num_field(m, u"minimumSequenceNumber", &base.msn);
        const json::Value* cid = m.get(u"clientId");
        std::string name = (cid && cid->kind == json::Value::String) ? json::to_utf8(cid->str.data(), cid->str.size()) : "";
        if (!collab) name = "";
        uint32_t sid;
        if (int rc = db.short_id(name, &sid, base.seq)) return rc;
        base.client = (uint8_t)sid;
        const json::Value* type = m.get(u"type");
        const json::Value* contents = m.get(u"contents");
        std::vector<const json::Value*> members;
        bool isOp = type && type->kind == json::Value::String && type->str == u"op" && contents &&
                    contents->kind == json::Value::Object;
        if (isOp) {
            if (collab && sid == 0) return fail(MTE_E_UNSUPPORTED, "observer never submits ops (ack path)");
            if (db.reused && base.ref_seq < db.cur_min) base.client = 255;  // refSeq below minSeq after a reuse
            int32_t t = -1;
            num_field(*contents, u"type", &t);
            if (t == 3) {
                const json::Value* g = contents->get(u"ops");
                if (g && g->kind == json::Value::Array)
                    for (auto& x : g->items) members.push_back(&x);
            } else {
                members.push_back(contents);
            }
        }
        size_t first = ops.size();
        for (const json::Value* c : members) {
            if (c->kind != json::Value::Object) continue;
            if (c->get(u"register")) return fail(MTE_E_UNSUPPORTED, "registers are out of scope");
            mte_op o = base;
            std::u16string mkid;
            bool mapMarker = false;
            int32_t t = -1;
            num_field(*c, u"type", &t);
            num_field(*c, u"pos1", &o.pos1);
            if (t == 0) {
                const json::Value* seg = c->get(u"seg");
                if (!seg) continue;
                const json::Value* props = nullptr;
                if (db.perm) {  // PermutationSegment.fromJSONObject (permutationvector.ts:41-44): [length, start]
                    if (seg->kind != json::Value::Array || seg->items.empty() || seg->items[0].kind != json::Value::Number ||
                        seg->items[0].num < 0 || seg->items[0].num > 0x7FFFFFFF)
                        return fail(MTE_E_UNSUPPORTED, "not a PermutationSegment spec");
                    o.type = MTE_OP_INSERT;
                    o.flags |= MTE_F_PERM;  // handles reset on insert (onDelta, :302-309)
                    o.a = 0;
                    o.b = (uint32_t)seg->items[0].num;
                } else if (seg->kind == json::Value::String) {
                    o.type = MTE_OP_INSERT;
                    o.a = (int32_t)payload.size();
                    o.b = (uint32_t)seg->str.size();
                    payload.insert(payload.end(), seg->str.begin(), seg->str.end());
                } else if (seg->kind == json::Value::Object && seg->get(u"marker")) {
                    o.type = MTE_OP_INSERT_MARKER;
                    const json::Value* mk = seg->get(u"marker");
                    int32_t rt = 0;
                    if (mk->kind == json::Value::Object) num_field(*mk, u"refType", &rt);
                    if (rt < 0 || rt > 0xFFFF) return fail(MTE_E_UNSUPPORTED, "refType beyond 16 bits");
                    o.b = (uint32_t)rt;
                    props = seg->get(u"props");
                    mapMarker = marker_id(props, &mkid);
                } else if (seg->kind == json::Value::Object && seg->get(u"text") &&
                           seg->get(u"text")->kind == json::Value::String) {
                    const json::Value* tx = seg->get(u"text");
                    o.type = MTE_OP_INSERT;
                    o.a = (int32_t)payload.size();
                    o.b = (uint32_t)tx->str.size();
                    payload.insert(payload.end(), tx->str.begin(), tx->str.end());
                    props = seg->get(u"props");
                } else {
                    return fail(MTE_E_UNSUPPORTED, "unknown segment spec");
                }
                if (props && json::truthy(props)) {
                    if (props->kind != json::Value::Object) return fail(MTE_E_UNSUPPORTED, "non-object props");
                    o.props = b->in->propset(*props);
                }
            } else if (t == 1) {
                o.type = MTE_OP_REMOVE;
                num_field(*c, u"pos2", &o.a);
            } else if (t == 2) {
                o.type = MTE_OP_ANNOTATE;
                num_field(*c, u"pos2", &o.a);
                const json::Value* props = c->get(u"props");
                const json::Value* comb = c->get(u"combiningOp");
                if (comb) {
                    const json::Value* nm = comb->kind == json::Value::Object ? comb->get(u"name") : nullptr;
                    if (nm && nm->kind == json::Value::String && nm->str == u"rewrite") o.flags |= MTE_F_REWRITE;
                    else return fail(MTE_E_UNSUPPORTED, "combiningOp other than rewrite is out of scope");
                }
                json::Value empty;
                empty.kind = json::Value::Object;
                o.props = b->in->propset(props && props->kind == json::Value::Object ? *props : empty);
            } else {
                continue;
            }
            // relativePos1 / relativePos2 where pos1 / pos2 is undefined (client.ts:493-510): a RELPOS
            // record before the op (an insert uses only its start)
            const json::Value* rp1 = c->get(u"relativePos1");
            const json::Value* rp2 = c->get(u"relativePos2");
            const bool r1 = rp1 && json::truthy(rp1) && !c->get(u"pos1");
            const bool r2 = t != 0 && rp2 && json::truthy(rp2) && !c->get(u"pos2");
            if (r1 || r2) {
                mte_op r = base;
                r.type = MTE_OP_RELPOS;
                r.flags = 0;
                r.props = 0;
                r.msn = 0;
                bool before = false;
                int32_t off = 0;
                if (r1) {
                    r.pos1 = (int32_t)db.rel_tag(*rp1, &off, &before);
                    r.msn = off;
                    if (before) r.flags |= MTE_F_REL_BEFORE1;
                }
                if (r2) {
                    r.a = (int32_t)db.rel_tag(*rp2, &off, &before);
                    r.props = (uint32_t)off;
                    if (before) r.flags |= MTE_F_REL_BEFORE2;
                }
                ops.push_back(r);
                o.flags |= MTE_F_REL;
            }
            if (mapMarker) db.map_marker(mkid, &o.b);  // after the op's own position (insertSegments)
            if (t == 2) {
                const json::Value* ap = c->get(u"props");
                if (ap && ap->kind == json::Value::Object && ap->get(u"markerId")) db.mk_annot = true;
            }
            ops.push_back(o);
        }
        if (ops.size() == first) {  // no merge-tree op: still a sequenced message
            mte_op o = base;
            o.type = MTE_OP_NOOP;
            ops.push_back(o);
        }
        ops.back().flags |= MTE_F_END_OF_MSG;
        if (collab && base.msn > db.cur_min) db.cur_min = base.msn;  // setMinSeq after the message
        if (collab && type && type->kind == json::Value::String && type->str == u"op") {
            db.stash.push_back(DocBuild::Msg{base.seq, base.ref_seq != base.seq - 1, (uint64_t)first, json::stringify(m)});
            if (db.stash.size() > 64) db.trim_stash();
        }
    }
    return MTE_OK;
}

// documents are added before the first open one (mte_builder_open_doc): a batch lists the committed
// documents, then the open ones
static int builder_closed(mte_builder* b) {
    b->err = "documents cannot be added after an open document (mte_builder_open_doc)";
    return MTE_E_STATE;
}

int mte_builder_add_doc(mte_builder* b, const char* observer_name, const char* text, size_t len) {
    if (!b || !text) return MTE_E_ARG;
    if (!b->open.empty()) return builder_closed(b);
    json::Value doc;
    try {
        doc = json::parse(text, len);
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    DocBuild db(observer_name);
    if (int rc = add_messages(b, doc, db)) {
        b->err = db.err;
        return rc;
    }
    db.commit(b->hb);
    b->paths.emplace_back();
    return MTE_OK;
}

// ------------------------------------------------------------------------------------------------
// Resume from a summary: SnapshotLoader (snapshotLoader.ts:38-216) as LOAD records (include/mte.h).

// A segment spec (sequenceFactory.ts:31-37: string | {text, props} | {marker, props}) -> o.a/o.b/props.
static int load_spec(mte_builder* b, DocBuild& db, const json::Value& seg, mte_op& o, std::u16string* mkid = nullptr,
                     bool* hasId = nullptr) {
    const json::Value* props = nullptr;
    if (db.perm) {  // PermutationSegment.fromJSONObject (permutationvector.ts:41-44): [length, start]
        if (seg.kind != json::Value::Array || seg.items.empty() || seg.items[0].kind != json::Value::Number ||
            seg.items[0].num < 0 || seg.items[0].num > 0x7FFFFFFF)
            return db.fail(MTE_E_UNSUPPORTED, "not a PermutationSegment spec");
        const double st = seg.items.size() > 1 && seg.items[1].kind == json::Value::Number ? seg.items[1].num : -2147483648.0;
        if (st >= 1 && (st > 0x7FFFFFFF || st != (double)(int32_t)st)) return db.fail(MTE_E_UNSUPPORTED, "start handle");
        o.b = (uint32_t)seg.items[0].num;
        o.a = st >= 1 ? (int32_t)st : 0;  // a loaded run keeps its handles (no onDelta reset on load)
        o.flags |= MTE_F_PERM;
        return MTE_OK;
    }
    if (seg.kind == json::Value::String) {
        o.a = (int32_t)db.payload.size();
        o.b = (uint32_t)seg.str.size();
        db.payload.insert(db.payload.end(), seg.str.begin(), seg.str.end());
    } else if (seg.kind == json::Value::Object && seg.get(u"marker")) {
        const json::Value* mk = seg.get(u"marker");
        int32_t rt = 0;
        if (mk->kind == json::Value::Object) num_field(*mk, u"refType", &rt);
        if (rt < 0 || rt > 0xFFFF) return db.fail(MTE_E_UNSUPPORTED, "refType beyond 16 bits");
        o.a = rt;
        o.b = 1;
        o.flags |= MTE_F_LOAD_MARKER;
        props = seg.get(u"props");
        if (mkid && hasId) *hasId = marker_id(props, mkid);
    } else if (seg.kind == json::Value::Object && seg.get(u"text") && seg.get(u"text")->kind == json::Value::String) {
        const json::Value* tx = seg.get(u"text");
        o.a = (int32_t)db.payload.size();
        o.b = (uint32_t)tx->str.size();
        db.payload.insert(db.payload.end(), tx->str.begin(), tx->str.end());
        props = seg.get(u"props");
    } else {
        return db.fail(MTE_E_UNSUPPORTED, "unknown segment spec");
    }
    if (props && json::truthy(props)) {
        if (props->kind != json::Value::Object) return db.fail(MTE_E_UNSUPPORTED, "non-object props");
        o.props = b->in->propset(*props);
    }
    return MTE_OK;
}

static const json::Value* tree_entry(const json::Value& tree, const char16_t* path) {
    const json::Value* es = tree.kind == json::Value::Object ? tree.get(u"entries") : nullptr;
    if (!es || es->kind != json::Value::Array) return nullptr;
    for (const json::Value& e : es->items) {
        const json::Value* p = e.kind == json::Value::Object ? e.get(u"path") : nullptr;
        if (p && p->kind == json::Value::String && p->str == path) return &e;
    }
    return nullptr;
}

// toLatestVersion for a legacy chunk (snapshotChunks.ts:135-176): segmentTexts -> segments, and for
// the header the metadata it carries or buildHeaderMetadataForLegecyChunk's (a "body" chunk when the
// header holds fewer chars than the document).
static int legacy_to_v1(const std::u16string& path, json::Value& c) {
    json::Value v1;
    v1.kind = json::Value::Object;
    v1.members.emplace_back(u"version", jstr(u"1"));
    for (auto& m : c.members) {
        if (m.first == u"segmentTexts") v1.members.emplace_back(u"segments", m.second);
        else if (m.first == u"headerMetadata") v1.members.emplace_back(u"headerMetadata", m.second);
    }
    if (path == u"header" && !c.get(u"headerMetadata")) {
        json::Value md, ids;
        md.kind = json::Value::Object;
        ids.kind = json::Value::Array;
        auto id = [&](const char16_t* n) {
            json::Value o;
            o.kind = json::Value::Object;
            o.members.emplace_back(u"id", jstr(n));
            ids.items.push_back(o);
        };
        id(u"header");
        const json::Value* cl = c.get(u"chunkLengthChars");
        const json::Value* tl = c.get(u"totalLengthChars");
        if (cl && tl && cl->num < tl->num) id(u"body");
        md.members.emplace_back(u"orderedChunkMetadata", ids);
        if (const json::Value* m = c.get(u"chunkMinSequenceNumber")) md.members.emplace_back(u"minSequenceNumber", *m);
        if (const json::Value* q = c.get(u"chunkSequenceNumber")) md.members.emplace_back(u"sequenceNumber", *q);
        if (tl) md.members.emplace_back(u"totalLength", *tl);
        if (const json::Value* ts = c.get(u"totalSegmentCount")) md.members.emplace_back(u"totalSegmentCount", *ts);
        v1.members.emplace_back(u"headerMetadata", md);
    }
    c = v1;
    return MTE_OK;
}

// Buffer.toString("utf8") of the decoded base64 bytes (fromBase64ToUtf8, common-utils
// base64Encoding.ts): the WHATWG UTF-8 decoder, each maximal invalid subpart becomes U+FFFD.
// Re-encoded as UTF-8 for the JSON parser.
static std::string utf8_replace_invalid(const std::string& in) {
    std::string out;
    out.reserve(in.size());
    auto put = [&](u32 cp) {
        if (cp < 0x80) {
            out.push_back((char)cp);
        } else if (cp < 0x800) {
            out.push_back((char)(0xC0 | (cp >> 6)));
            out.push_back((char)(0x80 | (cp & 0x3F)));
        } else if (cp < 0x10000) {
            out.push_back((char)(0xE0 | (cp >> 12)));
            out.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
            out.push_back((char)(0x80 | (cp & 0x3F)));
        } else {
            out.push_back((char)(0xF0 | (cp >> 18)));
            out.push_back((char)(0x80 | ((cp >> 12) & 0x3F)));
            out.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
            out.push_back((char)(0x80 | (cp & 0x3F)));
        }
    };
    u32 need = 0, seen = 0, cp = 0, lo = 0x80, hi = 0xBF;
    for (size_t i = 0; i < in.size();) {
        const u32 b = (unsigned char)in[i];
        if (need == 0) {
            i++;
            if (b < 0x80) put(b);
            else if (b >= 0xC2 && b <= 0xDF) { need = 1; cp = b & 0x1F; }
            else if (b >= 0xE0 && b <= 0xEF) { if (b == 0xE0) lo = 0xA0; if (b == 0xED) hi = 0x9F; need = 2; cp = b & 0xF; }
            else if (b >= 0xF0 && b <= 0xF4) { if (b == 0xF0) lo = 0x90; if (b == 0xF4) hi = 0x8F; need = 3; cp = b & 0x7; }
            else put(0xFFFD);
            continue;
        }
        if (b < lo || b > hi) {  // the byte starts over (not consumed)
            need = seen = cp = 0;
            lo = 0x80;
            hi = 0xBF;
            put(0xFFFD);
            continue;
        }
        i++;
        lo = 0x80;
        hi = 0xBF;
        cp = (cp << 6) | (b & 0x3F);
        if (++seen == need) {
            put(cp);
            need = seen = cp = 0;
        }
    }
    if (need) put(0xFFFD);
    return out;
}

// An ITree blob's text (IBlob { contents, encoding: "utf-8" | "base64" }): what storage.read(path) +
// fromBase64ToUtf8 give the loader (snapshotV1.ts:255,267; snapshotLoader.ts:225). Base64 as Node's
// Buffer.from(s, "base64") reads it: standard or url-safe alphabet, whitespace skipped, '=' ends the
// data. Returns 0, or -1 for a missing blob, -2 for an unknown encoding, -3 for a bad character.
static int blob_utf8(const json::Value* v, std::string& out) {
    const json::Value* c = v && v->kind == json::Value::Object ? v->get(u"contents") : nullptr;
    const json::Value* enc = v && v->kind == json::Value::Object ? v->get(u"encoding") : nullptr;
    if (!c || c->kind != json::Value::String) return -1;
    if (!enc || (enc->kind == json::Value::String && enc->str == u"utf-8")) {
        out = json::to_utf8(c->str.data(), c->str.size());
        return 0;
    }
    if (!(enc->kind == json::Value::String && enc->str == u"base64")) return -2;
    out.clear();
    u32 acc = 0, nb = 0;
    for (char16_t ch : c->str) {
        int d;
        if (ch >= u'A' && ch <= u'Z') d = ch - u'A';
        else if (ch >= u'a' && ch <= u'z') d = ch - u'a' + 26;
        else if (ch >= u'0' && ch <= u'9') d = ch - u'0' + 52;
        else if (ch == u'+' || ch == u'-') d = 62;
        else if (ch == u'/' || ch == u'_') d = 63;
        else if (ch == u'=') break;
        else if (ch == u' ' || ch == u'\n' || ch == u'\r' || ch == u'\t') continue;
        else return -3;
        acc = (acc << 6) | (u32)d;
        nb += 6;
        if (nb >= 8) {
            nb -= 8;
            out.push_back((char)((acc >> nb) & 0xff));
        }
    }
    out = utf8_replace_invalid(out);
    return 0;
}
static int blob_text(DocBuild& db, const json::Value* v, std::string& out, const char* missing) {
    switch (blob_utf8(v, out)) {
        case 0: return MTE_OK;
        case -1: return db.fail(MTE_E_PARSE, missing);
        case -2: return db.fail(MTE_E_UNSUPPORTED, "blob encoding other than utf-8 / base64");
        default: return db.fail(MTE_E_PARSE, "bad base64 blob contents");
    }
}

// storage.read(path) + SnapshotV1.processChunk (snapshotV1.ts:249-270)
static int load_chunk(DocBuild& db, const json::Value& tree, const std::u16string& path, json::Value* out) {
    const json::Value* e = tree_entry(tree, path.c_str());
    const json::Value* v = e ? e->get(u"value") : nullptr;
    std::string text;
    if (int rc = blob_text(db, v, text, "summary blob missing")) return rc;
    try {
        *out = json::parse(text.data(), text.size());
    } catch (std::exception& ex) {
        return db.fail(MTE_E_PARSE, ex.what());
    }
    const json::Value* ver = out->kind == json::Value::Object ? out->get(u"version") : nullptr;
    if (!ver && out->kind == json::Value::Object && out->get(u"segmentTexts")) return legacy_to_v1(path, *out);
    if (!ver || ver->kind != json::Value::String || ver->str != u"1")
        return db.fail(MTE_E_UNSUPPORTED, "unsupported snapshot chunk version");
    return MTE_OK;
}

// NonCollabClient (constants.ts) as a short id: the name getLongClientId gives it (client.ts:653-659).
// SnapshotV1 never emits it: universal segments carry no merge info (snapshotV1.ts:219-223).
static const char* const kNonCollabName = "original";

// One summary segment spec -> a LOAD_SEG-shaped record (SnapshotLoader.specToSegment,
// snapshotLoader.ts:79-111): merge info gives client / seq / removedSeq / removedClient; a bare spec,
// or merge info without client and seq, is NonCollab at the universal seq (*batchable: loadBody's
// flushBatch test, :193-195).
struct MarkerId {  // a summary marker's Marker.getId, tagged when the record is emitted
    bool has = false;
    std::u16string id;
};
static int summary_seg(mte_builder* b, DocBuild& db, const json::Value& sp, mte_op& o, bool* info, bool* batchable,
                       MarkerId* mid) {
    const json::Value* js = sp.kind == json::Value::Object ? sp.get(u"json") : nullptr;  // hasMergeInfo
    if (int rc = load_spec(b, db, js ? *js : sp, o, &mid->id, &mid->has)) return rc;
    std::string client = kNonCollabName;
    bool hasClient = false, hasSeq = false;
    if (js) {
        const json::Value* c = sp.get(u"client");
        if (c && c->kind == json::Value::String) {
            client = json::to_utf8(c->str.data(), c->str.size());
            hasClient = true;
        }
        hasSeq = num_field(sp, u"seq", &o.seq) != 0;
    }
    uint32_t cid;
    if (int rc = db.short_id(client, &cid, o.seq)) return rc;
    o.client = (uint8_t)cid;
    if (js && num_field(sp, u"removedSeq", &o.ref_seq)) {
        o.flags |= MTE_F_LOAD_REMOVED;
        const json::Value* rc = sp.get(u"removedClient");
        std::string rn = rc && rc->kind == json::Value::String ? json::to_utf8(rc->str.data(), rc->str.size())
                                                               : kNonCollabName;
        uint32_t rid;
        if (int e = db.short_id(rn, &rid, o.ref_seq)) return e;
        o.pos1 = (int32_t)rid;
    }
    *info = js != nullptr;
    *batchable = !hasClient && (!hasSeq || o.seq == 0);
    return MTE_OK;
}

static int add_summary(mte_builder* b, const json::Value& summary, DocBuild& db) {
    if (!db.collab) return db.fail(MTE_E_ARG, "a summary is loaded by a collaborating client (observer name)");
    db.loading = true;  // no short-id reuse inside the load records
    const json::Value* t = &summary;
    const json::Value* content = tree_entry(summary, u"content");
    if (content && content->get(u"value")) t = content->get(u"value");  // SharedString summary (sequence.ts:413-438)
    json::Value header;
    if (int rc = load_chunk(db, *t, u"header", &header)) return rc;
    const json::Value* md = header.get(u"headerMetadata");
    if (!md || md->kind != json::Value::Object) return db.fail(MTE_E_PARSE, "header metadata not available");
    bool mergeInfo = false;
    const size_t first = db.ops.size();
    const json::Value* hs = header.get(u"segments");
    if (hs && hs->kind == json::Value::Array) {
        for (const json::Value& sp : hs->items) {
            mte_op o{};
            o.type = MTE_OP_LOAD_SEG;
            bool info, batchable;
            MarkerId mid;
            if (int rc = summary_seg(b, db, sp, o, &info, &batchable, &mid)) return rc;
            mergeInfo |= info;
            // reloadFromSegments maps the live markers (blockUpdate -> addNodeReferences, mergeTree.ts:275-284)
            if (mid.has && !(o.flags & MTE_F_LOAD_REMOVED)) {
                uint32_t w = (uint32_t)o.a;
                db.map_marker(mid.id, &w);
                o.a = (int32_t)w;
            }
            db.ops.push_back(o);
        }
    }
    const size_t nHeader = db.ops.size() - first;
    // loadBody (:150-216): nothing when the header holds every segment (:159-161; the shipAsserts on
    // the lengths only log, :152-157, :176-182); otherwise every later chunk's segments in order
    const json::Value* ocm = md->get(u"orderedChunkMetadata");
    int32_t segCount = -1, totalSegs = -2;
    num_field(header, u"segmentCount", &segCount);
    num_field(*md, u"totalSegmentCount", &totalSegs);
    std::vector<mte_op> body;
    std::vector<uint8_t> bodyBatchable;
    std::vector<MarkerId> bodyIds;
    if (segCount != totalSegs && ocm && ocm->kind == json::Value::Array) {
        for (size_t i = 1; i < ocm->items.size(); i++) {
            const json::Value* id = ocm->items[i].kind == json::Value::Object ? ocm->items[i].get(u"id") : nullptr;
            if (!id || id->kind != json::Value::String) return db.fail(MTE_E_PARSE, "chunk id");
            json::Value ch;
            if (int rc = load_chunk(db, *t, id->str, &ch)) return rc;
            const json::Value* cs = ch.get(u"segments");
            if (!cs || cs->kind != json::Value::Array) continue;
            for (const json::Value& sp : cs->items) {
                mte_op o{};
                bool info, batchable;
                MarkerId mid;
                if (int rc = summary_seg(b, db, sp, o, &info, &batchable, &mid)) return rc;
                mergeInfo |= info;
                body.push_back(o);
                bodyBatchable.push_back(batchable ? 1 : 0);
                bodyIds.push_back(std::move(mid));
            }
        }
    }
    // Without merge info every body segment is NonCollab at seq 0 and loadBody is ONE append at the
    // document end: LOAD_SEG records whose tree shape the builder computes below. With merge info,
    // the appends go through the insert walk on the device (LOAD_APPEND after LOAD_END), in the
    // order loadBody issues them.
    // The appended markers are mapped by insertSegments (blockInsert, mergeTree.ts:2199-2205).
    auto tag_body = [&](size_t i, mte_op& o) {
        if (!bodyIds[i].has) return;
        uint32_t w = (uint32_t)o.a;
        db.map_marker(bodyIds[i].id, &w);
        o.a = (int32_t)w;
    };
    if (!mergeInfo) {
        for (size_t i = 0; i < body.size(); i++) {
            mte_op o = body[i];
            if (o.b == 0) continue;  // blockInsert skips empty segments (mergeTree.ts:2196)
            o.type = MTE_OP_LOAD_SEG;
            o.flags |= MTE_F_LOAD_BODY;
            tag_body(i, o);
            db.ops.push_back(o);
        }
    }
    // The loaded tree's shape (child counts per level, document order): reloadFromSegments packs the
    // header 7 to a block, level by level; each body append then lands at the end of the last leaf
    // (insertingWalk at the document end) and a block reaching 8 children splits 4+4 up to the root
    // (mergeTree.ts:2446-2489, 1876-1887). Segment ids and text are not part of the shape.
    std::vector<std::vector<uint32_t>> lv(1);
    for (size_t i = 0; i < nHeader; i += 7) lv[0].push_back((uint32_t)std::min<size_t>(7, nHeader - i));
    if (lv[0].empty()) lv[0].push_back(0);
    while (lv.back().size() > 1) {
        const size_t m = lv.back().size();
        std::vector<uint32_t> up;
        for (size_t i = 0; i < m; i += 7) up.push_back((uint32_t)std::min<size_t>(7, m - i));
        lv.push_back(up);
    }
    for (size_t k = first + nHeader; k < db.ops.size(); k++) {
        size_t l = 0;
        for (lv[0].back()++; l < lv.size() && lv[l].back() == 8; l++) {
            lv[l].back() = 4;
            lv[l].push_back(4);
            if (l + 1 == lv.size()) lv.push_back({2});  // the root split: updateRoot
            else lv[l + 1].back()++;
        }
    }
    // leaf boundaries onto the LOAD_SEG records
    size_t k = first;
    for (size_t leaf = 0; leaf < lv[0].size(); leaf++) {
        if (leaf > 0 && k < db.ops.size()) db.ops[k].flags |= MTE_F_LOAD_LEAF;
        k += lv[0][leaf];
    }
    if (k != db.ops.size()) return db.fail(MTE_E_PARSE, "loaded tree shape does not cover the segments");
    uint32_t nodes = 0;
    for (size_t l = 1; l < lv.size(); l++)
        for (uint32_t c : lv[l]) {
            mte_op o{};
            o.type = MTE_OP_LOAD_NODE;
            o.a = (int32_t)l;
            o.b = c;
            db.ops.push_back(o);
            nodes++;
        }
    mte_op end{};
    end.type = MTE_OP_LOAD_END;
    end.a = (int32_t)nodes;
    num_field(*md, u"sequenceNumber", &end.seq);
    end.msn = end.seq;
    num_field(*md, u"minSequenceNumber", &end.msn);
    db.ops.push_back(end);
    if (mergeInfo && !body.empty()) {
        // loadBody's appends (:184-213): a batchable segment joins `batch`; any other flushes the batch
        // (append at root.cachedLength, NonCollab, seq 0) and is appended alone with its own client and
        // seq. flushBatch never clears `batch` (:196-199): each later flush appends every earlier
        // batched segment object again (MTE_F_APPEND_REPEAT) before the new ones.
        std::vector<size_t> batch;
        std::vector<uint8_t> linked(body.size(), 0);
        auto emit = [&](size_t i, bool firstOfCall, uint32_t client, int32_t seq) {
            if (body[i].b == 0) return;  // blockInsert skips empty segments: no walk, no position
            mte_op o = body[i];
            o.type = MTE_OP_LOAD_APPEND;
            o.client = (uint8_t)client;
            o.seq = seq;
            o.flags = (uint16_t)(o.flags & (MTE_F_LOAD_MARKER | MTE_F_LOAD_REMOVED | MTE_F_PERM));
            if (firstOfCall) o.flags |= MTE_F_APPEND_FIRST;
            if (linked[i]) o.flags |= MTE_F_APPEND_REPEAT;
            else tag_body(i, o);  // a repeat is the same object: mapped already
            linked[i] = 1;
            db.ops.push_back(o);
        };
        uint32_t nc;
        if (int rc = db.short_id(kNonCollabName, &nc)) return rc;
        auto flush = [&]() {
            bool firstOfCall = true;
            for (size_t i : batch) {
                const size_t before = db.ops.size();
                emit(i, firstOfCall, nc, 0);
                firstOfCall &= db.ops.size() == before;
            }
        };
        for (size_t i = 0; i < body.size(); i++) {
            if (bodyBatchable[i]) {
                batch.push_back(i);
            } else {
                flush();
                emit(i, true, body[i].client, body[i].seq);
            }
        }
        flush();
    }
    db.loading = false;
    db.cur_min = std::max(db.cur_min, end.msn);  // startOrUpdateCollaboration(minSeq)
    // loadBodyAndCatchupOps (snapshotLoader.ts:55-77): one blob beyond the chunks holds catch-up
    // messages (legacy summaries), applied after the load like any sequenced message; any other blob
    // count is an error
    const json::Value* es = t->get(u"entries");
    size_t nChunks = ocm && ocm->kind == json::Value::Array ? ocm->items.size() : 1, nBlobs = 0;
    const json::Value* extra = nullptr;
    static const std::vector<json::Value> none;
    for (const json::Value& e : es ? es->items : none) {  // (a reference: `extra` points into it)
        const json::Value* ty = e.get(u"type");
        const json::Value* pth = e.get(u"path");
        if (!ty || ty->kind != json::Value::String || ty->str != u"Blob" || !pth) continue;
        nBlobs++;
        bool isChunk = false;
        for (size_t i = 0; ocm && ocm->kind == json::Value::Array && i < ocm->items.size(); i++) {
            const json::Value* id = ocm->items[i].get(u"id");
            isChunk |= id && id->kind == json::Value::String && id->str == pth->str;
        }
        if (!isChunk) extra = &e;
    }
    if (nBlobs == nChunks + 1 && extra) {
        std::string text;
        if (int rc = blob_text(db, extra->get(u"value"), text, "catch-up ops blob")) return rc;
        json::Value msgs;
        try {
            msgs = json::parse(text.data(), text.size());
        } catch (std::exception& ex) {
            return db.fail(MTE_E_PARSE, ex.what());
        }
        if (int rc = add_messages(b, msgs, db)) return rc;
    } else if (nBlobs != nChunks) {
        return db.fail(MTE_E_PARSE, "Unexpected blobs in snapshot");
    }
    return MTE_OK;
}

int mte_builder_add_doc_from_summary(mte_builder* b, const char* observer_name, const char* summary,
                                     size_t summary_len, const char* ops, size_t ops_len) {
    if (!b || !summary) return MTE_E_ARG;
    if (!b->open.empty()) return builder_closed(b);
    DocBuild db(observer_name);
    json::Value s, log;
    try {
        s = json::parse(summary, summary_len);
        if (ops) log = json::parse(ops, ops_len);
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    int rc = add_summary(b, s, db);
    if (!rc && ops) rc = add_messages(b, log, db);
    if (rc) {
        b->err = db.err;
        return rc;
    }
    db.commit(b->hb);
    b->paths.emplace_back();
    return MTE_OK;
}

// ------------------------------------------------------------------------------------------------
// Container-level op logs (clientReplayTool.ts:113-192, 258-347; fileDeltaStorageService.ts:23-31).

static const char16_t* const kSharedStringType = u"https://graph.microsoft.com/types/mergeTree";  // SharedStringFactory.Type

static std::string u8(const std::u16string& s) { return json::to_utf8(s.data(), s.size()); }

// getDssTreesFromAttach + processAttachMessage: every SharedString tree of an attach snapshot, by
// full path (the attach id, then "/"-joined tree entry paths). Later attaches of a path replace it.
static void attach_trees(const json::Value& attach, const std::string& id, std::deque<json::Value>& store,
                         std::vector<std::pair<std::string, const json::Value*>>& out) {
    const json::Value* snap = attach.get(u"snapshot");
    if (!snap || snap->kind != json::Value::Object) return;
    store.push_back(*snap);
    auto put = [&](const std::string& path, const json::Value* tree) {
        for (auto& o : out)
            if (o.first == path) {
                o.second = tree;
                return;
            }
        out.emplace_back(path, tree);
    };
    const json::Value* ty = attach.get(u"type");
    if (ty && ty->kind == json::Value::String && ty->str == kSharedStringType) put(id, &store.back());
    std::deque<std::pair<std::string, const json::Value*>> q{{id, &store.back()}};
    while (!q.empty()) {
        auto [full, tree] = q.front();
        q.pop_front();
        const json::Value* es = tree->get(u"entries");
        if (!es || es->kind != json::Value::Array) continue;
        for (const json::Value& e : es->items) {
            const json::Value* t = e.get(u"type");
            const json::Value* p = e.get(u"path");
            const json::Value* v = e.get(u"value");
            if (!t || t->kind != json::Value::String || !p || p->kind != json::Value::String || !v) continue;
            if (t->str == u"Tree") {
                q.emplace_back(full + "/" + u8(p->str), v);
            } else if (t->str == u"Blob" && p->str == u".attributes") {
                std::string at_text;
                if (blob_utf8(v, at_text)) continue;
                try {
                    json::Value a = json::parse(at_text.c_str(), at_text.size());
                    const json::Value* at = a.get(u"type");
                    if (at && at->kind == json::Value::String && at->str == kSharedStringType) put(full, tree);
                } catch (std::exception&) {
                }
            }
        }
    }
}

int mte_builder_add_container_log(mte_builder* b, const char* observer_name, const char* text, size_t len,
                                  uint32_t* n_docs) {
    if (!b || !text) return MTE_E_ARG;
    if (!b->open.empty()) return builder_closed(b);
    if (n_docs) *n_docs = 0;
    json::Value log;
    try {
        log = json::parse(text, len);
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    if (log.kind != json::Value::Array) {
        b->err = "container log must be a JSON array of messages";
        return MTE_E_PARSE;
    }
    std::deque<json::Value> store;                                   // attach snapshots / parsed strings
    std::vector<std::pair<std::string, const json::Value*>> trees;   // mergeTreeAttachTrees (insertion order)
    std::unordered_map<std::string, std::vector<json::Value>> msgs;  // merge-tree messages by full path
    // ChunkedOp parts per client (clientReplayTool.ts:118-141: any order, each index once)
    std::unordered_map<std::string, std::pair<std::vector<std::u16string>, std::vector<bool>>> chunks;
    std::vector<uint8_t> have;
    auto parse_str = [&](const std::u16string& s) -> const json::Value* {
        const std::string t = u8(s);
        store.push_back(json::parse(t.data(), t.size()));
        return &store.back();
    };
    try {
        for (const json::Value& m0 : log.items) {
            if (m0.kind != json::Value::Object) continue;
            json::Value m = m0;
            const json::Value* ty = m.get(u"type");
            const json::Value* cid = m.get(u"clientId");
            const std::string client = cid && cid->kind == json::Value::String ? u8(cid->str) : "";
            if (ty && ty->kind == json::Value::String && ty->str == u"chunkedOp") {  // ChunkedOp reassembly
                const json::Value* c = m.get(u"contents");
                const json::Value* ch = c && c->kind == json::Value::String ? parse_str(c->str) : c;
                if (!ch || ch->kind != json::Value::Object) continue;
                int32_t id = 0, total = 0;
                num_field(*ch, u"chunkId", &id);
                num_field(*ch, u"totalChunks", &total);
                const json::Value* part = ch->get(u"contents");
                if (total <= 0 || id < 1 || id > total) throw std::runtime_error("chunk id out of range");
                auto& pending = chunks[client];  // (texts, assigned) by chunk index
                if (pending.first.empty()) {
                    pending.first.assign((size_t)total, std::u16string());
                    pending.second.assign((size_t)total, false);
                }
                if ((size_t)id > pending.first.size()) throw std::runtime_error("chunk id out of range");
                if (pending.second[(size_t)(id - 1)]) throw std::runtime_error("Chunk already assigned");
                pending.second[(size_t)(id - 1)] = true;
                pending.first[(size_t)(id - 1)] = part && part->kind == json::Value::String ? part->str : std::u16string();
                if (id != total) continue;
                std::u16string joined;
                for (size_t q = 0; q < pending.first.size(); q++) {
                    if (!pending.second[q]) throw std::runtime_error("Chunk not assigned");
                    joined += pending.first[q];
                }
                chunks.erase(client);
                // `ch` may point into m's own "contents" member (object-form chunks): copy what is
                // needed from it before m's members are rewritten
                const json::Value* origp = ch->get(u"originalType");
                const bool hasOrig = origp != nullptr;
                const json::Value orig = hasOrig ? *origp : json::Value();
                for (auto& mem : m.members) {
                    if (mem.first == u"contents") {
                        json::Value joinedv;
                        joinedv.kind = json::Value::String;
                        joinedv.str = joined;
                        mem.second = std::move(joinedv);
                    } else if (mem.first == u"type" && hasOrig) {
                        mem.second = orig;
                    }
                }
                ty = m.get(u"type");
            }
            if (!ty || ty->kind != json::Value::String) continue;
            const json::Value* contents = m.get(u"contents");
            if (ty->str == u"attach") {  // ContainerMessageType.Attach
                const json::Value* a = contents && contents->kind == json::Value::String ? parse_str(contents->str) : contents;
                const json::Value* id = a ? a->get(u"id") : nullptr;
                if (a && id && id->kind == json::Value::String) attach_trees(*a, u8(id->str), store, trees);
                continue;
            }
            if (ty->str != u"op" || !contents || contents->kind == json::Value::Null) continue;
            // address envelopes: {address, contents: {address, contents: ...}}
            std::vector<std::string> parts;
            const json::Value* cur = contents;
            do {
                if (cur->kind == json::Value::String) cur = parse_str(cur->str);
                const json::Value* ad = cur->get(u"address");
                parts.push_back(ad && ad->kind == json::Value::String ? u8(ad->str) : "undefined");
                cur = cur->get(u"contents");
                if (!cur) break;
            } while (cur->get(u"contents"));
            if (!cur) continue;
            auto join = [&](const std::string& last) {
                std::string o;
                for (auto& x : parts) o += x + "/";
                return o + last;
            };
            const json::Value* ity = cur->get(u"type");
            if (ity && ity->kind == json::Value::String && ity->str == u"attach") {  // legacy attach envelope
                const json::Value* a = cur->get(u"content");
                const json::Value* id = a ? a->get(u"id") : nullptr;
                if (a && id && id->kind == json::Value::String) attach_trees(*a, join(u8(id->str)), store, trees);
                continue;
            }
            const json::Value* content = cur->get(u"content");
            if (!content || content->kind != json::Value::Object) continue;
            const json::Value* ad = content->get(u"address");
            const std::string path = join(ad && ad->kind == json::Value::String ? u8(ad->str) : "undefined");
            bool known = false;
            for (auto& t : trees) known |= t.first == path;
            const json::Value* op = content->get(u"contents");
            if (!known || !op || op->kind != json::Value::Object || op->get(u"key")) continue;  // interval ops: "key"
            json::Value nm = m;
            for (auto& mem : nm.members)
                if (mem.first == u"contents") mem.second = *op;
            msgs[path].push_back(std::move(nm));
        }
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    uint32_t added = 0;
    // every channel's document is built before any is committed: a failing channel leaves the
    // builder as it was (interned property sets aside, which no document references)
    std::vector<std::unique_ptr<DocBuild>> built;
    for (auto& [path, tree] : trees) {
        built.emplace_back(new DocBuild(observer_name));
        DocBuild& db = *built.back();
        json::Value arr;
        arr.kind = json::Value::Array;
        auto it = msgs.find(path);
        if (it != msgs.end()) arr.items = std::move(it->second);
        int rc = add_summary(b, *tree, db);
        if (!rc) rc = add_messages(b, arr, db);
        if (rc) {
            b->err = path + ": " + db.err;
            return rc;
        }
    }
    for (size_t i = 0; i < built.size(); i++) {
        built[i]->commit(b->hb);
        b->paths.push_back(trees[i].first);
        added++;
    }
    if (n_docs) *n_docs = added;
    return MTE_OK;
}

const char* mte_builder_doc_path(const mte_builder* b, uint32_t doc) {
    return b && doc < b->paths.size() ? b->paths[doc].c_str() : nullptr;
}

// SharedMatrix.processCore (matrix.ts:548-560): rows then cols, each PermutationVector fed the
// messages that target it; a cell op (no target) becomes an MTE_OP_CELL record in both, in message order.
// SharedMatrix.processCore (matrix.ts:548-560) of a message log into the rows / cols documents: the
// messages that target a vector go to it; a cell op (no target) becomes an MTE_OP_CELL record in both,
// in message order.
static int matrix_messages(mte_builder* b, const json::Value& log, DocBuild* dbs[2], uint32_t& cells) {
    auto fail = [&](int code, const std::string& m) {
        b->err = m;
        return code;
    };
    json::Value one;
    one.kind = json::Value::Array;
    one.items.resize(1);
    for (const json::Value& m : log.items) {
        const json::Value* c = m.kind == json::Value::Object ? m.get(u"contents") : nullptr;
        const json::Value* t = c && c->kind == json::Value::Object ? c->get(u"target") : nullptr;
        if (t) {
            const int i = t->kind != json::Value::String ? -1 : t->str == u"rows" ? 0 : t->str == u"cols" ? 1 : -1;
            if (i < 0) continue;
            one.items[0] = m;
            if (int rc = add_messages(b, one, *dbs[i])) return fail(rc, dbs[i]->err);
            continue;
        }
        const json::Value* type = m.kind == json::Value::Object ? m.get(u"type") : nullptr;
        if (!c || c->kind != json::Value::Object || !type || type->kind != json::Value::String || type->str != u"op")
            continue;
        // the remote set (matrix.ts:575-601; an observer never submits, so never the ACK branch)
        int32_t op = -1, rc_[2] = {-1, -1};
        num_field(*c, u"type", &op);
        if (op != 2) return fail(MTE_E_UNSUPPORTED, "SharedMatrix op without target that is not a set");
        const json::Value* rc[2] = {c->get(u"row"), c->get(u"col")};
        for (int i = 0; i < 2; i++) {
            if (!rc[i] || rc[i]->kind != json::Value::Number || rc[i]->num < 0 || rc[i]->num > 0x7FFFFFFF ||
                rc[i]->num != (double)(int32_t)rc[i]->num)
                return fail(MTE_E_UNSUPPORTED, "set row / col must be an integer >= 0");
            rc_[i] = (int32_t)rc[i]->num;
        }
        const json::Value* v = c->get(u"value");
        const uint32_t val = v ? b->in->val(json::stringify(*v)) : 0u;  // undefined -> null in the blob
        const json::Value* cid = m.get(u"clientId");
        const std::string name = (cid && cid->kind == json::Value::String) ? json::to_utf8(cid->str.data(), cid->str.size()) : "";
        for (int i = 0; i < 2; i++) {
            DocBuild& db = *dbs[i];
            mte_op o{};
            num_field(m, u"sequenceNumber", &o.seq);
            num_field(m, u"referenceSequenceNumber", &o.ref_seq);
            num_field(m, u"minimumSequenceNumber", &o.msn);
            uint32_t sid = 0;
            if (db.collab) {  // getOrAddShortClientId (matrix.ts:576, 580)
                if (int e2 = db.short_id(name, &sid, o.seq)) return fail(e2, db.err);
                if (sid == 0) return fail(MTE_E_UNSUPPORTED, "observer never submits ops (ack path)");
                if (db.reused && o.ref_seq < db.cur_min) sid = 255;
            }
            o.client = (uint8_t)sid;
            o.type = MTE_OP_CELL;
            o.flags = i ? MTE_F_CELL_COL : 0;
            o.pos1 = rc_[i];
            o.b = cells;
            o.props = val;
            db.ops.push_back(o);
        }
        cells++;
    }
    return MTE_OK;
}

int mte_builder_add_matrix_log(mte_builder* b, const char* observer_name, const char* text, size_t len) {
    if (!b || !text) return MTE_E_ARG;
    if (!b->open.empty()) return builder_closed(b);
    json::Value log;
    try {
        log = json::parse(text, len);
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    if (log.kind != json::Value::Array) {
        b->err = "matrix log must be a JSON array of messages";
        return MTE_E_PARSE;
    }
    std::vector<std::unique_ptr<DocBuild>> dbs;
    for (int i = 0; i < 2; i++) {
        dbs.emplace_back(new DocBuild(observer_name));
        dbs.back()->perm = true;
    }
    uint32_t cells = b->n_cells;
    DocBuild* two[2] = {dbs[0].get(), dbs[1].get()};
    if (int rc = matrix_messages(b, log, two, cells)) return rc;
    for (int i = 0; i < 2; i++) {
        dbs[i]->commit(b->hb);
        b->paths.emplace_back(i ? "cols" : "rows");
    }
    b->n_cells = cells;
    return MTE_OK;
}

// de-interleave a 32-bit Morton key into its odd (row) and even (col) 16-bit halves
static void unmorton(uint32_t k, uint32_t* r, uint32_t* c) {
    uint32_t rr = 0, cc = 0;
    for (int i = 0; i < 16; i++) {
        cc |= ((k >> (2 * i)) & 1u) << i;
        rr |= ((k >> (2 * i + 1)) & 1u) << i;
    }
    *r = rr;
    *c = cc;
}

// SharedMatrix.loadCore (matrix.ts:528-546) + processCore of the suffix (include/mte.h).
int mte_builder_add_matrix_from_summary(mte_builder* b, const char* observer_name, const char* summary,
                                        size_t summary_len, const char* ops, size_t ops_len) {
    if (!b || !summary) return MTE_E_ARG;
    if (!b->open.empty()) return builder_closed(b);
    json::Value s, log;
    try {
        s = json::parse(summary, summary_len);
        if (ops) log = json::parse(ops, ops_len);
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    if (ops && log.kind != json::Value::Array) {
        b->err = "matrix log must be a JSON array of messages";
        return MTE_E_PARSE;
    }
    auto fail = [&](int code, const std::string& m) {
        b->err = m;
        return code;
    };
    std::vector<std::unique_ptr<DocBuild>> dbs;
    const char16_t* paths[2] = {u"rows", u"cols"};
    for (int i = 0; i < 2; i++) {
        dbs.emplace_back(new DocBuild(observer_name));
        DocBuild& db = *dbs.back();
        db.perm = true;
        // PermutationVector.load (permutationvector.ts:284-294): the handle table, then the segments
        const json::Value* e = tree_entry(s, paths[i]);
        const json::Value* vt = e ? e->get(u"value") : nullptr;
        if (!vt) return fail(MTE_E_PARSE, "matrix summary without its rows / cols tree");
        const json::Value* he = tree_entry(*vt, u"handleTable");
        const json::Value* se = tree_entry(*vt, u"segments");
        std::string ht;
        if (!he || !se || !se->get(u"value")) return fail(MTE_E_PARSE, "vector summary entries");
        if (int rc = blob_text(db, he->get(u"value"), ht, "handleTable blob missing")) return fail(rc, db.err);
        json::Value hv;
        try {
            hv = json::parse(ht.data(), ht.size());
        } catch (std::exception& ex) {
            return fail(MTE_E_PARSE, ex.what());
        }
        if (hv.kind != json::Value::Array || hv.items.empty()) return fail(MTE_E_PARSE, "handleTable is not an array");
        if (int rc = add_summary(b, *se->get(u"value"), db)) return fail(rc, db.err);
        for (size_t h = 0; h < hv.items.size(); h++) {
            const json::Value& x = hv.items[h];
            if (x.kind != json::Value::Number || x.num < 0 || x.num > 0x7FFFFFFF) return fail(MTE_E_UNSUPPORTED, "handle value");
            mte_op o{};
            o.type = MTE_OP_NOOP;
            o.flags = MTE_F_MX_HANDLE;
            o.pos1 = (int32_t)h;
            o.a = (int32_t)x.num;
            db.ops.push_back(o);
        }
    }
    // SparseArray2D.load (sparsearray2d.ts:232-235) of [cells, pending][0]: every tile and cell
    const json::Value* ce = tree_entry(s, u"cells");
    std::string ct;
    if (!ce) return fail(MTE_E_PARSE, "cells blob missing");
    if (int rc = blob_text(*dbs[0], ce->get(u"value"), ct, "cells blob missing")) return fail(rc, dbs[0]->err);
    json::Value cv;
    try {
        cv = json::parse(ct.data(), ct.size());
    } catch (std::exception& ex) {
        return fail(MTE_E_PARSE, ex.what());
    }
    if (cv.kind != json::Value::Array || cv.items.empty() || cv.items[0].kind != json::Value::Array)
        return fail(MTE_E_PARSE, "cells blob is not [cells, pending]");
    DocBuild& rows = *dbs[0];
    std::function<int(const json::Value&, uint32_t, uint32_t, uint32_t)> tile = [&](const json::Value& a, uint32_t hi,
                                                                                  uint32_t depth, uint32_t pre) -> int {
        if (a.kind != json::Value::Array || a.items.size() > 256) return fail(MTE_E_PARSE, "cells tile");
        mte_op t{};
        t.type = MTE_OP_NOOP;
        t.flags = MTE_F_MX_TILE;
        t.pos1 = (int32_t)hi;
        t.a = (int32_t)pre;
        t.b = depth;
        rows.ops.push_back(t);
        for (uint32_t i = 0; i < a.items.size(); i++) {
            const json::Value& x = a.items[i];
            if (x.kind == json::Value::Null) continue;
            if (depth < 3) {
                if (int rc = tile(x, hi, depth + 1, pre | (i << (16 - 8 * depth)))) return rc;
                continue;
            }
            const uint32_t lo = (pre << 8) | i;  // the low key's bytes 0..3
            uint32_t rh, ch, rl, cl;
            unmorton(hi, &rh, &ch);
            unmorton(lo, &rl, &cl);
            mte_op o{};
            o.type = MTE_OP_NOOP;
            o.flags = MTE_F_MX_CELL;
            o.pos1 = (int32_t)((rh << 16) | rl);
            o.a = (int32_t)((ch << 16) | cl);
            o.props = b->in->val(json::stringify(x));
            rows.ops.push_back(o);
        }
        return MTE_OK;
    };
    const json::Value& root = cv.items[0];
    for (uint32_t k = 0; k < root.items.size(); k++)
        if (root.items[k].kind != json::Value::Null)
            if (int rc = tile(root.items[k], k, 0, 0)) return rc;
    if (root.items.size() > 1) {  // the root's length (trailing undefined entries included)
        mte_op t{};
        t.type = MTE_OP_NOOP;
        t.flags = MTE_F_MX_TILE;
        t.pos1 = (int32_t)root.items.size() - 1;
        t.b = 4;  // (no tile: only the root's extent)
        rows.ops.push_back(t);
    }
    uint32_t cells = b->n_cells;
    if (ops) {
        DocBuild* two[2] = {dbs[0].get(), dbs[1].get()};
        if (int rc = matrix_messages(b, log, two, cells)) return rc;
    }
    for (int i = 0; i < 2; i++) {
        dbs[i]->commit(b->hb);
        b->paths.emplace_back(i ? "cols" : "rows");
    }
    b->n_cells = cells;
    return MTE_OK;
}

// An open document (Client.applyMsg one message batch at a time, client.ts:805-836): its log grows
// by mte_builder_append_messages; every mte_builder_batch sees it as it is then (commit of a copy: the
// messages above minSeq at the end of the log so far are its catch-up messages).
int mte_builder_open_doc(mte_builder* b, const char* observer_name, uint32_t* doc) {
    if (!b || !doc) return MTE_E_ARG;
    *doc = b->hb.n_docs() + (uint32_t)b->open.size();
    b->open.emplace_back(new DocBuild(observer_name));
    b->paths.emplace_back();
    return MTE_OK;
}
// ... whose log starts with a summary's records (Client.load before the first applyMsg)
int mte_builder_open_doc_from_summary(mte_builder* b, const char* observer_name, const char* summary,
                                      size_t summary_len, uint32_t* doc) {
    if (!b || !summary || !doc) return MTE_E_ARG;
    std::unique_ptr<DocBuild> db(new DocBuild(observer_name));
    json::Value s;
    try {
        s = json::parse(summary, summary_len);
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    if (int rc = add_summary(b, s, *db)) {
        b->err = db->err;
        return rc;
    }
    *doc = b->hb.n_docs() + (uint32_t)b->open.size();
    b->open.push_back(std::move(db));
    b->paths.emplace_back();
    return MTE_OK;
}
int mte_builder_append_messages(mte_builder* b, uint32_t doc, const char* text, size_t len) {
    if (!b || !text) return MTE_E_ARG;
    const uint32_t nc = b->hb.n_docs();
    if (doc < nc || doc - nc >= b->open.size()) {
        b->err = "not an open document";
        return MTE_E_ARG;
    }
    json::Value msgs;
    try {
        msgs = json::parse(text, len);
    } catch (std::exception& ex) {
        b->err = ex.what();
        return MTE_E_PARSE;
    }
    DocBuild& db = *b->open[doc - nc];
    // all or nothing: a message the builder refuses leaves the document as it was
    DocBuild keep = db;
    if (int rc = add_messages(b, msgs, db)) {
        b->err = db.err;
        db = std::move(keep);
        return rc;
    }
    return MTE_OK;
}
mte_builder::~mte_builder() = default;

int mte_builder_batch(mte_builder* b, mte_batch* out) {
    if (!b || !out) return MTE_E_ARG;
    if (b->open.empty()) {
        b->hb.view(out);
        return MTE_OK;
    }
    b->view = b->hb;
    for (auto& d : b->open) {
        DocBuild c = *d;
        c.commit(b->view);
    }
    b->view.view(out);
    return MTE_OK;
}

}  // extern "C"
