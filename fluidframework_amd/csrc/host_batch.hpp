// host_batch.hpp — the host-side batch in struct-of-arrays form (include/mte.h mte_batch), the
// interning tables for its property keys, values and sets, and the small JSON helpers the builder and
// the engine's read-back share. Host-only C++: no HIP include, so the builder compiles without the
// HIP runtime.
//
// Everything declared here is internal to libmte.so (hidden visibility).
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mte.h"
#include "jsonlite.hpp"

using namespace mte;  // json:: (jsonlite.hpp); the engine files and the builder use engine_types.hpp's names too

#pragma GCC visibility push(hidden)

struct HostBatch {
    std::vector<uint64_t> doc_op_offsets{0};
    std::vector<mte_op> ops;
    std::vector<uint64_t> doc_payload_offsets{0};
    std::vector<uint16_t> payload;
    std::vector<mte_propset> propsets{mte_propset{0, 0}};
    std::vector<uint32_t> prop_keys, prop_vals;
    std::vector<uint64_t> key_offsets{0};
    std::string key_text;
    std::vector<uint64_t> val_offsets{0};
    std::string val_text;
    std::vector<uint32_t> doc_client_offsets{0};
    std::vector<uint64_t> client_name_offsets{0};
    std::string client_names;
    // legacy catch-up messages (include/mte.h mte_batch.msg_*)
    std::vector<uint64_t> doc_msg_offsets{0};
    std::vector<uint64_t> msg_first_op;
    std::vector<uint64_t> msg_text_offsets{0};
    std::string msg_text;

    uint32_t n_docs() const { return (uint32_t)doc_op_offsets.size() - 1; }
    void view(mte_batch* b) const {
        b->n_docs = n_docs();
        b->doc_op_offsets = doc_op_offsets.data();
        b->ops = ops.data();
        b->doc_payload_offsets = doc_payload_offsets.data();
        b->payload = payload.data();
        b->n_propsets = (uint32_t)propsets.size();
        b->propsets = propsets.data();
        b->prop_keys = prop_keys.data();
        b->prop_vals = prop_vals.data();
        b->n_keys = (uint32_t)key_offsets.size() - 1;
        b->key_offsets = key_offsets.data();
        b->key_text = key_text.data();
        b->n_vals = (uint32_t)val_offsets.size() - 1;
        b->val_offsets = val_offsets.data();
        b->val_text = val_text.data();
        b->doc_client_offsets = doc_client_offsets.data();
        b->client_name_offsets = client_name_offsets.data();
        b->client_names = client_names.data();
        const bool msgs = doc_msg_offsets.size() == (size_t)n_docs() + 1;  // generated batches keep none
        b->doc_msg_offsets = msgs ? doc_msg_offsets.data() : nullptr;
        b->msg_first_op = msgs ? msg_first_op.data() : nullptr;
        b->msg_text_offsets = msgs ? msg_text_offsets.data() : nullptr;
        b->msg_text = msgs ? msg_text.data() : nullptr;
    }
    std::string message(uint64_t i) const {
        return msg_text.substr(msg_text_offsets[i], msg_text_offsets[i + 1] - msg_text_offsets[i]);
    }
    std::string key(uint32_t k) const { return key_text.substr(key_offsets[k], key_offsets[k + 1] - key_offsets[k]); }
    std::string val(uint32_t v) const { return val_text.substr(val_offsets[v], val_offsets[v + 1] - val_offsets[v]); }
    std::string client(uint32_t doc, uint32_t shortId) const {
        uint32_t i = doc_client_offsets[doc] + shortId;
        if (i >= doc_client_offsets[doc + 1]) return std::string();
        return client_names.substr(client_name_offsets[i], client_name_offsets[i + 1] - client_name_offsets[i]);
    }
};

// Interning tables shared by the builder and the generator.
struct Interner {
    HostBatch* hb;
    std::unordered_map<std::string, uint32_t> keys, vals;
    std::map<std::vector<uint32_t>, uint32_t> sets;
    explicit Interner(HostBatch* h) : hb(h) {
        if (hb->val_offsets.size() == 1) {  // value id 0 == JSON null (a delete in annotate)
            hb->val_text = "null";
            hb->val_offsets.push_back(4);
        }
        vals["null"] = 0;
    }
    uint32_t key(const std::u16string& k) {
        std::string q;
        json::quote(q, k);
        auto it = keys.find(q);
        if (it != keys.end()) return it->second;
        uint32_t id = (uint32_t)hb->key_offsets.size() - 1;
        hb->key_text += q;
        hb->key_offsets.push_back(hb->key_text.size());
        keys[q] = id;
        return id;
    }
    uint32_t val(const std::string& canonical) {
        auto it = vals.find(canonical);
        if (it != vals.end()) return it->second;
        uint32_t id = (uint32_t)hb->val_offsets.size() - 1;
        hb->val_text += canonical;
        hb->val_offsets.push_back(hb->val_text.size());
        vals[canonical] = id;
        return id;
    }
    // A props object in Object.keys order (properties are applied key by key in that order,
    // segmentPropertiesManager.ts:81-106).
    uint32_t propset(const json::Value& obj) {
        std::vector<uint32_t> kv;
        for (size_t i : json::key_order(obj)) {
            kv.push_back(key(obj.members[i].first));
            kv.push_back(val(json::stringify(obj.members[i].second)));
        }
        return intern_kv(kv);
    }
    uint32_t intern_kv(const std::vector<uint32_t>& kv) {
        auto it = sets.find(kv);
        if (it != sets.end()) return it->second;
        uint32_t id = (uint32_t)hb->propsets.size();
        mte_propset ps{(uint32_t)hb->prop_keys.size(), (uint32_t)(kv.size() / 2)};
        for (size_t i = 0; i < kv.size(); i += 2) {
            hb->prop_keys.push_back(kv[i]);
            hb->prop_vals.push_back(kv[i + 1]);
        }
        hb->propsets.push_back(ps);
        sets[kv] = id;
        return id;
    }
};

// ---- small JSON helpers (jsonlite.hpp values)
inline int num_field(const json::Value& o, const char16_t* k, int32_t* out) {
    const json::Value* v = o.get(k);
    if (!v || v->kind != json::Value::Number) return 0;
    *out = (int32_t)v->num;
    return 1;
}

// Marker.getId (mergeTree.ts:690-695) of a segment's props: the "markerId" value when it is a
// non-empty string (a truthy non-string id is left unmapped: relative positions naming it fail).
inline bool marker_id(const json::Value* props, std::u16string* id) {
    const json::Value* v = props && props->kind == json::Value::Object ? props->get(u"markerId") : nullptr;
    if (!v || v->kind != json::Value::String || v->str.empty()) return false;
    *id = v->str;
    return true;
}

inline void set_member(json::Value& o, const char16_t* k, json::Value v) {
    for (auto& m : o.members)
        if (m.first == k) {
            m.second = std::move(v);
            return;
        }
    o.members.emplace_back(k, std::move(v));
}
inline json::Value jobj() {
    json::Value v;
    v.kind = json::Value::Object;
    return v;
}
inline json::Value jstr(const std::u16string& v) {
    json::Value x;
    x.kind = json::Value::String;
    x.str = v;
    return x;
}
// (the read-back's jnumv and the builder's jnum were the same function but for the names of the
// parameter and the local: one copy)
inline json::Value jnum(double v) {
    json::Value x;
    x.kind = json::Value::Number;
    x.num = v;
    return x;
}

#pragma GCC visibility pop
