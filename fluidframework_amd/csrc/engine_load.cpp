// engine_load.cpp — the engine's life cycle and everything that puts a batch on the device:
// mte_create / mte_destroy, mte_load and mte_generate (stage batches in HBM, size per-document arenas,
// upload the property tables), and mte_export_batch. Part of the C ABI of include/mte.h; the replay
// itself is engine_run.cpp, the outputs readback.cpp.
// There is no CPU execution path for replay: without a HIP device mte_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mte.h"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "host_batch.hpp"
#include "jsonlite.hpp"
#include "mte_kernels.h"

// The engine's copy of a caller's batch.
// with_ops = false: everything but the op records and the payload (mte_load uploads those straight
// from the caller's buffers; ensure_host_ops reads them back if a host walker ever needs them)
static void copy_batch(HostBatch& h, const mte_batch* b, bool with_ops = true) {
    const uint32_t n = b->n_docs;
    h.doc_op_offsets.assign(b->doc_op_offsets, b->doc_op_offsets + n + 1);
    h.doc_payload_offsets.assign(b->doc_payload_offsets, b->doc_payload_offsets + n + 1);
    if (with_ops) {
        h.ops.assign(b->ops, b->ops + h.doc_op_offsets[n]);
        h.payload.assign(b->payload, b->payload + h.doc_payload_offsets[n]);
    } else {
        std::vector<mte_op>().swap(h.ops);
        std::vector<uint16_t>().swap(h.payload);
    }
    h.propsets.assign(b->propsets, b->propsets + b->n_propsets);
    size_t nkv = 0;
    for (auto& ps : h.propsets) nkv = std::max<size_t>(nkv, (size_t)ps.first + ps.count);
    h.prop_keys.assign(b->prop_keys, b->prop_keys + nkv);
    h.prop_vals.assign(b->prop_vals, b->prop_vals + nkv);
    h.key_offsets.assign(b->key_offsets, b->key_offsets + b->n_keys + 1);
    h.key_text.assign(b->key_text, b->key_offsets[b->n_keys]);
    h.val_offsets.assign(b->val_offsets, b->val_offsets + b->n_vals + 1);
    h.val_text.assign(b->val_text, b->val_offsets[b->n_vals]);
    h.doc_client_offsets.assign(b->doc_client_offsets, b->doc_client_offsets + n + 1);
    uint32_t nn = h.doc_client_offsets[n];
    h.client_name_offsets.assign(b->client_name_offsets, b->client_name_offsets + nn + 1);
    h.client_names.assign(b->client_names, b->client_name_offsets[nn]);
    if (b->doc_msg_offsets && b->msg_first_op && b->msg_text_offsets && b->msg_text) {
        h.doc_msg_offsets.assign(b->doc_msg_offsets, b->doc_msg_offsets + n + 1);
        const uint64_t nm = h.doc_msg_offsets[n];
        h.msg_first_op.assign(b->msg_first_op, b->msg_first_op + nm);
        h.msg_text_offsets.assign(b->msg_text_offsets, b->msg_text_offsets + nm + 1);
        h.msg_text.assign(b->msg_text, b->msg_text_offsets[nm]);
    } else {
        h.doc_msg_offsets.assign(n + 1, 0);
        h.msg_first_op.clear();
        h.msg_text_offsets.assign(1, 0);
        h.msg_text.clear();
    }
}

// ------------------------------------------------------------------------------------------------
// Value / key metadata for the device: JS falsiness (rewrite), object-typed values and the
// matchProperties relation against object-typed values (properties.ts:62-93).
static int derive_value_tables(mte_engine* e) {
    const HostBatch& hb = e->hb;
    uint32_t nv = (uint32_t)hb.val_offsets.size() - 1;
    std::vector<json::Value> vals(nv);
    for (uint32_t v = 0; v < nv; v++) {
        std::string t = hb.val(v);
        try {
            vals[v] = json::parse(t.data(), t.size());
        } catch (std::exception& ex) {
            return set_err(e, MTE_E_PARSE, ex.what());
        }
    }
    e->val_flags.assign(nv, 0);
    e->val_objidx.assign(nv, NONE);
    e->val_objmatch.assign(nv, 0);
    // val_match(a, b) is a == b, or bit val_objidx[b] of val_objmatch[a]: a column only for an object
    // value that some OTHER value id equals (the same object in another key order, an array and its
    // index object, ...). Every other object value matches its own id alone, and a == b covers that.
    // A stored value is never null (id 0, a delete), so b is truthy, and matchProperties(a, b) then
    // needs a truthy with the same for-in keys: only values with equal key sets are compared.
    typedef std::vector<std::u16string> KeySet;
    auto key_set = [&](uint32_t v) {
        KeySet k = json::for_in(&vals[v]);
        std::sort(k.begin(), k.end());
        return k;
    };
    std::map<KeySet, std::vector<uint32_t>> groups;  // key set of some object value -> values with it
    std::vector<uint8_t> sizes;                      // sizes[n]: some object value has n keys
    for (uint32_t v = 0; v < nv; v++) {
        if (!json::truthy(&vals[v])) e->val_flags[v] |= 1u;
        if (json::is_object_typed(&vals[v]) && v != 0) {
            e->val_flags[v] |= 2u;
            KeySet k = key_set(v);
            if (sizes.size() <= k.size()) sizes.resize(k.size() + 1, 0);
            sizes[k.size()] = 1;
            groups[std::move(k)];
        }
    }
    for (uint32_t v = 1; v < nv && !groups.empty(); v++) {
        if (e->val_flags[v] & 1u) continue;
        // (a string's for-in keys are its indices: skip one no object value's key count equals)
        const size_t n = vals[v].kind == json::Value::String ? vals[v].str.size() : 0;
        if (vals[v].kind == json::Value::String && (n >= sizes.size() || !sizes[n])) continue;
        auto it = groups.find(key_set(v));
        if (it != groups.end()) it->second.push_back(v);
    }
    uint32_t n_cols = 0;
    for (auto& g : groups)
        for (uint32_t b : g.second) {
            if (!(e->val_flags[b] & 2u)) continue;
            for (uint32_t a : g.second) {
                if (a == b || !json::match_properties(&vals[a], &vals[b])) continue;
                if (e->val_objidx[b] == NONE) {
                    if (n_cols == 64)
                        return set_err(e, MTE_E_UNSUPPORTED,
                                       "more than 64 object values of the batch's properties equal another value "
                                       "(matchProperties): the match table has 64 columns");
                    e->val_objidx[b] = n_cols++;
                    e->val_objmatch[b] |= 1ull << e->val_objidx[b];
                }
                e->val_objmatch[a] |= 1ull << e->val_objidx[b];
            }
        }
    uint32_t nk = (uint32_t)hb.key_offsets.size() - 1;
    e->key_is_index.assign(nk, 0);
    e->key_index.assign(nk, 0);
    for (uint32_t k = 0; k < nk; k++) {
        std::string t = hb.key(k);
        json::Value kv = json::parse(t.data(), t.size());
        uint32_t idx;
        if (json::array_index(kv.str, &idx)) {
            e->key_is_index[k] = 1;
            e->key_index[k] = idx;
        }
    }
    return MTE_OK;
}

// Host -> device copy of a large caller buffer through two pinned chunks: host threads copy chunk i+1
// out of the (pageable) source while the DMA engine moves chunk i. A pageable hipMemcpyAsync stages
// through the runtime's own buffers and ran at 3.6 GB/s on the first C4-sized load
// (profiles/pcie_r02l_c4.json); this path does not depend on what the runtime has pinned before.
static constexpr size_t STAGE_BYTES = 64ull << 20;
int upload_staged(mte_engine* e, void* dst, const void* src, size_t bytes) {
    if (bytes < (4ull << 20)) {  // small: the runtime's path is fine
        HIP_TRY(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
        return MTE_OK;
    }
    for (int i = 0; i < 2; i++) {
        if (!e->stage[i]) HIP_TRY(e, hipHostMalloc(&e->stage[i], STAGE_BYTES, hipHostMallocDefault));
        if (!e->ev_stage[i]) HIP_TRY(e, hipEventCreateWithFlags(&e->ev_stage[i], hipEventDisableTiming));
    }
    const unsigned nt = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    int k = 0;
    for (size_t off = 0; off < bytes; off += STAGE_BYTES, k ^= 1) {
        const size_t n = std::min(STAGE_BYTES, bytes - off);
        auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(e, hipEventSynchronize(e->ev_stage[k]));  // the DMA out of this chunk is done
        auto t1 = std::chrono::steady_clock::now();
        char* stg = (char*)e->stage[k];
        const char* from = (const char*)src + off;
        const size_t piece = (n + nt - 1) / nt;
        std::atomic<unsigned> next{0};
        run_pool(nt, [&]() {
            for (unsigned t; (t = next.fetch_add(1)) < nt;) {
                const size_t a = (size_t)t * piece;
                if (a < n) memcpy(stg + a, from + a, std::min(piece, n - a));
            }
        });
        auto t2 = std::chrono::steady_clock::now();
        e->stage_wait_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
        e->stage_copy_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
        HIP_TRY(e, hipMemcpyAsync((char*)dst + off, stg, n, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(e, hipEventRecord(e->ev_stage[k], e->stream));
    }
    return MTE_OK;
}

// Output text pool: a document's final text never exceeds the text its log inserted, so the
// payload's size bounds the whole batch (Engine::finish gathers into it).
static int alloc_out_text(mte_engine* e) {
    const uint64_t pay = e->hb.doc_payload_offsets.empty() ? 0 : e->hb.doc_payload_offsets.back();
    const uint64_t n = std::max<uint64_t>(1, std::min<uint64_t>(pay, 0xFFFFFFFFull));
    if (n > e->d_out_text.n || !e->d_out_text.p) HIP_TRY(e, e->d_out_text.alloc(n));
    e->P.out_text = e->d_out_text.p;
    e->P.out_text_cap = n;
    return MTE_OK;
}

int alloc_slots(mte_engine* e) {
    uint32_t g, h;
    const uint32_t ns = solo_count(e);
    wave_plan(e, e->P.n_docs, g, h, nullptr, ns);
    const uint32_t n = g * LDS_WAVES + h;
    const size_t bytes = (size_t)n * e->P.slot_bytes;
    if (bytes > e->d_spill.n || !e->d_spill.p) HIP_TRY(e, e->d_spill.alloc(bytes));
    const size_t words = (n + 31) / 32 + 1;  // (k_rows may claim any of the n slots: rows_continue)
    if (words > e->d_slot_bits.n || !e->d_slot_bits.p) HIP_TRY(e, e->d_slot_bits.alloc(words));
    HIP_TRY(e, e->d_rows_cont.fit((size_t)std::max<uint32_t>(n, 1) * ROWS_CONT_WORDS));
    // (k_rows dumps a document's state into its slot before k_rows_cont converts it in place)
    e->P.rows_cont = e->P.slot_bytes >= ROWS_DUMP_BYTES ? e->d_rows_cont.p : nullptr;
    e->n_slots = n;
    e->P.spill = e->d_spill.p;
    e->P.slot_bits = e->d_slot_bits.p;
    // solo documents continue in slots of their own, sized for the longest of them
    e->P.n_solo = ns;
    if (ns) {
        uint64_t nmax = 0;
        for (uint32_t k = 0; k < ns; k++) nmax = std::max(nmax, e->n_ops_doc[e->order[k]]);
        hbm_caps(nmax, e->P.solo_blk, e->P.solo_ord, e->P.solo_in, e->P.solo_heap);
        e->P.solo_slot_bytes =
            (HbmLayout::of(e->P.solo_blk, e->P.solo_ord, e->P.solo_in, e->P.solo_heap).bytes + 255) & ~255ull;
        const size_t sb = (size_t)ns * e->P.solo_slot_bytes;
        if (sb > e->d_solo_spill.n || !e->d_solo_spill.p) HIP_TRY(e, e->d_solo_spill.alloc(sb));
        e->P.solo_spill = e->d_solo_spill.p;
    }
    return MTE_OK;
}

// Per-document arena sizing (see DESIGN.md "HBM layout").
static int layout_and_alloc(mte_engine* e, const std::vector<uint64_t>& n_ops, const std::vector<uint64_t>& pay_len,
                            const std::vector<uint64_t>& n_prop_ins, const std::vector<uint64_t>& n_ann,
                            const std::vector<uint8_t>& collab, const std::vector<uint8_t>& has_nl,
                            uint64_t arena_limit = 0, const uint64_t* op_offsets = nullptr,
                            const uint64_t* payload_offsets = nullptr, const uint32_t* doc_ids = nullptr) {
    const uint32_t nd = (uint32_t)n_ops.size();
    e->cfg.assign(nd, DocCfg{});
    e->n_ops_doc = n_ops;
    uint64_t op = 0, pay = 0, ar = 0, seg = 0, seg2 = 0, mp = 0, out = 0;
    bool any_props = false;
    for (uint32_t d = 0; d < nd; d++) {
        DocCfg& c = e->cfg[d];
        uint64_t n = n_ops[d];
        // a loaded batch's documents need not start at op / payload 0 (mte_batch offsets are absolute)
        c.op_begin = op_offsets ? op_offsets[d] : op;
        c.op_end = c.op_begin + n;
        op += n;
        c.payload_off = payload_offsets ? payload_offsets[d] : pay;
        c.payload_len = (uint32_t)pay_len[d];
        pay += pay_len[d];
        // merge arena semispace: live arena text <= 2x live text, a scour needs <= 4x a block's text
        uint64_t acap = 6 * pay_len[d] + 4096;
        if (arena_limit) acap = std::min<uint64_t>(acap, arena_limit);
        c.arena_cap = (uint32_t)std::min<uint64_t>(acap, 0x7FFFFFF0ull / 2);
        c.arena_off = ar;
        ar += 2ull * c.arena_cap;
        c.seg_cap = (uint32_t)std::min<uint64_t>(3 * n + 8, 0xFFFFFFF0ull);
        c.ovl_off = seg;
        seg += c.seg_cap;
        // a window of more than 64 clients (a loaded batch's names; the generator's stay below 64):
        // removedClientOverlap of clients 64..127 in a second per-segment word
        const auto& dco = e->hb.doc_client_offsets;
        c.ovl2_off = OVL2_NONE;
        if (dco.size() > d + 1 && dco[d + 1] - dco[d] > 64) {
            c.ovl2_off = seg2;
            seg2 += c.seg_cap;
        }
        c.map_cap = (uint32_t)(n_prop_ins[d] + 4 * n_ann[d] + 16);
        c.map_off = mp;
        mp += c.map_cap;
        any_props |= n_prop_ins[d] + n_ann[d] > 0;
        c.collab = collab[d];
        c.has_nl = has_nl[d];
        c.prio = 0;
        c.gid = doc_ids ? doc_ids[d] : (uint32_t)(e->doc_id_base + d);
        out += std::min<uint64_t>(3 * n + 8, 4096);
    }
    out += 1u << 20;
    // critical-path documents (Zipf heads): at least 8x the mean op count
    if (nd > 1) {
        const double mean = (double)op / nd;
        for (uint32_t d = 0; d < nd; d++)
            if ((double)n_ops[d] >= 8.0 * mean) e->cfg[d].prio = 1;
    }
    HIP_TRY(e, e->d_arena.fit(ar));
    HIP_TRY(e, e->d_ovl.fit(seg));
    if (seg2) HIP_TRY(e, e->d_ovl2.fit(seg2));
    HIP_TRY(e, e->d_maps.fit(mp * e->map_words));
    HIP_TRY(e, e->d_out_vis.fit(out));
    HIP_TRY(e, e->d_out_esc.fit(out));
    HIP_TRY(e, e->d_out_aux.fit(out));
    HIP_TRY(e, e->d_out_ovl.fit(out));
    if (seg2) HIP_TRY(e, e->d_out_ovl2.fit(out));
    if (any_props) HIP_TRY(e, e->d_out_maps.fit(out * e->map_words));  // some document can carry props
    HIP_TRY(e, e->d_counters.fit(16));
    HIP_TRY(e, e->d_rows_retry.fit(nd));
    HIP_TRY(e, e->d_res.fit(nd));
    HIP_TRY(e, e->d_prof.fit((size_t)nd * PROF_SLOTS));
    HIP_TRY(e, hipMemsetAsync(e->d_prof.p, 0, (size_t)nd * PROF_SLOTS * 8, e->stream));
    HIP_TRY(e, e->d_solo_clk.fit(4 * SOLO_CLK_SLOTS + 1));  // 4 u64 per solo workgroup + the bulk's start
    HIP_TRY(e, e->d_solo_started.fit(1));
    // LPT order: longest documents start first
    e->order.resize(nd);
    for (uint32_t d = 0; d < nd; d++) e->order[d] = d;
    std::stable_sort(e->order.begin(), e->order.end(), [&](uint32_t a, uint32_t b) { return n_ops[a] > n_ops[b]; });
    int rc;
    if ((rc = upload(e, e->d_cfg, e->cfg))) return rc;
    if ((rc = upload(e, e->d_order, e->order))) return rc;
    Params& P = e->P;
    P = Params{};
    P.n_docs = nd;
    P.docs = e->d_cfg.p;
    P.doc_list = e->d_order.p;
    P.n_list = nd;
    P.res = e->d_res.p;
    P.arena = e->d_arena.p;
    P.ovl = e->d_ovl.p;
    P.ovl2 = seg2 ? e->d_ovl2.p : nullptr;
    P.out_ovl2 = seg2 ? e->d_out_ovl2.p : nullptr;
    P.maps = e->d_maps.p;
    P.map_words = e->map_words;
    P.out_vis = e->d_out_vis.p;
    P.out_aux = e->d_out_aux.p;
    P.out_ovl = e->d_out_ovl.p;
    P.out_cap = out;
    P.out_maps = any_props ? e->d_out_maps.p : nullptr;
    P.counters = e->d_counters.p;
    P.prof = e->d_prof.p;
    P.solo_clk = e->d_solo_clk.p;
    P.solo_started = e->d_solo_started.p;
    P.rows_retry = e->d_rows_retry.p;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus <= 0) cus = 256;
    e->n_groups = (uint32_t)cus;
    // per-wave HBM slots, each sized for the longest document up to slot_ops_cap ops (hbm_caps);
    // a longer document that outgrows its slot is re-run by the host with worst-case capacities
    uint64_t nmax = 0;
    for (uint32_t d = 0; d < nd; d++) nmax = std::max<uint64_t>(nmax, n_ops[d]);
    hbm_caps(std::min<uint64_t>(nmax, e->slot_ops_cap), P.slot_blk, P.slot_ord, P.slot_in, P.slot_heap);
    if (e->slot_blk_limit) {  // test knob: slots that overflow (documents re-run by the host)
        P.slot_blk = std::min(P.slot_blk, e->slot_blk_limit);
        P.slot_ord = std::min(P.slot_ord, e->slot_blk_limit);
    }
    P.slot_bytes = (HbmLayout::of(P.slot_blk, P.slot_ord, P.slot_in, P.slot_heap).bytes + 255) & ~255ull;
    return alloc_slots(e);
}

static int upload_props(mte_engine* e) {
    int rc;
    if ((rc = derive_value_tables(e))) return rc;
    if ((rc = upload(e, e->d_propsets, e->hb.propsets))) return rc;
    if ((rc = upload(e, e->d_prop_keys, e->hb.prop_keys))) return rc;
    if ((rc = upload(e, e->d_prop_vals, e->hb.prop_vals))) return rc;
    if ((rc = upload(e, e->d_val_flags, e->val_flags))) return rc;
    if ((rc = upload(e, e->d_val_objidx, e->val_objidx))) return rc;
    if ((rc = upload(e, e->d_val_objmatch, e->val_objmatch))) return rc;
    e->P.propsets = e->d_propsets.p;
    e->P.prop_keys = e->d_prop_keys.p;
    e->P.prop_vals = e->d_prop_vals.p;
    e->P.val_flags = e->d_val_flags.p;
    e->P.val_objidx = e->d_val_objidx.p;
    e->P.val_objmatch = e->d_val_objmatch.p;
    e->P.n_propsets = (uint32_t)e->hb.propsets.size();
    e->P.n_vals = (uint32_t)e->val_flags.size();
    return MTE_OK;
}

// ------------------------------------------------------------------------------------------------
int mte_abi_version(void) { return MTE_ABI_VERSION; }

const char* mte_build_info(void) {
    static std::string s = std::string("mte gfx950 hip ") + std::to_string(HIP_VERSION_MAJOR) + "." +
                           std::to_string(HIP_VERSION_MINOR);
    return s.c_str();
}

int mte_create(const mte_config* cfg, mte_engine** out) {
    if (!out) return MTE_E_ARG;
    *out = nullptr;
    std::unique_ptr<mte_engine> e(new mte_engine());
    if (cfg) {
        e->device = cfg->device;
        if (cfg->chunk_size) e->chunk = cfg->chunk_size;
        e->legacy = cfg->snapshot_format == 1;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= e->device) {
        // No CPU fallback: the replay path runs on the GPU only.
        static thread_local std::string why;
        why = "mte: no HIP device available (MI355X/gfx950 required)";
        return MTE_E_HIP;
    }
    HIP_TRY(e.get(), hipSetDevice(e->device));
    HIP_TRY(e.get(), hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    HIP_TRY(e.get(), hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
    HIP_TRY(e.get(), hipStreamCreateWithFlags(&e->stream3, hipStreamNonBlocking));
    HIP_TRY(e.get(), hipEventCreateWithFlags(&e->ev3, hipEventDisableTiming));
    HIP_TRY(e.get(), hipEventCreate(&e->ev_s0));
    HIP_TRY(e.get(), hipEventCreate(&e->ev_s1));
    HIP_TRY(e.get(), hipEventCreateWithFlags(&e->ev2, hipEventDisableTiming));
    HIP_TRY(e.get(), hipEventCreateWithFlags(&e->ev_gate, hipEventDisableTiming));
    HIP_TRY(e.get(), hipEventCreateWithFlags(&e->ev_blk, hipEventDisableTiming));
    HIP_TRY(e.get(), hipEventCreate(&e->ev0));
    HIP_TRY(e.get(), hipEventCreate(&e->ev1));
    *out = e.release();
    return MTE_OK;
}

void mte_destroy(mte_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    mx_drop_tables(e);
    for (int i = 0; i < 2; i++) {
        if (e->stage[i]) (void)hipHostFree(e->stage[i]);
        if (e->ev_stage[i]) (void)hipEventDestroy(e->ev_stage[i]);
    }
    if (e->ev_gate) (void)hipEventDestroy(e->ev_gate);
    if (e->ev_blk) (void)hipEventDestroy(e->ev_blk);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->ev2) (void)hipEventDestroy(e->ev2);
    if (e->ev3) (void)hipEventDestroy(e->ev3);
    if (e->ev_s0) (void)hipEventDestroy(e->ev_s0);
    if (e->ev_s1) (void)hipEventDestroy(e->ev_s1);
    if (e->stream3) (void)hipStreamDestroy(e->stream3);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

const char* mte_last_error(const mte_engine* e) { return e ? e->err.c_str() : "null engine"; }

static void count_doc_ops(const mte_op* ops, const uint64_t* off, uint32_t d, uint64_t& pi, uint64_t& an,
                          bool* rel = nullptr) {
    pi = an = 0;
    for (uint64_t i = off[d]; i < off[d + 1]; i++) {
        const mte_op& o = ops[i];
        if (rel && o.type == MTE_OP_RELPOS) *rel = true;  // FULL kernels only
        if ((o.type == MTE_OP_INSERT || o.type == MTE_OP_INSERT_MARKER || o.type == MTE_OP_LOAD_SEG ||
             o.type == MTE_OP_LOAD_APPEND) && o.props)
            pi++;
        if (o.type == MTE_OP_ANNOTATE) an++;
    }
}

// SharedMatrix cell records (include/mte.h MTE_OP_CELL): each vector document with some gets a
// HandleTable region (1 + 2 * (records + 2) words) and the batch two words per cell index for each
// pass's results; the records' cell / seq / value are kept for the cells blob (mte_snapshot_matrix).
static int load_cells(mte_engine* e, const mte_batch* b, const std::vector<uint32_t>& n_cell) {
    e->cell_recs.clear();
    e->mx_init.clear();
    e->n_cells = 0;
    uint64_t words = 0;
    std::vector<uint32_t> init;  // every region's state at document start (Params::htab0)
    bool any = false;
    for (uint32_t d = 0; d < b->n_docs; d++) {
        DocCfg& c = e->cfg[d];
        c.ht_cap = 0;
        c.ht_off = 0;
        // a loaded HandleTable (MX_HANDLE records) and cells (MX_CELL / MX_TILE)
        std::vector<uint32_t> h0;
        for (uint64_t i = b->doc_op_offsets[d]; i < b->doc_op_offsets[d + 1]; i++) {
            const mte_op& o = b->ops[i];
            if (o.type != MTE_OP_NOOP || !(o.flags & MTE_F_MX_MASK)) continue;
            const uint32_t f = o.flags & MTE_F_MX_MASK;
            if (f == MTE_F_MX_HANDLE) {
                if (o.pos1 < 0 || o.pos1 > (1 << 26)) return set_err(e, MTE_E_RANGE, "loaded handle table too long");
                if (h0.size() <= (size_t)o.pos1) h0.resize((size_t)o.pos1 + 1, 0);
                h0[(size_t)o.pos1] = (uint32_t)o.a;
            } else if (f == MTE_F_MX_CELL) {
                e->mx_init[d].cells.push_back({(uint32_t)o.pos1, (uint32_t)o.a, o.props < b->n_vals ? o.props : 0u});
            } else if (o.b == 4) {
                e->mx_init[d].root_len = (uint32_t)o.pos1 + 1;
            } else {
                e->mx_init[d].tiles.push_back({(uint32_t)o.pos1, o.b, (uint32_t)o.a});
            }
        }
        if (!n_cell[d] && h0.empty()) continue;
        if (n_cell[d]) {
            std::vector<mte_engine::CellRec>& v = e->cell_recs[d];
            for (uint64_t i = b->doc_op_offsets[d]; i < b->doc_op_offsets[d + 1]; i++) {
                const mte_op& o = b->ops[i];
                if (o.type != MTE_OP_CELL) continue;
                if (o.b >= (1u << 28)) return set_err(e, MTE_E_RANGE, "cell index beyond 2^28");
                v.push_back({o.b, o.seq, o.props < b->n_vals ? o.props : 0u});
                e->n_cells = std::max<uint64_t>(e->n_cells, (uint64_t)o.b + 1);
            }
        }
        if (h0.empty()) h0.push_back(1);  // new HandleTable(): [1]
        // every set allocates at most one handle per vector
        c.ht_cap = (uint32_t)h0.size() + n_cell[d] + 2;
        c.ht_off = words;
        words += 1 + 2 * (uint64_t)c.ht_cap;
        init.push_back((uint32_t)h0.size());
        init.insert(init.end(), h0.begin(), h0.end());
        init.resize(words, 0u);  // the rest of the handles, and no handle freed yet
        any = true;
    }
    e->P.cell_pos = e->P.cell_h = e->P.htab = nullptr;
    e->P.htab0 = nullptr;
    if (!any) return MTE_OK;
    if (e->d_htab.n < words) HIP_TRY(e, e->d_htab.alloc(words));
    if (e->d_htab0.n < words) HIP_TRY(e, e->d_htab0.alloc(words));
    HIP_TRY(e, hipMemcpyAsync(e->d_htab0.p, init.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    e->P.htab = e->d_htab.p;
    e->P.htab0 = e->d_htab0.p;
    if (!e->n_cells) return MTE_OK;
    if (e->d_cell_pos.n < 2 * e->n_cells) HIP_TRY(e, e->d_cell_pos.alloc(2 * e->n_cells));
    if (e->d_cell_h.n < 2 * e->n_cells) HIP_TRY(e, e->d_cell_h.alloc(2 * e->n_cells));
    // a cell index no document carries keeps both positions undefined
    HIP_TRY(e, hipMemsetAsync(e->d_cell_pos.p, 0xFF, 2 * e->n_cells * sizeof(uint32_t), e->stream));
    HIP_TRY(e, hipMemsetAsync(e->d_cell_h.p, 0, 2 * e->n_cells * sizeof(uint32_t), e->stream));
    e->P.cell_pos = e->d_cell_pos.p;
    e->P.cell_h = e->d_cell_h.p;
    return MTE_OK;
}

int mte_load(mte_engine* e, const mte_batch* b) {
    if (!e || !b) return MTE_E_ARG;
    HIP_TRY(e, hipSetDevice(e->device));
    mx_drop_tables(e);
    mk_drop_cache(e);
    copy_batch(e->hb, b, false);
    e->emit_tables = false;
    e->generated = false;
    e->host_ops_valid = false;
    e->replayed = e->downloaded = false;
    e->stage_copy_ms = e->stage_wait_ms = 0;
    e->P.cell_mode = 0;  // (the last replay's pass number is not this batch's: solo_count reads it)
    const uint32_t nd = b->n_docs;
    std::vector<uint64_t> n_ops(nd), pay(nd), pi(nd), an(nd);
    std::vector<uint8_t> collab(nd), has_nl(nd, 0), not_lean(nd, 0), doc_ext(nd, 0), doc_cu(nd, 0), not_rows(nd, 0),
        wide(nd, 0);
    std::vector<uint32_t> doc_keys(nd, 0);  // distinct property keys of each document's ops
    std::vector<uint32_t> n_cell(nd, 0);    // SharedMatrix cell records (MTE_OP_CELL)
    // one pass over each document's ops and payload, documents spread over host threads (the scan is
    // most of mte_load's host time on large batches)
    auto scan = [&](uint32_t d) {
        for (uint64_t q = b->doc_payload_offsets[d]; q < b->doc_payload_offsets[d + 1]; q++)
            if (b->payload[q] == (uint16_t)'\n') {
                has_nl[d] = 1;
                break;
            }
        n_ops[d] = b->doc_op_offsets[d + 1] - b->doc_op_offsets[d];
        pay[d] = b->doc_payload_offsets[d + 1] - b->doc_payload_offsets[d];
        bool rel = false;
        count_doc_ops(b->ops, b->doc_op_offsets, d, pi[d], an[d], &rel);
        std::vector<uint32_t> keys;
        for (uint64_t i = b->doc_op_offsets[d]; i < b->doc_op_offsets[d + 1]; i++) {
            if ((b->ops[i].flags & MTE_F_PERM) || b->ops[i].type == MTE_OP_CELL) doc_ext[d] = 1;
            if (b->ops[i].type > MTE_OP_NOOP) not_rows[d] = 1;  // summary loads: the row engine would spill
            if (b->ops[i].type == MTE_OP_CELL) n_cell[d]++;
            if (b->ops[i].flags & MTE_F_CATCHUP) doc_cu[d] = 1;
            const uint32_t ps = b->ops[i].props;
            if (ps && ps < b->n_propsets)
                for (uint32_t q = 0; q < b->propsets[ps].count; q++) keys.push_back(b->prop_keys[b->propsets[ps].first + q]);
        }
        if (keys.size() > 7) {  // only a document that could exceed the narrow record pays the sort
            std::sort(keys.begin(), keys.end());
            doc_keys[d] = (uint32_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
        }
        collab[d] = e->hb.client(d, 0).empty() ? 0 : 1;  // empty observer name => local, non-collab
        // writers 32..63: FULL kernels (the lean LDS engine's removers masks are 32 bits), and the
        // WIDE row engine in k_rows (a second removers word per slot)
        const uint32_t n_names = e->hb.doc_client_offsets[d + 1] - e->hb.doc_client_offsets[d];
        wide[d] = n_names > 32;
        // (clients 64..127: the LDS / HBM engines only, whose overlap masks have a second word)
        not_rows[d] = not_rows[d] || has_nl[d] || rel || n_names > 64;
        not_lean[d] = not_rows[d] || wide[d] || pi[d] || an[d];
        // a local, non-collaborative document is the LDS engine's path (lean or not): RegEngine::replay
        // hands it over at op 0, and k_rows has no LDS plan to hand it to
        not_rows[d] = not_rows[d] || !collab[d];
        // a document with more than MTE_MAX_CLIENTS clients in a window fails alone (MTE_DOC_UNSUPPORTED at its
        // first op from a client beyond the cap), never the batch
    };
    {
        const unsigned nt = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (nd + 255) / 256}));
        std::atomic<uint32_t> next{0};
        auto work = [&]() {
            for (uint32_t d0; (d0 = next.fetch_add(256)) < nd;)
                for (uint32_t d = d0; d < std::min(nd, d0 + 256); d++) scan(d);
        };
        run_pool(nt, work);
    }
    bool lean = true, ext = false, cu_any = false, rows_ok = true, any_wide = false;
    uint32_t max_keys = 7;
    for (uint32_t d = 0; d < nd; d++) max_keys = std::max(max_keys, std::min<uint32_t>(doc_keys[d], MTE_MAX_PROPS));
    e->map_words = ((1 + 2 * max_keys) + 3) & ~3u;  // 16 for up to 7 keys, 128 for MTE_MAX_PROPS
    for (uint32_t d = 0; d < nd; d++) {
        lean = lean && !not_lean[d];
        rows_ok = rows_ok && !not_rows[d];
        any_wide = any_wide || wide[d];
        ext = ext || doc_ext[d];
        cu_any = cu_any || doc_cu[d];
    }
    auto t0 = std::chrono::steady_clock::now();
    int rc;
    // which documents carry cell records, before the layout: its slot plan asks solo_count, which
    // keeps them out of k_solo (load_cells fills in the records; the last load's set must not answer)
    e->cell_recs.clear();
    for (uint32_t d = 0; d < nd; d++)
        if (n_cell[d]) e->cell_recs[d];
    if ((rc = layout_and_alloc(e, n_ops, pay, pi, an, collab, has_nl, 0, b->doc_op_offsets, b->doc_payload_offsets)))
        return rc;
    e->last_alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // catch-up delta records (legacy summaries): an insert has one range, a remove / annotate at most
    // one per character of its range (every delta segment is visible in the op's view), or at most
    // every segment when a position is relative
    uint64_t cu = 0;
    for (uint32_t d = 0; d < nd && cu_any; d++) {  // (no catch-up record in a batch without catch-up ops)
        DocCfg& c = e->cfg[d];
        uint64_t cap = 0;
        for (uint64_t i = b->doc_op_offsets[d]; i < b->doc_op_offsets[d + 1]; i++) {
            const mte_op& o = b->ops[i];
            if (!(o.flags & MTE_F_CATCHUP)) continue;
            if (o.type == MTE_OP_INSERT || o.type == MTE_OP_INSERT_MARKER) cap += 1;
            else if (o.flags & MTE_F_REL) cap += c.seg_cap;
            else cap += (uint64_t)std::max<int64_t>(0, (int64_t)o.a - (int64_t)o.pos1);
        }
        c.cu_off = cu;
        c.cu_cap = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFF0ull);
        cu += c.cu_cap;
    }
    // (the catch-up offsets reach the device with the cell tables' below: the same size, copied into
    // the buffer the kernels' Params::docs already points at -- upload would reallocate it)
    if (cu) HIP_TRY(e, e->d_cu.alloc(2 * cu));
    e->P.cu_rec = cu ? e->d_cu.p : nullptr;
    if ((rc = load_cells(e, b, n_cell))) return rc;
    if (cu || e->n_cells)  // ht_off / ht_cap: the same re-upload as the catch-up offsets above
        HIP_TRY(e, hipMemcpyAsync(e->d_cfg.p, e->cfg.data(), e->cfg.size() * sizeof(DocCfg), hipMemcpyHostToDevice,
                                  e->stream));
    if ((rc = upload(e, e->d_ops, b->ops, b->doc_op_offsets[nd]))) return rc;
    if ((rc = upload(e, e->d_payload, b->payload, b->doc_payload_offsets[nd]))) return rc;
    if ((rc = upload_props(e))) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    e->last_h2d_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    e->P.ops = e->d_ops.p;
    e->P.payload = e->d_payload.p;
    // catch-up delta records are only read by the SnapshotLegacy writer: a batch whose only extension
    // is MTE_F_CATCHUP runs the lean / FULL kernels (which ignore the flag) unless the replay emits
    // the legacy format (run_kernel decides, snapshot_format may change after the load)
    e->lean_base = lean;
    e->props_rows_ok = rows_ok;
    e->doc_not_rows = not_rows;
    e->rows_wide = any_wide;
    e->ext_perm = ext;
    e->ext_cu = cu_any;
    e->lean_ok = lean && !ext;
    e->ext_needed = ext;
    if ((rc = alloc_out_text(e))) return rc;
    if (e->retain) return ck_match_batch(e, b);
    e->ck.reset();
    return MTE_OK;
}

// The generator's property sets: every single-key set and every two-key set over the C3 keys and
// values, in a fixed order.
static uint32_t build_generator_props(mte_engine* e) {
    Interner in(&e->hb);
    const char16_t* keys[4] = {u"bold", u"italic", u"color", u"size"};
    const char* vals[7] = {"true", "false", "\"red\"", "\"blue\"", "10", "12", "null"};
    uint32_t kid[4], vid[7];
    for (int i = 0; i < 4; i++) kid[i] = in.key(keys[i]);
    for (int i = 0; i < 7; i++) vid[i] = in.val(vals[i]);
    uint32_t n = 0;
    for (int k = 0; k < 4; k++)
        for (int v = 0; v < 7; v++) {
            in.intern_kv({kid[k], vid[v]});
            n++;
        }
    for (int k1 = 0; k1 < 4; k1++)
        for (int k2 = k1 + 1; k2 < 4; k2++)
            for (int v1 = 0; v1 < 7; v1++)
                for (int v2 = 0; v2 < 7; v2++) {
                    in.intern_kv({kid[k1], vid[v1], kid[k2], vid[v2]});
                    n++;
                }
    return n;
}

int mte_generate(mte_engine* e, uint32_t kind, uint32_t n_docs, uint32_t n_ops, const uint32_t* ops_per_doc,
                 uint32_t n_clients, uint64_t seed_base) {
    return mte_generate_ids(e, kind, n_docs, n_ops, ops_per_doc, nullptr, n_clients, seed_base);
}

int mte_generate_ids(mte_engine* e, uint32_t kind, uint32_t n_docs, uint32_t n_ops, const uint32_t* ops_per_doc,
                     const uint32_t* doc_ids, uint32_t n_clients, uint64_t seed_base) {
    if (!e || n_docs == 0 || n_clients == 0 || n_clients >= GEN_MAX_CLIENTS) return MTE_E_ARG;
    e->map_words = MAP_WORDS;  // the generator's property sets hold at most four keys
    if (kind != 2 && kind != 3 && kind != 5) return set_err(e, MTE_E_ARG, "generator kind must be 2, 3 or 5");
    HIP_TRY(e, hipSetDevice(e->device));
    mx_drop_tables(e);
    mk_drop_cache(e);
    e->ck.reset();  // (a new batch: no checkpoint of the last one may be continued)
    e->P.cell_mode = 0;
    e->hb = HostBatch();
    uint32_t nps = build_generator_props(e);
    std::vector<uint64_t> nops(n_docs), pay(n_docs), pi(n_docs), an(n_docs);
    std::vector<uint8_t> collab(n_docs, 1), has_nl(n_docs, 0);
    for (uint32_t d = 0; d < n_docs; d++) {
        uint64_t n = ops_per_doc ? ops_per_doc[d] : n_ops;
        nops[d] = n;
        pay[d] = 8 * n;
        // kind 3 draws 45 % inserts / 20 % annotates (engine.hpp generate_run): property-map capacity
        // from n/2 and n/4 (the layout adds 4 maps per annotate), not n each -- 5n maps per document
        // (3.2 MB) put the 64k-document C3 batch past the 288 GB of HBM
        pi[d] = kind == 3 ? n / 2 + 64 : 0;
        an[d] = kind == 3 ? n / 4 + 64 : 0;
        e->hb.doc_op_offsets.push_back(e->hb.doc_op_offsets.back() + n);
        e->hb.doc_payload_offsets.push_back(e->hb.doc_payload_offsets.back() + 8 * n);
    }
    int rc;
    // generated docs hover around a 2048-char target length: 64K-unit semispaces are ample
    if ((rc = layout_and_alloc(e, nops, pay, pi, an, collab, has_nl, 65536, nullptr, nullptr, doc_ids))) return rc;
    // generated documents carry no SharedMatrix cell ops: drop an earlier load's cell records, so
    // solo_count and the matrix snapshot never see them (load_cells does the same for a cell-free batch)
    e->cell_recs.clear();
    e->n_cells = 0;
    e->P.cell_pos = e->P.cell_h = e->P.htab = nullptr;
    for (uint32_t d = 0; d < n_docs; d++) e->cfg[d].ht_cap = e->cfg[d].ht_off = 0;
    HIP_TRY(e, e->d_ops.alloc(e->hb.doc_op_offsets.back()));
    HIP_TRY(e, e->d_payload.alloc(e->hb.doc_payload_offsets.back()));
    HIP_TRY(e, hipMemsetAsync(e->d_payload.p, 0, e->d_payload.n * sizeof(uint16_t), e->stream));
    HIP_TRY(e, e->d_first_seen.alloc((size_t)n_docs * GEN_MAX_CLIENTS));
    HIP_TRY(e, hipMemsetAsync(e->d_first_seen.p, 0xFF, (size_t)n_docs * GEN_MAX_CLIENTS * 4, e->stream));
    if ((rc = upload_props(e))) return rc;
    e->P.ops = e->d_ops.p;
    e->P.payload = e->d_payload.p;
    if ((rc = alloc_out_text(e))) return rc;
    e->P.gen_first_seen = e->d_first_seen.p;
    e->P.gen_kind = kind;
    e->P.gen_nclients = n_clients;
    e->P.gen_seed = seed_base;
    e->P.gen_n_propsets = nps;
    e->gen_kind = kind;
    e->emit_tables = false;  // names are known after the generator ran
    // kinds 2 and 5 draw no properties and no '\n'; short ids stay below 1 + n_clients
    e->lean_ok = e->lean_base = kind != 3 && n_clients < 32;
    e->props_rows_ok = true;
    e->rows_wide = n_clients >= 32;  // (and then FULL: lean_ok is false)
    e->ext_needed = e->ext_perm = e->ext_cu = false;
    rc = run_kernel(e, true);
    if (rc) return rc;
    // client names: observer + writers in first-appearance (short id) order
    std::vector<uint32_t> fs((size_t)n_docs * GEN_MAX_CLIENTS);
    HIP_TRY(e, hipMemcpy(fs.data(), e->d_first_seen.p, fs.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t d = 0; d < n_docs; d++) {
        std::vector<std::string> names{"__observer__"};
        for (uint32_t s = 1; s < GEN_MAX_CLIENTS; s++) {
            uint32_t w = fs[(size_t)d * GEN_MAX_CLIENTS + s];
            if (w == 0xFFFFFFFFu) break;
            names.push_back("client-" + std::to_string(w));
        }
        for (auto& nm : names) {
            e->hb.client_names += nm;
            e->hb.client_name_offsets.push_back(e->hb.client_names.size());
        }
        e->hb.doc_client_offsets.push_back(e->hb.doc_client_offsets.back() + (uint32_t)names.size());
    }
    e->generated = true;
    e->host_ops_valid = false;
    return MTE_OK;
}

int ensure_host_ops(mte_engine* e) {
    if (e->host_ops_valid) return MTE_OK;
    // (the device buffers may be larger than the batch: DevBuf::fit keeps earlier allocations)
    e->hb.ops.resize(e->hb.doc_op_offsets.empty() ? 0 : e->hb.doc_op_offsets.back());
    e->hb.payload.resize(e->hb.doc_payload_offsets.empty() ? 0 : e->hb.doc_payload_offsets.back());
    HIP_TRY(e, hipMemcpy(e->hb.ops.data(), e->d_ops.p, e->hb.ops.size() * sizeof(mte_op), hipMemcpyDeviceToHost));
    HIP_TRY(e, hipMemcpy(e->hb.payload.data(), e->d_payload.p, e->hb.payload.size() * 2, hipMemcpyDeviceToHost));
    e->host_ops_valid = true;
    return MTE_OK;
}

int mte_export_batch(mte_engine* e, mte_batch* out) {
    if (!e || !out) return MTE_E_ARG;
    if (!e->P.ops) return set_err(e, MTE_E_STATE, "nothing loaded");
    int rc = ensure_host_ops(e);
    if (rc) return rc;
    e->hb.view(out);
    return MTE_OK;
}
