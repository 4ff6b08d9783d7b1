// engine_ckpt.cpp — the device half of incremental replay (option retain): the checkpoint buffers of a
// retained pass, the block documents' regions and k_blk_ck, and the renumbering of kept block
// checkpoints. What is offered, where every region lies and what is kept for the next pass is decided
// in ck_plan.hpp, which makes no HIP call; engine_load.cpp (mte_load) and engine_run.cpp (run_kernel)
// call in here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/mte.h"
#include "ck_plan.hpp"
#include "engine_host.hpp"
#include "engine_types.hpp"
#include "mte_kernels.h"

// k_ck_xlate over the kept block checkpoints r lists (ck_match's, the tables did not extend the kept ones)
static int renumber(mte_engine* e, const CkRenumber& r) {
    DevBuf<uint64_t> d_off, d_cap;
    DevBuf<uint32_t> d_kx, d_vx;
    HIP_TRY(e, d_off.alloc(r.off.size()));
    HIP_TRY(e, d_cap.alloc(r.cap.size()));
    HIP_TRY(e, d_kx.alloc(r.key.size()));
    HIP_TRY(e, d_vx.alloc(r.val.size()));
    HIP_TRY(e, hipMemcpy(d_off.p, r.off.data(), r.off.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(d_cap.p, r.cap.data(), r.cap.size() * 8, hipMemcpyHostToDevice));
    if (!r.key.empty()) HIP_TRY(e, hipMemcpy(d_kx.p, r.key.data(), r.key.size() * 4, hipMemcpyHostToDevice));
    if (!r.val.empty()) HIP_TRY(e, hipMemcpy(d_vx.p, r.val.data(), r.val.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(e, launch_ck_xlate(e->d_ck[e->ck.cur].p, d_off.p, d_cap.p, (uint32_t)r.off.size(), d_kx.p, (uint32_t)r.key.size(),
                               d_vx.p, (uint32_t)r.val.size(), e->map_words, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return MTE_OK;
}

int ck_match_batch(mte_engine* e, const mte_batch* b) {
    const CkRenumber r = ck_match(e->ck, b, e->hb, e->map_words);
    if (r.off.empty()) return MTE_OK;
    const int rc = renumber(e, r);
    if (rc) e->ck.reset();  // (the kept tables are the loaded ones already, the checkpoints' ids are not)
    return rc;
}

// A retained pass's block documents (engine level <= 1): every document of the pass the row engines
// cannot replay, and every one whose offered checkpoint is a block checkpoint (a k_rows document that
// ever became a block document stays one). Lays out their HBM regions and map tables in e->cfg
// (layout_hbm_docs) and admits them to the checkpoint budget shortest first: one whose region does not
// fit is not listed (e->blk_ck 2) and runs where it runs without retain.
static int blk_plan(mte_engine* e, HbmDocLayout& lay) {
    const uint32_t nall = e->P.n_docs;
    e->blk_ck.assign(nall, 0);
    std::vector<uint32_t> cand;
    for (uint32_t d : e->order)
        if ((e->doc_not_rows.size() == nall && e->doc_not_rows[d]) || (e->ck.have(d) && e->ck.prev[d].kind == 1)) cand.push_back(d);
    if (cand.empty()) return MTE_OK;
    int rc;
    if ((rc = layout_hbm_docs(e, false, cand, lay))) return rc;
    std::vector<CkCand> cs;
    for (uint32_t d : cand) cs.push_back({d, blk_ck_region_words(e->cfg[d], e->map_words), e->n_ops_doc[d]});
    e->last_ck_blk_skipped = ck_admit(cs, e->ck_blk_budget, e->blk_ck);
    for (uint32_t d : cand)
        if (e->blk_ck[d] == 1) e->blk_list.push_back(d);
    if (e->blk_list.size() != cand.size()) return layout_hbm_docs(e, false, e->blk_list, lay);  // the admitted ones alone
    return MTE_OK;
}

int ck_blk_plan(mte_engine* e, bool on, BlkGuard& g) {
    e->blk_list.clear();
    e->blk_ck.clear();
    e->maps_blk.clear();
    e->last_ck_blk_skipped = 0;
    if (!on) return MTE_OK;
    int rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));  // (layout_hbm_docs reads the uploaded op records)
    if ((rc = blk_plan(e, g.lay)) || e->blk_list.empty()) return rc;
    // the rest of the pass is routed as if the block documents were not in the batch
    g.all = e->order;
    g.on = true;
    e->order.erase(std::remove_if(e->order.begin(), e->order.end(), [&](uint32_t d) { return e->blk_ck[d] == 1; }), e->order.end());
    e->d_order_stale = true;
    return upload(e, e->d_order, e->order);
}

// k_blk_ck's regions, map tables, list and counter
int ck_blk_setup(mte_engine* e, const BlkGuard& g, hipStream_t s) {
    if (e->blk_list.empty()) return MTE_OK;
    int rc;
    HIP_TRY(e, e->d_hbm_blk.fit(g.lay.bytes));
    HIP_TRY(e, e->maps_blk.d.fit(std::max<uint64_t>(g.lay.maps, 1) * e->map_words));
    HIP_TRY(e, e->d_blk_saved.fit(1));
    e->maps_blk.set(e->P.n_docs, e->blk_list, e->cfg);
    if ((rc = upload(e, e->d_blk_list, e->blk_list))) return rc;
    HIP_TRY(e, hipMemsetAsync(e->d_blk_saved.p, 0, sizeof(uint32_t), s));
    return MTE_OK;
}

int ck_begin(mte_engine* e) {
    const int out = e->ck.cur == 0 ? 1 : 0;
    const CkRegions r = ck_assign_regions(e->ck, e->cfg, e->blk_ck, e->map_words);
    e->last_ck_offered = r.offered;
    HIP_TRY(e, e->d_ck[out].fit(std::max<uint64_t>(r.total, 64)));
    // every row region invalid until saved; k_blk_ck_clear clears the block regions' header words
    HIP_TRY(e, hipMemsetAsync(e->d_ck[out].p, 0, r.row_total * 4, e->stream));
    HIP_TRY(e, hipMemcpyAsync(e->d_cfg.p, e->cfg.data(), e->cfg.size() * sizeof(DocCfg), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    e->P.ck_out = e->d_ck[out].p;
    e->P.ck_in = e->ck.cur >= 0 ? e->d_ck[e->ck.cur].p : nullptr;
    return MTE_OK;
}

// The block documents of a retained pass: k_blk_ck beside the bulk, each in its own HBM region and map
// table (read back like the re-run documents', fetch_map_record), joined before emission.
int ck_blk_launch(mte_engine* e, int full, hipStream_t s_blk, hipStream_t s_main) {
    const uint32_t n_blk = (uint32_t)e->blk_list.size();
    if (!n_blk) return MTE_OK;
    HIP_TRY(e, hipStreamWaitEvent(s_blk, e->ev_gate, 0));  // (its list and counter went out before ev0)
    Params pb = e->P;
    pb.doc_list = e->d_blk_list.p;
    pb.n_list = n_blk;
    pb.hbm = e->d_hbm_blk.p;
    pb.maps = e->maps_blk.d.p;
    pb.map_rerun = 1;  // (worst-case tables: a full one is a capacity failure)
    HIP_TRY(e, launch_blk_ck(pb, full, n_blk, e->d_blk_saved.p, s_blk));
    HIP_TRY(e, hipEventRecord(e->ev_blk, s_blk));
    HIP_TRY(e, hipStreamWaitEvent(s_main, e->ev_blk, 0));
    return MTE_OK;
}

int ck_end(mte_engine* e, const uint32_t* ctr) {
    const uint32_t nd = (uint32_t)e->cfg.size();
    if (!e->blk_list.empty()) HIP_TRY(e, hipMemcpy(&e->last_ck_blk_saved, e->d_blk_saved.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    // a document that left its rows mid-pass and finished in the checkpointing k_rows_cont (DocRes mode 6)
    // has a row region: its block state fitted if the valid word is there; else nothing was saved and the
    // document stays a row document
    std::vector<uint8_t> row_now_blk(nd, 0);
    for (uint32_t d = 0; d < nd; d++) {
        const bool is_blk = d < e->blk_ck.size() && e->blk_ck[d] == 1;
        if (is_blk || !e->cfg[d].ck_cap || d >= e->res.size() || e->res[d].mode != 6 || e->res[d].status != 0) continue;
        uint32_t magic = 0;
        HIP_TRY(e, hipMemcpy(&magic, e->P.ck_out + e->cfg[d].ck_out_off, sizeof magic, hipMemcpyDeviceToHost));
        row_now_blk[d] = magic == BCK_MAGIC;
        e->last_ck_blk_saved += row_now_blk[d];
    }
    ck_commit(e->ck, e->cfg, e->n_ops_doc, e->blk_ck, row_now_blk, e->hb, e->map_words);
    e->last_resumed_docs = ctr[12];
    e->last_resumed_ops = ctr[13];
    e->last_resumed_docs_blk = ctr[3];
    e->last_resumed_ops_blk = (uint64_t)ctr[14] | ((uint64_t)ctr[15] << 32);
    e->P.ck_out = nullptr;
    e->P.ck_in = nullptr;
    return MTE_OK;
}
