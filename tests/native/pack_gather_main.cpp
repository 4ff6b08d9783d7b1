// TEST INFRASTRUCTURE ONLY: the statistics build of the CPU row engine (reg_cpu.cpp, MTE_CPU_STATS) as a
// stand-alone host program under ASan and UBSan (tests/test_pack_gather_native.py), for the fused pack
// (reg_engine.hpp pack_fused): replays each document given on the command line and prints its event
// counters (reg_engine.hpp RgStat order). No HIP runtime in its link.
//   pack_gather_main <in> <out> [<in> <out> ...]
// The files have pack_fused_main's layout. in: 12 u64 {n_ops, pay_len, seg_cap, arena_cap, kind (0 lean,
// 1 paged, 2 PROPS, 3 PROPS + WIDE), pool_rows, n_propsets, n_keyvals, n_vals, map_words, map_cap, 0}, the
// op records, pay_len + 1 payload units, and for PROPS the propsets (2 words each), keys, values and value
// flags. out: the DocRes record, then n_segs rows of vis (4 words), aux (4 words), ovl (u64), the text
// (pay_len + 16 units) and n_segs map records. One "doc" and one "stats" line per document.
#include <stdio.h>
#include <stdlib.h>

#define MTE_CPU_STATS
#include "reg_cpu.cpp"

struct In {
    FILE* f;
    template <class T>
    std::vector<T> rd(size_t n) {
        std::vector<T> v(n + 1);
        if (n && fread(v.data(), sizeof(T), n, f) != n) {
            fprintf(stderr, "short input\n");
            exit(2);
        }
        return v;
    }
};

static int one(const char* src, const char* dst) {
    In in{fopen(src, "rb")};
    if (!in.f) return 2;
    const std::vector<uint64_t> h = in.rd<uint64_t>(12);
    const uint64_t n_ops = h[0], pay_len = h[1];
    const uint32_t seg_cap = (uint32_t)h[2], arena_cap = (uint32_t)h[3], kind = (uint32_t)h[4], pool = (uint32_t)h[5];
    const uint32_t n_ps = (uint32_t)h[6], n_kv = (uint32_t)h[7], n_vals = (uint32_t)h[8], mw = (uint32_t)h[9], map_cap = (uint32_t)h[10];
    const std::vector<mte_op> ops = in.rd<mte_op>(n_ops);
    const std::vector<uint16_t> pay = in.rd<uint16_t>(pay_len + 1);
    std::vector<uint32_t> ps, keys, vals, flags;
    if (kind >= 2) {
        ps = in.rd<uint32_t>(2 * (size_t)n_ps);
        keys = in.rd<uint32_t>(n_kv);
        vals = in.rd<uint32_t>(n_kv);
        flags = in.rd<uint32_t>(n_vals);
    }
    fclose(in.f);
    const size_t cap = seg_cap;
    std::vector<uint32_t> vis(cap * 4, 0), aux(cap * 4, 0), maps(cap * (mw ? mw : 1), 0);
    std::vector<uint64_t> ovl(cap, 0);
    std::vector<uint16_t> text(pay_len + 16, 0);
    DocRes res;
    memset(&res, 0, sizeof res);
    uint64_t at;
    if (kind == 0)
        at = regcpu_replay(ops.data(), n_ops, pay.data(), (uint32_t)pay_len, seg_cap, arena_cap, vis.data(), aux.data(),
                           ovl.data(), seg_cap, text.data(), text.size(), &res);
    else if (kind == 1)
        at = regcpu_replay_paged(ops.data(), n_ops, pay.data(), (uint32_t)pay_len, seg_cap, arena_cap, vis.data(), aux.data(),
                                 ovl.data(), seg_cap, text.data(), text.size(), &res, pool);
    else
        at = regcpu_replay_props(ops.data(), n_ops, pay.data(), (uint32_t)pay_len, seg_cap, arena_cap, vis.data(), aux.data(),
                                 ovl.data(), seg_cap, text.data(), text.size(), &res, pool, ps.data(), n_ps, keys.data(),
                                 vals.data(), flags.data(), n_vals, mw, map_cap, maps.data(), kind == 3);
    FILE* o = fopen(dst, "wb");
    if (!o) return 2;
    const size_t k = res.n_segs;
    fwrite(&res, sizeof res, 1, o);
    fwrite(vis.data(), 16, k, o);
    fwrite(aux.data(), 16, k, o);
    fwrite(ovl.data(), 8, k, o);
    fwrite(text.data(), 2, text.size(), o);
    fwrite(maps.data(), 4, k * mw, o);
    fclose(o);
    printf("doc stop=%llu status=%d n_segs=%u\n", (unsigned long long)at, res.status, res.n_segs);
    uint64_t st[RS_N + 2];
    regcpu_stats(st, RS_N + 2);
    printf("stats");
    for (uint32_t i = 0; i < RS_N; i++) printf(" %llu", (unsigned long long)st[i]);
    printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3 || !(argc & 1)) return 2;
    for (int i = 1; i + 1 < argc; i += 2)
        if (int rc = one(argv[i], argv[i + 1])) return rc;
    return 0;
}
