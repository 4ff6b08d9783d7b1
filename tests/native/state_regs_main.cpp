// TEST INFRASTRUCTURE ONLY: the statistics build of the CPU row engine (reg_cpu.cpp, MTE_CPU_STATS) as a
// stand-alone host program under ASan and UBSan (tests/test_state_regs_native.py): replays one document's
// op records from a file on the lean or the PROPS + WIDE engine, writes the engine's rows, text and
// result record to another, and prints the event counters (reg_engine.hpp RgStat order), the places
// round 13 restated among them. No HIP runtime in its link.
//   state_regs_main <in> <out>
//   state_regs_main --div      the pack's multiplier division against / and %, every T 0..64 and kk 1..7
// The files have pack_fused_main's layout. in: 12 u64 {n_ops, pay_len, seg_cap, arena_cap, kind (0 lean,
// 3 PROPS + WIDE), 0, n_propsets, n_keyvals, n_vals, map_words, map_cap, 0}, the op records, pay_len + 1
// payload units, and for PROPS the propsets (2 words each), keys, values and value flags. out: the DocRes
// record, then n_segs rows of vis (4 words), aux (4 words), ovl (u64), the text (pay_len + 16 units) and
// n_segs map records.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MTE_CPU_STATS
#include "reg_cpu.cpp"

template <class T>
static std::vector<T> rd(FILE* f, size_t n) {
    std::vector<T> v(n + 1);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return v;
}

static int div_check() {
    uint32_t n = 0;
    for (uint32_t kk = 1; kk <= 7; kk++)
        for (uint32_t T = 0; T <= 64; T++, n++) {
            uint32_t q = ~0u, r = ~0u;
            RegEngine<>::div_mul(T, kk, q, r);
            if (q != T / kk || r != T % kk) {
                printf("div_mul(%u, %u) = %u rem %u, not %u rem %u\n", T, kk, q, r, T / kk, T % kk);
                return 1;
            }
        }
    printf("div ok %u\n", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--div")) return div_check();
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[12];
    if (fread(h, 8, 12, f) != 12) return 2;
    const uint64_t n_ops = h[0], pay_len = h[1];
    const uint32_t seg_cap = (uint32_t)h[2], arena_cap = (uint32_t)h[3], kind = (uint32_t)h[4];
    const uint32_t n_ps = (uint32_t)h[6], n_kv = (uint32_t)h[7], n_vals = (uint32_t)h[8], mw = (uint32_t)h[9], map_cap = (uint32_t)h[10];
    std::vector<mte_op> ops = rd<mte_op>(f, n_ops);
    std::vector<uint16_t> pay = rd<uint16_t>(f, pay_len + 1);
    std::vector<uint32_t> ps, keys, vals, flags;
    if (kind == 3) {
        ps = rd<uint32_t>(f, 2 * (size_t)n_ps);
        keys = rd<uint32_t>(f, n_kv);
        vals = rd<uint32_t>(f, n_kv);
        flags = rd<uint32_t>(f, n_vals);
    } else if (kind != 0) {
        return 2;
    }
    fclose(f);
    const uint32_t cap = seg_cap;
    std::vector<uint32_t> vis((size_t)cap * 4, 0), aux((size_t)cap * 4, 0), maps((size_t)cap * (mw ? mw : 1), 0);
    std::vector<uint64_t> ovl(cap, 0);
    std::vector<uint16_t> text(pay_len + 16, 0);
    DocRes res;
    memset(&res, 0, sizeof res);
    uint64_t at;
    if (kind == 0)
        at = regcpu_replay(ops.data(), n_ops, pay.data(), (uint32_t)pay_len, seg_cap, arena_cap, vis.data(), aux.data(),
                           ovl.data(), cap, text.data(), text.size(), &res);
    else
        at = regcpu_replay_props(ops.data(), n_ops, pay.data(), (uint32_t)pay_len, seg_cap, arena_cap, vis.data(), aux.data(),
                                 ovl.data(), cap, text.data(), text.size(), &res, 0, ps.data(), n_ps, keys.data(),
                                 vals.data(), flags.data(), n_vals, mw, map_cap, maps.data(), 1);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const size_t k = res.n_segs;
    fwrite(&res, sizeof res, 1, o);
    fwrite(vis.data(), 16, k, o);
    fwrite(aux.data(), 16, k, o);
    fwrite(ovl.data(), 8, k, o);
    fwrite(text.data(), 2, text.size(), o);
    fwrite(maps.data(), 4, k * mw, o);
    fclose(o);
    printf("ok stop=%llu status=%d n_segs=%u\n", (unsigned long long)at, res.status, res.n_segs);
    uint64_t st[RS_N + 2];
    regcpu_stats(st, RS_N + 2);
    printf("stats");
    for (uint32_t i = 0; i < RS_N; i++) printf(" %llu", (unsigned long long)st[i]);
    printf("\n");
    return 0;
}
