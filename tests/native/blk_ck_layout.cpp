// TEST INFRASTRUCTURE: the block checkpoint region's layout (engine_types.hpp BlkCkLayout) as a
// stand-alone host program (tests/test_blk_incremental_cpu.py compiles it under ASan + UBSan): over a
// sweep of capacities the sections follow each other without overlap, each starts at a 16-byte
// boundary and holds its array, the total is the layout function's result, and the total is monotone
// in every capacity. It also writes every section of a region allocated at exactly that size, so an
// offset past the total is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fluidframework_amd/csrc/engine_types.hpp"

using namespace mte;

struct Caps {
    u32 blk, ord, in, heap, seg, arena, maps, mw;
    bool o2;
};

static int fails = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            fails++;                          \
            std::printf("FAIL %s: ", #c);     \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
        }                                     \
    } while (0)

static u64 total(const Caps& c) {
    return blk_ck_region_words(c.blk, c.ord, c.in, c.heap, c.seg, c.o2, c.arena, c.maps, c.mw);
}

static void check(const Caps& c) {
    const BlkCkLayout l = BlkCkLayout::of(c.blk, c.ord, c.in, c.heap, c.seg, c.o2, c.arena, c.maps, c.mw);
    // (offset, words the array needs), in region order
    const u64 sec[][2] = {{0, BCK_HDR_WORDS},
                          {l.vis, (u64)c.blk * 8 * 4},
                          {l.aux, (u64)c.blk * 8 * 4},
                          {l.bmeta, c.blk},
                          {l.ord, (u64)c.ord * 4},
                          {l.in_child, (u64)c.in * 8},
                          {l.in_cnt, c.in},
                          {l.in_par, c.in},
                          {l.heap, (u64)c.heap * 2},
                          {l.ovl, (u64)c.seg * 2},
                          {l.ovl2, c.o2 ? (u64)c.seg * 2 : 0},
                          {l.arena, ((u64)c.arena + 1) / 2},
                          {l.maps, (u64)c.maps * c.mw}};
    const size_t n = sizeof sec / sizeof sec[0];
    std::vector<u32> region(l.words);
    for (size_t i = 0; i < n; i++) {
        CHECK(sec[i][0] % 4 == 0, "section %zu at word %llu is not 16-byte aligned", i, (unsigned long long)sec[i][0]);
        const u64 end = sec[i][0] + sec[i][1], next = i + 1 < n ? sec[i + 1][0] : l.words;
        CHECK(end <= next, "section %zu [%llu, %llu) overlaps the next at %llu", i, (unsigned long long)sec[i][0],
              (unsigned long long)end, (unsigned long long)next);
        if (sec[i][1]) std::memset(region.data() + sec[i][0], (int)i + 1, sec[i][1] * 4);
    }
    // every word a section owns still carries that section's mark (no later section wrote into it)
    for (size_t i = 0; i < n; i++)
        for (u64 w = 0; w < sec[i][1]; w++)
            if (region[sec[i][0] + w] != 0x01010101u * (u32)(i + 1)) {
                CHECK(false, "section %zu word %llu overwritten", i, (unsigned long long)w);
                break;
            }
    CHECK(l.words == total(c), "total %llu != %llu", (unsigned long long)l.words, (unsigned long long)total(c));
    CHECK(l.words % 4 == 0, "total %llu not a multiple of 16 bytes", (unsigned long long)l.words);
    // monotone in every capacity
    const u64 t = l.words;
    Caps d;
    d = c, d.blk++;
    CHECK(total(d) >= t, "blk");
    d = c, d.ord++;
    CHECK(total(d) >= t, "ord");
    d = c, d.in++;
    CHECK(total(d) >= t, "in");
    d = c, d.heap++;
    CHECK(total(d) >= t, "heap");
    d = c, d.seg++;
    CHECK(total(d) >= t, "seg");
    d = c, d.arena++;
    CHECK(total(d) >= t, "arena");
    d = c, d.maps++;
    CHECK(total(d) >= t, "maps");
    d = c, d.mw += 4;
    CHECK(total(d) >= t, "map_words");
    d = c, d.o2 = true;
    CHECK(total(d) >= t, "ovl2");
}

int main() {
    const u32 small[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1000, 1021};
    u64 n = 0;
    // every capacity on its own over the small values (the others at odd sizes), then random mixes
    for (int which = 0; which < 7; which++)
        for (u32 v : small)
            for (int o2 = 0; o2 < 2; o2++) {
                Caps c{3, 5, 7, 9, 11, 13, 3, 16, o2 != 0};
                u32* f[] = {&c.blk, &c.ord, &c.in, &c.heap, &c.seg, &c.arena, &c.maps};
                *f[which] = v;
                check(c);
                n++;
            }
    unsigned s = 12345;
    auto rnd = [&](u32 m) {
        s = s * 1664525u + 1013904223u;
        return (s >> 8) % m;
    };
    for (int i = 0; i < 2000; i++) {
        Caps c{rnd(700), rnd(700), rnd(400), rnd(3000), rnd(5000), rnd(60000), rnd(300), 16 + 4 * rnd(29), rnd(2) != 0};
        check(c);
        n++;
    }
    // the capacities hbm_caps gives real documents, and the 32-bit limits (sizes only: no allocation)
    for (u64 ops : {1ull, 1500ull, 65536ull, 10000000ull, 0xFFFFFFFFull}) {
        u32 b, o, i, h;
        hbm_caps(ops, b, o, i, h);
        const u64 t = blk_ck_region_words(b, o, i, h, 0xFFFFFFF0u, true, 0x3FFFFFF8u, 0xFFFFFFF0u, 128);
        const BlkCkLayout l = BlkCkLayout::of(b, o, i, h, 0xFFFFFFF0u, true, 0x3FFFFFF8u, 0xFFFFFFF0u, 128);
        CHECK(t == l.words && l.maps > l.arena && l.arena > l.ovl2 && l.ovl2 > l.ovl && l.ovl > l.heap && l.vis == BCK_HDR_WORDS,
              "order at %llu ops", (unsigned long long)ops);
        CHECK(t > (u64)0xFFFFFFF0u * 128, "64-bit total at %llu ops", (unsigned long long)ops);
    }
    std::printf("%s: %llu layouts, %d failures\n", fails ? "FAILED" : "ok", (unsigned long long)n, fails);
    return fails ? 1 : 0;
}
