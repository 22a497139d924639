// Host check of the column map of the batch k_bs_repair (clay_amd/csrc/repair_batch_map.hpp):
// walks the map the way the kernel does (workgroup -> tile in the XCD-contiguous order, lane ->
// column -> stripe, position, valid bytes) for a sweep of lanes per plane layer, sub-chunk sizes
// and stripe counts, and checks that every byte of every stripe is owned by exactly one (tile,
// lane).  Built and run by tests/test_repair_batch_map_cpu.py; exits 0 and prints
// "repair batch map ok: <cases> cases" when every check holds, else prints the failures and exits 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "repair_batch_map.hpp"

using namespace clay::bs;

static int failures = 0;

#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (failures++ < 20) {             \
                printf("FAIL %s: ", #cond);    \
                printf(__VA_ARGS__);           \
                printf("\n");                  \
            }                                  \
        }                                      \
    } while (0)

static void check(uint32_t parts, uint32_t sc, uint32_t ns) {
    // the host side as engine.hip / repair_stream.hip compute it
    const uint32_t cps = uint32_t(rep_batch_cps(sc));
    const uint32_t ncols = uint32_t(rep_batch_ncols(sc, ns));
    const uint32_t ntiles = uint32_t(rep_batch_ntiles(ncols, parts));
    const uint32_t per_xcd = (ntiles + 7) / 8;
    // the same counts from first principles
    uint32_t cols1 = 0;
    for (uint32_t p = 0; p < sc; p += 32) cols1++;
    CHECK(cps == cols1, "parts %u sc %u: cps %u vs %u", parts, sc, cps, cols1);
    CHECK(ncols == cols1 * ns, "parts %u sc %u ns %u: ncols %u", parts, sc, ns, ncols);
    uint32_t tiles1 = 0;
    for (uint64_t c = 0; c < uint64_t(cols1) * ns; c += parts) tiles1++;
    CHECK(ntiles == tiles1, "parts %u sc %u ns %u: ntiles %u vs %u", parts, sc, ns, ntiles, tiles1);

    std::vector<uint8_t> owned(size_t(ns) * sc, 0), seen(ntiles, 0);
    for (uint32_t block = 0; block < per_xcd * 8; block++) {
        const uint32_t tix = (block & 7u) * per_xcd + (block >> 3);
        if (tix >= ntiles) continue;
        CHECK(!seen[tix], "parts %u sc %u ns %u: tile %u run twice", parts, sc, ns, tix);
        seen[tix] = 1;
        const bool full = rep_batch_tile_full(tix, parts, ncols, sc);
        for (uint32_t part = 0; part < parts; part++) {
            const uint32_t col = tix * parts + part;
            const RepBatchCol c = rep_batch_col(col, ncols, cps, sc);
            CHECK(c.nv <= 32, "parts %u sc %u ns %u col %u: nv %u", parts, sc, ns, col, c.nv);
            if (full) CHECK(c.nv == 32, "parts %u sc %u ns %u tile %u part %u: full tile with nv %u", parts, sc, ns, tix, part, c.nv);
            if (c.nv == 0) {
                CHECK(col >= ncols, "parts %u sc %u ns %u col %u: empty column inside the batch", parts, sc, ns, col);
                continue;
            }
            CHECK(c.stripe < ns && uint64_t(c.pos) + c.nv <= sc, "parts %u sc %u ns %u col %u: stripe %u pos %u nv %u", parts, sc,
                  ns, col, c.stripe, c.pos, c.nv);
            if (c.stripe >= ns || uint64_t(c.pos) + c.nv > sc) continue;
            for (uint32_t b = 0; b < c.nv; b++) owned[size_t(c.stripe) * sc + c.pos + b]++;
        }
    }
    for (uint32_t t = 0; t < ntiles; t++) CHECK(seen[t], "parts %u sc %u ns %u: tile %u never run", parts, sc, ns, t);
    for (size_t i = 0; i < owned.size(); i++)
        if (owned[i] != 1) {
            CHECK(owned[i] == 1, "parts %u sc %u ns %u: byte %zu of stripe %zu owned %u times", parts, sc, ns, i % sc, i / sc,
                  unsigned(owned[i]));
            break;
        }
}

int main() {
    std::vector<uint32_t> scs, nss;
    for (uint32_t sc = 1; sc <= 300; sc++) scs.push_back(sc);
    for (int d : {0, 5, 8}) {
        scs.push_back(2048u + uint32_t(d));
        if (d) scs.push_back(2048u - uint32_t(d));
    }
    scs.push_back(4101);
    for (uint32_t ns = 1; ns <= 70; ns++) nss.push_back(ns);
    nss.push_back(300);
    long cases = 0;
    for (uint32_t parts : {64u, 9u, 4u})  // (4,2,5), (9,3,11), (10,4,13)
        for (uint32_t sc : scs)
            for (uint32_t ns : nss) {
                check(parts, sc, ns);
                cases++;
            }
    if (failures) {
        printf("%d failures\n", failures);
        return 1;
    }
    printf("repair batch map ok: %ld cases\n", cases);
    return 0;
}
