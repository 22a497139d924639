// Host check of BalancedMap (clay_amd/csrc/stream_tile_map.hpp), the tile map of k_stream_encode:
// walks the map for a sweep of sub-chunk sizes and workgroup counts and checks that the tiles
// partition every row.  Built and run by tests/test_stream_tile_map_cpu.py; exits 0 and prints
// "tile map ok: <cases> cases" when every check holds, else prints the failures and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "stream_tile_map.hpp"

using clay::bs::BalancedMap;
using clay::bs::StreamTile;

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

// one (sc, ns): ns is the workgroup count per XCD the kernel is launched with (here swept, not
// stream_cut's); the region is the engine's
static void check(uint32_t sc, uint32_t ns, bool bench_shape) {
    const uint32_t region = clay::bs::stream_cut(sc, ns).region;
    std::vector<std::pair<uint32_t, uint32_t>> tiles;  // all tiles of the row, (b0, vend)
    for (uint32_t xcd = 0; xcd < 8; xcd++) {
        const uint32_t x0 = xcd * region, x1 = std::min(x0 + region, sc);
        if (x0 >= x1) {
            for (uint32_t slot = 0; slot < ns; slot++)
                CHECK(BalancedMap(sc, region, ns, xcd, slot).ntile() == 0, "sc %u ns %u xcd %u: tiles in an empty region", sc, ns, xcd);
            continue;
        }
        const uint32_t len = x1 - x0, R = (len + ns * 256 - 1) / (ns * 256);
        std::vector<uint32_t> per_slot(ns, 0), round_w(R, 0);
        uint32_t short_last = 0;
        for (uint32_t slot = 0; slot < ns; slot++) {
            const BalancedMap m(sc, region, ns, xcd, slot);
            CHECK(uint32_t(m.rounds()) == R, "sc %u ns %u xcd %u: %d rounds, expected %u", sc, ns, xcd, m.rounds(), R);
            CHECK(m.ntile() >= 0 && uint32_t(m.ntile()) <= R, "sc %u ns %u xcd %u slot %u: %d passes > R = %u", sc, ns, xcd, slot, m.ntile(), R);
            CHECK(uint32_t(m.ntile()) + 1 >= R, "sc %u ns %u xcd %u slot %u: %d passes, only the last tile may be empty", sc, ns, xcd, slot, m.ntile());
            for (int k = 0; k < m.ntile(); k++) {
                const StreamTile t = m.tile(k, slot, ns);
                const uint32_t w = t.vend - t.b0, full = m.width(uint32_t(k));
                CHECK(t.b0 < t.vend, "sc %u ns %u xcd %u slot %u tile %d: empty", sc, ns, xcd, slot, k);
                CHECK(t.b0 % 16 == 0, "sc %u ns %u tile start %u", sc, ns, t.b0);
                CHECK(w <= 256 && full <= 256 && full % 16 == 0 && full >= 16, "sc %u ns %u width %u (round width %u)", sc, ns, w, full);
                CHECK(w % 16 == 0 || t.vend == x1, "sc %u ns %u: width %u inside a region", sc, ns, w);
                CHECK(t.b0 >= x0 && t.vend <= x1, "sc %u ns %u xcd %u: tile [%u, %u) outside [%u, %u)", sc, ns, xcd, t.b0, t.vend, x0, x1);
                CHECK(w == full || uint32_t(k) + 1 == R, "sc %u ns %u: clipped tile in round %d of %u", sc, ns, k, R);
                if (slot == 0) round_w[uint32_t(k)] = full;
                per_slot[slot] += w;
                tiles.emplace_back(t.b0, t.vend);
            }
            if (uint32_t(m.ntile()) < R || m.tile(int(R) - 1, slot, ns).vend - m.tile(int(R) - 1, slot, ns).b0 < m.width(R - 1)) short_last++;
        }
        uint32_t wmin = 256, wmax = 0;
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t w = BalancedMap(sc, region, ns, xcd, 0).width(r);
            wmin = std::min(wmin, w);
            wmax = std::max(wmax, w);
        }
        CHECK(wmax - wmin <= 16, "sc %u ns %u xcd %u: round widths %u .. %u", sc, ns, xcd, wmin, wmax);
        const uint32_t lo = *std::min_element(per_slot.begin(), per_slot.end()), hi = *std::max_element(per_slot.begin(), per_slot.end());
        CHECK(hi - lo <= wmax, "sc %u ns %u xcd %u: per-slot bytes %u .. %u differ by more than a round width %u", sc, ns, xcd, lo, hi, wmax);
        if (bench_shape) {
            // T = 103 pieces over R = 7 rounds: five of 240 bytes, then two of 224
            CHECK(R == 7, "bench shape: %u rounds", R);
            for (uint32_t r = 0; r < R && R == 7; r++)
                CHECK(round_w[r] == (r < 5 ? 240u : 224u), "bench shape xcd %u: round %u is %u wide", xcd, r, round_w[r]);
            CHECK(short_last <= 3, "bench shape xcd %u: %u slots with a short or empty last tile", xcd, short_last);
        }
    }
    // partition of [0, sc): sorted by start, every tile begins where the one before ended
    std::sort(tiles.begin(), tiles.end());
    uint32_t pos = 0;
    for (const auto &t : tiles) {
        CHECK(t.first == pos, "sc %u ns %u: tile starts at %u, previous ended at %u (%s)", sc, ns, t.first, pos, t.first < pos ? "overlap" : "gap");
        pos = t.second;
    }
    CHECK(pos == sc, "sc %u ns %u: tiles end at %u", sc, ns, pos);
}

int main() {
    const uint32_t nss[] = {1, 2, 13, 32, 38};
    const int deltas[] = {0, 8, 16, 24, 40};
    long cases = 0;
    for (uint32_t ns : nss) {
        std::set<uint32_t> scs;
        for (uint32_t sc = 8; sc <= 20000; sc += 8) scs.insert(sc);
        for (uint32_t k = 1; k <= 8; k++)
            for (int d : deltas) {
                scs.insert(k * ns * 2048 + uint32_t(d));
                if (k * ns * 2048 > uint32_t(d)) scs.insert(k * ns * 2048 - uint32_t(d));
            }
        scs.insert(419432);
        for (uint32_t sc : scs) {
            check(sc, ns, sc == 419432 && ns == 32);
            cases++;
        }
    }
    if (failures) {
        printf("tile map: %d failures\n", failures);
        return 1;
    }
    printf("tile map ok: %ld cases\n", cases);
    return 0;
}
