// Host check of BatchMap (clay_amd/csrc/stream_tile_map.hpp), the tile map of the batched
// k_stream_encode: walks the map for a sweep of sub-chunk sizes, stripe counts and workgroups per
// XCD and checks that the launched workgroups' tiles partition every row of every stripe, stripe by
// stripe exactly as BalancedMap cuts one stripe.  Built and run by
// tests/test_stream_batch_map_cpu.py (and under ASan + UBSan by scripts/host_checks_sanitized.sh); exits
// 0 and prints "batch map ok: <cases> cases" when every check holds, else prints the failures and
// exits 1.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "stream_tile_map.hpp"

using clay::bs::BalancedMap;
using clay::bs::batch_groups;
using clay::bs::BatchMap;
using clay::bs::stream_cut;
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

using Tile = std::array<uint32_t, 5>;  // xcd, sub-slot, round, b0, vend

struct Shape {
    uint32_t groups, ns, idle;  // groups per XCD, workgroups per group, unlaunched slots per XCD
    int rounds;                 // of XCD 0
};

static Shape check(uint32_t sc, uint32_t n, uint32_t per_xcd) {
    // the launch geometry of one stripe (stream_cut, as the engine launches it)
    const uint32_t region = stream_cut(sc, per_xcd).region, ns = stream_cut(sc, per_xcd).nslots;
    const uint32_t G = batch_groups(per_xcd, ns, n);
    CHECK(G >= 1 && G <= n && (G * ns <= per_xcd || G == 1), "sc %u n %u per_xcd %u: %u groups of %u", sc, n, per_xcd, G, ns);
    // one stripe's cut, the reference
    std::vector<Tile> ref;
    for (uint32_t xcd = 0; xcd < 8; xcd++)
        for (uint32_t sub = 0; sub < ns; sub++) {
            const BalancedMap m(sc, region, ns, xcd, sub);
            for (int r = 0; r < m.ntile(); r++) {
                const StreamTile t = m.tile(r, sub, ns);
                ref.push_back({xcd, sub, uint32_t(r), t.b0, t.vend});
            }
        }
    std::sort(ref.begin(), ref.end());
    std::vector<std::vector<Tile>> got(n);
    std::vector<uint32_t> group_stripes(G, 0);
    const uint32_t launched = G * ns;  // grid = 8 * launched
    for (uint32_t xcd = 0; xcd < 8; xcd++) {
        for (uint32_t slot = 0; slot < launched; slot++) {
            const BatchMap bm(sc, region, ns, G, n, xcd, slot);
            const BalancedMap m(sc, region, ns, xcd, slot % ns);
            const int nt = m.ntile();
            CHECK(bm.ntile() == nt * bm.stripes(), "sc %u n %u slot %u: %d tiles, %d per stripe x %d stripes", sc, n, slot, bm.ntile(), nt, bm.stripes());
            const uint32_t j = slot / ns;
            CHECK(uint32_t(bm.stripes()) == (n - j + G - 1) / G, "sc %u n %u per_xcd %u group %u: %d stripes", sc, n, per_xcd, j, bm.stripes());
            if (xcd == 0 && slot % ns == 0) group_stripes[j] = uint32_t(bm.stripes());
            int64_t prev = -1;
            for (int k = 0; k < bm.ntile(); k++) {
                const StreamTile t = bm.tile(k, slot, ns);
                CHECK(t.stripe == bm.stripe(k), "sc %u n %u slot %u tile %d: stripe %u vs stripe(k) %u", sc, n, slot, k, t.stripe, bm.stripe(k));
                CHECK(t.stripe < n, "sc %u n %u slot %u tile %d: stripe %u", sc, n, slot, k, t.stripe);
                if (t.stripe >= n) continue;
                CHECK(t.stripe % G == j, "sc %u n %u slot %u: stripe %u in group %u of %u", sc, n, slot, t.stripe, j, G);
                // a stripe's tiles are rounds 0 .. nt - 1 in order, then the next (larger) stripe
                const int r = k % nt;
                if (r == 0) CHECK(int64_t(t.stripe) > prev, "sc %u n %u slot %u tile %d: stripe %u after %lld", sc, n, slot, k, t.stripe, (long long)prev);
                else CHECK(int64_t(t.stripe) == prev, "sc %u n %u slot %u tile %d: stripe %u inside stripe %lld", sc, n, slot, k, t.stripe, (long long)prev);
                prev = t.stripe;
                const StreamTile o = m.tile(r, slot % ns, ns);
                CHECK(t.b0 == o.b0 && t.vend == o.vend, "sc %u n %u slot %u tile %d: [%u, %u), one stripe's round %d is [%u, %u)", sc, n, slot, k, t.b0, t.vend, r, o.b0, o.vend);
                got[t.stripe].push_back({xcd, slot % ns, uint32_t(r), t.b0, t.vend});
            }
        }
        // nothing at or past the grid
        for (uint32_t slot = launched; slot < std::max(launched, per_xcd) + ns + 1; slot++)
            CHECK(BatchMap(sc, region, ns, G, n, xcd, slot).ntile() == 0, "sc %u n %u per_xcd %u xcd %u: slot %u past the grid has tiles", sc, n, per_xcd, xcd, slot);
    }
    const uint32_t lo = *std::min_element(group_stripes.begin(), group_stripes.end());
    const uint32_t hi = *std::max_element(group_stripes.begin(), group_stripes.end());
    CHECK(hi - lo <= 1 && lo >= 1, "sc %u n %u per_xcd %u: groups run %u .. %u stripes", sc, n, per_xcd, lo, hi);
    for (uint32_t s = 0; s < n; s++) {
        // exactly one stripe's cut ...
        std::sort(got[s].begin(), got[s].end());
        CHECK(got[s] == ref, "sc %u n %u per_xcd %u stripe %u: %zu tiles, one stripe's map has %zu", sc, n, per_xcd, s, got[s].size(), ref.size());
        // ... which partitions [0, sc): sorted by start, every tile begins where the one before ended
        std::vector<std::pair<uint32_t, uint32_t>> row;
        for (const Tile &t : got[s]) row.emplace_back(t[3], t[4]);
        std::sort(row.begin(), row.end());
        uint32_t pos = 0;
        for (const auto &t : row) {
            CHECK(t.first == pos, "sc %u n %u stripe %u: tile starts at %u, previous ended at %u (%s)", sc, n, s, t.first, pos, t.first < pos ? "overlap" : "gap");
            pos = t.second;
        }
        CHECK(pos == sc, "sc %u n %u stripe %u: tiles end at %u", sc, n, s, pos);
    }
    return {G, ns, per_xcd > launched ? per_xcd - launched : 0u, BalancedMap(sc, region, ns, 0, 0).rounds()};
}

int main() {
    const uint32_t per_xcds[] = {1, 2, 13, 32, 38};
    const uint32_t stripes[] = {1, 2, 3, 31, 32, 33, 70};
    std::set<uint32_t> scs;
    for (uint32_t sc = 16; sc <= 4096; sc += 8) scs.insert(sc);
    for (uint32_t sc : {6560u, 8200u, 8216u, 26216u, 66176u, 66184u, 419432u}) scs.insert(sc);
    scs.insert(2288);  // (in the sweep already; one of the pinned shapes below)
    long cases = 0;
    for (uint32_t per_xcd : per_xcds)
        for (uint32_t n : stripes)
            for (uint32_t sc : scs) {
                const Shape s = check(sc, n, per_xcd);
                cases++;
                if (per_xcd != 32 || n != 70) continue;
                // the shapes of a 256-CU device (32 workgroups per XCD)
                auto is = [&](uint32_t g, uint32_t ns, uint32_t idle, int rounds) {
                    CHECK(s.groups == g && s.ns == ns && s.idle == idle && s.rounds == rounds,
                          "sc %u: %u groups of %u, %u idle, %d rounds; expected %u of %u, %u idle, %d rounds", sc, s.groups, s.ns,
                          s.idle, s.rounds, g, ns, idle, rounds);
                };
                if (sc == 2048) is(32, 1, 0, 1);
                if (sc == 2288) is(16, 2, 0, 1);
                if (sc == 8216) is(6, 5, 2, 1);
                if (sc == 66176) is(1, 32, 0, 2);
            }
    if (failures) {
        printf("batch map: %d failures\n", failures);
        return 1;
    }
    printf("batch map ok: %ld cases\n", cases);
    return 0;
}
