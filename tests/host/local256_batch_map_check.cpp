// Host check of the tile map of the batched k_stream_local256 (clay_amd/csrc/stream_tile_map.hpp:
// BatchMapOf<StreamMap>, the decode's one-stripe cut under the batch grouping of BatchMap): walks
// the map for a sweep of sub-chunk sizes, stripe counts and workgroups per XCD and checks that the
// launched workgroups' tiles partition every row of every stripe, stripe by stripe exactly as
// StreamMap cuts one stripe, and that every tile is one the kernel can take (at most 256 bytes
// inside the row, 16-byte pieces with at most one 8-byte tail at the row's end).  The loader and the
// compute waves of a workgroup both count their tiles with ntile() of this one map, so the walk
// below is the count both sides see; the loader takes its tiles with tile(k), the compute waves with
// the map's division-free Walk, and the two sequences are compared tile by tile.  Built and run by
// tests/test_local256_batch_map_cpu.py; exits 0 and prints "local256 batch map ok: <cases> cases"
// when every check holds, else prints the failures and exits 1.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "stream_tile_map.hpp"

using clay::bs::batch_groups;
using clay::bs::BatchMapOf;
using clay::bs::stream_cut;
using clay::bs::StreamMap;
using clay::bs::StreamTile;
using Local256BatchMap = BatchMapOf<StreamMap>;

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

using Tile = std::array<uint32_t, 5>;  // xcd, sub-slot, tile of the stripe, b0, vend

struct Shape {
    uint32_t groups, ns, idle;   // groups per XCD, workgroups per group, unlaunched slots per XCD
    uint32_t full, partial;      // tiles of one stripe
    uint32_t empty_xcds;         // XCDs whose region lies past the row's end
    uint32_t most;               // the most tiles of one stripe in a workgroup
    uint32_t tail_b0, tail_end;  // the tile with a piece straddling the row's end (0, 0: none)
    bool full_first;             // every workgroup runs its full tiles before its partial one
};

static Shape check(uint32_t sc, uint32_t n, uint32_t per_xcd) {
    // the launch geometry of one stripe (stream_cut, as the engine launches it)
    const uint32_t region = stream_cut(sc, per_xcd).region, ns = stream_cut(sc, per_xcd).nslots;
    const uint32_t G = batch_groups(per_xcd, ns, n);
    CHECK(G >= 1 && G <= n && (G * ns <= per_xcd || G == 1), "sc %u n %u per_xcd %u: %u groups of %u", sc, n, per_xcd, G, ns);
    Shape sh{G, ns, 0, 0, 0, 0, 0, 0, 0, true};
    // one stripe's cut, the reference
    std::vector<Tile> ref;
    for (uint32_t xcd = 0; xcd < 8; xcd++) {
        uint32_t in_xcd = 0;
        for (uint32_t sub = 0; sub < ns; sub++) {
            const StreamMap m(sc, region, ns, xcd, sub);
            sh.most = std::max(sh.most, uint32_t(m.ntile()));
            bool seen_partial = false;
            for (int r = 0; r < m.ntile(); r++) {
                const StreamTile t = m.tile(r, sub, ns);
                ref.push_back({xcd, sub, uint32_t(r), t.b0, t.vend});
                in_xcd++;
                // what the kernel asks of a tile
                CHECK(t.b0 < t.vend && t.vend <= sc && t.vend - t.b0 <= 256u && t.b0 % 16u == 0 && t.vend >= 16u,
                      "sc %u per_xcd %u xcd %u sub %u tile %d: [%u, %u)", sc, per_xcd, xcd, sub, r, t.b0, t.vend);
                const uint32_t tail = (t.vend - t.b0) % 16u;
                CHECK(tail == 0 || (tail == 8 && t.vend == sc), "sc %u tile [%u, %u): tail of %u bytes", sc, t.b0, t.vend, tail);
                if (tail) {
                    CHECK(sh.tail_end == 0, "sc %u: a second tile with a tail, [%u, %u)", sc, t.b0, t.vend);
                    sh.tail_b0 = t.b0;
                    sh.tail_end = t.vend;
                }
                const bool whole = t.vend - t.b0 == 256u;
                (whole ? sh.full : sh.partial)++;
                if (whole && seen_partial) sh.full_first = false;
                seen_partial = seen_partial || !whole;
            }
        }
        sh.empty_xcds += in_xcd == 0 ? 1u : 0u;
    }
    std::sort(ref.begin(), ref.end());
    std::vector<std::vector<Tile>> got(n);
    std::vector<uint32_t> group_stripes(G, 0);
    const uint32_t launched = G * ns;  // grid = 8 * launched
    sh.idle = per_xcd > launched ? per_xcd - launched : 0u;
    for (uint32_t xcd = 0; xcd < 8; xcd++) {
        for (uint32_t slot = 0; slot < launched; slot++) {
            const Local256BatchMap bm(sc, region, ns, G, n, xcd, slot);
            const StreamMap m(sc, region, ns, xcd, slot % ns);
            const int nt = m.ntile();
            CHECK(bm.ntile() == nt * bm.stripes(), "sc %u n %u slot %u: %d tiles, %d per stripe x %d stripes", sc, n, slot, bm.ntile(), nt, bm.stripes());
            const uint32_t j = slot / ns;
            CHECK(uint32_t(bm.stripes()) == (n - j + G - 1) / G, "sc %u n %u per_xcd %u group %u: %d stripes", sc, n, per_xcd, j, bm.stripes());
            if (xcd == 0 && slot % ns == 0) group_stripes[j] = uint32_t(bm.stripes());
            int64_t prev = -1;
            Local256BatchMap::Walk walk(bm);  // the compute waves' division-free walk
            for (int k = 0; k < bm.ntile(); k++) {
                const StreamTile t = bm.tile(k, slot, ns);
                const StreamTile u = walk.next(bm);
                CHECK(u.b0 == t.b0 && u.vend == t.vend && u.stripe == t.stripe, "sc %u n %u slot %u tile %d: the walk gives [%u, %u) of stripe %u, tile() [%u, %u) of stripe %u",
                      sc, n, slot, k, u.b0, u.vend, u.stripe, t.b0, t.vend, t.stripe);
                CHECK(t.stripe == bm.stripe(k), "sc %u n %u slot %u tile %d: stripe %u vs stripe(k) %u", sc, n, slot, k, t.stripe, bm.stripe(k));
                CHECK(t.stripe < n, "sc %u n %u slot %u tile %d: stripe %u", sc, n, slot, k, t.stripe);
                if (t.stripe >= n) continue;
                CHECK(t.stripe % G == j, "sc %u n %u slot %u: stripe %u in group %u of %u", sc, n, slot, t.stripe, j, G);
                // a stripe's tiles are tiles 0 .. nt - 1 of the one-stripe map in order, then the
                // next (larger) stripe
                const int r = k % nt;
                if (r == 0) CHECK(int64_t(t.stripe) > prev, "sc %u n %u slot %u tile %d: stripe %u after %lld", sc, n, slot, k, t.stripe, (long long)prev);
                else CHECK(int64_t(t.stripe) == prev, "sc %u n %u slot %u tile %d: stripe %u inside stripe %lld", sc, n, slot, k, t.stripe, (long long)prev);
                prev = t.stripe;
                const StreamTile o = m.tile(r, slot % ns, ns);
                CHECK(t.b0 == o.b0 && t.vend == o.vend, "sc %u n %u slot %u tile %d: [%u, %u), one stripe's tile %d is [%u, %u)", sc, n, slot, k, t.b0, t.vend, r, o.b0, o.vend);
                got[t.stripe].push_back({xcd, slot % ns, uint32_t(r), t.b0, t.vend});
            }
        }
        // nothing at or past the grid
        for (uint32_t slot = launched; slot < std::max(launched, per_xcd) + ns + 1; slot++)
            CHECK(Local256BatchMap(sc, region, ns, G, n, xcd, slot).ntile() == 0, "sc %u n %u per_xcd %u xcd %u: slot %u past the grid has tiles", sc, n, per_xcd, xcd, slot);
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
    return sh;
}

int main() {
    const uint32_t per_xcds[] = {1, 2, 13, 32, 38};
    const uint32_t stripes[] = {2, 3, 31, 32, 33, 70};
    std::set<uint32_t> scs;
    for (uint32_t sc = 512; sc <= 4096; sc += 8) scs.insert(sc);
    for (uint32_t sc : {8216u, 66176u, 66184u, 419432u}) scs.insert(sc);
    long cases = 0;
    int pinned = 0;
    for (uint32_t per_xcd : per_xcds)
        for (uint32_t n : stripes)
            for (uint32_t sc : scs) {
                const Shape s = check(sc, n, per_xcd);
                cases++;
                if (per_xcd != 32 || n != 70) continue;
                // the shapes of a 256-CU device (32 workgroups per XCD)
                auto is = [&](uint32_t ns, uint32_t g, uint32_t idle, uint32_t tail_b0, uint32_t tail_end) {
                    pinned++;
                    CHECK(s.ns == ns && s.groups == g && s.idle == idle, "sc %u: %u groups of %u, %u idle; expected %u of %u, %u idle",
                          sc, s.groups, s.ns, s.idle, g, ns, idle);
                    CHECK(s.tail_b0 == tail_b0 && s.tail_end == tail_end, "sc %u: the tile with the row's tail is [%u, %u), expected [%u, %u)",
                          sc, s.tail_b0, s.tail_end, tail_b0, tail_end);
                };
                if (sc == 512) {
                    is(1, 32, 0, 0, 0);
                    CHECK(s.full == 0 && s.partial == 8 && s.empty_xcds == 0, "sc 512: %u full, %u partial, %u empty XCDs", s.full, s.partial, s.empty_xcds);
                }
                if (sc == 520) {
                    is(1, 32, 0, 480, 520);
                    CHECK(s.full == 0 && s.partial == 6 && s.empty_xcds == 2, "sc 520: %u full, %u partial, %u empty XCDs", s.full, s.partial, s.empty_xcds);
                }
                if (sc == 2048) {
                    is(1, 32, 0, 0, 0);
                    CHECK(s.full == 8 && s.partial == 0, "sc 2048: %u full, %u partial", s.full, s.partial);
                }
                if (sc == 2056) {
                    is(2, 16, 0, 2048, 2056);
                    CHECK(s.full == 0 && s.partial == 16, "sc 2056: %u full, %u partial", s.full, s.partial);
                }
                if (sc == 2288) {
                    is(2, 16, 0, 0, 0);
                    CHECK(s.full == 0 && s.partial > 0, "sc 2288: %u full, %u partial", s.full, s.partial);
                }
                if (sc == 8216) {
                    is(5, 6, 2, 8160, 8216);
                    CHECK(s.full == 0 && s.partial > 0, "sc 8216: %u full, %u partial", s.full, s.partial);
                }
                if (sc == 66184) {
                    is(32, 1, 0, 65952, 66184);
                    CHECK(s.most == 2 && s.full > 0 && s.partial > 0 && s.full_first, "sc 66184: at most %u tiles per workgroup, %u full, %u partial, full first %d",
                          s.most, s.full, s.partial, int(s.full_first));
                }
            }
    CHECK(pinned == 7, "%d of the 7 pinned shapes were swept", pinned);
    if (failures) {
        printf("local256 batch map: %d failures\n", failures);
        return 1;
    }
    printf("local256 batch map ok: %ld cases\n", cases);
    return 0;
}
