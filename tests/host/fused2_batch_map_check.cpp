// Host check of the tile map of the batched k_stream_fused2 (clay_amd/csrc/stream_tile_map.hpp:
// BatchMapOf<RoundRobinMap>, the fused decode's 64-byte round-robin cut of one stripe under the
// batch grouping of the other batches): walks the map for a sweep of sub-chunk sizes, stripe counts
// and workgroups per XCD and checks that
//   * every byte of a row of every stripe is owned by exactly one (workgroup, tile) -- a tile covers
//     the same byte range of every one of a chunk's 256 rows, so one row stands for all;
//   * every stripe keeps exactly the one-stripe cut, restated here from the kernel's rule: region =
//     ceil(sc / 8) rounded up to 64, nslots = min(per_xcd, region / 64), tile k of workgroup `slot`
//     of XCD x at x * region + (slot + k * nslots) * 64, clipped to the region's and the row's end;
//   * the map's division-free Walk (what both wave kinds of the kernel use) gives tile(k) for every k;
//   * a workgroup's stripes ascend, group j runs stripes j, j + G, ..., two groups' stripe counts
//     differ by at most one, and no slot at or past the grid of 8 x G x nslots workgroups has a tile;
//   * every tile is one the kernel can take (at most 64 bytes from a 64-byte boundary, a multiple of
//     8, ending at or after byte 16 of the row);
// and, for 32 workgroups per XCD, the facts about the four shapes that
// tests/test_gpu_decode_batch_fused2.py relies on.  Built and run by
// tests/test_fused2_batch_map_cpu.py; exits 0 and prints "fused2 batch map ok: <cases> cases" when
// every check holds, else prints the failures and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "stream_tile_map.hpp"

using clay::bs::batch_groups;
using clay::bs::BatchMapOf;
using clay::bs::round_robin_cut;
using clay::bs::RoundRobinMap;
using clay::bs::StreamTile;
using Fused2BatchMap = BatchMapOf<RoundRobinMap>;

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

struct Shape {
    uint32_t region, ns, groups, launched;  // per XCD: launched = groups * ns workgroups
    uint32_t lo, hi;                        // the fewest / most stripes of a group
    uint32_t most;                          // the most tiles of one stripe in a workgroup
    uint32_t two_tile_slots;                // sub-slots of XCD 0 with two tiles per stripe
    uint32_t xcd_tiles[8];                  // tiles of one stripe per XCD
    uint32_t last_width[8];                 // width of the XCD's last tile (0: none)
    uint32_t partial;                       // tiles narrower than 64 bytes in one stripe
};

static Shape check(uint32_t sc, uint32_t n, uint32_t per_xcd) {
    // the one-stripe cut, restated
    const uint32_t region = ((sc + 7u) / 8u + 63u) / 64u * 64u;
    const uint32_t ns = std::min(per_xcd, std::max(1u, region / 64u));
    CHECK(round_robin_cut(sc, per_xcd).region == region && round_robin_cut(sc, per_xcd).nslots == ns,
          "sc %u per_xcd %u: round_robin_cut gives region %u, %u slots; the kernel's rule %u, %u", sc, per_xcd,
          round_robin_cut(sc, per_xcd).region, round_robin_cut(sc, per_xcd).nslots, region, ns);
    const uint32_t G = batch_groups(per_xcd, ns, n);
    CHECK(G >= 1 && G <= n && (G * ns <= per_xcd || G == 1), "sc %u n %u per_xcd %u: %u groups of %u", sc, n, per_xcd, G, ns);
    Shape sh{};
    sh.region = region, sh.ns = ns, sh.groups = G, sh.launched = G * ns;
    // owner count of every byte of a row, per stripe
    std::vector<std::vector<uint8_t>> owners(n, std::vector<uint8_t>(sc, 0));
    std::vector<uint32_t> group_stripes(G, 0);
    for (uint32_t xcd = 0; xcd < 8; xcd++) {
        const uint32_t x0 = xcd * region, x1 = std::min(x0 + region, sc);
        for (uint32_t slot = 0; slot < sh.launched; slot++) {
            const Fused2BatchMap bm(sc, region, ns, G, n, xcd, slot);
            const uint32_t sub = slot % ns, j = slot / ns;
            // the one-stripe kernel's tiles of sub-slot `sub`
            std::vector<std::pair<uint32_t, uint32_t>> one;
            for (uint32_t b0 = x0 + sub * 64u; b0 < x1; b0 += ns * 64u) one.emplace_back(b0, std::min(b0 + 64u, x1));
            const uint32_t nt = uint32_t(one.size());
            sh.most = std::max(sh.most, nt);
            if (xcd == 0 && j == 0 && nt == 2) sh.two_tile_slots++;
            if (j == 0) {
                sh.xcd_tiles[xcd] += nt;
                for (const auto &t : one) {
                    if (t.second == x1) sh.last_width[xcd] = t.second - t.first;
                    sh.partial += t.second - t.first < 64u ? 1u : 0u;
                }
            }
            const uint32_t cnt = (n - j + G - 1) / G;
            CHECK(uint32_t(bm.stripes()) == cnt && uint32_t(bm.ntile()) == nt * cnt, "sc %u n %u per_xcd %u xcd %u slot %u: %d stripes, %d tiles; expected %u, %u",
                  sc, n, per_xcd, xcd, slot, bm.stripes(), bm.ntile(), cnt, nt * cnt);
            if (xcd == 0 && sub == 0) group_stripes[j] = cnt;
            Fused2BatchMap::Walk walk(bm);
            for (int k = 0; k < bm.ntile(); k++) {
                const StreamTile t = bm.tile(k, slot, ns), u = walk.next(bm);
                CHECK(u.b0 == t.b0 && u.vend == t.vend && u.stripe == t.stripe, "sc %u n %u slot %u tile %d: the walk gives [%u, %u) of stripe %u, tile() [%u, %u) of stripe %u",
                      sc, n, slot, k, u.b0, u.vend, u.stripe, t.b0, t.vend, t.stripe);
                // stripes j, j + G, ..., each with the one-stripe tiles in order
                const uint32_t i = uint32_t(k) / nt, r = uint32_t(k) % nt;
                CHECK(t.stripe == j + i * G && t.stripe < n, "sc %u n %u slot %u tile %d: stripe %u, expected %u", sc, n, slot, k, t.stripe, j + i * G);
                CHECK(t.b0 == one[r].first && t.vend == one[r].second, "sc %u n %u slot %u tile %d: [%u, %u), the one-stripe tile %u is [%u, %u)",
                      sc, n, slot, k, t.b0, t.vend, r, one[r].first, one[r].second);
                // what the kernel asks of a tile
                CHECK(t.b0 < t.vend && t.vend <= sc && t.vend - t.b0 <= 64u && t.b0 % 64u == 0 && (t.vend - t.b0) % 8u == 0 && t.vend >= 16u,
                      "sc %u per_xcd %u xcd %u slot %u tile %d: [%u, %u)", sc, per_xcd, xcd, slot, k, t.b0, t.vend);
                if (t.stripe >= n || t.vend > sc) continue;
                for (uint32_t b = t.b0; b < t.vend; b++) owners[t.stripe][b]++;
            }
        }
        // nothing at or past the grid
        for (uint32_t slot = sh.launched; slot < std::max(sh.launched, per_xcd) + ns + 1; slot++)
            CHECK(Fused2BatchMap(sc, region, ns, G, n, xcd, slot).ntile() == 0, "sc %u n %u per_xcd %u xcd %u: slot %u past the grid has tiles", sc, n, per_xcd, xcd, slot);
    }
    sh.lo = *std::min_element(group_stripes.begin(), group_stripes.end());
    sh.hi = *std::max_element(group_stripes.begin(), group_stripes.end());
    CHECK(sh.hi - sh.lo <= 1 && sh.lo >= 1, "sc %u n %u per_xcd %u: groups run %u .. %u stripes", sc, n, per_xcd, sh.lo, sh.hi);
    for (uint32_t s = 0; s < n; s++)
        for (uint32_t b = 0; b < sc; b++)
            if (owners[s][b] != 1) {
                CHECK(owners[s][b] == 1, "sc %u n %u per_xcd %u stripe %u byte %u: %u owners", sc, n, per_xcd, s, b, owners[s][b]);
                break;
            }
    return sh;
}

int main() {
    const uint32_t per_xcds[] = {1, 2, 13, 32, 38};
    const uint32_t stripes[] = {2, 3, 17, 34, 70};
    std::set<uint32_t> scs;
    for (uint32_t sc = 512; sc <= 4096; sc += 8) scs.insert(sc);
    for (uint32_t sc : {16904u, 66184u}) scs.insert(sc);
    long cases = 0;
    for (uint32_t per_xcd : per_xcds)
        for (uint32_t n : stripes)
            for (uint32_t sc : scs) {
                check(sc, n, per_xcd);
                cases++;
            }
    // the shapes of the GPU tests on a 256-CU device (32 workgroups per XCD)
    auto pin = [&](uint32_t sc, uint32_t n, uint32_t region, uint32_t ns, uint32_t G, uint32_t lo, uint32_t hi) {
        const Shape s = check(sc, n, 32);
        cases++;
        CHECK(s.region == region && s.ns == ns && s.groups == G && s.launched == G * ns, "%u x %u: region %u, %u slots, %u groups (8 x %u workgroups); expected %u, %u, %u",
              sc, n, s.region, s.ns, s.groups, s.launched, region, ns, G);
        CHECK(s.lo == lo && s.hi == hi, "%u x %u: groups run %u .. %u stripes, expected %u .. %u", sc, n, s.lo, s.hi, lo, hi);
        return s;
    };
    {
        const Shape s = pin(512, 2, 64, 1, 2, 1, 1);
        CHECK(s.partial == 0 && s.most == 1, "512 x 2: %u partial tiles, at most %u per workgroup", s.partial, s.most);
        for (int x = 0; x < 8; x++) CHECK(s.xcd_tiles[x] == 1 && s.last_width[x] == 64, "512 x 2 XCD %d: %u tiles, last %u wide", x, s.xcd_tiles[x], s.last_width[x]);
    }
    {
        const Shape s = pin(520, 34, 128, 2, 16, 2, 3);
        for (int x = 0; x < 4; x++) CHECK(s.xcd_tiles[x] == 2 && s.last_width[x] == 64, "520 x 34 XCD %d: %u tiles, last %u wide", x, s.xcd_tiles[x], s.last_width[x]);
        CHECK(s.xcd_tiles[4] == 1 && s.last_width[4] == 8 && s.partial == 1, "520 x 34 XCD 4: %u tiles, last %u wide, %u partial", s.xcd_tiles[4], s.last_width[4], s.partial);
        for (int x = 5; x < 8; x++) CHECK(s.xcd_tiles[x] == 0, "520 x 34 XCD %d: %u tiles", x, s.xcd_tiles[x]);
    }
    {
        const Shape s = pin(2056, 17, 320, 5, 6, 2, 3);  // 3, 3, 3, 3, 3, 2 stripes
        CHECK(s.xcd_tiles[6] == 3 && s.last_width[6] == 8 && s.partial == 1, "2056 x 17 XCD 6: %u tiles, last %u wide, %u partial", s.xcd_tiles[6], s.last_width[6], s.partial);
        CHECK(s.xcd_tiles[7] == 0 && s.xcd_tiles[0] == 5 && s.most == 1, "2056 x 17: XCD 7 %u tiles, XCD 0 %u, at most %u per workgroup", s.xcd_tiles[7], s.xcd_tiles[0], s.most);
    }
    {
        const Shape s = pin(16904, 3, 2176, 32, 1, 3, 3);
        CHECK(s.xcd_tiles[0] == 34 && s.two_tile_slots == 2 && s.most == 2, "16904 x 3: %u tiles in XCD 0, %u slots with two tiles, at most %u per workgroup",
              s.xcd_tiles[0], s.two_tile_slots, s.most);
    }
    if (failures) {
        printf("fused2 batch map: %d failures\n", failures);
        return 1;
    }
    printf("fused2 batch map ok: %ld cases\n", cases);
    return 0;
}
