// Host check of the XCD cut (clay_amd/csrc/stream_tile_map.hpp: xcd_region, stream_cut,
// batch_groups), the launch arithmetic of every kernel that streams XCD regions.  Prints one line
//   sc per_xcd tile region nslots g1 g2 g3 g33 g70
// per (sub-chunk size, workgroups per XCD, tile width), g<n> = batch_groups for n stripes;
// tests/test_stream_cut_cpu.py compares every line with tests/stream_cut.py, the tests' own
// restatement.  Checks the cut's bounds and the pinned shapes of a 256-CU device itself: exits 0 and
// ends with "stream cut ok: <cases> cases", else prints the failures and exits 1.  Also run under
// ASan + UBSan by scripts/host_checks_sanitized.sh.
#include <cstdint>
#include <cstdio>
#include <set>

#include "stream_tile_map.hpp"

using clay::bs::batch_groups;
using clay::bs::stream_cut;
using clay::bs::StreamCut;
using clay::bs::xcd_region;

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

int main() {
    const uint32_t per_xcds[] = {1, 2, 13, 32, 38};
    const uint32_t tiles[] = {256, 512};
    const uint32_t stripes[] = {1, 2, 3, 33, 70};
    std::set<uint32_t> scs;
    for (uint32_t sc = 16; sc <= 4096; sc += 8) scs.insert(sc);
    for (uint32_t sc : {6560u, 8200u, 8216u, 26216u, 66176u, 66184u, 262152u, 419432u}) scs.insert(sc);
    long cases = 0;
    for (uint32_t sc : scs)
        for (uint32_t per_xcd : per_xcds)
            for (uint32_t tile : tiles) {
                const StreamCut c = stream_cut(sc, per_xcd, tile);
                printf("%u %u %u %u %u", sc, per_xcd, tile, c.region, c.nslots);
                CHECK(c.region == xcd_region(sc), "sc %u: region %u, xcd_region %u", sc, c.region, xcd_region(sc));
                // 8 regions of whole 32-byte units cover the row, with less than 32 bytes to spare each
                CHECK(c.region % 32 == 0 && uint64_t(c.region) * 8 >= sc && uint64_t(c.region - 32) * 8 < sc, "sc %u: region %u", sc, c.region);
                // a workgroup per tile of the region, from 1 to per_xcd
                CHECK(c.nslots >= 1 && c.nslots <= per_xcd, "sc %u per_xcd %u: %u slots", sc, per_xcd, c.nslots);
                CHECK(c.nslots == per_xcd || (uint64_t(c.nslots) * tile >= c.region && uint64_t(c.nslots - 1) * tile < c.region),
                      "sc %u per_xcd %u tile %u: %u slots for a region of %u", sc, per_xcd, tile, c.nslots, c.region);
                for (uint32_t n : stripes) {
                    const uint32_t g = batch_groups(per_xcd, c.nslots, n);
                    printf(" %u", g);
                    CHECK(g >= 1 && g <= n && (g * c.nslots <= per_xcd || g == 1), "sc %u n %u per_xcd %u: %u groups of %u", sc, n, per_xcd, g, c.nslots);
                }
                printf("\n");
                cases++;
                if (per_xcd != 32 || tile != 256) continue;
                // the shapes of a 256-CU device (32 workgroups per XCD)
                auto is = [&](uint32_t region, uint32_t nslots) {
                    CHECK(c.region == region && c.nslots == nslots, "sc %u: (%u, %u), expected (%u, %u)", sc, c.region, c.nslots, region, nslots);
                };
                if (sc == 16) is(32, 1);
                if (sc == 1064) is(160, 1);
                if (sc == 2048) is(256, 1);
                if (sc == 2288) is(288, 2);
                if (sc == 66176) is(8288, 32);
            }
    if (failures) {
        printf("stream cut: %d failures\n", failures);
        return 1;
    }
    printf("stream cut ok: %ld cases\n", cases);
    return 0;
}
