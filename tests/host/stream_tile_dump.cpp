// Prints the tiles BalancedMap (clay_amd/csrc/stream_tile_map.hpp, the header k_stream_encode and
// its compare-ending variant use) gives every workgroup, for tests/test_scrub_stream_shapes_cpu.py.
// Arguments: triples `sc region ns` (sub-chunk bytes, XCD region bytes, workgroups per XCD).
// Output: one line `sc xcd slot round b0 vend` per tile.
#include <cstdio>
#include <cstdlib>

#include "stream_tile_map.hpp"

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 1) % 3 != 0) {
        std::fprintf(stderr, "usage: %s sc region ns [sc region ns ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i + 2 < argc; i += 3) {
        const uint32_t sc = uint32_t(std::strtoul(argv[i], nullptr, 10));
        const uint32_t region = uint32_t(std::strtoul(argv[i + 1], nullptr, 10));
        const uint32_t ns = uint32_t(std::strtoul(argv[i + 2], nullptr, 10));
        for (uint32_t xcd = 0; xcd < 8; xcd++)
            for (uint32_t slot = 0; slot < ns; slot++) {
                const clay::bs::BalancedMap tm(sc, region, ns, xcd, slot);
                for (int k = 0; k < tm.ntile(); k++) {
                    const clay::bs::StreamTile t = tm.tile(k, slot, ns);
                    std::printf("%u %u %u %d %u %u\n", sc, xcd, slot, k, t.b0, t.vend);
                }
            }
    }
    return 0;
}
