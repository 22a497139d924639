// stream_tile_map.hpp -- how k_stream_encode cuts a sub-chunk row of sc bytes into tiles.
// Plain integer code (no HIP builtins), so that a host program can include it and walk the map
// (tests/test_stream_tile_map_cpu.py).
//
// XCD x owns bytes [x * region, min((x + 1) * region, sc)) of every row (region: a multiple of
// 32); its ns workgroups (slots) cover that region in R = ceil(len / (ns * 256)) rounds, the
// fewest a 256-byte tile allows.  Instead of R - 1 rounds of full tiles and a narrow last one
// (StreamMap), the R rounds get near-equal widths: a slot's share of the region is
// T = ceil(len / (ns * 16)) 16-byte pieces, the first T mod R rounds are T / R + 1 pieces wide
// and the others T / R, so every width is a multiple of 16, at most 256, and two widths differ
// by at most 16.  A pass of the kernel costs the same math whatever the tile's width; with equal
// widths every pass also brings the same memory time to hide that math under, where the narrow
// last tile of StreamMap had half a tile's memory time for a whole tile's math.
// Round r covers ns adjacent tiles of its width, slot after slot (adjacent workgroups stream
// adjacent runs of the same rows in the same pass).  Tiles are clipped to the region's end; as
// ns * 16 * (T - 1) < len, only tiles of the last round can be short or empty, and a slot's tiles
// are rounds 0 .. ntile() - 1.  16-byte granularity: the kernel's loads and stores are 16-byte
// pieces of a row, nothing in it needs 32.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLAY_TILE_MAP_HD __host__ __device__
#else
#define CLAY_TILE_MAP_HD
#endif

namespace clay {
namespace bs {

struct StreamTile {
    uint32_t b0, vend;  // positions [b0, b0 + 256) of every row, valid below vend
};

struct BalancedMap {
    uint32_t x0, x1, nrounds, q, rem, nt;
    CLAY_TILE_MAP_HD BalancedMap(uint32_t sc, uint32_t region, uint32_t ns, uint32_t xcd, uint32_t slot) {
        x0 = xcd * region;
        x1 = x0 + region < sc ? x0 + region : sc;
        nrounds = q = rem = nt = 0;
        if (x0 >= x1) return;
        const uint32_t len = x1 - x0;
        nrounds = (len + ns * 256u - 1u) / (ns * 256u);
        const uint32_t pieces = (len + ns * 16u - 1u) / (ns * 16u);  // T >= R
        q = pieces / nrounds;
        rem = pieces % nrounds;
        // rounds before the last are whole; the slot's last tile may be clipped away
        nt = start(nrounds - 1u, slot, ns) < x1 ? nrounds : nrounds - 1u;
    }
    // width of the tiles of round r
    CLAY_TILE_MAP_HD uint32_t width(uint32_t r) const { return (q + (r < rem ? 1u : 0u)) * 16u; }
    // first byte of the tile of round r and slot `slot` (not clipped)
    CLAY_TILE_MAP_HD uint32_t start(uint32_t r, uint32_t slot, uint32_t ns) const {
        const uint32_t before = r * q + (r < rem ? r : rem);  // pieces per slot in rounds < r
        return x0 + (ns * before + slot * (q + (r < rem ? 1u : 0u))) * 16u;
    }
    CLAY_TILE_MAP_HD int rounds() const { return int(nrounds); }
    CLAY_TILE_MAP_HD int ntile() const { return int(nt); }
    CLAY_TILE_MAP_HD StreamTile tile(int k, uint32_t slot, uint32_t ns) const {
        const uint32_t b0 = start(uint32_t(k), slot, ns), e = b0 + width(uint32_t(k));
        return {b0, e < x1 ? e : x1};
    }
};

}  // namespace bs
}  // namespace clay
