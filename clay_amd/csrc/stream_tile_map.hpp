// stream_tile_map.hpp -- how the streaming kernels cut a sub-chunk row of sc bytes into tiles:
// BalancedMap (k_stream_encode), StreamMap (k_stream_local256 and the other streaming kernels),
// RoundRobinMap (the 64-byte tiles of k_stream_fused2's batch) and the batch grouping over any of
// them (BatchMapOf).
// Plain integer code (no HIP builtins), so that a host program can include it and walk the maps
// (tests/test_stream_tile_map_cpu.py, tests/test_local256_batch_map_cpu.py,
// tests/test_fused2_batch_map_cpu.py).
//
// BalancedMap.
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
    uint32_t stripe;    // BatchMap: the stripe the tile belongs to (the one-stripe maps leave it 0)
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
        return {b0, e < x1 ? e : x1, 0u};
    }
};

// StreamMap (k_stream_local256, the repair and 3-parity encode kernels, the encode probe's old-map
// builds): XCD x owns bytes [x * region, min((x + 1) * region, sc)); full W-byte tiles round robin
// over the XCD's ns workgroups, the remainder one partial tile per workgroup (its last), so every
// workgroup of an XCD streams the same number of bytes to within 32.
struct StreamMap {
    uint32_t x0, x1, nfull, p0, p1, w;
    CLAY_TILE_MAP_HD StreamMap(uint32_t sc, uint32_t region, uint32_t ns, uint32_t xcd, uint32_t slot, uint32_t W = 256u) {
        w = W;
        x0 = xcd * region;
        x1 = x0 + region < sc ? x0 + region : sc;
        nfull = p0 = p1 = 0;
        if (x0 >= x1) return;
        const uint32_t len = x1 - x0, round = ns * W;
        nfull = len / round;
        const uint32_t left = len - nfull * round;
        const uint32_t wp = ((left + ns - 1) / ns + 31u) & ~31u;
        const uint32_t q0 = x0 + nfull * round + slot * wp;
        if (left && q0 < x1) {
            p0 = q0;
            p1 = q0 + wp < x1 ? q0 + wp : x1;
        }
    }
    CLAY_TILE_MAP_HD int ntile() const { return int(nfull) + (p0 < p1 ? 1 : 0); }
    CLAY_TILE_MAP_HD StreamTile tile(int k, uint32_t slot, uint32_t ns) const {
        if (uint32_t(k) < nfull) {
            const uint32_t b0 = x0 + (uint32_t(k) * ns + slot) * w;
            return {b0, b0 + w, 0u};
        }
        return {p0, p1, 0u};
    }
};

// RoundRobinMap (k_stream_fused2 BATCH; the cut of StreamDec::Map, stream_decode.hpp, which the
// one-stripe decode kernels keep using): XCD x owns bytes [x * region, min((x + 1) * region, sc))
// (region: a multiple of 64); its 64-byte tiles go round robin over the XCD's ns workgroups, tile
// k of workgroup `slot` at x0 + (slot + k * ns) * 64, the region's last tile clipped to its end
// (sc a multiple of 8: a last tile of 8, 16, ... 56 bytes).
struct RoundRobinMap {
    static constexpr uint32_t W = 64u;
    uint32_t x0, x1, n;
    CLAY_TILE_MAP_HD RoundRobinMap(uint32_t sc, uint32_t region, uint32_t ns, uint32_t xcd, uint32_t slot) {
        x0 = xcd * region;
        x1 = x0 + region < sc ? x0 + region : sc;
        n = 0;
        if (x0 < x1) {
            const uint32_t nt = (x1 - x0 + W - 1u) / W;
            n = nt > slot ? (nt - slot + ns - 1u) / ns : 0u;
        }
    }
    CLAY_TILE_MAP_HD int ntile() const { return int(n); }
    CLAY_TILE_MAP_HD StreamTile tile(int k, uint32_t slot, uint32_t ns) const {
        const uint32_t b0 = x0 + (slot + uint32_t(k) * ns) * W;
        return {b0, b0 + W < x1 ? b0 + W : x1, 0u};
    }
};

// ... and the host's cut for it: an XCD's region is sc / 8 rounded up to 64 bytes, with one
// workgroup per 64-byte tile of a region, at least one and at most per_xcd.
CLAY_TILE_MAP_HD inline uint32_t round_robin_region(uint64_t sc) { return uint32_t(((sc + 7) / 8 + 63) / 64 * 64); }

// A batch of n_stripes stripes of one sub-chunk size in one launch (k_stream_encode BATCH with
// One = BalancedMap, k_stream_local256 BATCH with One = StreamMap, k_stream_fused2 BATCH with
// One = RoundRobinMap: BatchMapOf<One>).
// Every stripe keeps exactly the one-stripe cut: its region, ns = nsS workgroups per XCD and
// One(sc, region, nsS, xcd, sub); the encode's words below (BalancedMap, rounds) read the same for
// StreamMap and its tiles.  The per_xcd workgroups of an XCD form
// G = min(max(1, per_xcd / nsS), n_stripes) groups of nsS (batch_groups); workgroup `slot` is
// sub-slot slot % nsS of group j = slot / nsS, and slots from G * nsS on are not launched (grid =
// 8 * G * nsS).  Group j runs the stripes j, j + G, j + 2G, ... one after the other, each through
// the same BalancedMap: the workgroup's tile k is round k % nt of stripe j + (k / nt) * G, where
// nt = BalancedMap::ntile() is the same for every stripe because sc is.  So two groups' stripe
// counts differ by at most one, a workgroup's stripes ascend, and its tile sequence is the
// concatenation of one-stripe sequences (the kernel's flat step counter runs over it unchanged).
CLAY_TILE_MAP_HD inline uint32_t batch_groups(uint32_t per_xcd, uint32_t ns, uint32_t n_stripes) {
    const uint32_t fit = per_xcd / ns > 1u ? per_xcd / ns : 1u;
    return fit < n_stripes ? fit : n_stripes;
}

// The host's cut of a row of sc bytes over the 8 XCDs, for every kernel that streams XCD regions:
// an XCD's region is sc / 8 rounded up to 32 bytes ...
CLAY_TILE_MAP_HD inline uint32_t xcd_region(uint64_t sc) { return uint32_t(((sc + 7) / 8 + 31) / 32 * 32); }

// ... and it gets one workgroup per tile of the region, at least one and at most per_xcd (one per
// CU of the XCD).
struct StreamCut {
    uint32_t region, nslots;
};
CLAY_TILE_MAP_HD inline StreamCut stream_cut(uint64_t sc, uint32_t per_xcd, uint32_t tile = 256u) {
    const uint32_t region = xcd_region(sc);
    const uint32_t tiles = (region + tile - 1u) / tile > 1u ? (region + tile - 1u) / tile : 1u;
    return {region, per_xcd < tiles ? per_xcd : tiles};
}

CLAY_TILE_MAP_HD inline StreamCut round_robin_cut(uint64_t sc, uint32_t per_xcd) {
    const uint32_t region = round_robin_region(sc);
    const uint32_t tiles = region / 64u > 1u ? region / 64u : 1u;
    return {region, per_xcd < tiles ? per_xcd : tiles};
}

template <class One>
struct BatchMapOf {
    One one;  // the cut of every stripe, for this workgroup's sub-slot
    uint32_t ns, sub, first, groups, count, nt;  // nt: one.ntile(), the tiles of one stripe
    CLAY_TILE_MAP_HD BatchMapOf(uint32_t sc, uint32_t region, uint32_t ns_, uint32_t groups_, uint32_t n_stripes, uint32_t xcd,
                                uint32_t slot)
        : one(sc, region, ns_, xcd, slot % ns_), ns(ns_), sub(slot % ns_), first(slot / ns_), groups(groups_) {
        // stripes first, first + G, ... below n_stripes; none for a slot at or past G * ns
        count = first < groups && first < n_stripes ? (n_stripes - first + groups - 1u) / groups : 0u;
        nt = uint32_t(one.ntile());
    }
    CLAY_TILE_MAP_HD int stripes() const { return int(count); }
    CLAY_TILE_MAP_HD int ntile() const { return int(nt * count); }
    // stripe of the workgroup's tile k
    CLAY_TILE_MAP_HD uint32_t stripe(int k) const { return first + uint32_t(k) / nt * groups; }
    // (slot and ns of the one-stripe maps' signature are not used: the map holds its own)
    CLAY_TILE_MAP_HD StreamTile tile(int k, uint32_t, uint32_t) const {
        const uint32_t i = uint32_t(k) / nt;
        StreamTile t = one.tile(int(uint32_t(k) - i * nt), sub, ns);
        t.stripe = first + i * groups;
        return t;
    }
    // The same sequence, tile after tile, without the division by nt: next() returns tile(k) for
    // k = 0, 1, 2, ... (k_stream_local256's compute waves, which have no registers to spare for the
    // division's temporaries where they need the tile; tests/host/local256_batch_map_check.cpp
    // walks both and compares).  Not to be called more than ntile() times.
    struct Walk {
        uint32_t r, stripe;
        CLAY_TILE_MAP_HD explicit Walk(const BatchMapOf &m) : r(0u), stripe(m.first) {}
        CLAY_TILE_MAP_HD __attribute__((always_inline)) StreamTile next(const BatchMapOf &m) {
            StreamTile t = m.one.tile(int(r), m.sub, m.ns);
            t.stripe = stripe;
            if (++r == m.nt) {
                r = 0u;
                stripe += m.groups;
            }
            return t;
        }
    };
};
using BatchMap = BatchMapOf<BalancedMap>;  // k_stream_encode BATCH

}  // namespace bs
}  // namespace clay
