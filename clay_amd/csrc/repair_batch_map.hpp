// repair_batch_map.hpp -- how the batch form of k_bs_repair (repair_kernel.hpp) spreads many
// stripes over its workgroups.  Plain integer code (no HIP builtins), so that a host program can
// include it and walk the map (tests/test_repair_batch_map_cpu.py).
//
// A column is 32 byte positions of one stripe's sub-chunk rows: a stripe of sub-chunk size sc has
// cps = ceil(sc / 32) columns (the last one short when sc % 32 != 0), n_stripes stripes have
// ncols = n_stripes * cps.  Tile t (one workgroup pass) owns columns [t * parts, (t + 1) * parts),
// whatever stripes they belong to: with sc = 32 a (4,2,5) workgroup (parts = 64) repairs 64
// stripes, where the single-stripe kernel keeps 63 of its 64 lanes per plane layer idle.  The
// lane (plane layer j, part) takes column t * parts + part; columns past ncols touch no byte.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLAY_REPAIR_MAP_HD __host__ __device__ inline
#else
#define CLAY_REPAIR_MAP_HD inline
#endif

namespace clay {
namespace bs {

struct RepBatchCol {
    uint32_t stripe;  // the column's stripe
    uint32_t pos;     // its first byte position in the sub-chunk
    uint32_t nv;      // valid bytes, 0..32 (0: past the last stripe)
};

// columns per stripe / in all (64-bit: the caller checks that ncols fits 32 bits)
CLAY_REPAIR_MAP_HD uint64_t rep_batch_cps(uint64_t sc) { return (sc + 31u) / 32u; }
CLAY_REPAIR_MAP_HD uint64_t rep_batch_ncols(uint64_t sc, uint64_t n_stripes) { return rep_batch_cps(sc) * n_stripes; }
CLAY_REPAIR_MAP_HD uint64_t rep_batch_ntiles(uint64_t ncols, uint32_t parts) { return (ncols + parts - 1u) / parts; }

// column col of the batch (cps >= 1)
CLAY_REPAIR_MAP_HD RepBatchCol rep_batch_col(uint32_t col, uint32_t ncols, uint32_t cps, uint64_t sc) {
    RepBatchCol c;
    c.stripe = col / cps;
    c.pos = 32u * (col - c.stripe * cps);
    const uint64_t left = sc - c.pos;  // pos < sc: col % cps < cps = ceil(sc / 32)
    c.nv = col >= ncols ? 0u : left > 32u ? 32u : uint32_t(left);
    return c;
}

// every lane of tile t holds 32 valid bytes: whole columns only, none past the last stripe
CLAY_REPAIR_MAP_HD bool rep_batch_tile_full(uint32_t tile, uint32_t parts, uint32_t ncols, uint64_t sc) {
    return (sc & 31u) == 0 && (uint64_t(tile) + 1u) * parts <= ncols;
}

}  // namespace bs
}  // namespace clay
