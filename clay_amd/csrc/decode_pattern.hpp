// decode_pattern.hpp -- which streaming decode kernel an erasure pattern of a q = 4, t = 4 code
// with k = 9 / 10 runs on, and every kernel argument the pattern alone decides.  Plain integer code
// (no HIP, no code state, no GF arithmetic), so that a host program can include it and print the
// choice for every pattern (tests/host/decode_pattern_check.cpp; tests/test_decode_pattern_cpu.py
// compares it with the tests' own restatement, tests/decode_pattern.py).  The engine adds what
// needs the code and the device: the RS rows' tables, the pointers, the XCD cut and the launch.
//
// Nodes are internal ones, i = 4 y + x (section y, digit x); masks carry bit i for node i.
#pragma once

#include <algorithm>
#include <cstdint>

#include "decode_args.hpp"

namespace clay {

// Executor selection (clay_set_exec_mode; 4 and 7 are retired)
enum : int { kExecAuto = 0, kExecGrouped = 1, kExecTile = 2, kExecStream = 3, kExecStreamLocal = 5,
              kExecStreamFused2 = 6 };

namespace bs {

constexpr int kDecK = 12;  // RS data rows of both codes (k + shortened nodes): nodes [KD, 12) are shortened

// Erasures per y-section (`erased`: bit i = internal node i is erased)
struct SectionErasures {
    int per[4] = {0, 0, 0, 0};
    int nsec = 0;  // sections with an erasure
    int most = 0;  // the first section with the most erasures
};
inline SectionErasures section_erasures(uint32_t erased) {
    SectionErasures se;
    for (int i = 0; i < 16; i++) se.per[i / 4] += int((erased >> i) & 1u);
    for (int y = 0; y < 4; y++) {
        if (se.per[y] > se.per[se.most]) se.most = y;
        se.nsec += se.per[y] ? 1 : 0;
    }
    return se;
}

// What the streaming decodes share of a pattern.  `alive`: the nodes with an input pointer; R: the
// staging ring (10 unless a measurement sets CLAY_DECODE_RING); per_sec_max: the most erasures one
// y-section may hold.  Fills a (from DecArgs{}): g2 = -1, ne, rix, emask, used, alive, load_node,
// sec_off, nt, scase, ring; K: the four nodes outside the RS rows used, in order (the columns of
// H_K); *ring_ok: the R - 1 node buffers hold the loads the local kernel keeps in flight.  false:
// no streaming decode takes the pattern.
inline bool dec_pattern(int KD, uint32_t erased, uint32_t alive, uint32_t R, int per_sec_max, DecArgs &a, int (&K)[4],
                        bool *ring_ok) {
    a = DecArgs{};
    a.g2 = -1;
    *ring_ok = false;
    erased &= 0xFFFFu;
    const int ne = __builtin_popcount(erased);
    if (ne == 0 || ne > 4) return false;
    // every real node (not shortened) is erased or alive: the kernels read a node without data as
    // zeros, which only a shortened one is (the library's decode validation admits nothing else)
    const uint32_t real = 0xFFFFu & ~(((1u << kDecK) - 1u) & ~((1u << KD) - 1u));
    if (((alive | erased) & real) != real) return false;
    const SectionErasures se = section_erasures(erased);
    if (se.per[se.most] > per_sec_max) return false;
    // RS rows used: the first 12 present shards (reconstruct, decode.rs:374); K = the rest
    uint32_t used = 0;
    int nused = 0, nk = 0;
    for (int i = 0; i < 16; i++) {
        if (!((erased >> i) & 1u) && nused < kDecK) {
            used |= 1u << i;
            nused++;
        } else if (nk < 4) {
            K[nk++] = i;
        } else {
            return false;
        }
    }
    if (nused != kDecK || nk != 4) return false;
    a.ne = uint32_t(ne);
    for (int i = 0, r = 0; i < 16; i++) {
        a.rix[i] = (erased >> i) & 1u ? r++ : -1;
        if ((erased >> i) & 1u) a.emask[i / 4] |= 1u << (i % 4);
    }
    a.used = used;
    uint32_t n[4] = {0, 0, 0, 0}, nt = 0;
    for (int y = 0; y < 4; y++) {
        a.sec_off[y] = nt;
        for (int x = 0; x < 4; x++) {
            const int i = 4 * y + x;
            if ((alive >> i) & 1u) {
                a.alive |= 1u << i;
                a.load_node[nt++] = uint32_t(i);
                n[y]++;
            }
        }
    }
    a.sec_off[4] = nt;
    a.nt = nt;
    // k_stream_fused2's compile-time phase-A copies: section y with at most one erased node x,
    // every other node used and every node alive but that one and the shortened ones (i in [KD, 12))
    for (int y = 0; y < 4; y++) {
        uint32_t shortn = 0;
        for (int x = 0; x < 4; x++)
            if (4 * y + x >= KD && 4 * y + x < kDecK) shortn |= 1u << x;
        const uint32_t em = a.emask[y], un = (used >> (4 * y)) & 15u, al = (a.alive >> (4 * y)) & 15u;
        const bool ok1 = __builtin_popcount(em) <= 1 && un == (~em & 15u) && al == (~em & ~shortn & 15u);
        a.scase[y] = ok1 ? (em ? __builtin_ctz(em) : 4) : -1;
        // k_stream_local256 (one erased row): no erasure, every node alive and only node 0 / nodes
        // 0-1 used (the ignored nodes of one erasure: the last present ones); the fused decode
        // takes the run-time copy for these
        if (!ok1 && em == 0 && al == (~shortn & 15u) && (un == 1u || un == 3u)) a.scase[y] = un == 1u ? 5 : 6;
    }
    if (nt == 0) return false;
    // the local kernel streams through R - 1 buffers (the last holds tables): a step's
    // loads are issued during the step before it, across tiles too (section 3 -> section 0);
    // S/C region (4 buffers) + the phase-B table buffer: R >= 5
    *ring_ok = R >= 5;
    for (int y = 0; y < 4; y++)
        if (n[y] > R - 1 || n[y] + n[(y + 1) % 4] > R - 1) *ring_ok = false;
    a.ring = R;
    return true;
}

// Local decode (stream_local.hpp): erasures in one y-section G (any number) plus at most one
// erasure in one other section g2 -- every iscore dependency inside a wave, one launch, no
// workspace.  G = the section with the most erasures; section g2's digit goes to bits 0-1 of
// the lane column.  One erasure in section G plus at most one in g2, or two in G and none
// elsewhere: the 256-byte-run kernel (stream_local256.hpp), which also takes sub-chunks that are
// not a multiple of 8 (local_w64, a measurement knob: the 64-byte kernel for these too).
struct LocalShape {
    bool ok = false, w256 = false;
    int G = 0, g2 = -1;
};
inline LocalShape local_shape(uint32_t erased, bool local_w64) {
    LocalShape s;
    const SectionErasures se = section_erasures(erased & 0xFFFFu);
    if (se.nsec == 0 || se.nsec > 2) return s;
    s.G = se.most;
    for (int y = 0; y < 4; y++)
        if (y != s.G && se.per[y]) {
            if (se.per[y] > 1) return s;  // two sections with several erasures: rounds needed
            s.g2 = y;
        }
    s.w256 = (se.per[s.G] == 1 || (se.per[s.G] == 2 && s.g2 < 0)) && !local_w64;
    s.ok = true;
    return s;
}
// the local kernels' column digits (a.csh, a.g2, a.x2; after dec_pattern): section g2 (if any) at
// bits 0-1, the others above in section order
inline void local_columns(const LocalShape &s, DecArgs &a) {
    uint32_t sh = 4;
    for (int y = 0; y < 4; y++)
        if (y != s.G) a.csh[y] = y == s.g2 ? 0u : (sh -= 2) + 2;
    a.g2 = s.g2;
    if (s.g2 >= 0) a.x2 = uint32_t(__builtin_ctz(a.emask[s.g2]));
}

// Rounds of k_stream_fused2 (stream_fused2.hpp): per section Y with an erasure and iscore level L,
// the targets are the layers z with z_Y in E_Y and exactly L - 1 other sections y with z_y in E_y,
// P(Y, L) = ceil(targets x 8 / 64) passes of 64 lanes x (8-byte piece).  The four loader waves share
// them: each section with an erasure gets at least one wave, the spare waves go where they cut
// the sum over levels of the busiest wave's passes most, and a section's nw waves take every
// nw-th pass.  f2_plan packs, per loader wave li, byte li of a.lwave: bits 0-1 its section, 2-3 its
// part, 4-5 nw - 1, bit 6 set (no section: 0); false when a wave would hold more than the kernel's
// kF2Iters (TWO) / kF2Iters1 passes of some level.
inline uint32_t f2_targets(const uint32_t (&emask)[4], int Y, int L) {
    uint32_t n = 0;
    for (uint32_t z = 0; z < 256; z++) {
        int red = 0;
        bool ty = false;
        for (int y = 0; y < 4; y++) {
            const uint32_t d = (z >> (2 * (3 - y))) & 3u;
            const bool in = (emask[y] >> d) & 1u;
            red += in ? 1 : 0;
            if (y == Y) ty = in;
        }
        n += (ty && red == L) ? 1u : 0u;
    }
    return n;
}
inline bool f2_plan(const uint32_t (&emask)[4], bool two, uint32_t *lwave) {
    uint32_t P[4][4] = {}, nw[4] = {};
    int nact = 0;
    for (int Y = 0; Y < 4; Y++) {
        if (!emask[Y]) continue;
        nact++;
        nw[Y] = 1;
        for (int L = 1; L <= 4; L++) P[Y][L - 1] = (f2_targets(emask, Y, L) * 8u + 63u) / 64u;
    }
    const int *cap = two ? kF2Iters : kF2Iters1;
    // the spare waves: the split (every active section >= 1 wave, 4 in all) with the smallest sum
    // over levels of the busiest wave's passes (each level's round is one step) among those within
    // the kernel's item registers, first in lexicographic order of (nw[0], .., nw[3]) among equals
    if (nact > 0 && nact < 4) {
        uint32_t best[4] = {0, 0, 0, 0}, bcost = ~0u;
        for (uint32_t n0 = 0; n0 <= 4; n0++)
            for (uint32_t n1 = 0; n1 <= 4; n1++)
                for (uint32_t n2 = 0; n2 <= 4; n2++)
                    for (uint32_t n3 = 0; n3 <= 4; n3++) {
                        const uint32_t n[4] = {n0, n1, n2, n3};
                        if (n0 + n1 + n2 + n3 != 4) continue;
                        bool ok = true;
                        for (int Y = 0; Y < 4; Y++) ok = ok && ((n[Y] > 0) == (nw[Y] > 0));
                        if (!ok) continue;
                        uint32_t cost = 0;
                        for (int L = 0; L < 4; L++) {
                            uint32_t mx = 0;
                            for (int Y = 0; Y < 4; Y++)
                                if (n[Y]) mx = std::max(mx, (P[Y][L] + n[Y] - 1u) / n[Y]);
                            if (mx > uint32_t(cap[L])) ok = false;  // over the kernel's item registers
                            cost += mx;
                        }
                        if (!ok) continue;
                        if (cost < bcost) {
                            bcost = cost;
                            for (int Y = 0; Y < 4; Y++) best[Y] = n[Y];
                        }
                    }
        if (bcost == ~0u) return false;  // no split within the item registers
        for (int Y = 0; Y < 4; Y++) nw[Y] = best[Y];
    }
    uint32_t pack = 0;
    int li = 0;
    for (int Y = 0; Y < 4; Y++) {
        for (uint32_t part = 0; part < nw[Y]; part++, li++)
            pack |= (uint32_t(Y) | part << 2 | (nw[Y] - 1u) << 4 | 64u) << (8 * li);
        for (int L = 0; L < 4 && nw[Y]; L++)
            if ((P[Y][L] + nw[Y] - 1u) / nw[Y] > uint32_t(cap[L])) return false;
        if (two && P[Y][3]) return false;  // the TWO kernel inverts the pairs during the level-4 round's slot
    }
    *lwave = pack;
    return true;
}

// Fused decode v2 (stream_fused2.hpp): 2-4 erasures, at most two per section, one section included
// (two in a section: both-erased PFT pairs inverted after the rounds), one launch, rounds of tile
// k-1 on the loader waves while tile k streams.  Ring of 10 - ne node buffers + the S/C region.
// After dec_pattern with per_sec_max = 2: fills a.lwave, a.pinfo, a.npair, a.split and a.ring;
// *two: the TWO instantiation (a section with two erasures).  false: the kernel does not take it.
inline bool fused2_shape(DecArgs &a, bool *two) {
    if (a.ne < 2) return false;
    *two = false;
    for (int y = 0; y < 4; y++) *two = *two || __builtin_popcount(a.emask[y]) > 1;
    if (!f2_plan(a.emask, *two, &a.lwave)) return false;  // more round targets than the kernel's item registers
    // both-erased pairs: per erased row, the other erased row of its section
    a.npair = 0;
    for (int r = 0; r < 4; r++) a.pinfo[r] = 0;
    for (int y = 0; y < 4; y++) {
        if (__builtin_popcount(a.emask[y]) != 2) continue;
        const uint32_t x1 = uint32_t(__builtin_ctz(a.emask[y])), x2 = 31u - uint32_t(__builtin_clz(a.emask[y]));
        const int r1 = a.rix[4 * y + int(x1)], r2 = a.rix[4 * y + int(x2)];
        a.pinfo[r1] = 1u | uint32_t(r2) << 1 | uint32_t(y) << 3 | x1 << 5 | x2 << 7;
        a.pinfo[r2] = 1u | uint32_t(r1) << 1 | uint32_t(y) << 3 | x2 << 5 | x1 << 7;
        a.npair += 2;
    }
    const uint32_t RB = 10 - a.ne;  // the S/C region takes ne of the 10 node buffers of LDS
    // the loads of a step are issued during the step before it when the ring holds both; else
    // (two neighbouring sections with 7-8 alive nodes and RB = 6) the step is split: the rest of
    // its loads after its barrier, behind a second one.  Section 0 of tile k + 1 needs no split:
    // every ring buffer is free at B_r(k), before its barrier.
    a.split = 0;
    for (int y = 0; y < 4; y++) {
        const uint32_t ny = a.sec_off[y + 1] - a.sec_off[y];
        if (ny > RB) return false;
        if (y > 0 && (a.sec_off[y] - a.sec_off[y - 1]) + ny > RB) a.split |= 1u << y;
    }
    if (!*two) a.split = 0;  // (no pattern with one erasure per section overflows the ring)
    a.ring = RB;
    return true;
}

// The kernel a decode runs on
enum class DecKernel : int {
    None,         // no streaming kernel: the plan executor
    Local,        // k_stream_local, 64-byte tiles ("stream-local")
    Local256,     // k_stream_local256 on 8-byte rows ("stream-local256")
    Local256Any,  // its ANY instantiation: any sub-chunk size and chunk alignment ("stream-local256")
    Fused2,       // k_stream_fused2 ("stream-fused2")
};
struct DecChoice {
    DecKernel kernel = DecKernel::None;
    DecArgs a{};       // every field the pattern decides; the pointers, tabs, sc, region and nslots are the launcher's
    int K[4] = {};     // dec_pattern
    int G = 0;         // local kernels: the section instantiated
    bool two = false;  // fused decode: the TWO instantiation
};

// Streaming decodes of q = 4, t = 4 codes with KD = 9 / 10 data nodes, sub-chunks of 512 bytes up to
// 32-bit chunk offsets:
//  * the local decode: auto, "stream" and "stream-local"; on rows of 8-byte multiples at 8-byte
//    aligned chunks (rows8: sc % 8 == 0 and ptrs8) -- the 256-byte-run kernel at any alignment;
//  * the fused decode v2 (rows8): auto from 3 erasures, "stream" and "stream-fused2" from 2
//    ((10,4,13) 1 GiB: {0,4,8,12} 0.52 ms vs 0.92 on the grouped executor, {0,4,8} 0.48 vs 0.79;
//    {0,4} 0.458 vs 0.452 on the local decode; profiles/r04/fused2/).
// Where both are tried: (2,1) sections (two erasures in one section, one in another) take the fused
// decode v2 first -- 0.48-0.53 ms vs 0.50-0.54 on the 64-byte local decode
// (profiles/r06/decode/two_small_*) --, then the local decode, then the fused decode v2.
inline DecChoice choose_decode(int KD, uint32_t erased, uint32_t alive, int xmode, uint64_t sc, bool ptrs8, uint32_t R,
                               bool local_w64) {
    DecChoice c;
    erased &= 0xFFFFu;
    if ((KD != 9 && KD != 10) || sc < 512 || sc >= (uint64_t(1) << 24)) return c;  // 256 layers x sc < 2^32
    const int ne = __builtin_popcount(erased);
    const bool stream_all = xmode == kExecStream;
    const bool try_local = xmode == kExecAuto || stream_all || xmode == kExecStreamLocal;
    const bool try_f2 = xmode == kExecStreamFused2 || stream_all || (xmode == kExecAuto && ne >= 3);
    const SectionErasures se = section_erasures(erased);
    const bool f2_first = try_f2 && try_local && ne == 3 && se.nsec == 2 && se.per[se.most] == 2;
    const bool rows8 = sc % 8 == 0 && ptrs8;
    bool ring_ok = false;
    auto fused2 = [&] {
        if (rows8 && dec_pattern(KD, erased, alive, R, 2, c.a, c.K, &ring_ok) && ring_ok && fused2_shape(c.a, &c.two))
            c.kernel = DecKernel::Fused2;
        return c.kernel != DecKernel::None;
    };
    auto local = [&] {
        const LocalShape s = local_shape(erased, local_w64);
        if (!s.ok || (!s.w256 && !rows8) || !dec_pattern(KD, erased, alive, R, 4, c.a, c.K, &ring_ok) || !ring_ok)
            return false;
        local_columns(s, c.a);
        c.G = s.G;
        c.kernel = !s.w256 ? DecKernel::Local : rows8 ? DecKernel::Local256 : DecKernel::Local256Any;
        return true;
    };
    if (f2_first && fused2()) return c;
    if (try_local && local()) return c;
    if (try_f2 && !f2_first) fused2();
    return c;
}

}  // namespace bs
}  // namespace clay
