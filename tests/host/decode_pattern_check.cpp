// Host check of the decode dispatch (clay_amd/csrc/decode_pattern.hpp: choose_decode and what it is
// built from), the kernel every erasure pattern of (10,4,13) and (9,4,12) runs on.  For KD = 10 and
// 9, every set of 1-4 erased external nodes with every other node alive, the exec modes auto,
// stream, stream-local and stream-fused2, and sub-chunks of 512 and 520 bytes on 8-byte rows, 516
// bytes, and 512 bytes at chunk pointers off 8-byte alignment (ring R = 10, local_w64 off), one line
//   kd e0,e1,.. mode sc ptrs8 kernel [G g2 scase0..3 | scase0..3 lwave split npair]
// (the local kernels: the first form; fused2: the second; none: neither), then a few declines
//   decline kd e0,e1,.. mode sc ptrs8 R alive kernel
// tests/test_decode_pattern_cpu.py compares every line with tests/decode_pattern.py, the tests' own
// restatement.  Checks a few invariants itself: exits 0 and ends with "decode pattern ok: <cases>
// cases", else prints the failures and exits 1.  Also run under ASan + UBSan by
// scripts/host_checks_sanitized.sh.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "decode_pattern.hpp"

using clay::bs::choose_decode;
using clay::bs::DecChoice;
using clay::bs::DecKernel;

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

struct Mode {
    const char *name;
    int xmode;
};
static const Mode kModes[] = {{"auto", clay::kExecAuto},
                              {"stream", clay::kExecStream},
                              {"stream-local", clay::kExecStreamLocal},
                              {"stream-fused2", clay::kExecStreamFused2}};

static const char *name_of(DecKernel k) {
    switch (k) {
        case DecKernel::Local: return "local";
        case DecKernel::Local256: return "local256";
        case DecKernel::Local256Any: return "local256-any";
        case DecKernel::Fused2: return "fused2";
        default: return "none";
    }
}

static uint32_t internal_of(int kd, int e) { return uint32_t(e < kd ? e : e + 12 - kd); }

static std::string list_of(const std::vector<int> &er) {
    std::string s;
    for (size_t i = 0; i < er.size(); i++) s += (i ? "," : "") + std::to_string(er[i]);
    return s;
}

int main() {
    struct Rows {
        uint64_t sc;
        bool ptrs8;
    };
    const Rows rows[] = {{512, true}, {520, true}, {516, true}, {512, false}};
    long cases = 0;
    for (int kd : {10, 9}) {
        const int n = kd + 4;
        uint32_t every = 0;
        for (int e = 0; e < n; e++) every |= 1u << internal_of(kd, e);
        for (int ne = 1; ne <= 4; ne++) {
            std::vector<int> er(ne);
            for (int i = 0; i < ne; i++) er[i] = i;
            for (;;) {
                uint32_t erased = 0;
                for (int e : er) erased |= 1u << internal_of(kd, e);
                const std::string ers = list_of(er);
                for (const Rows &r : rows) {
                    DecKernel k_auto = DecKernel::None;
                    for (const Mode &m : kModes) {
                        const DecChoice c = choose_decode(kd, erased, every & ~erased, m.xmode, r.sc, r.ptrs8, 10, false);
                        printf("%d %s %s %llu %d %s", kd, ers.c_str(), m.name, (unsigned long long)r.sc, int(r.ptrs8),
                               name_of(c.kernel));
                        const bool rows8 = r.sc % 8 == 0 && r.ptrs8;
                        if (c.kernel == DecKernel::Fused2) {
                            printf(" %d %d %d %d %u %u %u", c.a.scase[0], c.a.scase[1], c.a.scase[2], c.a.scase[3],
                                   c.a.lwave, c.a.split, c.a.npair);
                            CHECK(rows8 && ne >= 2 && c.a.ring == uint32_t(10 - ne), "%d %s: ring %u", kd, ers.c_str(), c.a.ring);
                            CHECK(c.two == (c.a.npair != 0) && (c.two || !c.a.split), "%d %s: two %d npair %u split %u", kd,
                                  ers.c_str(), int(c.two), c.a.npair, c.a.split);
                        } else if (c.kernel != DecKernel::None) {
                            printf(" %d %d %d %d %d %d", c.G, c.a.g2, c.a.scase[0], c.a.scase[1], c.a.scase[2], c.a.scase[3]);
                            CHECK(c.G >= 0 && c.G < 4 && c.a.emask[c.G] && c.a.g2 != c.G && c.a.ring == 10, "%d %s: G %d g2 %d", kd,
                                  ers.c_str(), c.G, c.a.g2);
                            CHECK(rows8 == (c.kernel != DecKernel::Local256Any), "%d %s: %s", kd, ers.c_str(), name_of(c.kernel));
                        }
                        if (c.kernel != DecKernel::None)
                            CHECK(c.a.ne == uint32_t(ne) && c.a.nt == uint32_t(n - ne) && c.a.sec_off[4] == c.a.nt &&
                                      __builtin_popcount(c.a.used) == 12 && !(c.a.used & erased),
                                  "%d %s: ne %u nt %u used %x", kd, ers.c_str(), c.a.ne, c.a.nt, c.a.used);
                        printf("\n");
                        cases++;
                        // auto names the kernel "stream" names (the modes print in that order)
                        if (m.xmode == clay::kExecAuto) k_auto = c.kernel;
                        if (m.xmode == clay::kExecStream)
                            CHECK(c.kernel == k_auto, "%d %s sc %llu: auto %s, stream %s", kd, ers.c_str(),
                                  (unsigned long long)r.sc, name_of(k_auto), name_of(c.kernel));
                    }
                }
                // the next set in lexicographic order
                int i = ne - 1;
                while (i >= 0 && er[i] == n - ne + i) i--;
                if (i < 0) break;
                er[i]++;
                for (int j = i + 1; j < ne; j++) er[j] = er[j - 1] + 1;
            }
        }
    }
    // declines: a sub-chunk under 512 bytes, a ring of 4 buffers, a node that is neither erased nor alive
    struct Decline {
        int kd;
        std::vector<int> er;
        uint64_t sc;
        uint32_t R;
        int dead;  // an external node without an input pointer (-1: none)
    };
    const Decline declines[] = {{10, {0}, 504, 10, -1},         {10, {0, 4, 8, 12}, 504, 10, -1}, {9, {0, 4}, 504, 10, -1},
                                {10, {0}, 520, 4, -1},          {10, {0, 4, 8, 12}, 520, 4, -1},  {9, {0, 1, 4}, 520, 4, -1},
                                {10, {0, 4, 8, 12}, 520, 10, 5}};
    for (const Decline &d : declines) {
        uint32_t erased = 0, alive = 0;
        for (int e : d.er) erased |= 1u << internal_of(d.kd, e);
        for (int e = 0; e < d.kd + 4; e++)
            if (e != d.dead) alive |= 1u << internal_of(d.kd, e);
        alive &= ~erased;
        for (const Mode &m : kModes) {
            const DecChoice c = choose_decode(d.kd, erased, alive, m.xmode, d.sc, true, d.R, false);
            printf("decline %d %s %s %llu 1 %u %x %s\n", d.kd, list_of(d.er).c_str(), m.name, (unsigned long long)d.sc, d.R, alive,
                   name_of(c.kernel));
            CHECK(c.kernel == DecKernel::None,"%d %s sc %llu R %u: %s", d.kd, list_of(d.er).c_str(),
                  (unsigned long long)d.sc, d.R, name_of(c.kernel));
            cases++;
        }
    }
    if (failures) {
        printf("decode pattern: %d failures\n", failures);
        return 1;
    }
    printf("decode pattern ok: %ld cases\n", cases);
    return 0;
}
