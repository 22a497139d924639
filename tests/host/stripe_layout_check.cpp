// Host check of the stripe layout (clay_amd/csrc/stripe_layout.hpp): both forms of a family of
// `per` operands per stripe (pointer arrays, strides), per in 1..6 and 1..9 stripes, over odd,
// negative and zero strides.  Addresses are integers cast to pointers; nothing is dereferenced.
//  * at() equals the defining formula of each form (index map and absent operands included);
//  * pointer arrays built from a strided layout are uniform with that stride, for every subset of
//    operands listed and from every first stripe s0;
//  * moving any single entry (s >= 1, i) of a listed operand makes them non-uniform (but for two
//    stripes of a single operand, which sit at one stride wherever they are); moving an entry of
//    an operand that is not listed does not;
//  * one stripe: the strided form reports the caller's stripe stride, the pointer form 0.
// Built and run by tests/test_stripe_layout_cpu.py; exits 0 and prints
// "stripe layout ok: <cases> cases" when every check holds, else prints the failures and exits 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stripe_layout.hpp"

using clay::StripeOperands;
using clay::uniform_stride;

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

static const uintptr_t kBase = uintptr_t(1) << 40;

static uint8_t *ptr(uintptr_t a) { return reinterpret_cast<uint8_t *>(a); }
static uintptr_t addr(const uint8_t *p) { return reinterpret_cast<uintptr_t>(p); }

static long check(size_t per, size_t ns, int64_t node, int64_t stripe) {
    long cases = 0;
    // strides, plain / with an index map (operand i at node 2 * i + 1) / with absent operands
    std::vector<size_t> index(per);
    std::vector<uint8_t> absent(per);
    for (size_t i = 0; i < per; i++) {
        index[i] = 2 * i + 1;
        absent[i] = uint8_t(i % 2);
    }
    const StripeOperands plain = StripeOperands::from_strides(ptr(kBase), node, stripe, per);
    StripeOperands mapped = plain, holes = plain;
    mapped.index = index.data();
    holes.absent = absent.data();
    CHECK(plain.strided && !plain.null(), "per %zu", per);
    CHECK(StripeOperands::from_strides(nullptr, node, stripe, per).null(), "per %zu", per);
    for (size_t s = 0; s <= ns; s++)  // s == ns: the stripe past the last one is computed, not read
        for (size_t i = 0; i < per; i++) {
            const uintptr_t want = kBase + uintptr_t(int64_t(s) * stripe + int64_t(i) * node);
            CHECK(addr(plain.at(s, i)) == want, "per %zu s %zu i %zu", per, s, i);
            CHECK(addr(mapped.at(s, i)) == kBase + uintptr_t(int64_t(s) * stripe + int64_t(2 * i + 1) * node),
                  "index map: per %zu s %zu i %zu", per, s, i);
            CHECK(addr(holes.at(s, i)) == (i % 2 ? 0 : want), "absent: per %zu s %zu i %zu", per, s, i);
            cases += 3;
        }
    // O(1) and the caller's stride whatever the stripe count, one stripe included
    for (const StripeOperands &f : {plain, mapped, holes}) {
        int64_t st = 12345;
        CHECK(uniform_stride(f, 0, ns, nullptr, per, &st) && st == stripe, "ns %zu stride %lld", ns, (long long)st);
        st = 12345;
        CHECK(uniform_stride(f, 0, 1, nullptr, per, &st) && st == stripe, "one stripe: stride %lld", (long long)st);
        cases += 2;
    }

    // pointer arrays built from the strided layout (one spare stripe at the end)
    std::vector<uint8_t *> tab((ns + 1) * per), row(per);
    for (size_t s = 0; s <= ns; s++) {
        plain.stripe_ptrs(s, row.data());
        for (size_t i = 0; i < per; i++) tab[s * per + i] = row[i];
    }
    const StripeOperands arr = StripeOperands::from_arrays(tab.data(), per);
    CHECK(!arr.strided && !arr.null() && StripeOperands::from_arrays(nullptr, per).null(), "per %zu", per);
    for (size_t s = 0; s <= ns; s++)
        for (size_t i = 0; i < per; i++) {
            CHECK(arr.at(s, i) == tab[s * per + i] && arr.at(s, i) == plain.at(s, i), "per %zu s %zu i %zu", per, s, i);
            cases++;
        }
    {
        int64_t st = 12345;
        CHECK(uniform_stride(arr, 0, 1, nullptr, per, &st) && st == 0, "one stripe: stride %lld", (long long)st);
        cases++;
    }
    // every non-empty subset of operands, in ascending order (the first listed one gives the stride)
    for (uint32_t mask = 1; mask < (1u << per); mask++) {
        std::vector<size_t> idx;
        for (size_t i = 0; i < per; i++)
            if ((mask >> i) & 1u) idx.push_back(i);
        for (size_t s0 = 0; s0 < 2 && s0 < ns; s0++) {
            const size_t n = ns - s0;
            int64_t st = 12345;
            const bool u = uniform_stride(arr, s0, n, idx.data(), idx.size(), &st);
            CHECK(u && st == (n > 1 ? stripe : 0), "per %zu ns %zu s0 %zu mask %u: %d stride %lld", per, ns, s0, mask,
                  int(u), (long long)st);
            cases++;
        }
        // one entry moved by one byte
        for (size_t s = 1; s < ns; s++)
            for (size_t i = 0; i < per; i++) {
                uint8_t *const keep = tab[s * per + i];
                tab[s * per + i] = ptr(addr(keep) + 1);
                int64_t st = 0;
                const bool u = uniform_stride(arr, 0, ns, idx.data(), idx.size(), &st);
                const bool listed = ((mask >> i) & 1u) != 0;
                // (two stripes of a single operand sit at one stride wherever they are)
                const bool two_points = ns == 2 && idx.size() == 1;
                CHECK(u == (!listed || two_points), "per %zu ns %zu mask %u moved (%zu, %zu): uniform %d", per, ns, mask, s, i, int(u));
                // stripe 1 of the first listed operand sets the stride, moved or not
                if (!(listed && s == 1 && i == idx[0]))
                    CHECK(st == stripe, "per %zu ns %zu mask %u moved (%zu, %zu): stride %lld", per, ns, mask, s, i,
                          (long long)st);
                tab[s * per + i] = keep;
                cases++;
            }
    }
    // idx == nullptr lists operands 0..n-1: a moved entry of operand n or later does not count
    for (size_t n = 1; n <= per; n++)
        for (size_t i = 0; i < per && ns > 1; i++) {
            uint8_t *const keep = tab[(ns - 1) * per + i];
            tab[(ns - 1) * per + i] = ptr(addr(keep) + 8);
            int64_t st = 0;
            CHECK(uniform_stride(arr, 0, ns, nullptr, n, &st) == (i >= n || (ns == 2 && n == 1)),
                  "per %zu ns %zu first %zu moved %zu", per, ns, n, i);
            tab[(ns - 1) * per + i] = keep;
            cases++;
        }
    return cases;
}

int main() {
    long cases = 0;
    const int64_t nodes[] = {64, 61, -40, 0};
    const int64_t stripes[] = {1024, 1021, 7, -1024, -333, 0};
    for (size_t per = 1; per <= 6; per++)
        for (size_t ns = 1; ns <= 9; ns++)
            for (int64_t node : nodes)
                for (int64_t stripe : stripes) cases += check(per, ns, node, stripe);
    if (failures) {
        printf("stripe layout FAILED: %d checks\n", failures);
        return 1;
    }
    printf("stripe layout ok: %ld cases\n", cases);
    return 0;
}
