// stripe_layout.hpp -- where the operands of a batch of stripes live.  Host-only, plain integer
// code (no HIP), so that a host program can include it (tests/test_stripe_layout_cpu.py).
//
// A batched call names `per` operands per stripe (data nodes, parity nodes, helper buffers, one
// output, ...) in one of two forms:
//   * pointer arrays: operand i of stripe s is ptrs[s * per + i];
//   * strides: operand i of stripe s is base + s * stripe + node_of(i) * node, where node_of(i) is
//     index[i] (the repair's helpers sit at their external node ids) or i, and an operand with
//     absent[i] set is NULL in every stripe (the decode's erased inputs and its present outputs).
// Addresses are only computed here, never dereferenced: asking for a stripe past the last one, or
// for the distance between rows of unrelated buffers, is plain integer arithmetic.
//
// Inputs and outputs share the type: it holds uint8_t *, and an input family is built from const
// pointers (the kernels' argument structs restore the const).
#pragma once

#include <cstddef>
#include <cstdint>

namespace clay {

struct StripeOperands {
    bool strided = false;
    uint8_t *const *ptrs = nullptr;  // pointer arrays
    uint8_t *base = nullptr;         // strides
    int64_t node = 0, stripe = 0;
    size_t per = 0;                   // operands per stripe (set by whoever knows the code)
    const size_t *index = nullptr;    // strides: node of operand i (nullptr: i)
    const uint8_t *absent = nullptr;  // strides: operands that are NULL (nullptr: none)

    static StripeOperands from_arrays(const uint8_t *const *ptrs, size_t per = 0) {
        StripeOperands f;
        f.ptrs = const_cast<uint8_t *const *>(ptrs);
        f.per = per;
        return f;
    }
    static StripeOperands from_strides(const uint8_t *base, int64_t node, int64_t stripe, size_t per = 0) {
        StripeOperands f;
        f.strided = true;
        f.base = const_cast<uint8_t *>(base);
        f.node = node;
        f.stripe = stripe;
        f.per = per;
        return f;
    }
    // the caller passed NULL for the arrays / the base
    bool null() const { return strided ? !base : !ptrs; }

    uint8_t *at(size_t s, size_t i) const {
        if (!strided) return ptrs[s * per + i];
        if (absent && absent[i]) return nullptr;
        const int64_t off = int64_t(s) * stripe + int64_t(index ? index[i] : i) * node;
        return reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(base) + uintptr_t(off));
    }
    // stripe s as a plain pointer array of `per` entries
    void stripe_ptrs(size_t s, uint8_t **out) const {
        for (size_t i = 0; i < per; i++) out[i] = at(s, i);
    }
};

// Do the stripes [s0, s0 + ns) sit at one stride for the n operands idx[0..n) (idx == nullptr:
// operands 0..n-1): at(s0 + s, i) == at(s0, i) + s * *stride for every listed i and every s < ns?
// Strides: yes by construction, *stride = the caller's stripe stride (for ns == 1 too), O(1).
// Pointer arrays: *stride = the distance of the first listed operand between stripes s0 and s0 + 1
// (0 for ns == 1), then a scan.  *stride is set either way.  This answer picks between a
// single-launch kernel (base + stride in its arguments) and a pointer table, so a wrong "yes"
// sends a kernel to memory the caller never named.
inline bool uniform_stride(const StripeOperands &f, size_t s0, size_t ns, const size_t *idx, size_t n,
                           int64_t *stride) {
    if (f.strided) {
        *stride = f.stripe;
        return true;
    }
    auto addr = [&](size_t s, size_t j) {
        return reinterpret_cast<uintptr_t>(f.ptrs[(s0 + s) * f.per + (idx ? idx[j] : j)]);
    };
    const uintptr_t st = ns > 1 && n > 0 ? addr(1, 0) - addr(0, 0) : 0;
    *stride = int64_t(st);
    for (size_t s = 1; s < ns; s++)
        for (size_t j = 0; j < n; j++)
            if (addr(s, j) != addr(0, j) + uintptr_t(s) * st) return false;
    return true;
}

}  // namespace clay
