// scrub_kernels.hip -- instantiations and launchers of the compare-ending (SCRUB) variants of
// the bit-sliced encode kernels: k_bs_encode1 (bitslice_line.hpp) for (4,2,5) and k_bs_encode
// (bitslice.hpp, v1) for (4,2), (6,3), (8,4), (9,3) and (10,4) with d = n - 1, each with and
// without byte tails.  Same kernels as the encodes up to the last step, which loads the stored
// parity and compares where the encode stores.
#include "bitslice_line.hpp"
#include "scrub_args.hpp"

namespace clay {

hipError_t launch_bs_scrub1_kernel(int k, int m, bool bt, const bs::Enc1Args &a, hipStream_t stream) {
    if (k == 4 && m == 2) {
        constexpr int PG = ScrubPg<4, 2>::value;  // the encode's tile (line_kernels.hip)
        using Kn = bs::Enc1Kernel<4, 2, PG>;
        if (bt) bs::k_bs_encode1<4, 2, PG, true, true><<<dim3(a.nslots * 8), dim3(Kn::BLOCK), 0, stream>>>(a);
        else bs::k_bs_encode1<4, 2, PG, false, true><<<dim3(a.nslots * 8), dim3(Kn::BLOCK), 0, stream>>>(a);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

template <int KD, int M>
static hipError_t launch_v1(bool bt, const bs::BsArgs &a, hipStream_t stream) {
    constexpr int PG = ScrubPg<KD, M>::value;
    using Kn = bs::BsKernel<KD, M, PG>;
    if (bt) bs::k_bs_encode<KD, M, PG, true, true><<<dim3(a.nslots * 8), dim3(Kn::BLOCK), 0, stream>>>(a);
    else bs::k_bs_encode<KD, M, PG, false, true><<<dim3(a.nslots * 8), dim3(Kn::BLOCK), 0, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_bs_scrub_kernel(int k, int m, bool bt, const bs::BsArgs &a, hipStream_t stream) {
    switch (k * 100 + m) {
    case 402: return launch_v1<4, 2>(bt, a, stream);
    case 603: return launch_v1<6, 3>(bt, a, stream);
    case 804: return launch_v1<8, 4>(bt, a, stream);
    case 903: return launch_v1<9, 3>(bt, a, stream);
    case 1004: return launch_v1<10, 4>(bt, a, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace clay
