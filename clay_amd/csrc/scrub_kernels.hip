// scrub_kernels.hip -- instantiations and launchers of the compare-ending (SCRUB) variants of
// the bit-sliced encode kernels: k_bs_encode1 (bitslice_line.hpp) for (4,2,5) and k_bs_encode
// (bitslice.hpp, v1) for (4,2), (6,3), (8,4), (9,3) and (10,4) with d = n - 1, each with and
// without byte tails.  Same kernels as the encodes up to the last step, which loads the stored
// parity and compares where the encode stores.  And the compare-ending variant of the streaming
// encode k_stream_encode (stream_encode.hpp) for (10,4,13), one stripe per launch and, with the
// batched tile map (BATCH), many stripes in one.
#include "bitslice_line.hpp"
#include "lds_attr.hpp"
#include "scrub_args.hpp"
#include "stream_encode.hpp"

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

// The compare-ending k_stream_encode of (10,4,13): the library's encode instantiation (4 loader
// waves, lane map kStreamEncMap) with SCRUB.  No LOADERS == 0 variant: its counted vmcnt waits
// count the parity stores of the previous two steps.
hipError_t launch_stream_scrub_kernel(const bs::BsArgs &a, hipStream_t stream, int dev) {
    using Kn = bs::StreamEnc<10, 4>;
    constexpr auto kern = &bs::k_stream_encode<10, 4, 0, bs::kStreamEncMap, true>;
    if (hipError_t e = lds_attr_once(reinterpret_cast<const void *>(kern), Kn::LDS_BYTES, dev)) return e;
    kern<<<dim3(a.nslots * 8), dim3(Kn::BLOCK), Kn::LDS_BYTES, stream>>>(a);
    return hipGetLastError();
}

// The same kernel over many stripes in one launch (SCRUB && BATCH: BatchMap, a.ntiles groups of
// a.nslots workgroups per XCD, one result word per stripe).
hipError_t launch_stream_scrub_batch_kernel(const bs::BsArgs &a, hipStream_t stream, int dev) {
    using Kn = bs::StreamEnc<10, 4>;
    constexpr auto kern = &bs::k_stream_encode<10, 4, 0, bs::kStreamEncMap, true, true>;
    if (hipError_t e = lds_attr_once(reinterpret_cast<const void *>(kern), Kn::LDS_BYTES, dev)) return e;
    kern<<<dim3(8 * a.ntiles * a.nslots), dim3(Kn::BLOCK), Kn::LDS_BYTES, stream>>>(a);
    return hipGetLastError();
}

}  // namespace clay
