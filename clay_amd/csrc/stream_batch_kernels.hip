// stream_batch_kernels.hip -- instantiations and launcher of the batched (BATCH) variant of the
// streaming encode k_stream_encode (stream_encode.hpp) for (10,4,13) and (9,4,12): many stripes of
// one sub-chunk size at uniform strides in ONE launch.  The same kernel as the one-stripe encode
// (4 loader waves, lane map kStreamEncMap); only the tile map (BatchMap, stream_tile_map.hpp: tile
// k of a workgroup belongs to stripe i(k)) and the stripe's offset in the SGPR base of every
// access differ.
#include "lds_attr.hpp"
#include "stream_encode.hpp"

namespace clay {

template <int KD>
static hipError_t launch(const bs::BsArgs &a, hipStream_t stream, int dev) {
    using Kn = bs::StreamEnc<KD, 4>;
    constexpr auto kern = &bs::k_stream_encode<KD, 4, 0, bs::kStreamEncMap, false, true>;
    if (hipError_t e = lds_attr_once(reinterpret_cast<const void *>(kern), Kn::LDS_BYTES, dev)) return e;
    // a.ntiles groups of a.nslots workgroups per XCD
    kern<<<dim3(a.ntiles * a.nslots * 8), dim3(Kn::BLOCK), Kn::LDS_BYTES, stream>>>(a);
    return hipGetLastError();
}

hipError_t launch_stream_batch_kernel(int kd, const bs::BsArgs &a, hipStream_t stream, int dev) {
    if (kd == 10) return launch<10>(a, stream, dev);
    if (kd == 9) return launch<9>(a, stream, dev);
    return hipErrorInvalidValue;
}

}  // namespace clay
