// decode_local256_batch.hip -- instantiations and launcher of the batched (BATCH) variant of the
// local decode on 256-byte row runs (stream_local256.hpp) for (10,4,13) on 8-byte rows: many
// stripes of one sub-chunk size with the same one or two erasures, at uniform strides, in ONE
// launch.  The same kernel as the one-stripe decode; only the tile map (BatchMapOf<StreamMap>,
// stream_tile_map.hpp: tile k of a workgroup belongs to stripe i(k)) and the stripe's offset in
// the uniform base of every access differ.  (9,4,12) and rows off 8-byte alignment keep one launch
// per stripe.  The host-side planning (erasure pattern -> DecArgs, the strides) is in engine.hip.
#include <hip/hip_runtime.h>

#include "lds_attr.hpp"
#include "stream_local256.hpp"

namespace clay {

template <int G, int NE>
static hipError_t launch_l256_batch(const bs::DecArgs &a, hipStream_t stream, int dev) {
    using Kn = bs::Local256<10, G, NE, false, true>;
    constexpr auto kern = &bs::k_stream_local256<10, G, NE, false, true>;
    if (hipError_t e = lds_attr_once(reinterpret_cast<const void *>(kern), Kn::LDS_BYTES, dev)) return e;
    // a.groups groups of a.nslots workgroups per XCD
    kern<<<dim3(a.groups * a.nslots * 8), dim3(Kn::BLOCK), Kn::LDS_BYTES, stream>>>(a);
    return hipGetLastError();
}

template <int NE>
static hipError_t launch_l256_batch_g(int g, const bs::DecArgs &a, hipStream_t stream, int dev) {
    switch (g) {
    case 0: return launch_l256_batch<0, NE>(a, stream, dev);
    case 1: return launch_l256_batch<1, NE>(a, stream, dev);
    case 2: return launch_l256_batch<2, NE>(a, stream, dev);
    case 3: return launch_l256_batch<3, NE>(a, stream, dev);
    default: return hipErrorInvalidValue;
    }
}

// one erasure in section g plus at most one in another section, or two in g (ne = 1 or 2), in
// every one of a.nstripes stripes
hipError_t launch_stream_local256_batch_kernel(int kd, int g, const bs::DecArgs &a, hipStream_t stream, int dev) {
    if (kd != 10 || a.nstripes < 2 || a.groups == 0 || a.nslots == 0) return hipErrorInvalidValue;
    return a.ne == 1 ? launch_l256_batch_g<1>(g, a, stream, dev) : launch_l256_batch_g<2>(g, a, stream, dev);
}

}  // namespace clay
