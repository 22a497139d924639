// decode_fused2_batch.hip -- instantiations and launcher of the batched (BATCH) variant of the fused
// decode v2 (stream_fused2.hpp) for (10,4,13) on 8-byte rows: many stripes of one sub-chunk size with
// the same 2-4 erasures (at most two per y-section), at uniform strides, in ONE launch.  The same
// kernel as the one-stripe decode; only the tile map (BatchMapOf<RoundRobinMap>,
// stream_tile_map.hpp: tile k of a workgroup belongs to stripe i(k)) and the stripe's offset in the
// uniform base of the loads and the stores differ.  (9,4,12), the probe variants and the patterns
// of the local kernels are not instantiated here.  The host-side planning (erasure pattern ->
// DecArgs, the strides) is in engine.hip.
#include <hip/hip_runtime.h>

#include "lds_attr.hpp"
#include "stream_fused2.hpp"

namespace clay {

template <bool TWO>
static hipError_t launch_f2_batch(const bs::DecArgs &a, hipStream_t stream, int dev) {
    constexpr auto kern = &bs::k_stream_fused2<10, 3, 0, TWO, true>;
    const int lds = int(a.ring + a.ne) * bs::kDecBuf;  // ring + S/C region (ne rows)
    if (hipError_t e = lds_attr_once(reinterpret_cast<const void *>(kern), 160 * 1024, dev)) return e;
    // a.groups groups of a.nslots workgroups per XCD
    kern<<<dim3(a.groups * a.nslots * 8), dim3(bs::StreamDec<10, 3>::BLOCK), lds, stream>>>(a);
    return hipGetLastError();
}

// erasures in distinct y-sections, or (two = true) two erasures in some section, in every one of
// a.nstripes stripes
hipError_t launch_stream_fused2_batch_kernel(int kd, const bs::DecArgs &a, hipStream_t stream, int dev, bool two) {
    if (kd != 10 || a.nstripes < 2 || a.groups == 0 || a.nslots == 0 || int(a.ring + a.ne) * bs::kDecBuf > 160 * 1024)
        return hipErrorInvalidValue;
    return two ? launch_f2_batch<true>(a, stream, dev) : launch_f2_batch<false>(a, stream, dev);
}

}  // namespace clay
