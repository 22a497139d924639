// repair_stream.hip -- instantiations and launchers of the bit-sliced repair kernels
// (repair_kernel.hpp), in their own translation unit; the host-side checks are in engine.hip.
#include <hip/hip_runtime.h>

#include "lds_attr.hpp"
#include "repair_kernel.hpp"

namespace clay {

template <int KD, int M, int Y0>
static hipError_t launch_one(bs::RepArgs a, hipStream_t stream) {
    using Kn = bs::BsRepair<KD, M, Y0>;
    a.ntiles = uint32_t((a.sc - a.b_start + Kn::W - 1) / Kn::W);
    a.per_xcd = (a.ntiles + 7) / 8;
    bs::k_bs_repair<KD, M, Y0><<<dim3(a.per_xcd * 8), dim3(Kn::BLOCK), 0, stream>>>(a);
    return hipGetLastError();
}

// batch form: a.h / a.out are stripe 0's, a.sin / a.sout / a.cps / a.ncols set by the caller
// (ncols fits 32 bits); tiles of PARTS columns in the XCD-contiguous order of launch_one
template <int KD, int M, int Y0, bool JF>
static hipError_t launch_one_batch(bs::RepArgs a, hipStream_t stream) {
    using Kn = bs::BsRepair<KD, M, Y0>;
    a.b_start = 0;
    a.ntiles = uint32_t(bs::rep_batch_ntiles(a.ncols, uint32_t(Kn::PARTS)));
    a.per_xcd = (a.ntiles + 7) / 8;
    bs::k_bs_repair<KD, M, Y0, true, JF><<<dim3(a.per_xcd * 8), dim3(Kn::BLOCK), 0, stream>>>(a);
    return hipGetLastError();
}

template <int KD, int M, bool JF>
static hipError_t launch_km_batch(int y0, const bs::RepArgs &a, hipStream_t stream) {
    switch (y0) {
    case 0: return launch_one_batch<KD, M, 0, JF>(a, stream);
    case 1: return launch_one_batch<KD, M, 1, JF>(a, stream);
    case 2: return launch_one_batch<KD, M, 2, JF>(a, stream);
    default:
        if constexpr (bs::Shape<KD, M>::T > 3) return launch_one_batch<KD, M, 3, JF>(a, stream);
        return hipErrorInvalidValue;
    }
}

// streaming variant: one workgroup per CU; returns hipErrorNotSupported when the launch should
// fall back to the direct kernel
template <int KD, int M, int Y0, int PARTS, int LOADERS>
static hipError_t launch_stream(const bs::RepArgs &a, hipStream_t stream, int dev, int cus, bool force,
                                int *launches, bool *streamed) {
    using Kn = bs::BsRepairStream<KD, M, Y0, PARTS, LOADERS>;
    const uint64_t nfull = a.sc / uint64_t(Kn::W);
    const uint32_t ns = uint32_t(cus >= 8 ? cus / 8 : 1);
    if (!force && nfull < uint64_t(8) * ns) return hipErrorNotSupported;  // under one tile per CU
    if (a.sc < 16) return hipErrorNotSupported;  // a partial tile reads whole 16-byte pieces
    if (a.sc * uint64_t(Kn::B::ALPHA) >= (uint64_t(1) << 32)) return hipErrorNotSupported;  // 32-bit row offsets
    if (hipError_t e = lds_attr_once(reinterpret_cast<const void *>(&bs::k_bs_repair_stream<KD, M, Y0, PARTS, LOADERS>),
                                     Kn::LDS_BYTES, dev))
        return e;
    bs::RepStreamArgs sa{};
    sa.r = a;
    sa.region = bs::xcd_region(a.sc);
    sa.ns = ns;
    bs::k_bs_repair_stream<KD, M, Y0, PARTS, LOADERS><<<dim3(ns * 8), dim3(Kn::BLOCK), Kn::LDS_BYTES, stream>>>(sa);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    *launches += 1;
    *streamed = true;
    return hipSuccess;
}

template <int KD, int M, int PARTS, int LOADERS>
static hipError_t launch_km(int y0, const bs::RepArgs &a, hipStream_t stream, int dev, int cus, int stream_mode,
                            bool *streamed, int *launches) {
    *streamed = false;
    *launches = 1;
    if constexpr (PARTS > 0) {
        if (stream_mode > 0) {
            *launches = 0;
            hipError_t e = hipErrorNotSupported;
            const bool force = stream_mode == 2;
            switch (y0) {
            case 0: e = launch_stream<KD, M, 0, PARTS, LOADERS>(a, stream, dev, cus, force, launches, streamed); break;
            case 1: e = launch_stream<KD, M, 1, PARTS, LOADERS>(a, stream, dev, cus, force, launches, streamed); break;
            case 2: e = launch_stream<KD, M, 2, PARTS, LOADERS>(a, stream, dev, cus, force, launches, streamed); break;
            default:
                if constexpr (bs::Shape<KD, M>::T > 3) e = launch_stream<KD, M, 3, PARTS, LOADERS>(a, stream, dev, cus, force, launches, streamed);
                break;
            }
            if (e != hipErrorNotSupported) return e;
            if (stream_mode == 3) return hipErrorNotSupported;  // streaming kernel only
            *launches = 1;
        }
    }
    if (stream_mode == 3) return hipErrorNotSupported;
    switch (y0) {
    case 0: return launch_one<KD, M, 0>(a, stream);
    case 1: return launch_one<KD, M, 1>(a, stream);
    case 2: return launch_one<KD, M, 2>(a, stream);
    default:
        if constexpr (bs::Shape<KD, M>::T > 3) return launch_one<KD, M, 3>(a, stream);
        return hipErrorInvalidValue;
    }
}

// stream_mode: 0 = direct kernel, 1 = streaming kernel when the sub-chunk gives every CU a
// tile, 2 = streaming kernel whenever the code has one, 3 = the streaming kernel when the
// sub-chunk gives every CU a tile, else nothing.  Returns 1 = direct kernel launched, 2 =
// streaming kernel launched, 0 = no instantiation for (k, m) (or none launched in mode 3), < 0 =
// HIP error; *launches = kernel launches issued.
int launch_bs_repair_kernel(int k, int m, int y0, const bs::RepArgs &a, hipStream_t stream, int dev, int cus,
                            int stream_mode, int *launches) {
    hipError_t e;
    bool streamed = false;
    if (k == 9 && m == 3) e = launch_km<9, 3, 16, 7>(y0, a, stream, dev, cus, stream_mode, &streamed, launches);
    // (10,4): 128-byte tiles (12.8 per CU on the 1 GiB stripe's 419,432-byte sub-chunks; 256-byte
    // tiles: 6.4 per CU and a longer tail, 0.161 vs 0.139 ms, profiles/r04/repair/)
    else if (k == 10 && m == 4) e = launch_km<10, 4, 4, 4>(y0, a, stream, dev, cus, stream_mode, &streamed, launches);
    else if (k == 4 && m == 2) e = launch_km<4, 2, 0, 0>(y0, a, stream, dev, cus, stream_mode, &streamed, launches);
    else return 0;
    if (e == hipErrorNotSupported && stream_mode == 3) return 0;
    if (e != hipSuccess) return -int(e);
    return streamed ? 2 : 1;
}

// Batch form of k_bs_repair (column-flattened, repair_batch_map.hpp): one launch for every stripe
// of the batch.  Returns 1 = launched, 0 = no instantiation for (k, m), < 0 = HIP error.
// jfast: the j-fastest lane order (the caller's rule: engine.hip kRepairBatchJfastMaxSc).
int launch_bs_repair_batch_kernel(int k, int m, int y0, const bs::RepArgs &a, hipStream_t stream, bool jfast) {
    hipError_t e;
    if (a.ncols == 0 || a.cps == 0) return 0;
    if (k == 9 && m == 3) e = jfast ? launch_km_batch<9, 3, true>(y0, a, stream) : launch_km_batch<9, 3, false>(y0, a, stream);
    else if (k == 10 && m == 4) e = jfast ? launch_km_batch<10, 4, true>(y0, a, stream) : launch_km_batch<10, 4, false>(y0, a, stream);
    else if (k == 4 && m == 2) e = jfast ? launch_km_batch<4, 2, true>(y0, a, stream) : launch_km_batch<4, 2, false>(y0, a, stream);
    else return 0;
    if (e != hipSuccess) return -int(e);
    return 1;
}

}  // namespace clay
