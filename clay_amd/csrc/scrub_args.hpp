// scrub_args.hpp -- launchers of the compare-ending (SCRUB) instantiations of the two bit-sliced
// encode kernels, shared by the host (engine.hip) and their translation unit (scrub_kernels.hip).
// The kernels take the encodes' argument structs (Enc1Args of line_args.hpp, BsArgs of
// bitslice.hpp) with `res` set: they read data and stored parity, write nothing but res[stripe].
#pragma once
#include "bitslice.hpp"
#include "line_args.hpp"

namespace clay {

// scrub_kernels.hip: k_bs_encode1<.., SCRUB> for code (k, m), grid a.nslots * 8; bt = byte tails.
// hipErrorInvalidValue: no instantiation
hipError_t launch_bs_scrub1_kernel(int k, int m, bool bt, const bs::Enc1Args &a, hipStream_t stream);
// scrub_kernels.hip: k_bs_encode<.., SCRUB> (v1) for code (k, m) with d = k + m - 1, grid
// a.nslots * 8; bt = byte tails.  hipErrorInvalidValue: no instantiation
hipError_t launch_bs_scrub_kernel(int k, int m, bool bt, const bs::BsArgs &a, hipStream_t stream);
// scrub_kernels.hip: k_stream_encode<10, 4 loaders, .., SCRUB> for (10,4,13), one stripe: the
// streaming encode's arguments (a.tiles_per_xcd = XCD region bytes, grid a.nslots * 8) with a.res
// set; rows 8-byte aligned, a.sc % 8 == 0, a.sc >= 16, 256 * a.sc < 2^32.  Sets the kernel's
// dynamic-LDS attribute once per device `dev`
hipError_t launch_stream_scrub_kernel(const bs::BsArgs &a, hipStream_t stream, int dev);
// scrub_kernels.hip: k_stream_encode<10, 4 loaders, .., SCRUB, BATCH>: a.nstripes stripes of
// (10,4,13) in one launch, stripe i's nodes at a.data[node] + i * a.sdata and a.par[X] + i * a.spar,
// its result word a.res[i].  The batched streaming encode's arguments (a.nslots = workgroups per
// XCD of one stripe's cut, a.ntiles = groups of them; grid 8 * a.ntiles * a.nslots) with a.res set;
// the one-stripe launcher's conditions hold for every stripe.  Sets the dynamic-LDS attribute once
// per device `dev`
hipError_t launch_stream_scrub_batch_kernel(const bs::BsArgs &a, hipStream_t stream, int dev);

// The one column-group count (PG) per code the v1 scrub is instantiated with: the host sizes
// tiles and slots from BsKernel<KD, M, ScrubPg<KD, M>::value>
template <int KD, int M>
struct ScrubPg;
template <> struct ScrubPg<4, 2> { static constexpr int value = 64; };
template <> struct ScrubPg<6, 3> { static constexpr int value = 16; };
template <> struct ScrubPg<8, 4> { static constexpr int value = 8; };
template <> struct ScrubPg<9, 3> { static constexpr int value = 6; };
template <> struct ScrubPg<10, 4> { static constexpr int value = 2; };

}  // namespace clay
