// tail_kernel.hip -- finish_rows_kernel: the double-precision tail of the reads a launch_place_reads_deferred launch
// placed, a lane per reported row (tail_device.hpp).  Enqueued right behind that launch on the same stream; rows,
// n_rows and k-mer counts are final when the stream reaches the end of this kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tail_device.hpp"

namespace epik_amd {

constexpr uint32_t kTailBlock = 256;

template <uint32_t kGroup>
__global__ __launch_bounds__(kTailBlock) void finish_rows_kernel(PlaceParams p)
{
    const uint64_t thread = (uint64_t)blockIdx.x * kTailBlock + threadIdx.x;
    const uint64_t read = thread / kGroup;
    finish_rows_group<kGroup>(p, p.tail_ws, read, (uint32_t)(thread % kGroup), read < p.n_reads);
}

namespace {

template <uint32_t kGroup>
hipError_t launch_group(const PlaceParams &p, void *tail_ws, hipStream_t stream)
{
    PlaceParams q = p;
    q.tail_ws = tail_ws;
    const uint64_t blocks = (p.n_reads * kGroup + kTailBlock - 1u) / kTailBlock;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((finish_rows_kernel<kGroup>), dim3((unsigned)blocks), dim3(kTailBlock), 0, stream, q);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_finish_rows(const PlaceParams &p, void *tail_ws, hipStream_t stream)
{
    if (!tail_ws || p.keep_at_most == 0 || p.keep_at_most > kTailMaxKeep) return hipErrorInvalidValue;
    if (p.n_reads == 0) return hipSuccess;
    // the smallest power of two of lanes that holds a read's rows
    const uint32_t keep = p.keep_at_most;
    if (keep <= 1) return launch_group<1>(p, tail_ws, stream);
    if (keep <= 2) return launch_group<2>(p, tail_ws, stream);
    if (keep <= 4) return launch_group<4>(p, tail_ws, stream);
    if (keep <= 8) return launch_group<8>(p, tail_ws, stream);
    if (keep <= 16) return launch_group<16>(p, tail_ws, stream);
    if (keep <= 32) return launch_group<32>(p, tail_ws, stream);
    return launch_group<64>(p, tail_ws, stream);
}

}  // namespace epik_amd
