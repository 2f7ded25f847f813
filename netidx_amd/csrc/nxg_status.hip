// nxg_status.hip -- the status gather: the DevStatus slots of a run of calls, copied from the
// device ring to its pinned host mirror by a kernel enqueued behind those calls.
//
// nxg_ctx_sync reads the status of every pending call. A copy command for that costs a host round
// trip of its own: it can only be waited for after it was issued, and it goes through the copy
// path. This kernel runs in stream order the moment the last of the calls ends, with no host in
// the loop, and the end of the kernel makes its stores visible to the host: one
// hipStreamSynchronize then suffices.
#include "nxg_device.h"
#include "nxg_internal.h"

namespace {

constexpr int TPB = 256;
constexpr uint32_t Q = sizeof(DevStatus) / 16;  // 16-byte words per slot
static_assert(sizeof(DevStatus) % 16 == 0, "DevStatus is copied in 16-byte words");

// slots s0, s0 + 1, ... (n of them, modulo `ring`: a range that wraps is two ranges here)
__global__ __launch_bounds__(TPB) void nxg_status_gather_kernel(const DevStatus* __restrict__ dst,
                                                                DevStatus* __restrict__ hst,
                                                                uint32_t s0, uint32_t n,
                                                                uint32_t ring) {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(dst);
    uint4* __restrict__ out = reinterpret_cast<uint4*>(hst);
#pragma unroll 1
    for (uint32_t i = threadIdx.x; i < n * Q; i += TPB) {
        const uint32_t slot = (s0 + i / Q) % ring;
        const uint32_t w = slot * Q + i % Q;
        out[w] = src[w];
    }
}

}  // namespace

// `hst_dev`: the device address of the pinned mirror (hipHostGetDevicePointer). n <= ring.
hipError_t nxg_launch_status_gather(const DevStatus* dst, DevStatus* hst_dev, uint32_t s0,
                                    uint32_t n, uint32_t ring, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (n > ring || s0 >= ring) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nxg_status_gather_kernel, dim3(1), dim3(TPB), 0, s, dst, hst_dev, s0, n,
                       ring);
    return hipGetLastError();
}
