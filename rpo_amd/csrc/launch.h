// The one kernel launch of the C-ABI entry points.  Host code only; needs nothing but the HIP runtime, so the env units
// (cartsafe.hip, pendulum.hip, evopf.hip) take it without the MLP tiles that host_glue.h pulls in.
#pragma once
#include <hip/hip_runtime.h>

namespace rpo_host {

// Launch and answer like RPO_LAUNCH_CHECK: 0 or the hipError_t
template <class... P, class... A>
int launch(void (*kernel)(P...), dim3 grid, int threads, size_t lds, void* stream, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, (hipStream_t)stream, args...);
    return (int)hipGetLastError();
}

}  // namespace rpo_host
