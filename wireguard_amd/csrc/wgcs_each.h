// wgcs_each.h -- one lane per entry: the kernel and the launcher of every call whose rows are
// independent but for the atomics of their bodies.  A body is a struct of the call's arrays and
// scalars with operator()(uint32_t i) (wgcs_timers.h, wgcs_rekey.h, wgcs_cookiegen.h,
// wgcs_endpoint.h); the host forms run the same body in a plain loop.  A two-pass call is two
// bodies over one source and two launches on one stream, which orders them: the second pass sees
// every claim of the first.  n is not 0.
//
// The .hip file of a family includes this text and instantiates launch_each once per body; the
// entry points see the declarations of wgcs_kernels.h alone.  A kernel that ends in a block-wide
// helper (wgcs_compact.h) is no body: a lane past n returns here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wgcs_kernels.h"

namespace wgcs {

constexpr int kEachThreads = 256;

#ifdef __HIPCC__

template <class F>
__global__ __launch_bounds__(kEachThreads) void each_kernel(F f, uint32_t n) {
  const uint32_t i = blockIdx.x * kEachThreads + threadIdx.x;
  if (i < n) f(i);
}

template <class F>
hipError_t launch_each(const F& f, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(each_kernel<F>, dim3((n + kEachThreads - 1) / kEachThreads), dim3(kEachThreads), 0, s, f, n);
  return hipGetLastError();
}

template <class F, class G>
hipError_t launch_each(const F& first, const G& second, uint32_t n, hipStream_t s) {
  const hipError_t e = launch_each(first, n, s);
  return e != hipSuccess ? e : launch_each(second, n, s);
}

#endif  // __HIPCC__

}  // namespace wgcs
