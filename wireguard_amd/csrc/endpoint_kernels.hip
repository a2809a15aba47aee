// endpoint_kernels.hip -- the peer endpoints on device-resident tables
// (include/wgcsum.h), the row functions of wgcs_endpoint.h one lane at a time:
//   endpoint_recv_kernel          the endpoint of every slot of a receive batch   bind.go:308-319
//   SetEndpointFromPacket behind write_build, accept and finish                   peer.go:281-286
//     endpoint_set_claim_kernel   every candidate claims its peer's row
//     endpoint_set_commit_kernel  the holder, the highest candidate of its peer, stores its 64 bytes
//   Peer.Send up to bind.Send for jobs, initiations and responses                 peer.go:201-211
//     endpoint_dst_read_kernel    destination, family and status of every entry
//     endpoint_dst_clear_kernel   ClearSrc on the table rows whose flag was set
// The set and dst kernels are templated on the finder that turns an index into
// a peer row (wgcs_endpoint.h).  A recv lane walks at most a few control
// messages of its own slot in aligned words and stores one 64-byte row; a set
// or dst lane is two or three dependent loads, one 32-bit atomic and at most one
// row.  No kernel reads a clock or allocates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_endpoint.h"
#include "wgcs_kernels.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;

inline uint32_t blocks_of(uint32_t n) { return (n + kThreads - 1) / kThreads; }

__global__ __launch_bounds__(kThreads) void endpoint_recv_kernel(
    const wgcs_src_addr* __restrict__ addr, const int32_t* __restrict__ from, const int32_t* __restrict__ size,
    const uint8_t* __restrict__ oob, uint32_t oob_stride, const int32_t* __restrict__ nn, uint32_t n_msgs, uint32_t n,
    wgcs_endpoint* __restrict__ ep, wgcs_src_addr* __restrict__ addr_out) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  endpoint_recv(q, n_msgs, addr, from, size, oob, oob_stride, nn, ep, addr_out);
}

template <class Finder>
__global__ __launch_bounds__(kThreads) void endpoint_set_claim_kernel(Finder f, uint32_t n, uint32_t* claim) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  endpoint_set_claim(i, f.pick(i), claim);
}

template <class Finder>
__global__ __launch_bounds__(kThreads) void endpoint_set_commit_kernel(Finder f, uint32_t n,
                                                                       const wgcs_endpoint* __restrict__ ep,
                                                                       wgcs_endpoint* table, uint32_t* claim,
                                                                       wgcs_timers* timers) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  endpoint_set_commit(i, f.pick(i), ep, table, claim, timers);
}

// kJobs: the send jobs' form, which also writes nbufs and tx_bytes
template <class Finder, bool kJobs>
__global__ __launch_bounds__(kThreads) void endpoint_dst_read_kernel(Finder f, uint32_t n,
                                                                     const wgcs_endpoint* __restrict__ table,
                                                                     const wgcs_timers* __restrict__ timers,
                                                                     wgcs_endpoint* __restrict__ dst,
                                                                     int32_t* __restrict__ dst_v6,
                                                                     int32_t* __restrict__ dst_status, uint32_t max_segs,
                                                                     const int32_t* __restrict__ lens, int32_t* nbufs,
                                                                     uint64_t* __restrict__ tx_bytes) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint32_t row = f.row(j);
  const int32_t status = endpoint_dst_read(j, row, table, timers, dst, dst_v6, dst_status);
  if (kJobs) endpoint_dst_job(j, row, status, max_segs, lens, nbufs, tx_bytes);
}

template <class Finder>
__global__ __launch_bounds__(kThreads) void endpoint_dst_clear_kernel(Finder f, uint32_t n, wgcs_endpoint* table,
                                                                      wgcs_timers* timers) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  endpoint_dst_clear(f.row(j), table, timers);
}

template <class Finder>
hipError_t launch_set(const Finder& f, uint32_t n, const wgcs_endpoint* ep, wgcs_endpoint* table, uint32_t* claim,
                      wgcs_timers* timers, hipStream_t s) {
  hipLaunchKernelGGL(endpoint_set_claim_kernel<Finder>, dim3(blocks_of(n)), dim3(kThreads), 0, s, f, n, claim);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(endpoint_set_commit_kernel<Finder>, dim3(blocks_of(n)), dim3(kThreads), 0, s, f, n, ep, table,
                     claim, timers);
  return hipGetLastError();
}

template <class Finder, bool kJobs>
hipError_t launch_dst(const Finder& f, uint32_t n, wgcs_endpoint* table, wgcs_timers* timers, wgcs_endpoint* dst,
                      int32_t* dst_v6, int32_t* dst_status, uint32_t max_segs, const int32_t* lens, int32_t* nbufs,
                      uint64_t* tx_bytes, hipStream_t s) {
  hipLaunchKernelGGL((endpoint_dst_read_kernel<Finder, kJobs>), dim3(blocks_of(n)), dim3(kThreads), 0, s, f, n, table,
                     timers, dst, dst_v6, dst_status, max_segs, lens, nbufs, tx_bytes);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(endpoint_dst_clear_kernel<Finder>, dim3(blocks_of(n)), dim3(kThreads), 0, s, f, n, table, timers);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_endpoint_recv(const wgcs_src_addr* addr, const int32_t* from, const int32_t* size, const uint8_t* oob,
                                uint32_t oob_stride, const int32_t* nn, uint32_t n_msgs, uint32_t n, wgcs_endpoint* ep,
                                wgcs_src_addr* addr_out, hipStream_t s) {
  hipLaunchKernelGGL(endpoint_recv_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, addr, from, size, oob, oob_stride,
                     nn, n_msgs, n, ep, addr_out);
  return hipGetLastError();
}

hipError_t launch_endpoint_set_received(const EndpointReceived& f, uint32_t n, wgcs_endpoint* table, uint32_t* claim,
                                        wgcs_timers* timers, hipStream_t s) {
  return launch_set(f, n, f.ep, table, claim, timers, s);
}

hipError_t launch_endpoint_set_accepted(const EndpointAccepted& f, uint32_t n, wgcs_endpoint* table, uint32_t* claim,
                                        wgcs_timers* timers, hipStream_t s) {
  return launch_set(f, n, f.ep, table, claim, timers, s);
}

hipError_t launch_endpoint_set_finished(const EndpointFinished& f, uint32_t n, wgcs_endpoint* table, uint32_t* claim,
                                        wgcs_timers* timers, hipStream_t s) {
  return launch_set(f, n, f.ep, table, claim, timers, s);
}

hipError_t launch_endpoint_dst_jobs(const EndpointJobs& f, uint32_t n_jobs, const int32_t* lens, int32_t* nbufs,
                                    wgcs_endpoint* table, wgcs_timers* timers, wgcs_endpoint* dst, int32_t* dst_v6,
                                    int32_t* dst_status, uint64_t* tx_bytes, hipStream_t s) {
  return launch_dst<EndpointJobs, true>(f, n_jobs, table, timers, dst, dst_v6, dst_status, f.max_segs, lens, nbufs,
                                        tx_bytes, s);
}

hipError_t launch_endpoint_dst_initiated(const EndpointInitiated& f, uint32_t n, wgcs_endpoint* table,
                                         wgcs_timers* timers, wgcs_endpoint* dst, int32_t* dst_v6, int32_t* dst_status,
                                         hipStream_t s) {
  return launch_dst<EndpointInitiated, false>(f, n, table, timers, dst, dst_v6, dst_status, 0, nullptr, nullptr, nullptr,
                                              s);
}

hipError_t launch_endpoint_dst_responded(const EndpointResponded& f, uint32_t n, wgcs_endpoint* table,
                                         wgcs_timers* timers, wgcs_endpoint* dst, int32_t* dst_v6, int32_t* dst_status,
                                         hipStream_t s) {
  return launch_dst<EndpointResponded, false>(f, n, table, timers, dst, dst_v6, dst_status, 0, nullptr, nullptr,
                                              nullptr, s);
}

}  // namespace wgcs
