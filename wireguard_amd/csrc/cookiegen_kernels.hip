// cookiegen_kernels.hip -- the initiator's side of the cookie mechanism on
// device-resident tables (include/wgcsum.h), the row functions of
// wgcs_cookiegen.h one lane at a time:
//   lastMAC1 behind initiate and respond                        cookie.go:301-302
//     cookie_sent_claim_kernel    every descriptor that takes part claims its peer's row
//     cookie_sent_commit_kernel   the holder, the highest descriptor of its peer, stores its MAC1
//   cookie replies over a receive batch                         receive.go:246-269, cookie.go:319-339
//     cookie_open_kernel          lookup, XChaCha20-Poly1305 open, the cookie into d_work, the claim
//     cookie_commit_kernel        the holder stores cookie, bit and time; d_work is zeroed
//   cookie_age_kernel             CookieRefreshTime over the peer rows   cookie.go:306
// An open lane is two dependent slot probes, one HChaCha20, two ChaCha20 blocks
// and a three-block Poly1305 on registers (wgcs_xchacha.h: nothing is indexed
// at run time), 64 bytes in -- replies sit at any offset; b2s_load_block reads
// the aligned dwords that hold them -- and 16 bytes out.  The kernels read the
// arena and never write it, draw no randomness and read no clock.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_cookiegen.h"
#include "wgcs_kernels.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;

inline uint32_t blocks_of(uint32_t n) { return (n + kThreads - 1) / kThreads; }

// kResponded: descriptors of wgcs_handshake_respond_batch, else of wgcs_handshake_initiate_batch
template <bool kResponded>
__device__ __forceinline__ uint32_t sent_row(uint32_t j, const void* desc, const int32_t* status, uint32_t n_peers) {
  return kResponded ? cookiegen_responded_row(j, (const wgcs_hs_resp*)desc, status, n_peers)
                    : cookiegen_initiated_row(j, (const wgcs_hs_start*)desc, status, n_peers);
}

template <bool kResponded>
__global__ __launch_bounds__(kThreads) void cookie_sent_claim_kernel(const void* __restrict__ desc,
                                                                     const int32_t* __restrict__ status, uint32_t n,
                                                                     wgcs_cookie_gen* gen, uint32_t n_peers) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  cookiegen_sent_claim(j, sent_row<kResponded>(j, desc, status, n_peers), gen);
}

template <bool kResponded>
__global__ __launch_bounds__(kThreads) void cookie_sent_commit_kernel(const void* __restrict__ desc,
                                                                      const int32_t* __restrict__ status,
                                                                      const uint8_t* __restrict__ msgs, uint32_t n,
                                                                      wgcs_cookie_gen* gen, uint32_t n_peers) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  cookiegen_sent_commit(j, sent_row<kResponded>(j, desc, status, n_peers),
                        kResponded ? cookiegen_responded_mac1(j, msgs) : cookiegen_initiated_mac1(j, msgs), gen);
}

__global__ __launch_bounds__(kThreads) void cookie_open_kernel(const uint8_t* __restrict__ arena,
                                                               const wgcs_aead_pkt* __restrict__ pkts,
                                                               const int32_t* __restrict__ types, uint32_t n,
                                                               CookieGenTables t, wgcs_cookie_gen* gen,
                                                               uint32_t* __restrict__ work,
                                                               int32_t* __restrict__ verdict) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  verdict[q] = cookiegen_open(q, arena, pkts, types, t, gen, work);
}

__global__ __launch_bounds__(kThreads) void cookie_commit_kernel(const uint8_t* __restrict__ arena,
                                                                 const wgcs_aead_pkt* __restrict__ pkts,
                                                                 const int32_t* __restrict__ verdict, uint32_t n,
                                                                 CookieGenTables t, int64_t now, wgcs_cookie_gen* gen,
                                                                 wgcs_hs_peer* peers, uint32_t* work) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  cookiegen_commit(q, arena, pkts, verdict, t, now, gen, peers, work);
}

__global__ __launch_bounds__(kThreads) void cookie_age_kernel(int64_t now, const wgcs_cookie_gen* __restrict__ gen,
                                                              wgcs_hs_peer* peers, uint32_t n_peers) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= n_peers) return;
  cookiegen_age(r, now, gen, peers);
}

template <bool kResponded>
hipError_t launch_sent(const void* desc, const int32_t* status, const uint8_t* msgs, uint32_t n, wgcs_cookie_gen* gen,
                       uint32_t n_peers, hipStream_t s) {
  hipLaunchKernelGGL(cookie_sent_claim_kernel<kResponded>, dim3(blocks_of(n)), dim3(kThreads), 0, s, desc, status, n,
                     gen, n_peers);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cookie_sent_commit_kernel<kResponded>, dim3(blocks_of(n)), dim3(kThreads), 0, s, desc, status,
                     msgs, n, gen, n_peers);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_cookie_initiated(const wgcs_hs_start* start, const int32_t* status, const uint8_t* msgs, uint32_t n,
                                   wgcs_cookie_gen* gen, uint32_t n_peers, hipStream_t s) {
  return launch_sent<false>(start, status, msgs, n, gen, n_peers, s);
}

hipError_t launch_cookie_responded(const wgcs_hs_resp* resp, const int32_t* status, const uint8_t* msgs, uint32_t n,
                                   wgcs_cookie_gen* gen, uint32_t n_peers, hipStream_t s) {
  return launch_sent<true>(resp, status, msgs, n, gen, n_peers, s);
}

hipError_t launch_cookie_consume(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types, uint32_t n,
                                 int64_t now, const CookieGenTables& t, wgcs_cookie_gen* gen, wgcs_hs_peer* peers,
                                 uint32_t* work, int32_t* verdict, hipStream_t s) {
  hipLaunchKernelGGL(cookie_open_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, arena, pkts, types, n, t, gen, work,
                     verdict);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cookie_commit_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, arena, pkts, verdict, n, t, now,
                     gen, peers, work);
  return hipGetLastError();
}

hipError_t launch_cookie_age(int64_t now, const wgcs_cookie_gen* gen, wgcs_hs_peer* peers, uint32_t n_peers,
                             hipStream_t s) {
  hipLaunchKernelGGL(cookie_age_kernel, dim3(blocks_of(n_peers)), dim3(kThreads), 0, s, now, gen, peers, n_peers);
  return hipGetLastError();
}

}  // namespace wgcs
