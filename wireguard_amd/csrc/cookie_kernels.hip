// cookie_kernels.hip -- the denial-of-service screen at the top of
// RoutineHandshake on device-resident batches (include/wgcsum.h):
//   hs_screen_kernel   CheckMAC1, and under load CheckMAC2 and the cookie
//                      reply of SendHandshakeCookie
//                      device/receive.go:270-287, device/cookie.go:121-243, device/send.go:176-187
// One lane per message, as the route kernels: an initiation under load is
// nine BLAKE2s compressions and three ChaCha20 permutations on registers
// (wgcs_blake2s.h, wgcs_xchacha.h: nothing is indexed at run time), 148 bytes
// in -- messages sit at any offset; b2s_load_block reads the aligned dwords
// that hold them -- and 64 bytes out.  The kernel reads the arena and never
// writes it, draws no randomness and reads no clock: the secret and the reply
// nonces are the caller's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_cookie.h"
#include "wgcs_kernels.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kInitiationSize = 148, kResponseSize = 92;  // device/noise.go:63-66

__global__ __launch_bounds__(kThreads) void hs_screen_kernel(const uint8_t* __restrict__ arena,
                                                             const wgcs_aead_pkt* __restrict__ pkts,
                                                             const int32_t* __restrict__ types, uint32_t n,
                                                             const uint32_t* __restrict__ checker,
                                                             const wgcs_src_addr* __restrict__ srcs, uint32_t under_load,
                                                             const uint32_t* __restrict__ nonces,
                                                             int32_t* __restrict__ verdict,
                                                             uint32_t* __restrict__ replies) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  const int32_t type = types[q];
  if (type != 1 && type != 2) {  // transport, cookie replies, everything classify refused: not ours, nothing read
    verdict[q] = WGCS_HS_NONE;
    return;
  }
  const wgcs_aead_pkt pk = pkts[q];
  const uint32_t len = pk.len;
  if (len != (type == 1 ? kInitiationSize : kResponseSize)) {
    verdict[q] = WGCS_ERR_INVALID_ARG;
    return;
  }
  const uint8_t* const msg = arena + pk.off;
  uint32_t key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = checker[i];  // mac1_key
  if (!cookie_mac1_ok(key, msg, len)) {  // receive.go:272-275
    verdict[q] = WGCS_ERR_MAC1;
    return;
  }
  if (!under_load) {  // :280: MAC2 is looked at under load only
    verdict[q] = WGCS_HS_PASS;
    return;
  }
  const wgcs_src_addr* const src = srcs + q;
  const uint32_t src_len = src->len;
  if (src_len != 6 && src_len != 18) {
    verdict[q] = WGCS_ERR_INVALID_ARG;
    return;
  }
  uint32_t cookie[4];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = checker[16 + i];  // secret
  cookie_of_source(key, src->b, src_len, cookie);
  if (cookie_mac2_ok(cookie, msg, len)) {  // :281: the host's rate limiter is next
    verdict[q] = WGCS_HS_PASS;
    return;
  }
  // :282-284: SendHandshakeCookie
  uint32_t nonce[6], reply[16];
#pragma unroll
  for (int i = 0; i < 6; ++i) nonce[i] = nonces[6 * (uint64_t)q + i];
#pragma unroll
  for (int i = 0; i < 8; ++i) key[i] = checker[8 + i];  // cookie_key
  cookie_reply_words(key, cookie, msg, len, nonce, reply);
  uint32_t* const out = replies + 16 * (uint64_t)q;
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = reply[i];
  verdict[q] = WGCS_HS_COOKIE;
}

}  // namespace

hipError_t launch_hs_screen(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types, uint32_t n,
                            const wgcs_cookie_checker* checker, const wgcs_src_addr* srcs, uint32_t under_load,
                            const uint8_t* nonces, int32_t* verdict, uint8_t* replies, hipStream_t s) {
  hipLaunchKernelGGL(hs_screen_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, arena, pkts, types, n,
                     (const uint32_t*)checker, srcs, under_load, (const uint32_t*)nonces, verdict, (uint32_t*)replies);
  return hipGetLastError();
}

}  // namespace wgcs
