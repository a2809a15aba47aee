// noise_kernels.hip -- Curve25519 and the stateless part of
// ConsumeMessageInitiation on device-resident batches (include/wgcsum.h):
//   x25519_kernel       curve25519.X25519, one per row          device/noise_helpers.go:93-105
//   hs_consume_kernel   ConsumeMessageInitiation up to the replay / flood check
//                                                                device/noise.go:405-457
// One lane per row, as the handshake screen: a lane runs the Montgomery ladder
// of wgcs_x25519.h -- 255 steps of five multiplications, four squarings and
// one multiplication by a24, then the inversion, some 2,800 field
// multiplications of a hundred v_mad_u64_u32 each -- on field elements that
// are ten registers apiece, and around it the 36 BLAKE2s compressions, four
// ChaCha20 blocks and the two Poly1305 tags of wgcs_noise.h.  Nothing is
// indexed at run time.  The ladder is compute bound and the same for every
// lane of a wave (no branch depends on a key or a point); lanes part only where
// rows fail, and at the probes of the peer table, at most 15 for 16,384 peers.
// The kernel reads the arena -- the 30 aligned dwords that hold a message's
// first 116 bytes -- and never writes it, draws no randomness and reads no clock.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_noise.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void x25519_kernel(const uint32_t* __restrict__ scalars,
                                                          const uint32_t* __restrict__ points, uint32_t n,
                                                          uint32_t* __restrict__ out, int32_t* __restrict__ status) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  uint32_t k[8], u[8], r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    k[i] = scalars[8 * (uint64_t)q + i];
    u[i] = points[8 * (uint64_t)q + i];
  }
  const bool ok = x25519_words(k, u, r);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[8 * (uint64_t)q + i] = r[i];
  status[q] = ok ? WGCS_OK : WGCS_ERR_LOW_ORDER;
}

// The first 29 words of the message at p, any alignment: thirty aligned dword loads and a
// funnel shift by the pointer's low bits (the form of b2s_load_block).  The thirtieth dword
// ends at most 120 bytes into a message of 148.
__device__ __forceinline__ void load_body(const uint8_t* p, uint32_t m[kNoiseBodyWords]) {
  const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t* const w = (const uint32_t*)(p - sh);
  uint32_t d[kNoiseBodyWords + 1];
#pragma unroll
  for (uint32_t i = 0; i < kNoiseBodyWords + 1; ++i) d[i] = w[i];
#pragma unroll
  for (uint32_t i = 0; i < kNoiseBodyWords; ++i) m[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
}

__global__ __launch_bounds__(kThreads) void hs_consume_kernel(const uint8_t* __restrict__ arena,
                                                              const wgcs_aead_pkt* __restrict__ pkts,
                                                              const int32_t* __restrict__ types,
                                                              const int32_t* __restrict__ gate, uint32_t n,
                                                              const uint32_t* __restrict__ responder,
                                                              const wgcs_peer_key* __restrict__ table, uint32_t n_peers,
                                                              int32_t* __restrict__ verdict, uint32_t* __restrict__ out) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  if (types[q] != 1 || (gate && gate[q] != WGCS_HS_PASS)) {  // not an initiation, or one the screen or the rate
    verdict[q] = WGCS_HS_NONE;                               // limiter turned away: nothing else read
    return;
  }
  const wgcs_aead_pkt pk = pkts[q];
  if (pk.len != kNoiseInitiationSize) {
    verdict[q] = WGCS_ERR_INVALID_ARG;
    return;
  }
  uint32_t m[kNoiseBodyWords], priv[8], hash0[8], chain0[8], o[kHsInitWords];
  load_body(arena + pk.off, m);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    priv[i] = responder[i];
    hash0[i] = responder[8 + i];
    chain0[i] = responder[16 + i];
  }
  const int v = noise_consume_initiation(priv, hash0, chain0, table, n_peers, m, o);
  verdict[q] = v;
  if (v == WGCS_ERR_INVALID_ARG) return;  // a wrong type word: the row keeps what it held
  uint32_t* const row = out + kHsInitWords * (uint64_t)q;
#pragma unroll
  for (uint32_t i = 0; i < kHsInitWords; ++i) row[i] = o[i];
}

}  // namespace

hipError_t launch_x25519(const uint8_t* scalars, const uint8_t* points, uint32_t n, uint8_t* out, int32_t* status,
                         hipStream_t s) {
  hipLaunchKernelGGL(x25519_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s,
                     (const uint32_t*)scalars, (const uint32_t*)points, n, (uint32_t*)out, status);
  return hipGetLastError();
}

hipError_t launch_hs_consume(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types,
                             const int32_t* gate, uint32_t n, const wgcs_noise_responder* responder,
                             const wgcs_peer_key* table, uint32_t n_peers, int32_t* verdict, wgcs_hs_init* out,
                             hipStream_t s) {
  hipLaunchKernelGGL(hs_consume_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, arena, pkts, types,
                     gate, n, (const uint32_t*)responder, table, n_peers, verdict, (uint32_t*)out);
  return hipGetLastError();
}

}  // namespace wgcs
