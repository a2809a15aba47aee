// noise_kernels.hip -- Curve25519 and the stateless part of
// ConsumeMessageInitiation on device-resident batches (include/wgcsum.h):
//   x25519_kernel       curve25519.X25519, one per row          device/noise_helpers.go:93-105
//   hs_consume_kernel   ConsumeMessageInitiation up to the replay / flood check
//                                                                device/noise.go:405-457
//   hs_respond_kernel   CreateMessageResponse, AddMACs and the responder's session keys
//                                                                device/noise.go:494-546, :646-651
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

// The words of wgcs_hs_resp: 0 init_row | 1 peer_row | 2 local_index | 3 send_key | 4 recv_key | 5 flags |
// 6..7 pad | 8..15 ephemeral private | 16..19 cookie.
constexpr uint32_t kHsRespWords = sizeof(wgcs_hs_resp) / 4;
constexpr uint32_t kPeerKeyWords = sizeof(wgcs_peer_key) / 4;  // 0..7 public key | 8..15 shared | 16 peer | 17 flags
constexpr uint32_t kAeadKeyWords = sizeof(wgcs_aead_key) / 4;  // 0..7 key | 8 remote_index | 9..11 pad
constexpr uint32_t kRespPitchWords = 24;                       // a row of d_msgs: the 92 bytes and 4 of zero

// One descriptor per lane: noise_create_response, AddMACs and both key rows.  The three
// scalar multiplications share one ladder inside noise_create_response, so the kernel holds
// the registers of hs_consume_kernel and not three times its code.  Every load and store is
// an aligned dword; the lane reads its own d_msgs row back for the two MACs.
__global__ __launch_bounds__(kThreads) void hs_respond_kernel(const uint32_t* __restrict__ resp, uint32_t n,
                                                              const uint32_t* __restrict__ init,
                                                              const int32_t* __restrict__ gate, uint32_t n_init,
                                                              const uint32_t* __restrict__ table,
                                                              const uint32_t* __restrict__ psk_table, uint32_t n_peers,
                                                              uint32_t* keys, uint32_t n_keys, uint8_t* msgs,
                                                              int32_t* __restrict__ status) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  const uint32_t* const d = resp + kHsRespWords * (uint64_t)q;
  const uint32_t init_row = d[0], peer_row = d[1], local_index = d[2], send_row = d[3], recv_row = d[4], flags = d[5];
  if (init_row >= n_init || peer_row >= n_peers || send_row >= n_keys || recv_row >= n_keys || send_row == recv_row) {
    status[q] = WGCS_ERR_INVALID_ARG;
    return;
  }
  if (gate && gate[init_row] != WGCS_HS_CONSUMED) {  // the host's timestamp or flood rule masked it
    status[q] = WGCS_HS_NONE;
    return;
  }
  const uint32_t* const in = init + kHsInitWords * (uint64_t)init_row;
  const uint32_t* const peer = table + kPeerKeyWords * (uint64_t)peer_row;
  if (in[0] != peer[16]) {  // not the peer this initiation authenticated as
    status[q] = WGCS_ERR_NO_PEER;
    return;
  }
  uint32_t hash0[8], chain0[8], remote_eph[8], remote_static[8], psk[8], eph_priv[8], cookie[4];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash0[i] = in[8 + i];
    chain0[i] = in[16 + i];
    remote_eph[i] = in[24 + i];
    remote_static[i] = peer[i];
    psk[i] = psk_table ? psk_table[8 * (uint64_t)peer_row + i] : 0u;
    eph_priv[i] = d[8 + i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) cookie[i] = d[16 + i];
  uint32_t m[kNoiseResponseBodyWords], send_key[8], recv_key[8];
  const int rc = noise_create_response(hash0, chain0, remote_eph, remote_static, psk, eph_priv, local_index, in[1], m,
                                       send_key, recv_key);
  uint8_t* const row = msgs + 4 * kRespPitchWords * (uint64_t)q;
  if (rc != WGCS_OK) {  // a zero shared secret: no key row is touched
#pragma unroll
    for (uint32_t i = 0; i < kRespPitchWords; ++i) ((uint32_t*)row)[i] = 0;
    status[q] = rc;
    return;
  }
  uint32_t mac1_key[8];
  noise_mac1_key(remote_static, mac1_key);
  noise_write_response(row, m, mac1_key, (flags & WGCS_HS_RESP_COOKIE) != 0, cookie);
  ((uint32_t*)row)[kRespPitchWords - 1] = 0;
  uint32_t* const ks = keys + kAeadKeyWords * (uint64_t)send_row;
  uint32_t* const kr = keys + kAeadKeyWords * (uint64_t)recv_row;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ks[i] = send_key[i];
    kr[i] = recv_key[i];
  }
  ks[8] = in[1];  // the receiver index of every transport message sealed under this key
  kr[8] = 0;
#pragma unroll
  for (int i = 9; i < 12; ++i) ks[i] = kr[i] = 0;
  status[q] = WGCS_HS_RESPONDED;
}

}  // namespace

hipError_t launch_hs_respond(const wgcs_hs_resp* resp, uint32_t n, const wgcs_hs_init* init, const int32_t* gate,
                             uint32_t n_init, const wgcs_peer_key* table, const uint8_t* psk, uint32_t n_peers,
                             wgcs_aead_key* keys, uint32_t n_keys, uint8_t* msgs, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(hs_respond_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s,
                     (const uint32_t*)resp, n, (const uint32_t*)init, gate, n_init, (const uint32_t*)table,
                     (const uint32_t*)psk, n_peers, (uint32_t*)keys, n_keys, msgs, status);
  return hipGetLastError();
}

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
