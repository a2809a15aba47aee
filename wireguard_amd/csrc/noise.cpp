// noise.cpp -- the host functions of the handshake's consume and response steps
// (include/wgcsum.h), no context and no device:
//   wgcs_x25519                      curve25519.X25519              device/noise_helpers.go:93-105
//   wgcs_noise_responder_init        d.keys and the first mixHash   device/noise.go:91-94, :415
//   wgcs_peer_keys_build / _find     GetPeer and precomputedSharedSecret   :305, :432
//   wgcs_noise_consume_initiation    ConsumeMessageInitiation       :405-457
//   wgcs_noise_create_initiation     CreateMessageInitiation        :344-403
//   wgcs_noise_create_response       CreateMessageResponse, AddMACs and the responder's keys
//                                                                   :494-546, :646-651, cookie.go:287-314
//   wgcs_noise_consume_response      ConsumeMessageResponse and the initiator's keys   :548-620, :638-643
//   wgcs_handshake_initiate_host     wgcs_handshake_initiate_batch on host memory, row by row
//   wgcs_handshake_finish_host       wgcs_handshake_finish_batch on host memory, in its two passes
//   wgcs_peer_rows_build             peer id -> row of the peer table
//   wgcs_handshake_accept_host       wgcs_handshake_accept_batch on host memory, in its passes   :458-491
// They run the scalar code of wgcs_x25519.h and wgcs_noise.h, the code the
// lanes of noise_kernels.hip, noise_init_kernels.hip and noise_accept_kernels.hip
// run.  Plain C++: the host test programs (tests/noise_host/noise_host.cpp,
// tests/noise_resp_host/noise_resp_host.cpp, tests/noise_init_host/noise_init_host.cpp,
// tests/noise_accept_host/noise_accept_host.cpp) link this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_noise.h"

using namespace wgcs;

namespace {

const char kNoiseConstruction[] = "Noise_IKpsk2_25519_ChaChaPoly_BLAKE2s";  // noise.go:43
const char kWGIdentifier[] = "WireGuard v1 zx2c4 Jason@zx2c4.com";          // :44

void words_of(const uint8_t* p, uint32_t n_words, uint32_t* w) {
  for (uint32_t i = 0; i < n_words; ++i) w[i] = b2s_load_le32(p, 4 * i, 4 * n_words);
}

void bytes_of(const uint32_t* w, uint32_t n_words, uint8_t* p) {
  for (uint32_t i = 0; i < n_words; ++i) b2s_store_le32(p + 4 * i, w[i]);
}

// InitialChainKey and InitialHash of init() (noise.go:91-94)
void initial(uint8_t chain[32], uint8_t hash[32]) {
  blake2s_bytes(nullptr, 0, (const uint8_t*)kNoiseConstruction, sizeof kNoiseConstruction - 1, 32, chain);
  uint8_t in[32 + sizeof kWGIdentifier - 1];
  memcpy(in, chain, 32);
  memcpy(in + 32, kWGIdentifier, sizeof kWGIdentifier - 1);
  blake2s_bytes(nullptr, 0, in, sizeof in, 32, hash);
}

// mixHash(InitialHash, pub) and InitialChainKey: where both sides start for the static key pub (:358, :415)
void start_of(const uint32_t pub[8], uint32_t hash0[8], uint32_t chain0[8]) {
  uint8_t chain[32], hash[32];
  initial(chain, hash);
  words_of(chain, 8, chain0);
  words_of(hash, 8, hash0);
  const uint32_t data[12] = {pub[0], pub[1], pub[2], pub[3], pub[4], pub[5], pub[6], pub[7], 0, 0, 0, 0};
  noise_mix_hash(hash0, data, 32);
}

const uint32_t kBasePoint[8] = {9, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

extern "C" {

int wgcs_x25519(uint8_t out[32], const uint8_t scalar[32], const uint8_t point[32]) {
  if (!out || !scalar || !point) return WGCS_ERR_INVALID_ARG;
  uint32_t k[8], u[8], r[8];
  words_of(scalar, 8, k);
  words_of(point, 8, u);
  const bool ok = x25519_words(k, u, r);
  bytes_of(r, 8, out);
  return ok ? WGCS_OK : WGCS_ERR_LOW_ORDER;
}

int wgcs_noise_responder_init(wgcs_noise_responder* r, const uint8_t private_key[32], uint8_t public_key[32]) {
  if (!r || !private_key) return WGCS_ERR_INVALID_ARG;
  uint32_t k[8], pub[8], hash0[8], chain0[8];
  words_of(private_key, 8, k);
  x25519_words(k, kBasePoint, pub);  // publicKey(), noise_helpers.go:83-89
  start_of(pub, hash0, chain0);
  memmove(r->private_key, private_key, 32);
  bytes_of(hash0, 8, r->hash0);
  bytes_of(chain0, 8, r->chain0);
  if (public_key) bytes_of(pub, 8, public_key);
  return WGCS_OK;
}

int wgcs_peer_keys_build(const wgcs_noise_responder* r, const uint8_t* public_keys, const uint32_t* peers,
                         const uint32_t* flags, uint32_t n, wgcs_peer_key* table) {
  if (n == 0) return WGCS_OK;
  if (!r || !public_keys || !peers || !table) return WGCS_ERR_INVALID_ARG;
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) {
    if (peers[i] == WGCS_PEER_NONE) return WGCS_ERR_INVALID_ARG;
    order[i] = i;
  }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return memcmp(public_keys + 32 * (size_t)a, public_keys + 32 * (size_t)b, 32) < 0;
  });
  for (uint32_t i = 1; i < n; ++i)
    if (memcmp(public_keys + 32 * (size_t)order[i - 1], public_keys + 32 * (size_t)order[i], 32) == 0)
      return WGCS_ERR_INVALID_ARG;
  uint32_t k[8];
  words_of(r->private_key, 8, k);
  for (uint32_t i = 0; i < n; ++i) {
    const uint8_t* const pub = public_keys + 32 * (size_t)order[i];
    uint32_t u[8], shared[8];
    words_of(pub, 8, u);
    x25519_words(k, u, shared);  // all zero where the key is a low-order point: the row never authenticates
    wgcs_peer_key* const row = table + i;
    memcpy(row->public_key, pub, 32);
    bytes_of(shared, 8, row->shared);
    row->peer = peers[order[i]];
    row->flags = flags ? flags[order[i]] : WGCS_PEER_RUNNING;
  }
  return WGCS_OK;
}

int wgcs_peer_keys_find(const wgcs_peer_key* table, uint32_t n, const uint8_t public_key[32]) {
  if (!public_key || (n && !table)) return -1;
  uint32_t key[8];
  words_of(public_key, 8, key);
  return noise_find_peer(table, n, key);
}

int wgcs_noise_consume_initiation(const wgcs_noise_responder* r, const wgcs_peer_key* table, uint32_t n_peers,
                                  const uint8_t* msg, size_t len, wgcs_hs_init* out) {
  if (!r || !msg || !out || (n_peers && !table) || len != kNoiseInitiationSize) return WGCS_ERR_INVALID_ARG;
  uint32_t k[8], hash0[8], chain0[8], m[kNoiseBodyWords], o[kHsInitWords];
  words_of(r->private_key, 8, k);
  words_of(r->hash0, 8, hash0);
  words_of(r->chain0, 8, chain0);
  words_of(msg, kNoiseBodyWords, m);
  const int verdict = noise_consume_initiation(k, hash0, chain0, table, n_peers, m, o);
  if (verdict == WGCS_ERR_INVALID_ARG) return verdict;
  out->peer = o[0];
  out->sender = o[1];
  bytes_of(o + 2, 3, out->timestamp);
  bytes_of(o + 5, 3, out->pad);
  bytes_of(o + 8, 8, out->hash);
  bytes_of(o + 16, 8, out->chain_key);
  bytes_of(o + 24, 8, out->ephemeral);
  return verdict;
}

int wgcs_noise_create_initiation(const uint8_t static_private[32], const uint8_t remote_static[32],
                                 const uint8_t ephemeral_private[32], const uint8_t timestamp[12], uint32_t sender,
                                 uint8_t msg[148], uint8_t hash[32], uint8_t chain_key[32]) {
  if (!static_private || !remote_static || !ephemeral_private || !timestamp || !msg) return WGCS_ERR_INVALID_ARG;
  uint32_t sk[8], spub[8], remote[8], ek[8], ts[3], hash0[8], chain0[8], m[37], h[8], c[8];
  words_of(static_private, 8, sk);
  words_of(remote_static, 8, remote);
  words_of(ephemeral_private, 8, ek);
  words_of(timestamp, 3, ts);
  x25519_words(sk, kBasePoint, spub);  // d.keys.publicKey
  start_of(remote, hash0, chain0);
  const int rc = noise_create_initiation(sk, spub, remote, hash0, chain0, ek, ts, sender, m, h, c);
  if (rc != WGCS_OK) {
    memset(msg, 0, kNoiseInitiationSize);
    return rc;
  }
  bytes_of(m, 37, msg);
  if (hash) bytes_of(h, 8, hash);
  if (chain_key) bytes_of(c, 8, chain_key);
  return WGCS_OK;
}

int wgcs_noise_create_response(const wgcs_hs_init* init, const uint8_t remote_static[32],
                               const uint8_t preshared_key[32], const uint8_t ephemeral_private[32],
                               uint32_t local_index, const uint8_t cookie[16], uint8_t msg[92], uint8_t send_key[32],
                               uint8_t recv_key[32]) {
  if (!init || !remote_static || !ephemeral_private || !msg) return WGCS_ERR_INVALID_ARG;
  uint32_t h[8], c[8], reph[8], remote[8], psk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ek[8], ck[4] = {0, 0, 0, 0};
  uint32_t m[kNoiseResponseBodyWords], send[8], recv[8], mac1_key[8];
  words_of(init->hash, 8, h);
  words_of(init->chain_key, 8, c);
  words_of(init->ephemeral, 8, reph);
  words_of(remote_static, 8, remote);
  words_of(ephemeral_private, 8, ek);
  if (preshared_key) words_of(preshared_key, 8, psk);
  if (cookie) words_of(cookie, 4, ck);
  const int rc = noise_create_response(h, c, reph, remote, psk, ek, local_index, init->sender, m, send, recv);
  if (send_key) bytes_of(send, 8, send_key);  // zero where rc is not WGCS_OK
  if (recv_key) bytes_of(recv, 8, recv_key);
  if (rc != WGCS_OK) {
    memset(msg, 0, kNoiseResponseSize);
    return rc;
  }
  noise_mac1_key(remote, mac1_key);
  noise_write_response(msg, m, mac1_key, cookie != nullptr, ck);
  return WGCS_OK;
}

int wgcs_noise_consume_response(const uint8_t static_private[32], const uint8_t hash[32], const uint8_t chain_key[32],
                                const uint8_t ephemeral_private[32], const uint8_t preshared_key[32],
                                uint32_t local_index, const uint8_t* msg, size_t len, uint32_t* sender,
                                uint8_t send_key[32], uint8_t recv_key[32]) {
  uint32_t sk[8], h[8], c[8], ek[8], psk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m[kNoiseResponseBodyWords];
  uint32_t send[8] = {0, 0, 0, 0, 0, 0, 0, 0}, recv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, from = 0;
  int rc = WGCS_ERR_INVALID_ARG;
  if (static_private && hash && chain_key && ephemeral_private && msg && len == kNoiseResponseSize) {
    words_of(static_private, 8, sk);
    words_of(hash, 8, h);
    words_of(chain_key, 8, c);
    words_of(ephemeral_private, 8, ek);
    if (preshared_key) words_of(preshared_key, 8, psk);
    words_of(msg, kNoiseResponseBodyWords, m);
    rc = noise_consume_response(sk, h, c, ek, psk, local_index, m, &from, send, recv);
  }
  if (send_key) bytes_of(send, 8, send_key);
  if (recv_key) bytes_of(recv, 8, recv_key);
  if (rc == WGCS_OK && sender) *sender = from;
  return rc;
}

int wgcs_handshake_initiate_host(const wgcs_hs_start* start, uint32_t n, const uint8_t* static_public,
                                 const wgcs_peer_key* table, uint32_t n_peers, uint32_t n_keys, wgcs_hs_state* states,
                                 uint32_t n_states, uint8_t* msgs, int32_t* status) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !start || !static_public || !msgs || !status || (n_peers && !table) || (n_states && !states))
    return WGCS_ERR_INVALID_ARG;
  for (uint32_t q = 0; q < n; ++q)
    status[q] = noise_initiate_row(start + q, static_public, table, n_peers, n_keys, states, n_states,
                                   msgs + kNoiseInitiationPitch * (size_t)q);
  return WGCS_OK;
}

int wgcs_handshake_finish_host(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* type,
                               const int32_t* gate, uint32_t n, const wgcs_noise_responder* responder,
                               const wgcs_session_slot* slots, uint32_t n_slots, wgcs_hs_state* states,
                               uint32_t n_states, const uint8_t* psk, uint32_t n_peers, wgcs_aead_key* keys,
                               uint32_t n_keys, uint8_t* work, int32_t* verdict) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || (n_slots & (n_slots - 1)) || !arena || !pkts || !type || !responder || !work || !verdict ||
      gate == verdict || (n_slots && !slots) || (n_states && !states) || (n_keys && !keys))
    return WGCS_ERR_INVALID_ARG;
  // the two launches of the device form, each a loop: every row sees the states as they stood at the call
  for (uint32_t q = 0; q < n; ++q)
    verdict[q] = noise_finish_row(q, arena, pkts, type, gate, responder, slots, n_slots, states, n_states, psk, n_peers,
                                  n_keys, work);
  for (uint32_t q = 0; q < n; ++q)
    verdict[q] = noise_finish_commit(q, verdict[q], arena, pkts, slots, n_slots, states, keys, work);
  return WGCS_OK;
}

int wgcs_peer_rows_build(const wgcs_peer_key* table, uint32_t n, uint32_t* rows, uint32_t n_ids) {
  if ((n && !table) || (n_ids && !rows)) return WGCS_ERR_INVALID_ARG;
  for (uint32_t i = 0; i < n; ++i)
    if (table[i].peer >= n_ids) return WGCS_ERR_INVALID_ARG;
  for (uint32_t id = 0; id < n_ids; ++id) rows[id] = WGCS_PEER_NONE;
  for (uint32_t i = n; i-- > 0;) rows[table[i].peer] = i;  // a duplicated id keeps its lowest row
  return WGCS_OK;
}

int wgcs_handshake_accept_host(const wgcs_hs_init* init, const int32_t* gate, uint32_t n, int64_t now_ns,
                               const wgcs_peer_key* table, const uint32_t* peer_rows, uint32_t n_ids,
                               wgcs_hs_peer* peers, uint32_t n_peers, const wgcs_hs_ticket* tickets,
                               uint32_t n_tickets, wgcs_hs_resp* resp, uint32_t* count, int32_t* verdict) {
  if (!count || (n && (!init || !gate || !verdict)) || (n_tickets && (!tickets || !resp)) ||
      (n && n_peers && (!table || !peers)) || (n && n_ids && !peer_rows) || (n && (const int32_t*)verdict == gate) ||
      n > kMaxRows || n_tickets > kMaxRows)
    return WGCS_ERR_INVALID_ARG;
  // the passes of the device form, each a loop: every row sees the peer rows as they stood at the call
  for (uint32_t q = 0; q < n; ++q)
    verdict[q] = noise_accept_claim(q, init, gate, now_ns, table, peer_rows, n_ids, peers, n_peers);
  for (uint32_t q = 0; q < n; ++q) verdict[q] = noise_accept_verdict(q, verdict[q], init, n, peer_rows, peers);
  uint32_t winners = 0;  // the device form's scan: the winners in the rows below q
  for (uint32_t q = 0; q < n; ++q)
    if (verdict[q] == WGCS_HS_ACCEPTED && gate[q] == WGCS_HS_CONSUMED)  // not a verdict passed through
      verdict[q] = noise_accept_commit(q, winners++, now_ns, init, peer_rows, peers, tickets, n_tickets, resp);
  *count = winners < n_tickets ? winners : n_tickets;
  for (uint32_t j = *count; j < n_tickets; ++j) noise_accept_tail(resp + j);
  return WGCS_OK;
}

}  // extern "C"
