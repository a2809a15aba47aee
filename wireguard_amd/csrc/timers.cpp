// timers.cpp -- the peer timers on host memory (include/wgcsum.h), no context
// and no device:
//   wgcs_timers_jitter_ms         rand.Int64N(RekeyTimeoutJitterMaxMs) from a seed and a row
//   wgcs_timers_sent_host         device/send.go:498-510
//   wgcs_timers_received_host     device/receive.go:486-494
//   wgcs_timers_initiated_host    send.go:85-87, :117-126
//   wgcs_timers_responded_host    receive.go:311-312, send.go:158-160
//   wgcs_timers_finished_host     receive.go:339-348
//   wgcs_timers_rotated_host      receive.go:422-427
//   wgcs_timers_expire_host       device/timers.go:73-144, in the passes of the device form
// They run the bodies and row functions of wgcs_timers.h, the code the lanes of
// the device forms run, taken in row order.  Plain C++: the host test program
// (tests/timers_host/timers_host.cpp) links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_timers.h"

using namespace wgcs;

namespace {

// a table of n_peers rows and the id -> row map in front of it
inline bool rows_ok(const uint32_t* peer_rows, uint32_t n_ids, const void* table, uint32_t n_peers) {
  return (!n_ids || peer_rows) && (!n_peers || table) && n_peers <= kMaxPeers;
}

}  // namespace

extern "C" {

uint32_t wgcs_timers_jitter_ms(uint32_t seed, uint32_t row) { return timers_jitter_ms(seed, row); }

int wgcs_timers_sent_host(const int32_t* sizes, const uint32_t* peer, const int32_t* count, const int32_t* status,
                          const uint32_t* job_key, uint32_t n_jobs, uint32_t max_segs, int64_t now_ns,
                          uint32_t jitter_seed, const uint32_t* peer_rows, uint32_t n_ids, wgcs_timers* timers,
                          uint32_t n_peers) {
  if (n_jobs == 0) return WGCS_OK;
  if (!sizes || !peer || !count || !status || !job_key || max_segs == 0 || (uint64_t)n_jobs * max_segs > kMaxRows ||
      !rows_ok(peer_rows, n_ids, timers, n_peers))
    return WGCS_ERR_INVALID_ARG;
  const TimersSent body = {{{peer, count, status, max_segs, peer_rows, n_ids, n_peers}, job_key}, sizes, now_ns,
                           jitter_seed, timers};
  for (uint32_t j = 0; j < n_jobs; ++j) body(j);
  return WGCS_OK;
}

int wgcs_timers_received_host(const wgcs_write_group* groups, uint32_t n_batches, uint32_t calls_per_batch,
                              int64_t now_ns, const uint32_t* peer_rows, uint32_t n_ids, wgcs_timers* timers,
                              uint32_t n_peers) {
  const uint64_t n = (uint64_t)n_batches * calls_per_batch;
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !groups || !rows_ok(peer_rows, n_ids, timers, n_peers)) return WGCS_ERR_INVALID_ARG;
  const TimersReceived body = {{groups, peer_rows, n_ids, n_peers}, now_ns, timers};
  for (uint32_t c = 0; c < (uint32_t)n; ++c) body(c);
  return WGCS_OK;
}

int wgcs_timers_initiated_host(const uint32_t* reasons, const uint32_t* start_peer, const int32_t* init_status,
                               uint32_t n_tickets, int64_t now_ns, uint32_t jitter_seed, wgcs_timers* timers,
                               uint32_t n_peers) {
  if (n_peers == 0) return WGCS_OK;  // no row to write
  if (n_peers > kMaxPeers || n_tickets > kMaxRows || !reasons || !timers ||
      (n_tickets && (!start_peer || !init_status)))
    return WGCS_ERR_INVALID_ARG;
  // the launches of the device form, each a loop: the peer rows, then the tickets
  const TimersFresh fresh = {reasons, timers};
  const TimersInitiated body = {{start_peer, init_status, n_peers}, now_ns, jitter_seed, timers};
  for (uint32_t r = 0; r < n_peers; ++r) fresh(r);
  for (uint32_t k = 0; k < n_tickets; ++k) body(k);
  return WGCS_OK;
}

int wgcs_timers_responded_host(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t n, int64_t now_ns,
                               wgcs_timers* timers, uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || n_peers > kMaxPeers || !resp || !gate || (n_peers && !timers)) return WGCS_ERR_INVALID_ARG;
  const TimersResponded body = {{resp, gate, n_peers}, now_ns, timers};
  for (uint32_t j = 0; j < n; ++j) body(j);
  return WGCS_OK;
}

int wgcs_timers_finished_host(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* gate,
                              const int32_t* begun, uint32_t n, int64_t now_ns, const wgcs_session_slot* hs_slots,
                              uint32_t n_hs_slots, const wgcs_hs_state* states, uint32_t n_states, wgcs_timers* timers,
                              wgcs_rekey* rekey, uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxPeers || n_peers > kMaxPeers || !arena || !pkts || !gate || !begun || (n_hs_slots && !hs_slots) ||
      !pow2_or_0(n_hs_slots) || (n_states && !states) || (n_peers && (!timers || !rekey)))
    return WGCS_ERR_INVALID_ARG;
  const TimersFinished body = {{arena, pkts, gate, hs_slots, n_hs_slots, states, n_states, n_peers}, begun, now_ns,
                               timers, rekey};
  for (uint32_t q = 0; q < n; ++q) body(q);
  return WGCS_OK;
}

int wgcs_timers_rotated_host(const wgcs_aead_pkt* pkts, const uint32_t* rotated, uint32_t n, int64_t now_ns,
                             const uint32_t* key_peer, uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids,
                             wgcs_timers* timers, wgcs_rekey* rekey, uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !pkts || !rotated || (n_keys && !key_peer) || (n_peers && !rekey) ||
      !rows_ok(peer_rows, n_ids, timers, n_peers))
    return WGCS_ERR_INVALID_ARG;
  const TimersRotated body = {{pkts, key_peer, n_keys, peer_rows, n_ids, n_peers}, rotated, now_ns, timers, rekey};
  for (uint32_t i = 0; i < n; ++i) body(i);
  return WGCS_OK;
}

int wgcs_timers_expire_host(int64_t now_ns, wgcs_timers* timers, wgcs_rekey* rekey, const wgcs_peer_key* table,
                            uint32_t n_peers, const uint32_t* staged, wgcs_keypairs* kp, wgcs_session_slot* slots,
                            uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
                            wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys, uint32_t n_ka_max,
                            uint32_t* ka_peer, int32_t* ka_count, int32_t* ka_sizes, int32_t* ka_status,
                            uint32_t* n_ka, uint32_t* actions) {
  if (!n_ka || (n_peers && (!timers || !rekey || !table || !kp || !actions)) || (n_slots && !slots) ||
      (n_peer_slots && !peer_keys) || (n_keys && (!keys || !key_peer)) ||
      (n_ka_max && (!ka_peer || !ka_count || !ka_sizes || !ka_status)) || n_peers > kMaxPeers ||
      n_ka_max > kMaxPeers || !pow2_or_0(n_slots) || !pow2_or_0(n_peer_slots))
    return WGCS_ERR_INVALID_ARG;
  // the launches of the device form, each a loop: verdicts, then the owing rows by rank, then the tail
  for (uint32_t r = 0; r < n_peers; ++r)
    timers_expire_verdict(r, now_ns, timers, rekey, table, staged, kp, slots, n_slots, peer_keys, n_peer_slots, keys,
                          key_peer, n_keys, actions);
  uint32_t rank = 0;
  for (uint32_t r = 0; r < n_peers; ++r)
    if (actions[r] & WGCS_TIMERS_ACT_KEEPALIVE)
      timers_expire_commit(r, rank++, timers, table, n_ka_max, ka_peer, ka_count, ka_sizes, ka_status, actions);
  *n_ka = rank < n_ka_max ? rank : n_ka_max;
  for (uint32_t k = *n_ka; k < n_ka_max; ++k) timers_expire_tail(k, ka_peer, ka_count, ka_sizes, ka_status);
  return WGCS_OK;
}

}  // extern "C"
