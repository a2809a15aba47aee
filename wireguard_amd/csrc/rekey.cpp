// rekey.cpp -- keypair expiry, the rekey rules and the start of a handshake on
// host memory (include/wgcsum.h), no context and no device:
//   wgcs_rekey_recv_gate_host    device/receive.go:162-170
//   wgcs_rekey_send_gate_host    device/send.go:368-374
//   wgcs_rekey_sent_host         send.go:213-227, :419-420
//   wgcs_rekey_received_host     receive.go:80-91
//   wgcs_rekey_responded_host    send.go:131-133
//   wgcs_rekey_start_host        send.go:84-100, in the passes of the device form
// They run the bodies and row functions of wgcs_rekey.h, the code the lanes of
// the device forms run, taken in row order.  Plain C++: the host test program
// (tests/rekey_host/rekey_host.cpp) links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_rekey.h"

using namespace wgcs;

namespace {

inline bool rows_ok(const uint32_t* peer_rows, uint32_t n_ids, const wgcs_keypairs* kp, uint32_t n_peers) {
  return (!n_ids || peer_rows) && (!n_peers || kp);
}

bool jobs_ok(const uint32_t* peer, const int32_t* count, const int32_t* status, uint32_t n_jobs, uint32_t max_segs,
             const uint32_t* peer_rows, uint32_t n_ids, const wgcs_keypairs* kp, uint32_t n_peers,
             const uint64_t* send_nonce, uint32_t n_keys, const wgcs_rekey* rekey) {
  return peer && count && status && max_segs && (uint64_t)n_jobs * max_segs <= kMaxRows && (!n_keys || send_nonce) &&
         (!n_peers || rekey) && rows_ok(peer_rows, n_ids, kp, n_peers);
}

}  // namespace

extern "C" {

int wgcs_rekey_recv_gate_host(wgcs_aead_pkt* pkts, uint32_t n, int64_t now_ns, const uint32_t* key_peer,
                              uint32_t n_keys, const uint32_t* peer_rows, uint32_t n_ids, const wgcs_keypairs* kp,
                              uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !pkts || (n_keys && !key_peer) || !rows_ok(peer_rows, n_ids, kp, n_peers))
    return WGCS_ERR_INVALID_ARG;
  const RekeyRecvGate body = {{pkts, key_peer, n_keys, peer_rows, n_ids, n_peers}, now_ns, kp, pkts};
  for (uint32_t i = 0; i < n; ++i) body(i);
  return WGCS_OK;
}

int wgcs_rekey_send_gate_host(const uint32_t* peer, const int32_t* count, const int32_t* status_in, uint32_t n_jobs,
                              uint32_t max_segs, int64_t now_ns, const uint32_t* peer_rows, uint32_t n_ids,
                              const wgcs_keypairs* kp, uint32_t n_peers, const uint64_t* send_nonce, uint32_t n_keys,
                              uint64_t limit, wgcs_rekey* rekey, int32_t* status_out) {
  if (n_jobs == 0) return WGCS_OK;
  if (!status_out ||
      !jobs_ok(peer, count, status_in, n_jobs, max_segs, peer_rows, n_ids, kp, n_peers, send_nonce, n_keys, rekey))
    return WGCS_ERR_INVALID_ARG;
  const RekeySendGate body = {{peer, count, status_in, max_segs, peer_rows, n_ids, n_peers}, now_ns, kp, send_nonce,
                              n_keys, limit, rekey, status_out};
  for (uint32_t j = 0; j < n_jobs; ++j) body(j);
  return WGCS_OK;
}

int wgcs_rekey_sent_host(const uint32_t* peer, const int32_t* count, const int32_t* status, const uint32_t* job_key,
                         uint32_t n_jobs, uint32_t max_segs, int64_t now_ns, const uint32_t* peer_rows, uint32_t n_ids,
                         const wgcs_keypairs* kp, uint32_t n_peers, const uint64_t* send_nonce, uint32_t n_keys,
                         uint64_t limit, wgcs_rekey* rekey) {
  if (n_jobs == 0) return WGCS_OK;
  if (!job_key ||
      !jobs_ok(peer, count, status, n_jobs, max_segs, peer_rows, n_ids, kp, n_peers, send_nonce, n_keys, rekey))
    return WGCS_ERR_INVALID_ARG;
  const RekeySent body = {{peer, count, status, max_segs, peer_rows, n_ids, n_peers}, job_key, now_ns, kp, send_nonce,
                          n_keys, limit, rekey};
  for (uint32_t j = 0; j < n_jobs; ++j) body(j);
  return WGCS_OK;
}

int wgcs_rekey_received_host(const wgcs_write_group* groups, uint32_t n_batches, uint32_t calls_per_batch,
                             int64_t now_ns, const uint32_t* peer_rows, uint32_t n_ids, const wgcs_keypairs* kp,
                             uint32_t n_peers, wgcs_rekey* rekey) {
  const uint64_t n = (uint64_t)n_batches * calls_per_batch;
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !groups || (n_peers && !rekey) || !rows_ok(peer_rows, n_ids, kp, n_peers))
    return WGCS_ERR_INVALID_ARG;
  const RekeyReceived body = {{groups, peer_rows, n_ids, n_peers}, now_ns, kp, rekey};
  for (uint32_t c = 0; c < (uint32_t)n; ++c) body(c);
  return WGCS_OK;
}

int wgcs_rekey_responded_host(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t n, int64_t now_ns,
                              wgcs_rekey* rekey, uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !resp || !gate || (n_peers && !rekey)) return WGCS_ERR_INVALID_ARG;
  const RekeyResponded body = {{resp, gate, n_peers}, now_ns, rekey};
  for (uint32_t j = 0; j < n; ++j) body(j);
  return WGCS_OK;
}

int wgcs_rekey_start_host(int64_t now_ns, wgcs_rekey* rekey, const wgcs_hs_peer* hs_peers, uint32_t n_peers,
                          const wgcs_hs_start* tickets, uint32_t n_tickets, wgcs_hs_start* start,
                          uint32_t* start_peer, uint32_t* count, int32_t* status, uint32_t* reasons) {
  if (!count || (n_peers && (!rekey || !hs_peers || !status || !reasons)) ||
      (n_tickets && (!tickets || !start || !start_peer || start == tickets)) || n_peers > kMaxPeers ||
      n_tickets > kMaxRows)
    return WGCS_ERR_INVALID_ARG;
  // the launches of the device form, each a loop: verdicts, then the candidates by rank, then the tail
  for (uint32_t r = 0; r < n_peers; ++r) status[r] = rekey_start_verdict(r, now_ns, rekey, reasons);
  uint32_t rank = 0;
  for (uint32_t r = 0; r < n_peers; ++r)
    if (status[r] == WGCS_HS_STARTED)
      status[r] = rekey_start_commit(r, rank++, now_ns, rekey, hs_peers, tickets, n_tickets, start, start_peer);
  *count = rank < n_tickets ? rank : n_tickets;
  for (uint32_t k = *count; k < n_tickets; ++k) rekey_start_tail(k, start, start_peer);
  return WGCS_OK;
}

}  // extern "C"
