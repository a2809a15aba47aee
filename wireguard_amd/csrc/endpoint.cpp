// endpoint.cpp -- the peer endpoints on host memory (include/wgcsum.h), no
// context and no device:
//   wgcs_endpoint_recv_host            conn/bind.go:308-319, conn/sticky.go:46-94
//   wgcs_endpoint_set_received_host    SetEndpointFromPacket at device/receive.go:487
//   wgcs_endpoint_set_accepted_host    ... at :314
//   wgcs_endpoint_set_finished_host    ... at :335
//   wgcs_endpoint_dst_jobs_host        Peer.Send up to bind.Send, device/peer.go:201-211
//   wgcs_endpoint_dst_initiated_host   the same for the initiations of a start call
//   wgcs_endpoint_dst_responded_host   the same for the responses of an accept call
// They run the row functions of wgcs_endpoint.h, the code the lanes of
// endpoint_kernels.hip run, in the passes of the device forms with the rows
// taken in ascending order.  Plain C++: the host test program
// (tests/endpoint_host/endpoint_host.cpp) links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include "../../include/wgcsum.h"
#include "wgcs_endpoint.h"

using namespace wgcs;

namespace {

inline bool pow2_or_0(uint32_t n) { return (n & (n - 1)) == 0; }

// claim, then commit: the two launches of a set call
template <class Finder>
void set_rows(const Finder& f, uint32_t n, const wgcs_endpoint* ep, wgcs_endpoint* table, uint32_t* claim,
              wgcs_timers* timers) {
  for (uint32_t i = 0; i < n; ++i) endpoint_set_claim(i, f.pick(i), claim);
  for (uint32_t i = 0; i < n; ++i) endpoint_set_commit(i, f.pick(i), ep, table, claim, timers);
}

// read, then clear: the two launches of a dst call
template <class Finder>
void dst_rows(const Finder& f, uint32_t n, wgcs_endpoint* table, wgcs_timers* timers, wgcs_endpoint* dst,
              int32_t* dst_v6, int32_t* dst_status) {
  for (uint32_t j = 0; j < n; ++j) endpoint_dst_read(j, f.row(j), table, timers, dst, dst_v6, dst_status);
  for (uint32_t j = 0; j < n; ++j) endpoint_dst_clear(f.row(j), table, timers);
}

}  // namespace

extern "C" {

int wgcs_endpoint_recv_host(const wgcs_src_addr* addr, const int32_t* from, const int32_t* size, const uint8_t* oob,
                            uint32_t oob_stride, const int32_t* nn, uint32_t n_msgs, uint32_t n_batches,
                            wgcs_endpoint* ep, wgcs_src_addr* addr_out) {
  const uint64_t n = (uint64_t)n_batches * n_msgs;
  if (n == 0) return WGCS_OK;
  if (!endpoint_recv_args_ok(addr, from, size, oob, oob_stride, nn, n, ep, addr_out)) return WGCS_ERR_INVALID_ARG;
  for (uint32_t q = 0; q < (uint32_t)n; ++q) endpoint_recv(q, n_msgs, addr, from, size, oob, oob_stride, nn, ep, addr_out);
  return WGCS_OK;
}

int wgcs_endpoint_set_received_host(const wgcs_write_group* groups, uint32_t n_batches, uint32_t calls_per_batch,
                                    const wgcs_endpoint* ep, uint32_t n_rows, const uint32_t* peer_rows, uint32_t n_ids,
                                    wgcs_endpoint* table, uint32_t* claim, wgcs_timers* timers, uint32_t n_peers) {
  const uint64_t n = (uint64_t)n_batches * calls_per_batch;
  if (n == 0) return WGCS_OK;
  if (n > kMaxRows || !groups || endpoint_misaligned(groups, 7) || (n_ids && !peer_rows) ||
      endpoint_misaligned(peer_rows, 3) || !endpoint_set_tables_ok(ep, n_rows, table, claim, timers, n_peers))
    return WGCS_ERR_INVALID_ARG;
  set_rows(EndpointReceived{groups, ep, n_rows, peer_rows, n_ids, n_peers}, (uint32_t)n, ep, table, claim, timers);
  return WGCS_OK;
}

int wgcs_endpoint_set_accepted_host(const wgcs_hs_resp* resp, uint32_t n_tickets, const wgcs_endpoint* ep,
                                    uint32_t n_rows, wgcs_endpoint* table, uint32_t* claim, wgcs_timers* timers,
                                    uint32_t n_peers) {
  if (n_tickets == 0) return WGCS_OK;
  if (n_tickets > kMaxRows || !resp || endpoint_misaligned(resp, 3) ||
      !endpoint_set_tables_ok(ep, n_rows, table, claim, timers, n_peers))
    return WGCS_ERR_INVALID_ARG;
  set_rows(EndpointAccepted{resp, ep, n_rows, n_peers}, n_tickets, ep, table, claim, timers);
  return WGCS_OK;
}

int wgcs_endpoint_set_finished_host(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* gate, uint32_t n,
                                    const wgcs_session_slot* hs_slots, uint32_t n_hs_slots, const wgcs_hs_state* states,
                                    uint32_t n_states, const wgcs_endpoint* ep, wgcs_endpoint* table, uint32_t* claim,
                                    wgcs_timers* timers, uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (n > kMaxPeers || !arena || !pkts || !gate || (n_hs_slots && !hs_slots) || !pow2_or_0(n_hs_slots) ||
      (n_states && !states) || endpoint_misaligned(pkts, 7) || endpoint_misaligned(gate, 3) ||
      endpoint_misaligned(hs_slots, 3) || endpoint_misaligned(states, 3) ||
      !endpoint_set_tables_ok(ep, n, table, claim, timers, n_peers))
    return WGCS_ERR_INVALID_ARG;
  set_rows(EndpointFinished{arena, pkts, gate, hs_slots, n_hs_slots, states, n_states, ep, n_peers}, n, ep, table, claim,
           timers);
  return WGCS_OK;
}

int wgcs_endpoint_dst_jobs_host(const uint32_t* peer, const int32_t* count, const int32_t* status,
                                const uint32_t* job_key, uint32_t n_jobs, uint32_t max_segs, const int32_t* lens,
                                int32_t* nbufs, const uint32_t* peer_rows, uint32_t n_ids, wgcs_endpoint* table,
                                wgcs_timers* timers, uint32_t n_peers, wgcs_endpoint* dst, int32_t* dst_v6,
                                int32_t* dst_status, uint64_t* tx_bytes) {
  if (n_jobs == 0) return WGCS_OK;
  if (!peer || !count || !status || !job_key || !lens || !nbufs || max_segs == 0 ||
      (uint64_t)n_jobs * max_segs > kMaxRows || (n_ids && !peer_rows) || endpoint_misaligned(peer, 3) ||
      endpoint_misaligned(count, 3) || endpoint_misaligned(status, 3) || endpoint_misaligned(job_key, 3) ||
      endpoint_misaligned(lens, 3) || endpoint_misaligned(nbufs, 3) || endpoint_misaligned(peer_rows, 3) ||
      !endpoint_dst_tables_ok(n_jobs, table, timers, n_peers, dst, dst_v6, dst_status, tx_bytes, true))
    return WGCS_ERR_INVALID_ARG;
  const EndpointJobs f = {peer, count, status, job_key, max_segs, peer_rows, n_ids, n_peers};
  for (uint32_t j = 0; j < n_jobs; ++j) {
    const uint32_t row = f.row(j);
    endpoint_dst_job(j, row, endpoint_dst_read(j, row, table, timers, dst, dst_v6, dst_status), max_segs, lens, nbufs,
                     tx_bytes);
  }
  for (uint32_t j = 0; j < n_jobs; ++j) endpoint_dst_clear(f.row(j), table, timers);
  return WGCS_OK;
}

int wgcs_endpoint_dst_initiated_host(const wgcs_hs_start* start, const int32_t* status, uint32_t n,
                                     wgcs_endpoint* table, wgcs_timers* timers, uint32_t n_peers, wgcs_endpoint* dst,
                                     int32_t* dst_v6, int32_t* dst_status) {
  if (n == 0) return WGCS_OK;
  if (!start || !status || endpoint_misaligned(start, 3) || endpoint_misaligned(status, 3) ||
      !endpoint_dst_tables_ok(n, table, timers, n_peers, dst, dst_v6, dst_status, nullptr, false))
    return WGCS_ERR_INVALID_ARG;
  dst_rows(EndpointInitiated{start, status, n_peers}, n, table, timers, dst, dst_v6, dst_status);
  return WGCS_OK;
}

int wgcs_endpoint_dst_responded_host(const wgcs_hs_resp* resp, const int32_t* status, uint32_t n, wgcs_endpoint* table,
                                     wgcs_timers* timers, uint32_t n_peers, wgcs_endpoint* dst, int32_t* dst_v6,
                                     int32_t* dst_status) {
  if (n == 0) return WGCS_OK;
  if (!resp || !status || endpoint_misaligned(resp, 3) || endpoint_misaligned(status, 3) ||
      !endpoint_dst_tables_ok(n, table, timers, n_peers, dst, dst_v6, dst_status, nullptr, false))
    return WGCS_ERR_INVALID_ARG;
  dst_rows(EndpointResponded{resp, status, n_peers}, n, table, timers, dst, dst_v6, dst_status);
  return WGCS_OK;
}

}  // extern "C"
