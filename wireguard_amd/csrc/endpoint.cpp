// endpoint.cpp -- the peer endpoints on host memory (include/wgcsum.h), no
// context and no device:
//   wgcs_endpoint_recv_host            conn/bind.go:308-319, conn/sticky.go:46-94
//   wgcs_endpoint_set_received_host    SetEndpointFromPacket at device/receive.go:487
//   wgcs_endpoint_set_accepted_host    ... at :314
//   wgcs_endpoint_set_finished_host    ... at :335
//   wgcs_endpoint_dst_jobs_host        Peer.Send up to bind.Send, device/peer.go:201-211
//   wgcs_endpoint_dst_initiated_host   the same for the initiations of a start call
//   wgcs_endpoint_dst_responded_host   the same for the responses of an accept call
// They run the bodies of wgcs_endpoint.h, the code the lanes of the device
// forms run, in the passes of the device forms with the rows taken in
// ascending order.  Plain C++: the host test program
// (tests/endpoint_host/endpoint_host.cpp) links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include "../../include/wgcsum.h"
#include "wgcs_endpoint.h"

using namespace wgcs;

namespace {

// the two launches of a call, each a loop
template <class First, class Second>
void two_passes(const First& first, const Second& second, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) first(i);
  for (uint32_t i = 0; i < n; ++i) second(i);
}

// claim, then commit: a set call
template <class Rows>
void set_rows(const Rows& src, uint32_t n, const wgcs_endpoint* ep, uint32_t n_rows, wgcs_endpoint* table,
              uint32_t* claim, wgcs_timers* timers) {
  const EndpointSetClaim<Rows> first = {src, ep, n_rows, claim};
  two_passes(first, EndpointSetCommit<Rows>{src, ep, n_rows, table, claim, timers}, n);
}

// read, then clear: a dst call over descriptors
template <class Rows>
void dst_rows(const Rows& src, uint32_t n, wgcs_endpoint* table, wgcs_timers* timers, wgcs_endpoint* dst,
              int32_t* dst_v6, int32_t* dst_status) {
  const EndpointDstRead<Rows> first = {src, table, timers, dst, dst_v6, dst_status};
  two_passes(first, EndpointDstClear<Rows>{src, table, timers}, n);
}

}  // namespace

extern "C" {

int wgcs_endpoint_recv_host(const wgcs_src_addr* addr, const int32_t* from, const int32_t* size, const uint8_t* oob,
                            uint32_t oob_stride, const int32_t* nn, uint32_t n_msgs, uint32_t n_batches,
                            wgcs_endpoint* ep, wgcs_src_addr* addr_out) {
  const uint64_t n = (uint64_t)n_batches * n_msgs;
  if (n == 0) return WGCS_OK;
  if (!endpoint_recv_args_ok(addr, from, size, oob, oob_stride, nn, n, ep, addr_out)) return WGCS_ERR_INVALID_ARG;
  const EndpointRecv body = {n_msgs, addr, from, size, oob, oob_stride, nn, ep, addr_out};
  for (uint32_t q = 0; q < (uint32_t)n; ++q) body(q);
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
  set_rows(GroupRows{groups, peer_rows, n_ids, n_peers}, (uint32_t)n, ep, n_rows, table, claim, timers);
  return WGCS_OK;
}

int wgcs_endpoint_set_accepted_host(const wgcs_hs_resp* resp, uint32_t n_tickets, const wgcs_endpoint* ep,
                                    uint32_t n_rows, wgcs_endpoint* table, uint32_t* claim, wgcs_timers* timers,
                                    uint32_t n_peers) {
  if (n_tickets == 0) return WGCS_OK;
  if (n_tickets > kMaxRows || !resp || endpoint_misaligned(resp, 3) ||
      !endpoint_set_tables_ok(ep, n_rows, table, claim, timers, n_peers))
    return WGCS_ERR_INVALID_ARG;
  set_rows(AcceptedRows{resp, n_peers}, n_tickets, ep, n_rows, table, claim, timers);
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
  set_rows(FinishedRows{arena, pkts, gate, hs_slots, n_hs_slots, states, n_states, n_peers}, n, ep, n, table, claim,
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
  const KeptJobRows src = {{peer, count, status, max_segs, peer_rows, n_ids, n_peers}, job_key};
  two_passes(EndpointDstJobs{{src, table, timers, dst, dst_v6, dst_status}, lens, nbufs, tx_bytes},
             EndpointDstClear<KeptJobRows>{src, table, timers}, n_jobs);
  return WGCS_OK;
}

int wgcs_endpoint_dst_initiated_host(const wgcs_hs_start* start, const int32_t* status, uint32_t n,
                                     wgcs_endpoint* table, wgcs_timers* timers, uint32_t n_peers, wgcs_endpoint* dst,
                                     int32_t* dst_v6, int32_t* dst_status) {
  if (n == 0) return WGCS_OK;
  if (!start || !status || endpoint_misaligned(start, 3) || endpoint_misaligned(status, 3) ||
      !endpoint_dst_tables_ok(n, table, timers, n_peers, dst, dst_v6, dst_status, nullptr, false))
    return WGCS_ERR_INVALID_ARG;
  dst_rows(InitiatedRows{start, status, n_peers}, n, table, timers, dst, dst_v6, dst_status);
  return WGCS_OK;
}

int wgcs_endpoint_dst_responded_host(const wgcs_hs_resp* resp, const int32_t* status, uint32_t n, wgcs_endpoint* table,
                                     wgcs_timers* timers, uint32_t n_peers, wgcs_endpoint* dst, int32_t* dst_v6,
                                     int32_t* dst_status) {
  if (n == 0) return WGCS_OK;
  if (!resp || !status || endpoint_misaligned(resp, 3) || endpoint_misaligned(status, 3) ||
      !endpoint_dst_tables_ok(n, table, timers, n_peers, dst, dst_v6, dst_status, nullptr, false))
    return WGCS_ERR_INVALID_ARG;
  dst_rows(RespondedRows{resp, status, n_peers}, n, table, timers, dst, dst_v6, dst_status);
  return WGCS_OK;
}

}  // extern "C"
