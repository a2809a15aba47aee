// wgcs_events.h -- the peer-event sources, shared by host and device: which row
// of the peer tables entry i of a call stands for.  Each source is a struct of
// the call's input arrays with row(i), the peer row or WGCS_PEER_NONE for an
// entry that takes no part:
//   JobRows         the jobs of a send-assign batch         send-assign's own rule
//   KeptJobRows     those of them that send-assign kept     d_job_key
//   GroupRows       the write builder's groups              receive.go:486
//   RespondedRows   the descriptors of a respond batch      status WGCS_HS_RESPONDED
//   AcceptedRows    the same descriptors behind accept, which writes no status
//   InitiatedRows   the descriptors of an initiate batch    status WGCS_HS_INITIATED
//   TicketRows      the tickets of a start call             status WGCS_HS_INITIATED
//   FinishedRows    the rows of a finish batch              gate WGCS_HS_FINISHED
//   KeyRows         the packets of a receive batch          key -> peer id -> row
// The timers, the rekey rules, the cookie generator and the endpoints build
// their row bodies over them (wgcs_timers.h, wgcs_rekey.h, wgcs_cookiegen.h,
// wgcs_endpoint.h); wgcs_each.h runs a body one lane per entry, the host forms
// in entry order.  row() reads only what no other entry of the call writes, so
// both passes of a two-pass call see one row for an entry.
#pragma once

#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_keypairs.h"

namespace wgcs {

constexpr uint32_t kRekeyNoKey = 0xFFFFFFFFu;  // send-assign's d_job_key of a dropped job

// the row of the peer table that id names, or WGCS_PEER_NONE for "no row"
WGCS_HD uint32_t peer_row_of(uint32_t id, const uint32_t* peer_rows, uint32_t n_ids, uint32_t n_peers) {
  if (id >= n_ids) return WGCS_PEER_NONE;
  const uint32_t row = peer_rows[id];
  return row < n_peers ? row : WGCS_PEER_NONE;  // n_peers <= 2^24: WGCS_PEER_NONE itself is past it
}

// *claim = max(*claim, ticket): entry i of a two-pass call claims its peer's word with i + 1, and
// the one entry that finds its ticket there in the second pass commits and puts 0 back.  On the
// device a plain look comes first, as in keypairs_received_claim: the claim only rises within a
// pass, so a stale value costs an atomic and never a claim.
WGCS_HD void claim_max(uint32_t* claim, uint32_t ticket) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (ticket > __hip_atomic_load(claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(claim, ticket);
#else
  if (ticket > *claim) *claim = ticket;
#endif
}

// The peer row of job j by send-assign's own rule (status 0, 1 <= count <= max_segs, the first
// slot's peer), or WGCS_PEER_NONE for a job that is not taken or whose peer has no row.
struct JobRows {
  const uint32_t* peer;
  const int32_t *count, *status;
  uint32_t max_segs;
  const uint32_t* peer_rows;
  uint32_t n_ids, n_peers;
  WGCS_HD uint32_t row(uint32_t j) const {
    if (status[j] != 0) return WGCS_PEER_NONE;
    const int32_t c = count[j];
    if (c < 1 || (uint32_t)c > max_segs) return WGCS_PEER_NONE;
    return peer_row_of(peer[(uint64_t)j * max_segs], peer_rows, n_ids, n_peers);
  }
};

// send-assign kept job j: a dropped one sent nothing
WGCS_HD bool job_kept(const uint32_t* job_key, uint32_t j) { return job_key[j] != kRekeyNoKey; }

struct KeptJobRows {  // the jobs that went out: send.go:498-510 and Peer.Send
  JobRows jobs;
  const uint32_t* job_key;
  WGCS_HD uint32_t row(uint32_t j) const { return job_kept(job_key, j) ? jobs.row(j) : WGCS_PEER_NONE; }
};

struct GroupRows {  // receive.go:486 for row c of the write builder's groups
  const wgcs_write_group* groups;
  const uint32_t* peer_rows;
  uint32_t n_ids, n_peers;
  WGCS_HD int32_t tail(uint32_t c) const { return groups[c].tail; }
  WGCS_HD uint32_t flags(uint32_t c) const { return groups[c].flags; }
  WGCS_HD uint32_t row(uint32_t c) const {
    if (tail(c) < 0) return WGCS_PEER_NONE;  // an unused row, and dataPacketReceived implies a valid tail
    return peer_row_of(groups[c].peer, peer_rows, n_ids, n_peers);
  }
};

struct RespondedRows {  // descriptor j of a respond batch and its status
  const wgcs_hs_resp* resp;
  const int32_t* gate;
  uint32_t n_peers;
  WGCS_HD uint32_t row(uint32_t j) const {
    if (gate[j] != WGCS_HS_RESPONDED) return WGCS_PEER_NONE;
    const uint32_t r = resp[j].peer_row;
    return r < n_peers ? r : WGCS_PEER_NONE;
  }
};

struct AcceptedRows {  // descriptor j of an accept call: a tail row carries 0xFFFFFFFF
  const wgcs_hs_resp* resp;
  uint32_t n_peers;
  WGCS_HD uint32_t init_row(uint32_t j) const { return resp[j].init_row; }
  WGCS_HD uint32_t row(uint32_t j) const {
    const uint32_t r = resp[j].peer_row;
    return r < n_peers ? r : WGCS_PEER_NONE;
  }
};

struct InitiatedRows {  // descriptor j of an initiate batch and its status
  const wgcs_hs_start* start;
  const int32_t* status;
  uint32_t n_peers;
  WGCS_HD uint32_t row(uint32_t j) const {
    if (status[j] != WGCS_HS_INITIATED) return WGCS_PEER_NONE;
    const uint32_t r = start[j].peer_row;
    return r < n_peers ? r : WGCS_PEER_NONE;
  }
};

struct TicketRows {  // ticket k of a start call, once initiate has built its message
  const uint32_t* start_peer;
  const int32_t* init_status;
  uint32_t n_peers;
  WGCS_HD uint32_t row(uint32_t k) const {
    const uint32_t r = start_peer[k];
    return r < n_peers && init_status[k] == WGCS_HS_INITIATED ? r : WGCS_PEER_NONE;
  }
};

struct FinishedRows {  // row q of a finish batch: receiver -> state row -> peer row
  const uint8_t* arena;
  const wgcs_aead_pkt* pkts;
  const int32_t* gate;
  const wgcs_session_slot* hs_slots;
  uint32_t n_hs_slots;
  const wgcs_hs_state* states;
  uint32_t n_states, n_peers;
  WGCS_HD uint32_t row(uint32_t q) const {
    uint32_t f[4];
    if (keypairs_initiator_fields(arena, pkts, gate, q, hs_slots, n_hs_slots, states, n_states, f) != kKeypairsTaken)
      return WGCS_PEER_NONE;
    return f[0] < n_peers ? f[0] : WGCS_PEER_NONE;
  }
};

struct KeyRows {  // packet i of a receive batch: its key's peer
  const wgcs_aead_pkt* pkts;
  const uint32_t* key_peer;
  uint32_t n_keys;
  const uint32_t* peer_rows;
  uint32_t n_ids, n_peers;
  WGCS_HD uint32_t key(uint32_t i) const { return pkts[i].key; }
  WGCS_HD uint32_t row(uint32_t i) const {
    const uint32_t k = key(i);
    if (k >= n_keys) return WGCS_PEER_NONE;
    return peer_row_of(key_peer[k], peer_rows, n_ids, n_peers);
  }
};

}  // namespace wgcs
