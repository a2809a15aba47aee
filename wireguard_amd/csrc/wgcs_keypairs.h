// wgcs_keypairs.h -- keypair rotation as scalar row functions, shared by host
// and device: the tail of BeginSymmetricSession (device/noise.go:664-722) with
// sessions.AddKeypair (device/sessions.go:70-82) and DeleteSession, and
// ReceivedWithNewKeypair (noise.go:725-754) as receive.go:418-429 calls it.
// keypairs_kernels.hip runs them one lane per peer run (begin) or per row
// (received), keypairs.cpp in row order, and the stand-alone sanitizer program
// of tests/keypairs_host/ includes this one text.
//
// The tables are those of include/wgcsum.h: one wgcs_keypairs row per row of
// the peer table, the two slot arrays of wgcs_session_table_build (receiver
// index -> key row, peer id -> send-key row), the AEAD key table and its
// key -> peer id column.  A slot is found with SessionMap.Get's probe
// (wgcs_route_walk.h) and only its key is overwritten: the probe of a lane
// that runs beside this one sees the same chain of occupied slots.  Every row
// is 4-byte aligned and is read and written in 4-byte words.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_route_walk.h"

namespace wgcs {

constexpr uint32_t kKeypairsClaimNone = 0xFFFFFFFFu;  // wgcs_keypairs.claim outside a received call
constexpr int kKeypairsTaken = 1;  // keypairs_initiator_fields: the row is taken and its fields are found

// session_get's probe, for the slot itself: the position of `index`, or kSessionEmpty
WGCS_HD uint32_t session_slot_of(const wgcs_session_slot* slots, uint32_t n_slots, uint32_t index) {
  const uint32_t mask = n_slots - 1;
  uint32_t at = session_hash(index) & mask;
  for (uint32_t probe = 0; probe < n_slots; ++probe, at = (at + 1) & mask) {
    const wgcs_session_slot s = slots[at];
    if (s.key == kSessionEmpty) return kSessionEmpty;
    if (s.index == index) return at;
  }
  return kSessionEmpty;
}

// overwrite the key of index's slot; an index without a slot is left alone
WGCS_HD void session_set_key(wgcs_session_slot* slots, uint32_t n_slots, uint32_t index, uint32_t key) {
  const uint32_t at = session_slot_of(slots, n_slots, index);
  if (at != kSessionEmpty) slots[at].key = key;
}

WGCS_HD void keypair_ref_clear(wgcs_keypair_ref* r) {
  r->send_key = r->recv_key = r->local_index = r->flags = 0;
  r->created_ns = 0;
}

WGCS_HD void aead_key_zero(wgcs_aead_key* k) {
  uint32_t* const w = (uint32_t*)k;  // 48 B, 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < sizeof(wgcs_aead_key) / 4; ++i) w[i] = 0;
}

// d.DeleteSession(keypair), with the erasure the reference cannot do (keypair.go:12-17); x is a copy
WGCS_HD void delete_session(const wgcs_keypair_ref x, wgcs_session_slot* slots, uint32_t n_slots, wgcs_aead_key* keys,
                            uint32_t* key_peer, uint32_t n_keys) {
  if (!(x.flags & WGCS_KEYPAIR_SET)) return;  // keypair == nil
  session_set_key(slots, n_slots, x.local_index, WGCS_SESSION_NO_KEYPAIR);
  if (x.send_key < n_keys) {
    aead_key_zero(keys + x.send_key);
    key_peer[x.send_key] = WGCS_PEER_NONE;
  }
  if (x.recv_key < n_keys) {
    aead_key_zero(keys + x.recv_key);
    key_peer[x.recv_key] = WGCS_PEER_NONE;
  }
}

// The tail of BeginSymmetricSession for one handshake whose keys are in place: the status of
// its descriptor, with every table written as wgcs_keypairs_begin_*_batch says.
WGCS_HD int keypairs_begin(uint32_t peer_row, uint32_t local_index, uint32_t send_key, uint32_t recv_key,
                           bool is_initiator, int64_t now, const wgcs_peer_key* table, uint32_t n_peers,
                           wgcs_keypairs* kp, wgcs_session_slot* slots, uint32_t n_slots, wgcs_session_slot* peer_keys,
                           uint32_t n_peer_slots, wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys) {
  if (peer_row >= n_peers || send_key >= n_keys || recv_key >= n_keys || send_key == recv_key)
    return WGCS_ERR_INVALID_ARG;
  // sessions.AddKeypair (sessions.go:70-82) returns silently for an index it does not hold and the
  // reference goes on to rotate; here a keypair nobody could be reached under is not installed
  const uint32_t at = session_slot_of(slots, n_slots, local_index);
  if (at == kSessionEmpty || slots[at].key != WGCS_SESSION_NO_KEYPAIR) return WGCS_ERR_NO_HANDSHAKE;
  const uint32_t peer = table[peer_row].peer;
  slots[at].key = recv_key;  // :675
  key_peer[send_key] = key_peer[recv_key] = peer;
  wgcs_keypair_ref fresh;  // :664-673
  fresh.send_key = send_key;
  fresh.recv_key = recv_key;
  fresh.local_index = local_index;
  fresh.flags = WGCS_KEYPAIR_SET | (is_initiator ? WGCS_KEYPAIR_INITIATOR : 0u);
  fresh.created_ns = now;
  wgcs_keypairs* const k = kp + peer_row;
  const wgcs_keypair_ref current = k->current, previous = k->previous, next = k->next;  // :681-683
  if (is_initiator) {
    if (next.flags & WGCS_KEYPAIR_SET) {  // :703-707
      keypair_ref_clear(&k->next);
      k->previous = next;
      delete_session(current, slots, n_slots, keys, key_peer, n_keys);
    } else {  // :710
      k->previous = current;
    }
    delete_session(previous, slots, n_slots, keys, key_peer, n_keys);  // :712
    k->current = fresh;                                                // :713
    session_set_key(peer_keys, n_peer_slots, peer, send_key);          // the send chain seals under it from here on
  } else {
    k->next = fresh;                                                   // :717
    delete_session(next, slots, n_slots, keys, key_peer, n_keys);      // :718
    keypair_ref_clear(&k->previous);                                   // :719
    delete_session(previous, slots, n_slots, keys, key_peer, n_keys);  // :720
  }
  return WGCS_HS_BEGUN;
}

// What a descriptor of the responder's form names.  false: not taken (status WGCS_HS_NONE).
WGCS_HD bool keypairs_responder_fields(const wgcs_hs_resp* resp, const int32_t* gate, uint32_t j, uint32_t f[4]) {
  if (gate[j] != WGCS_HS_RESPONDED) return false;
  const wgcs_hs_resp* const r = resp + j;
  f[0] = r->peer_row;
  f[1] = r->local_index;
  f[2] = r->send_key;
  f[3] = r->recv_key;
  return true;
}

// LE32 msg[8:12] of the message at p: msg.Receiver of a response
WGCS_HD uint32_t keypairs_msg_receiver(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the one or two aligned words that hold the four bytes; both lie inside the 92-byte message
  const uint32_t sh = (uint32_t)(uintptr_t)(p + 8) & 3u;
  const uint32_t* const w = (const uint32_t*)(p + 8 - sh);
  const uint32_t lo = w[0];
  return sh ? __builtin_amdgcn_alignbyte(w[1], lo, sh) : lo;
#else
  return (uint32_t)p[8] | ((uint32_t)p[9] << 8) | ((uint32_t)p[10] << 16) | ((uint32_t)p[11] << 24);
#endif
}

// What row q of the initiator's form names, through the handshake's state row, which
// wgcs_handshake_finish_batch left in place when it zeroed the secrets.  WGCS_HS_NONE: not
// taken; WGCS_ERR_NO_HANDSHAKE: no state row answers to the index; kKeypairsTaken: f is filled.
WGCS_HD int keypairs_initiator_fields(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* gate, uint32_t q,
                                      const wgcs_session_slot* hs_slots, uint32_t n_hs_slots,
                                      const wgcs_hs_state* states, uint32_t n_states, uint32_t f[4]) {
  if (gate[q] != WGCS_HS_FINISHED) return WGCS_HS_NONE;
  const uint32_t index = keypairs_msg_receiver(arena + pkts[q].off);
  const uint32_t row = session_get(hs_slots, n_hs_slots, index);  // empty is past any table
  if (row >= n_states) return WGCS_ERR_NO_HANDSHAKE;
  const wgcs_hs_state* const st = states + row;
  if (st->local_index != index) return WGCS_ERR_NO_HANDSHAKE;
  f[0] = st->peer_row;
  f[1] = index;
  f[2] = st->send_key;
  f[3] = st->recv_key;
  return kKeypairsTaken;
}

// ---- ReceivedWithNewKeypair over the rows of a receive batch, in two passes ----

// the row of kp that row i's key belongs to, or WGCS_PEER_NONE for a row that takes no part
WGCS_HD uint32_t keypairs_received_row(uint32_t i, const wgcs_aead_pkt* pkts, const int32_t* verdict,
                                       const uint32_t* key_peer, uint32_t n_keys, const uint32_t* peer_rows,
                                       uint32_t n_ids, uint32_t n_peers, uint32_t* key_out, uint32_t* id_out) {
  const uint32_t key = pkts[i].key;
  if (key >= n_keys) return WGCS_PEER_NONE;
  const int32_t v = verdict[i];
  if (v < 0 && v != WGCS_ERR_PACKET_TOO_SHORT) return WGCS_PEER_NONE;  // not decrypted, or the filter said no
  const uint32_t id = key_peer[key];
  if (id >= n_ids) return WGCS_PEER_NONE;
  const uint32_t row = peer_rows[id];
  if (row == WGCS_PEER_NONE || row >= n_peers) return WGCS_PEER_NONE;
  *key_out = key;
  *id_out = id;
  return row;
}

// The first pass: 1 for a candidate (keypairs.next.Load() == new, :731), which takes the minimum
// of i and its peer's claim; 0 for any other row.  Nothing else is written.
WGCS_HD uint32_t keypairs_received_claim(uint32_t i, const wgcs_aead_pkt* pkts, const int32_t* verdict,
                                         const uint32_t* key_peer, uint32_t n_keys, const uint32_t* peer_rows,
                                         uint32_t n_ids, wgcs_keypairs* kp, uint32_t n_peers) {
  uint32_t key, id;
  const uint32_t row = keypairs_received_row(i, pkts, verdict, key_peer, n_keys, peer_rows, n_ids, n_peers, &key, &id);
  if (row == WGCS_PEER_NONE) return 0;
  wgcs_keypairs* const k = kp + row;
  if (!(k->next.flags & WGCS_KEYPAIR_SET) || k->next.recv_key != key) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
  // Every packet of a new session's first burst is a candidate: a plain look first keeps all but the low
  // rows off the atomic unit.  The claim only falls, so a stale value costs an atomic and never a claim.
  if (i < __hip_atomic_load(&k->claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&k->claim, i);
#else
  if (i < k->claim) k->claim = i;
#endif
  return 1;
}

// The second pass, for a candidate only: 1 and the rotation (:748-752) for the row that holds
// its peer's claim, 0 for the others, which the reference would turn away at :740.
WGCS_HD uint32_t keypairs_received_commit(uint32_t i, const wgcs_aead_pkt* pkts, uint32_t* key_peer, uint32_t n_keys,
                                          const uint32_t* peer_rows, uint32_t n_ids, wgcs_keypairs* kp,
                                          uint32_t n_peers, wgcs_session_slot* slots, uint32_t n_slots,
                                          wgcs_session_slot* peer_keys, uint32_t n_peer_slots, wgcs_aead_key* keys) {
  // The row the first pass found.  The checks can only fail where two peers' keypairs name one key
  // row (the caller's error) and a winner's DeleteSession has just cleared it: then nothing is read.
  const uint32_t id = key_peer[pkts[i].key];
  if (id >= n_ids) return 0;
  const uint32_t row = peer_rows[id];
  if (row >= n_peers) return 0;
  wgcs_keypairs* const k = kp + row;
  if (k->claim != i) return 0;  // a lower row's, or kKeypairsClaimNone once that row has committed: never i
  const wgcs_keypair_ref previous = k->previous, next = k->next;
  k->previous = k->current;
  delete_session(previous, slots, n_slots, keys, key_peer, n_keys);
  k->current = next;
  keypair_ref_clear(&k->next);
  k->claim = kKeypairsClaimNone;
  session_set_key(peer_keys, n_peer_slots, id, next.send_key);
  return 1;
}

}  // namespace wgcs
