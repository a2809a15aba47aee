// wgcs_rekey.h -- keypair expiry, the rekey rules and the start of a handshake
// as scalar row functions, shared by host and device:
//   the receive gate           device/receive.go:162-170
//   the send gate              device/send.go:368-374
//   keepKeyFreshSending        send.go:213-227 (called at :523), with the goto top of :419-420
//   keepKeyFreshReceiving      receive.go:80-91 (called at :486-488)
//   SendHandshakeResponse      send.go:131-133, its lastSentHandshake alone
//   SendHandshakeInitiation    send.go:84-100, up to CreateMessageInitiation
// The five per-entry calls are bodies over the sources of wgcs_events.h, which
// wgcs_each.h runs one lane per entry; rekey_kernels.hip runs the start call one
// lane per row, rekey.cpp all of it in row order, and the stand-alone sanitizer
// program of tests/rekey_host/ includes this one text.
//
// The tables are those of include/wgcsum.h: one wgcs_rekey row beside every
// wgcs_keypairs row, found from a peer id through wgcs_peer_rows_build's rows.
// Every clock rule is now - x in signed 64 bits against a constant, so a clock
// that went back fires no rule and, in the start call, counts as "within the
// timeout".  Several rows of a call may belong to one peer: they only OR bits
// into want and flags, so the tables come out the same whichever ran first.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_events.h"

namespace wgcs {

static_assert(sizeof(wgcs_rekey) == 16 && sizeof(wgcs_hs_start) == 96 && sizeof(wgcs_hs_peer) == 64, "row layouts");

WGCS_HD void rekey_want_or(wgcs_rekey* r, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(&r->want, bits);
#else
  r->want |= bits;
#endif
}

// ---- the receive gate, receive.go:162-170 ----

WGCS_HD bool rekey_ref_receives(const wgcs_keypair_ref* r, uint32_t key) {
  return (r->flags & WGCS_KEYPAIR_SET) && r->recv_key == key;
}

// Row i's key is the receive key of one of its peer's three keypairs, and that keypair is past
// RejectAfterTime (createdAt.Add(RejectAfterTime).Before(now): equality passes): the packet is
// turned away.  src reads pkts[i].key and only lane i writes it, behind its own read.
struct RekeyRecvGate {
  KeyRows src;
  int64_t now;
  const wgcs_keypairs* kp;
  wgcs_aead_pkt* pkts;  // src.pkts
  WGCS_HD void operator()(uint32_t i) const {
    const uint32_t row = src.row(i);
    if (row == WGCS_PEER_NONE) return;
    const uint32_t key = src.key(i);
    const wgcs_keypairs* const k = kp + row;
    const wgcs_keypair_ref* ref = nullptr;  // sessions.Get(receiver).keypair
    if (rekey_ref_receives(&k->current, key)) ref = &k->current;
    else if (rekey_ref_receives(&k->previous, key)) ref = &k->previous;
    else if (rekey_ref_receives(&k->next, key)) ref = &k->next;
    if (ref && now - ref->created_ns > WGCS_REJECT_AFTER_TIME_NS) pkts[i].key = WGCS_SESSION_EXPIRED;
  }
};

// ---- the send side: the gate in front of send-assign and keepKeyFreshSending behind it ----

// send.go:369-371 for peer row `row`: the reasons its current keypair cannot send, 0 for one that can.
// The staged queue's release asks the same question per row (wgcs_staged.h).
WGCS_HD uint32_t rekey_gate_want(uint32_t row, int64_t now, const wgcs_keypairs* kp, const uint64_t* send_nonce,
                                 uint32_t n_keys, uint64_t limit) {
  const wgcs_keypair_ref* const cur = &kp[row].current;
  if (!(cur->flags & WGCS_KEYPAIR_SET)) return WGCS_REKEY_WANT_NO_KEYPAIR;  // :369
  const uint32_t key = cur->send_key;
  if (key >= n_keys) return 0;  // no nonce to read: send-assign's business
  uint32_t w = 0;
  if (send_nonce[key] >= limit) w |= WGCS_REKEY_WANT_REJECT_MESSAGES;                      // :370
  if (now - cur->created_ns >= WGCS_REJECT_AFTER_TIME_NS) w |= WGCS_REKEY_WANT_REJECT_TIME;  // :371
  return w;
}

// send.go:368-374: what send-assign reads as job j's status.  status_out may be src.status: a
// lane reads its own word and then writes it.
struct RekeySendGate {
  JobRows src;
  int64_t now;
  const wgcs_keypairs* kp;
  const uint64_t* send_nonce;
  uint32_t n_keys;
  uint64_t limit;
  wgcs_rekey* rekey;
  int32_t* status_out;
  WGCS_HD void operator()(uint32_t j) const {
    int32_t st = src.status[j];
    const uint32_t row = src.row(j);
    const uint32_t w = row == WGCS_PEER_NONE ? 0u : rekey_gate_want(row, now, kp, send_nonce, n_keys, limit);
    if (w != 0) {
      rekey_want_or(rekey + row, w);  // :372
      st = WGCS_ERR_KEY_EXPIRED;      // :373: the job stays staged
    }
    status_out[j] = st;
  }
};

// keepKeyFreshSending (send.go:213-227) for a kept job, the goto top of :419-420 for a dropped one
struct RekeySent {
  JobRows src;
  const uint32_t* job_key;
  int64_t now;
  const wgcs_keypairs* kp;
  const uint64_t* send_nonce;
  uint32_t n_keys;
  uint64_t limit;
  wgcs_rekey* rekey;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = src.row(j);
    if (row == WGCS_PEER_NONE) return;
    const wgcs_keypair_ref* const cur = &kp[row].current;
    if (!(cur->flags & WGCS_KEYPAIR_SET)) return;  // :215-217
    const bool has_nonce = cur->send_key < n_keys;
    const uint64_t nonce = has_nonce ? send_nonce[cur->send_key] : 0;
    uint32_t w = 0;
    if (job_kept(job_key, j)) {
      if (nonce > WGCS_REKEY_AFTER_MESSAGES) w |= WGCS_REKEY_WANT_REKEY_MESSAGES;  // :223
      if ((cur->flags & WGCS_KEYPAIR_INITIATOR) && now - cur->created_ns > WGCS_REKEY_AFTER_TIME_NS)
        w |= WGCS_REKEY_WANT_REKEY_TIME;  // :224
    } else if (has_nonce && nonce >= limit) {
      w |= WGCS_REKEY_WANT_REJECT_MESSAGES;  // :385-390, :419-420 and then :370
    }
    if (w) rekey_want_or(rekey + row, w);
  }
};

// ---- keepKeyFreshReceiving, receive.go:80-91, for one row of the write builder's groups ----

struct RekeyReceived {
  GroupRows src;
  int64_t now;
  const wgcs_keypairs* kp;
  wgcs_rekey* rekey;
  WGCS_HD void operator()(uint32_t c) const {
    const uint32_t row = src.row(c);  // receive.go:486: no valid tail packet, no call
    if (row == WGCS_PEER_NONE) return;
    const wgcs_keypair_ref* const cur = &kp[row].current;
    const uint32_t both = WGCS_KEYPAIR_SET | WGCS_KEYPAIR_INITIATOR;
    if ((cur->flags & both) != both) return;  // :85-86
    if (!(now - cur->created_ns > WGCS_REJECT_AFTER_TIME_NS - WGCS_KEEPALIVE_TIMEOUT_NS - WGCS_REKEY_TIMEOUT_NS))
      return;  // :87
    wgcs_rekey* const r = rekey + row;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t old = atomicOr(&r->flags, WGCS_REKEY_LAST_MINUTE);  // :81, :88
#else
    const uint32_t old = r->flags;
    r->flags = old | WGCS_REKEY_LAST_MINUTE;
#endif
    if (!(old & WGCS_REKEY_LAST_MINUTE)) rekey_want_or(r, WGCS_REKEY_WANT_LAST_MINUTE);  // :89
  }
};

// ---- SendHandshakeResponse's lastSentHandshake, send.go:131-133 ----

struct RekeyResponded {
  RespondedRows src;
  int64_t now;
  wgcs_rekey* rekey;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = src.row(j);
    if (row != WGCS_PEER_NONE) rekey[row].last_sent_ns = now;
  }
};

// ---- SendHandshakeInitiation, send.go:84-100, over the peer rows in three passes ----

// The first pass, peer row r: WGCS_HS_NONE, WGCS_ERR_REKEY_TIMEOUT (the request is dropped, :89-98),
// or WGCS_HS_STARTED for a candidate, which the last pass confirms or turns into WGCS_ERR_BATCH_FULL.
WGCS_HD int rekey_start_verdict(uint32_t r, int64_t now, wgcs_rekey* rekey, uint32_t* reasons) {
  wgcs_rekey* const k = rekey + r;
  const uint32_t w = k->want;
  reasons[r] = w;
  if (w == 0) return WGCS_HS_NONE;
  if (now - k->last_sent_ns < WGCS_REKEY_TIMEOUT_NS) {
    k->want = 0;
    return WGCS_ERR_REKEY_TIMEOUT;
  }
  return WGCS_HS_STARTED;
}

// The last pass, for the candidate r that rank candidates precede: its status.  A candidate with
// a ticket takes it (:99) and writes its descriptor; one without leaves its row as it was.
WGCS_HD int rekey_start_commit(uint32_t r, uint32_t rank, int64_t now, wgcs_rekey* rekey, const wgcs_hs_peer* hs_peers,
                               const wgcs_hs_start* tickets, uint32_t n_tickets, wgcs_hs_start* start,
                               uint32_t* start_peer) {
  if (rank >= n_tickets) return WGCS_ERR_BATCH_FULL;
  rekey[r].last_sent_ns = now;
  rekey[r].want = 0;
  start_peer[rank] = r;
  const uint32_t* const t = (const uint32_t*)(tickets + rank);  // 96 B, 4-byte aligned
  const uint32_t* const p = (const uint32_t*)(hs_peers + r);     // 64 B: flags at word 6, cookie at words 9..12
  uint32_t* const d = (uint32_t*)(start + rank);
  const bool cookie = (p[6] & WGCS_HS_PEER_COOKIE) != 0;
  d[0] = t[0];  // state_row
  d[1] = r;     // peer_row
  d[2] = t[2];  // local_index
  d[3] = t[3];  // send_key
  d[4] = t[4];  // recv_key
  d[5] = cookie ? WGCS_HS_START_COOKIE : 0u;
  d[6] = t[6], d[7] = t[7], d[8] = t[8];  // timestamp
  d[9] = 0;                               // pad0
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 10; i < 18; ++i) d[i] = t[i];  // ephemeral_private
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < 4; ++i) d[18 + i] = cookie ? p[9 + i] : 0u;
  d[22] = d[23] = 0;  // pad1
  return WGCS_HS_STARTED;
}

// descriptor k past the count: nothing for wgcs_handshake_initiate_batch to do, and no secret in it
WGCS_HD void rekey_start_tail(uint32_t k, wgcs_hs_start* start, uint32_t* start_peer) {
  uint32_t* const d = (uint32_t*)(start + k);
  d[0] = 0xFFFFFFFFu;  // state_row past every table
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 1; i < sizeof(wgcs_hs_start) / 4; ++i) d[i] = 0;
  start_peer[k] = WGCS_PEER_NONE;
}

}  // namespace wgcs
