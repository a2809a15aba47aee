// wgcs_timers.h -- the peer timers as scalar row functions, shared by host and
// device: the Timer of device/timers.go:11-71 as a bit and a deadline, the hooks
// of timers.go:189-295 as the sites that call them name them
//   sent         send.go:498-510            traversal, packet sent, data sent
//   received     receive.go:486-494         traversal, packet received, data received
//   initiated    send.go:85-87, :117-126    !isRetry, then traversal, packet sent, initiated
//   responded    receive.go:311-312 and send.go:158-160
//   finished     receive.go:339-348         ... session derived, complete, SendKeepalive
//   rotated      receive.go:422-427         complete
// and the five expiry bodies of timers.go:73-144 with peer.go:246-251.
// The event calls are bodies over the sources of wgcs_events.h, which wgcs_each.h
// runs one lane per entry; timers_kernels.hip runs the expiry one lane per row,
// timers.cpp all of it in row order, and the stand-alone sanitizer program of
// tests/timers_host/ includes this one text.
//
// Several rows of an event call may belong to one peer.  They OR bits into or
// AND bits out of pending and flags, never both for one bit in one call, and
// every plain store writes a value all rows of the peer agree on (the call's
// clock plus a constant, plus a jitter that depends on the peer row alone), so
// the table comes out the same whichever lane ran first.  The expire call has
// one lane per peer row, which owns its rows of every table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_events.h"
#include "wgcs_keypairs.h"
#include "wgcs_rekey.h"

namespace wgcs {

static_assert(sizeof(wgcs_timers) == 64 && offsetof(wgcs_timers, pending) == 48, "row layout");

constexpr int64_t kTimersSecondNs = 1000000000ll;
constexpr int64_t kTimersMsNs = 1000000ll;

// rand.Int64N(RekeyTimeoutJitterMaxMs) of timers.go:204 and :271, drawn from (seed, row): the
// finalizer of MurmurHash3 over seed ^ row * 0x9E3779B9, scaled into [0, 334) by a multiply
WGCS_HD uint32_t timers_jitter_ms(uint32_t seed, uint32_t row) {
  uint32_t x = seed ^ (row * 0x9E3779B9u);
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return (uint32_t)(((uint64_t)x * WGCS_TIMERS_JITTER_MAX_MS) >> 32);
}

// *p |= bits, *p &= mask: the word before.  On the device a plain look comes first, as in
// keypairs_received_claim: a batch brings many rows of one peer, no call both sets and clears one
// bit, so a bit that reads as wanted stays so, and the atomic unit sees a lane per change, not per row.
WGCS_HD uint32_t timers_or(uint32_t* p, uint32_t bits) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t seen = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (seen & bits) == bits ? seen : atomicOr(p, bits);
#else
  const uint32_t old = *p;
  *p = old | bits;
  return old;
#endif
}

WGCS_HD uint32_t timers_and(uint32_t* p, uint32_t mask) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t seen = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return (seen & ~mask) == 0 ? seen : atomicAnd(p, mask);
#else
  const uint32_t old = *p;
  *p = old & mask;
  return old;
#endif
}

// ---- Timer, timers.go:42-71 ----

// now + d without signed overflow for any input; the caller keeps the values where no wrap happens
WGCS_HD int64_t timers_after(int64_t now, uint64_t d) { return (int64_t)((uint64_t)now + d); }

WGCS_HD void timer_mod(wgcs_timers* t, uint32_t i, int64_t now, uint64_t d) {
  timers_or(&t->pending, 1u << i);
  const int64_t when = timers_after(now, d);
  if (t->deadline_ns[i] != when) t->deadline_ns[i] = when;  // every row of the peer stores this value: once is enough
}

// if !IsPending() { Mod(d) }: true for the row that armed it
WGCS_HD bool timer_mod_if_idle(wgcs_timers* t, uint32_t i, int64_t now, uint64_t d) {
  if (timers_or(&t->pending, 1u << i) & (1u << i)) return false;
  t->deadline_ns[i] = timers_after(now, d);
  return true;
}

WGCS_HD void timer_del(wgcs_timers* t, uint32_t i) { timers_and(&t->pending, ~(1u << i)); }

WGCS_HD bool timers_active(const wgcs_timers* t) { return (t->flags & WGCS_TIMERS_ACTIVE) != 0; }  // :168-170

// ---- the hooks, timers.go:189-295 ----

WGCS_HD void timers_traversal(wgcs_timers* t, int64_t now) {  // :259-264
  const uint32_t keepalive = t->keepalive_interval_s;
  if (keepalive > 0 && timers_active(t)) timer_mod(t, WGCS_TIMER_KEEPALIVE, now, (uint64_t)keepalive * kTimersSecondNs);
}

WGCS_HD void timers_packet_sent(wgcs_timers* t) {  // :249-253
  if (timers_active(t)) timer_del(t, WGCS_TIMER_SEND_KEEPALIVE);
}

WGCS_HD void timers_packet_received(wgcs_timers* t) {  // :226-230
  if (timers_active(t)) timer_del(t, WGCS_TIMER_NEW_HANDSHAKE);
}

WGCS_HD void timers_data_sent(wgcs_timers* t, int64_t now, uint32_t jitter_ms) {  // :189-221
  if (timers_active(t))
    timer_mod_if_idle(t, WGCS_TIMER_NEW_HANDSHAKE, now,
                      (uint64_t)(WGCS_KEEPALIVE_TIMEOUT_NS + WGCS_REKEY_TIMEOUT_NS + jitter_ms * kTimersMsNs));
}

WGCS_HD void timers_data_received(wgcs_timers* t, int64_t now) {  // :235-244
  if (!timers_active(t)) return;
  if (!timer_mod_if_idle(t, WGCS_TIMER_SEND_KEEPALIVE, now, (uint64_t)WGCS_KEEPALIVE_TIMEOUT_NS))
    timers_or(&t->flags, WGCS_TIMERS_NEED_ANOTHER);
}

WGCS_HD void timers_handshake_initiated(wgcs_timers* t, int64_t now, uint32_t jitter_ms) {  // :268-274
  if (timers_active(t))
    timer_mod(t, WGCS_TIMER_RESEND_HANDSHAKE, now, (uint64_t)(WGCS_REKEY_TIMEOUT_NS + jitter_ms * kTimersMsNs));
}

WGCS_HD void timers_session_derived(wgcs_timers* t, int64_t now) {  // :291-295
  if (timers_active(t)) timer_mod(t, WGCS_TIMER_ZERO_OUT_KEYS, now, (uint64_t)WGCS_TIMERS_ZERO_KEYS_NS);
}

WGCS_HD void timers_handshake_complete(wgcs_timers* t, wgcs_rekey* r, int64_t now) {  // :279-286
  if (timers_active(t)) timer_del(t, WGCS_TIMER_RESEND_HANDSHAKE);
  t->attempts = 0;
  timers_and(&r->flags, ~WGCS_REKEY_LAST_MINUTE);
  t->last_handshake_ns = now;
}

// ---- the event calls: one body each over its source (wgcs_events.h), entry i ----

struct TimersSent {  // send.go:498-510 for job j of a send-assign batch
  KeptJobRows src;
  const int32_t* sizes;
  int64_t now;
  uint32_t seed;
  wgcs_timers* timers;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = src.row(j);  // a dropped job: nothing was sent
    if (row == WGCS_PEER_NONE) return;
    bool data_sent = false;  // :498-502: a keepalive's slot has size 0
    const int32_t* const sz = sizes + (uint64_t)j * src.jobs.max_segs;
    for (int32_t k = 0; k < src.jobs.count[j]; ++k) data_sent |= sz[k] != 0;
    wgcs_timers* const t = timers + row;
    timers_traversal(t, now);  // :505
    timers_packet_sent(t);     // :506
    if (data_sent) timers_data_sent(t, now, timers_jitter_ms(seed, row));  // :508-510
  }
};

struct TimersReceived {  // receive.go:486-494 for row c of the write builder's groups
  GroupRows src;
  int64_t now;
  wgcs_timers* timers;
  WGCS_HD void operator()(uint32_t c) const {
    const uint32_t row = src.row(c);  // :486
    if (row == WGCS_PEER_NONE) return;
    wgcs_timers* const t = timers + row;
    timers_traversal(t, now);   // :489
    timers_packet_received(t);  // :490
    if (src.flags(c) & WGCS_GROUP_DATA) timers_data_received(t, now);  // :492-494
  }
};

struct TimersFresh {  // send.go:85-87 for peer row r of the start call
  const uint32_t* reasons;
  wgcs_timers* timers;
  WGCS_HD void operator()(uint32_t r) const {
    if (reasons[r] & ~WGCS_REKEY_WANT_RETRY) timers[r].attempts = 0;
  }
};

struct TimersInitiated {  // send.go:117-126 for ticket k of the start call, once initiate has built its message
  TicketRows src;
  int64_t now;
  uint32_t seed;
  wgcs_timers* timers;
  WGCS_HD void operator()(uint32_t k) const {
    const uint32_t row = src.row(k);
    if (row == WGCS_PEER_NONE) return;
    wgcs_timers* const t = timers + row;
    timers_traversal(t, now);                                          // :117
    timers_packet_sent(t);                                             // :118
    timers_handshake_initiated(t, now, timers_jitter_ms(seed, row));   // :126
  }
};

struct TimersResponded {  // receive.go:311-312 and send.go:158-160 for descriptor j of a respond batch
  RespondedRows src;
  int64_t now;
  wgcs_timers* timers;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = src.row(j);
    if (row == WGCS_PEER_NONE) return;
    wgcs_timers* const t = timers + row;
    timers_traversal(t, now);        // receive.go:311
    timers_packet_received(t);       // :312
    timers_session_derived(t, now);  // send.go:158
    timers_traversal(t, now);        // :159
    timers_packet_sent(t);           // :160
  }
};

struct TimersFinished {  // receive.go:339-348 for row q of a begin-initiator batch
  FinishedRows src;
  const int32_t* begun;
  int64_t now;
  wgcs_timers* timers;
  wgcs_rekey* rekey;
  WGCS_HD void operator()(uint32_t q) const {
    if (begun[q] != WGCS_HS_BEGUN) return;  // :342-345: goto skip
    const uint32_t row = src.row(q);
    if (row == WGCS_PEER_NONE) return;
    wgcs_timers* const t = timers + row;
    timers_traversal(t, now);                          // :339
    timers_packet_received(t);                         // :340
    timers_session_derived(t, now);                    // :346
    timers_handshake_complete(t, rekey + row, now);    // :347
    timers_or(&t->flags, WGCS_TIMERS_KEEPALIVE_NOW);   // :348
  }
};

struct TimersRotated {  // receive.go:422-427 for row i of a keypairs-received batch
  KeyRows src;
  const uint32_t* rotated;
  int64_t now;
  wgcs_timers* timers;
  wgcs_rekey* rekey;
  WGCS_HD void operator()(uint32_t i) const {
    if (rotated[i] != 1) return;
    const uint32_t row = src.row(i);
    if (row == WGCS_PEER_NONE) return;
    timers_handshake_complete(timers + row, rekey + row, now);  // :426
  }
};

// ---- expiry, timers.go:73-144, over the peer rows in three passes ----

// peer.go:246-251 for peer row r, and the send chain's key of the peer
WGCS_HD void timers_zero_keys(uint32_t r, const wgcs_peer_key* table, wgcs_keypairs* kp, wgcs_session_slot* slots,
                              uint32_t n_slots, wgcs_session_slot* peer_keys, uint32_t n_peer_slots,
                              wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys) {
  wgcs_keypairs* const k = kp + r;
  delete_session(k->current, slots, n_slots, keys, key_peer, n_keys);   // :246
  delete_session(k->previous, slots, n_slots, keys, key_peer, n_keys);  // :247
  delete_session(k->next, slots, n_slots, keys, key_peer, n_keys);      // :248
  keypair_ref_clear(&k->current);                                       // :249
  keypair_ref_clear(&k->previous);                                      // :250
  keypair_ref_clear(&k->next);                                          // :251
  session_set_key(peer_keys, n_peer_slots, table[r].peer, WGCS_SESSION_NO_KEYPAIR);
}

// The first pass, peer row r: every due timer's body in the order of the deadlines, and d_actions[r]
// with WGCS_TIMERS_ACT_KEEPALIVE for a row that owes a keepalive job (the value returned), which the
// last pass confirms or turns into WGCS_TIMERS_ACT_DEFERRED.
WGCS_HD bool timers_expire_verdict(uint32_t r, int64_t now, wgcs_timers* timers, wgcs_rekey* rekey,
                                  const wgcs_peer_key* table, const uint32_t* staged, wgcs_keypairs* kp,
                                  wgcs_session_slot* slots, uint32_t n_slots, wgcs_session_slot* peer_keys,
                                  uint32_t n_peer_slots, wgcs_aead_key* keys, uint32_t* key_peer, uint32_t n_keys,
                                  uint32_t* actions) {
  wgcs_timers* const t = timers + r;
  actions[r] = 0;
  uint32_t flags = t->flags;
  if (!(flags & WGCS_TIMERS_ACTIVE)) return false;
  // the lane owns the row: its words are worked on in registers and stored once
  uint32_t pending = t->pending, attempts = t->attempts, act = 0, want = 0;
  int64_t deadline[WGCS_TIMERS_COUNT];
  for (uint32_t i = 0; i < WGCS_TIMERS_COUNT; ++i) deadline[i] = t->deadline_ns[i];
  bool owed = (flags & WGCS_TIMERS_KEEPALIVE_NOW) != 0;
  for (uint32_t turn = 0; turn < WGCS_TIMERS_COUNT; ++turn) {
    uint32_t due = WGCS_TIMERS_COUNT;  // the pending timer with the earliest deadline <= now, the lowest index of a tie
    for (uint32_t i = 0; i < WGCS_TIMERS_COUNT; ++i)
      if ((pending >> i & 1u) && deadline[i] <= now && (due == WGCS_TIMERS_COUNT || deadline[i] < deadline[due])) due = i;
    if (due == WGCS_TIMERS_COUNT) break;
    pending &= ~(1u << due);  // timers.go:34: isPending = false, then expFunc
    act |= WGCS_TIMERS_ACT_FIRED(due);
    if (due == WGCS_TIMER_NEW_HANDSHAKE) {  // :73-82
      flags |= WGCS_TIMERS_CLEAR_SRC;
      want |= WGCS_REKEY_WANT_NEW_HANDSHAKE;
    } else if (due == WGCS_TIMER_RESEND_HANDSHAKE) {  // :84-115
      if (attempts > WGCS_TIMERS_MAX_ATTEMPTS) {
        pending &= ~(1u << WGCS_TIMER_SEND_KEEPALIVE);                   // :91-93; the row is active
        act |= WGCS_TIMERS_ACT_GAVE_UP | WGCS_TIMERS_ACT_FLUSH_STAGED;  // :96
        if (!(pending >> WGCS_TIMER_ZERO_OUT_KEYS & 1u)) {               // :99-101
          pending |= 1u << WGCS_TIMER_ZERO_OUT_KEYS;
          deadline[WGCS_TIMER_ZERO_OUT_KEYS] = timers_after(now, (uint64_t)WGCS_TIMERS_ZERO_KEYS_NS);
        }
      } else {
        attempts += 1;                   // :103
        flags |= WGCS_TIMERS_CLEAR_SRC;  // :112
        want |= WGCS_REKEY_WANT_RETRY;   // :113
      }
    } else if (due == WGCS_TIMER_SEND_KEEPALIVE) {  // :119-127
      owed = true;
      if (flags & WGCS_TIMERS_NEED_ANOTHER) {
        flags &= ~WGCS_TIMERS_NEED_ANOTHER;
        pending |= 1u << WGCS_TIMER_SEND_KEEPALIVE;
        deadline[WGCS_TIMER_SEND_KEEPALIVE] = timers_after(now, (uint64_t)WGCS_KEEPALIVE_TIMEOUT_NS);
      }
    } else if (due == WGCS_TIMER_KEEPALIVE) {  // :131-135
      if (t->keepalive_interval_s > 0) owed = true;
    } else {  // :137-144 and peer.go:241-260
      timers_zero_keys(r, table, kp, slots, n_slots, peer_keys, n_peer_slots, keys, key_peer, n_keys);
      act |= WGCS_TIMERS_ACT_ZEROED | WGCS_TIMERS_ACT_FLUSH_STAGED;
    }
  }
  if (want) rekey_want_or(rekey + r, want);
  if (owed && staged && staged[r] != 0) {  // send.go:194: the staged packets go out in its place
    flags &= ~WGCS_TIMERS_KEEPALIVE_NOW;
    owed = false;
  }
  if (act) {
    for (uint32_t i = 0; i < WGCS_TIMERS_COUNT; ++i) t->deadline_ns[i] = deadline[i];
    t->pending = pending;
    t->attempts = attempts;
  }
  t->flags = flags;
  actions[r] = act | (owed ? WGCS_TIMERS_ACT_KEEPALIVE : 0u);
  return owed;
}

// The last pass, for the owing row r that `rank` owing rows precede: job `rank` if there is room for it
WGCS_HD void timers_expire_commit(uint32_t r, uint32_t rank, wgcs_timers* timers, const wgcs_peer_key* table,
                                  uint32_t n_ka_max, uint32_t* ka_peer, int32_t* ka_count, int32_t* ka_sizes,
                                  int32_t* ka_status, uint32_t* actions) {
  wgcs_timers* const t = timers + r;
  if (rank >= n_ka_max) {
    t->flags |= WGCS_TIMERS_KEEPALIVE_NOW;
    actions[r] ^= WGCS_TIMERS_ACT_KEEPALIVE | WGCS_TIMERS_ACT_DEFERRED;
    return;
  }
  t->flags &= ~WGCS_TIMERS_KEEPALIVE_NOW;
  ka_peer[rank] = table[r].peer;
  ka_count[rank] = 1;
  ka_sizes[rank] = 0;
  ka_status[rank] = 0;
}

// job k past the count: send-assign drops it by its count
WGCS_HD void timers_expire_tail(uint32_t k, uint32_t* ka_peer, int32_t* ka_count, int32_t* ka_sizes,
                                int32_t* ka_status) {
  ka_peer[k] = WGCS_PEER_NONE;
  ka_count[k] = 0;
  ka_sizes[k] = 0;
  ka_status[k] = 0;
}

}  // namespace wgcs
