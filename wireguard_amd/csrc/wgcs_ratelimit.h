// wgcs_ratelimit.h -- the rate limiter of ratelimiter/ratelimiter.go as scalar row
// functions, shared by host and device: the key of a source address and its home
// slot, the probe of the open-addressed table, the closed form of the m Allow
// calls one address gets under one clock value, and the three passes of a batch
//   find or claim    one row: the slot of its address, claimed if it has none
//   position         one position of the rows grouped by slot: verdicts and the entry
//   cleanup          one old slot: re-inserted into the new table unless it is idle
// ratelimit_kernels.hip runs them one lane per row, ratelimit.cpp in row order,
// and the stand-alone sanitizer program of tests/ratelimit_host/ includes this
// one text.
//
// Who touches what inside a batch call.  In the first pass the only word of the
// table that is written is `state`, by a compare-and-swap from 0 to
// WGCS_RL_CLAIMED | row, and it is read by an agent-scope atomic load; ip and
// family of a live entry were written by an earlier launch.  A claimed slot
// holds no key yet: whoever meets it compares its own key with the claiming
// row's d_src, an input nobody writes.  So no row ever waits for another one.
// In the last pass the first row of a slot's run is the only one that reads or
// writes the slot's entry, and it writes the verdicts of the run's first five
// rows; a row further back in its run writes its own refusal and reads nothing
// of the table.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/wgcsum.h"
#include "wgcs_route_walk.h"  // WGCS_HD

namespace wgcs {

static_assert(sizeof(wgcs_rl_entry) == 40 && offsetof(wgcs_rl_entry, state) == 16 &&
                  offsetof(wgcs_rl_entry, tokens) == 24,
              "row layout");
static_assert(sizeof(wgcs_src_addr) == 20, "row layout");

constexpr int64_t kRlPacketCost = WGCS_RL_PACKET_COST_NS, kRlMaxTokens = WGCS_RL_MAX_TOKENS_NS;
constexpr int64_t kRlCleanupNs = WGCS_RL_CLEANUP_NS;
constexpr uint32_t kRlBurst = 5;  // packetsBurst: no address passes more rows in one call
constexpr uint32_t kRlLive = 1, kRlMaxSlots = 1u << 24, kRlMaxRows = 1u << 24;
enum { kRlPassed = 0, kRlLimited = 1, kRlTableFull = 2, kRlCreated = 3, kRlStats = 4 };

inline bool rl_slots_ok(uint32_t n_slots) { return n_slots && !(n_slots & (n_slots - 1)) && n_slots <= kRlMaxSlots; }

struct RlKey {
  uint32_t family;  // 4 or 16
  uint32_t w[4];    // the 16 key bytes as LE32 words
};

// The key of a source address: false for a len that is neither 6 nor 18.  The row is 4-byte
// aligned on the device; the host reads it bytewise.
WGCS_HD bool rl_key_of(const wgcs_src_addr* s, RlKey* k) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t* p = (const uint32_t*)s;
  const uint32_t len = (p[4] >> 16) & 0xFF;
  k->w[0] = p[0];
  if (len == 6) {
    k->family = 4;
    k->w[1] = k->w[2] = k->w[3] = 0;
    return true;
  }
  k->family = 16;
  k->w[1] = p[1];
  k->w[2] = p[2];
  k->w[3] = p[3];
  return len == 18;
#else
  k->w[0] = k->w[1] = k->w[2] = k->w[3] = 0;
  if (s->len == 6) {
    k->family = 4;
    memcpy(k->w, s->b, 4);
    return true;
  }
  k->family = 16;
  if (s->len != 18) return false;
  memcpy(k->w, s->b, 16);
  return true;
#endif
}

// include/wgcsum.h spells this mix out; tests build colliding addresses through the export
WGCS_HD uint32_t rl_home(const RlKey& k, uint32_t n_slots) {
  uint32_t h = 0x811C9DC5u ^ k.family;
  for (int i = 0; i < 4; ++i) {
    h = (h ^ k.w[i]) * 0x01000193u;
    h ^= h >> 15;
  }
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h & (n_slots - 1);
}

WGCS_HD bool rl_key_eq(const RlKey& a, const RlKey& b) {
  return a.family == b.family && a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3];
}

// the key a live entry holds (the row is 8-byte aligned)
WGCS_HD RlKey rl_entry_key(const wgcs_rl_entry* e) {
  RlKey k;
  const uint32_t* p = (const uint32_t*)e->ip;
  k.family = e->family;
  k.w[0] = p[0];
  k.w[1] = p[1];
  k.w[2] = p[2];
  k.w[3] = p[3];
  return k;
}

WGCS_HD void rl_entry_fill(wgcs_rl_entry* e, const RlKey& k, int64_t tokens, int64_t now) {
  uint32_t* p = (uint32_t*)e->ip;
  p[0] = k.w[0];
  p[1] = k.w[1];
  p[2] = k.w[2];
  p[3] = k.w[3];
  e->family = k.family;
  e->tokens = tokens;
  e->last_ns = now;
}

// `state` as another row may have just changed it
WGCS_HD uint32_t rl_state_load(const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// *p: 0 -> want; the word before
WGCS_HD uint32_t rl_state_cas(uint32_t* p, uint32_t want) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(p, 0u, want);
#else
  const uint32_t old = *p;
  if (old == 0) *p = want;
  return old;
#endif
}

// Does a slot whose state reads `st` (not 0) hold the key k?  A live slot is compared by its
// entry, a claimed one by the source row of the row that claimed it.
WGCS_HD bool rl_slot_holds(const wgcs_rl_entry* e, uint32_t st, const RlKey& k, const wgcs_src_addr* src, uint32_t n) {
  if (st == kRlLive) return rl_key_eq(rl_entry_key(e), k);
  const uint32_t owner = st & ~WGCS_RL_CLAIMED;
  RlKey other;
  return (st & WGCS_RL_CLAIMED) && owner < n && rl_key_of(src + owner, &other) && rl_key_eq(other, k);
}

// ---- the closed form of m Allow calls under one clock value ----

struct RlOutcome {
  uint32_t pass;   // the first `pass` rows are allowed
  int64_t tokens;  // what the entry holds afterwards
};

// an entry that was found, :110-125; m >= 1 (rows past the fifth change nothing)
WGCS_HD RlOutcome rl_known(int64_t tokens, int64_t last_ns, int64_t now, uint32_t m) {
  int64_t t0 = tokens + (now - last_ns);
  if (t0 > kRlMaxTokens) t0 = kRlMaxTokens;
  const uint32_t a = t0 >= kRlPacketCost ? (uint32_t)(t0 / kRlPacketCost) : 0;  // <= 5
  RlOutcome o;
  o.pass = m < a ? m : a;
  o.tokens = t0 - (int64_t)o.pass * kRlPacketCost;
  return o;
}

// an address that was not found: :96-108 for the first row, then rl_known on maxTokens - packetCost
WGCS_HD RlOutcome rl_fresh(uint32_t m) {
  const uint32_t more = m - 1 < kRlBurst - 1 ? m - 1 : kRlBurst - 1;
  RlOutcome o;
  o.pass = 1 + more;
  o.tokens = (int64_t)(kRlBurst - 1 - more) * kRlPacketCost;
  return o;
}

// ---- pass 1: find or claim ----

// One probe step of row q with key k at slot s: 1 the slot is the row's (live, claimed by a row
// of its address, or claimed now), 0 go on to the next slot.  `cas` is false on a device lane's
// first look at an empty slot that its neighbour lane is about to claim (ratelimit_kernels.hip);
// then the answer is -1: look at this slot again.
WGCS_HD int rl_probe_step(wgcs_rl_entry* table, uint32_t s, uint32_t q, const RlKey& k, const wgcs_src_addr* src,
                          uint32_t n, bool cas) {
  wgcs_rl_entry* e = table + s;
  uint32_t st = rl_state_load(&e->state);
  if (st == 0) {
    if (!cas) return -1;
    st = rl_state_cas(&e->state, WGCS_RL_CLAIMED | q);
    if (st == 0) return 1;
  }
  return rl_slot_holds(e, st, k, src, n) ? 1 : 0;
}

// Row q of a batch: its slot, or n_slots for a row that is not charged -- the gate is not a
// pass, the len is bad (WGCS_ERR_INVALID_ARG), or the address is new and no slot is free
// (WGCS_ERR_RATE_TABLE_FULL, *full set) -- whose verdict is final and written here.  verdict
// may be gate: the row reads its own word first.
WGCS_HD uint32_t rl_find_or_claim(uint32_t q, const int32_t* gate, const wgcs_src_addr* src, uint32_t n,
                                  wgcs_rl_entry* table, uint32_t n_slots, int32_t* verdict, bool* full) {
  const int32_t g = gate[q];
  RlKey k;
  if (g != WGCS_HS_PASS) {
    verdict[q] = g;
    return n_slots;
  }
  if (!rl_key_of(src + q, &k)) {
    verdict[q] = WGCS_ERR_INVALID_ARG;
    return n_slots;
  }
  uint32_t s = rl_home(k, n_slots);
  for (uint32_t i = 0; i < n_slots; ++i, s = (s + 1) & (n_slots - 1))
    if (rl_probe_step(table, s, q, k, src, n, true) > 0) return s;
  verdict[q] = WGCS_ERR_RATE_TABLE_FULL;
  *full = true;
  return n_slots;
}

// ---- pass 2: verdicts and entries ----

// Position p of the rows in (slot, row) order.  counts: what this position adds to d_stats.
WGCS_HD void rl_position(uint32_t p, const uint32_t* keys, const uint32_t* slots, uint32_t n, uint32_t n_slots,
                         const wgcs_src_addr* src, wgcs_rl_entry* table, int64_t now, int32_t* verdict,
                         uint32_t counts[kRlStats]) {
  const uint32_t key = keys[p];
  if (key >= n_slots) return;  // pass 1 wrote the verdict
  if (p > 0 && keys[p - 1] == key) {
    // not the first of its run: the fifth row behind it tells whether it is past the burst
    if (p >= kRlBurst && keys[p - kRlBurst] == key) {
      verdict[slots[p]] = WGCS_ERR_RATE_LIMITED;
      counts[kRlLimited] += 1;
    }
    return;
  }
  uint32_t m = 1;  // min(rows of the run, 5)
  while (m < kRlBurst && p + m < n && keys[p + m] == key) ++m;
  wgcs_rl_entry* e = table + key;
  RlOutcome o;
  if (e->state == kRlLive) {
    o = rl_known(e->tokens, e->last_ns, now, m);
    e->tokens = o.tokens;
    e->last_ns = now;
  } else {  // claimed in pass 1 by a row of this run
    RlKey k;
    rl_key_of(src + slots[p], &k);
    o = rl_fresh(m);
    rl_entry_fill(e, k, o.tokens, now);
    e->state = kRlLive;
    counts[kRlCreated] += 1;
  }
  for (uint32_t i = 0; i < m; ++i) verdict[slots[p + i]] = i < o.pass ? WGCS_HS_PASS : WGCS_ERR_RATE_LIMITED;
  counts[kRlPassed] += o.pass;
  counts[kRlLimited] += m - o.pass;
}

// ---- cleanup, :77-89 ----

// Old slot i: true and inserted into the new table when it is live and not idle.  Keys are
// unique, so the first slot of the probe that this row turns from 0 to 1 is its own.
WGCS_HD bool rl_cleanup_row(uint32_t i, const wgcs_rl_entry* old_table, wgcs_rl_entry* new_table, uint32_t n_slots,
                            int64_t now) {
  const wgcs_rl_entry* e = old_table + i;
  if (e->state != kRlLive || now - e->last_ns > kRlCleanupNs) return false;
  const RlKey k = rl_entry_key(e);
  uint32_t s = rl_home(k, n_slots);
  for (uint32_t j = 0; j < n_slots; ++j, s = (s + 1) & (n_slots - 1)) {
    wgcs_rl_entry* d = new_table + s;
    if (rl_state_load(&d->state) == 0 && rl_state_cas(&d->state, kRlLive) == 0) {
      rl_entry_fill(d, k, e->tokens, e->last_ns);
      return true;
    }
  }
  return false;  // not reached: the new table has a slot for every old one
}

}  // namespace wgcs
