// wgcs_cookiegen.h -- the initiator's side of the cookie mechanism as scalar
// row functions, shared by host and device: CookieGenerator of device/cookie.go
//   sent       AddMACs' bookkeeping          cookie.go:301-302   lastMAC1, hasLastMAC1
//   consume    the cookie-reply case of RoutineHandshake with ConsumeReply
//                                            receive.go:246-269, cookie.go:319-339
//   age        the CookieRefreshTime rule    cookie.go:306
// Each pass is a body that wgcs_each.h runs one lane per row and cookiegen.cpp
// in row order, the recording calls over the sources of wgcs_events.h; the
// stand-alone sanitizer program of tests/cookiegen_host/ includes this one text.
//
// Several rows of a call may belong to one peer.  The reference takes them in
// turn, so the last one's 16 bytes stand; here every such row raises the peer's
// claim word to its row number + 1 in a first pass, and in a second pass the one
// row that holds the claim stores the 16 bytes and puts the claim back to 0.  No
// lane stores 16 bytes beside another lane that stores the same 16, and the
// tables come out the same whichever wave ran first.
//
// A wgcs_cookie_gen row and a wgcs_hs_peer row are read and written as sixteen
// 4-byte words each (both are 64 B, packed to 4): the word offsets are below.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_cookie.h"

#pragma push_macro("WGCS_HD")  // wgcs_route_walk.h defines its own, plain inline: keep the forced one of wgcs_poly1305.h
#undef WGCS_HD
#include "wgcs_events.h"  // and wgcs_route_walk.h's session_get
#pragma pop_macro("WGCS_HD")

namespace wgcs {

static_assert(sizeof(wgcs_cookie_gen) == 64 && offsetof(wgcs_cookie_gen, last_mac1) == 32 &&
                  offsetof(wgcs_cookie_gen, cookie_set_at_ns) == 48 && offsetof(wgcs_cookie_gen, flags) == 56 &&
                  offsetof(wgcs_cookie_gen, claim) == 60,
              "row layout");
static_assert(sizeof(wgcs_hs_peer) == 64 && offsetof(wgcs_hs_peer, flags) == 24 && offsetof(wgcs_hs_peer, cookie) == 36,
              "row layout");

constexpr uint32_t kGenKey = 0, kGenMac1 = 8, kGenSetAt = 12, kGenFlags = 14, kGenClaim = 15;  // words of wgcs_cookie_gen
constexpr uint32_t kHsPeerFlags = 6, kHsPeerCookie = 9;                                        // words of wgcs_hs_peer
constexpr uint32_t kCookieReplySize = 64;                // MessageCookieReplySize, device/noise.go:66
constexpr uint32_t kInitiationPitch = 160, kInitiationMac1 = 116;  // a row of wgcs_handshake_initiate_batch's d_msgs
constexpr uint32_t kResponsePitch = 96, kResponseMac1 = 60;        // a row of wgcs_handshake_respond_batch's d_msgs

WGCS_HD uint32_t* cookiegen_words(wgcs_cookie_gen* g) { return (uint32_t*)g; }
WGCS_HD const uint32_t* cookiegen_words(const wgcs_cookie_gen* g) { return (const uint32_t*)g; }
WGCS_HD uint32_t* cookiegen_words(wgcs_hs_peer* p) { return (uint32_t*)p; }

// ---- lastMAC1 behind initiate and respond, cookie.go:301-302, in two passes ----

// the MAC1 of message j of a 4-byte aligned d_msgs, as words, for the call's source
WGCS_HD const uint32_t* cookiegen_mac1(const InitiatedRows&, uint32_t j, const uint8_t* msgs) {
  return (const uint32_t*)(msgs + (uint64_t)kInitiationPitch * j + kInitiationMac1);
}

WGCS_HD const uint32_t* cookiegen_mac1(const RespondedRows&, uint32_t j, const uint8_t* msgs) {
  return (const uint32_t*)(msgs + (uint64_t)kResponsePitch * j + kResponseMac1);
}

// the first pass: descriptor j claims its peer's row
template <class Rows>
struct CookieSentClaim {
  Rows src;
  wgcs_cookie_gen* gen;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = src.row(j);
    if (row != WGCS_PEER_NONE) claim_max(cookiegen_words(gen + row) + kGenClaim, j + 1);
  }
};

// the second pass: the holder of the claim, the highest j of its peer, leaves its MAC1
template <class Rows>
struct CookieSentCommit {
  Rows src;
  const uint8_t* msgs;
  wgcs_cookie_gen* gen;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = src.row(j);
    if (row == WGCS_PEER_NONE) return;
    uint32_t* const g = cookiegen_words(gen + row);
    if (g[kGenClaim] != j + 1) return;  // a higher descriptor's, or 0 once that one has committed: never j + 1
    const uint32_t* const mac1 = cookiegen_mac1(src, j, msgs);
    // read whole, then stored: nothing tells the compiler that msgs and gen are apart
    const uint32_t m[4] = {mac1[0], mac1[1], mac1[2], mac1[3]};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4; ++i) g[kGenMac1 + i] = m[i];
    g[kGenFlags] |= WGCS_COOKIE_GEN_HAS_MAC1;
    g[kGenClaim] = 0;
  }
};

// ---- cookie replies, receive.go:246-269 and cookie.go:319-339, in two passes ----

// the sixteen words of the 64-byte message at p, which sits at any byte offset
WGCS_HD void cookiegen_load_reply(const uint8_t* p, uint32_t m[16]) {
#if defined(__HIP_DEVICE_COMPILE__)
  b2s_load_block(p, 0, kCookieReplySize, m);  // the aligned dwords that hold it
#else
  for (uint32_t i = 0; i < 16; ++i) m[i] = b2s_load_le32(p, 4 * i, kCookieReplySize);
#endif
}

// LE32 msg[4:8] of the message at p: msg.Receiver of a cookie reply
WGCS_HD uint32_t cookiegen_msg_receiver(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  // the one or two aligned words that hold the four bytes; both lie inside the 64-byte message
  const uint32_t sh = (uint32_t)(uintptr_t)(p + 4) & 3u;
  const uint32_t* const w = (const uint32_t*)(p + 4 - sh);
  const uint32_t lo = w[0];
  return sh ? __builtin_amdgcn_alignbyte(w[1], lo, sh) : lo;
#else
  return (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
#endif
}

// What the lookups of a row need.  The slot counts are 0 or a power of two.
struct CookieGenTables {
  const wgcs_session_slot* hs_slots;  // local index -> row of states: handshakes we initiated
  uint32_t n_hs_slots;
  const wgcs_hs_state* states;
  uint32_t n_states;
  const wgcs_session_slot* slots;  // local index -> key row: responses we sent
  uint32_t n_slots;
  const uint32_t* key_peer;  // key row -> peer id
  uint32_t n_keys;
  const uint32_t* peer_rows;  // peer id -> peer row
  uint32_t n_ids;
  uint32_t n_peers;
};

// d.indexTable.Lookup(reply.Receiver) and its peer (receive.go:255-259): the
// handshake that holds the index, else the keypair that does; WGCS_PEER_NONE for neither
WGCS_HD uint32_t cookiegen_peer_row(uint32_t receiver, const CookieGenTables& t) {
  const uint32_t st = session_get(t.hs_slots, t.n_hs_slots, receiver);  // empty is past any table
  if (st < t.n_states && t.states[st].local_index == receiver) {
    const uint32_t row = t.states[st].peer_row;
    return row < t.n_peers ? row : WGCS_PEER_NONE;
  }
  const uint32_t key = session_get(t.slots, t.n_slots, receiver);  // empty and WGCS_SESSION_NO_KEYPAIR are past any table
  if (key >= t.n_keys) return WGCS_PEER_NONE;
  const uint32_t id = t.key_peer[key];
  if (id >= t.n_ids) return WGCS_PEER_NONE;
  const uint32_t row = t.peer_rows[id];
  return row < t.n_peers ? row : WGCS_PEER_NONE;
}

// The first pass, row q: its verdict.  A reply that opens leaves its cookie in work[4q, 4q + 4)
// and claims its peer's row; nothing else is written.
struct CookieOpen {
  const uint8_t* arena;
  const wgcs_aead_pkt* pkts;
  const int32_t* types;
  CookieGenTables t;
  wgcs_cookie_gen* gen;
  uint32_t* work;
  int32_t* verdict;
  WGCS_HD void operator()(uint32_t q) const { verdict[q] = open(q); }
  WGCS_HD int32_t open(uint32_t q) const {
    if (types[q] != (int32_t)kCookieReplyType) return WGCS_HS_NONE;
    if (pkts[q].len != kCookieReplySize) return WGCS_ERR_INVALID_ARG;
    uint32_t m[16];
    cookiegen_load_reply(arena + pkts[q].off, m);
    if (m[0] != kCookieReplyType) return WGCS_ERR_INVALID_ARG;  // unmarshal, receive.go:249-253
    const uint32_t row = cookiegen_peer_row(m[1], t);
    if (row == WGCS_PEER_NONE) return WGCS_ERR_NO_PEER;  // :255-259
    uint32_t* const g = cookiegen_words(gen + row);
    if (!(g[kGenFlags] & WGCS_COOKIE_GEN_HAS_MAC1)) return WGCS_ERR_NO_HANDSHAKE;  // cookie.go:323-325
    uint32_t key[8], ad[4], pt[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 8; ++i) key[i] = g[kGenKey + i];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4; ++i) ad[i] = g[kGenMac1 + i];
    if (!xchacha_open16(key, m + 2, m + 8, m + 12, ad, pt)) return WGCS_ERR_AUTH;  // :326-335
    uint32_t* const w = work + 4 * (uint64_t)q;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4; ++i) w[i] = pt[i];
    claim_max(g + kGenClaim, q + 1);
    return WGCS_HS_COOKIE_KEPT;
  }
};

// The second pass, row q: the holder of its peer's claim, the highest row that opened, stores
// its cookie, the valid bit and the time (cookie.go:337-338); every row's work is zeroed.
struct CookieCommit {
  const uint8_t* arena;
  const wgcs_aead_pkt* pkts;
  const int32_t* verdict;
  CookieGenTables t;
  int64_t now;
  wgcs_cookie_gen* gen;
  wgcs_hs_peer* peers;
  uint32_t* work;
  WGCS_HD void operator()(uint32_t q) const {
    uint32_t* const w = work + 4 * (uint64_t)q;
    if (verdict[q] == WGCS_HS_COOKIE_KEPT) {
      // the row the first pass found: no table the lookup reads is written by either pass
      const uint32_t row = cookiegen_peer_row(cookiegen_msg_receiver(arena + pkts[q].off), t);
      if (row != WGCS_PEER_NONE) {
        uint32_t* const g = cookiegen_words(gen + row);
        if (g[kGenClaim] == q + 1) {  // else a higher row's, or 0 once that row has committed: never q + 1
          uint32_t* const p = cookiegen_words(peers + row);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
          for (uint32_t i = 0; i < 4; ++i) p[kHsPeerCookie + i] = w[i];
          p[kHsPeerFlags] |= WGCS_HS_PEER_COOKIE;  // the one lane of this launch that writes the row
          g[kGenSetAt] = (uint32_t)(uint64_t)now;
          g[kGenSetAt + 1] = (uint32_t)((uint64_t)now >> 32);
          g[kGenClaim] = 0;
        }
      }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4; ++i) w[i] = 0;
  }
};

// ---- ageing, cookie.go:306: time.Since(cookieSetAt) > CookieRefreshTime, peer row r ----

struct CookieAge {
  int64_t now;
  const wgcs_cookie_gen* gen;
  wgcs_hs_peer* peers;
  WGCS_HD void operator()(uint32_t r) const {
    uint32_t* const p = cookiegen_words(peers + r);
    const uint32_t flags = p[kHsPeerFlags];
    if (!(flags & WGCS_HS_PEER_COOKIE)) return;
    const uint32_t* const g = cookiegen_words(gen + r);
    const uint64_t set_at = (uint64_t)g[kGenSetAt] | ((uint64_t)g[kGenSetAt + 1] << 32);
    // signed: a clock that went back gives a negative age, and the cookie stays
    if ((int64_t)((uint64_t)now - set_at) > WGCS_COOKIE_REFRESH_NS) p[kHsPeerFlags] = flags & ~WGCS_HS_PEER_COOKIE;
  }
};

}  // namespace wgcs
