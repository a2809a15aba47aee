// cookiegen.cpp -- the cookie generator on host memory (include/wgcsum.h), no
// context and no device:
//   wgcs_cookie_gen_build          CookieGenerator.Init per peer row      device/cookie.go:269-282
//   wgcs_cookie_initiated_host     lastMAC1 behind initiate               cookie.go:301-302
//   wgcs_cookie_responded_host     lastMAC1 behind respond                cookie.go:301-302
//   wgcs_cookie_consume_host       cookie replies of a receive batch      device/receive.go:246-269, cookie.go:319-339
//   wgcs_cookie_age_host           CookieRefreshTime                      cookie.go:306
// They run the bodies of wgcs_cookiegen.h, the code the lanes of the device
// forms run, taken in row order, in the passes of the device form.  Plain C++:
// the host test program (tests/cookiegen_host/cookiegen_host.cpp)
// links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include <string.h>

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_cookiegen.h"

using namespace wgcs;

namespace {

inline bool misaligned4(const void* p) { return ((uintptr_t)p & 3) != 0; }

inline bool sent_ok(const void* desc, const int32_t* status, const uint8_t* msgs, uint32_t n, const wgcs_cookie_gen* gen,
                    uint32_t n_peers) {
  return desc && status && msgs && (!n_peers || gen) && n <= kMaxRows && n_peers <= kMaxPeers && !misaligned4(desc) &&
         !misaligned4(status) && !misaligned4(msgs) && !misaligned4(gen);
}

// the launches of the device form, each a loop: the claims, then the commits
template <class Rows>
void sent_rows(const Rows& src, const uint8_t* msgs, uint32_t n, wgcs_cookie_gen* gen) {
  const CookieSentClaim<Rows> claim = {src, gen};
  const CookieSentCommit<Rows> commit = {src, msgs, gen};
  for (uint32_t j = 0; j < n; ++j) claim(j);
  for (uint32_t j = 0; j < n; ++j) commit(j);
}

}  // namespace

extern "C" {

int wgcs_cookie_gen_build(const wgcs_peer_key* table, uint32_t n, wgcs_cookie_gen* rows) {
  if (n == 0) return WGCS_OK;
  if (!table || !rows || n > kMaxPeers) return WGCS_ERR_INVALID_ARG;
  for (uint32_t r = 0; r < n; ++r) {
    uint8_t in[40];  // BLAKE2s-256(WGLabelCookie | pk), cookie.go:279-281
    memcpy(in, "cookie--", 8);
    memcpy(in + 8, table[r].public_key, 32);
    memset(rows + r, 0, sizeof *rows);
    blake2s_bytes(nullptr, 0, in, sizeof in, 32, rows[r].cookie_key);
  }
  return WGCS_OK;
}

int wgcs_cookie_initiated_host(const wgcs_hs_start* start, const int32_t* status, const uint8_t* msgs, uint32_t n,
                               wgcs_cookie_gen* gen, uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (!sent_ok(start, status, msgs, n, gen, n_peers)) return WGCS_ERR_INVALID_ARG;
  sent_rows(InitiatedRows{start, status, n_peers}, msgs, n, gen);
  return WGCS_OK;
}

int wgcs_cookie_responded_host(const wgcs_hs_resp* resp, const int32_t* status, const uint8_t* msgs, uint32_t n,
                               wgcs_cookie_gen* gen, uint32_t n_peers) {
  if (n == 0) return WGCS_OK;
  if (!sent_ok(resp, status, msgs, n, gen, n_peers)) return WGCS_ERR_INVALID_ARG;
  sent_rows(RespondedRows{resp, status, n_peers}, msgs, n, gen);
  return WGCS_OK;
}

int wgcs_cookie_consume_host(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* type, uint32_t n,
                             int64_t now_ns, const wgcs_session_slot* hs_slots, uint32_t n_hs_slots,
                             const wgcs_hs_state* states, uint32_t n_states, const wgcs_session_slot* slots,
                             uint32_t n_slots, const uint32_t* key_peer, uint32_t n_keys, const uint32_t* peer_rows,
                             uint32_t n_ids, wgcs_cookie_gen* gen, wgcs_hs_peer* peers, uint32_t n_peers, void* work,
                             int32_t* verdict) {
  if (n == 0) return WGCS_OK;
  if (!arena || !pkts || !type || !work || !verdict || (n_hs_slots && !hs_slots) || (n_states && !states) ||
      (n_slots && !slots) || (n_keys && !key_peer) || (n_ids && !peer_rows) || (n_peers && (!gen || !peers)) ||
      n > kMaxRows || n_peers > kMaxPeers || !pow2_or_0(n_hs_slots) || !pow2_or_0(n_slots) || misaligned4(gen) ||
      misaligned4(peers) || misaligned4(work))
    return WGCS_ERR_INVALID_ARG;
  const CookieGenTables t = {hs_slots, n_hs_slots, states, n_states, slots, n_slots, key_peer, n_keys, peer_rows,
                             n_ids,    n_peers};
  uint32_t* const w = (uint32_t*)work;
  // the launches of the device form, each a loop: open and claim, then commit
  const CookieOpen open = {arena, pkts, type, t, gen, w, verdict};
  const CookieCommit commit = {arena, pkts, verdict, t, now_ns, gen, peers, w};
  for (uint32_t q = 0; q < n; ++q) open(q);
  for (uint32_t q = 0; q < n; ++q) commit(q);
  return WGCS_OK;
}

int wgcs_cookie_age_host(int64_t now_ns, const wgcs_cookie_gen* gen, wgcs_hs_peer* peers, uint32_t n_peers) {
  if (n_peers == 0) return WGCS_OK;
  if (!gen || !peers || n_peers > kMaxPeers || misaligned4(gen) || misaligned4(peers)) return WGCS_ERR_INVALID_ARG;
  const CookieAge age = {now_ns, gen, peers};
  for (uint32_t r = 0; r < n_peers; ++r) age(r);
  return WGCS_OK;
}

}  // extern "C"
