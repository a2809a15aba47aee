// ratelimit.cpp -- the rate limiter on host memory (include/wgcsum.h), no context
// and no device:
//   wgcs_ratelimit_home_slot      the home slot of an address
//   wgcs_ratelimit_allow          RateLimiter.Allow             ratelimiter/ratelimiter.go:91-126
//   wgcs_ratelimit_batch_host     Allow over a receive batch    device/receive.go:283-286
//   wgcs_ratelimit_cleanup_host   cleanup() as a rebuild        ratelimiter.go:77-89
// They run the row functions of wgcs_ratelimit.h, the code the lanes of
// ratelimit_kernels.hip run, taken in row order, in the passes of the device
// form.  Plain C++: the host test program (tests/ratelimit_host/ratelimit_host.cpp)
// links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_ratelimit.h"

using namespace wgcs;

extern "C" {

uint32_t wgcs_ratelimit_home_slot(const wgcs_src_addr* src, uint32_t n_slots) {
  RlKey k;
  if (!src || !rl_slots_ok(n_slots) || !rl_key_of(src, &k)) return 0;
  return rl_home(k, n_slots);
}

int wgcs_ratelimit_allow(wgcs_rl_entry* table, uint32_t n_slots, const wgcs_src_addr* src, int64_t now_ns) {
  RlKey k;
  if (!table || !src || !rl_slots_ok(n_slots) || !rl_key_of(src, &k)) return WGCS_ERR_INVALID_ARG;
  uint32_t s = rl_home(k, n_slots);
  for (uint32_t i = 0; i < n_slots; ++i, s = (s + 1) & (n_slots - 1)) {
    wgcs_rl_entry* e = table + s;
    if (e->state == 0) {  // :96-108
      rl_entry_fill(e, k, rl_fresh(1).tokens, now_ns);
      e->state = kRlLive;
      return 1;
    }
    if (e->state == kRlLive && rl_key_eq(rl_entry_key(e), k)) {  // :110-125
      const RlOutcome o = rl_known(e->tokens, e->last_ns, now_ns, 1);
      e->tokens = o.tokens;
      e->last_ns = now_ns;
      return (int)o.pass;
    }
  }
  return WGCS_ERR_RATE_TABLE_FULL;
}

int wgcs_ratelimit_batch_host(const int32_t* gate, const wgcs_src_addr* src, uint32_t n, wgcs_rl_entry* table,
                              uint32_t n_slots, int64_t now_ns, int32_t* verdict, uint32_t* stats) {
  if (!rl_slots_ok(n_slots) || n > kRlMaxRows || (n && (!gate || !src || !table || !verdict)))
    return WGCS_ERR_INVALID_ARG;
  uint32_t counts[kRlStats] = {0, 0, 0, 0};
  try {
    // the launches of the device form, each a loop: find or claim, the key order, the positions
    std::vector<uint32_t> keys_in(n), slots(n), keys(n);
    for (uint32_t q = 0; q < n; ++q) {
      bool full = false;
      keys_in[q] = rl_find_or_claim(q, gate, src, n, table, n_slots, verdict, &full);
      counts[kRlTableFull] += full;
      slots[q] = q;
    }
    std::stable_sort(slots.begin(), slots.end(), [&](uint32_t a, uint32_t b) { return keys_in[a] < keys_in[b]; });
    for (uint32_t p = 0; p < n; ++p) keys[p] = keys_in[slots[p]];
    for (uint32_t p = 0; p < n; ++p)
      rl_position(p, keys.data(), slots.data(), n, n_slots, src, table, now_ns, verdict, counts);
  } catch (const std::bad_alloc&) {
    return WGCS_ERR_NOMEM;
  }
  if (stats)
    for (int i = 0; i < kRlStats; ++i) stats[i] = counts[i];
  return WGCS_OK;
}

int wgcs_ratelimit_cleanup_host(const wgcs_rl_entry* old_table, wgcs_rl_entry* new_table, uint32_t n_slots,
                                int64_t now_ns, uint32_t* live) {
  if (!old_table || !new_table || !live || !rl_slots_ok(n_slots)) return WGCS_ERR_INVALID_ARG;
  const uint64_t bytes = (uint64_t)n_slots * sizeof *new_table;
  if (overlap(old_table, bytes, new_table, bytes)) return WGCS_ERR_INVALID_ARG;
  memset(new_table, 0, (size_t)n_slots * sizeof *new_table);
  uint32_t kept = 0;
  for (uint32_t i = 0; i < n_slots; ++i) kept += rl_cleanup_row(i, old_table, new_table, n_slots, now_ns);
  *live = kept;
  return WGCS_OK;
}

}  // extern "C"
