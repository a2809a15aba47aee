// timers_api.cpp -- C ABI of the peer timers (include/wgcsum.h):
//   wgcs_timers_sent_batch         behind send-assign                  device/send.go:498-510
//   wgcs_timers_received_batch     over the write groups               device/receive.go:486-494
//   wgcs_timers_initiated_batch    behind start and initiate           send.go:85-87, :117-126
//   wgcs_timers_responded_batch    behind respond                      receive.go:311-312, send.go:158-160
//   wgcs_timers_finished_batch     behind begin-initiator              receive.go:339-348
//   wgcs_timers_rotated_batch      behind keypairs-received            receive.go:422-427
//   wgcs_timers_expire_batch       the expiry of the five timers       device/timers.go:73-144
// The event calls run their bodies of wgcs_timers.h through launch_each, expire
// its kernels of timers_kernels.hip; every table and the expire call's scratch
// are the caller's device memory.  The host functions of the same section are in
// timers.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_timers.h"

using namespace wgcs;

namespace {

// what the lookups of a lane need: id -> row -> timers
int check_rows(wgcs_ctx* ctx, const uint32_t* d_peer_rows, uint32_t n_ids, const wgcs_timers* d_timers,
               uint32_t n_peers) {
  if ((n_ids && !d_peer_rows) || (n_peers && !d_timers)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_peers > kMaxPeers) return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_peers <= 2^24");
  if (misaligned(d_peer_rows, 3) || misaligned(d_timers, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned d_peer_rows, 8-byte aligned d_timers");
  return WGCS_OK;
}

}  // namespace

extern "C" {

int wgcs_timers_sent_batch(wgcs_ctx* ctx, const int32_t* d_sizes, const uint32_t* d_peer, const int32_t* d_count,
                           const int32_t* d_status, const uint32_t* d_job_key, uint32_t n_jobs, uint32_t max_segs,
                           int64_t now_ns, uint32_t jitter_seed, const uint32_t* d_peer_rows, uint32_t n_ids,
                           wgcs_timers* d_timers, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_jobs == 0) return WGCS_OK;
  if (!d_sizes || !d_peer || !d_count || !d_status || !d_job_key)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (max_segs == 0 || (uint64_t)n_jobs * max_segs > kMaxRows)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "max_segs >= 1, n_jobs * max_segs <= 2^28");
  if (misaligned(d_sizes, 3) || misaligned(d_peer, 3) || misaligned(d_count, 3) || misaligned(d_status, 3) ||
      misaligned(d_job_key, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned job arrays");
  if (int rc = check_rows(ctx, d_peer_rows, n_ids, d_timers, n_peers)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const TimersSent body = {{{d_peer, d_count, d_status, max_segs, d_peer_rows, n_ids, n_peers}, d_job_key},
                           d_sizes, now_ns, jitter_seed, d_timers};
  const hipError_t e = launch_each(body, n_jobs, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "timers_sent launch");
}

int wgcs_timers_received_batch(wgcs_ctx* ctx, const wgcs_write_group* d_groups, uint32_t n_batches,
                               uint32_t calls_per_batch, int64_t now_ns, const uint32_t* d_peer_rows, uint32_t n_ids,
                               wgcs_timers* d_timers, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  const uint64_t n = (uint64_t)n_batches * calls_per_batch;
  if (n == 0) return WGCS_OK;
  if (!d_groups) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || misaligned(d_groups, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_batches * calls_per_batch <= 2^28, 8-byte aligned d_groups");
  if (int rc = check_rows(ctx, d_peer_rows, n_ids, d_timers, n_peers)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const TimersReceived body = {{d_groups, d_peer_rows, n_ids, n_peers}, now_ns, d_timers};
  const hipError_t e = launch_each(body, (uint32_t)n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "timers_received launch");
}

int wgcs_timers_initiated_batch(wgcs_ctx* ctx, const uint32_t* d_reasons, const uint32_t* d_start_peer,
                                const int32_t* d_init_status, uint32_t n_tickets, int64_t now_ns,
                                uint32_t jitter_seed, wgcs_timers* d_timers, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_peers == 0) return WGCS_OK;  // no row to write
  if (!d_reasons || !d_timers || (n_tickets && (!d_start_peer || !d_init_status)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_peers > kMaxPeers || n_tickets > kMaxRows)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_peers <= 2^24, n_tickets <= 2^28");
  if (misaligned(d_reasons, 3) || misaligned(d_start_peer, 3) || misaligned(d_init_status, 3) ||
      misaligned(d_timers, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "8-byte aligned d_timers, 4-byte aligned rows");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  // the peer rows, then the tickets
  hipError_t e = launch_each(TimersFresh{d_reasons, d_timers}, n_peers, s);
  if (e == hipSuccess && n_tickets)
    e = launch_each(TimersInitiated{{d_start_peer, d_init_status, n_peers}, now_ns, jitter_seed, d_timers}, n_tickets,
                    s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "timers_initiated launch");
}

int wgcs_timers_responded_batch(wgcs_ctx* ctx, const wgcs_hs_resp* d_resp, const int32_t* d_gate, uint32_t n,
                                int64_t now_ns, wgcs_timers* d_timers, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_resp || !d_gate || (n_peers && !d_timers)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || n_peers > kMaxPeers || misaligned(d_resp, 3) || misaligned(d_gate, 3) || misaligned(d_timers, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^28, n_peers <= 2^24, 4-byte aligned d_resp / d_gate, 8-byte aligned d_timers");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const TimersResponded body = {{d_resp, d_gate, n_peers}, now_ns, d_timers};
  const hipError_t e = launch_each(body, n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "timers_responded launch");
}

int wgcs_timers_finished_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts,
                               const int32_t* d_gate, const int32_t* d_begun, uint32_t n, int64_t now_ns,
                               const wgcs_session_slot* d_hs_slots, uint32_t n_hs_slots, const wgcs_hs_state* d_states,
                               uint32_t n_states, wgcs_timers* d_timers, wgcs_rekey* d_rekey, uint32_t n_peers,
                               void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_gate || !d_begun || (n_hs_slots && !d_hs_slots) || (n_states && !d_states) ||
      (n_peers && (!d_timers || !d_rekey)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxPeers || n_peers > kMaxPeers || !pow2_or_0(n_hs_slots))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^24, n_peers <= 2^24, n_hs_slots 0 or a power of two");
  if (misaligned(d_pkts, 7) || misaligned(d_gate, 3) || misaligned(d_begun, 3) || misaligned(d_hs_slots, 3) ||
      misaligned(d_states, 3) || misaligned(d_timers, 7) || misaligned(d_rekey, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "8-byte aligned d_pkts / d_timers / d_rekey, 4-byte aligned rows");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const TimersFinished body = {{d_arena, d_pkts, d_gate, d_hs_slots, n_hs_slots, d_states, n_states, n_peers},
                               d_begun, now_ns, d_timers, d_rekey};
  const hipError_t e = launch_each(body, n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "timers_finished launch");
}

int wgcs_timers_rotated_batch(wgcs_ctx* ctx, const wgcs_aead_pkt* d_pkts, const uint32_t* d_rotated, uint32_t n,
                              int64_t now_ns, const uint32_t* d_key_peer, uint32_t n_keys, const uint32_t* d_peer_rows,
                              uint32_t n_ids, wgcs_timers* d_timers, wgcs_rekey* d_rekey, uint32_t n_peers,
                              void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_pkts || !d_rotated || (n_keys && !d_key_peer) || (n_peers && !d_rekey))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || misaligned(d_pkts, 7) || misaligned(d_rotated, 3) || misaligned(d_key_peer, 3) ||
      misaligned(d_rekey, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 8-byte aligned d_pkts / d_rekey, 4-byte aligned rows");
  if (int rc = check_rows(ctx, d_peer_rows, n_ids, d_timers, n_peers)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const TimersRotated body = {{d_pkts, d_key_peer, n_keys, d_peer_rows, n_ids, n_peers}, d_rotated, now_ns, d_timers,
                              d_rekey};
  const hipError_t e = launch_each(body, n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "timers_rotated launch");
}

int wgcs_timers_expire_batch(wgcs_ctx* ctx, int64_t now_ns, wgcs_timers* d_timers, wgcs_rekey* d_rekey,
                             const wgcs_peer_key* d_table, uint32_t n_peers, const uint32_t* d_staged,
                             wgcs_keypairs* d_kp, wgcs_session_slot* d_slots, uint32_t n_slots,
                             wgcs_session_slot* d_peer_keys, uint32_t n_peer_slots, wgcs_aead_key* d_keys,
                             uint32_t* d_key_peer, uint32_t n_keys, uint32_t n_ka_max, uint32_t* d_ka_peer,
                             int32_t* d_ka_count, int32_t* d_ka_sizes, int32_t* d_ka_status, uint32_t* d_n_ka,
                             uint32_t* d_actions, void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!d_n_ka || (n_peers && (!d_timers || !d_rekey || !d_table || !d_kp || !d_actions || !d_work)) ||
      (n_slots && !d_slots) || (n_peer_slots && !d_peer_keys) || (n_keys && (!d_keys || !d_key_peer)) ||
      (n_ka_max && (!d_ka_peer || !d_ka_count || !d_ka_sizes || !d_ka_status)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_peers > kMaxPeers || n_ka_max > kMaxPeers || !pow2_or_0(n_slots) || !pow2_or_0(n_peer_slots))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_peers, n_ka_max <= 2^24, slot counts 0 or a power of two");
  if (misaligned(d_timers, 7) || misaligned(d_rekey, 7) || misaligned(d_table, 3) || misaligned(d_staged, 3) ||
      misaligned(d_kp, 3) || misaligned(d_slots, 3) || misaligned(d_peer_keys, 3) || misaligned(d_keys, 3) ||
      misaligned(d_key_peer, 3) || misaligned(d_ka_peer, 3) || misaligned(d_ka_count, 3) ||
      misaligned(d_ka_sizes, 3) || misaligned(d_ka_status, 3) || misaligned(d_n_ka, 3) || misaligned(d_actions, 3) ||
      misaligned(d_work, 15))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "8-byte aligned d_timers / d_rekey, 16-byte aligned d_work, 4-byte aligned rows");
  if (n_peers && work_bytes < keyorder_work_bytes(n_peers))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "work_bytes %zu is too small for %u peer rows", work_bytes, n_peers);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_timers_expire(now_ns, d_timers, d_rekey, d_table, n_peers, d_staged, d_kp, d_slots,
                                            n_slots, d_peer_keys, n_peer_slots, d_keys, d_key_peer, n_keys, n_ka_max,
                                            d_ka_peer, d_ka_count, d_ka_sizes, d_ka_status, d_n_ka, d_actions,
                                            (uint32_t*)d_work, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "timers_expire launch");
}

}  // extern "C"
