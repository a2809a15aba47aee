// replay_api.cpp -- C ABI of the per-keypair state (include/wgcsum.h):
//   wgcs_replay_validate / _reset   replay.Filter on host memory       replay/replay.go
//   wgcs_replay_batch               keypair.replayFilter.Validate      device/receive.go:414-420
//   wgcs_send_assign_batch          key and nonces of the send jobs    device/send.go:383-390
//   wgcs_keyorder_work_bytes        the workspace both batches carve
//   keyorder_prepare                (wgcs_ctx.h) that carve, for every call on the key order
// The batches run in replay_kernels.hip on the key order of keyorder.hip; the
// filters, the send nonces and the workspace are the caller's device memory.
#include <hip/hip_runtime.h>

#include <string.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_replay.h"

using namespace wgcs;

int wgcs::keyorder_prepare(wgcs_ctx* ctx, void* d_work, size_t work_bytes, uint32_t n, uint32_t n_keys, hipStream_t s,
                           KeyOrder* ko) {
  if (!d_work || misaligned(d_work, 15)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "16-byte aligned d_work");
  bool fits = keyorder_carve(d_work, work_bytes, n, ko);
  if (fits) {
    const hipError_t e = keyorder_check(*ko, n, n_keys, s, &fits);
    if (e != hipSuccess) return hip_fail(ctx, e, "key order size query");
  }
  if (!fits) return set_err(ctx, WGCS_ERR_INVALID_ARG, "work_bytes %zu is too small for %u rows", work_bytes, n);
  return WGCS_OK;
}

extern "C" {

int wgcs_replay_validate(wgcs_replay_filter* f, uint64_t value, uint64_t limit) {
  if (!f) return WGCS_ERR_INVALID_ARG;
  return wgcs_replay_validate_one(f, value, limit) ? 1 : 0;
}

void wgcs_replay_reset(wgcs_replay_filter* f) {
  if (f) memset(f, 0, sizeof *f);  // replay.go:73-76
}

size_t wgcs_keyorder_work_bytes(uint32_t n) { return keyorder_work_bytes(n); }

int wgcs_replay_batch(wgcs_ctx* ctx, const wgcs_aead_pkt* d_pkts, const int32_t* d_pkt_len, const uint64_t* d_counter,
                      uint32_t n, wgcs_replay_filter* d_filters, uint32_t n_keys, uint64_t limit, int32_t* d_verdict,
                      void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_pkts || !d_pkt_len || !d_counter || !d_verdict || (n_keys && !d_filters))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kKeyOrderMaxRows || n_keys > kKeyOrderMaxKeys || misaligned(d_pkts, 7) || misaligned(d_counter, 7) ||
      misaligned(d_filters, 7) || misaligned(d_pkt_len, 3) || misaligned(d_verdict, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n, n_keys <= 2^24, 8-byte aligned d_pkts / d_counter / d_filters, 4-byte aligned int32 arrays");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  KeyOrder ko;
  if (int rc = keyorder_prepare(ctx, d_work, work_bytes, n, n_keys, s, &ko)) return rc;
  const hipError_t e = launch_replay(ko, d_pkts, d_pkt_len, d_counter, n, d_filters, n_keys, limit, d_verdict, s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "replay launch");
}

int wgcs_send_assign_batch(wgcs_ctx* ctx, const int32_t* d_sizes, const uint32_t* d_peer, const int32_t* d_count,
                           const int32_t* d_status, uint32_t n_jobs, uint32_t max_segs, uint64_t stride,
                           const wgcs_session_slot* d_peer_keys, uint32_t n_slots, uint64_t* d_send_nonce,
                           uint32_t n_keys, uint64_t limit, wgcs_aead_pkt* d_pkts, int32_t* d_nbufs,
                           uint32_t* d_job_key, void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_jobs == 0) return WGCS_OK;
  if (!d_sizes || !d_peer || !d_count || !d_status || !d_peer_keys || !d_pkts || !d_nbufs || !d_job_key ||
      (n_keys && !d_send_nonce))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_jobs > kKeyOrderMaxRows || n_keys > kKeyOrderMaxKeys || max_segs == 0 ||
      (uint64_t)n_jobs * max_segs > kMaxRows)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_jobs, n_keys <= 2^24, 1 <= max_segs, n_jobs * max_segs <= 2^28");
  if (misaligned(d_pkts, 7) || misaligned(d_send_nonce, 7) || misaligned(d_sizes, 3) || misaligned(d_peer, 3) ||
      misaligned(d_count, 3) || misaligned(d_status, 3) || misaligned(d_peer_keys, 3) || misaligned(d_nbufs, 3) ||
      misaligned(d_job_key, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "8-byte aligned d_pkts / d_send_nonce, 4-byte aligned 32-bit arrays");
  if (n_slots == 0 || (n_slots & (n_slots - 1)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_slots %u is not a power of two", n_slots);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  KeyOrder ko;
  if (int rc = keyorder_prepare(ctx, d_work, work_bytes, n_jobs, n_keys, s, &ko)) return rc;
  const hipError_t e = launch_send_assign(ko, d_sizes, d_peer, d_count, d_status, n_jobs, max_segs, stride, d_peer_keys,
                                          n_slots, d_send_nonce, n_keys, limit, d_pkts, d_nbufs, d_job_key, s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "send_assign launch");
}

}  // extern "C"
