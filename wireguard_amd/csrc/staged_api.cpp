// staged_api.cpp -- C ABI of the staged queue on device-resident rings (include/wgcsum.h):
//   wgcs_staged_stage_batch     StagePackets and the re-staging of :402-407   device/send.go:331-350
//   wgcs_staged_release_batch   SendStagedPackets up to the nonce loop        send.go:363-426
//   wgcs_staged_flush_batch     FlushStagedPackets                            send.go:352-361
// They run in staged_kernels.hip; the rings, every table and the scratch are the caller's
// device memory.  The host functions of the same section are in staged.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_staged.h"

using namespace wgcs;

namespace {

// the state's pointers and shape; lost is checked by the calls that write it
int check_rings(wgcs_ctx* ctx, const uint32_t* d_len, const uint32_t* d_head, const int32_t* d_slot_size,
                const uint8_t* d_ring, uint32_t n_peers, uint32_t cap, uint64_t stride) {
  if (n_peers > kKeyOrderMaxKeys || !staged_shape_ok(n_peers, cap, stride))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "cap a power of two in [1, 1024], n_peers <= 2^24, n_peers * cap <= 2^28, stride a multiple of 16");
  if (n_peers && (!d_len || !d_head || !d_slot_size || !d_ring)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (misaligned(d_len, 3) || misaligned(d_head, 3) || misaligned(d_slot_size, 3) || misaligned(d_ring, 15))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "16-byte aligned d_ring, 4-byte aligned d_len / d_head / d_slot_size");
  return WGCS_OK;
}

}  // namespace

extern "C" {

int wgcs_staged_stage_batch(wgcs_ctx* ctx, const uint8_t* d_arena, uint64_t stride, const int32_t* d_sizes,
                            const uint32_t* d_peer, const int32_t* d_count, const int32_t* d_status_in,
                            const int32_t* d_status_out, const uint32_t* d_job_key, uint32_t n_jobs, uint32_t max_segs,
                            const uint32_t* d_peer_rows, uint32_t n_ids, uint32_t* d_len, uint32_t* d_head,
                            uint32_t* d_lost, int32_t* d_slot_size, uint8_t* d_ring, uint32_t n_peers, uint32_t cap,
                            uint32_t* d_where, void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_jobs == 0) return WGCS_OK;
  if (!d_arena || !d_sizes || !d_peer || !d_count || !d_status_in || !d_status_out || !d_job_key || !d_where ||
      !d_work || (n_ids && !d_peer_rows) || (n_peers && !d_lost))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_jobs > kKeyOrderMaxRows || max_segs == 0 || (uint64_t)n_jobs * max_segs > kStagedMaxSlots)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_jobs <= 2^24, 1 <= max_segs, n_jobs * max_segs <= 2^28");
  if (int rc = check_rings(ctx, d_len, d_head, d_slot_size, d_ring, n_peers, cap, stride)) return rc;
  if (misaligned(d_arena, 15) || misaligned(d_work, 15) || misaligned(d_sizes, 3) || misaligned(d_peer, 3) ||
      misaligned(d_count, 3) || misaligned(d_status_in, 3) || misaligned(d_status_out, 3) || misaligned(d_job_key, 3) ||
      misaligned(d_peer_rows, 3) || misaligned(d_lost, 3) || misaligned(d_where, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "16-byte aligned d_arena / d_work, 4-byte aligned 32-bit arrays");
  if (overlap(d_arena, (uint64_t)n_jobs * max_segs * stride, d_ring, (uint64_t)n_peers * cap * stride))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_ring overlaps d_arena");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  KeyOrder ko;
  if (int rc = keyorder_prepare(ctx, d_work, work_bytes, n_jobs, n_peers, s, &ko)) return rc;
  const StagedRings st = {d_len, d_head, d_lost, d_slot_size, d_ring, n_peers, cap, stride};
  const hipError_t e = launch_staged_stage(ko, d_arena, d_sizes, d_peer, d_count, d_status_in, d_status_out, d_job_key, n_jobs, max_segs,
                          d_peer_rows, n_ids, st, d_where, s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "staged_stage launch");
}

int wgcs_staged_release_batch(wgcs_ctx* ctx, int64_t now_ns, const wgcs_peer_key* d_table, const wgcs_keypairs* d_kp,
                              const uint64_t* d_send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* d_rekey,
                              uint32_t* d_len, uint32_t* d_head, const int32_t* d_slot_size, const uint8_t* d_ring,
                              uint32_t n_peers, uint32_t cap, uint64_t stride, uint32_t n_out_max, uint8_t* d_out,
                              uint32_t* d_out_peer, int32_t* d_out_count, int32_t* d_out_sizes, int32_t* d_out_status,
                              uint32_t* d_n_out, int32_t* d_status, void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!d_n_out || (n_peers && (!d_table || !d_kp || !d_rekey || !d_status || !d_work)) || (n_keys && !d_send_nonce) ||
      (n_out_max && (!d_out || !d_out_peer || !d_out_count || !d_out_sizes || !d_out_status)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_out_max > kStagedMaxSlots) return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_out_max <= 2^28");
  if (int rc = check_rings(ctx, d_len, d_head, d_slot_size, d_ring, n_peers, cap, stride)) return rc;
  if (misaligned(d_out, 15) || misaligned(d_work, 15) || misaligned(d_send_nonce, 7) || misaligned(d_rekey, 7) ||
      misaligned(d_table, 3) || misaligned(d_kp, 3) || misaligned(d_out_peer, 3) || misaligned(d_out_count, 3) ||
      misaligned(d_out_sizes, 3) || misaligned(d_out_status, 3) || misaligned(d_n_out, 3) || misaligned(d_status, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "16-byte aligned d_out / d_work, 8-byte aligned d_send_nonce / d_rekey, 4-byte aligned rows");
  if (overlap(d_out, (uint64_t)n_out_max * stride, d_ring, (uint64_t)n_peers * cap * stride))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_out overlaps d_ring");
  if (n_peers && work_bytes < keyorder_work_bytes(n_peers))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "work_bytes %zu is too small for %u peer rows", work_bytes, n_peers);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const StagedRings st = {d_len, d_head, nullptr, const_cast<int32_t*>(d_slot_size), const_cast<uint8_t*>(d_ring),
                          n_peers, cap, stride};
  const hipError_t e = launch_staged_release(now_ns, d_table, d_kp, d_send_nonce, n_keys, limit, d_rekey, st, n_out_max,
                                             d_out, d_out_peer, d_out_count, d_out_sizes, d_out_status, d_n_out,
                                             d_status, (uint32_t*)d_work, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "staged_release launch");
}

int wgcs_staged_flush_batch(wgcs_ctx* ctx, const uint32_t* d_actions, uint32_t* d_len, uint32_t* d_head,
                            uint32_t* d_lost, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_peers == 0) return WGCS_OK;
  if (!d_len || !d_head || !d_lost) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_peers > kKeyOrderMaxKeys || misaligned(d_actions, 3) || misaligned(d_len, 3) || misaligned(d_head, 3) ||
      misaligned(d_lost, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_peers <= 2^24, 4-byte aligned rows");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e =
      launch_staged_flush(d_actions, d_len, d_head, d_lost, n_peers, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "staged_flush launch");
}

}  // extern "C"
