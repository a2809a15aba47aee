// rekey_api.cpp -- C ABI of keypair expiry, the rekey rules and the start of a handshake (include/wgcsum.h):
//   wgcs_rekey_recv_gate_batch    a packet under a keypair past RejectAfterTime     device/receive.go:162-170
//   wgcs_rekey_send_gate_batch    a job without a usable current keypair            device/send.go:368-374
//   wgcs_rekey_sent_batch         keepKeyFreshSending                               send.go:213-227, :419-420
//   wgcs_rekey_received_batch     keepKeyFreshReceiving                             receive.go:80-91
//   wgcs_rekey_responded_batch    SendHandshakeResponse's lastSentHandshake         send.go:131-133
//   wgcs_rekey_start_batch        SendHandshakeInitiation up to the message         send.go:84-100
// The per-entry calls run their bodies of wgcs_rekey.h through launch_each, start
// its kernels of rekey_kernels.hip; every table and the start call's scratch are
// the caller's device memory.  The host functions of the same section are in
// rekey.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_rekey.h"

using namespace wgcs;

namespace {

// what the lookups of a lane need: id -> row -> keypairs
int check_rows(wgcs_ctx* ctx, const uint32_t* d_peer_rows, uint32_t n_ids, const wgcs_keypairs* d_kp, uint32_t n_peers) {
  if ((n_ids && !d_peer_rows) || (n_peers && !d_kp)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (misaligned(d_peer_rows, 3) || misaligned(d_kp, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned d_peer_rows / d_kp");
  return WGCS_OK;
}

// what the send gate and sent share
int check_jobs(wgcs_ctx* ctx, const uint32_t* d_peer, const int32_t* d_count, const int32_t* d_status, uint32_t n_jobs,
               uint32_t max_segs, const uint32_t* d_peer_rows, uint32_t n_ids, const wgcs_keypairs* d_kp,
               uint32_t n_peers, const uint64_t* d_send_nonce, uint32_t n_keys, const wgcs_rekey* d_rekey) {
  if (!d_peer || !d_count || !d_status || (n_keys && !d_send_nonce) || (n_peers && !d_rekey))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (max_segs == 0 || (uint64_t)n_jobs * max_segs > kMaxRows)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "max_segs >= 1, n_jobs * max_segs <= 2^28");
  if (misaligned(d_peer, 3) || misaligned(d_count, 3) || misaligned(d_status, 3) || misaligned(d_send_nonce, 7) ||
      misaligned(d_rekey, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "8-byte aligned d_send_nonce / d_rekey, 4-byte aligned job arrays");
  return check_rows(ctx, d_peer_rows, n_ids, d_kp, n_peers);
}

}  // namespace

extern "C" {

int wgcs_rekey_recv_gate_batch(wgcs_ctx* ctx, wgcs_aead_pkt* d_pkts, uint32_t n, int64_t now_ns,
                               const uint32_t* d_key_peer, uint32_t n_keys, const uint32_t* d_peer_rows,
                               uint32_t n_ids, const wgcs_keypairs* d_kp, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_pkts || (n_keys && !d_key_peer)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || misaligned(d_pkts, 7) || misaligned(d_key_peer, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 8-byte aligned d_pkts, 4-byte aligned d_key_peer");
  if (int rc = check_rows(ctx, d_peer_rows, n_ids, d_kp, n_peers)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const RekeyRecvGate body = {{d_pkts, d_key_peer, n_keys, d_peer_rows, n_ids, n_peers}, now_ns, d_kp, d_pkts};
  const hipError_t e = launch_each(body, n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "rekey_recv_gate launch");
}

int wgcs_rekey_send_gate_batch(wgcs_ctx* ctx, const uint32_t* d_peer, const int32_t* d_count,
                               const int32_t* d_status_in, uint32_t n_jobs, uint32_t max_segs, int64_t now_ns,
                               const uint32_t* d_peer_rows, uint32_t n_ids, const wgcs_keypairs* d_kp,
                               uint32_t n_peers, const uint64_t* d_send_nonce, uint32_t n_keys, uint64_t limit,
                               wgcs_rekey* d_rekey, int32_t* d_status_out, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_jobs == 0) return WGCS_OK;
  if (!d_status_out) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (misaligned(d_status_out, 3)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned d_status_out");
  if (int rc = check_jobs(ctx, d_peer, d_count, d_status_in, n_jobs, max_segs, d_peer_rows, n_ids, d_kp, n_peers,
                          d_send_nonce, n_keys, d_rekey))
    return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const RekeySendGate body = {{d_peer, d_count, d_status_in, max_segs, d_peer_rows, n_ids, n_peers}, now_ns, d_kp,
                              d_send_nonce, n_keys, limit, d_rekey, d_status_out};
  const hipError_t e = launch_each(body, n_jobs, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "rekey_send_gate launch");
}

int wgcs_rekey_sent_batch(wgcs_ctx* ctx, const uint32_t* d_peer, const int32_t* d_count, const int32_t* d_status,
                          const uint32_t* d_job_key, uint32_t n_jobs, uint32_t max_segs, int64_t now_ns,
                          const uint32_t* d_peer_rows, uint32_t n_ids, const wgcs_keypairs* d_kp, uint32_t n_peers,
                          const uint64_t* d_send_nonce, uint32_t n_keys, uint64_t limit, wgcs_rekey* d_rekey,
                          void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_jobs == 0) return WGCS_OK;
  if (!d_job_key) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (misaligned(d_job_key, 3)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned d_job_key");
  if (int rc = check_jobs(ctx, d_peer, d_count, d_status, n_jobs, max_segs, d_peer_rows, n_ids, d_kp, n_peers,
                          d_send_nonce, n_keys, d_rekey))
    return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const RekeySent body = {{d_peer, d_count, d_status, max_segs, d_peer_rows, n_ids, n_peers}, d_job_key, now_ns, d_kp,
                          d_send_nonce, n_keys, limit, d_rekey};
  const hipError_t e = launch_each(body, n_jobs, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "rekey_sent launch");
}

int wgcs_rekey_received_batch(wgcs_ctx* ctx, const wgcs_write_group* d_groups, uint32_t n_batches,
                              uint32_t calls_per_batch, int64_t now_ns, const uint32_t* d_peer_rows, uint32_t n_ids,
                              const wgcs_keypairs* d_kp, uint32_t n_peers, wgcs_rekey* d_rekey, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  const uint64_t n = (uint64_t)n_batches * calls_per_batch;
  if (n == 0) return WGCS_OK;
  if (!d_groups || (n_peers && !d_rekey)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || misaligned(d_groups, 7) || misaligned(d_rekey, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_batches * calls_per_batch <= 2^28, 8-byte aligned d_groups / d_rekey");
  if (int rc = check_rows(ctx, d_peer_rows, n_ids, d_kp, n_peers)) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const RekeyReceived body = {{d_groups, d_peer_rows, n_ids, n_peers}, now_ns, d_kp, d_rekey};
  const hipError_t e = launch_each(body, (uint32_t)n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "rekey_received launch");
}

int wgcs_rekey_responded_batch(wgcs_ctx* ctx, const wgcs_hs_resp* d_resp, const int32_t* d_gate, uint32_t n,
                               int64_t now_ns, wgcs_rekey* d_rekey, uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_resp || !d_gate || (n_peers && !d_rekey)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || misaligned(d_resp, 3) || misaligned(d_gate, 3) || misaligned(d_rekey, 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 4-byte aligned d_resp / d_gate, 8-byte aligned d_rekey");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const RekeyResponded body = {{d_resp, d_gate, n_peers}, now_ns, d_rekey};
  const hipError_t e = launch_each(body, n, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "rekey_responded launch");
}

int wgcs_rekey_start_batch(wgcs_ctx* ctx, int64_t now_ns, wgcs_rekey* d_rekey, const wgcs_hs_peer* d_hs_peers,
                           uint32_t n_peers, const wgcs_hs_start* d_tickets, uint32_t n_tickets,
                           wgcs_hs_start* d_start, uint32_t* d_start_peer, uint32_t* d_count, int32_t* d_status,
                           uint32_t* d_reasons, void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!d_count || (n_peers && (!d_rekey || !d_hs_peers || !d_status || !d_reasons || !d_work)) ||
      (n_tickets && (!d_tickets || !d_start || !d_start_peer)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_peers > kMaxPeers || n_tickets > kMaxRows || (n_tickets && d_start == d_tickets))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_peers <= 2^24, n_tickets <= 2^28, d_start must not be d_tickets");
  if (misaligned(d_rekey, 7) || misaligned(d_hs_peers, 3) || misaligned(d_tickets, 3) || misaligned(d_start, 3) ||
      misaligned(d_start_peer, 3) || misaligned(d_count, 3) || misaligned(d_status, 3) || misaligned(d_reasons, 3) ||
      misaligned(d_work, 15))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "8-byte aligned d_rekey, 16-byte aligned d_work, 4-byte aligned rows");
  if (n_peers && work_bytes < keyorder_work_bytes(n_peers))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "work_bytes %zu is too small for %u peer rows", work_bytes, n_peers);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_rekey_start(now_ns, d_rekey, d_hs_peers, n_peers, d_tickets, n_tickets, d_start,
                                          d_start_peer, d_count, d_status, d_reasons, (uint32_t*)d_work,
                                          stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "rekey_start launch");
}

}  // extern "C"
