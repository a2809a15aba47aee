// cookiegen_api.cpp -- C ABI of the cookie generator on device-resident tables
// (include/wgcsum.h):
//   wgcs_cookie_initiated_batch    lastMAC1 behind initiate           device/cookie.go:301-302
//   wgcs_cookie_responded_batch    lastMAC1 behind respond            cookie.go:301-302
//   wgcs_cookie_consume_batch      cookie replies of a receive batch  device/receive.go:246-269, cookie.go:319-339
//   wgcs_cookie_age_batch          CookieRefreshTime                  cookie.go:306
// They run the bodies of wgcs_cookiegen.h through launch_each; every table and
// the consume call's scratch are the caller's device memory.  The host functions of the same section are
// in cookiegen.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_cookiegen.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"

using namespace wgcs;

namespace {

// the checks the two recording calls share: desc is d_start or d_resp
int check_sent(wgcs_ctx* ctx, const void* desc, const int32_t* d_status, const uint8_t* d_msgs, uint32_t n,
               const wgcs_cookie_gen* d_gen, uint32_t n_peers) {
  if (!desc || !d_status || !d_msgs || (n_peers && !d_gen)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || n_peers > kMaxPeers) return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, n_peers <= 2^24");
  if (misaligned(desc, 3) || misaligned(d_status, 3) || misaligned(d_msgs, 3) || misaligned(d_gen, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "4-byte aligned rows");
  return WGCS_OK;
}

}  // namespace

extern "C" {

int wgcs_cookie_initiated_batch(wgcs_ctx* ctx, const wgcs_hs_start* d_start, const int32_t* d_status,
                                const uint8_t* d_msgs, uint32_t n, wgcs_cookie_gen* d_gen, uint32_t n_peers,
                                void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (int rc = check_sent(ctx, d_start, d_status, d_msgs, n, d_gen, n_peers)) return rc;
  if (overlap(d_gen, (uint64_t)n_peers * sizeof *d_gen, d_msgs, (uint64_t)n * kInitiationPitch))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_gen overlaps d_msgs");
  if (n_peers == 0) return WGCS_OK;  // no row to write
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const InitiatedRows src = {d_start, d_status, n_peers};
  const hipError_t e = launch_each(CookieSentClaim<InitiatedRows>{src, d_gen},
                                   CookieSentCommit<InitiatedRows>{src, d_msgs, d_gen}, n,
                                   stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "cookie_initiated launch");
}

int wgcs_cookie_responded_batch(wgcs_ctx* ctx, const wgcs_hs_resp* d_resp, const int32_t* d_status,
                                const uint8_t* d_msgs, uint32_t n, wgcs_cookie_gen* d_gen, uint32_t n_peers,
                                void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (int rc = check_sent(ctx, d_resp, d_status, d_msgs, n, d_gen, n_peers)) return rc;
  if (overlap(d_gen, (uint64_t)n_peers * sizeof *d_gen, d_msgs, (uint64_t)n * kResponsePitch))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_gen overlaps d_msgs");
  if (n_peers == 0) return WGCS_OK;  // no row to write
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const RespondedRows src = {d_resp, d_status, n_peers};
  const hipError_t e = launch_each(CookieSentClaim<RespondedRows>{src, d_gen},
                                   CookieSentCommit<RespondedRows>{src, d_msgs, d_gen}, n,
                                   stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "cookie_responded launch");
}

int wgcs_cookie_consume_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts, const int32_t* d_type,
                              uint32_t n, int64_t now_ns, const wgcs_session_slot* d_hs_slots, uint32_t n_hs_slots,
                              const wgcs_hs_state* d_states, uint32_t n_states, const wgcs_session_slot* d_slots,
                              uint32_t n_slots, const uint32_t* d_key_peer, uint32_t n_keys,
                              const uint32_t* d_peer_rows, uint32_t n_ids, wgcs_cookie_gen* d_gen,
                              wgcs_hs_peer* d_peers, uint32_t n_peers, void* d_work, int32_t* d_verdict, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_type || !d_work || !d_verdict || (n_hs_slots && !d_hs_slots) ||
      (n_states && !d_states) || (n_slots && !d_slots) || (n_keys && !d_key_peer) || (n_ids && !d_peer_rows) ||
      (n_peers && (!d_gen || !d_peers)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || n_peers > kMaxPeers || !pow2_or_0(n_hs_slots) || !pow2_or_0(n_slots))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, n_peers <= 2^24, slot counts 0 or a power of two");
  if (misaligned(d_pkts, 7) || misaligned(d_type, 3) || misaligned(d_hs_slots, 3) || misaligned(d_states, 3) ||
      misaligned(d_slots, 3) || misaligned(d_key_peer, 3) || misaligned(d_peer_rows, 3) || misaligned(d_gen, 3) ||
      misaligned(d_peers, 3) || misaligned(d_work, 3) || misaligned(d_verdict, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "8-byte aligned d_pkts, 4-byte aligned rows");
  const uint64_t work_bytes = 16 * (uint64_t)n, verdict_bytes = 4 * (uint64_t)n;
  const uint64_t gen_bytes = (uint64_t)n_peers * sizeof *d_gen, peers_bytes = (uint64_t)n_peers * sizeof *d_peers;
  if (overlap(d_work, work_bytes, d_verdict, verdict_bytes) || overlap(d_work, work_bytes, d_gen, gen_bytes) ||
      overlap(d_work, work_bytes, d_peers, peers_bytes) || overlap(d_verdict, verdict_bytes, d_gen, gen_bytes) ||
      overlap(d_verdict, verdict_bytes, d_peers, peers_bytes) || overlap(d_gen, gen_bytes, d_peers, peers_bytes))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_work, d_verdict, d_gen and d_peers overlap");
  const CookieGenTables t = {d_hs_slots, n_hs_slots, d_states, n_states, d_slots,  n_slots,
                             d_key_peer, n_keys,     d_peer_rows, n_ids,  n_peers};
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  uint32_t* const work = (uint32_t*)d_work;
  const hipError_t e = launch_each(CookieOpen{d_arena, d_pkts, d_type, t, d_gen, work, d_verdict},
                                   CookieCommit{d_arena, d_pkts, d_verdict, t, now_ns, d_gen, d_peers, work}, n,
                                   stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "cookie_consume launch");
}

int wgcs_cookie_age_batch(wgcs_ctx* ctx, int64_t now_ns, const wgcs_cookie_gen* d_gen, wgcs_hs_peer* d_peers,
                          uint32_t n_peers, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_peers == 0) return WGCS_OK;
  if (!d_gen || !d_peers) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n_peers > kMaxPeers || misaligned(d_gen, 3) || misaligned(d_peers, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_peers <= 2^24, 4-byte aligned tables");
  if (overlap(d_gen, (uint64_t)n_peers * sizeof *d_gen, d_peers, (uint64_t)n_peers * sizeof *d_peers))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_gen overlaps d_peers");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const CookieAge body = {now_ns, d_gen, d_peers};
  const hipError_t e = launch_each(body, n_peers, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "cookie_age launch");
}

}  // extern "C"
