// ratelimit_api.cpp -- C ABI of the rate limiter on device-resident batches
// (include/wgcsum.h):
//   wgcs_ratelimit_batch           rateLimiter.Allow over the screened rows   device/receive.go:283-286
//   wgcs_ratelimit_cleanup_batch   cleanup() as a rebuild                     ratelimiter/ratelimiter.go:77-89
// They run in ratelimit_kernels.hip; the tables and the workspace are the
// caller's device memory.  The host functions of the same section are in
// ratelimit.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_keyorder.h"
#include "wgcs_ratelimit.h"

using namespace wgcs;

extern "C" {

int wgcs_ratelimit_batch(wgcs_ctx* ctx, const int32_t* d_gate, const wgcs_src_addr* d_src, uint32_t n,
                         wgcs_rl_entry* d_table, uint32_t n_slots, int64_t now_ns, int32_t* d_verdict,
                         uint32_t* d_stats, void* d_work, size_t work_bytes, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!rl_slots_ok(n_slots) || n > kRlMaxRows)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_slots a power of two in [1, 2^24], n <= 2^24");
  if (n && (!d_gate || !d_src || !d_table || !d_verdict || !d_work))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (misaligned(d_gate, 3) || misaligned(d_src, 3) || misaligned(d_verdict, 3) || misaligned(d_stats, 3) ||
      misaligned(d_table, 7) || misaligned(d_work, 15))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "8-byte aligned d_table, 16-byte aligned d_work, 4-byte aligned rows");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  KeyOrder ko = {};  // without rows the launch is the stats memset alone, and nothing is carved
  if (n)
    if (int rc = keyorder_prepare(ctx, d_work, work_bytes, n, n_slots, s, &ko)) return rc;
  const hipError_t e = launch_ratelimit(ko, d_gate, d_src, n, d_table, n_slots, now_ns, d_verdict, d_stats, s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "ratelimit launch");
}

int wgcs_ratelimit_cleanup_batch(wgcs_ctx* ctx, const wgcs_rl_entry* d_old, wgcs_rl_entry* d_new, uint32_t n_slots,
                                 int64_t now_ns, uint32_t* d_live, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!d_old || !d_new || !d_live) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (!rl_slots_ok(n_slots) || misaligned(d_old, 7) || misaligned(d_new, 7) || misaligned(d_live, 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_slots a power of two in [1, 2^24], 8-byte aligned tables");
  const uint64_t bytes = (uint64_t)n_slots * sizeof(wgcs_rl_entry);
  if (overlap(d_old, bytes, d_new, bytes)) return set_err(ctx, WGCS_ERR_INVALID_ARG, "d_new overlaps d_old");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e =
      launch_ratelimit_cleanup(d_old, d_new, n_slots, now_ns, d_live, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "ratelimit cleanup launch");
}

}  // extern "C"
