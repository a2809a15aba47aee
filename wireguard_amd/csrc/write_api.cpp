// write_api.cpp -- C ABI of the Write-call builder (include/wgcsum.h):
//   wgcs_write_build_batch   one Tun.Write per receive batch and peer, with that
//                            peer's bookkeeping     device/receive.go:178-228, :398-504
//   wgcs_write_build_host    the same on host arrays
// The device form runs in write_kernels.hip; the host form loops over the
// batches with the scalar rule both share (wgcs_write_plan.h).  Every table is
// the caller's memory; nothing is allocated and no workspace is needed.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_write_plan.h"

using namespace wgcs;

namespace {

// what both entry points ask of their arguments; NULL when they are fine
const char* check_args(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t n_msgs, uint32_t n_batches,
                       const uint32_t* key_peer, int32_t offset, uint32_t cap, uint32_t calls_per_batch,
                       const wgcs_gro_buf* bufs, const wgcs_gro_call* calls, const wgcs_write_group* groups,
                       const int32_t* n_groups, const int32_t* status) {
  if (!write_args_ok(n_msgs, n_batches, offset, cap, calls_per_batch))
    return "1 <= calls_per_batch <= n_msgs <= 128, n_batches * n_msgs <= 2^28, 0 <= offset <= cap";
  if (!pkts || !verdict || !key_peer || !bufs || !calls || !groups || !n_groups || !status) return "NULL pointer";
  if (((uintptr_t)pkts & 15) || ((uintptr_t)bufs & 15) || ((uintptr_t)calls & 15) || ((uintptr_t)groups & 7) ||
      ((uintptr_t)verdict & 3) || ((uintptr_t)key_peer & 3) || ((uintptr_t)n_groups & 3) || ((uintptr_t)status & 3))
    return "16-byte aligned d_pkts / d_bufs / d_calls, 8-byte aligned d_groups, 4-byte aligned 32-bit arrays";
  return nullptr;
}

}  // namespace

extern "C" {

int wgcs_write_build_batch(wgcs_ctx* ctx, const wgcs_aead_pkt* d_pkts, const int32_t* d_verdict, uint32_t n_msgs,
                           uint32_t n_batches, const uint32_t* d_key_peer, uint32_t n_keys, int32_t offset,
                           uint32_t cap, uint32_t gro_flags, uint32_t calls_per_batch, wgcs_gro_buf* d_bufs,
                           wgcs_gro_call* d_calls, wgcs_write_group* d_groups, int32_t* d_n_groups, int32_t* d_status,
                           void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n_batches == 0) return WGCS_OK;
  if (const char* why = check_args(d_pkts, d_verdict, n_msgs, n_batches, d_key_peer, offset, cap, calls_per_batch,
                                   d_bufs, d_calls, d_groups, d_n_groups, d_status))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "%s", why);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const hipError_t e = launch_write_build(d_pkts, d_verdict, n_msgs, n_batches, d_key_peer, n_keys, offset, cap,
                                          gro_flags, calls_per_batch, d_bufs, d_calls, d_groups, d_n_groups, d_status, s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "write_build launch");
}

int wgcs_write_build_host(const wgcs_aead_pkt* pkts, const int32_t* verdict, uint32_t n_msgs, uint32_t n_batches,
                          const uint32_t* key_peer, uint32_t n_keys, int32_t offset, uint32_t cap, uint32_t gro_flags,
                          uint32_t calls_per_batch, wgcs_gro_buf* bufs, wgcs_gro_call* calls, wgcs_write_group* groups,
                          int32_t* n_groups, int32_t* status) {
  if (n_batches == 0) return WGCS_OK;
  if (check_args(pkts, verdict, n_msgs, n_batches, key_peer, offset, cap, calls_per_batch, bufs, calls, groups,
                 n_groups, status))
    return WGCS_ERR_INVALID_ARG;
  for (uint32_t b = 0; b < n_batches; ++b)
    status[b] = write_plan_batch(pkts, verdict, b, n_msgs, key_peer, n_keys, offset, cap, gro_flags, calls_per_batch,
                                 bufs, calls, groups, n_groups + b);
  return WGCS_OK;
}

}  // extern "C"
