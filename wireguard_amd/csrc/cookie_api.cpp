// cookie_api.cpp -- C ABI of the device-resident handshake screen (include/wgcsum.h):
//   wgcs_handshake_screen_batch    the top of RoutineHandshake    device/receive.go:270-287
// It runs in cookie_kernels.hip; the checker, the sources and the nonces are
// the caller's device memory.  The host functions of the same section are in
// cookie.cpp.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"

using namespace wgcs;

extern "C" {

int wgcs_handshake_screen_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts,
                                const int32_t* d_type, uint32_t n, const wgcs_cookie_checker* d_checker,
                                const wgcs_src_addr* d_src, uint32_t under_load, const uint8_t* d_nonce,
                                int32_t* d_verdict, uint8_t* d_reply, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_type || !d_checker || !d_verdict || (under_load && (!d_src || !d_nonce || !d_reply)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_type & 3) || ((uintptr_t)d_checker & 3) ||
      ((uintptr_t)d_src & 3) || ((uintptr_t)d_nonce & 3) || ((uintptr_t)d_verdict & 3) || ((uintptr_t)d_reply & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG,
                   "n <= 2^28, 8-byte aligned d_pkts, 4-byte aligned d_type / d_checker / d_src / d_nonce / d_verdict / "
                   "d_reply");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = launch_hs_screen(d_arena, d_pkts, d_type, n, d_checker, d_src, under_load, d_nonce, d_verdict,
                                        d_reply, stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, "handshake_screen launch");
}

}  // extern "C"
