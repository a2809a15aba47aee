// route_api.cpp -- C ABI of the device-resident peer lookup (include/wgcsum.h,
// SURVEY.md §8 row f5):
//   wgcs_recv_classify_batch   the loop body of RoutineReceiveFromPeers   device/receive.go:145-207
//   wgcs_recv_source_batch     the allowed-source check                   receive.go:438-482
//   wgcs_route_dst_batch       the routing step of RoutineReadFromTUN     device/send.go:264-293
// Every lookup runs in route_kernels.hip; the tables (session slots, router
// image) are the caller's device memory, built by router.cpp's host functions.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"
#include "wgcs_route_walk.h"

using namespace wgcs;

namespace {

template <typename F>
int launch(wgcs_ctx* ctx, void* stream, const char* what, F&& f) {
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  const hipError_t e = f(stream ? (hipStream_t)stream : ctx->stream);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, what);
}

// the image arguments of the two routed entry points
int check_image(wgcs_ctx* ctx, const uint8_t* d_image, size_t image_bytes) {
  if (!d_image) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (((uintptr_t)d_image & 15) || image_bytes < kRouteHeaderBytes)
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "16-byte aligned d_image of at least %u bytes", kRouteHeaderBytes);
  return WGCS_OK;
}

}  // namespace

extern "C" {

int wgcs_recv_classify_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off, uint64_t stride,
                             const int32_t* d_size, uint32_t n, const wgcs_session_slot* d_slots, uint32_t n_slots,
                             wgcs_aead_pkt* d_pkts, int32_t* d_type, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_size || !d_slots || !d_pkts || !d_type) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_off & 7) || ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_size & 3) ||
      ((uintptr_t)d_slots & 3) || ((uintptr_t)d_type & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 8-byte aligned d_off / d_pkts, 4-byte aligned d_size / d_slots");
  if (n_slots == 0 || (n_slots & (n_slots - 1)))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n_slots %u is not a power of two", n_slots);
  return launch(ctx, stream, "recv_classify launch", [&](hipStream_t s) {
    return launch_recv_classify(d_arena, d_off, stride, d_size, n, d_slots, n_slots, d_pkts, d_type, s);
  });
}

int wgcs_recv_source_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const wgcs_aead_pkt* d_pkts, const int32_t* d_pkt_len,
                           const uint32_t* d_key_peer, uint32_t n_keys, uint32_t n, const uint8_t* d_image,
                           size_t image_bytes, int32_t* d_verdict, uint32_t* d_peer, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_pkt_len || !d_verdict || (n_keys && !d_key_peer))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_pkt_len & 3) || ((uintptr_t)d_key_peer & 3) ||
      ((uintptr_t)d_verdict & 3) || ((uintptr_t)d_peer & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 8-byte aligned d_pkts, 4-byte aligned int32 / uint32 arrays");
  if (int rc = check_image(ctx, d_image, image_bytes)) return rc;
  return launch(ctx, stream, "recv_source launch", [&](hipStream_t s) {
    return launch_recv_source(d_arena, d_pkts, d_pkt_len, d_key_peer, n_keys, n, d_image, image_bytes, d_verdict,
                              d_peer, s);
  });
}

int wgcs_route_dst_batch(wgcs_ctx* ctx, const uint8_t* d_arena, const uint64_t* d_off, uint64_t stride, uint32_t offset,
                         const int32_t* d_size, uint32_t n, const uint8_t* d_image, size_t image_bytes,
                         uint32_t* d_peer, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_size || !d_peer) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_off & 7) || ((uintptr_t)d_size & 3) || ((uintptr_t)d_peer & 3))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 8-byte aligned d_off, 4-byte aligned d_size / d_peer");
  if (int rc = check_image(ctx, d_image, image_bytes)) return rc;
  return launch(ctx, stream, "route_dst launch", [&](hipStream_t s) {
    return launch_route_dst(d_arena, d_off, stride, offset, d_size, n, d_image, image_bytes, d_peer, s);
  });
}

}  // extern "C"
