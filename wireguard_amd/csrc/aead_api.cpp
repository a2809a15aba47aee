// aead_api.cpp -- C ABI of the transport AEAD (include/wgcsum.h):
//   wgcs_padding                  padding()                       device/send.go:529-560
//   wgcs_aead_seal_batch          RoutineEncryption, device-resident batches   send.go:438-463
//   wgcs_aead_open_batch          RoutineDecryption + the length trim          receive.go:363-383, :432-482
//   wgcs_aead_seal / wgcs_aead_open   the same for one packet in host memory
// Every byte is sealed or opened by aead_kernels.hip; the per-call forms stage
// the packet in device memory and launch that kernel on a batch of one.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/wgcsum.h"
#include "wgcs_aead.h"
#include "wgcs_ctx.h"
#include "wgcs_kernels.h"

using namespace wgcs;

static_assert(sizeof(wgcs_aead_key) == 48 && sizeof(wgcs_aead_pkt) == 24, "wgcsum.h layouts");

namespace {

int batch(wgcs_ctx* ctx, int open, uint8_t* d_arena, const wgcs_aead_pkt* d_pkts, const wgcs_aead_key* d_keys,
          uint32_t n_keys, uint32_t n, uint32_t mtu, int32_t* d_len, uint64_t* d_counter, void* stream) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (n == 0) return WGCS_OK;
  if (!d_arena || !d_pkts || !d_len || (open && !d_counter) || (n_keys && !d_keys))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  if (n > kMaxRows || ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_keys & 3) || ((uintptr_t)d_len & 3) ||
      ((uintptr_t)d_counter & 7))
    return set_err(ctx, WGCS_ERR_INVALID_ARG, "n <= 2^28, 8-byte aligned d_pkts / d_counter, 4-byte aligned d_keys");
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  hipError_t e = launch_aead_batch(open, d_arena, d_pkts, d_keys, n_keys, n, mtu, d_len, d_counter, s);
  return e == hipSuccess ? WGCS_OK : hip_fail(ctx, e, open ? "aead_open launch" : "aead_seal launch");
}

// Staging of the per-call forms, one device buffer and its pinned mirror:
// key | descriptor | status | counter | message.
constexpr size_t kOffKey = 0, kOffPkt = 48, kOffLen = 72, kOffCtr = 80, kOffMsg = 96;

// One packet through the kernel: msg[0:in_len) goes up, msg[0:out_len) comes back.
int one(wgcs_ctx* ctx, int open, const uint8_t key[32], uint32_t remote_index, uint64_t counter, uint8_t* msg,
        size_t in_len, size_t out_len, uint32_t desc_len, uint32_t mtu, int32_t* status, uint64_t* ctr) {
  const size_t total = kOffMsg + (in_len > out_len ? in_len : out_len);
  std::lock_guard<std::mutex> g(ctx->mu);
  hipSetDevice(ctx->device);
  int rc;
  if ((rc = ensure_dev(ctx, ctx->d_arena, total)) || (rc = ensure_pinned(ctx, ctx->h_stage, total))) return rc;
  uint8_t* hs = (uint8_t*)ctx->h_stage.ptr;
  uint8_t* d = (uint8_t*)ctx->d_arena.ptr;
  wgcs_aead_key k;
  memset(&k, 0, sizeof k);
  memcpy(k.key, key, 32);
  k.remote_index = remote_index;
  wgcs_aead_pkt p;
  p.off = kOffMsg;
  p.counter = counter;
  p.len = desc_len;
  p.key = 0;
  memcpy(hs + kOffKey, &k, sizeof k);
  memcpy(hs + kOffPkt, &p, sizeof p);
  memset(hs + kOffLen, 0, kOffMsg - kOffLen);
  if (in_len) memcpy(hs + kOffMsg, msg, in_len);
  hipStream_t s = ctx->stream;
  hipError_t e = hipMemcpyAsync(d, hs, kOffMsg + in_len, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = launch_aead_batch(open, d, (const wgcs_aead_pkt*)(d + kOffPkt), (const wgcs_aead_key*)(d + kOffKey), 1, 1, mtu,
                          (int32_t*)(d + kOffLen), (uint64_t*)(d + kOffCtr), s);
  if (e == hipSuccess) e = hipMemsetAsync(d + kOffKey, 0, sizeof k, s);  // the key does not outlive the call
  if (e == hipSuccess) e = hipMemcpyAsync(hs + kOffLen, d + kOffLen, total - kOffLen, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  memset(&k, 0, sizeof k);
  memset(hs + kOffKey, 0, sizeof k);
  if (e != hipSuccess) return hip_fail(ctx, e, open ? "aead_open" : "aead_seal");
  memcpy(status, hs + kOffLen, 4);
  memcpy(ctr, hs + kOffCtr, 8);
  if (out_len) memcpy(msg, hs + kOffMsg, out_len);
  return WGCS_OK;
}

}  // namespace

extern "C" {

int wgcs_padding(size_t packet_size, uint32_t mtu) {
  if (packet_size <= kAeadMaxLen) return (int)aead_padding((uint32_t)packet_size, mtu);  // the kernel's own
  // beyond what a descriptor can carry: the same arithmetic in size_t
  size_t last_unit = packet_size;
  if (mtu == 0) return (int)(((last_unit + 15) & ~(size_t)15) - last_unit);
  if (last_unit > mtu) last_unit %= mtu;
  size_t padded = (last_unit + 15) & ~(size_t)15;
  if (padded > mtu) padded = mtu;
  return (int)(padded - last_unit);
}

int wgcs_aead_seal_batch(wgcs_ctx* ctx, uint8_t* d_arena, const wgcs_aead_pkt* d_pkts, const wgcs_aead_key* d_keys,
                         uint32_t n_keys, uint32_t n, uint32_t mtu, int32_t* d_out_len, void* stream) {
  return batch(ctx, 0, d_arena, d_pkts, d_keys, n_keys, n, mtu, d_out_len, nullptr, stream);
}

int wgcs_aead_open_batch(wgcs_ctx* ctx, uint8_t* d_arena, const wgcs_aead_pkt* d_pkts, const wgcs_aead_key* d_keys,
                         uint32_t n_keys, uint32_t n, int32_t* d_pkt_len, uint64_t* d_counter, void* stream) {
  return batch(ctx, 1, d_arena, d_pkts, d_keys, n_keys, n, 0, d_pkt_len, d_counter, stream);
}

int wgcs_aead_seal(wgcs_ctx* ctx, const uint8_t key[32], uint32_t remote_index, uint64_t counter, uint8_t* buf,
                   size_t len, size_t cap, uint32_t mtu, size_t* out_len) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!key || !buf || !out_len) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  *out_len = 0;
  if (len > kAeadMaxLen) return set_err(ctx, WGCS_ERR_OUT_OF_RANGE, "packet of %zu bytes", len);
  const size_t sealed = kAeadHeader + len + aead_padding((uint32_t)len, mtu) + kAeadTag;
  if (cap < sealed) return set_err(ctx, WGCS_ERR_OUT_OF_RANGE, "cap %zu < %zu", cap, sealed);
  int32_t st = 0;
  uint64_t ctr = 0;
  const int rc = one(ctx, 0, key, remote_index, counter, buf, kAeadHeader + len, sealed, (uint32_t)len, mtu, &st, &ctr);
  if (rc) return rc;
  if (st != (int32_t)sealed) return set_err(ctx, st < 0 ? st : WGCS_ERR_HIP, "seal kernel returned %d", st);
  *out_len = sealed;
  return WGCS_OK;
}

int wgcs_aead_open(wgcs_ctx* ctx, const uint8_t key[32], uint8_t* msg, size_t len, uint64_t* counter, int* pkt_len) {
  if (!ctx) return WGCS_ERR_INVALID_ARG;
  if (!key || !msg || !counter || !pkt_len) return set_err(ctx, WGCS_ERR_INVALID_ARG, "NULL pointer");
  *pkt_len = 0;
  if (len < kAeadHeader + kAeadTag || len > kAeadMaxLen)
    return set_err(ctx, WGCS_ERR_OUT_OF_RANGE, "message of %zu bytes", len);
  int32_t st = 0;
  const int rc = one(ctx, 1, key, 0, 0, msg, len, len, (uint32_t)len, 0, &st, counter);
  if (rc) return rc;
  if (st < 0) return st;  // WGCS_ERR_AUTH / WGCS_ERR_PACKET_TOO_SHORT
  *pkt_len = st;
  return WGCS_OK;
}

}  // extern "C"
