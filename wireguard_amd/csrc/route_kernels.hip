// route_kernels.hip -- the per-packet lookups of the reference's device package
// on device-resident batches (include/wgcsum.h):
//   recv_classify_kernel   the loop body of RoutineReceiveFromPeers    device/receive.go:145-207
//   recv_source_kernel     the allowed-source check                    receive.go:438-482
//   route_dst_kernel       the routing step of RoutineReadFromTUN      device/send.go:264-293
// One lane per packet.  A lookup is a chain of dependent loads -- trie nodes of
// 32 bytes, two dwordx4 each, or session slots -- that hit in L2 for any
// realistic table, so a lane's time is latency times depth and the launch is
// carried by how many lanes walk at once, not by bandwidth.  The arena is only
// read, by byte loads: packets and their addresses sit at any offset.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_kernels.h"
#include "wgcs_route_walk.h"

namespace wgcs {

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kMinMessageSize = 32;    // MinMessageSize = MessageTransportSize, device/noise.go:67-71
constexpr uint32_t kTransportContent = 16;  // MessageTransportContentOffset, noise.go:80
constexpr int32_t kMaxMessage = 65535;      // what a wgcs_aead_pkt may carry

__device__ inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ __launch_bounds__(kThreads) void recv_classify_kernel(const uint8_t* __restrict__ arena,
                                                                 const uint64_t* __restrict__ off_tab, uint64_t stride,
                                                                 const int32_t* __restrict__ sizes, uint32_t n,
                                                                 const wgcs_session_slot* __restrict__ slots,
                                                                 uint32_t n_slots, wgcs_aead_pkt* __restrict__ pkts,
                                                                 int32_t* __restrict__ types) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  const int32_t size = sizes[q];
  const uint64_t off = off_tab ? off_tab[q] : (uint64_t)q * stride;
  int32_t type = 0;
  uint32_t key = kSessionEmpty, len = (uint32_t)size;
  if (size < (int32_t)kMinMessageSize) {  // receive.go:146-148: skipped unread
  } else if (size > kMaxMessage || (!off_tab && (uint64_t)size > stride)) {
    type = WGCS_ERR_OUT_OF_RANGE;
    len = 0;
  } else {
    const uint8_t* const msg = arena + off;
    const uint32_t t = le32(msg);  // :150: all four bytes
    if (t == 4) {                  // MessageTransportType, :153-190 (size >= MessageTransportSize holds)
      key = session_get(slots, n_slots, le32(msg + 4));  // :159-166
      if (key != kSessionEmpty) type = 4;
    } else if ((t == 1 && size == 148) || (t == 2 && size == 92) || (t == 3 && size == 64)) {  // :192-203
      type = (int32_t)t;
    }
  }
  wgcs_aead_pkt pk;
  pk.off = off;
  pk.counter = 0;
  pk.len = len;
  pk.key = key;
  pkts[q] = pk;
  types[q] = type;
}

// Router.Find of the address in the IP header at p: IPv4 (at least 20 bytes)
// at byte at4, IPv6 (at least 40) at byte at6.  Both families go through one
// walk, so a wave with both kinds of packet walks once, not twice.  False for a
// packet that has no such address (*peer = WGCS_PEER_NONE); a walk that the
// image fails (not an image, an index past its node count) comes back as *bad.
__device__ inline bool find_at(const uint8_t* __restrict__ image, uint64_t image_bytes, const uint8_t* p, int32_t len,
                               int at4, int at6, uint32_t* peer, bool* bad) {
  const uint32_t version = p[0] >> 4;
  const bool v4 = version == 4 && len >= 20, v6 = version == 6 && len >= 40;
  *peer = WGCS_PEER_NONE;
  *bad = false;
  if (!v4 && !v6) return false;
  uint32_t a[4] = {0, 0, 0, 0};
  route_addr_words(p + (v6 ? at6 : at4), v6 ? 4 : 1, a);
  *bad = route_image_find(image, image_bytes, a, v6, peer) != WGCS_OK;
  return true;
}

// verdict may alias pkt_len: row i is read, then written, by the one lane that owns it
__global__ __launch_bounds__(kThreads) void recv_source_kernel(const uint8_t* __restrict__ arena,
                                                               const wgcs_aead_pkt* __restrict__ pkts,
                                                               const int32_t* pkt_len,
                                                               const uint32_t* __restrict__ key_peer, uint32_t n_keys,
                                                               uint32_t n, const uint8_t* __restrict__ image,
                                                               uint64_t image_bytes, int32_t* verdict,
                                                               uint32_t* __restrict__ peer_out) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t len = pkt_len[i];
  int32_t v = len;
  uint32_t peer = WGCS_PEER_NONE;
  if (len > 0) {  // receive.go:432-435: a keepalive, and every error of Open, passes through
    const wgcs_aead_pkt pk = pkts[i];
    if (pk.key >= n_keys) {
      v = WGCS_ERR_INVALID_ARG;
    } else {
      bool bad;
      // :438-478: the source at [12, 16) of an IPv4, [8, 24) of an IPv6 packet
      if (!find_at(image, image_bytes, arena + pk.off + kTransportContent, len, 12, 8, &peer, &bad))
        v = WGCS_ERR_PACKET_TOO_SHORT;  // :440-442, :460-462, :479-481
      else if (bad) v = WGCS_ERR_INVALID_ARG;
      else if (peer != key_peer[pk.key]) v = WGCS_ERR_SOURCE;  // no route: WGCS_PEER_NONE is no peer id
    }
  }
  verdict[i] = v;
  if (peer_out) peer_out[i] = peer;
}

__global__ __launch_bounds__(kThreads) void route_dst_kernel(const uint8_t* __restrict__ arena,
                                                             const uint64_t* __restrict__ off_tab, uint64_t stride,
                                                             uint32_t offset, const int32_t* __restrict__ sizes,
                                                             uint32_t n, const uint8_t* __restrict__ image,
                                                             uint64_t image_bytes, uint32_t* __restrict__ peer_out) {
  const uint32_t q = blockIdx.x * kThreads + threadIdx.x;
  if (q >= n) return;
  const int32_t size = sizes[q];
  uint32_t peer = WGCS_PEER_NONE;
  if (size >= 1) {  // send.go:267-269
    bool bad;
    // :275-287: the destination at [16, 20) of an IPv4, [24, 40) of an IPv6 packet
    find_at(image, image_bytes, arena + (off_tab ? off_tab[q] : (uint64_t)q * stride) + offset, size, 16, 24, &peer, &bad);
  }
  peer_out[q] = peer;  // :291-293: nil is dropped by the caller
}

inline uint32_t blocks_for(uint32_t n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

hipError_t launch_recv_classify(const uint8_t* arena, const uint64_t* off, uint64_t stride, const int32_t* sizes,
                                uint32_t n, const wgcs_session_slot* slots, uint32_t n_slots, wgcs_aead_pkt* pkts,
                                int32_t* types, hipStream_t s) {
  hipLaunchKernelGGL(recv_classify_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, arena, off, stride, sizes, n,
                     slots, n_slots, pkts, types);
  return hipGetLastError();
}

hipError_t launch_recv_source(const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* pkt_len,
                              const uint32_t* key_peer, uint32_t n_keys, uint32_t n, const uint8_t* image,
                              uint64_t image_bytes, int32_t* verdict, uint32_t* peer, hipStream_t s) {
  hipLaunchKernelGGL(recv_source_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, arena, pkts, pkt_len, key_peer,
                     n_keys, n, image, image_bytes, verdict, peer);
  return hipGetLastError();
}

hipError_t launch_route_dst(const uint8_t* arena, const uint64_t* off, uint64_t stride, uint32_t offset,
                            const int32_t* sizes, uint32_t n, const uint8_t* image, uint64_t image_bytes,
                            uint32_t* peer, hipStream_t s) {
  hipLaunchKernelGGL(route_dst_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, s, arena, off, stride, offset, sizes, n,
                     image, image_bytes, peer);
  return hipGetLastError();
}

}  // namespace wgcs
