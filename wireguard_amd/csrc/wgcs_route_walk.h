// wgcs_route_walk.h -- the read side of the peer lookup, shared by host and
// device: Router.Find (device/router.go:374-403) on a flat image of the two
// allowed-IPs tries, and SessionMap.Get (device/sessions.go:26-30) on an
// open-addressed slot array.  route_kernels.hip, router.cpp
// (wgcs_router_image_find, wgcs_session_table_build) and the stand-alone
// sanitizer program of tests/route_host/ include this one text.
//
// Image layout (private to the library, little-endian, 16-byte aligned on the
// device):
//   header, 32 B: magic | version | node count | IPv4 root | IPv6 root | 0 0 0
//   node i, 32 B at 32 + 32*i:
//     addr[4]   the masked address as big-endian 32-bit words (IPv4: word 0)
//     child[2]  node indices, kRouteNone for nil
//     peer      the peer id, WGCS_PEER_NONE for an empty node (peer == nil)
//     cidr
// An image is data from outside the walk: every index read from it is checked
// against the header's node count, and a path's cidr must strictly increase,
// so a walk visits at most 129 nodes (cidr 0..128) whatever the bytes are.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/wgcsum.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WGCS_HD __host__ __device__ inline
#else
#define WGCS_HD inline
#endif

namespace wgcs {

constexpr uint32_t kRouteMagic = 0x54524757u;  // "WGRT"
constexpr uint32_t kRouteVersion = 1;
constexpr uint32_t kRouteNone = 0xFFFFFFFFu;
constexpr uint32_t kRouteHeaderBytes = 32;
constexpr uint32_t kRouteNodeBytes = 32;
constexpr int kRouteMaxVisits = 129;

struct RouteHeader {
  uint32_t magic, version, n_nodes, root4, root6, pad[3];
};
struct RouteNode {
  uint32_t addr[4];
  uint32_t child[2];
  uint32_t peer;
  uint32_t cidr;
};
static_assert(sizeof(RouteHeader) == kRouteHeaderBytes && sizeof(RouteNode) == kRouteNodeBytes, "image layout");

// 32 image bytes at p.  On the device the image is 16-byte aligned (the entry
// points check it), so this is two dwordx4 loads; host images may sit anywhere.
template <typename T>
WGCS_HD T route_load(const uint8_t* p) {
  T v;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 lo = q[0], hi = q[1];
  uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  memcpy(&v, w, sizeof v);
#else
  memcpy(&v, p, sizeof v);
#endif
  return v;
}

WGCS_HD uint32_t route_clz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__clz((int)x);  // 32 for 0
#else
  return x ? (uint32_t)__builtin_clz(x) : 32u;
#endif
}

// commonBits(ip1, ip2), router.go:63-91, on big-endian words (words = 1 or 4):
// the number of equal leading bits, 32 or 128 for equal addresses.
WGCS_HD uint32_t route_common_bits(const uint32_t* a, const uint32_t* b, int words) {
  uint32_t bits = 0;
  for (int i = 0; i < words; ++i) {
    const uint32_t x = a[i] ^ b[i];
    if (x) return bits + route_clz32(x);
    bits += 32;
  }
  return bits;
}

// bit `cidr` of the address, counted from the most significant one:
// node.childIndex, router.go:95-97, with index = cidr / 8, shift = 7 - cidr % 8
WGCS_HD uint32_t route_child_index(const uint32_t* a, uint32_t cidr) { return (a[cidr >> 5] >> (31 - (cidr & 31))) & 1u; }

// The address bytes (4 or 16, any alignment) as big-endian words.
WGCS_HD void route_addr_words(const uint8_t* p, int words, uint32_t* out) {
  for (int i = 0; i < words; ++i)
    out[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
}

// node.find, router.go:374-403, on an image of image_bytes bytes.  *peer = the
// peer of the longest matching prefix or WGCS_PEER_NONE.  Returns WGCS_OK, or
// WGCS_ERR_INVALID_ARG (*peer = WGCS_PEER_NONE) for an image that is not one:
// too short for its header or its node count, wrong magic or version, an index
// at or past the node count, a cidr beyond the address or not above its
// parent's.  Never reads outside [image, image + image_bytes).
WGCS_HD int route_image_find(const uint8_t* image, uint64_t image_bytes, const uint32_t* addr, int is_v6,
                             uint32_t* peer) {
  *peer = 0xFFFFFFFFu;
  if (image_bytes < kRouteHeaderBytes) return WGCS_ERR_INVALID_ARG;
  const RouteHeader h = route_load<RouteHeader>(image);
  if (h.magic != kRouteMagic || h.version != kRouteVersion) return WGCS_ERR_INVALID_ARG;
  if (h.n_nodes > (image_bytes - kRouteHeaderBytes) / kRouteNodeBytes) return WGCS_ERR_INVALID_ARG;
  const int words = is_v6 ? 4 : 1;
  const uint32_t ip_bits = is_v6 ? 128u : 32u;
  uint32_t n = is_v6 ? h.root6 : h.root4;
  uint32_t found = 0xFFFFFFFFu;
  int64_t above = -1;  // the cidr of the node this one hangs under
  for (int visit = 0; n != kRouteNone; ++visit) {
    if (n >= h.n_nodes || visit >= kRouteMaxVisits) return WGCS_ERR_INVALID_ARG;
    const RouteNode nd = route_load<RouteNode>(image + kRouteHeaderBytes + (uint64_t)n * kRouteNodeBytes);
    if (nd.cidr > ip_bits || (int64_t)nd.cidr <= above) return WGCS_ERR_INVALID_ARG;
    above = nd.cidr;
    if (route_common_bits(nd.addr, addr, words) < nd.cidr) break;  // :379
    if (nd.peer != 0xFFFFFFFFu) found = nd.peer;                    // :380-382
    if (nd.cidr == ip_bits) break;                                  // :397-399, n.index == ipLen
    n = nd.child[route_child_index(addr, nd.cidr)];                 // :400
  }
  *peer = found;
  return WGCS_OK;
}

// ---- SessionMap.Get on the slot array wgcs_session_table_build fills ----
// Linear probing from a multiplicative hash; a slot whose key is 0xFFFFFFFF is
// empty and ends the probe, and a probe never runs past n_slots slots.
constexpr uint32_t kSessionEmpty = 0xFFFFFFFFu;

WGCS_HD uint32_t session_hash(uint32_t index) {
  uint32_t h = index * 0x9E3779B1u;
  return h ^ (h >> 15);
}

// the key index of `index`, or kSessionEmpty; n_slots is a power of two
WGCS_HD uint32_t session_get(const wgcs_session_slot* slots, uint32_t n_slots, uint32_t index) {
  const uint32_t mask = n_slots - 1;
  uint32_t at = session_hash(index) & mask;
  for (uint32_t probe = 0; probe < n_slots; ++probe, at = (at + 1) & mask) {
    const wgcs_session_slot s = slots[at];
    if (s.key == kSessionEmpty) return kSessionEmpty;
    if (s.index == index) return s.key;
  }
  return kSessionEmpty;
}

}  // namespace wgcs
