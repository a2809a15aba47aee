// wgcs_endpoint.h -- peer.endpoint as scalar row functions, shared by host and
// device:
//   the control-message walk   ParseOneSocketControlMessage in the loop of conn/gso.go:42 and
//                              conn/sticky.go:54, which getGSOSize and getSrcFromControl share
//   recv        the tail of ReceiveIPvX       conn/bind.go:308-319, conn/sticky.go:46-94
//   set         SetEndpointFromPacket         device/peer.go:281-286 at receive.go:487, :314, :335
//   dst         Peer.Send up to bind.Send     peer.go:201-211, with ClearSrc
// Each pass is a body that wgcs_each.h runs one lane per row and endpoint.cpp in
// row order, set and dst over the sources of wgcs_events.h; udp_msgs_api.cpp
// takes the walk for wgcs_get_gso_size, and the stand-alone sanitizer program of
// tests/endpoint_host/ includes this one text.
//
// Several rows of a set call may belong to one peer.  The reference takes them
// in turn, so the last one's endpoint stands; here every candidate raises the
// peer's claim word to its index + 1 in a first pass, and in a second pass the
// one that holds the claim stores the 64 bytes and puts the claim back to 0.
// A dst call reads in its first pass and clears in its second, and every lane
// that clears stores zeros, so the tables come out the same whichever wave ran
// first.
//
// A wgcs_endpoint row is read and written as sixteen 4-byte words: dst in
// words 0..4 (dst.len is byte 2 of word 4), src_len and its pad in word 5, src
// in words 6..15.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_bounds.h"
#include "wgcs_timers.h"

namespace wgcs {

static_assert(sizeof(wgcs_src_addr) == 20 && offsetof(wgcs_src_addr, len) == 18, "row layout");
static_assert(sizeof(wgcs_endpoint) == 64 && offsetof(wgcs_endpoint, src_len) == 20 && offsetof(wgcs_endpoint, src) == 24,
              "row layout");

constexpr uint32_t kEpWords = 16, kEpAddrWords = 5, kEpLenWord = 4, kEpSrcLen = 5, kEpSrc = 6, kEpSrcWords = 10;

// ---- the control messages of one recvmsg, golang.org/x/sys/unix on linux/amd64 ----

constexpr size_t kCmsgHdrSize = 16;           // SizeofCmsghdr: Len uint64, Level int32, Type int32
constexpr int32_t kCmsgSolUdp = 17, kCmsgUdpGro = 104;            // linux/udp.h
constexpr int32_t kCmsgIpProtoIp = 0, kCmsgIpPktinfo = 8;        // linux/in.h
constexpr int32_t kCmsgIpProtoIpv6 = 41, kCmsgIpv6Pktinfo = 50;  // linux/in6.h
constexpr uint32_t kCmsgSpacePktinfo4 = 32, kCmsgSpacePktinfo6 = 40;  // CmsgSpace(SizeofInet4Pktinfo = 12 / Inet6 = 20)
constexpr int kCmsgNone = 0, kCmsgOne = 1;    // cmsg_next: the loop is over; a message was parsed

WGCS_HD size_t cmsg_align(size_t n) { return (n + 7) & ~size_t(7); }

// LE32 of control[off, off + 4), the bytes at and past `limit` read as zero.  The device reads
// the aligned word: there control is 4-byte aligned, off a multiple of 4, and the buffer is
// readable through limit rounded up to 4.  The host reads the bytes below limit and no other.
WGCS_HD uint32_t cmsg_load32(const uint8_t* control, size_t off, size_t limit) {
  if (off >= limit) return 0;
  const size_t have = limit - off;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t w = *(const uint32_t*)(control + off);
  return have >= 4 ? w : w & ((1u << (8 * (uint32_t)have)) - 1u);
#else
  uint32_t w = 0;
  for (size_t i = 0; i < 4 && i < have; ++i) w |= (uint32_t)control[off + i] << (8 * i);
  return w;
#endif
}

struct CmsgWalk {  // remaining = control[off, off + rlen)
  size_t off, rlen;
};

struct CmsgHdr {
  uint64_t len;  // Cmsghdr.Len as received
  int32_t level, type;
  size_t at;  // where the message starts in control
};

// One turn of `for len(remaining) > unix.SizeofCmsghdr { ParseOneSocketControlMessage(remaining) }`:
// kCmsgNone when the loop is over, WGCS_ERR_CMSG for the EINVAL of a Len below 16 or past the
// rest, else kCmsgOne with *h filled and *w moved to the remainder (empty unless
// cmsgAlignOf(Len) lies inside the rest).
WGCS_HD int cmsg_next(const uint8_t* control, CmsgWalk* w, CmsgHdr* h) {
  if (w->rlen <= kCmsgHdrSize) return kCmsgNone;  // strictly greater, conn/gso.go:42 and conn/sticky.go:54
  const size_t limit = w->off + w->rlen;
  h->at = w->off;
  h->len = (uint64_t)cmsg_load32(control, w->off, limit) | ((uint64_t)cmsg_load32(control, w->off + 4, limit) << 32);
  h->level = (int32_t)cmsg_load32(control, w->off + 8, limit);
  h->type = (int32_t)cmsg_load32(control, w->off + 12, limit);
  if (h->len < kCmsgHdrSize || h->len > w->rlen) return WGCS_ERR_CMSG;
  const size_t adv = cmsg_align((size_t)h->len);
  if (adv < w->rlen) {
    w->off += adv;
    w->rlen -= adv;
  } else {
    w->rlen = 0;
  }
  return kCmsgOne;
}

// getGSOSize(control), conn/gso.go:35-67: the UDP_GRO size of the first such message that
// carries two bytes, 0 without one, WGCS_ERR_CMSG for a parse error
WGCS_HD int cmsg_gso_size(const uint8_t* control, size_t len, int* gso) {
  *gso = 0;
  CmsgWalk w = {0, len};
  CmsgHdr h;
  for (int rc; (rc = cmsg_next(control, &w, &h)) != kCmsgNone;) {
    if (rc < 0) return rc;
    if (h.level == kCmsgSolUdp && h.type == kCmsgUdpGro && h.len - kCmsgHdrSize >= 2) {  // :55-64
      *gso = (int)(cmsg_load32(control, h.at + kCmsgHdrSize, h.at + kCmsgHdrSize + 2));
      return WGCS_OK;
    }
  }
  return WGCS_OK;
}

// getSrcFromControl(control, endpoint), conn/sticky.go:46-94: *src_len = len(endpoint.src) and
// src[0, 10) its bytes as words, zero at and past src_len.  The header is copied as received,
// Len included; data = control[at + 16 : at + Len] is cut to the room behind the header.
WGCS_HD void endpoint_src_from_control(const uint8_t* control, size_t len, uint32_t* src_len, uint32_t src[kEpSrcWords]) {
  *src_len = 0;  // ClearSrc
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < kEpSrcWords; ++i) src[i] = 0;
  CmsgWalk w = {0, len};
  CmsgHdr h;
  while (cmsg_next(control, &w, &h) == kCmsgOne) {  // a parse error returns with the source empty
    uint32_t space;
    if (h.level == kCmsgIpProtoIp && h.type == kCmsgIpPktinfo) space = kCmsgSpacePktinfo4;
    else if (h.level == kCmsgIpProtoIpv6 && h.type == kCmsgIpv6Pktinfo) space = kCmsgSpacePktinfo6;
    else continue;
    *src_len = space;
    src[0] = (uint32_t)h.len;
    src[1] = (uint32_t)(h.len >> 32);
    src[2] = (uint32_t)h.level;
    src[3] = (uint32_t)h.type;
    const size_t room = space - kCmsgHdrSize, data = (size_t)h.len - kCmsgHdrSize;
    const size_t from = h.at + kCmsgHdrSize, limit = from + (data < room ? data : room);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < kEpSrcWords - 4; ++i) src[4 + i] = cmsg_load32(control, from + 4 * i, limit);
    return;
  }
}

// ---- rows ----

WGCS_HD uint32_t* endpoint_words(wgcs_endpoint* e) { return (uint32_t*)e; }
WGCS_HD const uint32_t* endpoint_words(const wgcs_endpoint* e) { return (const uint32_t*)e; }

// dst.len of the row whose word 4 is w: 0 is "no endpoint", 6 and 18 are addresses
WGCS_HD uint32_t endpoint_dst_len(uint32_t w) { return (w >> 16) & 0xFFu; }

WGCS_HD void endpoint_store(wgcs_endpoint* e, const uint32_t row[kEpWords]) {
  uint32_t* const w = endpoint_words(e);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t i = 0; i < kEpWords; ++i) w[i] = row[i];
}

// ---- bind.go:308-319 for slot q of a receive batch ----

struct EndpointRecv {
  uint32_t n_msgs;
  const wgcs_src_addr* addr;
  const int32_t *from, *size;
  const uint8_t* oob;
  uint32_t oob_stride;
  const int32_t* nn;
  wgcs_endpoint* ep;
  wgcs_src_addr* addr_out;
  WGCS_HD void operator()(uint32_t q) const {
    uint32_t row[kEpWords];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < kEpWords; ++i) row[i] = 0;
    const int32_t f = from ? from[q] : -1;
    if (size[q] != 0 && f >= -1 && f < (int32_t)n_msgs) {  // :311-313: a slot of size 0 gets no endpoint
      // :314: msg.Addr, which splitMessages copied from message f of the batch (bind.go:570)
      const uint32_t a = f < 0 ? q : q - q % n_msgs + (uint32_t)f;
      const uint32_t* const aw = (const uint32_t*)(addr + a);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t i = 0; i < kEpAddrWords; ++i) row[i] = aw[i];
      // :317: msg.OOB[:msg.NN] of slot q itself
      const int32_t c = nn[q];
      const size_t len = c < 0 || (uint32_t)c > oob_stride ? 0 : (size_t)c;
      endpoint_src_from_control(oob + (uint64_t)q * oob_stride, len, &row[kEpSrcLen], row + kEpSrc);
    }
    endpoint_store(ep + q, row);
    if (addr_out) {
      uint32_t* const o = (uint32_t*)(addr_out + q);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t i = 0; i < kEpAddrWords; ++i) o[i] = row[i];
    }
  }
};

// ---- SetEndpointFromPacket, peer.go:281-286, in two passes ----

struct EndpointPick {
  uint32_t row;  // the peer row that takes an endpoint, or WGCS_PEER_NONE for no candidate
  uint32_t src;  // the row of ep it takes
};

// the row of ep that entry i of a set call's source brings: receive.go:487 (a tail < 0 lies past n_rows), :314, :335
WGCS_HD uint32_t endpoint_src(const GroupRows& s, uint32_t c) { return (uint32_t)s.tail(c); }
WGCS_HD uint32_t endpoint_src(const AcceptedRows& s, uint32_t j) { return s.init_row(j); }
WGCS_HD uint32_t endpoint_src(const FinishedRows&, uint32_t q) { return q; }

// the pick of entry i: its peer row if its row of ep lies in the table and holds an address
template <class Rows>
WGCS_HD EndpointPick endpoint_pick(const Rows& s, uint32_t i, const wgcs_endpoint* ep, uint32_t n_rows) {
  const uint32_t src = endpoint_src(s, i);
  if (src >= n_rows) return {WGCS_PEER_NONE, 0};
  const uint32_t row = s.row(i);
  if (row == WGCS_PEER_NONE) return {WGCS_PEER_NONE, 0};
  const uint32_t len = endpoint_dst_len(endpoint_words(ep + src)[kEpLenWord]);
  return {len == 6 || len == 18 ? row : WGCS_PEER_NONE, src};
}

// the first pass: candidate i claims its peer's row
template <class Rows>
struct EndpointSetClaim {
  Rows src;
  const wgcs_endpoint* ep;
  uint32_t n_rows;
  uint32_t* claim;
  WGCS_HD void operator()(uint32_t i) const {
    const EndpointPick p = endpoint_pick(src, i, ep, n_rows);
    if (p.row != WGCS_PEER_NONE) claim_max(claim + p.row, i + 1);
  }
};

// the second pass: the holder of the claim, the highest candidate of its peer, leaves its endpoint
template <class Rows>
struct EndpointSetCommit {
  Rows src;
  const wgcs_endpoint* ep;
  uint32_t n_rows;
  wgcs_endpoint* table;
  uint32_t* claim;
  wgcs_timers* timers;
  WGCS_HD void operator()(uint32_t i) const {
    const EndpointPick p = endpoint_pick(src, i, ep, n_rows);
    if (p.row == WGCS_PEER_NONE) return;
    if (claim[p.row] != i + 1) return;  // a higher candidate's, or 0 once that one has committed: never i + 1
    const uint32_t* const s = endpoint_words(ep + p.src);
    uint32_t row[kEpWords];  // read whole, then stored: no member says that ep and table are apart
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < kEpWords; ++k) row[k] = s[k];
    endpoint_store(table + p.row, row);                             // peer.go:284
    timers_and(&timers[p.row].flags, ~WGCS_TIMERS_CLEAR_SRC);       // :285
    claim[p.row] = 0;
  }
};

// ---- Peer.Send up to bind.Send, peer.go:201-211, in two passes ----

// The first pass, entry j: d_dst[j], d_dst_v6[j] and the status, which read() returns too.
// Neither table is written.
template <class Rows>
struct EndpointDstRead {
  Rows src;
  const wgcs_endpoint* table;
  const wgcs_timers* timers;
  wgcs_endpoint* dst;
  int32_t *dst_v6, *dst_status;
  WGCS_HD void operator()(uint32_t j) const { read(j, src.row(j)); }
  WGCS_HD int32_t read(uint32_t j, uint32_t row) const {
    uint32_t out[kEpWords];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < kEpWords; ++i) out[i] = 0;
    int32_t status = WGCS_OK, v6 = 0;
    if (row != WGCS_PEER_NONE) {
      const uint32_t* const t = endpoint_words(table + row);
      const uint32_t len = endpoint_dst_len(t[kEpLenWord]);
      if (len == 0) {
        status = WGCS_ERR_NO_ENDPOINT;  // peer.go:202-205: returns before clearSrcOnTx is looked at
      } else {
        const bool clear = (timers[row].flags & WGCS_TIMERS_CLEAR_SRC) != 0;  // :206-209
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < kEpWords; ++i) out[i] = clear && i >= kEpSrcLen ? 0u : t[i];
        v6 = len == 18;  // DstIP().Is6(): every 16-byte address, conn/bind.go:405
      }
    }
    endpoint_store(dst + j, out);
    dst_v6[j] = v6;
    dst_status[j] = status;
    return status;
  }
};

// The first pass of the send jobs' form: no message for a job without an endpoint, and the
// bytes of peer.go:213-218 for one with a destination.
struct EndpointDstJobs {
  EndpointDstRead<KeptJobRows> rd;
  const int32_t* lens;
  int32_t* nbufs;
  uint64_t* tx_bytes;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = rd.src.row(j);
    const int32_t status = rd.read(j, row);
    const uint32_t max_segs = rd.src.jobs.max_segs;
    uint64_t tx = 0;
    if (status == WGCS_ERR_NO_ENDPOINT) {
      nbufs[j] = 0;
    } else if (row != WGCS_PEER_NONE) {
      const int32_t nb = nbufs[j];
      const uint32_t n = nb < 0 ? 0u : (uint32_t)nb > max_segs ? max_segs : (uint32_t)nb;
      const int32_t* const l = lens + (uint64_t)j * max_segs;
      for (uint32_t k = 0; k < n; ++k) tx += l[k] > 0 ? (uint64_t)l[k] : 0u;
    }
    tx_bytes[j] = tx;
  }
};

// The second pass: ClearSrc on the table row of a peer the first pass gave a cleared source, and
// clearSrcOnTx = false.  Every entry of the peer stores the same zeros.
template <class Rows>
struct EndpointDstClear {
  Rows src;
  wgcs_endpoint* table;
  wgcs_timers* timers;
  WGCS_HD void operator()(uint32_t j) const {
    const uint32_t row = src.row(j);
    if (row == WGCS_PEER_NONE) return;
    uint32_t* const t = endpoint_words(table + row);
    if (endpoint_dst_len(t[kEpLenWord]) == 0) return;  // no endpoint: the flag stays
    if (!(timers[row].flags & WGCS_TIMERS_CLEAR_SRC)) return;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = kEpSrcLen; i < kEpWords; ++i)
      if (t[i] != 0) t[i] = 0;
    timers_and(&timers[row].flags, ~WGCS_TIMERS_CLEAR_SRC);
  }
};

// ---- the argument rules the device entry points and the host forms share (host code) ----

inline bool endpoint_misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

inline bool endpoint_recv_args_ok(const wgcs_src_addr* addr, const int32_t* from, const int32_t* size, const uint8_t* oob,
                                  uint32_t oob_stride, const int32_t* nn, uint64_t n, const wgcs_endpoint* ep,
                                  const wgcs_src_addr* addr_out) {
  if (!addr || !size || !nn || !ep || (oob_stride && !oob) || n > kMaxRows || (oob_stride & 3)) return false;
  if (endpoint_misaligned(addr, 3) || endpoint_misaligned(from, 3) || endpoint_misaligned(size, 3) ||
      endpoint_misaligned(oob, 3) || endpoint_misaligned(nn, 3) || endpoint_misaligned(ep, 3) ||
      endpoint_misaligned(addr_out, 3))
    return false;
  const uint64_t ep_bytes = n * sizeof(wgcs_endpoint), out_bytes = addr_out ? n * sizeof(wgcs_src_addr) : 0;
  const void* const in[] = {addr, from, size, oob, nn};
  const uint64_t in_bytes[] = {n * sizeof(wgcs_src_addr), from ? n * 4 : 0, n * 4, n * oob_stride, n * 4};
  for (int i = 0; i < 5; ++i)
    if (overlap(ep, ep_bytes, in[i], in_bytes[i]) || overlap(addr_out, out_bytes, in[i], in_bytes[i])) return false;
  return !overlap(ep, ep_bytes, addr_out, out_bytes);
}

// the tables a set call writes against the source rows it reads
inline bool endpoint_set_tables_ok(const wgcs_endpoint* ep, uint64_t n_rows, const wgcs_endpoint* table,
                                   const uint32_t* claim, const wgcs_timers* timers, uint32_t n_peers) {
  if (n_peers > kMaxPeers || n_rows > kMaxRows || (n_rows && !ep) || (n_peers && (!table || !claim || !timers)))
    return false;
  if (endpoint_misaligned(ep, 3) || endpoint_misaligned(table, 3) || endpoint_misaligned(claim, 3) ||
      endpoint_misaligned(timers, 7))
    return false;
  const uint64_t t_bytes = (uint64_t)n_peers * sizeof(wgcs_endpoint), c_bytes = (uint64_t)n_peers * 4;
  const uint64_t tm_bytes = (uint64_t)n_peers * sizeof(wgcs_timers), e_bytes = n_rows * sizeof(wgcs_endpoint);
  return !overlap(table, t_bytes, ep, e_bytes) && !overlap(claim, c_bytes, ep, e_bytes) &&
         !overlap(timers, tm_bytes, ep, e_bytes) && !overlap(table, t_bytes, claim, c_bytes) &&
         !overlap(table, t_bytes, timers, tm_bytes) && !overlap(claim, c_bytes, timers, tm_bytes);
}

// the tables and the outputs of a dst call over n entries; tx_bytes is the jobs form's
inline bool endpoint_dst_tables_ok(uint64_t n, const wgcs_endpoint* table, const wgcs_timers* timers, uint32_t n_peers,
                                   const wgcs_endpoint* dst, const int32_t* dst_v6, const int32_t* dst_status,
                                   const uint64_t* tx_bytes, bool with_tx) {
  if (n > kMaxRows || n_peers > kMaxPeers || !dst || !dst_v6 || !dst_status || (with_tx && !tx_bytes) ||
      (n_peers && (!table || !timers)))
    return false;
  if (endpoint_misaligned(table, 3) || endpoint_misaligned(timers, 7) || endpoint_misaligned(dst, 3) ||
      endpoint_misaligned(dst_v6, 3) || endpoint_misaligned(dst_status, 3) || endpoint_misaligned(tx_bytes, 7))
    return false;
  const void* const out[] = {dst, dst_v6, dst_status, with_tx ? tx_bytes : nullptr};
  const uint64_t out_bytes[] = {n * sizeof(wgcs_endpoint), n * 4, n * 4, with_tx ? n * 8 : 0};
  const uint64_t t_bytes = (uint64_t)n_peers * sizeof(wgcs_endpoint), tm_bytes = (uint64_t)n_peers * sizeof(wgcs_timers);
  if (overlap(table, t_bytes, timers, tm_bytes)) return false;
  for (int i = 0; i < 4; ++i) {
    if (overlap(out[i], out_bytes[i], table, t_bytes) || overlap(out[i], out_bytes[i], timers, tm_bytes)) return false;
    for (int k = i + 1; k < 4; ++k)
      if (overlap(out[i], out_bytes[i], out[k], out_bytes[k])) return false;
  }
  return true;
}

}  // namespace wgcs
