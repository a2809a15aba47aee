// gso_device.h -- the GSO split's shared device code: the job decoder
// (decode_job), the byte-granular general path (gso_general_row), GSO_NONE
// (none_segment), the fast header, the row stream (stream_row), the decoded
// path (decode_publish, decoded_rows), finish_row and gso_rows_body.
// Included by gso_kernels.hip (the batch kernels) and ring_kernels.hip (the
// resident ring, which defines WGCS_RING_TU first: wgcs_copy.h then makes
// every load of request bytes a system-scope one).  The mapping and the
// reference quirks are described at the top of gso_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wgcsum.h"
#include "wgcs_common.h"
#include "wgcs_copy.h"
#include "wgcs_rows.h"
#include "wgcs_kernels.h"

namespace wgcs {

namespace {

constexpr int kMaxHdrLen = 240;  // header bytes held by the 16 lanes of a row (+ destination phase <= 15)

enum : int { GSO_NONE = 0, GSO_TCPV4 = 1, GSO_TCPV6 = 4, GSO_UDP_L4 = 5 };

__device__ __forceinline__ uint32_t u8at(const uint8_t* p) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)ldg8(p)); }
__device__ __forceinline__ uint32_t be16at(const uint8_t* p) { return (u8at(p) << 8) | u8at(p + 1); }

// The first 256 bytes of a job ([virtio hdr | packet...]) held across the
// wave, one byte per lane per register: a single batch of byte loads instead
// of a chain of dependent scalar reads.  byte(k) for uniform k < 256.
struct HdrBytes {
  uint32_t r0, r1, r2, r3;
  int len;
  const uint8_t* base;
  __device__ __forceinline__ void load(const uint8_t* vb, int n, int lane) {
    base = vb;
    len = n;
    r0 = lane < n ? ldg8(vb + lane) : 0u;
    r1 = lane + 64 < n ? ldg8(vb + lane + 64) : 0u;
    r2 = lane + 128 < n ? ldg8(vb + lane + 128) : 0u;
    r3 = lane + 192 < n ? ldg8(vb + lane + 192) : 0u;
  }
  __device__ __forceinline__ uint32_t operator()(int k) const {  // k wave-uniform
    if (k >= 256) return u8at(base + k);
    const int l = k & 63;
    const uint32_t v = k < 64 ? r0 : (k < 128 ? r1 : (k < 192 ? r2 : r3));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
  }
  __device__ __forceinline__ uint32_t le16(int k) const { return (*this)(k) | ((*this)(k + 1) << 8); }
  __device__ __forceinline__ uint32_t be16(int k) const { return ((*this)(k) << 8) | (*this)(k + 1); }
  __device__ __forceinline__ uint32_t be32(int k) const { return (be16(k) << 16) | be16(k + 2); }
};

struct Job {
  int status;    // 0 or WGCS_ERR_*
  int nseg;      // segments to write (<= max_segs)
  int count;     // return value n
  int type, flags, ipv;
  int hdr_len, gso, cs, co, plen;
  int spare;     // bytes of readBuf's spare capacity after the packet (WGCS_GSO_JOB_SPARE)
  int gen;       // 1: byte-granular general path (gso_general_row); 0: the row-streaming fast path
};

// Bytes of bufs[i][offset:] one gsoSplit segment writes (gro.go:1419-1488,
// oracle or_gso_split_need): the packet plus fixed-position header writes that
// may lie past it (IPv4 [2:12), IPv6 [4:6), seq / UDP length at csumStart+4,
// the flags byte on non-last segments, the checksum field; u16 positions).
__device__ __forceinline__ int split_need(const Job& j, int pkt_len, bool any_non_last) {
  const bool tcp = j.type != GSO_UDP_L4;
  int need = max(pkt_len, j.ipv == 4 ? 12 : 6);
  need = max(need, ((j.cs + 4) & 0xFFFF) + (tcp ? 4 : 2));
  if (tcp && any_non_last) need = max(need, ((j.cs + 13) & 0xFFFF) + 1);
  return max(need, ((j.cs + j.co) & 0xFFFF) + 2);
}

// Segment count / ErrTooManySegments (gro.go:1406-1410) + output room.
__device__ void count_segments(Job& j, uint32_t out_room, uint32_t max_segs) {
  const int plen = j.plen;
  long nseg = 0;
  if (j.hdr_len < plen) nseg = j.gso == 0 ? 0x7FFFFFFF : ((long)plen - j.hdr_len + j.gso - 1) / j.gso;
  if (nseg > 0) {  // segment 0 is the largest; Go panics on a bufs[0] slice shorter than what it writes
    const int first = j.hdr_len + min(j.gso, plen - j.hdr_len);
    const bool non_last = nseg > 1;
    if ((uint32_t)split_need(j, first, non_last) > out_room) { j.status = WGCS_ERR_OUT_OF_RANGE; return; }
  }
  if (nseg > (long)max_segs) {  // gro.go:1409-1410: all bufs written, n = i - 1
    j.nseg = (int)max_segs;
    j.count = (int)max_segs - 1;
    j.status = WGCS_ERR_TOO_MANY_SEGMENTS;
  } else {
    j.nseg = (int)nseg;
    j.count = (int)nseg;
  }
}

// gsoSplit's own bounds (gro.go:1387-1405 before the loop; :1419-1478 once it
// runs): an index the Go code would panic on is OUT_OF_RANGE.  Every position
// is the reference's uint16 sum.  The pseudo-header address slices may reach
// past len(readBuf) into the job's spare capacity (WGCS_GSO_JOB_SPARE), not
// past it.  Then: does the
// job fit the row-streaming path (header <= 240 bytes, IP header at least the
// fixed IPv4 / IPv6 size, checksum field inside the header), or does it take
// the byte-granular general path?
__device__ bool split_bounds(Job& j) {
  const int plen = j.plen;
  const bool v4 = j.ipv == 4, tcp = j.type != GSO_UDP_L4;
  const int ca = (j.cs + j.co) & 0xFFFF;
  if (v4 && plen < 12) return false;                           // readBuf[10], [11]
  if (ca + 2 > plen) return false;                             // readBuf[checksumAt+1]
  if (tcp && ((j.cs + 4) & 0xFFFF) + 4 > plen) return false;   // Uint32(readBuf[csumStart+4:])
  if (j.hdr_len < plen) {                                      // the loop runs
    if (j.cs > j.hdr_len) return false;                        // pkt[csumStart:hdrLen]
    if (plen + j.spare < (v4 ? 20 : 40)) return false;         // address slices: up to cap(readBuf)
  }
  // (and every per-segment L4 field inside the header: a seq / UDP length /
  // flags byte past hdrLen can land past a short segment's end, which only the
  // general path writes)
  j.gen = !(j.cs >= (v4 ? 20 : 40) && ca + 2 <= j.hdr_len && j.hdr_len <= kMaxHdrLen &&
            j.cs + (tcp ? 14 : 6) <= j.hdr_len);
  return true;
}

// handleVirtioRead's checks (tun/tun.go:522-630), then gsoSplit's.
__device__ Job decode_job(const HdrBytes& hb, uint32_t len, uint32_t jflags, uint32_t out_room, uint32_t max_segs) {
  Job j = {};
  if (len < 10) { j.status = WGCS_ERR_SHORT_BUFFER; return j; }  // gro.go:84-86
  j.flags = (int)hb(0);
  j.type = (int)hb(1);
  j.hdr_len = (int)hb.le16(2);
  j.gso = (int)hb.le16(4);
  j.cs = (int)hb.le16(6);
  j.co = (int)hb.le16(8);
  const int plen = (int)len - 10;
  j.plen = plen;
  j.spare = (int)((jflags >> 8) & 0xFFu);
  if (jflags & WGCS_GSO_JOB_RAW) {  // gsoSplit with the caller's header (gro.go:1373)
    j.ipv = (jflags & WGCS_GSO_JOB_V6) ? 6 : 4;
    if (j.type != GSO_TCPV4 && j.type != GSO_TCPV6) j.type = GSO_UDP_L4;  // protocol choice :1398-1405
    if (!split_bounds(j)) { j.status = WGCS_ERR_OUT_OF_RANGE; return j; }
    count_segments(j, out_room, max_segs);
    return j;
  }
  if (j.type == GSO_NONE) {  // tun/tun.go:532-556
    if (j.flags & 1) {
      const int at = (j.cs + j.co) & 0xFFFF;
      if (at + 2 > plen || j.cs > plen) { j.status = WGCS_ERR_OUT_OF_RANGE; return j; }
    }
    if ((uint32_t)plen > out_room) { j.status = WGCS_ERR_READ_OVERFLOW; return j; }
    j.nseg = 1;
    j.count = 1;
    return j;
  }
  if (j.type != GSO_TCPV4 && j.type != GSO_TCPV6 && j.type != GSO_UDP_L4) {
    j.status = WGCS_ERR_UNSUPPORTED_GSO;  // :564-568
    return j;
  }
  if (plen < 1) { j.status = WGCS_ERR_OUT_OF_RANGE; return j; }
  j.ipv = (int)(hb(10) >> 4);  // :570
  if (j.ipv == 4) {
    if (j.type != GSO_TCPV4 && j.type != GSO_UDP_L4) { j.status = WGCS_ERR_IP_GSO_MISMATCH; return j; }
  } else if (j.ipv == 6) {
    if (j.type != GSO_TCPV6 && j.type != GSO_UDP_L4) { j.status = WGCS_ERR_IP_GSO_MISMATCH; return j; }
  } else {
    j.status = WGCS_ERR_BAD_IP_VERSION;
    return j;
  }
  if (j.type == GSO_UDP_L4) {  // :597-614
    j.hdr_len = (j.cs + 8) & 0xFFFF;
  } else {
    const int at = (j.cs + 12) & 0xFFFF;
    if (plen <= at) { j.status = WGCS_ERR_PACKET_TOO_SHORT; return j; }
    const int th = (int)((hb(10 + at) >> 4) * 4);
    if (th < 20 || th > 60) { j.status = WGCS_ERR_TCP_HDR_LEN; return j; }
    j.hdr_len = (j.cs + th) & 0xFFFF;
  }
  if (plen < j.hdr_len) { j.status = WGCS_ERR_HDR_LEN; return j; }               // :615-621
  const int csum_at = (j.cs + j.co) & 0xFFFF;
  if (csum_at + 1 >= plen) { j.status = WGCS_ERR_CSUM_OFFSET; return j; }        // :622-630
  if (!split_bounds(j)) { j.status = WGCS_ERR_OUT_OF_RANGE; return j; }
  count_segments(j, out_room, max_segs);
  return j;
}

// ---------------------------------------------------------------------------
// General path: one 16-lane row per segment, byte-granular, for every header
// geometry the reference accepts that the row-streaming path does not take
// (IP headers shorter than 20 / 40 bytes, headers over 240 bytes, checksum
// fields outside the header or wrapped past 2^16).  Each output byte is the
// last value gsoSplit's write sequence leaves at its position
// (gro.go:1419-1488, in order: IP header copy, id / length / IPv4 checksum,
// L4 header copy, seq + flags or UDP length, payload, L4 checksum), computed
// from readBuf with its zeroed fields (:1388, :1393).  Three passes over the
// segment's chunks: IPv4 header sum, L4 sum, store.
struct GenSeg {
  const uint8_t* rb;
  int plen, cs, hdr_len, ca, s4, f13, i;
  int seg_start, pkt_len;
  bool v4, tcp, last;
  uint32_t id45;    // IPv4 bytes 4-5 after the id step (i > 0: BE16 + 1)
  uint32_t seq, ulen;
  uint32_t ipc;     // IPv4 header checksum (bytes 10-11)
};

// readBuf byte x after gsoSplit zeroed its IPv4 checksum and L4 checksum fields
__device__ __forceinline__ uint32_t rbz(const GenSeg& g, int x) {
  if ((g.v4 && (x == 10 || x == 11)) || x == g.ca || x == g.ca + 1) return 0u;
  return ldg8(g.rb + x);
}

// byte x of the IP header after the id / length writes (x < csumStart = iphLen)
__device__ __forceinline__ uint32_t ip_stage(const GenSeg& g, int x) {
  if (g.v4) {
    if (x == 2) return ((uint32_t)g.pkt_len >> 8) & 0xFFu;
    if (x == 3) return (uint32_t)g.pkt_len & 0xFFu;
    if (x == 4) return g.id45 >> 8;
    if (x == 5) return g.id45 & 0xFFu;
  } else {
    const uint32_t pl = (uint32_t)(g.pkt_len - g.cs) & 0xFFFFu;  // :1439
    if (x == 4) return pl >> 8;
    if (x == 5) return pl & 0xFFu;
  }
  return rbz(g, x);
}

// byte x (< pkt_len) before the L4 checksum store
__device__ __forceinline__ uint32_t pre_csum(const GenSeg& g, int x) {
  if (x >= g.hdr_len) return rbz(g, g.seg_start + (x - g.hdr_len));  // payload (:1468)
  const int t = x - g.s4;
  if (g.tcp && t >= 0 && t < 4) return (g.seq >> (24 - 8 * t)) & 0xFFu;
  if (!g.tcp && t >= 0 && t < 2) return (g.ulen >> (8 - 8 * t)) & 0xFFu;
  uint32_t b;
  if (x >= g.cs) b = rbz(g, x);
  else if (g.v4 && x == 10) b = g.ipc >> 8;
  else if (g.v4 && x == 11) b = g.ipc & 0xFFu;
  else b = ip_stage(g, x);
  if (g.tcp && !g.last && x == g.f13) b &= ~0x09u;  // FIN|PSH (:1447-1459)
  return b;
}

// One segment on one 16-lane row (lane r): the three passes, then sizes[].
__device__ void gso_general_row(const uint8_t* rb, int plen, int type, int ipv, int hdr_len, int gso, int cs, int co,
                                int i, uint8_t* dst, int r, int32_t* size_out, bool tails) {
  GenSeg g;
  g.rb = rb;
  g.plen = plen;
  g.cs = cs;
  g.hdr_len = hdr_len;
  g.v4 = ipv == 4;
  g.tcp = type != GSO_UDP_L4;
  g.ca = (cs + co) & 0xFFFF;
  g.s4 = (cs + 4) & 0xFFFF;
  g.f13 = (cs + 13) & 0xFFFF;
  g.i = i;
  g.seg_start = hdr_len + i * gso;
  const int seg_end = min(plen, g.seg_start + gso);
  const int seg_len = seg_end - g.seg_start;
  g.pkt_len = hdr_len + seg_len;
  g.last = seg_end == plen;
  g.seq = 0;
  if (g.tcp) {  // firstSeq from the zeroed readBuf (:1402), u16 product (:1445)
    const uint32_t s0 = (rbz(g, g.s4) << 24) | (rbz(g, g.s4 + 1) << 16) | (rbz(g, g.s4 + 2) << 8) | rbz(g, g.s4 + 3);
    g.seq = s0 + (uint32_t)(uint16_t)((uint16_t)gso * (uint16_t)i);
  }
  g.ulen = (uint32_t)(uint16_t)(seg_len + (hdr_len - cs));  // :1462-1465
  g.id45 = 0;
  if (g.v4) {  // pkt[4:6] after copy(pkt, readBuf[:iphLen]); bytes past iphLen are what bufs[i] held (:1427)
    const uint32_t b4 = 4 < cs ? rbz(g, 4) : ldg8(dst + 4);
    const uint32_t b5 = 5 < cs ? rbz(g, 5) : ldg8(dst + 5);
    g.id45 = (b4 << 8) | b5;
    if (i > 0) g.id45 = (g.id45 + 1) & 0xFFFFu;  // quirk: id0 + 1 (:1426-1431)
  }
  // pass 1: IPv4 header checksum over pkt[:iphLen] after the id / length writes (:1434)
  g.ipc = 0;
  const int dalign = (int)((uintptr_t)dst & 15u);
  uint8_t* dbase = dst - dalign;
  if (g.v4) {
    uint64_t acc = 0;
    for (int x = r; x < cs; x += 16) acc += (uint64_t)ip_stage(g, x) << ((x & 1) ? 0 : 8);
    const uint32_t t = fold32_16(row16_sum_u32(fold64_16(acc)));
    g.ipc = (~t) & 0xFFFFu;
  }
  // pass 2: L4 sum over pkt[csumStart:pktLen] + the pseudo header (:1469-1483)
  uint64_t acc = 0;
  for (int x = cs + r; x < g.pkt_len; x += 16) acc += (uint64_t)pre_csum(g, x) << (((x - cs) & 1) ? 0 : 8);
  {
    const int a_lo = g.v4 ? 12 : 8, a_n = g.v4 ? 4 : 16;  // address words (readBuf, zeroed fields)
    if (r < a_n) acc += (rbz(g, a_lo + 2 * r) << 8) | rbz(g, a_lo + 2 * r + 1);
  }
  const uint32_t tlen = (uint32_t)(uint16_t)(hdr_len - cs + seg_len);
  uint32_t t = fold32_16(row16_sum_u32(fold64_16(acc)));
  t = fold32_16(t + (g.tcp ? 6u : 17u) + tlen);
  const uint32_t l4c = (~t) & 0xFFFFu;
  // pass 3: every byte of the packet, the checksum last (:1485-1488)
  const int nk = (g.pkt_len + dalign + 15) >> 4;
  for (int k = r; k < nk; k += 16) {
    const int x0 = 16 * k - dalign;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const int x = x0 + b;
      uint32_t v = 0;
      if (x >= 0 && x < g.pkt_len) {
        if (x == g.ca) v = l4c >> 8;
        else if (x == g.ca + 1) v = l4c & 0xFFu;
        else v = pre_csum(g, x);
      }
      w[b >> 2] |= v << (8 * (b & 3));
    }
    store_chunk(dbase + 16 * k, make_uint4(w[0], w[1], w[2], w[3]), x0, g.pkt_len);
  }
  // The header writes that land past the packet's end (a header geometry with
  // fields beyond hdrLen and a short segment): gsoSplit writes them into
  // bufs[i] all the same, in its order -- id / length / IPv4 checksum (:1426-
  // 1439), seq + flags or UDP length (:1443-1466), the L4 checksum last
  // (:1485-1488).  Every position lies inside the slot: the decoder refused
  // (OUT_OF_RANGE) a slot shorter than segment 0's reach (split_need).  A
  // packed host region sized for the packets alone says !tails (GsoOutPos).
  if (r == 0 && tails) {
    auto put = [&](int x, uint32_t v) {
      if (x >= g.pkt_len) dst[x] = (uint8_t)v;
    };
    if (g.v4) {
      if (i > 0) {
        put(4, g.id45 >> 8);
        put(5, g.id45 & 0xFFu);
      }
      put(2, ((uint32_t)g.pkt_len >> 8) & 0xFFu);
      put(3, (uint32_t)g.pkt_len & 0xFFu);
      put(10, g.ipc >> 8);
      put(11, g.ipc & 0xFFu);
    } else {
      const uint32_t pl = (uint32_t)(g.pkt_len - cs) & 0xFFFFu;
      put(4, pl >> 8);
      put(5, pl & 0xFFu);
    }
    if (g.tcp) {
      for (int t = 0; t < 4; ++t) put(g.s4 + t, (g.seq >> (24 - 8 * t)) & 0xFFu);
      if (!g.last && g.f13 >= g.pkt_len) dst[g.f13] = (uint8_t)(ldg8(dst + g.f13) & ~0x09u);
    } else {
      put(g.s4, g.ulen >> 8);
      put(g.s4 + 1, g.ulen & 0xFFu);
    }
    put(g.ca, l4c >> 8);
    put(g.ca + 1, l4c & 0xFFu);
  }
  if (r == 0) *size_out = g.pkt_len;
}
// gsoNoneChecksum + copy to bufs[0] (tun/tun.go:532-556, gro.go:1497-1517).
__device__ void none_segment(const uint8_t* rb, const Job& j, uint8_t* dst, int lane) {
  const int plen = j.plen;
  int pf = -1;
  uint32_t pv = 0;
  if (j.flags & 1) {
    const int cs = j.cs;
    const int at = (j.cs + j.co) & 0xFFFF;
    const uint32_t initial = be16at(rb + at);
    // pass 1: sum rb[cs:plen] with the field zeroed (16-byte chunks, whole wave)
    const int rel0 = cs - (int)(((uintptr_t)rb + (uintptr_t)cs) & 15u);
    const uint8_t* a0 = rb + rel0;
    const int nch = plen > cs ? (plen - rel0 + 15) >> 4 : 0;
    uint64_t acc = 0;
    for (int c = lane; c < nch; c += 64) {
      const uint4 v = ld16(a0 + 16 * c);
      const int x0 = rel0 + 16 * c;
      uint4 w = v;
      const int j0 = at - x0, j1 = at + 1 - x0;
      if (j0 >= 0 && j0 < 16) w = set_chunk_byte(w, j0, 0);
      if (j1 >= 0 && j1 < 16) w = set_chunk_byte(w, j1, 0);
      acc += chunk_sum(w, x0, cs, plen);
    }
    uint32_t s = fold32_16(wave_sum_u32(fold64_16(acc)));
    if ((((uintptr_t)rb + (uintptr_t)cs) & 1u) == 0) s = bswap16(s);
    const uint32_t t = fold32_16(s + initial);
    pf = at;
    pv = (~t) & 0xFFFFu;
  }
  const int dalign = (int)((uintptr_t)dst & 15);
  uint8_t* dbase = dst - dalign;
  const int nk = (plen + dalign + 15) >> 4;
  uint64_t dummy = 0;
  stream_copy<false>(rb, rb, rb + plen, dbase, dalign, 0, nk, plen, plen, pf, pv, lane, dummy);
}

}  // namespace

// ---------------------------------------------------------------------------
// Row-per-segment split: one 16-lane DPP row per OUTPUT segment, 16 rows per
// 256-thread block; grid = (job, group of 16 segments).  Per row:
//   * payload windows are dword-aligned 16-byte raw buffer loads over the
//     job's bytes (range-checked: nothing past the job is touched, no page
//     test), U per lane in flight;
//   * destination chunk k = r + 16u is assembled from window k and the next
//     lane's first dword (DPP row_ror:15) with a per-row byte shift, summed
//     (v_dot2) and stored as one dwordx4 (byte-exact pieces at the edges);
//   * the checksums come from the row sum plus job constants plus the
//     rewritten field values (gro.go:1419-1465), and the header bytes are
//     stored last with both checksums filled in.
// Each output byte is written exactly once, each input byte read once.

__device__ __forceinline__ uint32_t add4(uint32_t acc, const uint4& v) {
  return add_halves(add_halves(add_halves(add_halves(acc, v.x), v.y), v.z), v.w);
}

// acc + the chunk's bytes selected by the 16-bit byte mask m16 (rot: the
// range pairs bytes with the opposite parity of acc's range, wgcs_common.h).
__device__ __forceinline__ uint32_t add4_masked(uint32_t acc, const uint4& v, uint32_t m16, bool rot) {
  uint32_t y0 = v.x & expand_nibble(m16 & 0xFu), y1 = v.y & expand_nibble((m16 >> 4) & 0xFu);
  uint32_t y2 = v.z & expand_nibble((m16 >> 8) & 0xFu), y3 = v.w & expand_nibble((m16 >> 12) & 0xFu);
  if (rot) {
    y0 = rotl8(y0);
    y1 = rotl8(y1);
    y2 = rotl8(y2);
    y3 = rotl8(y3);
  }
  return add_halves(add_halves(add_halves(add_halves(acc, y0), y1), y2), y3);
}

// Per-byte select: bytes whose bit is set in m16 from a, the rest from b.
__device__ __forceinline__ uint4 select_bytes(const uint4& a, const uint4& b, uint32_t m16) {
  const uint32_t m0 = expand_nibble(m16 & 0xF), m1 = expand_nibble((m16 >> 4) & 0xF);
  const uint32_t m2 = expand_nibble((m16 >> 8) & 0xF), m3 = expand_nibble((m16 >> 12) & 0xF);
  return make_uint4((a.x & m0) | (b.x & ~m0), (a.y & m1) | (b.y & ~m1), (a.z & m2) | (b.z & ~m2),
                    (a.w & m3) | (b.w & ~m3));
}

// Write byte value b at packet position pos into the chunk at position x0,
// if pos < lim (header bytes only; the payload copy wins above hdrLen).
__device__ __forceinline__ void put_byte(uint4& v, int x0, int pos, uint32_t b, int lim) {
  const int t = pos - x0;
  if (pos < lim && t >= 0 && t < 16) v = set_chunk_byte(v, t, b);
}
__device__ __forceinline__ void put_be16(uint4& v, int x0, int pos, uint32_t val, int lim) {
  put_byte(v, x0, pos, val >> 8, lim);
  put_byte(v, x0, pos + 1, val, lim);
}

// Job-uniform header sums for the common case ("fast" header): every
// per-segment header write lands inside hdrLen at a position disjoint from the
// L4 checksum field, so the per-segment IPv4 and L4 header sums are a job
// constant plus the rewritten field values (no per-segment byte sums).
struct HdrFast {
  bool fast;
  uint32_t ip_base;   // BE words of readBuf[0:csumStart) with [2:6) and [10:12) zero (IPv4)
  uint32_t l4_base;   // BE words of readBuf[csumStart:hdrLen) pairing from csumStart, csum field and
                      // seq / UDP-length zero, FIN|PSH cleared
  uint32_t addr;      // BE words of the pseudo-header addresses
  uint32_t flags;     // readBuf[csumStart + 13] (TCP flags byte)
};

// The fast header path's geometry condition: every per-segment header write
// lands inside hdrLen, disjoint from the L4 checksum field, which lies in the
// L4 header (so the raw readBuf header bytes equal the zeroed ones outside it).
__device__ __forceinline__ bool fast_header(int cs, int hl, int ca, bool tcp) {
  const int vlo = cs + 4, vhi = tcp ? cs + 8 : cs + 6;  // per-segment L4 field bytes
  return (tcp ? cs + 14 <= hl : vhi <= hl) && (ca + 2 <= vlo || ca >= vhi) && ca >= cs &&
         (!tcp || (ca != cs + 13 && ca + 1 != cs + 13));
}

__device__ __forceinline__ HdrFast header_fast(const HdrBytes& hb, const Job& j, int lane) {
  HdrFast h;
  const int cs = j.cs, hl = j.hdr_len, ca = (j.cs + j.co) & 0xFFFF;
  const bool v4 = j.ipv == 4, tcp = j.type != GSO_UDP_L4;
  const int vlo = cs + 4, vhi = tcp ? cs + 8 : cs + 6;  // per-segment L4 field bytes
  h.fast = fast_header(cs, hl, ca, tcp);
  const int a_lo = v4 ? 12 : 8, a_hi = v4 ? 20 : 40;
  uint32_t ip = 0, l4 = 0, ad = 0;
  const uint32_t regs[4] = {hb.r0, hb.r1, hb.r2, hb.r3};
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int x = lane + 64 * m - 10;  // readBuf position of this lane's byte
    const uint32_t b = regs[m];
    if (x < 0 || x >= hl) continue;
    const uint32_t hi8 = b << 8;
    if (v4 && x < cs && (x < 2 || x >= 6) && x != 10 && x != 11) ip += (x & 1) ? b : hi8;
    if (x >= cs && x != ca && x != ca + 1 && (x < vlo || x >= vhi)) {
      const uint32_t bb = (tcp && x == cs + 13) ? (b & ~0x09u) : b;
      l4 += ((x - cs) & 1) ? bb : (bb << 8);
    }
    if (x >= a_lo && x < a_hi) ad += (x & 1) ? b : hi8;
  }
  h.ip_base = wave_sum_u32(ip);
  h.l4_base = wave_sum_u32(l4);
  h.addr = wave_sum_u32(ad);
  h.flags = tcp ? hb(10 + cs + 13) : 0u;
  return h;
}

// Header chunks in packet coordinates (lane r: bytes [16r, 16r + 16)):
// write byte / big-endian u16 `val` at the wave-uniform position pos.
__device__ __forceinline__ void put_u(uint4& P, int r, int pos, uint32_t val, uint32_t nbytes_mask) {
  const int sh = 8 * (pos & 3);
  const uint32_t m = r == (pos >> 4) ? (nbytes_mask << sh) : 0u;
  const uint32_t v = val << sh;
  switch ((pos >> 2) & 3) {
    case 0: P.x = (P.x & ~m) | (v & m); break;
    case 1: P.y = (P.y & ~m) | (v & m); break;
    case 2: P.z = (P.z & ~m) | (v & m); break;
    default: P.w = (P.w & ~m) | (v & m); break;
  }
}
__device__ __forceinline__ void put_be16_u(uint4& P, int r, int pos, uint32_t val) {
  if ((pos & 1) == 0) {  // both bytes in one dword (pos & 3 is 0 or 2)
    put_u(P, r, pos, bswap16(val & 0xFFFFu), 0xFFFFu);
  } else {
    put_u(P, r, pos, (val >> 8) & 0xFFu, 0xFFu);
    put_u(P, r, pos + 1, val & 0xFFu, 0xFFu);
  }
}

// Job-level values decoded once per block by the decoder wave, published
// through LDS (read by the rows before their header phase).
struct JobInfo {
  int32_t status, count, nseg;
  uint32_t shape;  // type | ipv << 8 | gen << 16 | fast << 24
  int32_t hdr_len, gso, cs, co, plen, flags;
  uint32_t id0, seq0, ip_base, l4_base, addr, tflags;
};

__device__ __forceinline__ int ufl(int x) { return __builtin_amdgcn_readfirstlane(x); }

// Buffer resource over one job's bytes [vb, vb + jlen): every dword holding a
// job byte passes the range check (num_records jlen + 3), loads past it
// return zeros instead of touching memory past the arena.  Built from
// wave-uniform values only (one descriptor per wave, no waterfall).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t job_rsrc(const uint8_t* vb, uint32_t jlen) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(vb), (short)0, (int)(jlen + 3u), 0x00020000);
}
template <bool NT>
__device__ __forceinline__ uint4 bld16(__amdgpu_buffer_rsrc_t rs, int off) {
  const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, WGCS_LD_AUX(NT));
  return make_uint4(t[0], t[1], t[2], t[3]);
}
// One batch of dword-aligned windows: lane r loads windows k0 + r + 16u at job
// offset aoff + 16 * window (lane 15 also the first dword of the window after
// the batch, E), each only when it overlaps the job bytes [lo, hi).
// A window that is not needed gets an offset past the resource's range instead
// of a branch around its load: the range check returns zeros and touches no
// memory, so the loads are issued unconditionally (no exec-mask branches, and
// the compiler can wait on them one by one with vmcnt(n)).
constexpr int kOobOffset = 0x7FFFFFF0;
template <int U, bool NT>
__device__ __forceinline__ void load_windows(__amdgpu_buffer_rsrc_t rs, int aoff, int k0, int r, int lo, int hi,
                                             uint4 (&A)[U], uint32_t& E) {
  const int o0 = aoff + 16 * (k0 + r);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int o = o0 + 256 * u;
    A[u] = bld16<NT>(rs, (o < hi && o + 16 > lo) ? o : kOobOffset);
  }
  const int oe = aoff + 16 * (k0 + 16 * U);
  E = __builtin_amdgcn_raw_buffer_load_b32(rs, (r == 15 && oe < hi && oe + 4 > lo) ? oe : kOobOffset, 0,
                                           WGCS_LD_AUX(NT));
}

// Wave-uniform: no lane of the wave has `pred` set (a scalar compare, no exec-mask branch).
__device__ __forceinline__ bool wave_none(bool pred) { return __builtin_amdgcn_ballot_w64(pred) == 0; }

// A row's source geometry for segment i: the dword-aligned window of its
// destination chunk 0 (job-relative offset aoff, byte shift sb), the job
// bytes [lo, hi) of its payload, its chunk count nk and packet length.
struct RowSrc {
  int aoff, sb, lo, hi, nk, pkt_len;
};
__device__ __forceinline__ RowSrc row_src(const uint8_t* rb, int i, int gso, int hdr_len, int plen, int dalign) {
  RowSrc g;
  const int seg_start = hdr_len + i * gso;
  const int seg_end = min(plen, seg_start + gso);
  g.pkt_len = hdr_len + (seg_end - seg_start);
  g.nk = (g.pkt_len + dalign + 15) >> 4;
  const uint8_t* w0 = rb + (int64_t)i * gso - dalign;  // source of destination chunk 0 (payload positions)
  g.sb = (int)((uintptr_t)w0 & 3u);
  g.aoff = (int)(w0 - g.sb - (rb - 10));               // its dword-aligned window, job-relative
  g.lo = 10 + seg_start;
  g.hi = 10 + seg_end;
  return g;
}

// One batch of a row's payload stream: destination chunk k = bytes [sb, sb +
// 16) of the dword-aligned source window k and the first dword of window k + 1
// (next lane, DPP row_ror).  Sums the L4 bytes [hdrLen, pktLen) from the same
// registers (v_dot2) and stores the payload bytes of every chunk (those of a
// chunk shared with the header as byte-exact pieces; the header phase stores
// the chunk's header bytes).
template <int U>
__device__ __forceinline__ void consume_batch(const uint4 (&A)[U], uint32_t E, int k0, const RowSrc& g, int hdr_len,
                                              int dalign, uint8_t* dbase, int r, uint32_t& acc) {
  const int pkt_len = g.pkt_len, nk = g.nk, sb = g.sb;
  uint32_t Rc = row_next(A[0].x);  // lane 15: lane 0's next-u dword
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k = k0 + r + 16 * u;
    const uint32_t Rx = u + 1 < U ? row_next(A[u + 1 < U ? u + 1 : u].x) : E;
    const uint32_t nx = r == 15 ? Rx : Rc;
    Rc = Rx;
    const int x0 = 16 * k - dalign;
    const uint4 v = make_uint4(__builtin_amdgcn_alignbyte(A[u].y, A[u].x, sb),
                               __builtin_amdgcn_alignbyte(A[u].z, A[u].y, sb),
                               __builtin_amdgcn_alignbyte(A[u].w, A[u].z, sb),
                               __builtin_amdgcn_alignbyte(nx, A[u].w, sb));
    if (wave_none(x0 < hdr_len || x0 + 16 > pkt_len)) {
      // every chunk of this step in every row of the wave is whole payload
      // (the bulk of a segment): unmasked sum and a full store, no branches
      acc = add4(acc, v);
      int ko = 16 * k;
      asm volatile("" : "+v"(ko));
      st128(dbase + ko, v);
    } else if (k < nk) {
      if (x0 >= hdr_len && x0 + 16 <= pkt_len) acc = add4(acc, v);
      else acc = add4_masked(acc, v, byte_bits16(hdr_len - x0, pkt_len - x0), false);
      // the chunk's address formed here, not hoisted for all U chunks up front
      // (six 64-bit addresses held across the stream cost an occupancy step)
      int ko = 16 * k;
      asm volatile("" : "+v"(ko));
      store_chunk(dbase + ko, v, x0 - hdr_len, pkt_len - hdr_len);  // bytes [hdrLen, pktLen)
    }
  }
}

// Where gso_lds_kernel's row writes: its segment's destination chunks at
// dbase (= out + obase + dro), and, when `wt`, a buffer resource over the
// job's output region (out + obase) for write-through full-chunk stores
// (`sc1`: the line leaves L2 at once instead of staying dirty until the
// end-of-kernel writeback).  The stores go through the buffer intrinsic, not
// inline asm: the compiler then sees them (wait counts, and the hazard of a
// VALU overwriting a 16-byte store's data registers right behind it).
struct RowOut {
  uint4 keep;  // this lane's header-shared chunk's payload bytes (consume_batch_img)
  __amdgpu_buffer_rsrc_t rs;
  int dro;  // dbase - (out + obase), when wt
  bool wt;  // block-uniform: every offset of the job's output region fits the resource
};
__device__ __forceinline__ void store16_row(const RowOut& o, uint8_t* dbase, int ko, const uint4& v) {
  if (o.wt) {
    typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
    const u32x4v vv = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(vv, o.rs, o.dro + ko, 0, 16);  // sc1
  } else {
    st128(dbase + ko, v);
  }
}
// store_chunk with its full-chunk case through store16_row.
__device__ __forceinline__ void store_chunk_row(const RowOut& o, uint8_t* dbase, int ko, const uint4& v, int x0,
                                                int pkt_len) {
  if (x0 >= 0 && x0 + 16 <= pkt_len) store16_row(o, dbase, ko, v);
  else store_chunk(dbase + ko, v, x0, pkt_len);
}

// consume_batch for gso_lds_kernel.  A chunk the row shares with the header
// (x0 < hdrLen: only step 0 of the first batch, hdrLen + dalign <= 255) is not
// stored here: its payload bytes are kept in `keep` (lane r: chunk r) and
// finish_row stores them with the header bytes as one 16-byte store.  Whole
// payload chunks are stored write-through, the packet's last partial chunk as
// pieces.  The sums are consume_batch's.
template <int U>
__device__ __forceinline__ void consume_batch_img(const uint4 (&A)[U], uint32_t E, int k0, const RowSrc& g,
                                                  int hdr_len, int dalign, uint8_t* dbase, int r, uint32_t& acc,
                                                  RowOut& ro) {
  const int pkt_len = g.pkt_len, sb = g.sb;
  uint32_t Rc = row_next(A[0].x);  // lane 15: lane 0's next-u dword
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k = k0 + r + 16 * u;
    const uint32_t Rx = u + 1 < U ? row_next(A[u + 1 < U ? u + 1 : u].x) : E;
    const uint32_t nx = r == 15 ? Rx : Rc;
    Rc = Rx;
    const int x0 = 16 * k - dalign;
    const uint4 v = make_uint4(__builtin_amdgcn_alignbyte(A[u].y, A[u].x, sb),
                               __builtin_amdgcn_alignbyte(A[u].z, A[u].y, sb),
                               __builtin_amdgcn_alignbyte(A[u].w, A[u].z, sb),
                               __builtin_amdgcn_alignbyte(nx, A[u].w, sb));
    int ko = 16 * k;
    asm volatile("" : "+v"(ko));
    if (wave_none(x0 < hdr_len || x0 + 16 > pkt_len)) {  // every chunk of the step whole payload
      acc = add4(acc, v);
      store16_row(ro, dbase, ko, v);
    } else {
      acc = add4_masked(acc, v, byte_bits16(hdr_len - x0, pkt_len - x0), false);
      if (u == 0) ro.keep = k0 == 0 ? v : ro.keep;
      if (x0 >= hdr_len && x0 < pkt_len) {
        if (x0 + 16 <= pkt_len) store16_row(ro, dbase, ko, v);
        else store_lo(dbase + ko, v, pkt_len - x0);  // the packet's last bytes
      }
    }
  }
}

// One row's whole payload stream, batch by batch.
template <int U, bool NT>
__device__ __forceinline__ void stream_row(const uint8_t* rb, int i, int gso, int hdr_len, int plen, int dalign,
                                           uint8_t* dbase, int r, uint32_t& acc, __amdgpu_buffer_rsrc_t rs) {
  const RowSrc g = row_src(rb, i, gso, hdr_len, plen, dalign);
  acc = 0;
  for (int k0 = 0; k0 < g.nk; k0 += 16 * U) {
    uint4 A[U];
    uint32_t E;
    load_windows<U, NT>(rs, g.aoff, k0, r, g.lo, g.hi, A, E);
    consume_batch<U>(A, E, k0, g, hdr_len, dalign, dbase, r, acc);
  }
}

// Byte `pos` (wave-uniform, < 16 * 16) of the header chunks in packet
// coordinates (lane r of each row holds readBuf[16r, 16r + 16)), from the
// wave's first row.
__device__ __forceinline__ uint32_t qdw(const uint4& Q, int dw) {  // dword dw (wave-uniform, < 64)
  return (uint32_t)__builtin_amdgcn_readlane((int)dword_at(Q, dw & 3), dw >> 2);
}
__device__ __forceinline__ uint32_t qbyte(const uint4& Q, int pos) { return (qdw(Q, pos >> 2) >> (8 * (pos & 3))) & 0xFFu; }
// Bytes [pos, pos + 4) as a little-endian u32 (two readlanes).
__device__ __forceinline__ uint32_t qle32(const uint4& Q, int pos) {
  const uint64_t w = ((uint64_t)qdw(Q, (pos >> 2) + 1) << 32) | qdw(Q, pos >> 2);
  return (uint32_t)(w >> (8 * (pos & 3)));
}
// The decoded path's decoder (wave 0 of the block): handleVirtioRead's /
// gsoSplit's checks and geometry (decode_job) and the job-constant header
// sums (header_fast), published in `ji`; count / status of the job.  Kept out
// of line: the rare path's registers do not count against the clean path's.
__device__ __noinline__ void decode_publish(const uint8_t* vb, uint32_t jlen, uint32_t jflags, uint32_t room,
                                            uint32_t max_segs, int lane, JobInfo* jip, bool first_block,
                                            int32_t* count_j, int32_t* status_j) {
  JobInfo& ji = *jip;
  __builtin_amdgcn_s_setprio(3);
  HdrBytes hb;
  hb.load(vb, (int)min(jlen, 256u), lane);
  const Job jd = decode_job(hb, jlen, jflags, room, max_segs);
  const bool ok = jd.status == 0 || jd.status == WGCS_ERR_TOO_MANY_SEGMENTS;
  uint32_t fst = 0, i0 = 0, q0 = 0;
  HdrFast hf = {};
  if (ok && jd.nseg > 0 && jd.type != GSO_NONE && !jd.gen) {
    hf = header_fast(hb, jd, lane);
    // readBuf bytes after gsoSplit zeroed the L4 checksum field (gro.go:1393;
    // the IPv4 checksum bytes 10-11 are neither id nor seq here: cs >= 20)
    const int ca = (jd.cs + jd.co) & 0xFFFF;
    auto zb = [&](int x) { return (x == ca || x == ca + 1) ? 0u : hb(10 + x); };
    const int sq = jd.cs + 4;
    i0 = jd.ipv == 4 ? (zb(4) << 8) | zb(5) : 0u;
    q0 = jd.type != GSO_UDP_L4 ? (zb(sq) << 24) | (zb(sq + 1) << 16) | (zb(sq + 2) << 8) | zb(sq + 3) : 0u;
    fst = hf.fast ? 1u : 0u;
  }
  if (lane == 0) {
    ji.status = jd.status;
    ji.count = ok ? jd.count : 0;
    ji.nseg = ok ? jd.nseg : 0;
    ji.shape = (uint32_t)(jd.type & 0xFF) | ((uint32_t)(jd.ipv & 0xFF) << 8) |
               ((uint32_t)(jd.gen ? 1 : 0) << 16) | (fst << 24);
    ji.hdr_len = jd.hdr_len;
    ji.gso = jd.gso;
    ji.cs = jd.cs;
    ji.co = jd.co;
    ji.plen = jd.plen;
    ji.flags = jd.flags;
    ji.id0 = i0;
    ji.seq0 = q0;
    ji.ip_base = fold32_16(hf.ip_base);
    ji.l4_base = fold32_16(hf.l4_base) + fold32_16(hf.addr);
    ji.tflags = hf.flags;
    if (first_block) {
      *count_j = ok ? jd.count : 0;
      *status_j = jd.status;
    }
  }
  __builtin_amdgcn_s_setprio(0);
}

// Row-per-segment split.  Block = 4 waves = 16 rows = 16 consecutive output
// segments of one job; grid = (job, segment group).
//
// Clean jobs (the common case) need no decode step and no barrier.  Every
// wave reads the virtio header (one wave-uniform load) and derives the split
// geometry; when that geometry takes the row-streaming path and its first
// segment fits the caller's room, handleVirtioRead's and gsoSplit's checks
// (tun/tun.go:557-631, gro.go:1387-1410) can fail only through the TCP data
// offset, which the wave reads from the header chunks it loads anyway
// (hdrLen = csumStart + dataOffset, tun.go:601-614).  Such a job's status is
// 0 or ErrTooManySegments from the segment count alone, and each row
// computes the header sums it needs from its own header chunks.  The row
// streams its payload (loads issued right after the virtio header arrives),
// then rewrites and stores its header chunks.
//
// Every other job (GSO_NONE, errors, unusual geometry) takes the decoded
// path: wave 0 runs decode_job and the job-constant sums and publishes them
// through LDS; after the barrier each row follows that verdict (nothing on an
// error, the byte-granular general path, or the stream with the decoded
// geometry and the general header path).
// The segment's header chunk and checksums, given the row's payload sum
// `acc` and the job-constant header values: on the fast layout the header
// chunk in packet coordinates (Q) rewritten field by field and shifted to the
// destination phase; otherwise a byte-exact replay of the reference's write
// order on the chunk in destination coordinates.  Stores the header bytes
// [0, hdrLen) of the segment (the stream stored the rest) and its size.
__device__ __forceinline__ void finish_row(bool fast, const uint4 Q, int type, int ipv, int hdr_len, int gso, int cs,
                                           int co, int plen, int i, int r, int dalign, const uint8_t* dst,
                                           uint8_t* dbase, uint32_t acc, uint32_t ip_base, uint32_t l4_base,
                                           uint32_t tflags, uint32_t id0, uint32_t seq0, int32_t* size_out,
                                           const RowOut* ro = nullptr) {
  const uint4 z = make_uint4(0, 0, 0, 0);
  // ---- segment geometry (row-uniform)
  const bool v4 = ipv == 4, tcp = type != GSO_UDP_L4;
  const int csum_at = (cs + co) & 0xFFFF;
  const int seg_start = hdr_len + i * gso;
  const int seg_end = min(plen, seg_start + gso);
  const int seg_len = seg_end - seg_start;
  const int pkt_len = hdr_len + seg_len;
  const bool last = seg_end == plen;
  const int nk = (pkt_len + dalign + 15) >> 4;
  const int hk = min((hdr_len + dalign + 15) >> 4, nk);
  const uint32_t id = i > 0 ? ((id0 + 1) & 0xFFFFu) : id0;  // quirk: id0 + 1 for every i >= 1 (:1426-1431)
  const uint32_t seq = seq0 + (uint32_t)(uint16_t)((uint16_t)gso * (uint16_t)i);  // uint16 product (:1445)
  const uint32_t ulen = (uint32_t)(uint16_t)(seg_len + (hdr_len - cs));           // UDP length (:1462-1465)
  const uint32_t tlen = (uint32_t)(uint16_t)(hdr_len - cs + seg_len);             // transportLen (:1469-1471)
  const uint32_t proto = tcp ? 6u : 17u;
  const int x0h = 16 * r - dalign;

  if (fast) {
    // ---- sums: payload (row reduction) + job constants + rewritten fields
    uint32_t t_pay = fold32_16(row16_sum_u32(acc));
    if ((((uintptr_t)dst + (uintptr_t)cs) & 1u) == 0) t_pay = bswap16(t_pay);  // pairing from csumStart
    const uint32_t var = tcp ? (seq >> 16) + (seq & 0xFFFFu) + (last ? (tflags & 0x09u) : 0u) : ulen;
    const uint32_t l4c = (~fold32_16(t_pay + l4_base + var + proto + tlen)) & 0xFFFFu;
    // ---- header chunk in packet coordinates, rewritten (gro.go:1418-1465, :1486-1490)
    uint4 P = Q;
    if (v4) {
      const uint32_t ipc = (~fold32_16(ip_base + (uint32_t)pkt_len + id)) & 0xFFFFu;
      put_be16_u(P, r, 2, (uint32_t)pkt_len);  // total length (:1433)
      put_be16_u(P, r, 4, id);                 // identification (:1426-1431)
      put_be16_u(P, r, 10, ipc);               // header checksum (:1434-1436)
    } else {
      put_be16_u(P, r, 4, (uint32_t)(pkt_len - cs));  // payload length (:1439)
    }
    if (tcp) {
      put_be16_u(P, r, cs + 4, seq >> 16);  // sequence number (:1445-1446)
      put_be16_u(P, r, cs + 6, seq);
      put_u(P, r, cs + 13, last ? tflags : (tflags & ~0x09u), 0xFFu);  // FIN|PSH on the last only (:1447-1459)
    } else {
      put_be16_u(P, r, cs + 4, ulen);
    }
    put_be16_u(P, r, csum_at, l4c);  // L4 checksum (:1486-1490)
    // ---- to the destination phase (previous chunk of the row: DPP row_shr:1),
    // merged with the payload bytes, stored
    const uint4 Pp = row_prev4(P);
    const uint4 D = dalign ? funnel_v(Pp, P, 16 - dalign) : P;
    if (ro) {
      // gso_lds_kernel: the stream kept these chunks' payload bytes
      // (consume_batch_img); header and payload go out as one store
      if (r < hk)
        store_chunk_row(*ro, dbase, 16 * r, select_bytes(D, ro->keep, byte_bits16(-x0h, hdr_len - x0h)), x0h, pkt_len);
    } else if (r < hk) {
      store_chunk(dbase + 16 * r, D, x0h, hdr_len);  // header bytes [0, hdrLen)
    }
  } else {
    // ---- general header path (unusual csum offsets): byte-exact replay of
    // the reference's write order on the chunk (destination coordinates)
    const int a_lo = v4 ? 12 : 8, a_hi = v4 ? 20 : 40;
    uint32_t acc_ip = 0;
    uint4 hv = z;
    if (r < hk) {
      hv = Q;
      // readBuf's zeroed fields (gro.go:1388,:1393), then the per-segment header writes in order
      if (v4) put_be16(hv, x0h, 10, 0, hdr_len);
      put_be16(hv, x0h, csum_at, 0, hdr_len);
      if (v4) {
        put_be16(hv, x0h, 4, id, hdr_len);
        put_be16(hv, x0h, 2, pkt_len, hdr_len);
      } else {
        put_be16(hv, x0h, 4, pkt_len - cs, hdr_len);
      }
      if (tcp) {
        put_be16(hv, x0h, cs + 4, seq >> 16, hdr_len);
        put_be16(hv, x0h, cs + 6, seq, hdr_len);
        const int fl = cs + 13 - x0h;
        if (!last && cs + 13 < hdr_len && fl >= 0 && fl < 16) hv = set_chunk_byte(hv, fl, chunk_byte(hv, fl) & ~0x09u);
      } else {
        put_be16(hv, x0h, cs + 4, ulen, hdr_len);
      }
      if (v4) acc_ip = add4_masked(0u, hv, byte_bits16(-x0h, cs - x0h), false);
      acc = add4_masked(acc, hv, byte_bits16(cs - x0h, hdr_len - x0h), false);
      acc = add4_masked(acc, hv, byte_bits16(a_lo - x0h, a_hi - x0h), (cs & 1) != 0);  // pseudo-header addresses
    }
    uint32_t t_ip = fold32_16(row16_sum_u32(acc_ip));
    if ((((uintptr_t)dst) & 1u) == 0) t_ip = bswap16(t_ip);
    uint32_t t_l4 = fold32_16(row16_sum_u32(acc));
    if ((((uintptr_t)dst + (uintptr_t)cs) & 1u) == 0) t_l4 = bswap16(t_l4);
    const uint32_t l4c = (~fold32_16(t_l4 + proto + tlen)) & 0xFFFFu;
    if (r < hk) {
      if (v4) put_be16(hv, x0h, 10, (~t_ip) & 0xFFFFu, hdr_len);
      put_be16(hv, x0h, csum_at, l4c, hdr_len);
      store_chunk(dbase + 16 * r, hv, x0h, hdr_len);  // header bytes [0, hdrLen)
    }
  }
  if (r == 0) *size_out = pkt_len;
}

// Every job that is not clean (GSO_NONE, errors, unusual geometry): wave 0
// runs the full validation (decode_publish) and publishes its verdict through
// LDS, the rows follow it.  Out of line, so that its registers do not count
// against the clean path's occupancy (it spills, if at all, only here).
// Returns the job's live segment count from the published verdict (0 for an
// error, GSO_NONE or no segment): block-uniform, so the caller's group loop
// stops after the last group that holds a segment.
template <int U, bool NT>
__device__ __noinline__ int decoded_rows(const uint8_t* vb_a, uint32_t jlen_a, uint32_t jflags_a, uint32_t room,
                                          uint32_t max_segs, int i, bool first_block, int32_t* count_j,
                                          int32_t* status_j, uint8_t* out0, uint8_t* dst, int32_t* sizes_j,
                                          uint32_t tails_a) {
  __shared__ JobInfo ji;
  const uint4 z = make_uint4(0, 0, 0, 0);
  const int lane = threadIdx.x & 63;
  const int r = lane & 15;
  const int wv = threadIdx.x >> 6;
  // the job's values are wave-uniform (arguments arrive in VGPRs)
  const uint64_t vbu = ((uint64_t)(uint32_t)ufl((int)(uint32_t)(uintptr_t)vb_a)) |
                       ((uint64_t)(uint32_t)ufl((int)(uint32_t)((uintptr_t)vb_a >> 32)) << 32);
  const uint8_t* vb = reinterpret_cast<const uint8_t*>(vbu);
  const uint32_t jlen = (uint32_t)ufl((int)jlen_a), jflags = (uint32_t)ufl((int)jflags_a);
  const uint8_t* rb = vb + 10;
  const int dalign = (int)((uintptr_t)dst & 15u);
  uint8_t* dbase = dst - dalign;
  const int hph = (int)((uintptr_t)rb & 15u);
  const uint8_t* hab = rb - hph + 16 * r;
  // ---- decoded path: wave 0 decodes, every wave follows its verdict
  if (wv == 0) decode_publish(vb, jlen, jflags, room, max_segs, lane, &ji, first_block, count_j, status_j);
  lds_barrier();  // the decoder's verdict
  const int st = ufl(ji.status);
  const int nseg = ufl(ji.nseg);
  const uint32_t shape = (uint32_t)ufl((int)ji.shape);
  const int type = (int)(shape & 0xFFu);
  if ((st != 0 && st != WGCS_ERR_TOO_MANY_SEGMENTS) || nseg == 0) return 0;
  const int plen = ufl(ji.plen);
  if (type == GSO_NONE) {  // one packet into bufs[0], by wave 0 of the job's first block
    if (first_block && wv == 0) {
      Job jn = {};
      jn.flags = ufl(ji.flags);
      jn.cs = ufl(ji.cs);
      jn.co = ufl(ji.co);
      jn.plen = plen;
      none_segment(rb, jn, out0, lane);
      if (lane == 0) *sizes_j = plen;
    }
    return 0;
  }
  if (i >= nseg) return nseg;  // whole rows retire; DPP below stays inside live rows
  const int ipv = (int)((shape >> 8) & 0xFFu);
  const bool fast = (shape >> 24) != 0;
  const int hdr_len = ufl(ji.hdr_len);
  const int gso = ufl(ji.gso);
  const int cs = ufl(ji.cs);
  const int co = ufl(ji.co);
  if ((shape >> 16) & 0xFFu) {  // block-uniform
    gso_general_row(rb, plen, type, ipv, hdr_len, gso, cs, co, i, dst, r, sizes_j + i, ufl((int)tails_a) != 0);
    return nseg;
  }
  uint32_t acc = 0;
  stream_row<U, NT>(rb, i, gso, hdr_len, plen, dalign, dbase, r, acc, job_rsrc(vb, jlen));
  // header chunks: packet coordinates on the fast layout, destination
  // coordinates for the general header path
  const uint8_t* hend = rb + hdr_len;
  const int hphd = (int)((uintptr_t)(rb - dalign) & 15u);
  const uint8_t* hb2 = fast ? hab : rb - dalign - hphd + 16 * r;
  uint4 H0 = z, H1 = z;
  if (hb2 < hend && hb2 + 16 > rb) H0 = ld16(hb2);
  if (hb2 + 16 < hend && hb2 + 32 > rb) H1 = ld16(hb2 + 16);
  const uint4 Q = fast ? funnel(H0, H1, hph) : funnel_v(H0, H1, hphd);
  const uint32_t ip_base = (uint32_t)ufl((int)ji.ip_base);
  const uint32_t l4_base = (uint32_t)ufl((int)ji.l4_base);
  const uint32_t tflags = (uint32_t)ufl((int)ji.tflags);
  const uint32_t id0 = (uint32_t)ufl((int)ji.id0);
  const uint32_t seq0 = (uint32_t)ufl((int)ji.seq0);
  finish_row(fast, Q, type, ipv, hdr_len, gso, cs, co, plen, i, r, dalign, dst, dbase, acc, ip_base, l4_base, tflags,
             id0, seq0, sizes_j + i);
  return nseg;
}

// Build-time tunables (defaults measured on cfg4):
// payload windows per lane in flight, and the occupancy the kernel is compiled
// for.  The out-of-line decoded path would otherwise set the register count
// (151 VGPRs, 3 waves per SIMD); at 5 waves (<= 96 VGPRs) the clean path runs
// without spills and the decoded path spills only inside its own call.
#ifndef WGCS_GSO_U
#define WGCS_GSO_U 6
#endif
#ifndef WGCS_GSO_WAVES
#define WGCS_GSO_WAVES 5
#endif
#ifndef WGCS_GSO_GROUPS
#define WGCS_GSO_GROUPS 3  // blocks per job (grid y); each takes every WGCS_GSO_GROUPS-th segment group
#endif
// One (job, segment-group set) of gso_rows_kernel: block `by` of `gy` blocks
// per job takes the job's segment groups by, by + gy, ...  The descriptor and
// output position come by value (the resident ring kernel passes a request's,
// gso_rows_kernel its grid's); `has_pos`: use pos, else fixed slots.
// 16 bytes at a 4-byte aligned generic pointer that points into LDS (ds reads)
__device__ __forceinline__ uint4 lds16_a4(const uint8_t* p) {
  typedef __attribute__((address_space(3))) const uint32_t l32;
  const l32* q = (const l32*)(const __attribute__((address_space(3))) uint8_t*)p;
  return make_uint4(q[0], q[1], q[2], q[3]);
}

template <int U, bool NT, int ROWS = 16>
__device__ __forceinline__ void gso_rows_body(const uint8_t* arena, const wgcs_gso_job job, uint32_t jb, int by,
                                              int gy, uint32_t max_segs, uint8_t* out, uint32_t out_stride,
                                              bool has_pos, const GsoOutPos pos, uint32_t offset, uint32_t room,
                                              int32_t* sizes, int32_t* count, int32_t* status,
                                              const uint8_t* hlds = nullptr) {
  static_assert(ROWS % 4 == 0, "4 rows per wave");  // ROWS = 4 x the workgroup's waves
  const int lane = threadIdx.x & 63;
  const int r = lane & 15;
  const int wv = threadIdx.x >> 6;
  const uint8_t* vb = arena + job.off;
  const uint32_t jlen = job.len;
  const uint8_t* rb = vb + 10;
  const uint64_t slot0 = (uint64_t)jb * max_segs;  // sizes[] index of segment 0
  // segment i of this job at out + obase + i * opitch (+ offset): fixed slots,
  // or the caller's packed per-job layout (the stager's compact D2H region)
  uint64_t obase = slot0 * out_stride;
  uint32_t opitch = out_stride;
  uint32_t tails = 1;  // gsoSplit's header writes past a segment's end (GsoOutPos)
  if (has_pos) {
    obase = pos.base;
    opitch = pos.pitch;
    tails = pos.flags & kOutPosTails;
  }
  // ---- header chunks in packet coordinates (lane r of each row: the
  // dword-aligned 16-byte window r from the dword holding readBuf[0]; shifted
  // to readBuf[16r, 16r + 16) with the next lane's first dword below), issued
  // first: they need only the descriptor.  A raw buffer load over the job's
  // bytes: windows past the job read as zeros.  Lane 15's last bytes
  // (readBuf[253..255]) come from the wrong lane; every use of the chunks is
  // below hdrLen <= 240.
  const int hph = (int)((uintptr_t)rb & 3u);
  const uint8_t* hbase = rb - hph;
  const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(hbase), (short)0, (int)(jlen + 3u) - (int)(hbase - vb), 0x00020000);
  // (hlds: the resident ring's copy of vb[0, 272) in LDS, vb[k] at hlds[k],
  // same phase mod 16 as vb -- the header without a host-memory round trip)
  const uint4 H0 = hlds ? lds16_a4(hlds + (hbase - vb) + 16 * r) : bld16<false>(hrs, 16 * r);

  // ---- virtio header + the IP version byte: 16 bytes from the dword below
  // vb, one wave-uniform load (readable: jlen >= 14 and the arena contract)
  const bool raw = (job.flags & WGCS_GSO_JOB_RAW) != 0;
  const int plen_s = jlen > 10 ? (int)jlen - 10 : 0;
  uint32_t t1 = 0, hl = 0, g = 0, c = 0, o = 0, b0 = 0;
  if (jlen >= 14) {
    const int sh = (int)((uintptr_t)vb & 3u);
    // a range-checked vector load (zeros past the job), not a scalar one: the
    // resident ring kernel reads requests that change at the same address
    const uint4 w = hlds ? lds16_a4(hlds - sh)
                         : bld16<false>(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(vb - sh), (short)0,
                                                                          (int)(jlen + 3u + (uint32_t)sh), 0x00020000),
                                        0);
    const uint64_t lo = ((uint64_t)w.y << 32) | w.x, hi = ((uint64_t)w.w << 32) | w.z;
    // bytes [sh, sh + 11) of the 16: the virtio header and readBuf[0]
    const uint64_t v0 = sh ? (lo >> (8 * sh)) | (hi << (64 - 8 * sh)) : lo;  // vb[0..8)
    const uint64_t v1 = hi >> (8 * sh);                                      // vb[8..)
    t1 = (uint32_t)(v0 >> 8) & 0xFFu;
    hl = (uint32_t)(v0 >> 16) & 0xFFFFu;
    g = (uint32_t)(v0 >> 32) & 0xFFFFu;
    c = (uint32_t)(v0 >> 48) & 0xFFFFu;
    o = (uint32_t)v1 & 0xFFFFu;
    b0 = (uint32_t)(v1 >> 16) & 0xFFu;
  }
  const int type_s = raw ? ((t1 == GSO_TCPV4 || t1 == GSO_TCPV6) ? (int)t1 : GSO_UDP_L4) : (int)t1;
  const int ipv_s = raw ? ((job.flags & WGCS_GSO_JOB_V6) ? 6 : 4) : (int)(b0 >> 4);
  const bool tcp_s = type_s != GSO_UDP_L4;
  const bool ok_s = jlen >= 14 && g != 0 &&
                    (type_s == GSO_TCPV4 || type_s == GSO_TCPV6 || type_s == GSO_UDP_L4) &&
                    ((ipv_s == 4 && type_s != GSO_TCPV6) || (ipv_s == 6 && type_s != GSO_TCPV4));
  const int gso_s = (int)g, cs_s = (int)c, co_s = (int)o;
  const int hdr_s = (raw || tcp_s) ? (int)hl : ((cs_s + 8) & 0xFFFF);
  const int ca_s = (cs_s + co_s) & 0xFFFF;
  const int pkt0_s = hdr_s + min(gso_s, plen_s - hdr_s);  // segment 0, the largest
  const bool clean_s = ok_s && hdr_s < plen_s && cs_s >= (ipv_s == 4 ? 20 : 40) && ca_s + 2 <= hdr_s &&
                       hdr_s <= kMaxHdrLen && (raw || !tcp_s || (hdr_s - cs_s >= 20 && hdr_s - cs_s <= 60)) &&
                       fast_header(cs_s, hdr_s, ca_s, tcp_s) && (uint32_t)pkt0_s <= room;
  // Row i of a clean job holds a segment iff i < max_segs and hdrLen + i *
  // gsoSize < len(readBuf) (i < ceil((plen - hdrLen) / gsoSize)): a multiply,
  // no division, on the clean path.
  auto has_seg = [&](int i) { return i < (int)max_segs && hdr_s + (int64_t)i * gso_s < plen_s; };
  // Segment groups: this block takes groups blockIdx.y, + gridDim.y, ... of
  // the job's ceil(max_segs / 16).  The grid has only a few blocks per job
  // (callers size bufs for the largest read, conn.IdealBatchSize = 128 slots,
  // so most groups of a 64-KiB read are empty): groups past the job's last
  // segment under every verdict cost no dispatch and are never entered.
  // hdrLen >= csumStart + 20 (TCP, tun.go:608-613) or = csumStart + 8 (UDP) or
  // the virtio value (raw jobs) bounds the segment count from above.  Group 0
  // always runs: it writes count / status and the GSO_NONE packet.
  // Groups that may hold a segment: gbound = max(1, min(ngroups, ceil(nbound /
  // 16))) with nbound = ceil((plen - hmin) / gsoSize); group y < gbound iff y
  // == 0 or (y < ngroups and 16 y gsoSize < plen - hmin).
  const int ngroups = (int)((max_segs + ROWS - 1) / ROWS);
  const int hmin = raw ? (int)hl : (tcp_s ? cs_s + 20 : cs_s + 8);
  const bool split_type = jlen >= 14 && ok_s && cs_s + 60 <= 0xFFFF;
  const bool gso_none = jlen >= 14 && !raw && t1 == GSO_NONE;
  auto group_live = [&](int y) {
    if (y == 0) return true;
    if (gso_none || y >= ngroups) return false;
    return !split_type || (plen_s > hmin && hmin + (int64_t)y * ROWS * gso_s < plen_s);
  };
  if (!group_live(by)) return;

  uint4 Q;  // readBuf[16r, 16r + 16) (bytes below hdrLen)
  {
    const uint32_t nx = row_next(H0.x);
    Q = make_uint4(__builtin_amdgcn_alignbyte(H0.y, H0.x, hph), __builtin_amdgcn_alignbyte(H0.z, H0.y, hph),
                   __builtin_amdgcn_alignbyte(H0.w, H0.z, hph), __builtin_amdgcn_alignbyte(nx, H0.w, hph));
  }
  // the TCP data offset decides hdrLen (tun.go:601-614): block-uniform verdict
  bool clean = clean_s;
  if (clean && tcp_s && !raw) {
    const int th = (int)((qbyte(Q, cs_s + 12) >> 4) * 4);
    clean = ((cs_s + th) & 0xFFFF) == hdr_s;
  }

  // The payload loads are issued only after this verdict: no payload window
  // is live across the decoded path's call, so the clean path's registers
  // stay its own (the verdict waits on the header chunks, which arrive with
  // the virtio header).  readfirstlane makes the branch provably uniform.
  if (ufl(clean ? 1 : 0)) {
    if (by == 0 && threadIdx.x == 0) {  // the checks can only end in the segment count here
      const int nfull_s = (plen_s - hdr_s + gso_s - 1) / gso_s;
      const bool many = nfull_s > (int)max_segs;
      count[jb] = many ? (int)max_segs - 1 : nfull_s;
      status[jb] = many ? WGCS_ERR_TOO_MANY_SEGMENTS : 0;
    }
    const int type = type_s, ipv = ipv_s, hdr_len = hdr_s, gso = gso_s, cs = cs_s, co = co_s, plen = plen_s;
    // job-constant header sums from this row's own header chunks (header_fast's
    // values): IPv4 header without total length / id / checksum, the L4
    // header from csumStart without checksum field, seq / UDP length and the
    // flags byte, and the pseudo-header addresses, each as BE words
    uint32_t ip_base = 0, l4_base = 0, tflags = 0, id0 = 0, seq0 = 0;
    {
      const int x0 = 16 * r;
      const bool tcp_c = type != GSO_UDP_L4;
      const int vlo = cs + 4, vhi = tcp_c ? cs + 8 : cs + 6;
      const int ca = (cs + co) & 0xFFFF;
      if (ipv == 4) {
        const uint32_t m = byte_bits16(-x0, cs - x0) & ~byte_bits16(2 - x0, 6 - x0) & ~byte_bits16(10 - x0, 12 - x0);
        ip_base = (uint32_t)ufl((int)bswap16(fold32_16(row16_sum_u32(add4_masked(0u, Q, m, false)))));
      }
      uint32_t ml4 = byte_bits16(cs - x0, hdr_len - x0) & ~byte_bits16(ca - x0, ca + 2 - x0) &
                     ~byte_bits16(vlo - x0, vhi - x0);
      if (tcp_c) ml4 &= ~byte_bits16(cs + 13 - x0, cs + 14 - x0);
      const int a_lo = ipv == 4 ? 12 : 8, a_hi = ipv == 4 ? 20 : 40;
      uint32_t s4 = add4_masked(0u, Q, ml4, false);
      s4 = add4_masked(s4, Q, byte_bits16(a_lo - x0, a_hi - x0), (cs & 1) != 0);
      uint32_t t4 = fold32_16(row16_sum_u32(s4));
      if ((cs & 1) == 0) t4 = bswap16(t4);  // pairing from csumStart (packet coordinates)
      if (tcp_c) tflags = qbyte(Q, cs + 13);
      l4_base = (uint32_t)ufl((int)t4) + (tflags & ~0x09u);
      if (ipv == 4) {
        const uint32_t b45 = qdw(Q, 1);  // readBuf[4:8)
        id0 = ((b45 & 0xFFu) << 8) | ((b45 >> 8) & 0xFFu);
      }
      if (tcp_c) seq0 = __builtin_bswap32(qle32(Q, vlo));
    }
    for (int grp = by; has_seg(grp * ROWS); grp += gy) {  // block-uniform
      const int i = grp * ROWS + wv * 4 + (lane >> 4);  // this row's segment
      if (has_seg(i)) {  // row-uniform
        uint8_t* dst = out + obase + (uint64_t)i * opitch + offset;
        const int dalign = (int)((uintptr_t)dst & 15u);
        uint8_t* dbase = dst - dalign;
        // ---- the payload stream
        uint32_t acc = 0;
        stream_row<U, NT>(rb, i, gso, hdr_len, plen, dalign, dbase, r, acc, job_rsrc(vb, jlen));
        finish_row(true, Q, type, ipv, hdr_len, gso, cs, co, plen, i, r, dalign, dst, dbase, acc, ip_base, l4_base,
                   tflags, id0, seq0, &sizes[slot0 + (uint32_t)i]);
      }
    }
  } else {
    for (int grp = by; group_live(grp); grp += gy) {  // block-uniform
      const int i = grp * ROWS + wv * 4 + (lane >> 4);
      uint8_t* dst = out + obase + (uint64_t)i * opitch + offset;
      const int live = decoded_rows<U, NT>(vb, jlen, job.flags, room, max_segs, i, grp == 0, &count[jb], &status[jb],
                                           out + obase + offset, dst, &sizes[slot0], tails);
      lds_barrier();  // every wave is done with this group's verdict before the next one is published
      // the verdict bounds the job's segments (0 for an error / GSO_NONE): no
      // decode + barrier round for groups past it, whatever max_segs is
      if ((int64_t)(grp + gy) * ROWS >= (int64_t)ufl(live)) break;
    }
  }
}

}  // namespace wgcs
