// wgcs_cs_plan.h -- the per-packet geometry of the batch checksum kernel
// (checksum_kernels.hip): which bytes of a packet are summed,
// how they are cut into 16-byte chunks, which chunks need a byte mask ("edge")
// and which are summed whole ("interior"), and the parity / pseudo-header terms
// of the final fold.  Plain C++ and no HIP types, like wgcs_batch_plan.h: the
// kernel and the stand-alone sanitizer program of tests/cs_plan_host/ use the
// same functions.  In the kernel cs_geom() runs on the scalar unit, once per
// row of lanes (once per wave when the rows' descriptors agree), and cs_plan()
// per lane on the few words the lanes pick up from it.
//
// Two steps:
//  - cs_geom(): descriptor + mode -> byte ranges relative to the packet start.
//    Nothing here depends on where the packet lies in memory.
//  - cs_plan(): geometry + the low bits of the packet's address + `amask` (the
//    chunk grid origin is rounded down to amask + 1 bytes: 16, or 128 so that a
//    row's loads cover whole cache lines) -> chunk counts and parity bits.
//
// Chunk c of a packet covers packet bytes [rel0 + 16 c, rel0 + 16 c + 16).
// Edge chunks are e = 0 .. n_edge - 1: chunk e while e < c_lo (up to the end of
// the address range / gap / checksum field), then c_hi + (e - c_lo) (a partial
// last chunk).  Interior chunks are [c_lo, c_hi); the lanes walk them from c_it
// (c_lo rounded down to a 128-byte line with a 128-byte origin).
#pragma once

#include <stdint.h>

#include "../../include/wgcsum.h"

#if defined(__HIP__)
#define WGCS_CS_HD __attribute__((host)) __attribute__((device)) inline
#else
#define WGCS_CS_HD inline
#endif

namespace wgcs {

constexpr int kCsNoField = -1000000;  // fld of a mode without an excluded field

WGCS_CS_HD int cs_min(int a, int b) { return a < b ? a : b; }
WGCS_CS_HD int cs_max(int a, int b) { return a > b ? a : b; }
WGCS_CS_HD int cs_clamp16(int x) { return cs_min(cs_max(x, 0), 16); }

// Byte ranges of one packet, all positions relative to the packet start.
struct CsGeom {
  int main_lo, main_hi;  // summed range (BE word pairing starts at main_lo)
  int addr_lo, addr_hi;  // pseudo-header address range (empty: both 0)
  int fld;               // 2 excluded bytes at [fld, fld + 2), or kCsNoField
  int lo_all, hi_all;    // hull of both ranges
  int hole_end;          // chunks that end at or before it need a mask
  uint32_t pre;          // {0, proto} + BE16(len - csum_start) (L4_FILL, VALIDATE)
  bool past;             // csum_start past the packet: VALIDATE 0, L4_FILL 0 and no field write
};

// `active` false (a row past the end of the batch): nothing is summed or read.
WGCS_CS_HD CsGeom cs_geom(int mode, bool active, uint32_t len_word, uint32_t cs_word, uint32_t proto, uint32_t flags) {
  CsGeom g;
  const int len = active ? (int)len_word : 0;
  const int cs = (int)(cs_word & 0xFFFFu);
  const int fld16 = (int)((cs_word + (cs_word >> 16)) & 0xFFFFu);  // u16 field position: csum_start + csum_offset
  const bool v6 = (flags & WGCS_PKT_V6) != 0;
  g.main_lo = 0;
  g.main_hi = len;
  g.addr_lo = g.addr_hi = 0;
  g.fld = kCsNoField;
  g.pre = 0;
  g.past = false;
  if (mode == WGCS_MODE_L4_FILL || mode == WGCS_MODE_VALIDATE) {
    g.main_lo = cs_min(cs, len);
    // the address slices are not bounded by len: a packet shorter than its
    // addresses has them read from the arena bytes after it
    if (active) {
      g.addr_lo = v6 ? 8 : 12;
      g.addr_hi = v6 ? 40 : 20;
    }
    if (mode == WGCS_MODE_L4_FILL) g.fld = fld16;
    g.pre = proto + ((uint32_t)(len - cs) & 0xFFFFu);
    g.past = cs > len;
  } else if (mode == WGCS_MODE_PARTIAL) {
    g.main_lo = cs_min(cs, len);
    g.fld = fld16;
  } else if (mode == WGCS_MODE_IP4HDR) {
    g.main_hi = cs_min(cs, len);
    g.fld = 10;
  }
  // pseudo-header addresses that end where the summed range starts (header
  // length 20 / 40, the usual case) pair the same way: one range
  // [addr_lo, len) with one mask, and from there no gap to mask
  if (g.addr_hi > g.addr_lo && g.addr_hi == g.main_lo && ((g.addr_lo ^ g.main_lo) & 1) == 0) {
    g.main_lo = g.addr_lo;
    g.addr_lo = g.addr_hi = 0;
  }
  // the hull of both ranges, and where the masked head ends; an empty address
  // range is (0, 0), which the maxima pass over (main_hi, main_lo >= 0)
  g.lo_all = cs_min(g.main_lo, g.addr_hi > g.addr_lo ? g.addr_lo : 0x7FFFFFFF);
  g.hi_all = cs_max(g.main_hi, g.addr_hi);
  g.hole_end = cs_max(g.main_lo, g.addr_hi);
  if (g.fld + 2 > g.lo_all && g.fld < g.hi_all) g.hole_end = cs_max(g.hole_end, g.fld + 2);
  return g;
}

// One contiguous summed range and nothing else: the edge chunks' masks follow
// from two byte counts (cs_contig_mask16).
WGCS_CS_HD bool cs_geom_contiguous(const CsGeom& g) { return g.addr_hi <= g.addr_lo && g.fld == kCsNoField; }

struct CsPlan {
  int rel0;      // chunk grid origin relative to the packet start (<= lo_all, > lo_all - amask - 1)
  int nch;       // chunks that hold a summed byte or lie before one
  int c_lo;      // first interior chunk
  int c_hi;      // end of the interior chunks
  int n_edge;    // c_lo + (1 if the last chunk is partial)
  bool swap;     // main range starts at an even address: the LE sum is byte-swapped
  bool rot_addr; // address range pairs the other way round than the main range
};

WGCS_CS_HD CsPlan cs_plan(const CsGeom& g, uint32_t pbase_low, uint32_t amask) {
  CsPlan p;
  p.rel0 = g.lo_all - (int)((pbase_low + (uint32_t)g.lo_all) & amask);
  p.nch = g.hi_all > g.lo_all ? (g.hi_all - p.rel0 + 15) >> 4 : 0;
  p.c_lo = cs_min((g.hole_end - p.rel0 + 15) >> 4, p.nch);
  // none for an empty range: with a 128-byte origin rel0 may lie 127 bytes below it
  p.c_hi = p.nch ? cs_max((g.hi_all - p.rel0) >> 4, p.c_lo) : 0;
  p.n_edge = p.c_lo + (p.nch - p.c_hi);
  p.swap = ((pbase_low + (uint32_t)g.main_lo) & 1u) == 0;
  p.rot_addr = ((g.addr_lo ^ g.main_lo) & 1) != 0;
  return p;
}

// First chunk of the interior walk: with a 128-byte origin the iterations
// start on a line boundary too (the lanes below c_lo idle in the first one).
WGCS_CS_HD uint32_t cs_it_mask(uint32_t amask) { return amask >= 127u ? ~7u : ~0u; }
WGCS_CS_HD int cs_first_it(int c_lo, uint32_t it_mask) { return (int)((uint32_t)c_lo & it_mask); }

// Edge chunk e -> chunk index.
WGCS_CS_HD int cs_edge_chunk_index(int e, int c_lo, int c_hi) { return e < c_lo ? e : c_hi + (e - c_lo); }
// Edge chunks wholly before the first summed byte have an empty mask and are
// not loaded.  `head` = lo_all - rel0.
WGCS_CS_HD bool cs_edge_loaded(int ce, int head) { return 16 * ce + 16 > head; }

// Bit mask of bytes [lo, hi) inside a 16-byte chunk (lo / hi relative to the
// chunk, any int; clamped).
WGCS_CS_HD uint32_t cs_byte_bits16(int lo, int hi) {
  lo = cs_clamp16(lo);
  hi = cs_clamp16(hi);
  const uint32_t h = (1u << hi) - 1u;
  const uint32_t l = (1u << lo) - 1u;
  return h & ~l;
}

// Contiguous case: mask of chunk ce from head = lo_all - rel0 and
// end = hi_all - rel0.  Empty for every chunk outside the range, so a lane
// that holds no edge chunk needs no other test.
WGCS_CS_HD uint32_t cs_contig_mask16(int ce, int head, int end) {
  const int a = cs_clamp16(head - 16 * ce);
  const int b = cs_min(cs_max(end - 16 * ce, a), 16);
  return (1u << b) - (1u << a);
}

// General case: the main-range mask and the address-range mask of the chunk
// at packet position pos, the field's two bytes taken out of both.
WGCS_CS_HD uint32_t cs_field_bits16(int fld, int pos) {
  const int f = fld - pos;
  return (f >= -1 && f < 16) ? (((3u << (f + 1)) >> 1) & 0xFFFFu) : 0u;
}
WGCS_CS_HD uint32_t cs_main_mask16(const CsGeom& g, int pos) {
  return cs_byte_bits16(g.main_lo - pos, g.main_hi - pos) & ~cs_field_bits16(g.fld, pos);
}
WGCS_CS_HD uint32_t cs_addr_mask16(const CsGeom& g, int pos) {
  return cs_byte_bits16(g.addr_lo - pos, g.addr_hi - pos) & ~cs_field_bits16(g.fld, pos);
}

}  // namespace wgcs
