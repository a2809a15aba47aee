// checksum_kernels.hip -- gfx950 (CDNA4) batch Internet-checksum kernels.
//
// Replaces, at batch granularity, the per-packet Go loops of
//   checksum()                     /root/reference/tun/checksum.go:152-167
//   checksumValid()                /root/reference/tun/gro.go:554-612
//   gsoSplit's L4 checksum step    /root/reference/tun/gro.go:1469-1488
//   gsoNoneChecksum()              /root/reference/tun/gro.go:1497-1517
//   IPv4 header checksum sites     /root/reference/tun/gro.go:1134-1138,1434-1436
//
// Design: the launched kernel is checksum_batch_kernel<MODE,
// G = 32, U = 4, NT>: one G-lane group (half a wave64) per packet, two packets
// per wave, an XCD-aware block order, one pass of the grid over batches of up
// to num_cu x 1,024 x 8 frames (grid-stride beyond that; round 5, wgcs_host.h).
// A packet's geometry (wgcs_cs_plan.h) is worked out on the scalar unit from the
// wave-uniform descriptors; the lanes pick up a few words of it and add what
// depends on the packet's alignment.  Each lane streams 16-byte chunks of its
// packet with non-temporal global_load_dwordx4 (U loads in flight per lane:
// 2 KiB per half-wave step, so one iteration covers a 1500-B frame), masks only
// the head / checksum field / tail chunks, and adds both u16 halves of every
// dword into a u32 accumulator with one v_dot2 whose weight is the slot's
// validity (a slot that was not loaded needs no zero fill).  Per-lane fold to 16
// bits, DPP row sums + one cross-row exchange, parity correction,
// pseudo-header / initial, final fold.  G = 16 (a DPP row) and G = 64 (a
// wave) are the tuning alternatives (WGCS_LANES_PER_PKT).  No LDS staging:
// each byte is read once and used once, and a 16-B register load per lane
// already moves 1 KiB per wave instruction -- measured, LDS-DMA staging ties
// register loads on this pattern (profiles/r1_probe_glds.jsonl) -- and no MFMA
// (a byte reduction, not a contraction).
#include <hip/hip_runtime.h>

#include "../../include/wgcsum.h"
#include "wgcs_batch_plan.h"
#include "wgcs_common.h"
#include "wgcs_cs_plan.h"
#include "wgcs_kernels.h"

namespace wgcs {

// Frame and descriptor loads go through global-address-space pointers made
// from the row's scalar address (a generic pointer would turn them into
// flat_load, which waits on both counters).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) u32x4* chunk_ptr;
typedef __attribute__((address_space(1))) uint8_t* gbyte_ptr;

template <bool NT>
__device__ __forceinline__ u32x4 ld_chunk(chunk_ptr p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}

// A chunk whose value does not matter, because an empty mask or a zero weight
// follows: some registers, no instruction (a slot that is not loaded needs no
// zero fill).
__device__ __forceinline__ u32x4 any_chunk() {
  u32x4 v;
  asm volatile("" : "=v"(v));
  return v;
}

// acc + wt.lo * lo16(w) + wt.hi * hi16(w): add_halves with the slot's validity
// as the weight (0x10001 or 0).
__device__ __forceinline__ uint32_t add_halves_w(uint32_t acc, uint32_t w, uint32_t wt) {
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
  return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, w), __builtin_bit_cast(us2, wt), acc, false);
}

// The bytes of w that the 4-bit mask keeps, the others zero: one v_perm_b32
// whose selector byte j is 4 + j (byte j of w) or j (byte j of the zero
// operand).  nib * 0x810204 puts bit j at bit 8 j + 2 (a full-rate 24-bit
// multiply; the stray products fall on other bits and are masked off).
// The two selector constants live in registers (PermK, set once per kernel), so
// that the mask and the merge are one v_and_or_b32: a VOP3 takes no literal.
struct PermK {
  uint32_t keep, ident;
};
__device__ __forceinline__ PermK perm_consts() {
  PermK k = {0x04040404u, 0x03020100u};
  asm volatile("" : "+s"(k.keep), "+v"(k.ident));
  return k;
}
__device__ __forceinline__ uint32_t keep_bytes(uint32_t w, uint32_t nib, const PermK& k) {
  const uint32_t sel = ((nib * 0x00810204u) & k.keep) | k.ident;
  return __builtin_amdgcn_perm(w, 0u, sel);
}

__device__ __forceinline__ uint32_t add_masked(uint32_t acc, const u32x4& v, uint32_t m16, const PermK& k) {
  acc = add_halves(acc, keep_bytes(v.x, m16 & 0xFu, k));
  acc = add_halves(acc, keep_bytes(v.y, (m16 >> 4) & 0xFu, k));
  acc = add_halves(acc, keep_bytes(v.z, (m16 >> 8) & 0xFu, k));
  acc = add_halves(acc, keep_bytes(v.w, (m16 >> 12) & 0xFu, k));
  return acc;
}

// Masked contribution of an edge chunk (head: addresses / gap / field; tail)
// at packet position `pos`, general case.
// `addr`: wave-uniform, false when no packet of the wave has a separate
// address range (merged into the main range, wgcs_cs_plan.h): the second mask is skipped.
__device__ __forceinline__ uint32_t edge_chunk(uint32_t acc, const u32x4& v, int pos, const CsGeom& r, bool rot_addr,
                                               bool addr, const PermK& pk) {
  acc = add_masked(acc, v, cs_main_mask16(r, pos), pk);
  if (addr) {
    const uint32_t a16 = cs_addr_mask16(r, pos);  // the field is zeroed memory
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t y = keep_bytes(w[k], (a16 >> (4 * k)) & 0xFu, pk);
      if (rot_addr) y = rotl8(y);  // 256*y (mod 2^32-1): address pairing parity differs from the main range
      acc = add_halves(acc, y);
    }
  }
  return acc;
}

// Row `grp`'s word of a per-row array of wave-uniform words: w[0] with the
// bits that differ in the lane's own row flipped.  m[k] is all ones in the
// lanes of row k (row_masks).  Two VALU instructions per further row, each
// with one scalar operand; a v_cndmask_b32 of two scalars needs two v_mov
// first (one constant-bus read per instruction).
template <int PPW>
struct RowMasks {
  uint32_t m[PPW];
};
template <int PPW>
__device__ __forceinline__ RowMasks<PPW> row_masks(int grp) {
  RowMasks<PPW> r;
#pragma unroll
  for (int k = 0; k < PPW; ++k) {
    r.m[k] = grp == k ? ~0u : 0u;
    asm volatile("" : "+v"(r.m[k]));  // keep it a mask: as a compare it would become a select again
  }
  return r;
}
template <int PPW>
__device__ __forceinline__ uint32_t row_pick(const uint32_t (&w)[PPW], const RowMasks<PPW>& rm) {
  uint32_t r = w[0];
#pragma unroll
  for (int k = 1; k < PPW; ++k) r ^= (w[0] ^ w[k]) & rm.m[k];
  return r;
}

// Descriptor i (include/wgcsum.h wgcs_pkt) as one dwordx4; i is wave-uniform,
// so this is an s_load_dwordx4: no TA/TD round trip before the first frame load.
__device__ __forceinline__ uint4 row_desc(const uint4* __restrict__ pkts, uint32_t i, uint32_t n) {
  return i < n ? pkts[i] : make_uint4(0, 0, 0, 0);
}

#ifndef WGCS_CS_BLOCK
#define WGCS_CS_BLOCK 256  // threads per block (A/B builds: 512, 1024)
#endif
// The body of one batch: this block is block `blk` of the `nblk` blocks that
// work on it (the whole grid in the single-batch kernel, the batch's share of
// the grid in the multi-batch one).
//
// One packet per group ("row") of G lanes (G = 16: 4 packets per wave in
// flight; G = 64: one wavefront per packet).  The descriptors of a wave's rows
// are consecutive and arrive by scalar loads.  When the rows agree in len,
// csum_start, csum_offset, proto and flags (MTU-sized traffic), cs_geom()
// (wgcs_cs_plan.h: descriptor -> byte ranges) runs once, on the scalar unit,
// and the lanes pick up only their packet's address; when they differ, each
// lane picks up its row's descriptor words and runs cs_geom() itself.
// cs_plan() (what depends on the packet's alignment) always runs per lane.
// The packet's 16-byte chunks are split into "edge" chunks (the
// first ones, up to the end of the address range / gap / checksum field, and a
// partial last one) that need byte masks, and interior chunks that are summed
// unmasked: lanes stream interior chunk c = c_it + sub + G*(u + U*it), so one
// wave instruction reads 64/G contiguous 16*G-byte runs, and each lane owns at
// most a few edge chunks.  A wave with one step (the one-pass grid) runs the
// step without a loop; otherwise the next step's descriptors are prefetched
// by scalar loads, which the frame loads do not wait on.
template <int MODE, int G, int U, bool NT>
__device__ __forceinline__ void checksum_batch_body(uint8_t* __restrict__ arena, const uint4* __restrict__ pkts,
                                                    const uint64_t* __restrict__ initial, uint32_t n,
                                                    void* __restrict__ out, int inplace, uint32_t amask, int xcd,
                                                    uint32_t blk, const uint32_t nblk) {
  static_assert(G == 16 || G == 32 || G == 64, "group = DPP row, half wave or wave");
  constexpr int PPW = 64 / G;  // packets per wave per step
  // VALIDATE and FOLD sum one contiguous byte range unless a packet's address
  // range could not be merged into it; the other modes cut a field out
  // (VALIDATE's wide unrolls, short of registers with both edge paths, keep to the general one)
  constexpr bool kContigMode = MODE == WGCS_MODE_FOLD || (MODE == WGCS_MODE_VALIDATE && U <= 4);
  const int lane = threadIdx.x & 63;
  const int grp = lane / G;
  const int sub = lane % G;
  // XCD-aware order (xcd != 0, nblk a multiple of 8): blocks are dealt
  // round-robin over the 8 XCDs, so logical block (b % 8) * (nblk / 8) + b / 8
  // gives each XCD one contiguous eighth of every grid-stride pass -- frames
  // that share a 128-B line at their boundary are fetched through one L2.
  if (xcd) blk = (blk & 7u) * (nblk >> 3) + (blk >> 3);
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blk * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const uint32_t step = nblk * (blockDim.x >> 6) * PPW;
  const uint32_t it_mask = cs_it_mask(amask);
  const RowMasks<PPW> rm = row_masks<PPW>(grp);
  const PermK pk = perm_consts();
  // one step: the PPW packets from `base` on, descriptors d
  auto do_step = [&](const uint32_t base, const uint4(&d)[PPW]) __attribute__((always_inline)) {
    // scalar: the packets' addresses, and whether the rows share a geometry
    uint32_t w_pa_lo[PPW], w_pa_hi[PPW], w_y[PPW], w_z[PPW], w_w[PPW];
    bool same = base + (uint32_t)PPW <= n;
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
      const uint64_t pa = (uint64_t)(uintptr_t)arena + ((uint64_t)d[k].x | ((uint64_t)(d[k].y & 0xFFFFu) << 32));
      w_pa_lo[k] = (uint32_t)pa;
      w_pa_hi[k] = (uint32_t)(pa >> 32);
      w_y[k] = d[k].y;
      w_z[k] = d[k].z;
      w_w[k] = d[k].w;
      if (k > 0) same = same && ((d[k].z ^ d[0].z) | (d[k].w ^ d[0].w) | ((d[k].y ^ d[0].y) >> 16)) == 0;
    }
    const uint32_t p = base + grp;
    const bool active = p < n;
    const uint32_t pa_lo = row_pick<PPW>(w_pa_lo, rm);
    const uint64_t pa = (uint64_t)pa_lo | ((uint64_t)row_pick<PPW>(w_pa_hi, rm) << 32);
    CsGeom r;  // what the plan and the masks read
    bool contig, any_addr;  // wave-uniform
    if (same) {  // every row active and of one geometry: once, on the scalar unit
      r = cs_geom(MODE, true, d[0].z, d[0].w, (d[0].y >> 16) & 0xFFu, d[0].y >> 24);
      contig = kContigMode && cs_geom_contiguous(r);
      any_addr = r.addr_hi > r.addr_lo;
    } else {  // per lane, from the row's descriptor words
      const uint32_t dy = row_pick<PPW>(w_y, rm);
      r = cs_geom(MODE, active, row_pick<PPW>(w_z, rm), row_pick<PPW>(w_w, rm), (dy >> 16) & 0xFFu, dy >> 24);
      contig = kContigMode && __builtin_amdgcn_ballot_w64(!cs_geom_contiguous(r)) == 0;
      any_addr = __builtin_amdgcn_ballot_w64(r.addr_hi > r.addr_lo) != 0;
    }
    const uint32_t pre = r.pre;
    const bool past = r.past;
    const CsPlan pl = cs_plan(r, pa_lo, amask);
    const int rel0 = pl.rel0, c_lo = pl.c_lo, c_hi = pl.c_hi, n_edge = pl.n_edge;
    const int head = r.lo_all - rel0;
    const int end = r.hi_all - rel0;
    const chunk_ptr src = (chunk_ptr)(pa + (uint64_t)(int64_t)rel0);
    const gbyte_ptr pkt = (gbyte_ptr)pa;
    const int len = r.main_hi;  // L4_FILL and PARTIAL: the summed range ends with the packet
    uint64_t init = 0;
    if (MODE == WGCS_MODE_FOLD) {
      init = (initial && active) ? initial[p] : 0;
    } else if (MODE == WGCS_MODE_PARTIAL) {
      if (r.fld + 1 < len) init = ((uint32_t)pkt[r.fld] << 8) | pkt[r.fld + 1];  // gro.go:1508
    }
    // Slot u of an interior iteration at c0 holds chunk c0 + u G: inside
    // [c_lo, c_hi) and loaded, or not loaded and weighted 0.  Only slot 0 can
    // lie below c_lo (c_lo - c_it < 8 <= G).
    // The weights are worked out again from `left` when the sums run, so
    // that no register per slot stays live across the loads.  The wide
    // unrolls (U > 4, tuning alternatives short of registers) zero-fill instead.
    constexpr bool kWeights = U <= 4;
    u32x4 v[U];
    int left, left0;  // chunks left from c0 on; the same, or 0 where slot 0 lies below c_lo
    auto load_slots = [&](int c0) {
      const chunk_ptr at = src + c0;
      left = c_hi - c0;
      left0 = c0 >= c_lo ? left : 0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (kWeights) v[u] = any_chunk();
        else v[u] = u32x4{0, 0, 0, 0};
        if (u * G < (u ? left : left0)) v[u] = ld_chunk<NT>(at + u * G);
      }
    };
    // two independent v_dot2 chains (x,y / z,w), joined once per iteration:
    // half the serial dependency length of one chain of 4U (round 6)
    auto sum_slots = [&](uint32_t acc) {
      uint32_t acc2 = 0;
      if (kWeights) asm volatile("" : "+v"(left), "+v"(left0) : "v"(v[0].x));  // not before slot 0's data is there
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint32_t wt = (!kWeights || u * G < (u ? left : left0)) ? 0x00010001u : 0u;
        acc = add_halves_w(acc, v[u].x, wt);
        acc2 = add_halves_w(acc2, v[u].z, wt);
        acc = add_halves_w(acc, v[u].y, wt);
        acc2 = add_halves_w(acc2, v[u].w, wt);
      }
      return acc + acc2;  // < 2^17 + 2^21 + 16 U x 2^17: no overflow
    };
    // edge chunks: issued first, consumed after the first interior batch is in flight
    const int ce = cs_edge_chunk_index(sub, c_lo, c_hi);
    u32x4 ve = any_chunk();
    if (sub < n_edge && cs_edge_loaded(ce, head)) ve = ld_chunk<NT>(src + ce);
    // With a 128-byte chunk grid origin (amask 127) the interior iterations
    // start on a line boundary too (c_it: c_lo rounded down to 8 chunks; the
    // lanes below c_lo idle in the first one), so no 128-byte line is shared by
    // two iterations of a row -- with non-temporal loads such a line can be
    // evicted between them and read twice (round 5, profiles/r5_cfg5_traffic*)
    int c0 = cs_first_it(c_lo, it_mask) + sub;
    load_slots(c0);
    uint32_t acc = 0;
    if (contig) {
      // one byte range: the mask is empty wherever the lane holds no edge chunk.
      // One edge chunk per lane is enough: with no hole c_lo <= (amask + 16) / 16, and the
      // context accepts WGCS_ALIGN up to 128 only (api.cpp), amask <= 127, so n_edge <= 9 <= G.
      acc = add_masked(acc, ve, cs_contig_mask16(ce, head, end), pk);
    } else {
      const bool rot_addr = ((r.addr_lo ^ r.main_lo) & 1) != 0;
      u32x4 vg = ve;
      int cg = ce;
      for (int e = sub;;) {  // rows with more than G edge chunks (long field offsets) loop
        if (e < n_edge) acc = edge_chunk(acc, vg, rel0 + 16 * cg, r, rot_addr, any_addr, pk);
        e += G;
        if (e >= n_edge) break;
        cg = cs_edge_chunk_index(e, c_lo, c_hi);
        vg = any_chunk();
        if (cs_edge_loaded(cg, head)) vg = ld_chunk<NT>(src + cg);
      }
    }
    acc = sum_slots(acc);
    for (c0 += G * U; c0 < c_hi; c0 += G * U) {  // frames of more than 16 G U bytes
      acc = (acc >> 16) + (acc & 0xFFFFu);       // keep the u32 partial sum far from overflow (huge packets)
      load_slots(c0);
      acc = sum_slots(acc);
    }
    // all lanes converge here: per-lane fold, group sum, parity, pseudo/initial
    uint32_t s = fold32_16(acc);
    if (G == 16) {
      s = row16_sum_u32(s);
    } else if (G == 32) {  // two DPP rows of the half wave: row sums, then the partner row's (lane ^ 16:
                           // ds_swizzle_b32 in bit mode, and 0x1F / or 0 / xor 0x10 -- no index register)
      s = row16_sum_u32(s);
      s += (uint32_t)__builtin_amdgcn_ds_swizzle((int)s, 0x401F);
    } else {
      s = wave_sum_u32(s);
    }
    s = fold32_16(s);
    if (pl.swap) s = bswap16(s);
    uint32_t t = fold32_16(s + pre + fold64_16(init));  // == the reference's checksum(...)
    // csum_start past the packet: the reference panics on pkt[iphLen:] (a
    // batch has no error channel: VALIDATE 0, L4_FILL 0 and no field write)
    if (sub == 0 && active) {
      if (MODE == WGCS_MODE_VALIDATE) {
        reinterpret_cast<uint8_t*>(out)[p] = (t == 0xFFFFu && !past) ? 1 : 0;  // ^checksum == 0
      } else if (MODE == WGCS_MODE_FOLD) {
        reinterpret_cast<uint16_t*>(out)[p] = (uint16_t)t;
      } else {
        const uint16_t c = past ? (uint16_t)0 : (uint16_t)~t;
        reinterpret_cast<uint16_t*>(out)[p] = c;
        if (inplace && !past && r.fld >= 0 && r.fld + 1 < len) {
          pkt[r.fld] = (uint8_t)(c >> 8);
          pkt[r.fld + 1] = (uint8_t)c;
        }
      }
    }
  };
  uint32_t base = wave * PPW;
  if (base >= n) return;
  uint4 d[PPW];
#pragma unroll
  for (int k = 0; k < PPW; ++k) d[k] = row_desc(pkts, base + (uint32_t)k, n);
  if (base + step >= n) {  // the wave's only step (wave-uniform): no loop, nothing carried
    do_step(base, d);
    return;
  }
  for (;;) {  // wave-uniform loop
    const uint32_t next = base + step;
    uint4 dn[PPW];
    if (next < n) {  // prefetch the next step's descriptors (scalar: the frame loads do not wait on them)
#pragma unroll
      for (int k = 0; k < PPW; ++k) dn[k] = row_desc(pkts, next + (uint32_t)k, n);
    }
    do_step(base, d);
    if (next >= n) break;
    base = next;
#pragma unroll
    for (int k = 0; k < PPW; ++k) d[k] = dn[k];
  }
}

template <int MODE, int G, int U, bool NT>
__global__ __launch_bounds__(WGCS_CS_BLOCK) void checksum_batch_kernel(uint8_t* __restrict__ arena,
                                                             const uint4* __restrict__ pkts,
                                                             const uint64_t* __restrict__ initial,
                                                             uint32_t n, void* __restrict__ out,
                                                             int inplace, uint32_t amask, int xcd) {
  checksum_batch_body<MODE, G, U, NT>(arena, pkts, initial, n, out, inplace, amask, xcd, blockIdx.x, gridDim.x);
}

// The multi-batch form (wgcs_batch_plan.h): one launch walks the batches of a
// group in call order, batch e on blocks [first[e], first[e] + blocks).  The
// table lives in the kernel-argument segment and the block index is
// wave-uniform, so the lookup runs on the scalar path: the 32 prefix words in
// two wide loads and a branch-free count (or one shift when every batch has
// the same power-of-two block count), then the entry as one more scalar load.
// Every first[e] is a multiple of 8, so a block's XCD (blockIdx % 8) is the
// same inside its batch as in the grid, and the grid stride stays per batch.
// Never in place: such calls keep their per-batch launches.
template <int MODE, int G, int U, bool NT>
__global__ __launch_bounds__(WGCS_CS_BLOCK) void checksum_batch_kernel(const BatchTable t, uint32_t amask, int xcd) {
  const uint32_t bi = blockIdx.x;
  uint32_t e;
  if (t.same_shift != kBatchNoEntry) {
    e = bi >> t.same_shift;
  } else {
    e = 0;  // first[] ascends (kBatchNoEntry behind the last entry): the last entry that starts at or below bi
#pragma unroll
    for (uint32_t k = 1; k < kBatchGroupMax; ++k) e = bi >= t.first[k] ? k : e;
  }
  const BatchEntry& b = t.e[e];
  checksum_batch_body<MODE, G, U, NT>(b.arena, reinterpret_cast<const uint4*>(b.pkts), b.initial, b.n, b.out, 0, amask,
                                      xcd, bi - b.first, b.blocks);
}

template <int MODE>
static hipError_t launch_mode(uint8_t* arena, const wgcs_pkt* pkts, const uint64_t* init, uint32_t n, void* out,
                              int inplace, hipStream_t s, int num_cu, const LaunchTuning& t) {
  const int ppb = (64 / t.lanes_per_pkt) * (WGCS_CS_BLOCK / 64);  // packets per block per step
  long want = ((long)n + ppb - 1) / ppb;
  want = (want + 7) & ~7L;  // a multiple of 8 keeps the XCD-aware order (blocks past n exit at once)
  long cap = (long)num_cu * t.blocks_per_cu;
  cap = cap > 8 ? cap & ~7L : cap;
  const int grid = (int)(want < cap ? want : cap);
  const uint32_t amask = (uint32_t)(t.align >= 16 ? t.align : 16) - 1u;
  const int xcd = (t.xcd && grid % 8 == 0) ? 1 : 0;
  const uint4* d = reinterpret_cast<const uint4*>(pkts);
#define WGCS_LAUNCH(G, U)                                                                                    \
  do {                                                                                                      \
    if (t.nt)                                                                                               \
      hipLaunchKernelGGL((checksum_batch_kernel<MODE, G, U, true>), dim3(grid), dim3(WGCS_CS_BLOCK), 0, s, arena, d, \
                         init, n, out, inplace, amask, xcd);                                                \
    else                                                                                                    \
      hipLaunchKernelGGL((checksum_batch_kernel<MODE, G, U, false>), dim3(grid), dim3(WGCS_CS_BLOCK), 0, s, arena, d, \
                         init, n, out, inplace, amask, xcd);                                                \
  } while (0)
  if (t.lanes_per_pkt == 64) {
    if (t.unroll >= 4) WGCS_LAUNCH(64, 4);
    else WGCS_LAUNCH(64, 2);
  } else if (t.lanes_per_pkt == 32) {
    if (t.unroll >= 6) WGCS_LAUNCH(32, 6);
    else if (t.unroll >= 4) WGCS_LAUNCH(32, 4);
    else WGCS_LAUNCH(32, 3);
  } else {
    if (t.unroll >= 8) WGCS_LAUNCH(16, 8);
    else if (t.unroll >= 6) WGCS_LAUNCH(16, 6);
    else WGCS_LAUNCH(16, 4);
  }
#undef WGCS_LAUNCH
  return hipGetLastError();
}

template <int MODE>
static hipError_t launch_group_mode(const BatchTable& tab, hipStream_t s, const LaunchTuning& t) {
  const uint32_t amask = (uint32_t)(t.align >= 16 ? t.align : 16) - 1u;
  const int xcd = t.xcd ? 1 : 0;  // every batch's block count is a multiple of 8
#define WGCS_LAUNCH(G, U)                                                                                          \
  do {                                                                                                            \
    if (t.nt)                                                                                                     \
      hipLaunchKernelGGL((checksum_batch_kernel<MODE, G, U, true>), dim3(tab.total), dim3(WGCS_CS_BLOCK), 0, s, tab, \
                         amask, xcd);                                                                             \
    else                                                                                                          \
      hipLaunchKernelGGL((checksum_batch_kernel<MODE, G, U, false>), dim3(tab.total), dim3(WGCS_CS_BLOCK), 0, s, tab, \
                         amask, xcd);                                                                             \
  } while (0)
  if (t.lanes_per_pkt == 64) {
    if (t.unroll >= 4) WGCS_LAUNCH(64, 4);
    else WGCS_LAUNCH(64, 2);
  } else if (t.lanes_per_pkt == 32) {
    if (t.unroll >= 6) WGCS_LAUNCH(32, 6);
    else if (t.unroll >= 4) WGCS_LAUNCH(32, 4);
    else WGCS_LAUNCH(32, 3);
  } else {
    if (t.unroll >= 8) WGCS_LAUNCH(16, 8);
    else if (t.unroll >= 6) WGCS_LAUNCH(16, 6);
    else WGCS_LAUNCH(16, 4);
  }
#undef WGCS_LAUNCH
  return hipGetLastError();
}

int checksum_pkts_per_block(const LaunchTuning& t) { return (64 / t.lanes_per_pkt) * (WGCS_CS_BLOCK / 64); }

hipError_t launch_checksum_group(int mode, const BatchTable& tab, hipStream_t s, const LaunchTuning& tune) {
  if (tab.count == 0 || tab.total == 0) return hipSuccess;
  switch (mode) {
    case WGCS_MODE_FOLD:
      return launch_group_mode<WGCS_MODE_FOLD>(tab, s, tune);
    case WGCS_MODE_L4_FILL:
      return launch_group_mode<WGCS_MODE_L4_FILL>(tab, s, tune);
    case WGCS_MODE_VALIDATE:
      return launch_group_mode<WGCS_MODE_VALIDATE>(tab, s, tune);
    case WGCS_MODE_PARTIAL:
      return launch_group_mode<WGCS_MODE_PARTIAL>(tab, s, tune);
    case WGCS_MODE_IP4HDR:
      return launch_group_mode<WGCS_MODE_IP4HDR>(tab, s, tune);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t launch_checksum_batch(int mode, unsigned flags, uint8_t* arena, const wgcs_pkt* pkts,
                                 const uint64_t* init, uint32_t n, void* out, hipStream_t s, int num_cu,
                                 const LaunchTuning& tune) {
  if (n == 0) return hipSuccess;
  const int inplace = (flags & WGCS_F_INPLACE) ? 1 : 0;
  switch (mode) {
    case WGCS_MODE_FOLD:
      return launch_mode<WGCS_MODE_FOLD>(arena, pkts, init, n, out, inplace, s, num_cu, tune);
    case WGCS_MODE_L4_FILL:
      return launch_mode<WGCS_MODE_L4_FILL>(arena, pkts, init, n, out, inplace, s, num_cu, tune);
    case WGCS_MODE_VALIDATE:
      return launch_mode<WGCS_MODE_VALIDATE>(arena, pkts, init, n, out, inplace, s, num_cu, tune);
    case WGCS_MODE_PARTIAL:
      return launch_mode<WGCS_MODE_PARTIAL>(arena, pkts, init, n, out, inplace, s, num_cu, tune);
    case WGCS_MODE_IP4HDR:
      return launch_mode<WGCS_MODE_IP4HDR>(arena, pkts, init, n, out, inplace, s, num_cu, tune);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace wgcs
