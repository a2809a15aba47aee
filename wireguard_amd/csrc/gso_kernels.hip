// gso_kernels.hip -- gfx950 GSO split (TSO/USO super-packet -> MSS segments).
//
// Device-resident batch of the reference's Tun.Read path:
//   handleVirtioRead validation/dispatch   /root/reference/tun/tun.go:514-632
//   gsoSplit                               /root/reference/tun/gro.go:1373-1493
//   gsoNoneChecksum (GSO_NONE + NEEDS_CSUM) /root/reference/tun/gro.go:1497-1517
//
// Mapping (gso_rows_kernel): one 16-lane DPP row per OUTPUT segment (slot =
// job * max_segs + i), 16 segments per 256-thread block, grid = (job,
// segment group).  For the common ("clean") job every wave derives the split
// geometry from the virtio header and the header chunks it loads (one
// 16-byte load of the virtio header + one dword-aligned 16-byte window per
// lane), issues its payload loads (dword-aligned
// 16-byte windows, U per lane in flight) and, with no decode step and no
// barrier,
//   1. shifts each window to the destination's byte phase (alignbyte with the
//      next lane's first dword via DPP row_ror), sums the L4 bytes from the
//      same registers (v_dot2) and stores full global_store_dwordx4 chunks;
//   2. computes the IPv4 and L4 checksums from the row sum plus the header
//      sums of its own header chunks and the rewritten field values, rewrites
//      the header chunk and stores it last -- every output byte written once.
// Any other job takes the decoded path: wave 0 runs the full validation and
// publishes its verdict through LDS (one barrier), the rows follow it.
// Reference quirks reproduced bit-for-bit: IPv4 ID is
// id0 + 1 for every segment i >= 1; TCP seq uses a uint16 product
// gsoSize * uint16(i); FIN/PSH cleared on all but the last segment; no UDP
// 0 -> 0xFFFF substitution; ErrTooManySegments returns n = max_segs - 1.
#include "gso_device.h"

namespace wgcs {

template <int U, bool NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WGCS_GSO_WAVES, 8))) void gso_rows_kernel(const uint8_t* __restrict__ arena,
                                                       const wgcs_gso_job* __restrict__ jobs, uint32_t max_segs,
                                                       uint8_t* __restrict__ out, uint32_t out_stride,
                                                       const GsoOutPos* __restrict__ outpos, uint32_t offset,
                                                       uint32_t room, int32_t* __restrict__ sizes,
                                                       int32_t* __restrict__ count, int32_t* __restrict__ status) {
  const uint32_t jb = blockIdx.x;
  const GsoOutPos pos = outpos ? outpos[jb] : GsoOutPos{};
  gso_rows_body<U, NT>(arena, jobs[jb], jb, (int)blockIdx.y, (int)gridDim.y, max_segs, out, out_stride,
                       outpos != nullptr, pos, offset, room, sizes, count, status);
}

// ---------------------------------------------------------------------------
// Job staged whole in LDS (round 5): one workgroup of NW waves per job.
//
// gso_rows_kernel's payload loads wait on a dependent chain: the job
// descriptor, then the virtio header and header chunks, then the verdict and
// the segment geometry; only then does a row know which bytes to load
// (≈ 4.7 µs of a one-stream cfg4 launch).  Here the payload
// loads depend on the descriptor alone: every wave issues, right after its
// header loads, LDS-DMA loads (global_load_lds_dwordx4) of its share of the
// job's 16-byte chunks into a 65-KiB LDS image of the job, whatever the
// geometry turns out to be.  The head (verdict, segment count, job-constant
// sums) runs while those loads are in flight; then one vmcnt(0) + barrier,
// and every row streams its segments out of LDS through the same consume /
// finish code as the register path (dword-aligned 16-byte windows, shifted to
// the destination phase, summed, stored; header chunk last).  So every input
// byte is read from HBM once, by one load issued at the start of the launch.
//
// A job larger than the image (> 65,545 bytes at a 15-byte phase) streams
// its rows from HBM as gso_rows_kernel does; every job that is not clean
// takes the decoded path (decoded_rows) with NW * 4 rows per group.
constexpr int kVmcnt0 = 0x0F70;  // s_waitcnt vmcnt(0) expcnt(7) lgkmcnt(15): gfx9 encoding, loads / stores only
constexpr int kImgBytes = 66560;  // 4,160 chunks: a 65,545-byte job ([virtio hdr | 65,535 B]) at any 16-B phase

// 16 bytes at the 4-byte aligned LDS offset o of the image (two ds_read2_b32).
__device__ __forceinline__ uint4 img16(const uint8_t* img, int o) {
  typedef unsigned int u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));
  const u32x4a4 t = *reinterpret_cast<const u32x4a4*>(__builtin_assume_aligned(img + o, 4));
  return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ uint32_t img4(const uint8_t* img, int o) {
  return *reinterpret_cast<const uint32_t*>(__builtin_assume_aligned(img + o, 4));
}

// load_windows from the LDS image (job byte x at image offset ibias + x).
// Unlike the HBM form, windows outside the row's payload bytes [lo, hi) are
// read too (from LDS, no memory traffic) and not zeroed: consume_batch masks
// every byte of a chunk outside [hdrLen, pktLen) -- the bytes such a window
// contributes -- out of every sum and store.  Offsets below the image (a
// window before the payload) clamp to 0; the image array has room for every
// window past the job's end (>= 1,552 bytes of slack, gso_lds_kernel).
template <int U>
__device__ __forceinline__ void img_windows(const uint8_t* img, int ibias, int aoff, int k0, int r, uint4 (&A)[U],
                                            uint32_t& E) {
  const int o0 = ibias + aoff + 16 * (k0 + r);
#pragma unroll
  for (int u = 0; u < U; ++u) A[u] = img16(img, max(o0 + 256 * u, 0));
  E = img4(img, max(ibias + aoff + 16 * (k0 + 16 * U), 0));  // used by lane 15 only
}

template <int U>
__device__ __forceinline__ void stream_row_img(const uint8_t* img, int ibias, const uint8_t* rb, int i, int gso,
                                               int hdr_len, int plen, int dalign, uint8_t* dbase, int r,
                                               uint32_t& acc, RowOut& ro) {
  const RowSrc g = row_src(rb, i, gso, hdr_len, plen, dalign);
  acc = 0;
  for (int k0 = 0; k0 < g.nk; k0 += 16 * U) {
    uint4 A[U];
    uint32_t E;
    img_windows<U>(img, ibias, g.aoff, k0, r, A, E);
    consume_batch_img<U>(A, E, k0, g, hdr_len, dalign, dbase, r, acc, ro);
  }
}

// The head's inputs: the header chunks (lane r of each row: readBuf[16r, 16r +
// 16) from the dword holding it) and the 16 bytes from the dword holding vb[0].
struct HeadIn {
  uint4 H0, w;
};
// The head's results in registers (wave-uniform except Q: lane r of each
// row holds readBuf[16r, 16r + 16)).
struct HeadRes {
  int clean, type, ipv, hdr_len, gso, cs, co, plen;
  uint32_t ip_base, l4_base, tflags, id0, seq0;
  uint4 Q;
};
// The head's results, published by the head wave through LDS.
struct LdsHead {
  int32_t clean;  // 1: the row-streaming path (a clean job, gso_rows_kernel's criterion)
  int32_t type, ipv, hdr_len, gso, cs, co, plen;
  uint32_t ip_base, l4_base, tflags, id0, seq0;
  uint4 q[16];  // readBuf[16r, 16r + 16) per row lane r (P > 1)
};

// Launch shape: P = 3 workgroups of 4 waves per read (round 5, late):
// 6.35-6.46 us per cfg4 launch on four streams against 6.73-7.31 for one
// workgroup of 8 waves, 9.72-9.88 against 9.13-9.18 on one stream, the same
// HBM bytes (profiles/r5_gso_p3_ab*.jsonl, r5_pmc/); several reads in flight
// (the bench's four streams, a stager's batches) is the regime this serves.
#ifndef WGCS_GSO_LDS_WAVES
#define WGCS_GSO_LDS_WAVES 4
#endif
#ifndef WGCS_GSO_PARTS
#define WGCS_GSO_PARTS 3
#endif
// One workgroup of NW waves per job.  Wave 0 issues the header loads, then
// every wave its share of the LDS-DMA loads of the whole job; wave 0 runs the
// head (verdict, segment count, job-constant header sums) while they are in
// flight and publishes it through LDS; one vmcnt(0) + barrier; then every row
// streams its segments out of the image (header chunks read from it as well)
// with write-through full-chunk stores: the segment stores follow the loads in
// this kernel, so the lines go to HBM while the rows still work instead of
// in one end-of-kernel writeback of every segment (≈ 17 MB for cfg4).
// P > 1 (round 5): P workgroups per job, each staging about 1/P of the job
// (part p: the segments whose payload starts in job bytes [p H, (p + 1) H),
// H = len / P rounded up to 16, plus one segment's worth past that for the
// last one), so a block holds 1/P of the LDS and rows -- P = 2: 40 KB, 4
// blocks per CU instead of 2 -- and its rows run one pass.  The parts of a job
// are dealt to one XCD (their shared header lines and boundary bytes meet in
// one L2).  Every part runs the head; part 0 writes count / status and runs
// the decoded path of a job that is not clean.  A row whose bytes lie outside
// its part's image (gsoSize > 1,536) streams from HBM.
template <int NW, int U, bool NT, int P>
__global__ __launch_bounds__(NW * 64) void gso_lds_kernel(const uint8_t* __restrict__ arena,
                                                          const wgcs_gso_job* __restrict__ jobs, uint32_t max_segs,
                                                          uint8_t* __restrict__ out, uint32_t out_stride,
                                                          const GsoOutPos* __restrict__ outpos, uint32_t offset,
                                                          uint32_t room, int32_t* __restrict__ sizes,
                                                          int32_t* __restrict__ count, int32_t* __restrict__ status,
                                                          uint32_t n_jobs) {
  constexpr int ROWS = NW * 4;  // 16-lane rows per workgroup
  // a part's staged bytes: H (at most kImgBytes / P rounded up) + 48 before +
  // kPartTail past its end; the image also holds 1,552 bytes of window slack
  constexpr int kPartTail = 1536 + 32;
  constexpr int kStage = P == 1 ? kImgBytes : ((kImgBytes + P - 1) / P + 15) / 16 * 16 + 48 + kPartTail + 16;
  constexpr int kIters = ((kStage + 1552) / 16 + NW * 64 - 1) / (NW * 64);  // LDS-DMA instructions per wave
  constexpr int kArr = kIters * NW * 64 * 16;                      // every slot a DMA writes
  static_assert(kArr >= kStage + 1552, "image slack for the windows past a job's end");
  __shared__ __attribute__((aligned(16))) uint8_t img[kArr];
  __shared__ LdsHead hd;
  const int lane = threadIdx.x & 63;
  const int r = lane & 15;
  const int wv = threadIdx.x >> 6;
  uint32_t jb = blockIdx.x;
  int part = 0;
  if (P > 1) {  // blocks b, b + 8, ... share an XCD: job (k / P) * 8 + b % 8, part k % P (k = b / 8)
    const uint32_t k = blockIdx.x >> 3;
    jb = (k / P) * 8 + (blockIdx.x & 7u);
    part = (int)(k % P);
    if (jb >= n_jobs) return;  // the grid is padded to a multiple of 8 jobs
  }
  const wgcs_gso_job job = jobs[jb];
  const uint8_t* vb = arena + job.off;
  const uint32_t jlen = job.len;
  const uint8_t* rb = vb + 10;
  const uint64_t slot0 = (uint64_t)jb * max_segs;
  uint64_t obase = slot0 * out_stride;
  uint32_t opitch = out_stride;
  uint32_t tails = 1;
  if (outpos) {
    obase = outpos[jb].base;
    opitch = outpos[jb].pitch;
    tails = outpos[jb].flags & kOutPosTails;
  }
  const int ibias = (int)((uintptr_t)vb & 15u);
  const int nch = (int)((jlen + (uint32_t)ibias + 15u) >> 4);
  // this part's image: chunks [q_lo, q_lo + q_n) of the job (chunk q = the
  // aligned 16 bytes at (vb & ~15) + 16 q); job byte x at image offset x + ib_p
  const int H = P == 1 ? 0 : (int)(((jlen + P - 1) / P + 15u) & ~15u);
  int q_lo = 0, q_n = nch;
  if (P > 1) {
    q_lo = max(0, (part * H + ibias) / 16 - 3);
    const int q_hi = part == P - 1 ? nch : min(nch, ((part + 1) * H + kPartTail + ibias + 15) / 16);
    q_n = max(0, q_hi - q_lo);
  }
  const int ib_p = ibias - 16 * q_lo;
  const bool use_img = P == 1 ? (jlen >= 14 && nch <= kImgBytes / 16)  // block-uniform
                              : (jlen >= 14 && q_n <= kStage / 16);
  const bool raw = (job.flags & WGCS_GSO_JOB_RAW) != 0;
  // ---- the head wave (wave 0): header chunks (as gso_rows_kernel) and the
  // virtio header + readBuf[0] (16 bytes from the dword holding vb[0],
  // range-checked: zeros past the job), issued ahead of its bulk loads so
  // that the head waits for them alone (a counted vmcnt)
  const int hph = (int)((uintptr_t)rb & 3u);
  const uint8_t* hbase = rb - hph;
  const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(hbase), (short)0, (int)(jlen + 3u) - (int)(hbase - vb), 0x00020000);
  const int sh = (int)((uintptr_t)vb & 3u);
  // P > 1, a read long enough: the head's inputs through the
  // scalar path (s_load from uniform addresses), so they do not queue in the
  // CU's vector-memory pipeline behind the LDS-DMA of the blocks already on
  // it; the 64 header dwords become per-lane chunks by selects
  const bool shead = P > 1 && jlen >= 288;  // block-uniform
  // (returned by value: a lambda writing outer H0 / w variables by reference
  // put them in scratch memory, whose loads then queued behind the bulk DMA)
  auto head_loads = [&]() -> HeadIn {
    uint4 H0 = make_uint4(0, 0, 0, 0), w = make_uint4(0, 0, 0, 0);
    if (!shead) {
      H0 = bld16<false>(hrs, 16 * r);
      const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<uint8_t*>(vb - sh), (short)0, (int)(jlen + 3u + (uint32_t)sh), 0x00020000);
      w = bld16<false>(vrs, 0);
    } else {
      typedef const __attribute__((address_space(4))) uint32_t* cptr;  // constant space: s_load
      const cptr vp = (cptr)(const void*)(vb - sh);
      w = make_uint4(vp[0], vp[1], vp[2], vp[3]);
      const cptr hp = (cptr)(const void*)hbase;
      uint32_t hv[64];
#pragma unroll
      for (int k = 0; k < 64; ++k) hv[k] = hp[k];
#pragma unroll
      for (int k = 0; k < 16; ++k) {  // lane r of each row takes dwords 4r .. 4r + 3
        const bool m = r == k;
        H0.x = m ? hv[4 * k] : H0.x;
        H0.y = m ? hv[4 * k + 1] : H0.y;
        H0.z = m ? hv[4 * k + 2] : H0.z;
        H0.w = m ? hv[4 * k + 3] : H0.w;
      }
    }
    return HeadIn{H0, w};
  };
  // ---- every wave: its share of the whole job into the LDS image.  Chunk q
  // = the aligned 16 bytes at (vb & ~15) + 16 q, image offset 16 q (job byte x
  // at ibias + x); an aligned chunk holding a job byte lies in that byte's
  // page.  kIters instructions per wave unconditionally, through a
  // range-checked resource over the job's chunks (loads past it are dropped;
  // a job too large for the image gets an empty range): a fixed count of
  // loads behind wave 0's header loads.
  auto bulk_loads = [&]() {
    const __amdgpu_buffer_rsrc_t irs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(vb - ibias + 16 * q_lo), (short)0, use_img ? 16 * q_n : 0, 0x00020000);
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
      const int q0 = (it * NW + wv) * 64;  // this wave-instruction's first chunk (1 KiB of LDS)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(irs, (__attribute__((address_space(3))) void*)(img + 16 * q0), 16,
                                               16 * (q0 + lane), 0, 0, NT ? 2 : 0);
    }
  };
  // ---- wave 0: the head, while the bulk loads are in flight.
  // The job-constant header sums (as gso_rows_kernel) of a clean job:
  auto head_sums = [&](HeadRes& h) {
    const bool tcp_s = h.type != GSO_UDP_L4;
    const uint4 Q = h.Q;
    const int cs = h.cs, hdr_len = h.hdr_len, ipv = h.ipv;
    const int x0 = 16 * r;
    const int vlo = cs + 4, vhi = tcp_s ? cs + 8 : cs + 6;
    const int ca = (cs + h.co) & 0xFFFF;
    uint32_t ip_base = 0, l4_base = 0, tflags = 0, id0 = 0, seq0 = 0;
    if (ipv == 4) {
      const uint32_t m = byte_bits16(-x0, cs - x0) & ~byte_bits16(2 - x0, 6 - x0) & ~byte_bits16(10 - x0, 12 - x0);
      ip_base = (uint32_t)ufl((int)bswap16(fold32_16(row16_sum_u32(add4_masked(0u, Q, m, false)))));
    }
    uint32_t ml4 = byte_bits16(cs - x0, hdr_len - x0) & ~byte_bits16(ca - x0, ca + 2 - x0) &
                   ~byte_bits16(vlo - x0, vhi - x0);
    if (tcp_s) ml4 &= ~byte_bits16(cs + 13 - x0, cs + 14 - x0);
    const int a_lo = ipv == 4 ? 12 : 8, a_hi = ipv == 4 ? 20 : 40;
    uint32_t s4 = add4_masked(0u, Q, ml4, false);
    s4 = add4_masked(s4, Q, byte_bits16(a_lo - x0, a_hi - x0), (cs & 1) != 0);
    uint32_t t4 = fold32_16(row16_sum_u32(s4));
    if ((cs & 1) == 0) t4 = bswap16(t4);
    if (tcp_s) tflags = qbyte(Q, cs + 13);
    l4_base = (uint32_t)ufl((int)t4) + (tflags & ~0x09u);
    if (ipv == 4) {
      const uint32_t b45 = qdw(Q, 1);
      id0 = ((b45 & 0xFFu) << 8) | ((b45 >> 8) & 0xFFu);
    }
    if (tcp_s) seq0 = __builtin_bswap32(qle32(Q, vlo));
    h.ip_base = ip_base;
    h.l4_base = l4_base;
    h.tflags = tflags;
    h.id0 = id0;
    h.seq0 = seq0;
  };
  // the LDS copy of the head's results (every wave reads it after the barrier)
  auto head_publish = [&](const HeadRes& h) {
    if (lane == 0) {
      hd.clean = h.clean;
      hd.type = h.type;
      hd.ipv = h.ipv;
      hd.hdr_len = h.hdr_len;
      hd.gso = h.gso;
      hd.cs = h.cs;
      hd.co = h.co;
      hd.plen = h.plen;
      hd.ip_base = h.ip_base;
      hd.l4_base = h.l4_base;
      hd.tflags = h.tflags;
      hd.id0 = h.id0;
      hd.seq0 = h.seq0;
    }
    if (P > 1) {  // the head's Q (every row of the wave holds it; row 0 publishes)
      if (lane < 16) hd.q[lane] = h.Q;
    }
  };
  // The verdict and geometry, count / status (part 0) and, for a clean job,
  // the job-constant header sums.
  auto head = [&](const uint4 H0, const uint4 w) -> HeadRes {
    // the virtio header words become scalars only here, behind the bulk loads
    // (a wave-uniform load's value is otherwise moved into SGPRs at the load,
    // with a vmcnt(0) in front of every bulk load)
    uint4 wq = w;
    asm volatile("" : "+v"(wq.x), "+v"(wq.y), "+v"(wq.z), "+v"(wq.w));
    wq = make_uint4((uint32_t)ufl((int)wq.x), (uint32_t)ufl((int)wq.y), (uint32_t)ufl((int)wq.z),
                    (uint32_t)ufl((int)wq.w));
    uint32_t t1 = 0, hl = 0, g = 0, c = 0, o = 0, b0 = 0;
    if (jlen >= 14) {
      const uint64_t lo = ((uint64_t)wq.y << 32) | wq.x, hi = ((uint64_t)wq.w << 32) | wq.z;
      const uint64_t v0 = sh ? (lo >> (8 * sh)) | (hi << (64 - 8 * sh)) : lo;
      const uint64_t v1 = hi >> (8 * sh);
      t1 = (uint32_t)(v0 >> 8) & 0xFFu;
      hl = (uint32_t)(v0 >> 16) & 0xFFFFu;
      g = (uint32_t)(v0 >> 32) & 0xFFFFu;
      c = (uint32_t)(v0 >> 48) & 0xFFFFu;
      o = (uint32_t)v1 & 0xFFFFu;
      b0 = (uint32_t)(v1 >> 16) & 0xFFu;
    }
    const int plen_s = jlen > 10 ? (int)jlen - 10 : 0;
    const int type_s = raw ? ((t1 == GSO_TCPV4 || t1 == GSO_TCPV6) ? (int)t1 : GSO_UDP_L4) : (int)t1;
    const int ipv_s = raw ? ((job.flags & WGCS_GSO_JOB_V6) ? 6 : 4) : (int)(b0 >> 4);
    const bool tcp_s = type_s != GSO_UDP_L4;
    const bool ok_s = jlen >= 14 && g != 0 && (type_s == GSO_TCPV4 || type_s == GSO_TCPV6 || type_s == GSO_UDP_L4) &&
                      ((ipv_s == 4 && type_s != GSO_TCPV6) || (ipv_s == 6 && type_s != GSO_TCPV4));
    const int gso_s = (int)g, cs_s = (int)c, co_s = (int)o;
    const int hdr_s = (raw || tcp_s) ? (int)hl : ((cs_s + 8) & 0xFFFF);
    const int ca_s = (cs_s + co_s) & 0xFFFF;
    const int pkt0_s = hdr_s + min(gso_s, plen_s - hdr_s);
    const bool clean_s = ok_s && hdr_s < plen_s && cs_s >= (ipv_s == 4 ? 20 : 40) && ca_s + 2 <= hdr_s &&
                         hdr_s <= kMaxHdrLen && (raw || !tcp_s || (hdr_s - cs_s >= 20 && hdr_s - cs_s <= 60)) &&
                         fast_header(cs_s, hdr_s, ca_s, tcp_s) && (uint32_t)pkt0_s <= room;
    uint4 Q;
    {
      const uint32_t nx = row_next(H0.x);
      Q = make_uint4(__builtin_amdgcn_alignbyte(H0.y, H0.x, hph), __builtin_amdgcn_alignbyte(H0.z, H0.y, hph),
                     __builtin_amdgcn_alignbyte(H0.w, H0.z, hph), __builtin_amdgcn_alignbyte(nx, H0.w, hph));
    }
    bool clean = clean_s;
    if (clean && tcp_s && !raw) {  // the TCP data offset decides hdrLen (tun.go:601-614)
      const int th = (int)((qbyte(Q, cs_s + 12) >> 4) * 4);
      clean = ((cs_s + th) & 0xFFFF) == hdr_s;
    }
    if (ufl(clean ? 1 : 0)) {
      if (lane == 0 && part == 0) {  // the checks can only end in the segment count here (gso_rows_kernel)
        const int nfull_s = (plen_s - hdr_s + gso_s - 1) / gso_s;
        const bool many = nfull_s > (int)max_segs;
        count[jb] = many ? (int)max_segs - 1 : nfull_s;
        status[jb] = many ? WGCS_ERR_TOO_MANY_SEGMENTS : 0;
      }
    }
    HeadRes res = {clean ? 1 : 0, type_s, ipv_s, hdr_s, gso_s, cs_s, co_s, plen_s, 0u, 0u, 0u, 0u, 0u, Q};
    if (res.clean) head_sums(res);
    return res;
  };
  // the head's results from the LDS copy (after the barrier)
  auto head_from_lds = [&]() -> HeadRes {
    HeadRes h;
    h.clean = ufl(hd.clean);
    h.type = ufl(hd.type);
    h.ipv = ufl(hd.ipv);
    h.hdr_len = ufl(hd.hdr_len);
    h.gso = ufl(hd.gso);
    h.cs = ufl(hd.cs);
    h.co = ufl(hd.co);
    h.plen = ufl(hd.plen);
    h.ip_base = (uint32_t)ufl((int)hd.ip_base);
    h.l4_base = (uint32_t)ufl((int)hd.l4_base);
    h.tflags = (uint32_t)ufl((int)hd.tflags);
    h.id0 = (uint32_t)ufl((int)hd.id0);
    h.seq0 = (uint32_t)ufl((int)hd.seq0);
    h.Q = P > 1 ? hd.q[r] : make_uint4(0, 0, 0, 0);
    return h;
  };
  HeadIn hi = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  if (wv == 0) hi = head_loads();
  __builtin_amdgcn_sched_barrier(0);  // keep the header loads ahead of the bulk loads
  bulk_loads();
  if (wv == 0) head_publish(head(hi.H0, hi.w));
  // ---- every wave's bulk loads have landed (the compiler's own s_waitcnt,
  // not inline asm: its wait-count pass then knows no LDS-DMA is pending and
  // puts no vmcnt(0) -- which would also wait for the row's earlier stores --
  // in front of the image reads of the row loop); the barrier publishes the
  // image and the head
  __builtin_amdgcn_s_waitcnt(kVmcnt0);
  lds_barrier();
  const HeadRes hr = head_from_lds();
  if (ufl(hr.clean)) {
    const int type = ufl(hr.type), ipv = ufl(hr.ipv), hdr_len = ufl(hr.hdr_len), gso = ufl(hr.gso);
    const int cs = ufl(hr.cs), co = ufl(hr.co), plen = ufl(hr.plen);
    const uint32_t ip_base = (uint32_t)ufl((int)hr.ip_base), l4_base = (uint32_t)ufl((int)hr.l4_base);
    const uint32_t tflags = (uint32_t)ufl((int)hr.tflags), id0 = (uint32_t)ufl((int)hr.id0);
    const uint32_t seq0 = (uint32_t)ufl((int)hr.seq0);
    auto has_seg = [&](int i) { return i < (int)max_segs && hdr_len + (int64_t)i * gso < plen; };
    // readBuf[16r, 16r + 16): wave 0's LDS copy (P > 1), from the image, or
    // (a job too large for it) from HBM as gso_rows_kernel reads it
    uint4 Q;
    if (P > 1) {
      Q = hr.Q;
    } else if (use_img) {
      const int dq = ibias + 10 + 16 * r, s = dq & 3;
      const uint4 T = img16(img, dq - s);
      const uint32_t T4 = img4(img, dq - s + 16);
      Q = make_uint4(__builtin_amdgcn_alignbyte(T.y, T.x, s), __builtin_amdgcn_alignbyte(T.z, T.y, s),
                     __builtin_amdgcn_alignbyte(T.w, T.z, s), __builtin_amdgcn_alignbyte(T4, T.w, s));
    } else {
      const uint4 Hq = bld16<false>(hrs, 16 * r);
      const uint32_t nx = row_next(Hq.x);
      Q = make_uint4(__builtin_amdgcn_alignbyte(Hq.y, Hq.x, hph), __builtin_amdgcn_alignbyte(Hq.z, Hq.y, hph),
                     __builtin_amdgcn_alignbyte(Hq.w, Hq.z, hph), __builtin_amdgcn_alignbyte(nx, Hq.w, hph));
    }
    // write-through stores through a resource over the job's output region
    // when every row offset fits it (block-uniform; else plain stores)
    // (based at out + obase rounded down to 16 bytes: every row's dbase lies
    // at a non-negative 16-byte multiple from it)
    const bool wt = (uint64_t)max_segs * opitch + offset < 0x7FFF0000ull;
    uint8_t* const obase16 = out + obase - ((uintptr_t)(out + obase) & 15u);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(obase16, (short)0, 0x7FFFFFFF, 0x00020000);
    // this part's segments: payload start (job byte 10 + hdrLen + i gso) in
    // [part H, (part + 1) H)
    int i0 = 0, i1 = 0x7FFFFFFF;
    if (P > 1) {
      const int64_t a = (int64_t)part * H - 10 - hdr_len, b = a + H;
      // ceil(x / gso) in 32 bits where x fits (every read the image holds): a
      // 64-bit division is a long serial chain on this critical path
      auto cdiv = [&](int64_t x) -> int {
        if (x <= 0) return 0;
        if (x < 0x40000000) return (int)(((uint32_t)x + (uint32_t)gso - 1u) / (uint32_t)gso);
        return (int)min((x + gso - 1) / gso, (int64_t)0x7FFFFFFF);
      };
      i0 = cdiv(a);
      if (part < P - 1) i1 = cdiv(b);
    }
    const int lo_b = 16 * q_lo - ibias, hi_b = 16 * (q_lo + q_n) - ibias;  // staged job bytes
    for (int i = i0 + wv * 4 + (lane >> 4); i < i1 && has_seg(i); i += ROWS) {  // row-uniform
      uint8_t* dst = out + obase + (uint64_t)i * opitch + offset;
      const int dalign = (int)((uintptr_t)dst & 15u);
      uint8_t* dbase = dst - dalign;
      uint32_t acc = 0;
      bool in_img = use_img;
      if (P > 1 && in_img) {  // the row's payload windows staged, and every window it reads inside the image
        const RowSrc g = row_src(rb, i, gso, hdr_len, plen, dalign);
        in_img = g.lo - 18 >= lo_b && (g.hi + 20 <= hi_b || q_lo + q_n >= nch) &&
                 ib_p + g.aoff + 16 * ((g.nk + 16 * U - 1) / (16 * U) * 16 * U) + 4 <= kArr;
      }
      RowOut ro;
      ro.keep = make_uint4(0, 0, 0, 0);
      ro.rs = ors;
      ro.dro = (int)(dbase - obase16);
      ro.wt = wt;
      if (in_img) {
        stream_row_img<U>(img, ib_p, rb, i, gso, hdr_len, plen, dalign, dbase, r, acc, ro);
      } else {
        stream_row<U, NT>(rb, i, gso, hdr_len, plen, dalign, dbase, r, acc, job_rsrc(vb, jlen));
      }
      if (in_img)
        finish_row(true, Q, type, ipv, hdr_len, gso, cs, co, plen, i, r, dalign, dst, dbase, acc, ip_base, l4_base,
                   tflags, id0, seq0, &sizes[slot0 + (uint32_t)i], &ro);
      else
        finish_row(true, Q, type, ipv, hdr_len, gso, cs, co, plen, i, r, dalign, dst, dbase, acc, ip_base, l4_base,
                   tflags, id0, seq0, &sizes[slot0 + (uint32_t)i]);
    }
  } else if (part == 0) {
    // every other job: the decoded path, NW * 4 rows per group (the image's
    // loads have drained above, so no LDS-DMA write can land after the
    // workgroup retires)
    for (int grp = 0;; ++grp) {  // block-uniform
      const int i = grp * ROWS + wv * 4 + (lane >> 4);
      uint8_t* dst = out + obase + (uint64_t)i * opitch + offset;
      const int live = decoded_rows<U, NT>(vb, jlen, job.flags, room, max_segs, i, grp == 0, &count[jb], &status[jb],
                                           out + obase + offset, dst, &sizes[slot0], tails);
      lds_barrier();
      if ((int64_t)(grp + 1) * ROWS >= (int64_t)ufl(live)) break;
    }
  }
}

// WGCS_GSO_KERNEL=rows selects the round-4 grid (A/B builds and probes)
static int gso_use_rows() {
  static const int use_rows = [] {
    const char* e = getenv("WGCS_GSO_KERNEL");
    return e && e[0] == 'r' ? 1 : 0;
  }();
  return use_rows;
}

void gso_kernel_shape(int* lds_waves, int* parts, int* u, int* rows) {
  if (lds_waves) *lds_waves = WGCS_GSO_LDS_WAVES;
  if (parts) *parts = WGCS_GSO_PARTS;
  if (u) *u = WGCS_GSO_U;
  if (rows) *rows = gso_use_rows();
}

hipError_t launch_gso_split_batch(const uint8_t* arena, const wgcs_gso_job* jobs, uint32_t n_jobs, uint8_t* out,
                                  uint32_t out_stride, uint32_t offset, uint32_t max_segs, int32_t* sizes,
                                  int32_t* count, int32_t* status, hipStream_t s, const GsoOutPos* outpos,
                                  uint32_t room) {
  if (n_jobs == 0 || max_segs == 0) return hipSuccess;
  if (!outpos) room = out_stride > offset ? out_stride - offset : 0;
  const int use_rows = gso_use_rows();
  if (!use_rows) {
    constexpr int NW = WGCS_GSO_LDS_WAVES;
    constexpr int P = WGCS_GSO_PARTS;
    if (P == 1) {
      hipLaunchKernelGGL((gso_lds_kernel<NW, WGCS_GSO_U, true, 1>), dim3(n_jobs), dim3(NW * 64), 0, s, arena, jobs,
                         max_segs, out, out_stride, outpos, offset, room, sizes, count, status, n_jobs);
    } else {  // (n_jobs rounded up to 8) x P blocks
      // in 64 bits before the check (n_jobs + 7 wrapped in 32)
      const uint64_t nblk = ((uint64_t)n_jobs + 7u) / 8u * 8u * (uint64_t)P;
      if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
      hipLaunchKernelGGL((gso_lds_kernel<NW, WGCS_GSO_U, true, P>), dim3((uint32_t)nblk), dim3(NW * 64), 0,
                         s, arena, jobs, max_segs, out, out_stride, outpos, offset, room, sizes, count, status, n_jobs);
    }
    return hipGetLastError();
  }
  // 16 segments (4 waves) per block and group; a few blocks per job, each
  // looping over its groups (a 65,535-B read at MSS 1460 has 3 groups)
  const uint32_t ngroups = (max_segs + 15) / 16;
  const uint32_t gy = ngroups < (uint32_t)WGCS_GSO_GROUPS ? ngroups : (uint32_t)WGCS_GSO_GROUPS;
  hipLaunchKernelGGL((gso_rows_kernel<WGCS_GSO_U, true>), dim3(n_jobs, gy), dim3(256), 0, s, arena, jobs, max_segs, out,
                     out_stride, outpos, offset, room, sizes, count, status);
  return hipGetLastError();
}

}  // namespace wgcs
