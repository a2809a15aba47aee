// ring_kernels.hip -- the resident per-call ring's kernel (ring_kernel,
// launch_ring; host side ring.cpp).  It runs a virtio read through
// gso_device.h's gso_rows_body, compiled here with WGCS_RING_TU: every load of
// request bytes is a system-scope one (wgcs_copy.h: ld16 / ldg8 relaxed
// atomics, buffer loads sc0 sc1), since the kernel stays resident while the
// host rewrites the same buffers between requests and a plain load may hit
// the CU's L1 copy of the last request.  The macro decides load scope only;
// the batch kernels live in gso_kernels.hip.
#define WGCS_RING_TU 1
#include "gso_device.h"

namespace wgcs {

// ---------------------------------------------------------------------------
// The resident per-call ring (round 6).  A launch plus a
// completion wait costs ~20 us per Go call, more than the Go
// code of one Tun.Read.  ring_kernel stays resident on a few CUs instead:
// wave 0 of every workgroup polls the request record in coherent pinned host
// memory -- seq-tagged 16-byte chunks (word 0 of each is the request's
// number), three system-scope 16-byte loads per lane and poll, two polls in
// flight, s_sleep between them -- and takes a request once every chunk it
// needs carries the same new seq (an untorn record, and an inline packet or
// virtio header with it).  The workgroups run the request -- checksumValid of
// one packet (workgroup 0's first wave) or one handleVirtioRead
// (gso_rows_body: workgroup b takes segment groups b, b + nb, ...) -- reading
// the request bytes from coherent host memory and writing the results there;
// then each workgroup releases its stores at system scope and stores
// {seq, valid} in one 8-byte write-through store on its own line of the
// control block, which the host spins on.  Every wave leaves the loop on the
// stop word or when no request came for `idle_ticks` of s_memrealtime
// (100 MHz), so no launch can outlive its use.

typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));

// checksumValid(pkt, iphLen, proto, isV6) (gro.go:554-612) by one wave: the
// batch kernel's VALIDATE arithmetic (checksum_kernels.hip) over every chunk
// with byte masks -- the main range pkt[iphLen:len] paired from iphLen, the
// pseudo-header addresses paired from their own start (rotl8 when the two
// parities differ) -- then proto + (len - iphLen).  Loads are system-scope
// (sc0 sc1) buffer loads: the bytes change between requests at one address.
__device__ uint32_t ring_validate(const uint8_t* pkt, int len, int cs, int proto, bool v6) {
  const int lane = threadIdx.x & 63;
  const int main_lo = min(cs, len), main_hi = len;
  const int addr_lo = v6 ? 8 : 12, addr_hi = v6 ? 40 : 20;
  const uintptr_t pbase = (uintptr_t)pkt;
  const bool rot_addr = (((pbase + (uintptr_t)addr_lo) ^ (pbase + (uintptr_t)main_lo)) & 1u) != 0;
  const int lo_all = min(main_lo, addr_lo), hi_all = max(main_hi, addr_hi);
  const int rel0 = lo_all - (int)((pbase + (uintptr_t)lo_all) & 15u);
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(pkt + rel0), (short)0,
                                                                      hi_all - rel0, 0x00020000);
  uint32_t acc = 0;
  for (int c = lane; rel0 + 16 * c < hi_all; c += 64) {
    const int pos = rel0 + 16 * c;
    const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * c, 0, 17);
    const uint32_t w[4] = {t[0], t[1], t[2], t[3]};
    const uint32_t m16 = byte_bits16(main_lo - pos, main_hi - pos);
    const uint32_t a16 = byte_bits16(addr_lo - pos, addr_hi - pos);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      acc = add_halves(acc, w[k] & expand_nibble((m16 >> (4 * k)) & 0xFu));
      uint32_t y = w[k] & expand_nibble((a16 >> (4 * k)) & 0xFu);
      if (rot_addr) y = rotl8(y);
      acc = add_halves(acc, y);
    }
    acc = (acc >> 16) + (acc & 0xFFFFu);
  }
  uint32_t s = fold32_16(wave_sum_u32(fold32_16(acc)));
  if (((pbase + (uintptr_t)main_lo) & 1u) == 0) s = bswap16(s);
  const uint32_t t = fold32_16(s + (uint32_t)proto + ((uint32_t)(len - cs) & 0xFFFFu));
  return (t == 0xFFFFu && cs <= len) ? 1u : 0u;
}

// checksumValid of an inline request from the poll's registers: lane l of
// load j holds chunk 64 j + l, i.e. payload bytes [12 p, 12 p + 12) for
// p = 64 j + l - 8 >= 0 in its words 1-3 (word 0 is seq).  Every word starts
// at an offset that is a multiple of 4, so the 16-bit pairing is the
// packet's own; bytes past what the host wrote are masked off (main range
// [iphLen, len), addresses within the bytes carried).
__device__ uint32_t ring_validate_inline(const u32x4s (&x)[3], int len, int cs, int proto, bool v6) {
  const int lane = threadIdx.x & 63;
  const int main_lo = min(cs, len), main_hi = len;
  const int addr_lo = v6 ? 8 : 12, addr_hi = v6 ? 40 : 20;
  const bool rot_addr = ((addr_lo ^ main_lo) & 1) != 0;
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int p = 64 * j + lane - 8;
    if (p >= 0) {
#pragma unroll
      for (int m = 1; m < 4; ++m) {
        const int b0 = 12 * p + 4 * (m - 1);
        const uint32_t w = x[j][m];
        acc = add_halves(acc, w & expand_nibble(byte_bits16(main_lo - b0, main_hi - b0) & 0xFu));
        uint32_t y = w & expand_nibble(byte_bits16(addr_lo - b0, addr_hi - b0) & 0xFu);
        if (rot_addr) y = rotl8(y);
        acc = add_halves(acc, y);
      }
    }
  }
  uint32_t s = fold32_16(wave_sum_u32(fold32_16(acc)));
  if ((main_lo & 1) == 0) s = bswap16(s);
  const uint32_t t = fold32_16(s + (uint32_t)proto + ((uint32_t)(len - cs) & 0xFFFFu));
  return (t == 0xFFFFu && cs <= len) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void ring_kernel(RingCtl* ctl, uint32_t last0, uint64_t idle_ticks) {
  __shared__ uint32_t s_q, s_valid;
  __shared__ uint32_t s_w[32];  // the request record's words
  __shared__ __attribute__((aligned(16))) uint32_t s_hdr[3 * kRingHdrChunks];  // a virtio read's first bytes
  RingReq* const rq = &ctl->req;
  uint32_t last = last0;
  uint64_t t_last = __builtin_amdgcn_s_memrealtime();
  for (;;) {
    if (threadIdx.x < 64) {
      // wave 0 polls the record and the inline payload after it with three
      // system-scope 16-B loads per lane (chunk 64 j + lane) per poll, so the
      // request's fields -- and an inline packet -- arrive with its number:
      // one PCIe round trip, not one per field
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(rq, (short)0, (int)(16 * kRingPollChunks),
                                                                          0x00020000);
      const int lane = threadIdx.x;
      uint32_t q = 0;
      // 0: keep polling; 1: a new untorn record (and payload); 2: stop / idle deadline
      auto check = [&](const u32x4s (&x)[3]) -> int {
        q = (uint32_t)__builtin_amdgcn_readlane((int)x[0][0], 0);
        if (__builtin_amdgcn_readlane((int)x[0][kRqStop & 3], 0) != 0) return 2;
        // all eight chunks carry the same new seq: an untorn record
        const bool same = __builtin_amdgcn_ballot_w64(lane < 8 && x[0][0] != q) == 0;
        if (q != last && same) {
          const uint32_t op = (uint32_t)__builtin_amdgcn_readlane((int)x[0][kRqOp & 3], kRqOp >> 2);
          const uint32_t nin =
              (blockIdx.x == 0 && op == kRingOpChecksumInline)
                  ? (uint32_t)__builtin_amdgcn_readlane((int)x[0][kRqInl & 3], kRqInl >> 2)
              : op == kRingOpVirtioRead ? (uint32_t)__builtin_amdgcn_readlane((int)x[0][kRqHdrInl & 3], kRqHdrInl >> 2)
                                        : 0u;
          if (nin != 0) {
            // ... and every payload chunk the request carries
            const int nch = ((int)nin + 11) / 12;
            const bool torn = (lane >= 8 && lane - 8 < nch && x[0][0] != q) || (56 + lane < nch && x[1][0] != q) ||
                              (120 + lane < nch && x[2][0] != q);
            if (__builtin_amdgcn_ballot_w64(torn) != 0) return 0;
          }
          return 1;
        }
        if (__builtin_amdgcn_s_memrealtime() - t_last > idle_ticks) return 2;
        return 0;
      };
      // workgroup 0 reads the inline payload too; the others need only the
      // record and a virtio read's inline header (chunks < 64): their loads
      // 1-2 point past the record and return zeros without a memory access
      const int o1 = blockIdx.x == 0 ? 16 * (64 + lane) : 0x7FFFFFF0;
      const int o2 = blockIdx.x == 0 ? 16 * (128 + lane) : 0x7FFFFFF0;
      auto poll = [&](u32x4s (&x)[3]) {
        x[0] = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * lane, 0, 17);  // sc0 sc1
        x[1] = __builtin_amdgcn_raw_buffer_load_b128(rs, o1, 0, 17);
        x[2] = __builtin_amdgcn_raw_buffer_load_b128(rs, o2, 0, 17);
      };
      // two polls in flight, issued half a round trip apart: a posted request
      // is seen ~RTT/4 sooner on average than with one poll at a time
      u32x4s va[3], vb[3], v[3];
      poll(va);
      int st;
      for (;;) {
        __builtin_amdgcn_s_sleep(1);
        poll(vb);
        if ((st = check(va)) != 0) {
#pragma unroll
          for (int j = 0; j < 3; ++j) v[j] = va[j];
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        poll(va);
        if ((st = check(vb)) != 0) {
#pragma unroll
          for (int j = 0; j < 3; ++j) v[j] = vb[j];
          break;
        }
      }
      if (st == 2) q = 0xFFFFFFFFu;
      if (lane < 8) {
        s_w[4 * lane] = v[0][0];
        s_w[4 * lane + 1] = v[0][1];
        s_w[4 * lane + 2] = v[0][2];
        s_w[4 * lane + 3] = v[0][3];
      }
      // a virtio read's inline header bytes into LDS (zeros past them): word
      // 3p + m - 1 = chunk p's word m, the buffer's phase mod 16 kept
      if (st == 1 && (uint32_t)__builtin_amdgcn_readlane((int)v[0][kRqOp & 3], kRqOp >> 2) == kRingOpVirtioRead) {
        const int nch = ((int)__builtin_amdgcn_readlane((int)v[0][kRqHdrInl & 3], kRqHdrInl >> 2) + 11) / 12;
        const int p = lane - 8;
        if (p >= 0 && p < (int)kRingHdrChunks) {
          s_hdr[3 * p] = p < nch ? v[0][1] : 0u;
          s_hdr[3 * p + 1] = p < nch ? v[0][2] : 0u;
          s_hdr[3 * p + 2] = p < nch ? v[0][3] : 0u;
        }
      }
      uint32_t iv = 0;
      if (st == 1 && blockIdx.x == 0 &&
          (uint32_t)__builtin_amdgcn_readlane((int)v[0][kRqOp & 3], kRqOp >> 2) == kRingOpChecksumInline) {
        auto f = [&](uint32_t k) { return __builtin_amdgcn_readlane((int)v[0][k & 3], (int)(k >> 2)); };
        iv = ring_validate_inline(v, f(kRqLen), f(kRqCs), f(kRqProto), (f(kRqFlags) & WGCS_PKT_V6) != 0);
      }
      if (lane == 0) {
        s_q = q;
        s_valid = iv;
      }
    }
    __syncthreads();
    const uint32_t q = s_q;
    if (q == 0xFFFFFFFFu) break;  // block-uniform: every wave leaves
    auto w = [&](uint32_t k) { return (uint32_t)ufl((int)s_w[k]); };
    auto p64 = [&](uint32_t lo, uint32_t hi) { return (uint64_t)w(lo) | ((uint64_t)w(hi) << 32); };
    // request pointers as global-address-space ones: the inlined body then
    // emits global_load / global_store, not flat (which also waits on lgkmcnt)
    typedef __attribute__((address_space(1))) uint8_t g8;
    auto gptr = [&](uint32_t lo, uint32_t hi) { return (uint8_t*)(g8*)(uintptr_t)p64(lo, hi); };
    const uint32_t op = w(kRqOp);
    uint32_t valid = 0;
    if (op == kRingOpChecksumInline) {
      valid = s_valid;  // workgroup 0's wave 0 checked it from the poll's registers
    } else if (op == kRingOpChecksumValid) {
      if (blockIdx.x == 0 && threadIdx.x < 64)
        valid = ring_validate(gptr(kRqPktLo, kRqPktHi), (int)w(kRqLen),
                              (int)w(kRqCs), (int)w(kRqProto), (w(kRqFlags) & WGCS_PKT_V6) != 0);
    } else if (op == kRingOpVirtioRead) {
      const wgcs_gso_job job = {0, w(kRqVlen), w(kRqJflags)};
      const GsoOutPos pos = {0, w(kRqPitch), w(kRqPosFlags)};
      int32_t* h = (int32_t*)(__attribute__((address_space(1))) int32_t*)(uintptr_t)p64(kRqMetaLo, kRqMetaHi);
      const uint32_t kb = w(kRqKbufs);
      const uint8_t* vb = gptr(kRqVbufLo, kRqVbufHi);
      // the inline header: vb[k] at LDS byte (vb & 15) + k
      const uint8_t* hl = w(kRqHdrInl) ? reinterpret_cast<const uint8_t*>(s_hdr) + ((uintptr_t)vb & 15u) : nullptr;
      gso_rows_body<WGCS_GSO_U, false, 4 * kRingWaves>(vb, job, 0, (int)blockIdx.x, (int)gridDim.x, kb,
                                                         gptr(kRqOutLo, kRqOutHi), 0, true, pos, 0, w(kRqRoom), h,
                                                         h + kb, h + kb + 1, hl);
    }
    // completion: every wave's stores done; a request that stored results
    // releases them at system scope (the fence's own wait made explicit:
    // MI355X_MICROARCH.md); then {seq, valid} in ONE 8-byte write-through
    // store on this workgroup's own line, which the host spins on
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      if (op == kRingOpVirtioRead) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      const __amdgpu_buffer_rsrc_t ds = __builtin_amdgcn_make_buffer_rsrc(&ctl->dn[blockIdx.x], (short)0, 64,
                                                                          0x00020000);
      const u32x2 w = {q, valid};
      __builtin_amdgcn_raw_buffer_store_b64(w, ds, 0, 0, 17);  // sc0 sc1
    }
    last = q;
    t_last = __builtin_amdgcn_s_memrealtime();
  }
  if (threadIdx.x == 0)
    __hip_atomic_fetch_add(&ctl->dn[blockIdx.x].exited, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_ring(RingCtl* ctl, uint32_t nb, uint32_t last, uint64_t idle_ticks, hipStream_t s) {
  if (nb == 0 || nb > kRingMaxBlocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ring_kernel, dim3(nb), dim3(64 * kRingWaves), 0, s, ctl, last, idle_ticks);
  return hipGetLastError();
}

}  // namespace wgcs
