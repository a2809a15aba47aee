// aead_kernels.hip -- batched ChaCha20-Poly1305 (RFC 8439, empty AAD) of
// WireGuard transport messages, in place on one arena:
//   SEAL  RoutineEncryption   device/send.go:438-463 (header, padding, Seal)
//   OPEN  RoutineDecryption   device/receive.go:363-383 (Open) and the length
//         trim of RoutineSendToInternet, :432-482
//
// Mapping.  One 16-lane DPP row per packet, one 16-byte chunk per lane per
// iteration, so a row moves 256 contiguous bytes per load / store instruction.
// Chunks are counted from the start of the ciphertext, wherever that lies in
// memory: loads and stores of whole chunks are 16-byte accesses at byte
// alignment, the ragged last chunk goes byte by byte, and no byte outside the
// packet is ever written.
//
// ChaCha20 runs "vertically": the four lanes of a quad hold one 64-byte block,
// lane j column j (state words j, 4+j, 8+j, 12+j).  A column round is a plain
// quarter round per lane; for the diagonal round b, c, d come from the lane
// 1, 2, 3 to the right (DPP quad_perm) and go back afterwards.  A 4x4 exchange
// inside the quad then hands lane j words 4j .. 4j+3, the keystream of its own
// chunk.  A row computes blocks 4 it + 1 .. 4 it + 4 in iteration it; block 0
// (the Poly1305 key) is computed by every quad before the loop.
//
// Poly1305 runs one block per lane per iteration, acc = acc * r^16 + m, and
// the 16 accumulators are combined with the powers r^1 .. r^16 at the end
// (wgcs_poly1305.h explains why that is exact).  The length block is simply
// the block after the last ciphertext block.
//
// Every loop bound derives from a descriptor len <= 65535; nothing here spins,
// waits on memory or stays resident.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wgcs_aead.h"
#include "wgcs_common.h"
#include "wgcs_kernels.h"
#include "wgcs_poly1305.h"

namespace wgcs {
namespace {

constexpr int kSeal = 0, kOpen = 1;
constexpr int kThreads = 256;  // 16 rows = 16 packets per workgroup

typedef unsigned int u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));

// 16 bytes at any byte address (gfx950 global accesses need no alignment).
__device__ __forceinline__ uint4 ld16_u(const uint8_t* p) {
  const u32x4a1 t = *reinterpret_cast<const u32x4a1*>(p);
  return make_uint4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void st16_u(uint8_t* p, const uint4& v) {
  u32x4a1 t;
  t.x = v.x, t.y = v.y, t.z = v.z, t.w = v.w;
  *reinterpret_cast<u32x4a1*>(p) = t;
}

// The first nb (< 16) bytes at p, the rest zero; and the matching store.
__device__ __forceinline__ uint4 ld_tail(const uint8_t* p, uint32_t nb) {
  uint64_t lo = 0, hi = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint64_t v = p[b];
    if (b < 8) lo |= v << (8 * b);
    else hi |= v << (8 * (b - 8));
  }
  return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
__device__ __forceinline__ void st_tail(uint8_t* p, const uint4& v, uint32_t nb) {
  const uint64_t lo = v.x | ((uint64_t)v.y << 32), hi = v.z | ((uint64_t)v.w << 32);
  for (uint32_t b = 0; b < nb; ++b) p[b] = (uint8_t)(b < 8 ? lo >> (8 * b) : hi >> (8 * (b - 8)));
}

// v with the bytes from index k (0..16) on cleared.
__device__ __forceinline__ uint4 keep_bytes(const uint4& v, uint32_t k) {
  const uint64_t lo = k >= 8 ? ~0ull : (1ull << (8 * k)) - 1;
  const uint64_t hi = k >= 16 ? ~0ull : k <= 8 ? 0ull : (1ull << (8 * (k - 8))) - 1;
  return make_uint4(v.x & (uint32_t)lo, v.y & (uint32_t)(lo >> 32), v.z & (uint32_t)hi, v.w & (uint32_t)(hi >> 32));
}

// DPP quad_perm: lane j of each quad reads lane (CTRL >> 2 j) & 3.
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
constexpr int kQuadRot1 = 0x39, kQuadRot2 = 0x4E, kQuadRot3 = 0x93;  // lane j reads lane j + 1, 2, 3 (mod 4)

// One of four values by a 2-bit index, on plain values (no private array).
__device__ __forceinline__ uint32_t sel4(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, int i) {
  const uint32_t lo = (i & 1) ? v1 : v0, hi = (i & 1) ? v3 : v2;
  return (i & 2) ? hi : lo;
}

__device__ __forceinline__ uint32_t rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

__device__ __forceinline__ void quarter_round(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  a += b; d ^= a; d = rotl(d, 16);
  c += d; b ^= c; b = rotl(b, 12);
  a += b; d ^= a; d = rotl(d, 8);
  c += d; b ^= c; b = rotl(b, 7);
}

// The ChaCha20 block function (RFC 8439 §2.3) on one column per lane: in and
// out, lane j of a quad holds state words j, 4+j, 8+j, 12+j in a, b, c, d.
__device__ __forceinline__ void chacha_block(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d) {
  const uint32_t a0 = a, b0 = b, c0 = c, d0 = d;
#pragma unroll 2
  for (int i = 0; i < 10; ++i) {
    quarter_round(a, b, c, d);  // columns
    b = quad_perm<kQuadRot1>(b);
    c = quad_perm<kQuadRot2>(c);
    d = quad_perm<kQuadRot3>(d);
    quarter_round(a, b, c, d);  // diagonals
    b = quad_perm<kQuadRot3>(b);
    c = quad_perm<kQuadRot2>(c);
    d = quad_perm<kQuadRot1>(d);
  }
  a += a0, b += b0, c += c0, d += d0;
}

// The 4x4 exchange: lane j holds o_i = word 4i + j and gets words 4j .. 4j+3.
// Word 4j + i is lane i's o_j.  For shift s every lane sends o[(own - s) & 3]
// and reads lane (own + s) & 3: reader j gets that lane's o_j, its word (j + s) & 3.
__device__ __forceinline__ uint4 quad_transpose(uint32_t o0, uint32_t o1, uint32_t o2, uint32_t o3, int j) {
  const uint32_t g0 = sel4(o0, o1, o2, o3, j);  // lane j keeps its own o[j] = word 4j + j
  const uint32_t g1 = quad_perm<kQuadRot1>(sel4(o0, o1, o2, o3, (j - 1) & 3));  // word 4j + (j + 1 & 3)
  const uint32_t g2 = quad_perm<kQuadRot2>(sel4(o0, o1, o2, o3, (j - 2) & 3));  // word 4j + (j + 2 & 3)
  const uint32_t g3 = quad_perm<kQuadRot3>(sel4(o0, o1, o2, o3, (j - 3) & 3));  // word 4j + (j + 3 & 3)
  // g_s is word (j + s) & 3 of the chunk: word i is g[(i - j) & 3]
  return make_uint4(sel4(g0, g1, g2, g3, (0 - j) & 3), sel4(g0, g1, g2, g3, (1 - j) & 3),
                    sel4(g0, g1, g2, g3, (2 - j) & 3), sel4(g0, g1, g2, g3, (3 - j) & 3));
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void aead_batch_kernel(uint8_t* __restrict__ arena,
                                                              const wgcs_aead_pkt* __restrict__ pkts,
                                                              const wgcs_aead_key* __restrict__ keys, uint32_t n_keys,
                                                              uint32_t n, uint32_t mtu, int32_t* __restrict__ out_len,
                                                              uint64_t* __restrict__ out_ctr) {
  const uint32_t row = blockIdx.x * (kThreads / 16) + (threadIdx.x >> 4);
  const int lane = threadIdx.x & 15, col = lane & 3, quad = lane >> 2;
  if (row >= n) return;  // whole rows leave: every DPP below sees full quads and rows
  const wgcs_aead_pkt pk = pkts[row];
  const uint32_t len = pk.len;
  int32_t bad = 0;
  if (len > kAeadMaxLen || (MODE == kOpen && len < kAeadHeader + kAeadTag)) bad = WGCS_ERR_OUT_OF_RANGE;
  else if (pk.key >= n_keys) bad = WGCS_ERR_INVALID_ARG;
  if (bad) {  // nothing of the packet is read or written
    if (lane == 0) {
      out_len[row] = bad;
      if (MODE == kOpen) out_ctr[row] = 0;
    }
    return;
  }
  uint8_t* const msg = arena + pk.off;
  uint8_t* const ct = msg + kAeadHeader;
  const wgcs_aead_key* const key = keys + pk.key;
  uint32_t ctlen;
  uint64_t ctr;
  if (MODE == kSeal) {
    ctlen = len + aead_padding(len, mtu);
    ctr = pk.counter;
    // header: LE32 type 4 | LE32 receiver index | LE64 counter (send.go:440-446), byte `lane` by lane `lane`
    const uint32_t hw = sel4(4u, key->remote_index, (uint32_t)ctr, (uint32_t)(ctr >> 32), quad);
    msg[lane] = (uint8_t)(hw >> (8 * col));
  } else {
    ctlen = len - (kAeadHeader + kAeadTag);
    uint32_t lo = 0, hi = 0;  // the counter field, bytes [8, 16) (receive.go:369)
    for (int b = 0; b < 4; ++b) {
      lo |= (uint32_t)msg[8 + b] << (8 * b);
      hi |= (uint32_t)msg[12 + b] << (8 * b);
    }
    ctr = lo | ((uint64_t)hi << 32);
  }

  // this lane's column of the initial state; word 12 is the block counter,
  // words 13..15 the nonce: four zero bytes, then the LE64 counter
  const uint32_t* const kw = reinterpret_cast<const uint32_t*>(key->key);
  const uint32_t st_a = sel4(0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, col);
  const uint32_t st_b = kw[col], st_c = kw[4 + col];
  const uint32_t st_d = col == 2 ? (uint32_t)ctr : col == 3 ? (uint32_t)(ctr >> 32) : 0u;

  // block 0: r = words 0..3 (lanes' a), s = words 4..7 (lanes' b) -- RFC 8439 §2.6
  uint32_t a = st_a, b = st_b, c = st_c, d = st_d;
  chacha_block(a, b, c, d);
  const P1305 r = p1305_clamp_r(quad_perm<0x00>(a), quad_perm<0x55>(a), quad_perm<0xAA>(a), quad_perm<0xFF>(a));
  const uint32_t s0 = quad_perm<0x00>(b), s1 = quad_perm<0x55>(b), s2 = quad_perm<0xAA>(b), s3 = quad_perm<0xFF>(b);

  const uint32_t nct = (ctlen + 15) >> 4;  // ciphertext blocks; block nct is the length block
  const uint32_t nblk = nct + 1;
  P1305 r16;
  const P1305 rpow = p1305_pow_1_16(r, p1305_lane_exponent(nblk, lane), &r16);
  P1305 acc = p1305_zero();
  uint32_t f0 = 0, f1 = 0;  // OPEN, lane 0: plaintext bytes 0..7

  const uint32_t iters = (nblk + 15) >> 4;
  for (uint32_t it = 0; it < iters; ++it) {
    const uint32_t blk = it * 16 + lane;
    uint4 ks = make_uint4(0, 0, 0, 0);
    if (it * 16 < nct) {  // uniform in the row
      a = st_a, b = st_b, c = st_c, d = col == 0 ? it * 4 + quad + 1 : st_d;
      chacha_block(a, b, c, d);
      ks = quad_transpose(a, b, c, d, col);
    }
    P1305 m;
    if (blk < nct) {
      const uint32_t pos = blk * 16;
      uint8_t* const p = ct + pos;
      const uint32_t nb = ctlen - pos < 16 ? ctlen - pos : 16;
      uint4 in = nb == 16 ? ld16_u(p) : ld_tail(p, nb);
      // SEAL: bytes from len on are the zero padding, whatever the buffer held (send.go:451)
      if (MODE == kSeal && pos + 16 > len) in = keep_bytes(in, len > pos ? len - pos : 0);
      uint4 out = make_uint4(in.x ^ ks.x, in.y ^ ks.y, in.z ^ ks.z, in.w ^ ks.w);
      if (nb == 16) {
        st16_u(p, out);
      } else {
        out = keep_bytes(out, nb);
        st_tail(p, out, nb);
      }
      const uint4 mac = MODE == kSeal ? out : in;  // the MAC is over the ciphertext
      // pad16(ct): a ragged last chunk is MACed zero-filled as a whole block (RFC 8439 §2.8),
      // not as a short Poly1305 block with its 0x01 byte at the true length
      m = p1305_from_words(mac.x, mac.y, mac.z, mac.w, 1);
      if (MODE == kOpen && blk == 0) f0 = out.x, f1 = out.y;
    } else {
      m = p1305_from_words(0, 0, ctlen, 0, 1);  // LE64(len(aad) = 0) | LE64(len(ct))
    }
    if (blk <= nct) acc = p1305_add(p1305_mul(acc, r16), m);
  }

  P1305 h = p1305_mul(acc, rpow);
#pragma unroll
  for (int i = 0; i < 5; ++i) h.l[i] = row16_sum_u32(h.l[i]);  // 16 carried limbs: < 2^31
  uint32_t tag[4];
  p1305_finish(h, s0, s1, s2, s3, tag);
  const uint32_t tag_byte = (sel4(tag[0], tag[1], tag[2], tag[3], quad) >> (8 * col)) & 0xFFu;
  uint8_t* const tp = ct + ctlen;
  if (MODE == kSeal) {
    tp[lane] = (uint8_t)tag_byte;
    if (lane == 0) out_len[row] = (int32_t)(kAeadHeader + ctlen + kAeadTag);
    return;
  }
  const uint32_t diff = row16_sum_u32(tag_byte ^ tp[lane]);
  int32_t res;
  if (diff != 0) {
    // what Open leaves of its output on failure: zeros; header and tag stay
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (uint32_t blk = lane; blk < nct; blk += 16) {
      const uint32_t pos = blk * 16;
      if (ctlen - pos >= 16) st16_u(ct + pos, z);
      else st_tail(ct + pos, z, ctlen - pos);
    }
    res = WGCS_ERR_AUTH;
  } else {
    res = aead_trim(ctlen, f0 & 0xFFu, (f0 >> 16) & 0xFFu, f0 >> 24, f1 & 0xFFu, (f1 >> 8) & 0xFFu);
  }
  if (lane == 0) {
    out_len[row] = res;
    out_ctr[row] = ctr;
  }
}

}  // namespace

hipError_t launch_aead_batch(int open, uint8_t* arena, const wgcs_aead_pkt* pkts, const wgcs_aead_key* keys,
                             uint32_t n_keys, uint32_t n, uint32_t mtu, int32_t* out_len, uint64_t* out_ctr,
                             hipStream_t s) {
  const uint32_t blocks = (n + kThreads / 16 - 1) / (kThreads / 16);
  if (open)
    hipLaunchKernelGGL(aead_batch_kernel<kOpen>, dim3(blocks), dim3(kThreads), 0, s, arena, pkts, keys, n_keys, n, 0u,
                       out_len, out_ctr);
  else
    hipLaunchKernelGGL(aead_batch_kernel<kSeal>, dim3(blocks), dim3(kThreads), 0, s, arena, pkts, keys, n_keys, n,
                       mtu, out_len, out_ctr);
  return hipGetLastError();
}

}  // namespace wgcs
