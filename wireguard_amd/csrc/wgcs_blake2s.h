// wgcs_blake2s.h -- BLAKE2s (RFC 7693), shared by the gfx950 handshake screen
// (cookie_kernels.hip), the host functions of cookie_api.cpp and a host test
// program (tests/cookie_host/cookie_host.cpp) that drives the very same code.
//
// One lane hashes one short message: the chaining value, the work vector and
// the sixteen message words are all named by constants -- the ten rounds are
// written out with the sigma schedule of §2.7 as literal indices -- so on the
// device nothing is indexed at run time and everything stays in registers.
//
// A key is given as eight little-endian words, zero-padded (its block is
// those words and eight zero words, §3.3), so a key that was just computed --
// the cookie that keys MAC2 -- never goes through memory.  The message is a
// pointer at any byte alignment.  Host code reads it by byte loads and never
// outside its length; the device reads the aligned dwords that hold it
// (b2s_load_block), so the memory around a message on the device must be
// readable to the next 4-byte boundary on either side.
//
// The last-block rule of §3.3: the final block is the one that holds the last
// byte, so a message of a whole number of blocks ends with a full final block
// and no empty one follows; only the unkeyed hash of nothing compresses an
// empty block, and the keyed hash of nothing compresses the key block alone as
// final.  Counters stay below 2^32 (messages here are a few hundred bytes).
#pragma once

#include <stdint.h>

#include "wgcs_poly1305.h"  // WGCS_HD

namespace wgcs {

WGCS_HD uint32_t b2s_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// Bytes [at, at + 4) of base[0, len) as a little-endian word, zero where they lie at or past
// len.  No byte outside base[0, len) is read: an index past the end is clamped to the last
// byte and its value dropped, so the four loads stand without a branch around them and a
// lane has all the loads of a block in flight at once.  len == 0 reads nothing (base may be NULL).
WGCS_HD uint32_t b2s_load_le32(const uint8_t* base, uint32_t at, uint32_t len) {
  if (len == 0) return 0;
  const uint32_t last = len - 1;
  uint32_t w = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = at + k;
    const uint32_t byte = base[i < last ? i : last];
    w |= (i < len ? byte : 0u) << (8 * k);
  }
  return w;
}

#if defined(__HIP_DEVICE_COMPILE__)
// The device's form of sixteen such words, bytes [at, at + 64) of base[0, len) with at < len:
// seventeen aligned dword loads and a funnel shift by the pointer's low bits, in place of
// sixty-four byte loads.  A wave's lanes read messages a pitch apart, so every load
// instruction costs the L1 one line per lane whatever its width: a quarter of the
// instructions is a quarter of that.  It reads whole aligned dwords, so up to three bytes
// before base + at and after base + len - 1, inside the dwords that hold the message's first
// and last byte and nowhere else (the index is clamped to the last of them); the bytes past
// len are masked off.  Host code keeps the byte loads: there a buffer may end with the message.
__device__ __forceinline__ void b2s_load_block(const uint8_t* base, uint32_t at, uint32_t len, uint32_t m[16]) {
  const uint8_t* const p = base + at;
  const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t* const w = (const uint32_t*)(p - sh);  // pointer arithmetic: the loads stay global loads
  const uint32_t avail = len - at;               // >= 1
  const uint32_t last = (sh + avail - 1u) >> 2;  // the dword that holds the message's last byte
  uint32_t d[17];
#pragma unroll
  for (uint32_t i = 0; i < 17; ++i) d[i] = w[i < last ? i : last];
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    const uint32_t x = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
    const int32_t have = (int32_t)avail - (int32_t)(4 * i);  // bytes of this word inside the message
    m[i] = have >= 4 ? x : have <= 0 ? 0u : x & ((1u << (8 * have)) - 1u);
  }
}
#endif

WGCS_HD void b2s_store_le32(uint8_t* p, uint32_t w) {
  p[0] = (uint8_t)w;
  p[1] = (uint8_t)(w >> 8);
  p[2] = (uint8_t)(w >> 16);
  p[3] = (uint8_t)(w >> 24);
}

#define WGCS_B2S_G(a, b, c, d, x, y) \
  a = a + b + (x);                   \
  d = b2s_rotr(d ^ a, 16);           \
  c = c + d;                         \
  b = b2s_rotr(b ^ c, 12);           \
  a = a + b + (y);                   \
  d = b2s_rotr(d ^ a, 8);            \
  c = c + d;                         \
  b = b2s_rotr(b ^ c, 7);

// one round: the columns, then the diagonals, with the round's row of sigma
#define WGCS_B2S_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
  WGCS_B2S_G(v0, v4, v8, v12, m[s0], m[s1])                                                  \
  WGCS_B2S_G(v1, v5, v9, v13, m[s2], m[s3])                                                  \
  WGCS_B2S_G(v2, v6, v10, v14, m[s4], m[s5])                                                 \
  WGCS_B2S_G(v3, v7, v11, v15, m[s6], m[s7])                                                 \
  WGCS_B2S_G(v0, v5, v10, v15, m[s8], m[s9])                                                 \
  WGCS_B2S_G(v1, v6, v11, v12, m[s10], m[s11])                                               \
  WGCS_B2S_G(v2, v7, v8, v13, m[s12], m[s13])                                                \
  WGCS_B2S_G(v3, v4, v9, v14, m[s14], m[s15])

constexpr uint32_t kB2sIv0 = 0x6A09E667u, kB2sIv1 = 0xBB67AE85u, kB2sIv2 = 0x3C6EF372u, kB2sIv3 = 0xA54FF53Au;
constexpr uint32_t kB2sIv4 = 0x510E527Fu, kB2sIv5 = 0x9B05688Cu, kB2sIv6 = 0x1F83D9ABu, kB2sIv7 = 0x5BE0CD19u;

// The compression function F of §3.2 on h, for the block m whose last byte is
// byte t of the input (t < 2^32); last: this is the final block.
WGCS_HD void blake2s_compress(uint32_t h[8], const uint32_t m[16], uint32_t t, bool last) {
  uint32_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
  uint32_t v8 = kB2sIv0, v9 = kB2sIv1, v10 = kB2sIv2, v11 = kB2sIv3;
  uint32_t v12 = kB2sIv4 ^ t, v13 = kB2sIv5, v14 = last ? ~kB2sIv6 : kB2sIv6, v15 = kB2sIv7;
  WGCS_B2S_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  WGCS_B2S_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  WGCS_B2S_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  WGCS_B2S_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  WGCS_B2S_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  WGCS_B2S_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  WGCS_B2S_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  WGCS_B2S_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  WGCS_B2S_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  WGCS_B2S_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
  h[0] ^= v0 ^ v8;
  h[1] ^= v1 ^ v9;
  h[2] ^= v2 ^ v10;
  h[3] ^= v3 ^ v11;
  h[4] ^= v4 ^ v12;
  h[5] ^= v5 ^ v13;
  h[6] ^= v6 ^ v14;
  h[7] ^= v7 ^ v15;
}

#undef WGCS_B2S_ROUND
#undef WGCS_B2S_G

// BLAKE2s of msg[0, len) with digest length out_len (16 or 32) under a key of
// key_len bytes (0: unkeyed, 16 or 32) given as zero-padded words.  h receives
// the whole chaining value; the digest is its first out_len bytes.  One loop,
// one compression per trip: trip 0 of a keyed hash takes the key block.
WGCS_HD void blake2s_words(const uint32_t key[8], uint32_t key_len, const uint8_t* msg, uint32_t len, uint32_t out_len,
                           uint32_t h[8]) {
  h[0] = kB2sIv0 ^ 0x01010000u ^ (key_len << 8) ^ out_len;  // §2.5: fanout 1, depth 1
  h[1] = kB2sIv1;
  h[2] = kB2sIv2;
  h[3] = kB2sIv3;
  h[4] = kB2sIv4;
  h[5] = kB2sIv5;
  h[6] = kB2sIv6;
  h[7] = kB2sIv7;
  const uint32_t key_bytes = key_len ? 64u : 0u;
  const uint32_t total = key_bytes + len;
  const uint32_t n_blocks = total ? (total + 63u) / 64u : 1u;
  for (uint32_t b = 0; b < n_blocks; ++b) {
    uint32_t m[16];
    if (key_len && b == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) m[i] = key[i];
#pragma unroll
      for (int i = 8; i < 16; ++i) m[i] = 0;
    } else {
      const uint32_t at = b * 64u - key_bytes;
#if defined(__HIP_DEVICE_COMPILE__)
      if (at < len) {
        b2s_load_block(msg, at, len, m);
      } else {  // only the unkeyed hash of nothing gets here
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i] = 0;
      }
#else
#pragma unroll
      for (uint32_t i = 0; i < 16; ++i) m[i] = b2s_load_le32(msg, at + 4 * i, len);
#endif
    }
    const bool last = b + 1 == n_blocks;
    blake2s_compress(h, m, last ? total : (b + 1) * 64u, last);
  }
}

// a key of key_len <= 32 bytes (any alignment) as zero-padded words
WGCS_HD void b2s_key_words(const uint8_t* key, uint32_t key_len, uint32_t w[8]) {
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) w[i] = b2s_load_le32(key, 4 * i, key_len);
}

// the same on bytes: out receives out_len (16 or 32) bytes
WGCS_HD void blake2s_bytes(const uint8_t* key, uint32_t key_len, const uint8_t* msg, uint32_t len, uint32_t out_len,
                           uint8_t* out) {
  uint32_t kw[8], h[8];
  b2s_key_words(key, key_len, kw);
  blake2s_words(kw, key_len, msg, len, out_len, h);
#pragma unroll
  for (int i = 0; i < 4; ++i) b2s_store_le32(out + 4 * i, h[i]);
  if (out_len > 16) {
#pragma unroll
    for (int i = 4; i < 8; ++i) b2s_store_le32(out + 4 * i, h[i]);
  }
}

// hmac.Equal on 16 bytes held as words: an OR of XORs over all of them, no early exit
WGCS_HD bool tag16_equal(const uint32_t a[4], const uint32_t b[4]) {
  return ((a[0] ^ b[0]) | (a[1] ^ b[1]) | (a[2] ^ b[2]) | (a[3] ^ b[3])) == 0;
}

}  // namespace wgcs
