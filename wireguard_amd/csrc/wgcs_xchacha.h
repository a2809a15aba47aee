// wgcs_xchacha.h -- HChaCha20 and the XChaCha20-Poly1305 seal / open
// (draft-irtf-cfrg-xchacha-03 over RFC 8439) of exactly what a cookie reply
// carries: 16 bytes of plaintext with 16 bytes of additional data
// (device/cookie.go:235-241, :326-332).  A scalar form that one lane can run;
// shared by cookie_kernels.hip, cookie_api.cpp and
// tests/cookie_host/cookie_host.cpp.  Poly1305 is wgcs_poly1305.h's.
//
// Everything is little-endian words: the key is 8, the 24-byte nonce 6, and
// plaintext, ciphertext, additional data and tag are 4 each.  The subkey is
// HChaCha20(key, nonce[0:16]); the AEAD of RFC 8439 §2.8 follows under it with
// the nonce 00 00 00 00 | nonce[16:24].  With both inputs one whole block the
// MAC runs over three blocks: the additional data, the ciphertext, and the two
// lengths LE64(16) | LE64(16).
#pragma once

#include <stdint.h>

#include "wgcs_poly1305.h"

namespace wgcs {

WGCS_HD uint32_t chacha_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

#define WGCS_CHACHA_QR(a, b, c, d) \
  a += b;                          \
  d = chacha_rotl(d ^ a, 16);      \
  c += d;                          \
  b = chacha_rotl(b ^ c, 12);      \
  a += b;                          \
  d = chacha_rotl(d ^ a, 8);       \
  c += d;                          \
  b = chacha_rotl(b ^ c, 7);

// the 20 rounds of RFC 8439 §2.3 on x, without the final addition
WGCS_HD void chacha20_rounds(uint32_t x[16]) {
  uint32_t x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], x4 = x[4], x5 = x[5], x6 = x[6], x7 = x[7];
  uint32_t x8 = x[8], x9 = x[9], x10 = x[10], x11 = x[11], x12 = x[12], x13 = x[13], x14 = x[14], x15 = x[15];
  for (int i = 0; i < 10; ++i) {
    WGCS_CHACHA_QR(x0, x4, x8, x12)
    WGCS_CHACHA_QR(x1, x5, x9, x13)
    WGCS_CHACHA_QR(x2, x6, x10, x14)
    WGCS_CHACHA_QR(x3, x7, x11, x15)
    WGCS_CHACHA_QR(x0, x5, x10, x15)
    WGCS_CHACHA_QR(x1, x6, x11, x12)
    WGCS_CHACHA_QR(x2, x7, x8, x13)
    WGCS_CHACHA_QR(x3, x4, x9, x14)
  }
  x[0] = x0; x[1] = x1; x[2] = x2; x[3] = x3; x[4] = x4; x[5] = x5; x[6] = x6; x[7] = x7;
  x[8] = x8; x[9] = x9; x[10] = x10; x[11] = x11; x[12] = x12; x[13] = x13; x[14] = x14; x[15] = x15;
}

#undef WGCS_CHACHA_QR

WGCS_HD void chacha20_init(uint32_t x[16], const uint32_t key[8], uint32_t w12, uint32_t w13, uint32_t w14,
                           uint32_t w15) {
  x[0] = 0x61707865u;  // "expand 32-byte k"
  x[1] = 0x3320646eu;
  x[2] = 0x79622d32u;
  x[3] = 0x6b206574u;
#pragma unroll
  for (int i = 0; i < 8; ++i) x[4 + i] = key[i];
  x[12] = w12;
  x[13] = w13;
  x[14] = w14;
  x[15] = w15;
}

// HChaCha20 (draft §2.2): the first and last rows of the permuted state
WGCS_HD void hchacha20(const uint32_t key[8], const uint32_t nonce[4], uint32_t out[8]) {
  uint32_t x[16];
  chacha20_init(x, key, nonce[0], nonce[1], nonce[2], nonce[3]);
  chacha20_rounds(x);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    out[i] = x[i];
    out[4 + i] = x[12 + i];
  }
}

// the first eight words of ChaCha20 block `counter` under key and the nonce 0 | n1 | n2
WGCS_HD void chacha20_block_head(const uint32_t key[8], uint32_t counter, uint32_t n1, uint32_t n2, uint32_t out[8]) {
  uint32_t x[16];
  chacha20_init(x, key, counter, 0, n1, n2);
  chacha20_rounds(x);
  out[0] = x[0] + 0x61707865u;
  out[1] = x[1] + 0x3320646eu;
  out[2] = x[2] + 0x79622d32u;
  out[3] = x[3] + 0x6b206574u;
#pragma unroll
  for (int i = 4; i < 8; ++i) out[i] = x[i] + key[i - 4];
}

// The tag over ad | ct | LE64(16) | LE64(16) with the one-time key otk
// (r = otk[0:4], s = otk[4:8]), RFC 8439 §2.8.
WGCS_HD void xchacha_tag16(const uint32_t otk[8], const uint32_t ad[4], const uint32_t ct[4], uint32_t tag[4]) {
  const P1305 r = p1305_clamp_r(otk[0], otk[1], otk[2], otk[3]);
  P1305 h = p1305_mul(p1305_from_words(ad[0], ad[1], ad[2], ad[3], 1), r);
  h = p1305_mul(p1305_add(h, p1305_from_words(ct[0], ct[1], ct[2], ct[3], 1)), r);
  h = p1305_mul(p1305_add(h, p1305_from_words(16, 0, 16, 0, 1)), r);
  p1305_finish(h, otk[4], otk[5], otk[6], otk[7], tag);
}

// The one-time key and the 16 keystream bytes of the AEAD under key and the 24-byte nonce.
WGCS_HD void xchacha_streams16(const uint32_t key[8], const uint32_t nonce[6], uint32_t otk[8], uint32_t ks[4]) {
  uint32_t sub[8], b1[8];
  hchacha20(key, nonce, sub);
  chacha20_block_head(sub, 0, nonce[4], nonce[5], otk);
  chacha20_block_head(sub, 1, nonce[4], nonce[5], b1);
#pragma unroll
  for (int i = 0; i < 4; ++i) ks[i] = b1[i];
}

// xchapoly.Seal(dst, nonce, pt, ad) for 16-byte pt and ad: ct and tag.
WGCS_HD void xchacha_seal16(const uint32_t key[8], const uint32_t nonce[6], const uint32_t pt[4], const uint32_t ad[4],
                            uint32_t ct[4], uint32_t tag[4]) {
  uint32_t otk[8], ks[4];
  xchacha_streams16(key, nonce, otk, ks);
#pragma unroll
  for (int i = 0; i < 4; ++i) ct[i] = pt[i] ^ ks[i];
  xchacha_tag16(otk, ad, ct, tag);
}

// xchapoly.Open: true and the plaintext when the tag matches (an OR of XORs
// over all 16 bytes); pt is written either way and means nothing on false.
WGCS_HD bool xchacha_open16(const uint32_t key[8], const uint32_t nonce[6], const uint32_t ct[4], const uint32_t tag[4],
                            const uint32_t ad[4], uint32_t pt[4]) {
  uint32_t otk[8], ks[4], want[4];
  xchacha_streams16(key, nonce, otk, ks);
  xchacha_tag16(otk, ad, ct, want);
#pragma unroll
  for (int i = 0; i < 4; ++i) pt[i] = ct[i] ^ ks[i];
  return ((want[0] ^ tag[0]) | (want[1] ^ tag[1]) | (want[2] ^ tag[2]) | (want[3] ^ tag[3])) == 0;
}

}  // namespace wgcs
