// wgcs_poly1305.h -- Poly1305 (RFC 8439 §2.5) limb arithmetic, shared by the
// gfx950 AEAD kernel (aead_kernels.hip) and a host test program
// (tests/aead_host/poly1305_host.cpp) that drives the very same functions.
//
// Numbers mod p = 2^130 - 5 are five 26-bit limbs in uint32_t, value
// sum(l[i] << 26 i).  A "loose" number has limbs < 2^28: a carried result has
// limbs < 2^26 except limb 1, which may exceed that by the last carry
// (< 2^11), and adding a message block adds < 2^26 per limb.  p1305_mul takes
// two loose numbers: every product is < 2^28 * 5 * 2^28 < 2^59 and a column
// sums five of them, < 2^62, so the uint64_t columns cannot overflow.
//
// Row-parallel Horner.  The MAC of blocks m_0 .. m_{N-1} is
//   h = sum_k m_k r^(N-k)  (mod p).
// A 16-lane row gives block k to lane k & 15; each lane runs
//   acc = acc * r^16 + m_k
// over its own blocks, so after the loop lane l holds
//   sum_j m_{l+16j} r^(16 (n_l - 1 - j)),
// n_l its number of blocks.  Its last block k_last = l + 16 (n_l - 1) still
// lacks the factor r^(N - k_last), which is p1305_lane_exponent(N, l) in
// [1, 16].  Multiplying by it and adding the 16 lanes gives exactly the sum
// above: this is a regrouping of a polynomial in r over the field Z/p, and
// every step is exact modular arithmetic, so the tag is bit-identical to the
// serial form.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WGCS_HD __host__ __device__ __forceinline__
#else
#define WGCS_HD inline
#endif

namespace wgcs {

struct P1305 {
  uint32_t l[5];
};

constexpr uint32_t kP1305Mask = 0x3FFFFFFu;

WGCS_HD P1305 p1305_zero() { return P1305{{0, 0, 0, 0, 0}}; }
WGCS_HD P1305 p1305_one() { return P1305{{1, 0, 0, 0, 0}}; }

// The 128-bit little-endian number t3:t2:t1:t0 plus hibit << 128, as limbs.
WGCS_HD P1305 p1305_from_words(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t hibit) {
  P1305 m;
  m.l[0] = t0 & kP1305Mask;
  m.l[1] = ((t0 >> 26) | (t1 << 6)) & kP1305Mask;
  m.l[2] = ((t1 >> 20) | (t2 << 12)) & kP1305Mask;
  m.l[3] = ((t2 >> 14) | (t3 << 18)) & kP1305Mask;
  m.l[4] = (t3 >> 8) | (hibit << 24);
  return m;
}

// r of the one-time key: the clamp of RFC 8439 §2.5.1, then limbs.
WGCS_HD P1305 p1305_clamp_r(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
  return p1305_from_words(t0 & 0x0FFFFFFFu, t1 & 0x0FFFFFFCu, t2 & 0x0FFFFFFCu, t3 & 0x0FFFFFFCu, 0);
}

// One message block of n bytes (1..16) given as words whose bytes >= n are
// zero: the 0x01 byte goes at its true length (§2.5.1: "add one bit beyond
// the number of octets").  This is plain Poly1305; the AEAD MACs pad16(ct),
// where every block is whole, so the kernel builds its blocks with
// p1305_from_words(.., 1) and only the host program uses this one.
WGCS_HD P1305 p1305_block(uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, int n) {
  if (n >= 16) return p1305_from_words(t0, t1, t2, t3, 1);
  const uint32_t one = 1u << (8 * (n & 3));
  const int w = n >> 2;
  if (w == 0) t0 |= one;
  if (w == 1) t1 |= one;
  if (w == 2) t2 |= one;
  if (w == 3) t3 |= one;
  return p1305_from_words(t0, t1, t2, t3, 0);
}

WGCS_HD P1305 p1305_add(const P1305& a, const P1305& b) {
  return P1305{{a.l[0] + b.l[0], a.l[1] + b.l[1], a.l[2] + b.l[2], a.l[3] + b.l[3], a.l[4] + b.l[4]}};
}

// a * b mod p for loose a, b; the result is carried: limbs 0, 2, 3, 4 < 2^26,
// limb 1 < 2^26 + 2^11.
WGCS_HD P1305 p1305_mul(const P1305& a, const P1305& b) {
  const uint64_t a0 = a.l[0], a1 = a.l[1], a2 = a.l[2], a3 = a.l[3], a4 = a.l[4];
  const uint64_t b0 = b.l[0], b1 = b.l[1], b2 = b.l[2], b3 = b.l[3], b4 = b.l[4];
  const uint64_t s1 = b1 * 5, s2 = b2 * 5, s3 = b3 * 5, s4 = b4 * 5;  // 2^130 = 5 (mod p)
  uint64_t d0 = a0 * b0 + a1 * s4 + a2 * s3 + a3 * s2 + a4 * s1;
  uint64_t d1 = a0 * b1 + a1 * b0 + a2 * s4 + a3 * s3 + a4 * s2;
  uint64_t d2 = a0 * b2 + a1 * b1 + a2 * b0 + a3 * s4 + a4 * s3;
  uint64_t d3 = a0 * b3 + a1 * b2 + a2 * b1 + a3 * b0 + a4 * s4;
  uint64_t d4 = a0 * b4 + a1 * b3 + a2 * b2 + a3 * b1 + a4 * b0;
  P1305 h;
  d1 += d0 >> 26;
  d2 += d1 >> 26;
  d3 += d2 >> 26;
  d4 += d3 >> 26;
  const uint64_t c = (d0 & kP1305Mask) + (d4 >> 26) * 5;  // < 2^26 + 5 * 2^34
  h.l[0] = (uint32_t)(c & kP1305Mask);
  h.l[1] = (uint32_t)((d1 & kP1305Mask) + (c >> 26));
  h.l[2] = (uint32_t)(d2 & kP1305Mask);
  h.l[3] = (uint32_t)(d3 & kP1305Mask);
  h.l[4] = (uint32_t)(d4 & kP1305Mask);
  return h;
}

// One carry pass over limbs of any size below 2^32 (value unchanged mod p).
WGCS_HD P1305 p1305_carry(const P1305& a) {
  P1305 h = a;
  uint32_t c;
  c = h.l[0] >> 26; h.l[0] &= kP1305Mask; h.l[1] += c;
  c = h.l[1] >> 26; h.l[1] &= kP1305Mask; h.l[2] += c;
  c = h.l[2] >> 26; h.l[2] &= kP1305Mask; h.l[3] += c;
  c = h.l[3] >> 26; h.l[3] &= kP1305Mask; h.l[4] += c;
  c = h.l[4] >> 26; h.l[4] &= kP1305Mask; h.l[0] += c * 5;
  return h;
}

// r^e for e in [1, 16], and r^16 in *r16 (square and multiply; four squarings).
WGCS_HD P1305 p1305_pow_1_16(const P1305& r, int e, P1305* r16) {
  P1305 p = r, res = p1305_one();
  for (int b = 0; b < 4; ++b) {
    if ((e >> b) & 1) res = p1305_mul(res, p);
    p = p1305_mul(p, p);
  }
  *r16 = p;
  return (e & 15) ? res : p;
}

// The exponent lane `lane` of a 16-lane row still owes after its last block
// when the row splits n_blocks blocks round-robin (see the file comment).
WGCS_HD int p1305_lane_exponent(uint32_t n_blocks, int lane) {
  return (int)((((n_blocks - 1u) & 15u) - (uint32_t)lane) & 15u) + 1;
}

// tag = ((h mod p) + s) mod 2^128 as four little-endian words, for h with
// limbs of any size below 2^31.
WGCS_HD void p1305_finish(const P1305& acc, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t tag[4]) {
  // two wrapping passes leave the value below 2^130 + 2^27; the straight pass
  // then makes limbs 0..3 canonical (h4 may keep one excess bit, value < 2 p)
  P1305 h = p1305_carry(p1305_carry(acc));
  uint32_t c;
  c = h.l[0] >> 26; h.l[0] &= kP1305Mask; h.l[1] += c;
  c = h.l[1] >> 26; h.l[1] &= kP1305Mask; h.l[2] += c;
  c = h.l[2] >> 26; h.l[2] &= kP1305Mask; h.l[3] += c;
  c = h.l[3] >> 26; h.l[3] &= kP1305Mask; h.l[4] += c;
  // g = h - p = h + 5 - 2^130; keep it iff it did not borrow
  uint32_t g0 = h.l[0] + 5;
  c = g0 >> 26; g0 &= kP1305Mask;
  uint32_t g1 = h.l[1] + c;
  c = g1 >> 26; g1 &= kP1305Mask;
  uint32_t g2 = h.l[2] + c;
  c = g2 >> 26; g2 &= kP1305Mask;
  uint32_t g3 = h.l[3] + c;
  c = g3 >> 26; g3 &= kP1305Mask;
  const uint32_t g4 = h.l[4] + c - (1u << 26);
  const uint32_t take_g = (g4 >> 31) - 1u;  // all ones iff h >= p
  const uint32_t h0 = (h.l[0] & ~take_g) | (g0 & take_g), h1 = (h.l[1] & ~take_g) | (g1 & take_g);
  const uint32_t h2 = (h.l[2] & ~take_g) | (g2 & take_g), h3 = (h.l[3] & ~take_g) | (g3 & take_g);
  const uint32_t h4 = (h.l[4] & ~take_g) | (g4 & take_g);
  // 26-bit limbs -> 32-bit words (mod 2^128), then + s
  const uint32_t w0 = h0 | (h1 << 26), w1 = (h1 >> 6) | (h2 << 20), w2 = (h2 >> 12) | (h3 << 14);
  const uint32_t w3 = (h3 >> 18) | (h4 << 8);
  uint64_t f = (uint64_t)w0 + s0;
  tag[0] = (uint32_t)f;
  f = (uint64_t)w1 + s1 + (f >> 32);
  tag[1] = (uint32_t)f;
  f = (uint64_t)w2 + s2 + (f >> 32);
  tag[2] = (uint32_t)f;
  f = (uint64_t)w3 + s3 + (f >> 32);
  tag[3] = (uint32_t)f;
}

}  // namespace wgcs
