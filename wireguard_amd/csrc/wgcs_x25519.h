// wgcs_x25519.h -- X25519 (RFC 7748 §5) as golang.org/x/crypto/curve25519.X25519
// behaves (device/noise_helpers.go:93-105), shared by the gfx950 kernels of
// noise_kernels.hip, the host functions of noise.cpp and a host test program
// (tests/noise_host/noise_host.cpp) that drives the very same code.
//
// One lane runs one scalar multiplication.  A number mod p = 2^255 - 19 is ten
// limbs in uint32_t, 26 and 25 bits in turn (limb i starts at bit ceil(25.5 i):
// 0, 26, 51, 77, 102, 128, 153, 179, 204, 230), each a named member, so on the
// device nothing is indexed at run time and a field element is ten registers.
// Products are 32 x 32 -> 64 bits and a column is a chain of ten
// multiply-adds into one 64-bit accumulator, which is v_mad_u64_u32 on gfx950.
//
// Bounds.  A "carried" element (what fe_mul, fe_sq and fe_mul_a24 return) has
// every limb below its nominal 2^26 / 2^25 except limb 1 < 2^25 + 2^17.
// fe_add of two carried elements has limbs < 2^27 + 2^18; fe_sub adds 2 p limb
// by limb before it subtracts, so of two carried elements it has even limbs
// < 2^26 + 2^27 and odd limbs < 2^25 + 2^17 + 2^26, and never borrows.  fe_mul
// and fe_sq take any such "loose" element (even limbs < 3 * 2^26, odd limbs
// < 3 * 2^25 + 2^17):
//   19 * (3 * 2^26) and 38 * (3 * 2^25 + 2^17) are below 2^32, so the
//   premultiplied limbs stay in 32 bits; a product is at most
//   (2 * 3 * 2^26) * (19 * 3 * 2^26) < 2^60.5 and a column sums ten of them,
//   < 2^64, so the uint64_t columns cannot overflow.
// The ladder only ever adds or subtracts carried elements, and multiplies what
// comes of it.
//
// No branch and no index depends on the scalar or on a field element: the
// ladder's conditional swap is a mask, the scalar's bits come off the top of a
// 256-bit shift register, and the inversion is the fixed addition chain for
// p - 2.  The only data-dependent result is the caller's test of the output
// for zero ("low order point"), which the reference makes too.
#pragma once

#include <stdint.h>

#include "wgcs_poly1305.h"  // WGCS_HD

namespace wgcs {

struct Fe25519 {
  uint32_t v0, v1, v2, v3, v4, v5, v6, v7, v8, v9;
};

constexpr uint32_t kFeMask26 = 0x3FFFFFFu, kFeMask25 = 0x1FFFFFFu;

WGCS_HD Fe25519 fe_zero() { return Fe25519{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }
WGCS_HD Fe25519 fe_one() { return Fe25519{1, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }

// The 255-bit little-endian number w[7] : .. : w[0] with bit 255 ignored (RFC 7748 §5: "mask the
// most significant bit in the final byte").  A value in [p, 2^255) is taken as it is: the
// arithmetic reduces it.
WGCS_HD Fe25519 fe_from_words(const uint32_t w[8]) {
  Fe25519 f;
  f.v0 = w[0] & kFeMask26;                              // bits   0 ..  25
  f.v1 = ((w[0] >> 26) | (w[1] << 6)) & kFeMask25;      // bits  26 ..  50
  f.v2 = ((w[1] >> 19) | (w[2] << 13)) & kFeMask26;     // bits  51 ..  76
  f.v3 = ((w[2] >> 13) | (w[3] << 19)) & kFeMask25;     // bits  77 .. 101
  f.v4 = (w[3] >> 6) & kFeMask26;                       // bits 102 .. 127
  f.v5 = w[4] & kFeMask25;                              // bits 128 .. 152
  f.v6 = ((w[4] >> 25) | (w[5] << 7)) & kFeMask26;      // bits 153 .. 178
  f.v7 = ((w[5] >> 19) | (w[6] << 13)) & kFeMask25;     // bits 179 .. 203
  f.v8 = ((w[6] >> 12) | (w[7] << 20)) & kFeMask26;     // bits 204 .. 229
  f.v9 = (w[7] >> 6) & kFeMask25;                       // bits 230 .. 254
  return f;
}

WGCS_HD Fe25519 fe_add(const Fe25519& a, const Fe25519& b) {
  return Fe25519{a.v0 + b.v0, a.v1 + b.v1, a.v2 + b.v2, a.v3 + b.v3, a.v4 + b.v4,
                 a.v5 + b.v5, a.v6 + b.v6, a.v7 + b.v7, a.v8 + b.v8, a.v9 + b.v9};
}

// a - b + 2 p for carried b (see the bounds above)
WGCS_HD Fe25519 fe_sub(const Fe25519& a, const Fe25519& b) {
  return Fe25519{a.v0 + 0x7FFFFDAu - b.v0, a.v1 + 0x3FFFFFEu - b.v1, a.v2 + 0x7FFFFFEu - b.v2,
                 a.v3 + 0x3FFFFFEu - b.v3, a.v4 + 0x7FFFFFEu - b.v4, a.v5 + 0x3FFFFFEu - b.v5,
                 a.v6 + 0x7FFFFFEu - b.v6, a.v7 + 0x3FFFFFEu - b.v7, a.v8 + 0x7FFFFFEu - b.v8,
                 a.v9 + 0x3FFFFFEu - b.v9};
}

// the ten columns h0 .. h9 (any size below 2^63) as a carried element: one pass up, the
// carry out of limb 9 times 19 into limb 0 (2^255 = 19 mod p), and that limb's carry into limb 1
#define WGCS_FE_CARRY_COLUMNS(r)                  \
  h1 += h0 >> 26;                                 \
  h2 += h1 >> 25;                                 \
  h3 += h2 >> 26;                                 \
  h4 += h3 >> 25;                                 \
  h5 += h4 >> 26;                                 \
  h6 += h5 >> 25;                                 \
  h7 += h6 >> 26;                                 \
  h8 += h7 >> 25;                                 \
  h9 += h8 >> 26;                                 \
  const uint64_t c0 = (h0 & kFeMask26) + (h9 >> 25) * 19; /* < 2^26 + 19 * 2^39 */ \
  r.v0 = (uint32_t)(c0 & kFeMask26);              \
  r.v1 = (uint32_t)((h1 & kFeMask25) + (c0 >> 26)); /* < 2^25 + 2^17 */ \
  r.v2 = (uint32_t)(h2 & kFeMask26);              \
  r.v3 = (uint32_t)(h3 & kFeMask25);              \
  r.v4 = (uint32_t)(h4 & kFeMask26);              \
  r.v5 = (uint32_t)(h5 & kFeMask25);              \
  r.v6 = (uint32_t)(h6 & kFeMask26);              \
  r.v7 = (uint32_t)(h7 & kFeMask25);              \
  r.v8 = (uint32_t)(h8 & kFeMask26);              \
  r.v9 = (uint32_t)(h9 & kFeMask25);

// f * g mod p for loose f, g; carried.  Limb i times limb j lands on bit ceil(25.5 i) +
// ceil(25.5 j), one above column i + j's when both are odd (the factor 2), and a column past
// the ninth wraps with 19.
WGCS_HD Fe25519 fe_mul(const Fe25519& f, const Fe25519& g) {
  const uint32_t f0 = f.v0, f1 = f.v1, f2 = f.v2, f3 = f.v3, f4 = f.v4, f5 = f.v5, f6 = f.v6, f7 = f.v7, f8 = f.v8,
                 f9 = f.v9;
  const uint32_t g0 = g.v0, g1 = g.v1, g2 = g.v2, g3 = g.v3, g4 = g.v4, g5 = g.v5, g6 = g.v6, g7 = g.v7, g8 = g.v8,
                 g9 = g.v9;
  const uint32_t g1_19 = 19 * g1, g2_19 = 19 * g2, g3_19 = 19 * g3, g4_19 = 19 * g4, g5_19 = 19 * g5, g6_19 = 19 * g6,
                 g7_19 = 19 * g7, g8_19 = 19 * g8, g9_19 = 19 * g9;
  const uint32_t f1_2 = 2 * f1, f3_2 = 2 * f3, f5_2 = 2 * f5, f7_2 = 2 * f7, f9_2 = 2 * f9;
  uint64_t h0 = (uint64_t)f0 * g0 + (uint64_t)f1_2 * g9_19 + (uint64_t)f2 * g8_19 + (uint64_t)f3_2 * g7_19 +
                (uint64_t)f4 * g6_19 + (uint64_t)f5_2 * g5_19 + (uint64_t)f6 * g4_19 + (uint64_t)f7_2 * g3_19 +
                (uint64_t)f8 * g2_19 + (uint64_t)f9_2 * g1_19;
  uint64_t h1 = (uint64_t)f0 * g1 + (uint64_t)f1 * g0 + (uint64_t)f2 * g9_19 + (uint64_t)f3 * g8_19 +
                (uint64_t)f4 * g7_19 + (uint64_t)f5 * g6_19 + (uint64_t)f6 * g5_19 + (uint64_t)f7 * g4_19 +
                (uint64_t)f8 * g3_19 + (uint64_t)f9 * g2_19;
  uint64_t h2 = (uint64_t)f0 * g2 + (uint64_t)f1_2 * g1 + (uint64_t)f2 * g0 + (uint64_t)f3_2 * g9_19 +
                (uint64_t)f4 * g8_19 + (uint64_t)f5_2 * g7_19 + (uint64_t)f6 * g6_19 + (uint64_t)f7_2 * g5_19 +
                (uint64_t)f8 * g4_19 + (uint64_t)f9_2 * g3_19;
  uint64_t h3 = (uint64_t)f0 * g3 + (uint64_t)f1 * g2 + (uint64_t)f2 * g1 + (uint64_t)f3 * g0 +
                (uint64_t)f4 * g9_19 + (uint64_t)f5 * g8_19 + (uint64_t)f6 * g7_19 + (uint64_t)f7 * g6_19 +
                (uint64_t)f8 * g5_19 + (uint64_t)f9 * g4_19;
  uint64_t h4 = (uint64_t)f0 * g4 + (uint64_t)f1_2 * g3 + (uint64_t)f2 * g2 + (uint64_t)f3_2 * g1 +
                (uint64_t)f4 * g0 + (uint64_t)f5_2 * g9_19 + (uint64_t)f6 * g8_19 + (uint64_t)f7_2 * g7_19 +
                (uint64_t)f8 * g6_19 + (uint64_t)f9_2 * g5_19;
  uint64_t h5 = (uint64_t)f0 * g5 + (uint64_t)f1 * g4 + (uint64_t)f2 * g3 + (uint64_t)f3 * g2 +
                (uint64_t)f4 * g1 + (uint64_t)f5 * g0 + (uint64_t)f6 * g9_19 + (uint64_t)f7 * g8_19 +
                (uint64_t)f8 * g7_19 + (uint64_t)f9 * g6_19;
  uint64_t h6 = (uint64_t)f0 * g6 + (uint64_t)f1_2 * g5 + (uint64_t)f2 * g4 + (uint64_t)f3_2 * g3 +
                (uint64_t)f4 * g2 + (uint64_t)f5_2 * g1 + (uint64_t)f6 * g0 + (uint64_t)f7_2 * g9_19 +
                (uint64_t)f8 * g8_19 + (uint64_t)f9_2 * g7_19;
  uint64_t h7 = (uint64_t)f0 * g7 + (uint64_t)f1 * g6 + (uint64_t)f2 * g5 + (uint64_t)f3 * g4 +
                (uint64_t)f4 * g3 + (uint64_t)f5 * g2 + (uint64_t)f6 * g1 + (uint64_t)f7 * g0 +
                (uint64_t)f8 * g9_19 + (uint64_t)f9 * g8_19;
  uint64_t h8 = (uint64_t)f0 * g8 + (uint64_t)f1_2 * g7 + (uint64_t)f2 * g6 + (uint64_t)f3_2 * g5 +
                (uint64_t)f4 * g4 + (uint64_t)f5_2 * g3 + (uint64_t)f6 * g2 + (uint64_t)f7_2 * g1 +
                (uint64_t)f8 * g0 + (uint64_t)f9_2 * g9_19;
  uint64_t h9 = (uint64_t)f0 * g9 + (uint64_t)f1 * g8 + (uint64_t)f2 * g7 + (uint64_t)f3 * g6 +
                (uint64_t)f4 * g5 + (uint64_t)f5 * g4 + (uint64_t)f6 * g3 + (uint64_t)f7 * g2 +
                (uint64_t)f8 * g1 + (uint64_t)f9 * g0;
  Fe25519 r;
  WGCS_FE_CARRY_COLUMNS(r)
  return r;
}

// f * f mod p for loose f; carried.  The columns of fe_mul with equal products taken once.
WGCS_HD Fe25519 fe_sq(const Fe25519& f) {
  const uint32_t f0 = f.v0, f1 = f.v1, f2 = f.v2, f3 = f.v3, f4 = f.v4, f5 = f.v5, f6 = f.v6, f7 = f.v7, f8 = f.v8,
                 f9 = f.v9;
  const uint32_t f0_2 = 2 * f0, f1_2 = 2 * f1, f2_2 = 2 * f2, f3_2 = 2 * f3, f4_2 = 2 * f4, f5_2 = 2 * f5,
                 f6_2 = 2 * f6, f7_2 = 2 * f7;
  const uint32_t f5_38 = 38 * f5, f6_19 = 19 * f6, f7_38 = 38 * f7, f8_19 = 19 * f8, f9_38 = 38 * f9;
  uint64_t h0 = (uint64_t)f0 * f0 + (uint64_t)f1_2 * f9_38 + (uint64_t)f2_2 * f8_19 + (uint64_t)f3_2 * f7_38 +
                (uint64_t)f4_2 * f6_19 + (uint64_t)f5 * f5_38;
  uint64_t h1 = (uint64_t)f0_2 * f1 + (uint64_t)f2 * f9_38 + (uint64_t)f3_2 * f8_19 + (uint64_t)f4 * f7_38 +
                (uint64_t)f5_2 * f6_19;
  uint64_t h2 = (uint64_t)f0_2 * f2 + (uint64_t)f1_2 * f1 + (uint64_t)f3_2 * f9_38 + (uint64_t)f4_2 * f8_19 +
                (uint64_t)f5_2 * f7_38 + (uint64_t)f6 * f6_19;
  uint64_t h3 = (uint64_t)f0_2 * f3 + (uint64_t)f1_2 * f2 + (uint64_t)f4 * f9_38 + (uint64_t)f5_2 * f8_19 +
                (uint64_t)f6 * f7_38;
  uint64_t h4 = (uint64_t)f0_2 * f4 + (uint64_t)f1_2 * f3_2 + (uint64_t)f2 * f2 + (uint64_t)f5_2 * f9_38 +
                (uint64_t)f6_2 * f8_19 + (uint64_t)f7 * f7_38;
  uint64_t h5 = (uint64_t)f0_2 * f5 + (uint64_t)f1_2 * f4 + (uint64_t)f2_2 * f3 + (uint64_t)f6 * f9_38 +
                (uint64_t)f7_2 * f8_19;
  uint64_t h6 = (uint64_t)f0_2 * f6 + (uint64_t)f1_2 * f5_2 + (uint64_t)f2_2 * f4 + (uint64_t)f3_2 * f3 +
                (uint64_t)f7_2 * f9_38 + (uint64_t)f8 * f8_19;
  uint64_t h7 = (uint64_t)f0_2 * f7 + (uint64_t)f1_2 * f6 + (uint64_t)f2_2 * f5 + (uint64_t)f3_2 * f4 +
                (uint64_t)f8 * f9_38;
  uint64_t h8 = (uint64_t)f0_2 * f8 + (uint64_t)f1_2 * f7_2 + (uint64_t)f2_2 * f6 + (uint64_t)f3_2 * f5_2 +
                (uint64_t)f4 * f4 + (uint64_t)f9 * f9_38;
  uint64_t h9 = (uint64_t)f0_2 * f9 + (uint64_t)f1_2 * f8 + (uint64_t)f2_2 * f7 + (uint64_t)f3_2 * f6 +
                (uint64_t)f4_2 * f5;
  Fe25519 r;
  WGCS_FE_CARRY_COLUMNS(r)
  return r;
}

// 121665 f mod p = a24 f of RFC 7748 §5, (486662 - 2) / 4, for loose f; carried
WGCS_HD Fe25519 fe_mul_a24(const Fe25519& f) {
  uint64_t h0 = (uint64_t)f.v0 * 121665u, h1 = (uint64_t)f.v1 * 121665u, h2 = (uint64_t)f.v2 * 121665u;
  uint64_t h3 = (uint64_t)f.v3 * 121665u, h4 = (uint64_t)f.v4 * 121665u, h5 = (uint64_t)f.v5 * 121665u;
  uint64_t h6 = (uint64_t)f.v6 * 121665u, h7 = (uint64_t)f.v7 * 121665u, h8 = (uint64_t)f.v8 * 121665u;
  uint64_t h9 = (uint64_t)f.v9 * 121665u;
  Fe25519 r;
  WGCS_FE_CARRY_COLUMNS(r)
  return r;
}

#undef WGCS_FE_CARRY_COLUMNS

// f^(2^n), n >= 1
WGCS_HD Fe25519 fe_sq_n(Fe25519 f, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < n; ++i) f = fe_sq(f);
  return f;
}

// z^(p - 2) = z^(2^255 - 21) by the fixed chain: 254 squarings and 11 multiplications
WGCS_HD Fe25519 fe_invert(const Fe25519& z) {
  const Fe25519 z2 = fe_sq(z);                                // 2
  const Fe25519 z9 = fe_mul(fe_sq_n(z2, 2), z);               // 9
  const Fe25519 z11 = fe_mul(z9, z2);                         // 11
  const Fe25519 z_5_0 = fe_mul(fe_sq(z11), z9);               // 2^5 - 2^0 = 31
  const Fe25519 z_10_0 = fe_mul(fe_sq_n(z_5_0, 5), z_5_0);    // 2^10 - 2^0
  const Fe25519 z_20_0 = fe_mul(fe_sq_n(z_10_0, 10), z_10_0); // 2^20 - 2^0
  const Fe25519 z_40_0 = fe_mul(fe_sq_n(z_20_0, 20), z_20_0); // 2^40 - 2^0
  const Fe25519 z_50_0 = fe_mul(fe_sq_n(z_40_0, 10), z_10_0); // 2^50 - 2^0
  const Fe25519 z_100_0 = fe_mul(fe_sq_n(z_50_0, 50), z_50_0);     // 2^100 - 2^0
  const Fe25519 z_200_0 = fe_mul(fe_sq_n(z_100_0, 100), z_100_0);  // 2^200 - 2^0
  const Fe25519 z_250_0 = fe_mul(fe_sq_n(z_200_0, 50), z_50_0);    // 2^250 - 2^0
  return fe_mul(fe_sq_n(z_250_0, 5), z11);                         // 2^255 - 2^5 + 11 = 2^255 - 21
}

// the one representative in [0, p) of a carried element, as eight little-endian words
WGCS_HD void fe_to_words(const Fe25519& f, uint32_t w[8]) {
  // A carried element is below 2^255 + 2^17 * 2^26 < 2 p.  q = floor((f + 19) / 2^255) is 1
  // exactly when f >= p; f + 19 q with bit 255 dropped is then f - q p.
  uint32_t q = (f.v0 + 19) >> 26;
  q = (f.v1 + q) >> 25;
  q = (f.v2 + q) >> 26;
  q = (f.v3 + q) >> 25;
  q = (f.v4 + q) >> 26;
  q = (f.v5 + q) >> 25;
  q = (f.v6 + q) >> 26;
  q = (f.v7 + q) >> 25;
  q = (f.v8 + q) >> 26;
  q = (f.v9 + q) >> 25;
  uint32_t c;
  uint32_t h0 = f.v0 + 19 * q;
  c = h0 >> 26; h0 &= kFeMask26;
  uint32_t h1 = f.v1 + c;
  c = h1 >> 25; h1 &= kFeMask25;
  uint32_t h2 = f.v2 + c;
  c = h2 >> 26; h2 &= kFeMask26;
  uint32_t h3 = f.v3 + c;
  c = h3 >> 25; h3 &= kFeMask25;
  uint32_t h4 = f.v4 + c;
  c = h4 >> 26; h4 &= kFeMask26;
  uint32_t h5 = f.v5 + c;
  c = h5 >> 25; h5 &= kFeMask25;
  uint32_t h6 = f.v6 + c;
  c = h6 >> 26; h6 &= kFeMask26;
  uint32_t h7 = f.v7 + c;
  c = h7 >> 25; h7 &= kFeMask25;
  uint32_t h8 = f.v8 + c;
  c = h8 >> 26; h8 &= kFeMask26;
  const uint32_t h9 = (f.v9 + c) & kFeMask25;  // the carry out of limb 9 is q 2^255: dropped
  w[0] = h0 | (h1 << 26);
  w[1] = (h1 >> 6) | (h2 << 19);
  w[2] = (h2 >> 13) | (h3 << 13);
  w[3] = (h3 >> 19) | (h4 << 6);
  w[4] = h5 | (h6 << 25);
  w[5] = (h6 >> 7) | (h7 << 19);
  w[6] = (h7 >> 13) | (h8 << 12);
  w[7] = (h8 >> 20) | (h9 << 6);
}

// swap a and b where mask is all ones, leave them where it is zero
WGCS_HD void fe_cswap(Fe25519& a, Fe25519& b, uint32_t mask) {
  uint32_t t;
  t = mask & (a.v0 ^ b.v0); a.v0 ^= t; b.v0 ^= t;
  t = mask & (a.v1 ^ b.v1); a.v1 ^= t; b.v1 ^= t;
  t = mask & (a.v2 ^ b.v2); a.v2 ^= t; b.v2 ^= t;
  t = mask & (a.v3 ^ b.v3); a.v3 ^= t; b.v3 ^= t;
  t = mask & (a.v4 ^ b.v4); a.v4 ^= t; b.v4 ^= t;
  t = mask & (a.v5 ^ b.v5); a.v5 ^= t; b.v5 ^= t;
  t = mask & (a.v6 ^ b.v6); a.v6 ^= t; b.v6 ^= t;
  t = mask & (a.v7 ^ b.v7); a.v7 ^= t; b.v7 ^= t;
  t = mask & (a.v8 ^ b.v8); a.v8 ^= t; b.v8 ^= t;
  t = mask & (a.v9 ^ b.v9); a.v9 ^= t; b.v9 ^= t;
}

// X25519(scalar, point) on little-endian words: the scalar is clamped here
// (decodeScalar25519), bit 255 of the point is ignored, a point in [p, 2^255)
// is reduced, and out is the one representative below p.  False, with out all
// zero, is curve25519's "bad input point: low order point".
WGCS_HD bool x25519_words(const uint32_t scalar[8], const uint32_t point[8], uint32_t out[8]) {
  // the clamped scalar, shifted up by one so that bit 254 is on top: every step takes the top
  // bit and shifts once more (bit 255 of a clamped scalar is clear and is not a ladder step)
  uint32_t k0 = scalar[0] & 0xFFFFFFF8u, k1 = scalar[1], k2 = scalar[2], k3 = scalar[3], k4 = scalar[4],
           k5 = scalar[5], k6 = scalar[6], k7 = (scalar[7] & 0x7FFFFFFFu) | 0x40000000u;
  k7 = (k7 << 1) | (k6 >> 31);
  k6 = (k6 << 1) | (k5 >> 31);
  k5 = (k5 << 1) | (k4 >> 31);
  k4 = (k4 << 1) | (k3 >> 31);
  k3 = (k3 << 1) | (k2 >> 31);
  k2 = (k2 << 1) | (k1 >> 31);
  k1 = (k1 << 1) | (k0 >> 31);
  k0 <<= 1;
  const Fe25519 x1 = fe_from_words(point);
  Fe25519 x2 = fe_one(), z2 = fe_zero(), x3 = x1, z3 = fe_one();
  uint32_t swap = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int t = 254; t >= 0; --t) {
    const uint32_t bit = k7 >> 31;
    k7 = (k7 << 1) | (k6 >> 31);
    k6 = (k6 << 1) | (k5 >> 31);
    k5 = (k5 << 1) | (k4 >> 31);
    k4 = (k4 << 1) | (k3 >> 31);
    k3 = (k3 << 1) | (k2 >> 31);
    k2 = (k2 << 1) | (k1 >> 31);
    k1 = (k1 << 1) | (k0 >> 31);
    k0 <<= 1;
    swap ^= bit;
    const uint32_t mask = 0u - swap;
    fe_cswap(x2, x3, mask);
    fe_cswap(z2, z3, mask);
    swap = bit;
    // the step of RFC 7748 §5
    const Fe25519 a = fe_add(x2, z2), aa = fe_sq(a);
    const Fe25519 b = fe_sub(x2, z2), bb = fe_sq(b);
    const Fe25519 e = fe_sub(aa, bb);
    const Fe25519 c = fe_add(x3, z3), d = fe_sub(x3, z3);
    const Fe25519 da = fe_mul(d, a), cb = fe_mul(c, b);
    x3 = fe_sq(fe_add(da, cb));
    z3 = fe_mul(x1, fe_sq(fe_sub(da, cb)));
    x2 = fe_mul(aa, bb);
    z2 = fe_mul(e, fe_add(aa, fe_mul_a24(e)));
  }
  const uint32_t mask = 0u - swap;
  fe_cswap(x2, x3, mask);
  fe_cswap(z2, z3, mask);
  fe_to_words(fe_mul(x2, fe_invert(z2)), out);
  return (out[0] | out[1] | out[2] | out[3] | out[4] | out[5] | out[6] | out[7]) != 0;
}

}  // namespace wgcs
