// wgcs_noise.h -- the scalar steps of the reference's Noise_IKpsk2 handshake:
// the initiation and its consumption (device/noise.go:91-94, :324-457,
// device/noise_helpers.go:18-58), the response, its consumption and the
// session keys of both sides (noise.go:494-546, :573-604, :636-655), and the
// rows of the initiator's two batches over a table of handshake states (the
// section before the last), shared by hs_consume_kernel and hs_respond_kernel
// (noise_kernels.hip), hs_initiate_kernel, hs_finish_kernel and
// hs_finish_commit_kernel (noise_init_kernels.hip), the kernels of
// noise_accept_kernels.hip (the timestamp and flood rules, noise.go:458-491, the
// last section), the host functions of noise.cpp and the host test programs
// tests/noise_host/noise_host.cpp, tests/noise_resp_host/noise_resp_host.cpp,
// tests/noise_init_host/noise_init_host.cpp and
// tests/noise_accept_host/noise_accept_host.cpp.
//
// Everything is little-endian words in registers: a hash, a chaining key, a
// key, a public key and a shared secret are 8 words, a message is its 37.
//   mixHash(h, data)   = BLAKE2s-256(h | data)                       noise.go:332-338
//   mixKey(c, data)    = KDF1(c, data)                               :340-342
//   HMAC               = HMAC over unkeyed BLAKE2s-256, 64-byte block, noise_helpers.go:18-35
//                        (not keyed BLAKE2s); every key of the handshake is 32 bytes
//   KDF1 / KDF2 / KDF3 = HKDF (RFC 5869) with that HMAC              :37-58
//   the AEAD           = ChaCha20-Poly1305 (RFC 8439 §2.8) under the zero nonce
//                        with the 32-byte hash as additional data and a text
//                        of 32 (a static key), 12 (a timestamp) or 0 bytes
// Inputs of the hash are zero-padded word arrays with a byte length; every
// length is a constant where the kernel calls, so the block loops unroll and
// nothing is indexed at run time (the rule of wgcs_blake2s.h).
//
// An initiation (MessageInitiation, noise.go:100-125) in words:
//   0 type | 1 sender | 2..9 ephemeral | 10..17 static ct | 18..21 its tag |
//   22..24 timestamp ct | 25..28 its tag | 29..32 MAC1 | 33..36 MAC2
// A response (MessageResponse, noise.go:159-174) in words:
//   0 type | 1 sender | 2 receiver | 3..10 ephemeral | 11..14 the empty text's tag |
//   15..18 MAC1 | 19..22 MAC2
#pragma once

#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_blake2s.h"
#include "wgcs_cookie.h"
#include "wgcs_x25519.h"
#include "wgcs_xchacha.h"

#pragma push_macro("WGCS_HD")  // wgcs_route_walk.h defines its own, plain inline: keep the forced one of wgcs_poly1305.h
#undef WGCS_HD
#include "wgcs_route_walk.h"  // session_get
#pragma pop_macro("WGCS_HD")

namespace wgcs {

constexpr uint32_t kNoiseInitiationSize = 148;  // MessageInitiationSize, noise.go:60
constexpr uint32_t kNoiseInitiationType = 1;    // MessageInitiationType
constexpr uint32_t kNoiseBodyWords = 29;        // everything before MAC1: what ConsumeMessageInitiation reads

// BLAKE2s-256, unkeyed, of the first len <= 128 bytes of in (zero-padded words)
WGCS_HD void noise_hash(const uint32_t in[32], uint32_t len, uint32_t h[8]) {
  h[0] = kB2sIv0 ^ 0x01010020u;  // §2.5: digest 32, no key, fanout 1, depth 1
  h[1] = kB2sIv1;
  h[2] = kB2sIv2;
  h[3] = kB2sIv3;
  h[4] = kB2sIv4;
  h[5] = kB2sIv5;
  h[6] = kB2sIv6;
  h[7] = kB2sIv7;
  if (len <= 64) {
    blake2s_compress(h, in, len, true);
  } else {
    blake2s_compress(h, in, 64, false);
    blake2s_compress(h, in + 16, len, true);
  }
}

// mixHash (noise.go:332-338): h = BLAKE2s-256(h | data), data of len <= 48 bytes
WGCS_HD void noise_mix_hash(uint32_t h[8], const uint32_t data[12], uint32_t len) {
  uint32_t in[32];
#pragma unroll
  for (int i = 0; i < 8; ++i) in[i] = h[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) in[8 + i] = data[i];
#pragma unroll
  for (int i = 20; i < 32; ++i) in[i] = 0;
  noise_hash(in, 32 + len, h);
}

// HMAC1 (noise_helpers.go:18-25): HMAC-BLAKE2s-256 of len <= 64 bytes under a 32-byte key
WGCS_HD void noise_hmac1(const uint32_t key[8], const uint32_t data[16], uint32_t len, uint32_t out[8]) {
  uint32_t in[32], inner[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) in[i] = key[i] ^ 0x36363636u;  // ipad
#pragma unroll
  for (int i = 8; i < 16; ++i) in[i] = 0x36363636u;
#pragma unroll
  for (int i = 0; i < 16; ++i) in[16 + i] = data[i];
  noise_hash(in, 64 + len, inner);
#pragma unroll
  for (int i = 0; i < 8; ++i) in[i] = key[i] ^ 0x5c5c5c5cu;  // opad
#pragma unroll
  for (int i = 8; i < 16; ++i) in[i] = 0x5c5c5c5cu;
#pragma unroll
  for (int i = 0; i < 8; ++i) in[16 + i] = inner[i];
#pragma unroll
  for (int i = 24; i < 32; ++i) in[i] = 0;
  noise_hash(in, 96, out);
}

// HMAC2 (:27-35) as the KDFs use it: the 32 bytes of in0, then the one byte in1
WGCS_HD void noise_hmac2(const uint32_t key[8], const uint32_t in0[8], uint32_t in1, uint32_t out[8]) {
  const uint32_t data[16] = {in0[0], in0[1], in0[2], in0[3], in0[4], in0[5], in0[6], in0[7], in1 & 0xFFu,
                             0,      0,      0,      0,      0,      0,      0};
  noise_hmac1(key, data, 33, out);
}

// the expansion of KDF1 / KDF2 / KDF3 under the pseudo-random key prk
WGCS_HD void noise_kdf_first(const uint32_t prk[8], uint32_t t0[8]) {
  const uint32_t one[16] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  noise_hmac1(prk, one, 1, t0);
}

// KDF1 (:37-40), input of len <= 64 bytes; t0 may be key
WGCS_HD void noise_kdf1(uint32_t t0[8], const uint32_t key[8], const uint32_t input[16], uint32_t len) {
  uint32_t prk[8];
  noise_hmac1(key, input, len, prk);
  noise_kdf_first(prk, t0);
}

// KDF2 (:42-49); t0 may be key
WGCS_HD void noise_kdf2(uint32_t t0[8], uint32_t t1[8], const uint32_t key[8], const uint32_t input[16], uint32_t len) {
  uint32_t prk[8];
  noise_hmac1(key, input, len, prk);
  noise_kdf_first(prk, t0);
  noise_hmac2(prk, t0, 2, t1);
}

// KDF3 (:51-58); t0 may be key
WGCS_HD void noise_kdf3(uint32_t t0[8], uint32_t t1[8], uint32_t t2[8], const uint32_t key[8], const uint32_t input[16],
                        uint32_t len) {
  uint32_t prk[8];
  noise_hmac1(key, input, len, prk);
  noise_kdf_first(prk, t0);
  noise_hmac2(prk, t0, 2, t1);
  noise_hmac2(prk, t1, 3, t2);
}

// KDF1 / KDF2 of a 32-byte input, the only size the handshake feeds them
WGCS_HD void noise_pad32(const uint32_t in[8], uint32_t out[16]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = in[i];
#pragma unroll
  for (int i = 8; i < 16; ++i) out[i] = 0;
}

// mixKey (noise.go:340-342) of 32 bytes
WGCS_HD void noise_mix_key(uint32_t chain[8], const uint32_t data[8]) {
  uint32_t in[16];
  noise_pad32(data, in);
  noise_kdf1(chain, chain, in, 32);
}

// KDF2(&chain, &key, chain[:], secret[:]) of noise.go:371-376, :384-389, :425, :444-449
WGCS_HD void noise_mix_secret(uint32_t chain[8], uint32_t key[8], const uint32_t secret[8]) {
  uint32_t in[16];
  noise_pad32(secret, in);
  noise_kdf2(chain, key, chain, in, 32);
}

// The Poly1305 tag of RFC 8439 §2.8 over ad (32 bytes) | ct (n <= 32 bytes, a multiple of 4,
// zero-padded: pad16 is part of the construction) | LE64(32) | LE64(n), under the one-time key.
WGCS_HD void noise_aead_tag(const uint32_t otk[8], const uint32_t ad[8], const uint32_t ct[8], uint32_t n,
                            uint32_t tag[4]) {
  const P1305 r = p1305_clamp_r(otk[0], otk[1], otk[2], otk[3]);
  P1305 h = p1305_mul(p1305_from_words(ad[0], ad[1], ad[2], ad[3], 1), r);
  h = p1305_mul(p1305_add(h, p1305_from_words(ad[4], ad[5], ad[6], ad[7], 1)), r);
  if (n > 0) h = p1305_mul(p1305_add(h, p1305_from_words(ct[0], ct[1], ct[2], ct[3], 1)), r);
  if (n > 16) h = p1305_mul(p1305_add(h, p1305_from_words(ct[4], ct[5], ct[6], ct[7], 1)), r);
  h = p1305_mul(p1305_add(h, p1305_from_words(32, 0, n, 0, 1)), r);
  p1305_finish(h, otk[4], otk[5], otk[6], otk[7], tag);
}

// aead.Seal(dst[:0], ZeroNonce[:], pt, ad): ct (n bytes as words, zero past them) and tag
WGCS_HD void noise_seal(const uint32_t key[8], const uint32_t pt[8], uint32_t n, const uint32_t ad[8], uint32_t ct[8],
                        uint32_t tag[4]) {
  uint32_t otk[8], ks[8];
  chacha20_block_head(key, 0, 0, 0, otk);
  chacha20_block_head(key, 1, 0, 0, ks);
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) ct[i] = 4 * i < n ? pt[i] ^ ks[i] : 0u;
  noise_aead_tag(otk, ad, ct, n, tag);
}

// aead.Open: true and the plaintext when the tag matches (an OR of XORs over all 16 bytes);
// pt is written either way and means nothing on false.  ct is zero past its n bytes.
WGCS_HD bool noise_open(const uint32_t key[8], const uint32_t ct[8], uint32_t n, const uint32_t tag[4],
                        const uint32_t ad[8], uint32_t pt[8]) {
  uint32_t otk[8], ks[8], want[4];
  chacha20_block_head(key, 0, 0, 0, otk);
  chacha20_block_head(key, 1, 0, 0, ks);
  noise_aead_tag(otk, ad, ct, n, want);
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) pt[i] = 4 * i < n ? ct[i] ^ ks[i] : 0u;
  return tag16_equal(want, tag);
}

// eight words of a table row's key or secret
WGCS_HD void noise_row_words(const uint8_t* p, uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t* const d = (const uint32_t*)p;  // rows are 4-byte aligned on the device
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = d[i];
#else
  b2s_key_words(p, 32, w);
#endif
}

WGCS_HD uint32_t noise_bswap(uint32_t x) {
  return (x << 24) | ((x & 0xFF00u) << 8) | ((x >> 8) & 0xFF00u) | (x >> 24);
}

// memcmp of two 32-byte strings held as little-endian words: -1, 0 or 1
WGCS_HD int noise_key_cmp(const uint32_t a[8], const uint32_t b[8]) {
  int r = 0;
#pragma unroll
  for (int i = 7; i >= 0; --i) {  // the lowest word that differs decides: later ones are overridden
    const uint32_t x = noise_bswap(a[i]), y = noise_bswap(b[i]);
    r = x < y ? -1 : x > y ? 1 : r;
  }
  return r;
}

// GetPeer (device.go) over the table of wgcs_peer_keys_build, rows sorted by public key:
// the row of key, or -1.  At most ceil(log2(n + 1)) probes.
WGCS_HD int32_t noise_find_peer(const wgcs_peer_key* table, uint32_t n, const uint32_t key[8]) {
  uint32_t lo = 0, hi = n;  // the first row >= key lies in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    uint32_t row[8];
    noise_row_words(table[mid].public_key, row);
    if (noise_key_cmp(row, key) < 0) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= n) return -1;
  uint32_t row[8];
  noise_row_words(table[lo].public_key, row);
  return noise_key_cmp(row, key) == 0 ? (int32_t)lo : -1;
}

// The words of wgcs_hs_init: 0 peer | 1 sender | 2..4 timestamp | 5..7 pad |
// 8..15 hash | 16..23 chain_key | 24..31 ephemeral.
constexpr uint32_t kHsInitWords = 32;

// ConsumeMessageInitiation up to the replay / flood check (noise.go:405-457)
// for the message words m under the responder's private key, hash0 =
// mixHash(InitialHash, its public key) (:415) and chain0 = InitialChainKey.
// Returns the verdict of wgcs_handshake_consume_batch and fills o as that
// function's table says: untouched for WGCS_ERR_INVALID_ARG, the whole row for
// WGCS_HS_CONSUMED, else zero but for the sender and the peer found so far.
WGCS_HD int noise_consume_initiation(const uint32_t priv[8], const uint32_t hash0[8], const uint32_t chain0[8],
                                     const wgcs_peer_key* table, uint32_t n_peers, const uint32_t m[kNoiseBodyWords],
                                     uint32_t o[kHsInitWords]) {
  if (m[0] != kNoiseInitiationType) return WGCS_ERR_INVALID_ARG;  // :406-408
#pragma unroll
  for (uint32_t i = 0; i < kHsInitWords; ++i) o[i] = 0;
  o[0] = WGCS_PEER_NONE;
  o[1] = m[1];
  uint32_t hash[8], chain[8], key[8], eph[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash[i] = hash0[i];
    chain[i] = chain0[i];
    eph[i] = m[2 + i];
  }
  const uint32_t eph12[12] = {eph[0], eph[1], eph[2], eph[3], eph[4], eph[5], eph[6], eph[7], 0, 0, 0, 0};
  noise_mix_hash(hash, eph12, 32);  // :416
  noise_mix_key(chain, eph);        // :417
  // decrypt static key
  uint32_t shared[8];
  if (!x25519_words(priv, eph, shared)) return WGCS_ERR_LOW_ORDER;  // :421-424
  noise_mix_secret(chain, key, shared);                              // :425
  uint32_t peer_pub[8];
  if (!noise_open(key, m + 10, 32, m + 18, hash, peer_pub)) return WGCS_ERR_AUTH;  // :427-430
  noise_mix_hash(hash, m + 10, 48);                                                 // :431
  const int32_t row = noise_find_peer(table, n_peers, peer_pub);                    // :432
  if (row < 0) return WGCS_ERR_NO_PEER;
  o[0] = table[row].peer;
  if (!(table[row].flags & 1u)) return WGCS_ERR_NO_PEER;  // :433-435: !peer.isRunning
  // verify identity
  noise_row_words(table[row].shared, shared);
  if ((shared[0] | shared[1] | shared[2] | shared[3] | shared[4] | shared[5] | shared[6] | shared[7]) == 0)
    return WGCS_ERR_NO_PEER;                // :440-443: isZero(precomputedSharedSecret)
  noise_mix_secret(chain, key, shared);     // :444-449
  const uint32_t ts_ct[8] = {m[22], m[23], m[24], 0, 0, 0, 0, 0};
  uint32_t ts[8];
  if (!noise_open(key, ts_ct, 12, m + 25, hash, ts)) return WGCS_ERR_AUTH;  // :451-455
  const uint32_t ts_field[12] = {m[22], m[23], m[24], m[25], m[26], m[27], m[28], 0, 0, 0, 0, 0};
  noise_mix_hash(hash, ts_field, 28);  // :456
  o[2] = ts[0];
  o[3] = ts[1];
  o[4] = ts[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[8 + i] = hash[i];
    o[16 + i] = chain[i];
    o[24 + i] = eph[i];
  }
  return WGCS_HS_CONSUMED;
}

// CreateMessageInitiation (noise.go:344-403) with the caller's ephemeral private key,
// timestamp and sender index: the 37 words of the message with zero MACs, and the handshake's
// hash and chaining key after it.  hash0 = mixHash(InitialHash, remote static) (:358), chain0 =
// InitialChainKey; static_pub is the sender's own public key.  WGCS_ERR_LOW_ORDER where either
// shared secret is zero (:366-369, :381-383), m then means nothing.
WGCS_HD int noise_create_initiation(const uint32_t static_priv[8], const uint32_t static_pub[8],
                                    const uint32_t remote_static[8], const uint32_t hash0[8],
                                    const uint32_t chain0[8], const uint32_t eph_priv[8], const uint32_t ts[3],
                                    uint32_t sender, uint32_t m[37], uint32_t hash[8], uint32_t chain[8]) {
  const uint32_t base[8] = {9, 0, 0, 0, 0, 0, 0, 0};
  uint32_t eph[8], key[8], shared[8];
#pragma unroll
  for (int i = 0; i < 37; ++i) m[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash[i] = hash0[i];
    chain[i] = chain0[i];
  }
  x25519_words(eph_priv, base, eph);  // :361
  m[0] = kNoiseInitiationType;
  m[1] = sender;
#pragma unroll
  for (int i = 0; i < 8; ++i) m[2 + i] = eph[i];
  noise_mix_key(chain, eph);  // :363
  const uint32_t eph12[12] = {eph[0], eph[1], eph[2], eph[3], eph[4], eph[5], eph[6], eph[7], 0, 0, 0, 0};
  noise_mix_hash(hash, eph12, 32);  // :364
  // encrypt static key
  if (!x25519_words(eph_priv, remote_static, shared)) return WGCS_ERR_LOW_ORDER;  // :366-369
  noise_mix_secret(chain, key, shared);                                            // :371-376
  noise_seal(key, static_pub, 32, hash, m + 10, m + 18);                           // :378
  noise_mix_hash(hash, m + 10, 48);                                                // :379
  // encrypt timestamp
  if (!x25519_words(static_priv, remote_static, shared)) return WGCS_ERR_LOW_ORDER;  // :381-383
  noise_mix_secret(chain, key, shared);                                               // :384-389
  const uint32_t ts_pt[8] = {ts[0], ts[1], ts[2], 0, 0, 0, 0, 0};
  uint32_t ts_ct[8], ts_tag[4];
  noise_seal(key, ts_pt, 12, hash, ts_ct, ts_tag);  // :392
  m[22] = ts_ct[0];
  m[23] = ts_ct[1];
  m[24] = ts_ct[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[25 + i] = ts_tag[i];
  noise_mix_hash(hash, m + 22, 28);  // :400: m[29..33] are still zero
  return WGCS_OK;
}

constexpr uint32_t kNoiseResponseSize = 92;       // MessageResponseSize, noise.go:62
constexpr uint32_t kNoiseResponseType = 2;        // MessageResponseType
constexpr uint32_t kNoiseResponseBodyWords = 15;  // everything before MAC1

// CreateMessageResponse (noise.go:494-546) and the responder's half of BeginSymmetricSession
// (:645-652) for one consumed initiation -- hash0, chain0 and remote_eph are the hash,
// chain_key and ephemeral of its wgcs_hs_init row, remote_index its sender -- with the
// caller's ephemeral private key and session index: the 15 words of the message before its
// MACs, send_key = encrypt and recv_key = decrypt.  psk is all zero where the peer has none.
// WGCS_ERR_LOW_ORDER where one of the three X25519 results is zero (:520-528; the public key
// of base point 9 never is, but it runs the one code path); m and both keys are then zero.
// The three scalar multiplications do not depend on the hashing between them, so they come
// first and share one ladder: the body of x25519_words exists once in the code.
WGCS_HD int noise_create_response(const uint32_t hash0[8], const uint32_t chain0[8], const uint32_t remote_eph[8],
                                  const uint32_t remote_static[8], const uint32_t psk[8], const uint32_t eph_priv[8],
                                  uint32_t local_index, uint32_t remote_index, uint32_t m[kNoiseResponseBodyWords],
                                  uint32_t send_key[8], uint32_t recv_key[8]) {
  uint32_t eph[8], ee[8], es[8];
  bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < 3; ++i) {  // the step is the same for every lane: no secret decides it
    uint32_t point[8], r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) point[j] = i == 0 ? (j == 0 ? 9u : 0u) : i == 1 ? remote_eph[j] : remote_static[j];
    ok = x25519_words(eph_priv, point, r) && ok;
    if (i == 0) {  // :517 localEphemeral.publicKey()
#pragma unroll
      for (int j = 0; j < 8; ++j) eph[j] = r[j];
    } else if (i == 1) {  // :520 sharedSecret(hs.remoteEphemeral)
#pragma unroll
      for (int j = 0; j < 8; ++j) ee[j] = r[j];
    } else {  // :525 sharedSecret(hs.remoteStatic)
#pragma unroll
      for (int j = 0; j < 8; ++j) es[j] = r[j];
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < kNoiseResponseBodyWords; ++i) m[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) send_key[i] = recv_key[i] = 0;
  if (!ok) return WGCS_ERR_LOW_ORDER;  // :520-528
  uint32_t hash[8], chain[8], tau[8], key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash[i] = hash0[i];
    chain[i] = chain0[i];
  }
  m[0] = kNoiseResponseType;  // :509
  m[1] = local_index;         // :510
  m[2] = remote_index;        // :511
#pragma unroll
  for (int i = 0; i < 8; ++i) m[3 + i] = eph[i];  // :517
  const uint32_t eph12[12] = {eph[0], eph[1], eph[2], eph[3], eph[4], eph[5], eph[6], eph[7], 0, 0, 0, 0};
  noise_mix_hash(hash, eph12, 32);  // :518
  noise_mix_key(chain, eph);        // :519
  noise_mix_key(chain, ee);         // :524
  noise_mix_key(chain, es);         // :529
  // add preshared key
  uint32_t in[16];
  noise_pad32(psk, in);
  noise_kdf3(chain, tau, key, chain, in, 32);  // :533-539
  const uint32_t tau12[12] = {tau[0], tau[1], tau[2], tau[3], tau[4], tau[5], tau[6], tau[7], 0, 0, 0, 0};
  noise_mix_hash(hash, tau12, 32);  // :540
  const uint32_t none[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t ct[8];
  noise_seal(key, none, 0, hash, ct, m + 11);  // :542
  // :543 mixes msg.Empty into hs.hash, which nothing reads before BeginSymmetricSession zeroes it (:658)
  noise_kdf2(recv_key, send_key, chain, none, 0);  // :646-651: KDF2(&decryptKey, &encryptKey, chainKey, nil)
  return WGCS_OK;
}

// The key of MAC1 for a message to the holder of the static public key pub:
// BLAKE2s-256("mac1----" | pub), CookieGenerator.Init (cookie.go:269-275)
WGCS_HD void noise_mac1_key(const uint32_t pub[8], uint32_t key[8]) {
  const uint32_t in[32] = {0x3163616Du, 0x2D2D2D2Du, pub[0], pub[1], pub[2], pub[3], pub[4], pub[5], pub[6], pub[7],
                           0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  noise_hash(in, 40, key);
}

// n words to p: aligned dword stores on the device, where a row is 4-byte aligned, byte stores on the host
WGCS_HD void noise_store_words(uint8_t* p, const uint32_t* w, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t* const d = (uint32_t*)p;
#pragma unroll
  for (uint32_t i = 0; i < n; ++i) d[i] = w[i];
#else
  for (uint32_t i = 0; i < n; ++i) b2s_store_le32(p + 4 * i, w[i]);
#endif
}

// The 92 bytes of a response at msg from the words of noise_create_response, with AddMACs
// (cookie.go:287-314): MAC1 under mac1_key over the 60 bytes before it, and MAC2 under the
// cookie over the 76 bytes before it, or zero without one (:307-309).  The MACs are taken over
// the bytes just stored.
WGCS_HD void noise_write_response(uint8_t* msg, const uint32_t m[kNoiseResponseBodyWords], const uint32_t mac1_key[8],
                                  bool has_cookie, const uint32_t cookie[4]) {
  uint32_t mac[4];
  noise_store_words(msg, m, kNoiseResponseBodyWords);
  cookie_mac128(mac1_key, 32, msg, kNoiseResponseSize - 2 * kMacSize, mac);  // :296-300
  noise_store_words(msg + (kNoiseResponseSize - 2 * kMacSize), mac, 4);
  if (has_cookie) {
    const uint32_t key[8] = {cookie[0], cookie[1], cookie[2], cookie[3], 0, 0, 0, 0};
    cookie_mac128(key, 16, msg, kNoiseResponseSize - kMacSize, mac);  // :309-313
  } else {
    mac[0] = mac[1] = mac[2] = mac[3] = 0;
  }
  noise_store_words(msg + (kNoiseResponseSize - kMacSize), mac, 4);
}

// ConsumeMessageResponse (noise.go:548-620) and the initiator's half of BeginSymmetricSession
// (:637-644) for the words m of a response, under the initiator's static private key, the
// hash, chaining key and ephemeral private key it kept from CreateMessageInitiation and the
// preshared key (zero where there is none).  local_index is the index this handshake is
// registered under: sessions.Get(msg.Receiver) finding another one, or none (:553-557), and a
// wrong type word (:549-551) are WGCS_ERR_INVALID_ARG.  WGCS_ERR_LOW_ORDER where a shared
// secret is zero (:575-584), WGCS_ERR_AUTH where the empty text does not open (:600-603);
// both keys are zero for every failure.  Else WGCS_OK, *sender = msg.Sender (:614),
// send_key = encrypt and recv_key = decrypt.
WGCS_HD int noise_consume_response(const uint32_t static_priv[8], const uint32_t hash0[8], const uint32_t chain0[8],
                                   const uint32_t eph_priv[8], const uint32_t psk[8], uint32_t local_index,
                                   const uint32_t m[kNoiseResponseBodyWords], uint32_t* sender, uint32_t send_key[8],
                                   uint32_t recv_key[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) send_key[i] = recv_key[i] = 0;
  if (m[0] != kNoiseResponseType || m[2] != local_index) return WGCS_ERR_INVALID_ARG;  // :549-557
  uint32_t hash[8], chain[8], eph[8], shared[8], tau[8], key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash[i] = hash0[i];
    chain[i] = chain0[i];
    eph[i] = m[3 + i];
  }
  // finish 3-way DH
  const uint32_t eph12[12] = {eph[0], eph[1], eph[2], eph[3], eph[4], eph[5], eph[6], eph[7], 0, 0, 0, 0};
  noise_mix_hash(hash, eph12, 32);                                               // :573
  noise_mix_key(chain, eph);                                                     // :574
  if (!x25519_words(eph_priv, eph, shared)) return WGCS_ERR_LOW_ORDER;           // :575-578
  noise_mix_key(chain, shared);                                                  // :579
  if (!x25519_words(static_priv, eph, shared)) return WGCS_ERR_LOW_ORDER;        // :581-584
  noise_mix_key(chain, shared);                                                  // :585
  // add preshared key (psk)
  uint32_t in[16];
  noise_pad32(psk, in);
  noise_kdf3(chain, tau, key, chain, in, 32);  // :590-596
  const uint32_t tau12[12] = {tau[0], tau[1], tau[2], tau[3], tau[4], tau[5], tau[6], tau[7], 0, 0, 0, 0};
  noise_mix_hash(hash, tau12, 32);  // :597
  // authenticate transcript
  const uint32_t none[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t pt[8];
  if (!noise_open(key, none, 0, m + 11, hash, pt)) return WGCS_ERR_AUTH;  // :599-603
  // :604 mixes msg.Empty into the hash, which nothing reads before BeginSymmetricSession zeroes it (:658)
  *sender = m[1];                                  // :614
  noise_kdf2(send_key, recv_key, chain, none, 0);  // :638-643: KDF2(&encryptKey, &decryptKey, chainKey, nil)
  return WGCS_OK;
}

// ---- the initiator's batches: wgcs_handshake_initiate_batch / _finish_batch and their host
// forms (include/wgcsum.h).  One row function per step, the same text for a lane of
// hs_initiate_kernel / hs_finish_kernel / hs_finish_commit_kernel (noise_init_kernels.hip) and
// for the loops of noise.cpp: struct members are read as they are (4-byte aligned on both
// sides), byte arrays through noise_load_words / noise_store_words.

constexpr uint32_t kNoiseInitiationPitch = 160;  // a row of d_msgs: the 148 bytes and 12 of zero
constexpr uint32_t kHsClaimNone = 0xFFFFFFFFu;   // wgcs_hs_state.claim outside a finish call
constexpr uint32_t kHsWorkWords = 16;            // a row of d_work: encrypt | decrypt

// InitialHash and InitialChainKey of init() (noise.go:91-94): BLAKE2s-256 of the construction
// name, and of that | the identifier.  noise.cpp computes the same two from the strings.
WGCS_HD void noise_initial(uint32_t hash[8], uint32_t chain[8]) {
  const uint32_t h[8] = {0x61B31122u, 0x66C51A08u, 0xDB431269u, 0x32D58A45u,
                         0x666C9C2Du, 0xB7E89322u, 0x659CE10Eu, 0xF39E07BAu};
  const uint32_t c[8] = {0xAE6DE260u, 0xC0EF27F3u, 0xE235C32Eu, 0xD0D225A0u,
                         0x0642EB16u, 0xF57772F8u, 0x98D1382Du, 0x36CD788Bu};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash[i] = h[i];
    chain[i] = c[i];
  }
}

// n words of a row's byte array
WGCS_HD void noise_load_words(const uint8_t* p, uint32_t* w, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t* const d = (const uint32_t*)p;  // rows are 4-byte aligned on the device
#pragma unroll
  for (uint32_t i = 0; i < n; ++i) w[i] = d[i];
#else
  for (uint32_t i = 0; i < n; ++i) w[i] = b2s_load_le32(p, 4 * i, 4 * n);
#endif
}

// The first N words of the message at p, any alignment.  On the device N + 1 aligned dword
// loads and a funnel shift by the pointer's low bits (the form of b2s_load_block): the last
// dword ends at most 4 N + 4 bytes into the message, so N + 1 words of it must exist.
template <uint32_t N>
WGCS_HD void noise_msg_words(const uint8_t* p, uint32_t m[N]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t sh = (uint32_t)(uintptr_t)p & 3u;
  const uint32_t* const w = (const uint32_t*)(p - sh);
  uint32_t d[N + 1];
#pragma unroll
  for (uint32_t i = 0; i < N + 1; ++i) d[i] = w[i];
#pragma unroll
  for (uint32_t i = 0; i < N; ++i) m[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
#else
  for (uint32_t i = 0; i < N; ++i) m[i] = b2s_load_le32(p, 4 * i, 4 * N);
#endif
}

// noise_create_initiation where the static-static secret is the peer's precomputedSharedSecret
// (noise.go:305, :381-383), as CreateMessageInitiation itself has it: two scalar
// multiplications, base point x ephemeral (:361) and ephemeral x remote static (:366), which
// do not depend on the hashing between them and share one ladder, as the three of
// noise_create_response do.  The same m, hash and chain as noise_create_initiation gives for
// precomputed = X25519(static private, remote static); WGCS_ERR_LOW_ORDER, with m zeroed,
// where that or ephemeral x remote static is all zero.
WGCS_HD int noise_create_initiation_shared(const uint32_t static_pub[8], const uint32_t remote_static[8],
                                           const uint32_t precomputed[8], const uint32_t hash0[8],
                                           const uint32_t chain0[8], const uint32_t eph_priv[8], const uint32_t ts[3],
                                           uint32_t sender, uint32_t m[37], uint32_t hash[8], uint32_t chain[8]) {
  uint32_t eph[8], es[8], key[8];
  bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < 2; ++i) {  // the step is the same for every lane: no secret decides it
    uint32_t point[8], r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) point[j] = i == 0 ? (j == 0 ? 9u : 0u) : remote_static[j];
    ok = x25519_words(eph_priv, point, r) && ok;
    if (i == 0) {  // :361 hs.localEphemeral.publicKey()
#pragma unroll
      for (int j = 0; j < 8; ++j) eph[j] = r[j];
    } else {  // :366 sharedSecret(hs.remoteStatic)
#pragma unroll
      for (int j = 0; j < 8; ++j) es[j] = r[j];
    }
  }
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) any |= precomputed[i];
#pragma unroll
  for (int i = 0; i < 37; ++i) m[i] = 0;
  if (!ok || any == 0) return WGCS_ERR_LOW_ORDER;  // :366-369, :381-383
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash[i] = hash0[i];
    chain[i] = chain0[i];
  }
  m[0] = kNoiseInitiationType;
  m[1] = sender;
#pragma unroll
  for (int i = 0; i < 8; ++i) m[2 + i] = eph[i];
  noise_mix_key(chain, eph);  // :363
  const uint32_t eph12[12] = {eph[0], eph[1], eph[2], eph[3], eph[4], eph[5], eph[6], eph[7], 0, 0, 0, 0};
  noise_mix_hash(hash, eph12, 32);  // :364
  // encrypt static key
  noise_mix_secret(chain, key, es);                       // :371-376
  noise_seal(key, static_pub, 32, hash, m + 10, m + 18);  // :378
  noise_mix_hash(hash, m + 10, 48);                       // :379
  // encrypt timestamp
  noise_mix_secret(chain, key, precomputed);  // :384-389
  const uint32_t ts_pt[8] = {ts[0], ts[1], ts[2], 0, 0, 0, 0, 0};
  uint32_t ts_ct[8], ts_tag[4];
  noise_seal(key, ts_pt, 12, hash, ts_ct, ts_tag);  // :392
  m[22] = ts_ct[0];
  m[23] = ts_ct[1];
  m[24] = ts_ct[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) m[25 + i] = ts_tag[i];
  noise_mix_hash(hash, m + 22, 28);  // :400: m[29..33] are still zero
  return WGCS_OK;
}

// The 160 bytes of a d_msgs row at msg from the words of noise_create_initiation_shared, with
// AddMACs (cookie.go:287-314): MAC1 under mac1_key over the 116 bytes before it, MAC2 under
// the cookie over the 132 bytes before it, or zero without one, and 12 bytes of zero.  The
// MACs are taken over the bytes just stored.
WGCS_HD void noise_write_initiation(uint8_t* msg, const uint32_t m[kNoiseBodyWords], const uint32_t mac1_key[8],
                                    bool has_cookie, const uint32_t cookie[4]) {
  uint32_t mac[4];
  noise_store_words(msg, m, kNoiseBodyWords);
  cookie_mac128(mac1_key, 32, msg, kNoiseInitiationSize - 2 * kMacSize, mac);  // :296-300
  noise_store_words(msg + (kNoiseInitiationSize - 2 * kMacSize), mac, 4);
  if (has_cookie) {
    const uint32_t key[8] = {cookie[0], cookie[1], cookie[2], cookie[3], 0, 0, 0, 0};
    cookie_mac128(key, 16, msg, kNoiseInitiationSize - kMacSize, mac);  // :309-313
  } else {
    mac[0] = mac[1] = mac[2] = mac[3] = 0;
  }
  noise_store_words(msg + (kNoiseInitiationSize - kMacSize), mac, 4);
  const uint32_t zero[3] = {0, 0, 0};
  noise_store_words(msg + kNoiseInitiationSize, zero, 3);
}

// One descriptor of wgcs_handshake_initiate_batch: its status, with the message row at msg
// and the state row written as that function's table says.
WGCS_HD int noise_initiate_row(const wgcs_hs_start* d, const uint8_t* static_public, const wgcs_peer_key* table,
                               uint32_t n_peers, uint32_t n_keys, wgcs_hs_state* states, uint32_t n_states,
                               uint8_t* msg) {
  const uint32_t state_row = d->state_row, peer_row = d->peer_row, local_index = d->local_index;
  const uint32_t send_row = d->send_key, recv_row = d->recv_key, flags = d->flags;
  if (state_row >= n_states || peer_row >= n_peers || send_row >= n_keys || recv_row >= n_keys || send_row == recv_row)
    return WGCS_ERR_INVALID_ARG;
  const wgcs_peer_key* const peer = table + peer_row;
  uint32_t static_pub[8], remote[8], shared[8], eph_priv[8], ts[3], cookie[4], hash0[8], chain0[8];
  noise_row_words(static_public, static_pub);
  noise_row_words(peer->public_key, remote);
  noise_row_words(peer->shared, shared);
  noise_row_words(d->ephemeral_private, eph_priv);
  noise_load_words(d->timestamp, ts, 3);
  noise_load_words(d->cookie, cookie, 4);
  noise_initial(hash0, chain0);
  const uint32_t remote12[12] = {remote[0], remote[1], remote[2], remote[3], remote[4], remote[5],
                                 remote[6], remote[7], 0,         0,         0,         0};
  noise_mix_hash(hash0, remote12, 32);  // :358
  uint32_t m[37], hash[8], chain[8];
  const int rc =
      noise_create_initiation_shared(static_pub, remote, shared, hash0, chain0, eph_priv, ts, local_index, m, hash, chain);
  if (rc != WGCS_OK) {  // a zero shared secret: the state row is not touched
    noise_store_words(msg, m, 37);
    const uint32_t zero[3] = {0, 0, 0};
    noise_store_words(msg + kNoiseInitiationSize, zero, 3);
    return rc;
  }
  uint32_t mac1_key[8];
  noise_mac1_key(remote, mac1_key);
  noise_write_initiation(msg, m, mac1_key, (flags & WGCS_HS_START_COOKIE) != 0, cookie);
  wgcs_hs_state* const st = states + state_row;
  st->state = WGCS_HS_STATE_INITIATED;
  st->local_index = local_index;
  st->peer_row = peer_row;
  st->remote_index = 0;
  st->send_key = send_row;
  st->recv_key = recv_row;
  st->claim = kHsClaimNone;
  st->pad = 0;
  noise_store_words(st->hash, hash, 8);
  noise_store_words(st->chain_key, chain, 8);
  noise_store_words(st->ephemeral_private, eph_priv, 8);
  return WGCS_HS_INITIATED;
}

// The cryptography of noise_consume_response (noise.go:573-604, :638-643) without its lookup:
// the two scalar multiplications, ephemeral x msg.Ephemeral (:575) and static x msg.Ephemeral
// (:581), come first and share one ladder.  WGCS_OK with send_key = encrypt and recv_key =
// decrypt, or WGCS_ERR_LOW_ORDER / WGCS_ERR_AUTH with both zero.
WGCS_HD int noise_finish_response(const uint32_t static_priv[8], const uint32_t hash0[8], const uint32_t chain0[8],
                                  const uint32_t eph_priv[8], const uint32_t psk[8],
                                  const uint32_t m[kNoiseResponseBodyWords], uint32_t send_key[8],
                                  uint32_t recv_key[8]) {
  uint32_t eph[8], ee[8], se[8];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) eph[i] = m[3 + i];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int i = 0; i < 2; ++i) {  // the step is the same for every lane: no secret decides it
    uint32_t k[8], r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = i == 0 ? eph_priv[j] : static_priv[j];
    ok = x25519_words(k, eph, r) && ok;
    if (i == 0) {  // :575 hs.localEphemeral.sharedSecret(msg.Ephemeral)
#pragma unroll
      for (int j = 0; j < 8; ++j) ee[j] = r[j];
    } else {  // :581 device.staticIdentity.privateKey.sharedSecret(msg.Ephemeral)
#pragma unroll
      for (int j = 0; j < 8; ++j) se[j] = r[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) send_key[i] = recv_key[i] = 0;
  if (!ok) return WGCS_ERR_LOW_ORDER;  // :575-584
  uint32_t hash[8], chain[8], tau[8], key[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    hash[i] = hash0[i];
    chain[i] = chain0[i];
  }
  const uint32_t eph12[12] = {eph[0], eph[1], eph[2], eph[3], eph[4], eph[5], eph[6], eph[7], 0, 0, 0, 0};
  noise_mix_hash(hash, eph12, 32);  // :573
  noise_mix_key(chain, eph);        // :574
  noise_mix_key(chain, ee);         // :579
  noise_mix_key(chain, se);         // :585
  // add preshared key (psk)
  uint32_t in[16];
  noise_pad32(psk, in);
  noise_kdf3(chain, tau, key, chain, in, 32);  // :590-596
  const uint32_t tau12[12] = {tau[0], tau[1], tau[2], tau[3], tau[4], tau[5], tau[6], tau[7], 0, 0, 0, 0};
  noise_mix_hash(hash, tau12, 32);  // :597
  // authenticate transcript
  const uint32_t none[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t pt[8];
  if (!noise_open(key, none, 0, m + 11, hash, pt)) return WGCS_ERR_AUTH;  // :599-603
  noise_kdf2(send_key, recv_key, chain, none, 0);                         // :638-643
  return WGCS_OK;
}

// The first pass over row q of wgcs_handshake_finish_batch: its verdict before the duplicate
// rule.  The states are only read, but for the claim: an authentic row leaves its two keys in
// its row of work and takes the minimum of q and the state's claim.
WGCS_HD int noise_finish_row(uint32_t q, const uint8_t* arena, const wgcs_aead_pkt* pkts, const int32_t* types,
                             const int32_t* gate, const wgcs_noise_responder* self, const wgcs_session_slot* slots,
                             uint32_t n_slots, wgcs_hs_state* states, uint32_t n_states, const uint8_t* psk_table,
                             uint32_t n_peers, uint32_t n_keys, uint8_t* work) {
  if (types[q] != (int32_t)kNoiseResponseType || (gate && gate[q] != WGCS_HS_PASS)) return WGCS_HS_NONE;
  const wgcs_aead_pkt pk = pkts[q];
  if (pk.len != kNoiseResponseSize) return WGCS_ERR_INVALID_ARG;
  uint32_t m[kNoiseResponseBodyWords];
  noise_msg_words<kNoiseResponseBodyWords>(arena + pk.off, m);
  if (m[0] != kNoiseResponseType) return WGCS_ERR_INVALID_ARG;  // :549-551
  const uint32_t row = session_get(slots, n_slots, m[2]);       // :553 sessions.Get(msg.Receiver); empty is past any table
  if (row >= n_states) return WGCS_ERR_NO_HANDSHAKE;
  wgcs_hs_state* const st = states + row;
  if (st->state != WGCS_HS_STATE_INITIATED || st->local_index != m[2]) return WGCS_ERR_NO_HANDSHAKE;  // :566
  const uint32_t peer_row = st->peer_row;
  if (peer_row >= n_peers || st->send_key >= n_keys || st->recv_key >= n_keys) return WGCS_ERR_INVALID_ARG;
  uint32_t priv[8], hash0[8], chain0[8], eph_priv[8], psk[8], keys[kHsWorkWords];
  noise_row_words(self->private_key, priv);
  noise_row_words(st->hash, hash0);
  noise_row_words(st->chain_key, chain0);
  noise_row_words(st->ephemeral_private, eph_priv);
  if (psk_table) {
    noise_row_words(psk_table + 32 * (uint64_t)peer_row, psk);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) psk[i] = 0;
  }
  const int rc = noise_finish_response(priv, hash0, chain0, eph_priv, psk, m, keys, keys + 8);
  if (rc != WGCS_OK) return rc;
  noise_store_words(work + 4 * kHsWorkWords * (uint64_t)q, keys, kHsWorkWords);
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(&st->claim, q);
#else
  if (q < st->claim) st->claim = q;
#endif
  return WGCS_HS_FINISHED;
}

// The second pass: the final verdict of row q from the first pass's.  The authentic row that
// holds its state's claim writes both key rows and zeroes the handshake (:658-662); the other
// authentic rows are the copies the reference would meet in a state that is no longer
// handshakeInitiationCreated.  Every row's work is zeroed.
WGCS_HD int noise_finish_commit(uint32_t q, int verdict, const uint8_t* arena, const wgcs_aead_pkt* pkts,
                                const wgcs_session_slot* slots, uint32_t n_slots, wgcs_hs_state* states,
                                wgcs_aead_key* keys, uint8_t* work) {
  uint8_t* const mine = work + 4 * kHsWorkWords * (uint64_t)q;
  const uint32_t zero[kHsWorkWords] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (verdict == WGCS_HS_FINISHED) {
    uint32_t m[3];
    noise_msg_words<3>(arena + pkts[q].off, m);
    wgcs_hs_state* const st = states + session_get(slots, n_slots, m[2]);  // the row the first pass found
    if (st->claim != q) {  // a lower row's, or kHsClaimNone once that row has committed: never q
      verdict = WGCS_ERR_NO_HANDSHAKE;
    } else {
      uint32_t k[kHsWorkWords];
      noise_load_words(mine, k, kHsWorkWords);
      wgcs_aead_key* const ks = keys + st->send_key;
      wgcs_aead_key* const kr = keys + st->recv_key;
      noise_store_words(ks->key, k, 8);
      noise_store_words(kr->key, k + 8, 8);
      ks->remote_index = m[1];  // the receiver index of every transport message sealed under this key
      kr->remote_index = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) ks->pad[i] = kr->pad[i] = 0;
      st->state = WGCS_HS_STATE_ZEROED;
      st->remote_index = m[1];  // :614
      st->claim = kHsClaimNone;
      noise_store_words(st->hash, zero, 8);
      noise_store_words(st->chain_key, zero, 8);
      noise_store_words(st->ephemeral_private, zero, 8);
    }
  }
  noise_store_words(mine, zero, kHsWorkWords);
  return verdict;
}

// ---- the responder's stateful tail: wgcs_handshake_accept_batch and its host form
// (include/wgcsum.h), noise.go:458-491 for a batch judged in row order under one clock value.
// Three row functions, the same text for a lane of hs_accept_claim_kernel /
// hs_accept_verdict_kernel / hs_accept_commit_kernel (noise_accept_kernels.hip) and for the
// loops of noise.cpp.  Of a wgcs_hs_init row only peer, sender and timestamp are read.

constexpr int64_t kHandshakeInitiationRateNs = 20000000;  // HandshakeInitationRate = time.Second / 50, constants.go:33
constexpr uint32_t kHsRespNone = 0xFFFFFFFFu;             // init_row of a descriptor that holds no response

// a.After(b), tai64n.go:54: bytes.Compare over the 12 bytes, which the words hold little-endian
WGCS_HD bool noise_timestamp_after(const uint32_t a[3], const uint32_t b[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const uint32_t x = noise_bswap(a[i]), y = noise_bswap(b[i]);
    if (x != y) return x > y;
  }
  return false;
}

// the row of table and of peers that the initiation's peer id names, or WGCS_PEER_NONE
WGCS_HD uint32_t noise_accept_peer_row(const wgcs_hs_init* in, const wgcs_peer_key* table, const uint32_t* peer_rows,
                                       uint32_t n_ids, uint32_t n_peers) {
  const uint32_t peer = in->peer;
  if (peer >= n_ids) return WGCS_PEER_NONE;
  const uint32_t row = peer_rows[peer];
  if (row == WGCS_PEER_NONE || row >= n_peers || table[row].peer != peer) return WGCS_PEER_NONE;
  return row;
}

// time.Since(hs.lastInitiationConsumption) <= HandshakeInitationRate (:459) with the clock at
// now; a peer that never consumed holds Go's zero time and does not flood.  No signed overflow:
// the difference is taken only where it is positive.
WGCS_HD bool noise_accept_flooding(const wgcs_hs_peer* p, int64_t now) {
  if (!(p->flags & WGCS_HS_PEER_SEEN)) return false;
  const int64_t last = p->last_consumption_ns;
  return now <= last || (uint64_t)now - (uint64_t)last <= (uint64_t)kHandshakeInitiationRateNs;
}

// The first pass over row q: consume's verdict passed through, WGCS_ERR_NO_PEER, or
// WGCS_HS_CONSUMED for a row the second pass judges.  The peer rows are only read, but for the
// claim: a row that the peer's state at the call would accept (:458-459) takes the minimum of q
// and the claim.
WGCS_HD int noise_accept_claim(uint32_t q, const wgcs_hs_init* init, const int32_t* gate, int64_t now,
                               const wgcs_peer_key* table, const uint32_t* peer_rows, uint32_t n_ids,
                               wgcs_hs_peer* peers, uint32_t n_peers) {
  const int g = gate[q];
  if (g != WGCS_HS_CONSUMED) return g;
  const wgcs_hs_init* const in = init + q;
  const uint32_t row = noise_accept_peer_row(in, table, peer_rows, n_ids, n_peers);
  if (row == WGCS_PEER_NONE) return WGCS_ERR_NO_PEER;
  wgcs_hs_peer* const p = peers + row;
  if (!noise_accept_flooding(p, now)) {
    uint32_t ts[3], last[3];
    noise_load_words(in->timestamp, ts, 3);
    noise_load_words(p->last_timestamp, last, 3);
    if (noise_timestamp_after(ts, last)) {
#if defined(__HIP_DEVICE_COMPILE__)
      // A flood is thousands of rows of one peer: a plain look first keeps all but the low rows off the
      // atomic unit.  The claim only falls, so a stale value costs an atomic and never a claim.
      if (q < __hip_atomic_load(&p->claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&p->claim, q);
#else
      if (q < p->claim) p->claim = q;
#endif
    }
  }
  return WGCS_HS_CONSUMED;
}

// The second pass: the verdict of a row the first pass left at WGCS_HS_CONSUMED, with every
// claim final and no peer row written yet.  The row that holds its peer's claim is the one the
// reference, taking the rows in turn, accepts; behind it lastTimestamp is its timestamp and
// lastInitiationConsumption is now, so a later row is a replay (:458, tested first, :461) or
// floods (:459, :469); a row in front of it was a replay of the stored timestamp, which is below
// the winner's.  Without a winner the stored timestamp decides.
WGCS_HD int noise_accept_verdict(uint32_t q, int verdict, const wgcs_hs_init* init, uint32_t n,
                                 const uint32_t* peer_rows, const wgcs_hs_peer* peers) {
  if (verdict != WGCS_HS_CONSUMED) return verdict;
  const wgcs_hs_init* const in = init + q;
  const wgcs_hs_peer* const p = peers + peer_rows[in->peer];  // the row the first pass found
  const uint32_t claim = p->claim;
  if (claim == q) return WGCS_HS_ACCEPTED;
  uint32_t ts[3], bar[3];
  noise_load_words(in->timestamp, ts, 3);
  // a claim is a row of this call or kHsClaimNone; one the caller left behind is taken for none
  noise_load_words(claim < n ? init[claim].timestamp : p->last_timestamp, bar, 3);
  return noise_timestamp_after(ts, bar) ? WGCS_ERR_FLOOD : WGCS_ERR_REPLAY;
}

// The third pass, for a WGCS_HS_ACCEPTED row only: rank counts the winners in the rows below q.
// With a ticket the winner commits its peer's state (:474-488) and writes its descriptor;
// without one it only gives the claim back.
WGCS_HD int noise_accept_commit(uint32_t q, uint32_t rank, int64_t now, const wgcs_hs_init* init,
                                const uint32_t* peer_rows, wgcs_hs_peer* peers, const wgcs_hs_ticket* tickets,
                                uint32_t n_tickets, wgcs_hs_resp* resp) {
  const wgcs_hs_init* const in = init + q;
  const uint32_t row = peer_rows[in->peer];
  wgcs_hs_peer* const p = peers + row;
  p->claim = kHsClaimNone;
  if (rank >= n_tickets) return WGCS_ERR_BATCH_FULL;
  uint32_t ts[3], eph[8], cookie[4] = {0, 0, 0, 0};
  noise_load_words(in->timestamp, ts, 3);
  const uint32_t flags = p->flags;
  noise_store_words(p->last_timestamp, ts, 3);  // :480-482
  p->last_consumption_ns = now;                 // :483-486: now is after it, or the peer would have flooded
  p->flags = flags | WGCS_HS_PEER_SEEN;
  p->remote_index = in->sender;                 // :477
  p->state = WGCS_HS_PEER_CONSUMED;             // :487
  const wgcs_hs_ticket* const t = tickets + rank;
  wgcs_hs_resp* const r = resp + rank;
  r->init_row = q;
  r->peer_row = row;
  r->local_index = t->local_index;
  r->send_key = t->send_key;
  r->recv_key = t->recv_key;
  r->flags = (flags & WGCS_HS_PEER_COOKIE) ? WGCS_HS_RESP_COOKIE : 0;
  r->pad[0] = r->pad[1] = 0;
  noise_load_words(t->ephemeral_private, eph, 8);
  noise_store_words(r->ephemeral_private, eph, 8);
  if (flags & WGCS_HS_PEER_COOKIE) noise_load_words(p->cookie, cookie, 4);
  noise_store_words(r->cookie, cookie, 4);
  return WGCS_HS_ACCEPTED;
}

// a descriptor past the count: no response, which wgcs_handshake_respond_batch turns away unread
WGCS_HD void noise_accept_tail(wgcs_hs_resp* r) {
  const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  r->init_row = kHsRespNone;
  r->peer_row = r->local_index = r->send_key = r->recv_key = r->flags = r->pad[0] = r->pad[1] = 0;
  noise_store_words(r->ephemeral_private, zero, 8);
  noise_store_words(r->cookie, zero, 4);
}

}  // namespace wgcs
