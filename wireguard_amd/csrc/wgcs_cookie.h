// wgcs_cookie.h -- the scalar steps of the reference's cookie checker and
// generator (device/cookie.go), shared by hs_screen_kernel (cookie_kernels.hip),
// the host functions of cookie_api.cpp and tests/cookie_host/cookie_host.cpp.
//
// A handshake message of len bytes ends with two 16-byte fields: MAC1 at
// [len - 32, len - 16) and MAC2 at [len - 16, len).
//   MAC1   = BLAKE2s-128(key = mac1_key,  msg[0 : len - 32])     cookie.go:142-145
//   cookie = BLAKE2s-128(key = secret,    source address bytes)  :162-165
//   MAC2   = BLAKE2s-128(key = cookie,    msg[0 : len - 16])     :171-175
// Keys, MACs and the cookie are little-endian words; messages are byte
// pointers at any alignment.
#pragma once

#include <stdint.h>

#include "wgcs_blake2s.h"
#include "wgcs_xchacha.h"

namespace wgcs {

constexpr uint32_t kMacSize = 16;         // blake2s.Size128
constexpr uint32_t kCookieReplyType = 3;  // MessageCookieReplyType, device/noise.go

// 16 bytes at any alignment as words
WGCS_HD void cookie_load16(const uint8_t* p, uint32_t w[4]) {
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) w[i] = b2s_load_le32(p, 4 * i, 16);
}

WGCS_HD void cookie_store16(uint8_t* p, const uint32_t w[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) b2s_store_le32(p + 4 * i, w[i]);
}

// BLAKE2s-128 of msg[0, n) under a key of key_len bytes (16 or 32)
WGCS_HD void cookie_mac128(const uint32_t key[8], uint32_t key_len, const uint8_t* msg, uint32_t n, uint32_t mac[4]) {
  uint32_t h[8];
  blake2s_words(key, key_len, msg, n, kMacSize, h);
#pragma unroll
  for (int i = 0; i < 4; ++i) mac[i] = h[i];
}

// CheckMAC1 (cookie.go:121-146), len >= 32
WGCS_HD bool cookie_mac1_ok(const uint32_t mac1_key[8], const uint8_t* msg, uint32_t len) {
  uint32_t mac[4], field[4];
  cookie_mac128(mac1_key, 32, msg, len - 2 * kMacSize, mac);
  cookie_load16(msg + (len - 2 * kMacSize), field);
  return tag16_equal(mac, field);
}

// the cookie of a source address (cookie.go:160-166, :205-215)
WGCS_HD void cookie_of_source(const uint32_t secret[8], const uint8_t* src, uint32_t src_len, uint32_t cookie[4]) {
  cookie_mac128(secret, 32, src, src_len, cookie);
}

// the MAC2 comparison of CheckMAC2 (cookie.go:167-175) under a cookie, len >= 32
WGCS_HD bool cookie_mac2_ok(const uint32_t cookie[4], const uint8_t* msg, uint32_t len) {
  const uint32_t key[8] = {cookie[0], cookie[1], cookie[2], cookie[3], 0, 0, 0, 0};
  uint32_t mac[4], field[4];
  cookie_mac128(key, 16, msg, len - kMacSize, mac);
  cookie_load16(msg + (len - kMacSize), field);
  return tag16_equal(mac, field);
}

// The MessageCookieReply of CreateReply (cookie.go:204-242, send.go:176-187)
// as sixteen words: type 3, the sender index msg[4:8] as the receiver, the
// nonce, and the cookie sealed with the message's MAC1 as additional data.
WGCS_HD void cookie_reply_words(const uint32_t cookie_key[8], const uint32_t cookie[4], const uint8_t* msg, uint32_t len,
                                const uint32_t nonce[6], uint32_t reply[16]) {
  uint32_t ad[4];
  cookie_load16(msg + (len - 2 * kMacSize), ad);
  reply[0] = kCookieReplyType;
  reply[1] = b2s_load_le32(msg, 4, len);
#pragma unroll
  for (int i = 0; i < 6; ++i) reply[2 + i] = nonce[i];
  xchacha_seal16(cookie_key, nonce, cookie, ad, reply + 8, reply + 12);
}

}  // namespace wgcs
