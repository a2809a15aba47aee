// cookie.cpp -- the host functions of the handshake screen (include/wgcsum.h),
// no context and no device:
//   wgcs_cookie_checker_init / _check_mac1 / _check_mac2 / _create_reply
//                                  CookieChecker                  device/cookie.go:87-243
//   wgcs_cookie_add_macs / _consume_reply
//                                  CookieGenerator                cookie.go:247-339
// They run the scalar code of wgcs_cookie.h, the code the lanes of
// hs_screen_kernel (cookie_kernels.hip) run.  Plain C++: a host test program
// (tests/cookie_host/cookie_host.cpp) links this file as it is.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // the library's build compiles every file as HIP: WGCS_HD's qualifiers
#endif

#include <string.h>

#include "../../include/wgcsum.h"
#include "wgcs_cookie.h"

using namespace wgcs;

namespace {

constexpr size_t kMaxMessage = 65535;

int check_len(size_t len) { return len < 2 * kMacSize || len > kMaxMessage ? WGCS_ERR_OUT_OF_RANGE : WGCS_OK; }

bool src_ok(const wgcs_src_addr* src) { return src && (src->len == 6 || src->len == 18); }

// BLAKE2s-256(label | pub), cookie.go:106-114
void label_key(const char label[8], const uint8_t pub[32], uint8_t out[32]) {
  uint8_t in[40];
  memcpy(in, label, 8);
  memcpy(in + 8, pub, 32);
  blake2s_bytes(nullptr, 0, in, sizeof in, 32, out);
}

}  // namespace

extern "C" {

int wgcs_cookie_checker_init(wgcs_cookie_checker* ck, const uint8_t pub[32]) {
  if (!ck || !pub) return WGCS_ERR_INVALID_ARG;
  label_key("mac1----", pub, ck->mac1_key);      // WGLabelMAC1
  label_key("cookie--", pub, ck->cookie_key);    // WGLabelCookie
  memset(ck->secret, 0, sizeof ck->secret);
  return WGCS_OK;
}

int wgcs_cookie_check_mac1(const wgcs_cookie_checker* ck, const uint8_t* msg, size_t len) {
  if (!ck || !msg) return WGCS_ERR_INVALID_ARG;
  if (int rc = check_len(len)) return rc;
  uint32_t key[8];
  b2s_key_words(ck->mac1_key, 32, key);
  return cookie_mac1_ok(key, msg, (uint32_t)len) ? 1 : 0;
}

int wgcs_cookie_check_mac2(const wgcs_cookie_checker* ck, const uint8_t* msg, size_t len, const wgcs_src_addr* src) {
  if (!ck || !msg || !src_ok(src)) return WGCS_ERR_INVALID_ARG;
  if (int rc = check_len(len)) return rc;
  uint32_t secret[8], cookie[4];
  b2s_key_words(ck->secret, 32, secret);
  cookie_of_source(secret, src->b, src->len, cookie);
  return cookie_mac2_ok(cookie, msg, (uint32_t)len) ? 1 : 0;
}

int wgcs_cookie_create_reply(const wgcs_cookie_checker* ck, const uint8_t* msg, size_t len, const wgcs_src_addr* src,
                             const uint8_t nonce[24], uint8_t out[64]) {
  if (!ck || !msg || !nonce || !out || !src_ok(src)) return WGCS_ERR_INVALID_ARG;
  if (int rc = check_len(len)) return rc;
  uint32_t key[8], cookie[4], nw[6], reply[16];
  b2s_key_words(ck->secret, 32, key);
  cookie_of_source(key, src->b, src->len, cookie);
  b2s_key_words(ck->cookie_key, 32, key);
  for (uint32_t i = 0; i < 6; ++i) nw[i] = b2s_load_le32(nonce, 4 * i, 24);
  cookie_reply_words(key, cookie, msg, (uint32_t)len, nw, reply);
  for (int i = 0; i < 16; ++i) b2s_store_le32(out + 4 * i, reply[i]);
  return WGCS_OK;
}

int wgcs_cookie_add_macs(const uint8_t mac1_key[32], const uint8_t* cookie, uint8_t* msg, size_t len,
                         uint8_t* last_mac1) {
  if (!mac1_key || !msg) return WGCS_ERR_INVALID_ARG;
  if (int rc = check_len(len)) return rc;
  uint32_t key[8], mac[4];
  b2s_key_words(mac1_key, 32, key);
  cookie_mac128(key, 32, msg, (uint32_t)len - 2 * kMacSize, mac);  // cookie.go:296-300
  cookie_store16(msg + len - 2 * kMacSize, mac);
  if (last_mac1) cookie_store16(last_mac1, mac);  // :301-302
  if (!cookie) return WGCS_OK;                    // :306-308
  b2s_key_words(cookie, 16, key);
  cookie_mac128(key, 16, msg, (uint32_t)len - kMacSize, mac);  // :309-313
  cookie_store16(msg + len - kMacSize, mac);
  return WGCS_OK;
}

int wgcs_cookie_consume_reply(const uint8_t cookie_key[32], const uint8_t last_mac1[16], const uint8_t reply[64],
                              uint8_t cookie[16]) {
  if (!cookie_key || !last_mac1 || !reply || !cookie) return WGCS_ERR_INVALID_ARG;
  uint32_t key[8], nw[6], ct[4], tag[4], ad[4], pt[4];
  b2s_key_words(cookie_key, 32, key);
  for (uint32_t i = 0; i < 6; ++i) nw[i] = b2s_load_le32(reply, 8 + 4 * i, 64);
  cookie_load16(reply + 32, ct);
  cookie_load16(reply + 48, tag);
  cookie_load16(last_mac1, ad);
  if (!xchacha_open16(key, nw, ct, tag, ad, pt)) return 0;  // cookie.go:333-335
  cookie_store16(cookie, pt);
  return 1;
}

}  // extern "C"
