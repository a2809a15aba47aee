// cookie_host.cpp -- drives wireguard_amd/csrc/wgcs_blake2s.h, wgcs_xchacha.h
// and the host functions of cookie.cpp, the scalar code the lanes of
// hs_screen_kernel run, as plain host code (built by tests/test_cookie_host.py
// with -fsanitize=address,undefined together with cookie.cpp).
//
// Every input is copied into a heap buffer of exactly its size (at byte offset
// `shift` of a buffer of size + shift where a case gives one), so a read past
// either end is a sanitizer report.
//
// stdin, one case per line, hex fields ("-" = empty):
//   b2s <key|-> <outlen> <shift> <msg|->        BLAKE2s               -> digest
//   hch <key:32B> <nonce:16B>                   HChaCha20             -> 32 bytes
//   seal <key:32B> <nonce:24B> <pt:16B> <ad:16B>                      -> ct | tag
//   open <key:32B> <nonce:24B> <ct|tag:32B> <ad:16B>                  -> pt, or "fail"
//   init <pub:32B>                              checker_init          -> the 96 bytes
//   mac1 <checker:96B> <msg>                    check_mac1            -> status
//   mac2 <checker:96B> <src> <msg>              check_mac2            -> status
//   reply <checker:96B> <src> <nonce:24B> <msg> create_reply          -> 64 bytes, or the status
//   add <mac1_key:32B> <cookie|-> <msg>         add_macs              -> msg | last_mac1, or the status
//   consume <cookie_key:32B> <mac1:16B> <reply:64B>  consume_reply    -> cookie, or "fail"
// stdout: one line per case, then "cookie_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_blake2s.h"
#include "wgcs_xchacha.h"

using namespace wgcs;

// a heap copy of exactly the bytes given, `shift` bytes into its allocation
struct Exact {
  std::unique_ptr<uint8_t[]> mem;
  uint8_t* p = nullptr;
  size_t n = 0;
  Exact(const std::vector<uint8_t>& v, size_t shift = 0) : n(v.size()) {
    if (n + shift == 0) return;
    mem.reset(new uint8_t[n + shift]);
    p = mem.get() + shift;
    if (n) memcpy(p, v.data(), n);
  }
};

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

static void print_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}

static void words(const uint8_t* p, int n, uint32_t* w) {
  for (int i = 0; i < n; ++i) w[i] = b2s_load_le32(p, 4 * (uint32_t)i, 4 * (uint32_t)n);
}

static void print_words(const uint32_t* w, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 4; ++j) printf("%02x", (w[i] >> (8 * j)) & 0xFF);
}

static wgcs_src_addr src_of(const std::vector<uint8_t>& b) {
  wgcs_src_addr s;
  memset(&s, 0, sizeof s);
  if (!b.empty()) memcpy(s.b, b.data(), b.size() < sizeof s.b ? b.size() : sizeof s.b);
  s.len = (uint8_t)b.size();
  return s;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    std::vector<std::vector<uint8_t>> f;
    std::vector<std::string> raw;
    for (std::string t; in >> t;) raw.push_back(t);
    if (op == "b2s") {
      if (raw.size() != 4) return 2;
      const Exact key(unhex(raw[0])), msg(unhex(raw[3]), std::stoul(raw[2]));
      const uint32_t out_len = (uint32_t)std::stoul(raw[1]);
      const Exact out{std::vector<uint8_t>(out_len)};
      blake2s_bytes(key.p, (uint32_t)key.n, msg.n ? msg.p : nullptr, (uint32_t)msg.n, out_len, out.p);
      print_hex(out.p, out_len);
    } else {
      for (const std::string& t : raw) f.push_back(unhex(t));
      if (op == "hch" && f.size() == 2 && f[0].size() == 32 && f[1].size() == 16) {
        uint32_t k[8], nw[4], o[8];
        words(Exact(f[0]).p, 8, k);
        words(Exact(f[1]).p, 4, nw);
        hchacha20(k, nw, o);
        print_words(o, 8);
      } else if ((op == "seal" || op == "open") && f.size() == 4 && f[0].size() == 32 && f[1].size() == 24 &&
                 f[2].size() == (op == "seal" ? 16u : 32u) && f[3].size() == 16) {
        uint32_t k[8], nw[6], a[8], ad[4], ct[4], tag[4];
        words(Exact(f[0]).p, 8, k);
        words(Exact(f[1]).p, 6, nw);
        words(Exact(f[2]).p, (int)f[2].size() / 4, a);
        words(Exact(f[3]).p, 4, ad);
        if (op == "seal") {
          xchacha_seal16(k, nw, a, ad, ct, tag);
          print_words(ct, 4);
          print_words(tag, 4);
        } else if (xchacha_open16(k, nw, a, a + 4, ad, ct)) {
          print_words(ct, 4);
        } else {
          printf("fail");
        }
      } else if (op == "init" && f.size() == 1 && f[0].size() == 32) {
        const Exact pub(f[0]), ck(std::vector<uint8_t>(sizeof(wgcs_cookie_checker), 0xEE));
        if (wgcs_cookie_checker_init((wgcs_cookie_checker*)ck.p, pub.p) != WGCS_OK) return 3;
        print_hex(ck.p, ck.n);
      } else if (op == "mac1" && f.size() == 2 && f[0].size() == 96) {
        const Exact ck(f[0]), msg(f[1]);
        printf("%d", wgcs_cookie_check_mac1((const wgcs_cookie_checker*)ck.p, msg.p, msg.n));
      } else if (op == "mac2" && f.size() == 3 && f[0].size() == 96) {
        const Exact ck(f[0]), msg(f[2]);
        const wgcs_src_addr s = src_of(f[1]);
        printf("%d", wgcs_cookie_check_mac2((const wgcs_cookie_checker*)ck.p, msg.p, msg.n, &s));
      } else if (op == "reply" && f.size() == 4 && f[0].size() == 96 && f[2].size() == 24) {
        const Exact ck(f[0]), nonce(f[2]), msg(f[3]), out{std::vector<uint8_t>(64)};
        const wgcs_src_addr s = src_of(f[1]);
        const int rc = wgcs_cookie_create_reply((const wgcs_cookie_checker*)ck.p, msg.p, msg.n, &s, nonce.p, out.p);
        if (rc == WGCS_OK) print_hex(out.p, 64);
        else printf("%d", rc);
      } else if (op == "add" && f.size() == 3 && f[0].size() == 32) {
        const Exact key(f[0]), cookie(f[1]), msg(f[2]), last{std::vector<uint8_t>(16)};
        const int rc = wgcs_cookie_add_macs(key.p, cookie.n ? cookie.p : nullptr, msg.p, msg.n, last.p);
        if (rc == WGCS_OK) {
          print_hex(msg.p, msg.n);
          print_hex(last.p, 16);
        } else {
          printf("%d", rc);
        }
      } else if (op == "consume" && f.size() == 3 && f[0].size() == 32 && f[1].size() == 16 && f[2].size() == 64) {
        const Exact key(f[0]), mac1(f[1]), reply(f[2]), out{std::vector<uint8_t>(16)};
        const int rc = wgcs_cookie_consume_reply(key.p, mac1.p, reply.p, out.p);
        if (rc == 1) print_hex(out.p, 16);
        else if (rc == 0) printf("fail");
        else printf("%d", rc);
      } else {
        return 2;
      }
    }
    printf("\n");
  }
  printf("cookie_host: ok\n");
  return 0;
}
