// noise_resp_host.cpp -- drives the response half of wireguard_amd/csrc/wgcs_noise.h
// and the host functions wgcs_noise_create_response / wgcs_noise_consume_response of
// noise.cpp, the scalar code the lanes of hs_respond_kernel run, as plain host code
// (built by tests/test_noise_resp_host.py with -fsanitize=address,undefined together
// with noise.cpp).
//
// Every input is copied into a heap buffer of exactly its size, and every output is
// a heap buffer of exactly its size filled with 0xEE, so a read or a write past
// either end is a sanitizer report.
//
// stdin, one case per line, hex fields ("-" = absent: a NULL pointer):
//   mac1key <public:32B>                                  noise_mac1_key           -> 32 bytes
//   core <hash:32B> <chain:32B> <remote eph:32B> <remote static:32B> <psk:32B> <ephemeral:32B>
//        <local:4B LE> <remote:4B LE>                     noise_create_response    -> rc:the 60 bytes | send | recv
//   write <m:60B> <mac1 key:32B> <cookie:16B|->           noise_write_response     -> the 92 bytes
//   respond <init:128B> <remote static:32B> <psk:32B|-> <ephemeral:32B> <local:4B LE> <cookie:16B|->
//                                                         wgcs_noise_create_response   -> rc:msg | send | recv
//   consume <static:32B> <hash:32B> <chain:32B> <ephemeral:32B> <psk:32B|-> <local:4B LE> <msg>
//                                                         wgcs_noise_consume_response  -> rc:sender (4B LE) | send | recv
// stdout: one line per case, then "noise_resp_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/wgcsum.h"
#include "wgcs_noise.h"

using namespace wgcs;

// a heap copy of exactly the bytes given; p stays NULL for none
struct Exact {
  std::unique_ptr<uint8_t[]> mem;
  uint8_t* p = nullptr;
  size_t n = 0;
  Exact(const std::vector<uint8_t>& v) : n(v.size()) {
    if (n == 0) return;
    mem.reset(new uint8_t[n]);
    p = mem.get();
    memcpy(p, v.data(), n);
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

// the bytes of e as n_words zero-padded words: never a byte past e.n is read
static void words(const Exact& e, uint32_t n_words, uint32_t* w) {
  for (uint32_t i = 0; i < n_words; ++i) w[i] = b2s_load_le32(e.p, 4 * i, (uint32_t)e.n);
}

static void print_words(const uint32_t* w, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 4; ++j) printf("%02x", (w[i] >> (8 * j)) & 0xFF);
}

static std::vector<uint8_t> filled(size_t n) { return std::vector<uint8_t>(n, 0xEE); }

static bool sized(const std::vector<std::vector<uint8_t>>& f, std::initializer_list<size_t> sizes) {
  if (f.size() != sizes.size()) return false;
  size_t i = 0;
  for (size_t s : sizes)
    if (f[i++].size() != s) return false;
  return true;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    std::vector<std::vector<uint8_t>> f;
    for (std::string t; in >> t;) f.push_back(unhex(t));
    if (op == "mac1key" && sized(f, {32})) {
      uint32_t pub[8], key[8];
      words(Exact(f[0]), 8, pub);
      noise_mac1_key(pub, key);
      print_words(key, 8);
    } else if (op == "core" && sized(f, {32, 32, 32, 32, 32, 32, 4, 4})) {
      uint32_t a[6][8], m[kNoiseResponseBodyWords], send[8], recv[8];
      for (int i = 0; i < 6; ++i) words(Exact(f[i]), 8, a[i]);
      const uint32_t local = b2s_load_le32(Exact(f[6]).p, 0, 4), remote = b2s_load_le32(Exact(f[7]).p, 0, 4);
      for (uint32_t i = 0; i < kNoiseResponseBodyWords; ++i) m[i] = 0xEEEEEEEEu;
      for (int i = 0; i < 8; ++i) send[i] = recv[i] = 0xEEEEEEEEu;
      printf("%d:", noise_create_response(a[0], a[1], a[2], a[3], a[4], a[5], local, remote, m, send, recv));
      print_words(m, kNoiseResponseBodyWords);
      print_words(send, 8);
      print_words(recv, 8);
    } else if (op == "write" && f.size() == 3 && f[0].size() == 60 && f[1].size() == 32 &&
               (f[2].empty() || f[2].size() == 16)) {
      uint32_t m[kNoiseResponseBodyWords], key[8], cookie[4];
      words(Exact(f[0]), kNoiseResponseBodyWords, m);
      words(Exact(f[1]), 8, key);
      words(Exact(f[2]), 4, cookie);
      const Exact msg(filled(kNoiseResponseSize));
      noise_write_response(msg.p, m, key, !f[2].empty(), cookie);
      print_hex(msg.p, msg.n);
    } else if (op == "respond" && f.size() == 6 && f[0].size() == sizeof(wgcs_hs_init) && f[1].size() == 32 &&
               (f[2].empty() || f[2].size() == 32) && f[3].size() == 32 && f[4].size() == 4 &&
               (f[5].empty() || f[5].size() == 16)) {
      std::unique_ptr<wgcs_hs_init> init(new wgcs_hs_init);  // memory of its own type, exactly one row
      memcpy(init.get(), f[0].data(), sizeof(wgcs_hs_init));
      const Exact remote(f[1]), psk(f[2]), eph(f[3]), cookie(f[5]), msg(filled(kNoiseResponseSize)), send(filled(32)),
          recv(filled(32));
      const uint32_t local = b2s_load_le32(Exact(f[4]).p, 0, 4);
      const int rc = wgcs_noise_create_response(init.get(), remote.p, psk.p, eph.p, local, cookie.p, msg.p, send.p, recv.p);
      // the optional outputs may be NULL: the message must not change
      const Exact again(filled(kNoiseResponseSize));
      if (wgcs_noise_create_response(init.get(), remote.p, psk.p, eph.p, local, cookie.p, again.p, nullptr, nullptr) != rc ||
          memcmp(again.p, msg.p, kNoiseResponseSize) != 0)
        return 3;
      printf("%d:", rc);
      print_hex(msg.p, msg.n);
      print_hex(send.p, 32);
      print_hex(recv.p, 32);
    } else if (op == "consume" && f.size() == 7 && f[0].size() == 32 && f[1].size() == 32 && f[2].size() == 32 &&
               f[3].size() == 32 && (f[4].empty() || f[4].size() == 32) && f[5].size() == 4) {
      const Exact sk(f[0]), hash(f[1]), chain(f[2]), eph(f[3]), psk(f[4]), msg(f[6]), send(filled(32)), recv(filled(32));
      const uint32_t local = b2s_load_le32(Exact(f[5]).p, 0, 4);
      std::unique_ptr<uint32_t> sender(new uint32_t(0xEEEEEEEEu));
      const int rc = wgcs_noise_consume_response(sk.p, hash.p, chain.p, eph.p, psk.p, local, msg.p, msg.n, sender.get(),
                                                 send.p, recv.p);
      if (wgcs_noise_consume_response(sk.p, hash.p, chain.p, eph.p, psk.p, local, msg.p, msg.n, nullptr, nullptr,
                                      nullptr) != rc)
        return 3;
      printf("%d:", rc);
      print_words(sender.get(), 1);
      print_hex(send.p, 32);
      print_hex(recv.p, 32);
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("noise_resp_host: ok\n");
  return 0;
}
