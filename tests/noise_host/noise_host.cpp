// noise_host.cpp -- drives wireguard_amd/csrc/wgcs_x25519.h, wgcs_noise.h and
// the host functions of noise.cpp, the scalar code the lanes of
// noise_kernels.hip run, as plain host code (built by tests/test_noise_host.py
// with -fsanitize=address,undefined together with noise.cpp).
//
// Every input is copied into a heap buffer of exactly its size, so a read past
// either end is a sanitizer report.
//
// stdin, one case per line, hex fields ("-" = empty):
//   x <scalar:32B> <point:32B>                  wgcs_x25519           -> 32 bytes, or "low" (out zeroed)
//   xiter <count>                               k, u = X25519(k, u), k from k = u = 9   -> k
//   hmac <key:32B> <in:0..64B|->                HMAC1                 -> 32 bytes
//   hmac2 <key:32B> <in0:32B> <in1:1B>          HMAC2                 -> 32 bytes
//   kdf1 | kdf2 | kdf3 <key:32B> <in:0..64B|->  KDF1 / KDF2 / KDF3    -> t0 [| t1 [| t2]]
//   mixhash <h:32B> <data:0..48B|->             mixHash               -> 32 bytes
//   seal <key:32B> <pt:0|12|32B|-> <ad:32B>     the handshake's AEAD  -> ct | tag
//   open <key:32B> <ct|tag> <ad:32B>                                  -> pt ("-" if empty), or "fail"
//   init <private:32B>                          responder_init        -> the 96 bytes | public key
//   build <responder:96B> <keys|-> <peers|-> <flags|->  peer_keys_build  -> the table ("-" if empty), or the status
//   find <table|-> <key:32B>                    peer_keys_find        -> row
//   consume <responder:96B> <table|-> <msg>     consume_initiation    -> verdict:the 128 bytes (0xEE-filled before)
//   create <static:32B> <remote:32B> <ephemeral:32B> <timestamp:12B> <sender:4B LE>
//                                               create_initiation     -> msg | hash | chain key, or the status
// stdout: one line per case, then "noise_host: ok".
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

// a heap copy of exactly the bytes given
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
  if (n == 0) printf("-");
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

// a table's rows in memory of their own type (4-byte aligned, exactly n rows)
static std::unique_ptr<wgcs_peer_key[]> table_of(const std::vector<uint8_t>& b) {
  const size_t n = b.size() / sizeof(wgcs_peer_key);
  std::unique_ptr<wgcs_peer_key[]> t(n ? new wgcs_peer_key[n] : nullptr);
  if (n) memcpy(t.get(), b.data(), n * sizeof(wgcs_peer_key));
  return t;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    std::vector<std::string> raw;
    for (std::string t; in >> t;) raw.push_back(t);
    if (op == "xiter") {
      if (raw.size() != 1) return 2;
      const Exact k(std::vector<uint8_t>(32, 0)), u(std::vector<uint8_t>(32, 0)), r(std::vector<uint8_t>(32, 0));
      k.p[0] = u.p[0] = 9;
      for (unsigned long i = 0, n = std::stoul(raw[0]); i < n; ++i) {
        if (wgcs_x25519(r.p, k.p, u.p) != WGCS_OK) return 3;
        memcpy(u.p, k.p, 32);
        memcpy(k.p, r.p, 32);
      }
      print_hex(k.p, 32);
      printf("\n");
      continue;
    }
    std::vector<std::vector<uint8_t>> f;
    for (const std::string& t : raw) f.push_back(unhex(t));
    if (op == "x" && f.size() == 2 && f[0].size() == 32 && f[1].size() == 32) {
      const Exact k(f[0]), u(f[1]), out(std::vector<uint8_t>(32, 0xEE));
      const int rc = wgcs_x25519(out.p, k.p, u.p);
      bool zero = true;
      for (int i = 0; i < 32; ++i) zero = zero && out.p[i] == 0;
      if (rc == WGCS_OK && !zero) print_hex(out.p, 32);
      else if (rc == WGCS_ERR_LOW_ORDER && zero) printf("low");
      else return 3;
    } else if (op == "hmac" && f.size() == 2 && f[0].size() == 32 && f[1].size() <= 64) {
      uint32_t key[8], data[16], out[8];
      words(Exact(f[0]), 8, key);
      words(Exact(f[1]), 16, data);
      noise_hmac1(key, data, (uint32_t)f[1].size(), out);
      print_words(out, 8);
    } else if (op == "hmac2" && f.size() == 3 && f[0].size() == 32 && f[1].size() == 32 && f[2].size() == 1) {
      uint32_t key[8], in0[8], out[8];
      words(Exact(f[0]), 8, key);
      words(Exact(f[1]), 8, in0);
      noise_hmac2(key, in0, Exact(f[2]).p[0], out);
      print_words(out, 8);
    } else if ((op == "kdf1" || op == "kdf2" || op == "kdf3") && f.size() == 2 && f[0].size() == 32 &&
               f[1].size() <= 64) {
      uint32_t key[8], data[16], t0[8], t1[8], t2[8];
      words(Exact(f[0]), 8, key);
      words(Exact(f[1]), 16, data);
      const uint32_t len = (uint32_t)f[1].size();
      if (op == "kdf1") {
        noise_kdf1(t0, key, data, len);
        print_words(t0, 8);
      } else if (op == "kdf2") {
        noise_kdf2(t0, t1, key, data, len);
        print_words(t0, 8);
        print_words(t1, 8);
      } else {
        noise_kdf3(t0, t1, t2, key, data, len);
        print_words(t0, 8);
        print_words(t1, 8);
        print_words(t2, 8);
      }
    } else if (op == "mixhash" && f.size() == 2 && f[0].size() == 32 && f[1].size() <= 48) {
      uint32_t h[8], data[12];
      words(Exact(f[0]), 8, h);
      words(Exact(f[1]), 12, data);
      noise_mix_hash(h, data, (uint32_t)f[1].size());
      print_words(h, 8);
    } else if (op == "seal" && f.size() == 3 && f[0].size() == 32 && f[1].size() <= 32 && f[1].size() % 4 == 0 &&
               f[2].size() == 32) {
      uint32_t key[8], pt[8], ad[8], ct[8], tag[4];
      words(Exact(f[0]), 8, key);
      words(Exact(f[1]), 8, pt);
      words(Exact(f[2]), 8, ad);
      noise_seal(key, pt, (uint32_t)f[1].size(), ad, ct, tag);
      if (!f[1].empty()) print_words(ct, (int)f[1].size() / 4);
      print_words(tag, 4);
    } else if (op == "open" && f.size() == 3 && f[0].size() == 32 && f[1].size() >= 16 && f[1].size() <= 48 &&
               f[1].size() % 4 == 0 && f[2].size() == 32) {
      const uint32_t n = (uint32_t)f[1].size() - 16;
      uint32_t key[8], ct[8], tag[4], ad[8], pt[8];
      words(Exact(f[0]), 8, key);
      words(Exact(std::vector<uint8_t>(f[1].begin(), f[1].begin() + n)), 8, ct);
      words(Exact(std::vector<uint8_t>(f[1].begin() + n, f[1].end())), 4, tag);
      words(Exact(f[2]), 8, ad);
      if (!noise_open(key, ct, n, tag, ad, pt)) printf("fail");
      else if (n == 0) printf("-");
      else print_words(pt, (int)n / 4);
    } else if (op == "init" && f.size() == 1 && f[0].size() == 32) {
      const Exact priv(f[0]), r(std::vector<uint8_t>(sizeof(wgcs_noise_responder), 0xEE)),
          pub(std::vector<uint8_t>(32, 0xEE));
      if (wgcs_noise_responder_init((wgcs_noise_responder*)r.p, priv.p, pub.p) != WGCS_OK) return 3;
      if (wgcs_noise_responder_init((wgcs_noise_responder*)r.p, priv.p, nullptr) != WGCS_OK) return 3;
      print_hex(r.p, r.n);
      print_hex(pub.p, 32);
    } else if (op == "build" && f.size() == 4 && f[0].size() == 96 && f[1].size() % 32 == 0 &&
               f[2].size() == f[1].size() / 8 && (f[3].empty() || f[3].size() == f[2].size())) {
      const uint32_t n = (uint32_t)f[1].size() / 32;
      const Exact r(f[0]), keys(f[1]);
      std::unique_ptr<uint32_t[]> peers(n ? new uint32_t[n] : nullptr), flags(f[3].empty() ? nullptr : new uint32_t[n]);
      if (n) memcpy(peers.get(), f[2].data(), 4 * (size_t)n);
      if (flags) memcpy(flags.get(), f[3].data(), 4 * (size_t)n);
      std::unique_ptr<wgcs_peer_key[]> table(n ? new wgcs_peer_key[n] : nullptr);
      if (n) memset(table.get(), 0xEE, n * sizeof(wgcs_peer_key));
      const int rc = wgcs_peer_keys_build((const wgcs_noise_responder*)r.p, keys.p, peers.get(), flags.get(), n,
                                          table.get());
      if (rc == WGCS_OK) print_hex((const uint8_t*)table.get(), n * sizeof(wgcs_peer_key));
      else printf("%d", rc);
    } else if (op == "find" && f.size() == 2 && f[0].size() % sizeof(wgcs_peer_key) == 0 && f[1].size() == 32) {
      const std::unique_ptr<wgcs_peer_key[]> table = table_of(f[0]);
      const Exact key(f[1]);
      printf("%d", wgcs_peer_keys_find(table.get(), (uint32_t)(f[0].size() / sizeof(wgcs_peer_key)), key.p));
    } else if (op == "consume" && f.size() == 3 && f[0].size() == 96 && f[1].size() % sizeof(wgcs_peer_key) == 0) {
      const std::unique_ptr<wgcs_peer_key[]> table = table_of(f[1]);
      const Exact r(f[0]), msg(f[2]);
      std::unique_ptr<wgcs_hs_init> out(new wgcs_hs_init);
      memset(out.get(), 0xEE, sizeof(wgcs_hs_init));
      const int rc = wgcs_noise_consume_initiation((const wgcs_noise_responder*)r.p, table.get(),
                                                   (uint32_t)(f[1].size() / sizeof(wgcs_peer_key)), msg.p, msg.n,
                                                   out.get());
      printf("%d:", rc);
      print_hex((const uint8_t*)out.get(), sizeof(wgcs_hs_init));
    } else if (op == "create" && f.size() == 5 && f[0].size() == 32 && f[1].size() == 32 && f[2].size() == 32 &&
               f[3].size() == 12 && f[4].size() == 4) {
      const Exact sk(f[0]), remote(f[1]), ek(f[2]), ts(f[3]), msg(std::vector<uint8_t>(148, 0xEE)),
          hash(std::vector<uint8_t>(32, 0xEE)), chain(std::vector<uint8_t>(32, 0xEE));
      const uint32_t sender = b2s_load_le32(Exact(f[4]).p, 0, 4);
      const int rc = wgcs_noise_create_initiation(sk.p, remote.p, ek.p, ts.p, sender, msg.p, hash.p, chain.p);
      if (rc == WGCS_OK) {
        print_hex(msg.p, 148);
        print_hex(hash.p, 32);
        print_hex(chain.p, 32);
      } else {
        printf("%d", rc);
      }
    } else {
      return 2;
    }
    printf("\n");
  }
  printf("noise_host: ok\n");
  return 0;
}
