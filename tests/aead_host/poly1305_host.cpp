// poly1305_host.cpp -- drives wireguard_amd/csrc/wgcs_poly1305.h, the limb
// arithmetic the gfx950 AEAD kernel runs, as plain host code (built by
// tests/test_poly1305_host.py with -fsanitize=address,undefined).
//
// stdin, one case per line, hex fields ("-" = empty):
//   mac <key:32B> <msg>        serial Horner, acc = (acc + m) * r per block
//   row <key:32B> <msg>        the kernel's schedule: block k on lane k & 15,
//                              acc = acc * r^16 + m, combined with powers of r
//   fin <l0> <l1> <l2> <l3> <l4> <s:16B>   p1305_finish on raw limbs (hex u32)
// stdout: one 16-byte tag in hex per case, then "poly1305_host: ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "wgcs_poly1305.h"

using namespace wgcs;

static std::vector<uint8_t> unhex(const std::string& s) {
  std::vector<uint8_t> out;
  if (s == "-") return out;
  for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
  return out;
}

static uint32_t le32(const uint8_t* p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// Block k of msg as the kernel presents it: words with the bytes beyond the
// message zero, and the number of bytes.
static P1305 block(const std::vector<uint8_t>& msg, size_t k) {
  uint8_t b[16] = {0};
  const size_t n = msg.size() - 16 * k < 16 ? msg.size() - 16 * k : 16;
  memcpy(b, msg.data() + 16 * k, n);
  return p1305_block(le32(b), le32(b + 4), le32(b + 8), le32(b + 12), (int)n);
}

static void print_tag(const uint32_t tag[4]) {
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) printf("%02x", (tag[i] >> (8 * j)) & 0xFF);
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    if (!(in >> op)) continue;
    uint32_t tag[4];
    if (op == "fin") {
      P1305 h;
      std::string f;
      for (int i = 0; i < 5; ++i) {
        in >> f;
        h.l[i] = (uint32_t)std::stoul(f, nullptr, 16);
      }
      in >> f;
      const std::vector<uint8_t> s = unhex(f);
      if (s.size() != 16) return 2;
      p1305_finish(h, le32(&s[0]), le32(&s[4]), le32(&s[8]), le32(&s[12]), tag);
      print_tag(tag);
      continue;
    }
    std::string kh, mh;
    in >> kh >> mh;
    const std::vector<uint8_t> key = unhex(kh), msg = unhex(mh);
    if (key.size() != 32) return 2;
    const P1305 r = p1305_clamp_r(le32(&key[0]), le32(&key[4]), le32(&key[8]), le32(&key[12]));
    const size_t nblk = (msg.size() + 15) / 16;
    P1305 h = p1305_zero();
    if (op == "mac") {
      for (size_t k = 0; k < nblk; ++k) h = p1305_mul(p1305_add(h, block(msg, k)), r);
    } else if (op == "row") {
      P1305 acc[16], rpow[16], r16 = p1305_zero();
      for (int lane = 0; lane < 16; ++lane) {
        acc[lane] = p1305_zero();
        rpow[lane] = p1305_pow_1_16(r, p1305_lane_exponent((uint32_t)nblk, lane), &r16);
      }
      for (size_t k = 0; k < nblk; ++k) acc[k & 15] = p1305_add(p1305_mul(acc[k & 15], r16), block(msg, k));
      for (int lane = 0; lane < 16; ++lane) {  // the row sum of the carried products
        const P1305 t = p1305_mul(acc[lane], rpow[lane]);
        for (int i = 0; i < 5; ++i) h.l[i] += t.l[i];
      }
    } else {
      return 2;
    }
    p1305_finish(h, le32(&key[16]), le32(&key[20]), le32(&key[24]), le32(&key[28]), tag);
    print_tag(tag);
  }
  printf("poly1305_host: ok\n");
  return 0;
}
