// wgcs_aead.h -- the two pieces of host arithmetic around the transport AEAD
// that the kernel and the host API share: padding() of device/send.go:529-560
// and the length trim of RoutineSendToInternet, device/receive.go:432-482.
#pragma once

#include <stdint.h>

#include "../../include/wgcsum.h"
#include "wgcs_poly1305.h"  // WGCS_HD

namespace wgcs {

constexpr uint32_t kAeadHeader = 16;   // MessageTransportHeaderSize = MessageTransportContentOffset
constexpr uint32_t kAeadTag = 16;      // chacha20poly1305.Overhead
constexpr uint32_t kAeadMaxLen = 65535;  // largest descriptor len either mode accepts
constexpr uint32_t kPaddingMultiple = 16;

// padding(packetSize, mtu) -- send.go:529-560, for packetSize <= 65535.
WGCS_HD uint32_t aead_padding(uint32_t packet_size, uint32_t mtu) {
  uint32_t last_unit = packet_size;
  if (mtu == 0) return ((last_unit + kPaddingMultiple - 1) & ~(kPaddingMultiple - 1)) - last_unit;
  if (last_unit > mtu) last_unit %= mtu;
  uint32_t padded = (last_unit + kPaddingMultiple - 1) & ~(kPaddingMultiple - 1);
  if (padded > mtu) padded = mtu;
  return padded - last_unit;
}

// The packet length RoutineSendToInternet keeps of a plaintext of n bytes
// whose first six bytes are b0 .. b5 (those beyond n are not looked at):
// 0 for a keepalive, WGCS_ERR_PACKET_TOO_SHORT for every `continue` of :438-482.
WGCS_HD int32_t aead_trim(uint32_t n, uint32_t b0, uint32_t b2, uint32_t b3, uint32_t b4, uint32_t b5) {
  if (n == 0) return 0;  // :432
  const uint32_t ver = b0 >> 4;
  if (ver == 4) {
    if (n < 20) return WGCS_ERR_PACKET_TOO_SHORT;  // :440
    const uint32_t length = (b2 << 8) | b3;
    if (length > n || length < 20) return WGCS_ERR_PACKET_TOO_SHORT;  // :446
    return (int32_t)length;
  }
  if (ver == 6) {
    if (n < 40) return WGCS_ERR_PACKET_TOO_SHORT;  // :460
    const uint32_t length = (((b4 << 8) | b5) + 40u) & 0xFFFFu;  // uint16 arithmetic, :465-466
    if (length > n) return WGCS_ERR_PACKET_TOO_SHORT;  // :467
    return (int32_t)length;
  }
  return WGCS_ERR_PACKET_TOO_SHORT;  // :479
}

}  // namespace wgcs
