// byte_map.cpp — host side of the byte map (wc.hpp ByteMap): the validity
// check the Engine constructor applies and the builder behind the CLI flags
// (--fold-case, --split-punct, --split) and ops.byte_map().
#include <cstdio>

#include "../kernels/keys.hpp"
#include "wc/wc.hpp"

namespace wc {

namespace {
std::string hex(uint32_t b) {
  char s[8];
  std::snprintf(s, sizeof s, "0x%02X", b & 0xFFu);
  return s;
}
}  // namespace

std::string byte_map_check(const uint8_t m[256]) {
  // the delimiters stay: shard ranges, stream pieces and checkpoint intervals
  // are cut on raw delimiters and must still end on a token boundary
  for (uint32_t d : {0x20u, 0x0Du, 0x0Au})
    if (m[d] != d) return "byte map moves the delimiter " + hex(d) + " (to " + hex(m[d]) + "): delimiters must map to themselves";
  // idempotent: text translated in place may be translated again
  for (uint32_t b = 0; b < 256; ++b)
    if (m[m[b]] != m[b])
      return "byte map is not idempotent at byte " + hex(b) + ": it maps to " + hex(m[b]) + ", which maps on to " +
             hex(m[m[b]]);
  return std::string();
}

ByteMap make_byte_map(bool fold_case, const uint8_t* split, uint64_t split_n, bool split_punct) {
  ByteMap bm;
  if (fold_case)
    for (uint32_t b = 'A'; b <= 'Z'; ++b) bm.m[b] = (uint8_t)(b + 32);
  if (split_punct)
    for (uint32_t b = 0x21; b <= 0x7E; ++b)
      if ((b <= 0x2F) || (b >= 0x3A && b <= 0x40) || (b >= 0x5B && b <= 0x60) || b >= 0x7B) bm.m[b] = 0x20;
  // a listed byte splits whatever the fold made of it ('A' listed: 'A' -> space,
  // 'a' stays); listing a delimiter changes nothing
  for (uint64_t i = 0; i < split_n; ++i)
    if (!is_delim(split[i])) bm.m[split[i]] = 0x20;
  // close the two-step chains ('A' -> 'a' -> space when 'a' is split): every
  // target is then space or an unsplit lower-case letter, both fixed points
  for (uint32_t b = 0; b < 256; ++b) bm.m[b] = bm.m[bm.m[b]];
  bm.on = 1;
  return bm;
}

}  // namespace wc
