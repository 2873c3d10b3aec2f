// translate.hip — the byte map (wc.hpp ByteMap) applied to device text in place.
//
//  wc_translate   text[i] = map[text[i]] for i in [0, n): case folding, "split on
//                 punctuation" and "split on these bytes" are instances of it.
//                 It runs once where a piece of text becomes device-resident
//                 (engine.cpp Impl::translate), so the tokenizer, the hot-word
//                 byte verification, the reduce's arena copies and the LONG-word
//                 compares all see translated bytes only; the map and reduce
//                 kernels know nothing of it.
//
// A pure streaming kernel: n bytes read, n bytes written, 16 bytes per lane per
// step (non-temporal), grid-stride over the 16-byte vectors, the last n % 16
// bytes byte-wise.
// The table lives in LDS as 64 dwords — 256 bytes are exactly one dword per
// bank, so lanes that look up different bytes read different banks or the same
// dword (a broadcast): no bank conflicts by construction.  Each byte is looked
// up with a one-byte LDS read at its own value and the vector is reassembled
// in registers.
//
// Reference: the reference program has no such stage (it splits on ' ', '\r',
// '\n' only and compares raw bytes).
#include <algorithm>

#include "../common/hip_util.hpp"
#include "kernels.hpp"
#include "wc/wc.hpp"

namespace wc {
namespace dev {

constexpr int TR_THREADS = 256;
// Memory-bound grid: enough blocks to fill the chip (256 CUs x 8 blocks of 256
// threads = 32 waves per CU, ~32 KiB of loads in flight per CU), the rest of
// the text by the grid stride.
constexpr uint32_t TR_MAX_BLOCKS = 2048;

__device__ __forceinline__ uint32_t tr_word(const uint8_t* tab, uint32_t x) {
  return (uint32_t)tab[x & 0xFFu] | ((uint32_t)tab[(x >> 8) & 0xFFu] << 8) | ((uint32_t)tab[(x >> 16) & 0xFFu] << 16) |
         ((uint32_t)tab[x >> 24] << 24);
}

// One 16-byte vector.  The text is far larger than the caches and every byte
// is touched once, so it is loaded and stored non-temporally (measured against
// plain accesses and against two and four vectors in flight per lane:
// profiles/translate_cost.md).
typedef uint32_t tr_vec4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(TR_THREADS) wc_translate(uint8_t* __restrict__ text, uint64_t n, ByteMap map) {
  __shared__ uint32_t tab32[64];
  if (threadIdx.x < 64) {
    const uint32_t b = threadIdx.x * 4;
    tab32[threadIdx.x] = (uint32_t)map.m[b] | ((uint32_t)map.m[b + 1] << 8) | ((uint32_t)map.m[b + 2] << 16) |
                         ((uint32_t)map.m[b + 3] << 24);
  }
  __syncthreads();
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(tab32);
  const uint64_t nvec = n >> 4;
  tr_vec4* v = reinterpret_cast<tr_vec4*>(text);
  const uint64_t stride = (uint64_t)gridDim.x * TR_THREADS;
  for (uint64_t i = (uint64_t)blockIdx.x * TR_THREADS + threadIdx.x; i < nvec; i += stride) {
    tr_vec4 x = __builtin_nontemporal_load(v + i);
    x.x = tr_word(tab, x.x);
    x.y = tr_word(tab, x.y);
    x.z = tr_word(tab, x.z);
    x.w = tr_word(tab, x.w);
    __builtin_nontemporal_store(x, v + i);
  }
  // the last n % 16 bytes: one lane each, nothing at or beyond n is touched
  if (blockIdx.x == 0) {
    const uint64_t j = (nvec << 4) + threadIdx.x;
    if (threadIdx.x < 16 && j < n) text[j] = tab[text[j]];
  }
}

}  // namespace dev

void launch_translate(uint8_t* text, uint64_t n, const ByteMap& map, hipStream_t s) {
  if (n == 0) return;
  WC_CHECK((reinterpret_cast<uintptr_t>(text) & 15) == 0, "translated text must be 16-byte aligned");
  const uint64_t nvec = n >> 4;
  const uint32_t blocks =
      (uint32_t)std::min<uint64_t>(dev::TR_MAX_BLOCKS, std::max<uint64_t>(1, (nvec + dev::TR_THREADS - 1) / dev::TR_THREADS));
  hipLaunchKernelGGL(dev::wc_translate, dim3(blocks), dim3(dev::TR_THREADS), 0, s, text, n, map);
}

}  // namespace wc
