// wordorder.hip — the finalized key table ordered by word, bytewise, on the
// device (Engine::result_by_word): a permutation of row indices.
//
// The order is Python's sorted() on bytes: bytes compare unsigned, a proper
// prefix comes first.  A word is compared 8 bytes at a time.  The chunk at
// byte offset `off` is the pair
//
//   (bswap64 of bytes [off, off + 8) packed little-endian and zero-padded,
//    tie class min(len - off, 9))
//
// The tie class tells zero padding from NUL bytes of the word (b"ab" <
// b"ab\0"): 0..8 = the word ends in this chunk after that many bytes, 9 = it
// continues.  Two rows equal in a chunk with a tie class below 9 are the same
// word — a duplicate key in the table; the order fails the job naming them.
//
// Level 0 sorts every row by the chunk at offset 0 (k0).  A run of rows equal
// in (chunk, tie class) is a segment; rows in segments of one are final, the
// others are compacted in order (a scan) into the next level's slots.  A slot
// keeps its output position: later levels only permute rows among the slots
// of their segment.  Level L >= 1 sorts its slots by (segment, chunk at the
// segment's offset, tie class), re-segments and compacts again; the chunk
// comes from k1 (MEDIUM keys, offset 8) or the key arena (LONG keys).  From
// level 2 on, a segment first advances its offset to 8 * floor(LCP / 8), LCP
// the longest common prefix of its members (wc_word_lcp, wc_word_skip): the
// level count does not grow with the length of a shared prefix.
//
// Launches per level: [lcp, skip] chunk | keys + radix sort on the tie class | keys
// + radix sort on the chunk | [keys + radix sort on the segment] | mark |
// scan | write.  The host reads one state block per level (rows unresolved,
// segments, the duplicate word, the bounds word) and stops at zero.
#include <algorithm>
#include <cstring>
#include <string>

#include "../common/hip_util.hpp"
#include "bounds.hpp"
#include "kernels.hpp"
#include "keys.hpp"

namespace wc {
namespace dev {

constexpr int WO_THREADS = 256;
constexpr int WO_WAVES = WO_THREADS / 64;
constexpr int WO_ROUNDS = 4;                               // compaction: rows per lane
constexpr uint32_t WO_TILE = WO_THREADS * WO_ROUNDS;       // 1024 slots per block
constexpr uint32_t WO_WAVE_ROWS = 64 * WO_ROUNDS;          // a wave's contiguous slots of the tile
constexpr int WO_SCAN_THREADS = 1024;
constexpr uint32_t WO_UNRES = 1, WO_HEAD = 2, WO_DUP = 4;  // wo_flags bits

// One level's slots (device arrays).
struct WordLevel {
  uint32_t* row;  // the table row in the slot
  uint32_t* pos;  // the slot's output position (fixed while the level lasts)
  uint32_t* seg;  // its segment, ascending with the slot index
  uint32_t* off;  // the segment's byte offset
};
// The level's sort: slot v = vals[i] is i-th in (segment, chunk, tie class).
struct WordSorted {
  const uint32_t* vals;
  const uint64_t* ck;   // per slot: bswap64 of the chunk
  const uint32_t* tie;  // per slot: the tie class
  const uint32_t* seg;
};

__device__ __forceinline__ uint32_t wo_len(const WordCols& c, uint32_t r, uint64_t k1) {
  return key_is_hashed(k1) ? c.slen[r] : inline_len(k1);
}

// Bytes [off, off + 8) of row r's word (len bytes), packed little-endian and
// zero-padded past its end.  Arena bytes are read inside [soff, soff + len)
// and inside the arena only; a reference that leaves it is reported (err) and
// reads as zeros.
__device__ __forceinline__ uint64_t wo_chunk(const WordCols& c, uint32_t r, uint64_t k1, uint32_t len, uint32_t off,
                                             unsigned long long* err) {
  if (off == 0) return c.k0[r];
  if (!key_is_hashed(k1)) return (!key_is_short(k1) && off == 8) ? (k1 & ((1ull << 56) - 1)) : 0ull;
  if (off >= len) return 0;
  const uint32_t nb = len - off < 8u ? len - off : 8u;
  const uint64_t base = c.soff[r];
  if (base >= c.arena_bytes || (uint64_t)off + nb > c.arena_bytes - base) {
    bounds_ok(Bounds{err, c.arena_bytes}, BND_WORD_ARENA, base >= c.arena_bytes ? base : base + off + nb - 1);
    return 0;
  }
  const uint8_t* p = c.arena + base + off;
  uint64_t v = 0;
  if (nb == 8) {
    __builtin_memcpy(&v, p, 8);  // a whole chunk: one load, any alignment
    return v;
  }
  for (uint32_t i = 0; i < nb; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

__device__ __forceinline__ unsigned long long wo_wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;  // lane 0
}

// Exclusive prefix of one value per thread over the scan block (every thread
// calls); total = the block's sum.
__device__ __forceinline__ unsigned long long wo_block_excl(unsigned long long v, unsigned long long* wtot,
                                                            unsigned long long& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(incl, o);
    if (lane >= o) incl += y;
  }
  __syncthreads();  // wtot may still be read from an earlier call
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  unsigned long long before = 0, all = 0;
  for (int w = 0; w < WO_SCAN_THREADS / 64; ++w) {
    const unsigned long long x = wtot[w];
    if (w < wave) before += x;
    all += x;
  }
  total = all;
  return before + incl - v;
}

// Level 0: slot i holds row i at output position i; one segment at offset 0.
__global__ void wc_word_init(WordLevel lv, uint64_t n, Bounds bnd) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!bounds_ok(bnd, BND_WORD_KEYS, i)) continue;
    lv.row[i] = (uint32_t)i;
    lv.pos[i] = (uint32_t)i;
    lv.seg[i] = 0;
    lv.off[i] = 0;
  }
}

// Per slot: the chunk at its segment's offset, byte-swapped (integer order =
// byte order), and the tie class.
__global__ void wc_word_chunk(WordCols c, WordLevel lv, uint64_t m, uint64_t* ck, uint32_t* tie, Bounds bnd) {
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    if (!bounds_ok(bnd, BND_WORD_KEYS, j)) continue;
    const uint32_t r = lv.row[j], off = lv.off[j];
    uint64_t v = 0;
    uint32_t t = 0;
    if (bounds_ok(Bounds{bnd.err, c.n}, BND_WORD_KEYS, r)) {  // a row outside the table is reported, not read
      const uint64_t k1 = c.k1[r];
      const uint32_t len = wo_len(c, r, k1);
      v = wo_chunk(c, r, k1, len, off, bnd.err);
      t = len <= off ? 0u : (len - off < 9u ? len - off : 9u);
    }
    ck[j] = __builtin_bswap64(v);
    tie[j] = t;
  }
}

// Keys of the level's three stable sorts, least significant first: WHICH 0 =
// the tie class (vals = the slot indices), 1 = the chunk, 2 = the segment of
// slot vals[i].
template <int WHICH>
__global__ void wc_word_keys(const uint64_t* ck, const uint32_t* tie, const uint32_t* seg, uint64_t m, uint64_t* keys,
                             uint32_t* vals, Bounds bnd) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    if (!bounds_ok(bnd, BND_WORD_KEYS, i)) continue;
    if (WHICH == 0) {
      keys[i] = tie[i];
      vals[i] = (uint32_t)i;
    } else {
      const uint32_t v = vals[i];
      const bool ok = bounds_ok(Bounds{bnd.err, m}, BND_WORD_KEYS, v);
      keys[i] = !ok ? 0ull : (WHICH == 1 ? ck[v] : (uint64_t)seg[v]);
    }
  }
}

// Slot at sorted place i (i < m); a value outside the level is reported and
// read as slot 0.
__device__ __forceinline__ uint32_t wo_slot(const WordSorted& sv, uint64_t i, uint64_t m, unsigned long long* err) {
  const uint32_t v = sv.vals[i];
  return bounds_ok(Bounds{err, m}, BND_WORD_MARK, v) ? v : 0u;
}

// Flags of sorted place i: WO_UNRES = it shares (segment, chunk, tie class)
// with a neighbour, WO_HEAD = and is the first of its run, WO_DUP = it equals
// its predecessor and the word ended (*prev = the predecessor's slot).
__device__ __forceinline__ uint32_t wo_flags(const WordSorted& sv, uint64_t i, uint64_t m, unsigned long long* err,
                                             uint32_t* slot, uint32_t* prev) {
  const uint32_t v = wo_slot(sv, i, m, err);
  const uint32_t sg = sv.seg[v], t = sv.tie[v];
  const uint64_t k = sv.ck[v];
  *slot = v;
  bool sp = false, sn = false;
  if (i > 0) {
    const uint32_t u = wo_slot(sv, i - 1, m, err);
    *prev = u;
    sp = sv.seg[u] == sg && sv.ck[u] == k && sv.tie[u] == t;
  }
  if (i + 1 < m) {
    const uint32_t w = wo_slot(sv, i + 1, m, err);
    sn = sv.seg[w] == sg && sv.ck[w] == k && sv.tie[w] == t;
  }
  return ((sp || sn) ? WO_UNRES : 0u) | ((!sp && sn) ? WO_HEAD : 0u) | ((sp && t < 9u) ? WO_DUP : 0u);
}

// Compaction, launch 1.  Every sorted row goes to its slot's output position
// (a row still tied is placed again by a later level); per tile of WO_TILE
// places, the rows still tied and the runs they form.
__global__ void __launch_bounds__(WO_THREADS) wc_word_mark(WordSorted sv, WordLevel lv, uint64_t m, uint32_t* perm,
                                                           WordState* st, uint32_t* blk_u, uint32_t* blk_h,
                                                           Bounds bnd) {
  __shared__ unsigned long long wsum[WO_WAVES];
  const uint64_t base = (uint64_t)blockIdx.x * WO_TILE;
  uint32_t u = 0, h = 0;
#pragma unroll
  for (int j = 0; j < WO_ROUNDS; ++j) {
    const uint64_t i = base + (uint64_t)j * WO_THREADS + threadIdx.x;
    if (i < m) {
      uint32_t v, pv = 0;
      const uint32_t f = wo_flags(sv, i, m, bnd.err, &v, &pv);
      const uint32_t r = lv.row[v], p = lv.pos[i];
      if (bounds_ok(bnd, BND_WORD_PERM, p)) perm[p] = r;
      if ((f & WO_DUP) && atomicCAS(&st->dup, 0ull, 1ull) == 0ull) {  // the first pair found, for the host's message
        st->dup_a = lv.row[pv];
        st->dup_b = r;
      }
      u += (f & WO_UNRES) != 0;
      h += (f & WO_HEAD) != 0;
    }
  }
  const unsigned long long both = wo_wave_sum(((unsigned long long)u << 32) | h);  // <= 1024 each: no carry
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = both;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < WO_WAVES; ++w) t += wsum[w];
    blk_u[blockIdx.x] = (uint32_t)(t >> 32);
    blk_h[blockIdx.x] = (uint32_t)t;
  }
}

// Launch 2 (one block): the tile counts -> their exclusive prefixes, in place;
// the totals into the state and the end of the segment list.
__global__ void __launch_bounds__(WO_SCAN_THREADS) wc_word_scan(uint32_t* blk_u, uint32_t* blk_h, uint32_t nblk,
                                                                WordState* st, uint32_t* seg_start) {
  __shared__ unsigned long long wtot[WO_SCAN_THREADS / 64];
  const uint32_t per = (nblk + WO_SCAN_THREADS - 1) / WO_SCAN_THREADS;
  const uint64_t t0 = (uint64_t)threadIdx.x * per, b0 = t0 < nblk ? t0 : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
  unsigned long long u = 0, h = 0;
  for (uint64_t b = b0; b < b1; ++b) {
    u += blk_u[b];
    h += blk_h[b];
  }
  unsigned long long tu, th;
  u = wo_block_excl(u, wtot, tu);
  h = wo_block_excl(h, wtot, th);
  for (uint64_t b = b0; b < b1; ++b) {
    const uint32_t x = blk_u[b], y = blk_h[b];
    blk_u[b] = (uint32_t)u;
    blk_h[b] = (uint32_t)h;
    u += x;
    h += y;
  }
  if (threadIdx.x == 0) {
    st->unresolved = tu;
    st->segments = th;
    seg_start[th] = (uint32_t)tu;  // th <= tu / 2 < the list's rows
  }
}

// Launch 3: the rows still tied, in sorted order, into the next level's
// slots: slot U (the tied rows before it) keeps the output position of its
// place, takes segment H - 1 (H = the runs begun at or before it) and the
// offset past this chunk.  A wave owns WO_WAVE_ROWS contiguous places.
__global__ void __launch_bounds__(WO_THREADS) wc_word_write(WordSorted sv, WordLevel lv, uint64_t m,
                                                            const uint32_t* blk_u, const uint32_t* blk_h, WordLevel nx,
                                                            uint32_t* seg_start, Bounds bnd) {
  __shared__ uint32_t wu[WO_WAVES], wh[WO_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * WO_TILE + (uint64_t)wave * WO_WAVE_ROWS;
  uint32_t f[WO_ROUNDS], v[WO_ROUNDS];
  uint32_t u = 0, h = 0;
#pragma unroll
  for (int j = 0; j < WO_ROUNDS; ++j) {
    const uint64_t i = base + (uint64_t)j * 64 + lane;
    uint32_t pv = 0;
    v[j] = 0;
    f[j] = i < m ? wo_flags(sv, i, m, nullptr, &v[j], &pv) : 0u;
    u += (uint32_t)__popcll(__ballot((f[j] & WO_UNRES) != 0));
    h += (uint32_t)__popcll(__ballot((f[j] & WO_HEAD) != 0));
  }
  if (lane == 0) {
    wu[wave] = u;
    wh[wave] = h;
  }
  __syncthreads();
  uint64_t U = blk_u[blockIdx.x], H = blk_h[blockIdx.x];
  for (int w = 0; w < wave; ++w) {
    U += wu[w];
    H += wh[w];
  }
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < WO_ROUNDS; ++j) {
    const uint64_t i = base + (uint64_t)j * 64 + lane;
    const bool un = (f[j] & WO_UNRES) != 0, hd = (f[j] & WO_HEAD) != 0;
    const unsigned long long mu = __ballot(un), mh = __ballot(hd);
    if (un) {
      const uint64_t jp = U + (uint64_t)__popcll(mu & below);
      const uint64_t sid = H + (uint64_t)__popcll(mh & below) + (hd ? 1u : 0u) - 1u;  // a tied row follows its run's head
      if (bounds_ok(bnd, BND_WORD_COMPACT, jp)) {
        nx.row[jp] = lv.row[v[j]];
        nx.pos[jp] = lv.pos[i];
        nx.seg[jp] = (uint32_t)sid;
        nx.off[jp] = lv.off[i] + 8u;
        if (hd && bounds_ok(Bounds{bnd.err, m / 2 + 1}, BND_WORD_COMPACT, sid)) seg_start[sid] = (uint32_t)jp;
      }
    }
    U += (uint64_t)__popcll(mu);
    H += (uint64_t)__popcll(mh);
  }
}

// Prefix skip, launch 1: seg_lcp[s] (preset to all ones) = the longest common
// prefix of segment s's LONG words — min over its slots of the length slot j's
// word shares with the word of the segment's first slot.  A lane compares its
// slot's pair for WO_LCP_LANE chunks from the segment's offset on; a pair
// still equal after that is finished by the whole wave, 64 chunks per step
// (two 70 000-byte words: 137 steps, not 8 750 iterations of one lane).  A
// segment with an inline key (level 1 only) is left where it is.
constexpr uint32_t WO_LCP_LANE = 8;
__global__ void __launch_bounds__(WO_THREADS) wc_word_lcp(WordCols c, WordLevel lv, uint64_t m,
                                                          const uint32_t* seg_start, uint64_t nseg, uint32_t* seg_lcp,
                                                          Bounds bnd) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * WO_THREADS + threadIdx.x) >> 6;
  const uint64_t waves = (uint64_t)gridDim.x * WO_WAVES;
  for (uint64_t base = wave * 64; base < m; base += waves * 64) {
    const uint64_t j = base + lane;
    bool in = j < m;
    uint32_t sg = 0, r0 = 0, r = 0, q = 0, lim = 0, len0 = 0, len = 0;
    uint64_t k10 = 0, k1 = 0;
    if (in) {
      sg = lv.seg[j];
      in = bounds_ok(Bounds{bnd.err, nseg}, BND_WORD_LCP, sg);
    }
    if (in) {
      const uint32_t a = seg_start[sg];
      in = bounds_ok(Bounds{bnd.err, m}, BND_WORD_LCP, a);
      if (in) {
        r0 = lv.row[a];
        r = lv.row[j];
        q = lv.off[j];
        in = bounds_ok(Bounds{bnd.err, c.n}, BND_WORD_LCP, r0) && bounds_ok(Bounds{bnd.err, c.n}, BND_WORD_LCP, r);
      }
    }
    bool pending = false;
    if (in) {
      k10 = c.k1[r0];
      k1 = c.k1[r];
      if (key_is_hashed(k10) && key_is_hashed(k1)) {
        len0 = wo_len(c, r0, k10);
        len = wo_len(c, r, k1);
        lim = len < len0 ? len : len0;
        pending = true;
        for (uint32_t it = 0; it < WO_LCP_LANE && q < lim; ++it) {
          const uint64_t x = wo_chunk(c, r0, k10, len0, q, bnd.err) ^ wo_chunk(c, r, k1, len, q, bnd.err);
          if (x) {
            q += (uint32_t)(__builtin_ctzll(x) >> 3);
            pending = false;
            break;
          }
          q += 8;
        }
        if (q >= lim) pending = false;
      } else {
        lim = q;  // an inline key: the segment's prefix stays at its offset
      }
    }
    unsigned long long todo = __ballot(pending);
    while (todo) {  // the wave finishes lane w's pair
      const int w = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const uint32_t wr0 = __shfl(r0, w), wr = __shfl(r, w), wlim = __shfl(lim, w), wlen0 = __shfl(len0, w),
                     wlen = __shfl(len, w);
      const uint64_t wk10 = __shfl(k10, w), wk1 = __shfl(k1, w);
      uint32_t wq = __shfl(q, w);
      while (wq < wlim) {  // wave-uniform
        const uint64_t mine = (uint64_t)wq + 8ull * lane;
        uint64_t x = 0;
        if (mine < wlim)
          x = wo_chunk(c, wr0, wk10, wlen0, (uint32_t)mine, bnd.err) ^ wo_chunk(c, wr, wk1, wlen, (uint32_t)mine, bnd.err);
        const unsigned long long diff = __ballot(x != 0);
        if (diff) {
          const int d = __ffsll((long long)diff) - 1;
          wq = __shfl((uint32_t)mine + (uint32_t)(__builtin_ctzll(x | (1ull << 63)) >> 3), d);
          break;
        }
        const uint64_t next = (uint64_t)wq + 8ull * 64;
        wq = next < wlim ? (uint32_t)next : wlim;
      }
      if (lane == w) q = wq;
    }
    const uint32_t l = !in ? 0xFFFFFFFFu : (q < lim ? q : lim);
    const unsigned long long act = __ballot(in);
    if (act) {  // wave-uniform
      const int f = __ffsll((long long)act) - 1;
      const uint32_t s0 = __shfl(sg, f);
      if (__ballot(in && sg != s0) == 0) {  // the wave's slots share a segment: one add for all of them
        uint32_t v = l;
        for (int o = 32; o > 0; o >>= 1) {
          const uint32_t y = __shfl_xor(v, o);
          v = y < v ? y : v;
        }
        if (lane == f) atomicMin(&seg_lcp[s0], v);
      } else if (in) {
        atomicMin(&seg_lcp[sg], l);
      }
    }
  }
}

// Launch 2: every slot of a segment moves to 8 * floor(LCP / 8).
__global__ void wc_word_skip(WordLevel lv, uint64_t m, const uint32_t* seg_lcp, uint64_t nseg, Bounds bnd) {
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t sg = lv.seg[j];
    if (!bounds_ok(bnd, BND_WORD_LCP, j) || !bounds_ok(Bounds{bnd.err, nseg}, BND_WORD_LCP, sg)) continue;
    const uint32_t l = seg_lcp[sg];
    const uint32_t noff = l == 0xFFFFFFFFu ? 0u : (l & ~7u);
    if (noff > lv.off[j]) lv.off[j] = noff;
  }
}

inline uint32_t wo_grid(uint64_t n, uint32_t per_block, uint32_t cap) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, (n + per_block - 1) / per_block));
}

}  // namespace dev

static uint64_t wo_tiles(uint64_t m) { return std::max<uint64_t>(1, (m + dev::WO_TILE - 1) / dev::WO_TILE); }
static size_t wo_pad(size_t b) { return (b + 255) / 256 * 256; }

// state | perm [n] | two levels of (row, pos, seg, off) [n] | chunk [n], tie
// [n] | keys, tmp keys [n], values, tmp values [n] | radix workspace | tile
// counts 2 x [tiles] | segment starts, segment prefixes [n / 2 + 2]
size_t word_order_ws_bytes(uint64_t n) {
  const size_t nn = n ? n : 1;
  return wo_pad(sizeof(WordState)) + wo_pad(nn * 4) + 8 * wo_pad(nn * 4) + wo_pad(nn * 8) + wo_pad(nn * 4) +
         2 * wo_pad(nn * 8) + 2 * wo_pad(nn * 4) + wo_pad(radix_hist_words(nn) * 4) + 2 * wo_pad(wo_tiles(nn) * 4) +
         2 * wo_pad((nn / 2 + 2) * 4);
}

const uint32_t* word_order(const WordCols& c, void* ws, hipStream_t s, unsigned long long* bounds_err,
                           unsigned long long* h_state, WordOrderInfo* info, void (*stage)(void*, const char*),
                           void* stage_arg) {
  const uint64_t n = c.n;
  WC_CHECK(n < (1ull << 32), "word_order: at most 2^32 - 1 rows (row indices are 32-bit)");
  const size_t nn = n ? n : 1;
  uint8_t* p = static_cast<uint8_t*>(ws);
  auto take = [&](size_t b) {
    uint8_t* r = p;
    p += wo_pad(b);
    return r;
  };
  WordState* st = reinterpret_cast<WordState*>(take(sizeof(WordState)));
  uint32_t* perm = reinterpret_cast<uint32_t*>(take(nn * 4));
  dev::WordLevel lv{}, nx{};
  for (dev::WordLevel* l : {&lv, &nx}) {
    l->row = reinterpret_cast<uint32_t*>(take(nn * 4));
    l->pos = reinterpret_cast<uint32_t*>(take(nn * 4));
    l->seg = reinterpret_cast<uint32_t*>(take(nn * 4));
    l->off = reinterpret_cast<uint32_t*>(take(nn * 4));
  }
  uint64_t* ck = reinterpret_cast<uint64_t*>(take(nn * 8));
  uint32_t* tie = reinterpret_cast<uint32_t*>(take(nn * 4));
  uint64_t* keys = reinterpret_cast<uint64_t*>(take(nn * 8));
  uint64_t* tkeys = reinterpret_cast<uint64_t*>(take(nn * 8));
  uint32_t* vals = reinterpret_cast<uint32_t*>(take(nn * 4));
  uint32_t* tvals = reinterpret_cast<uint32_t*>(take(nn * 4));
  uint32_t* hist = reinterpret_cast<uint32_t*>(take(radix_hist_words(nn) * 4));
  uint32_t* blk_u = reinterpret_cast<uint32_t*>(take(wo_tiles(nn) * 4));
  uint32_t* blk_h = reinterpret_cast<uint32_t*>(take(wo_tiles(nn) * 4));
  uint32_t* seg_start = reinterpret_cast<uint32_t*>(take((nn / 2 + 2) * 4));
  uint32_t* seg_lcp = reinterpret_cast<uint32_t*>(take((nn / 2 + 2) * 4));
  const bool events = info && info->time_events;
  if (info) *info = WordOrderInfo{};
  if (n == 0) return perm;
  hipEvent_t ev[WordOrderInfo::MAX_LEVEL_ROWS + 1] = {};
  uint32_t n_ev = 0;
  auto event = [&] {
    if (!events || n_ev > WordOrderInfo::MAX_LEVEL_ROWS) return;
    WC_HIP_CHECK(hipEventCreate(&ev[n_ev]));
    WC_HIP_CHECK(hipEventRecord(ev[n_ev++], s));
  };
  unsigned long long local[9];
  unsigned long long* hs = h_state ? h_state : local;
  // a LONG word's bytes lie in the arena and a level consumes 8 of them: more levels than that cannot be
  const uint64_t max_levels = 3 + c.arena_bytes / 8;
  WC_HIP_CHECK(hipMemsetAsync(st, 0, sizeof(WordState), s));
  hipLaunchKernelGGL(dev::wc_word_init, dim3(dev::wo_grid(n, 256, 2048)), dim3(256), 0, s, lv, n,
                     Bounds{bounds_err, n});
  event();
  std::string dup_msg;
  uint64_t m = n, nseg = 1;
  for (uint32_t level = 0; m > 0; ++level) {
    WC_CHECK(level < max_levels, "word_order: more levels than the longest word has chunks");
    const double t_level = now_seconds();
    const Bounds bm{bounds_err, m};
    const dim3 grid(dev::wo_grid(m, 256, 2048)), block(256);
    if (level >= 2 && nseg > 0) {
      WC_CHECK(nseg <= nn / 2 + 1, "word_order: more segments than pairs of rows");
      WC_HIP_CHECK(hipMemsetAsync(seg_lcp, 0xFF, nseg * 4, s));
      hipLaunchKernelGGL(dev::wc_word_lcp, dim3(dev::wo_grid(m, dev::WO_THREADS, 2048)), dim3(dev::WO_THREADS), 0, s, c,
                         lv, m, seg_start, nseg, seg_lcp, bm);
      hipLaunchKernelGGL(dev::wc_word_skip, grid, block, 0, s, lv, m, seg_lcp, nseg, bm);
      if (stage) stage(stage_arg, "prefix skip");
    }
    hipLaunchKernelGGL(dev::wc_word_chunk, grid, block, 0, s, c, lv, m, ck, tie, bm);
    if (stage) stage(stage_arg, "chunks");
    bool in_tmp = false;
    auto sorted = [&] {
      if (in_tmp) {
        std::swap(keys, tkeys);
        std::swap(vals, tvals);
      }
    };
    hipLaunchKernelGGL(dev::wc_word_keys<0>, grid, block, 0, s, ck, tie, lv.seg, m, keys, vals, bm);
    radix_sort_pairs(keys, vals, tkeys, tvals, hist, m, 4, s, &in_tmp);
    sorted();
    hipLaunchKernelGGL(dev::wc_word_keys<1>, grid, block, 0, s, ck, tie, lv.seg, m, keys, vals, bm);
    radix_sort_pairs(keys, vals, tkeys, tvals, hist, m, 64, s, &in_tmp);
    sorted();
    if (nseg > 1) {  // back into segment order (stable: the chunk order inside a segment stays)
      int bits = 1;
      while (bits < 32 && ((nseg - 1) >> bits) != 0) ++bits;
      hipLaunchKernelGGL(dev::wc_word_keys<2>, grid, block, 0, s, ck, tie, lv.seg, m, keys, vals, bm);
      radix_sort_pairs(keys, vals, tkeys, tvals, hist, m, bits, s, &in_tmp);
      sorted();
    }
    if (stage) stage(stage_arg, "sort");
    const dev::WordSorted sv{vals, ck, tie, lv.seg};
    const uint32_t tiles = (uint32_t)wo_tiles(m);
    hipLaunchKernelGGL(dev::wc_word_mark, dim3(tiles), dim3(dev::WO_THREADS), 0, s, sv, lv, m, perm, st, blk_u, blk_h,
                       Bounds{bounds_err, n});
    hipLaunchKernelGGL(dev::wc_word_scan, dim3(1), dim3(dev::WO_SCAN_THREADS), 0, s, blk_u, blk_h, tiles, st,
                       seg_start);
    hipLaunchKernelGGL(dev::wc_word_write, dim3(tiles), dim3(dev::WO_THREADS), 0, s, sv, lv, m, blk_u, blk_h, nx,
                       seg_start, bm);
    if (stage) stage(stage_arg, "segments");
    WC_HIP_CHECK(hipMemcpyAsync(hs, st, sizeof(WordState), hipMemcpyDeviceToHost, s));
    if (bounds_err) WC_HIP_CHECK(hipMemcpyAsync(hs + 8, bounds_err, 8, hipMemcpyDeviceToHost, s));
    event();
    WC_HIP_CHECK(hipStreamSynchronize(s));  // the level's wait
    WordState h;
    std::memcpy(&h, hs, sizeof h);
    const uint64_t bw = bounds_err ? hs[8] : 0;
    if (info) {
      info->levels = level + 1;
      if (level == 0) info->unresolved = h.unresolved;
      info->bounds_word = bw;
      if (level < WordOrderInfo::MAX_LEVEL_ROWS) {
        info->level_rows[level] = m;
        info->level_ms[level] = (now_seconds() - t_level) * 1e3;
      }
    }
    if (bw) break;  // the caller reports it (check_bounds)
    if (h.dup) {
      dup_msg = "word order: rows " + std::to_string(h.dup_a) + " and " + std::to_string(h.dup_b) +
                " of the table hold the same word (a duplicate key)";
      break;
    }
    WC_CHECK(h.unresolved <= m && h.unresolved != 1 && h.segments * 2 <= h.unresolved,
             "word_order: inconsistent segment state");
    m = h.unresolved;
    nseg = h.segments;
    std::swap(lv, nx);
  }
  for (uint32_t i = 0; i < n_ev; ++i) {  // every recorded event has completed: each level ended with a wait
    float ms = 0;
    if (i > 0 && hipEventElapsedTime(&ms, ev[i - 1], ev[i]) == hipSuccess) info->level_dev_ms[i - 1] = ms;
  }
  for (uint32_t i = 0; i < n_ev; ++i) (void)hipEventDestroy(ev[i]);
  if (!dup_msg.empty()) fail(dup_msg);
  return perm;
}

}  // namespace wc
