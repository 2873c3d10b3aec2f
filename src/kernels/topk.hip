// topk.hip — the K most frequent rows of the finalized key table, selected on
// the device (Engine::top_k): only the K rows and their words reach the host.
//
// "Top K" = the min(K, n) rows first under (count descending, row ascending);
// the rows are in first-occurrence order, so the tie-break is first offset.
//
//   1. threshold   T = the K-th largest count, n_gt = rows with count > T, the
//                  column sum: a radix select from the top bit down
//                  (wc_topk_hist + wc_topk_pick)
//   2. compaction  rows with count > T and the first K - n_gt rows with count
//                  == T, their indices in ascending row order (wc_topk_count,
//                  wc_topk_scan, wc_topk_write: a scan, no atomic cursor)
//   3. order       (count, row) pairs by descending count: one block ranking in
//                  LDS up to TOPK_SMALL rows (wc_topk_rank), radix_sort_pairs on
//                  ~count above (wc_topk_keys)
//   4. gather      the K rows' columns and the bytes of their arena words into
//                  compact buffers (wc_topk_gather, wc_topk_offsets,
//                  wc_topk_words)
//
// Reads of the count column, worst case: 1 (log-scale pass: bin = position of
// the highest set bit, + sum) + ceil(63 / TK_DB) = 5 (refinement, TK_DB bits
// per pass, only rows inside the threshold bin counted) + 2 (compaction: count
// and write) = 8, for any 64-bit counts.  A refinement pass whose bits are
// already fixed exits at once, so Zipf-like counts read the column 1 + ceil((b
// - 1) / TK_DB) + 2 times, b = the bit length of T: 3 reads when T < 2 (the
// tail), 5 for a T of 2^26 (the head of a 1 GiB text).
//
// Every hand-off between blocks is a kernel boundary: a pass's histogram is
// folded into global memory (one add per nonzero bin per block) and a
// one-block kernel picks the bin — no in-launch inter-block protocol.
#include <algorithm>

#include "../common/hip_util.hpp"
#include "bounds.hpp"
#include "kernels.hpp"
#include "keys.hpp"

namespace wc {
namespace dev {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_DB = 13;                 // digit bits per refinement pass
constexpr int TK_BINS = 1 << TK_DB;       // 32 KiB of LDS counters
constexpr int TK_REFINE = (63 + TK_DB - 1) / TK_DB;
constexpr int TK_PICK_THREADS = 1024;
constexpr int TK_PICK_PER = TK_BINS / TK_PICK_THREADS;  // bins per thread of the pick
constexpr int TK_ROUNDS = 16;             // compaction: rows per lane
constexpr uint32_t TK_TILE = TK_THREADS * TK_ROUNDS;      // 4096 rows per block
constexpr uint32_t TK_WAVE_ROWS = 64 * TK_ROUNDS;         // a wave's contiguous rows of the tile
constexpr int TK_PEEL = 4;                // distinct bins a wave folds by ballot before per-lane adds
static_assert(TK_BINS % TK_PICK_THREADS == 0 && TK_BINS >= 65, "pick: whole bins per thread, room for the log bins");

// ++lh[bin] for the active lanes.  The tail of a Zipf-like column is millions
// of equal counts: a wave whose lanes share a bin adds once (ballot + popcount)
// instead of 64 serialised LDS atomics; after TK_PEEL distinct bins the rest
// add per lane.  Every lane of the wave calls.
__device__ __forceinline__ void hist_add(uint32_t* lh, bool active, uint32_t bin) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(active);
  for (int it = 0; it < TK_PEEL && todo; ++it) {
    const int lead = __ffsll((long long)todo) - 1;
    const uint32_t b0 = __shfl(bin, lead);
    const unsigned long long same = __ballot(active && bin == b0);
    if (lane == lead) atomicAdd(&lh[b0], (uint32_t)__popcll(same));
    if (bin == b0) active = false;
    todo &= ~same;
  }
  if (active) atomicAdd(&lh[bin], 1u);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;  // lane 0
}

// Exclusive prefix of one value per thread over a block of T threads (every
// thread calls); total = the block's sum.
template <int T>
__device__ __forceinline__ unsigned long long block_excl(unsigned long long v, unsigned long long* wtot,
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
  for (int w = 0; w < T / 64; ++w) {
    const unsigned long long x = wtot[w];
    if (w < wave) before += x;
    all += x;
  }
  total = all;
  return before + incl - v;
}

// One read of the column.  FIRST: hist[b] += rows whose highest set bit is b -
// 1 (b = 0: count 0), st->sum += the column.  Else, while bits of T remain
// open (st->rem_bits): of the rows inside the threshold bin (count >> rem ==
// st->thresh), hist[d] += rows by their next min(rem, TK_DB) bits.
template <bool FIRST>
__global__ void __launch_bounds__(TK_THREADS) wc_topk_hist(const uint64_t* __restrict__ cnt, uint64_t n, TopkState* st,
                                                           uint32_t* hist) {
  __shared__ uint32_t lh[TK_BINS];
  __shared__ unsigned long long wsum[TK_WAVES];
  uint32_t rem = 0, d = 0;
  uint64_t prefix = 0;
  if (!FIRST) {
    rem = (uint32_t)st->rem_bits;
    if (rem == 0) return;  // T is fixed: nothing to read
    prefix = st->thresh;
    d = rem < (uint32_t)TK_DB ? rem : (uint32_t)TK_DB;
  }
  const uint32_t nb = FIRST ? 65u : (1u << d);
  const uint32_t shift = rem - d;
  for (uint32_t b = threadIdx.x; b < nb; b += TK_THREADS) lh[b] = 0;
  __syncthreads();
  unsigned long long sum = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * TK_THREADS; base < n; base += (uint64_t)gridDim.x * TK_THREADS) {
    const uint64_t i = base + threadIdx.x;
    const bool in = i < n;
    const uint64_t c = in ? cnt[i] : 0;
    if (FIRST) {
      sum += c;
      hist_add(lh, in, c ? 64u - (uint32_t)__builtin_clzll(c) : 0u);
    } else {
      hist_add(lh, in && (c >> rem) == prefix, (uint32_t)(c >> shift) & (nb - 1u));
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nb; b += TK_THREADS) {
    const uint32_t v = lh[b];
    if (v) atomicAdd(&hist[b], v);  // one global add per nonzero bin per block
  }
  if (FIRST) {
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < TK_WAVES; ++w) t += wsum[w];
      if (t) atomicAdd(&st->sum, t);
    }
  }
}

// One block: the bin of the pass's histogram that holds the k-th largest row,
// from the top bin down; the state moves into that bin and the histogram is
// left zeroed for the next pass.
template <bool FIRST>
__global__ void __launch_bounds__(TK_PICK_THREADS) wc_topk_pick(TopkState* st, uint32_t* hist, uint64_t k) {
  __shared__ unsigned long long wtot[TK_PICK_THREADS / 64];
  __shared__ uint32_t top_bin;
  const uint32_t rem = FIRST ? 0u : (uint32_t)st->rem_bits;
  if (!FIRST && rem == 0) return;
  const uint32_t d = rem < (uint32_t)TK_DB ? rem : (uint32_t)TK_DB;
  const uint32_t nb = FIRST ? 65u : (1u << d);
  const uint64_t k_rem = FIRST ? k : st->k_rem;
  const uint64_t prefix = FIRST ? 0 : st->thresh, n_gt = FIRST ? 0 : st->n_gt;
  if (threadIdx.x == 0) top_bin = 0;
  // thread t owns the bins nb - 1 - r, r in [PER t, PER t + PER): descending value
  uint32_t h[TK_PICK_PER];
  unsigned long long s = 0;
#pragma unroll
  for (int j = 0; j < TK_PICK_PER; ++j) {
    const uint32_t r = threadIdx.x * TK_PICK_PER + j;
    h[j] = 0;
    if (r < nb) {
      h[j] = hist[nb - 1 - r];
      hist[nb - 1 - r] = 0;
    }
    s += h[j];
  }
  unsigned long long total;
  unsigned long long cum = block_excl<TK_PICK_THREADS>(s, wtot, total);  // rows in the bins above this thread's
#pragma unroll
  for (int j = 0; j < TK_PICK_PER; ++j) {
    const uint32_t r = threadIdx.x * TK_PICK_PER + j;
    if (h[j]) {
      const uint32_t bin = nb - 1 - r;
      if (FIRST) atomicMax(&top_bin, bin);
      if (cum < k_rem && k_rem <= cum + h[j]) {  // exactly one bin of the block
        st->n_gt = n_gt + cum;
        st->k_rem = k_rem - cum;
        if (FIRST) {  // bin b >= 1: counts in [2^(b-1), 2^b) — the top bit is fixed, b - 1 bits open
          st->thresh = bin ? 1 : 0;
          st->rem_bits = bin ? bin - 1 : 0;
        } else {
          st->thresh = (prefix << d) | bin;
          st->rem_bits = rem - d;
        }
      }
    }
    cum += h[j];
  }
  if (FIRST) {
    __syncthreads();
    if (threadIdx.x == 0) st->max_bits = top_bin;  // bit length of the largest count
  }
}

// Compaction, launch 1: per tile of TK_TILE rows, the rows above and at T.
__global__ void __launch_bounds__(TK_THREADS) wc_topk_count(const uint64_t* __restrict__ cnt, uint64_t n,
                                                            const TopkState* st, uint32_t* blk_gt, uint32_t* blk_eq) {
  __shared__ unsigned long long wsum[TK_WAVES];
  const uint64_t T = st->thresh;
  const uint64_t base = (uint64_t)blockIdx.x * TK_TILE;
  uint32_t gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < TK_ROUNDS; ++j) {
    const uint64_t i = base + (uint64_t)j * TK_THREADS + threadIdx.x;
    if (i < n) {
      const uint64_t c = cnt[i];
      gt += c > T;
      eq += c == T;
    }
  }
  const unsigned long long both = wave_sum(((unsigned long long)gt << 32) | eq);  // <= 4096 each: no carry
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = both;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < TK_WAVES; ++w) t += wsum[w];
    blk_gt[blockIdx.x] = (uint32_t)(t >> 32);
    blk_eq[blockIdx.x] = (uint32_t)t;
  }
}

// Launch 2 (one block): the tile counts -> their exclusive prefixes, in place.
__global__ void __launch_bounds__(TK_PICK_THREADS) wc_topk_scan(uint32_t* blk_gt, uint32_t* blk_eq, uint32_t nblk) {
  __shared__ unsigned long long wtot[TK_PICK_THREADS / 64];
  const uint32_t per = (nblk + TK_PICK_THREADS - 1) / TK_PICK_THREADS;
  const uint64_t b0 = (uint64_t)threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
  unsigned long long g = 0, e = 0;
  for (uint64_t b = b0; b < b1; ++b) {
    g += blk_gt[b];
    e += blk_eq[b];
  }
  unsigned long long total;
  g = block_excl<TK_PICK_THREADS>(g, wtot, total);
  e = block_excl<TK_PICK_THREADS>(e, wtot, total);
  for (uint64_t b = b0; b < b1; ++b) {
    const uint32_t x = blk_gt[b], y = blk_eq[b];
    blk_gt[b] = (uint32_t)g;
    blk_eq[b] = (uint32_t)e;
    g += x;
    e += y;
  }
}

// Launch 3: row i is selected when count > T, or count == T and fewer than
// k_rem rows at T precede it; it goes to sel[G + min(E, k_rem)], G / E = the
// rows above / at T before it — ascending row order.  A wave owns TK_WAVE_ROWS
// contiguous rows of the tile.  k1 (nullable): st->blob_bytes += the arena
// bytes of the selected rows' words.
__global__ void __launch_bounds__(TK_THREADS) wc_topk_write(const uint64_t* __restrict__ cnt, const uint64_t* k1,
                                                            const uint32_t* slen, uint64_t n, TopkState* st,
                                                            const uint32_t* blk_gt, const uint32_t* blk_eq,
                                                            uint32_t* sel, Bounds bnd) {
  __shared__ uint32_t wg[TK_WAVES], we[TK_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t T = st->thresh, ties = st->k_rem;
  const uint64_t base = (uint64_t)blockIdx.x * TK_TILE + (uint64_t)wave * TK_WAVE_ROWS;
  uint64_t c[TK_ROUNDS];
  uint32_t gt = 0, eq = 0;
#pragma unroll
  for (int j = 0; j < TK_ROUNDS; ++j) {
    const uint64_t i = base + (uint64_t)j * 64 + lane;
    c[j] = i < n ? cnt[i] : 0;
    gt += (uint32_t)__popcll(__ballot(i < n && c[j] > T));
    eq += (uint32_t)__popcll(__ballot(i < n && c[j] == T));
  }
  if (lane == 0) {
    wg[wave] = gt;
    we[wave] = eq;
  }
  __syncthreads();
  uint64_t G = blk_gt[blockIdx.x], E = blk_eq[blockIdx.x];
  for (int w = 0; w < wave; ++w) {
    G += wg[w];
    E += we[w];
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long bytes = 0;
#pragma unroll
  for (int j = 0; j < TK_ROUNDS; ++j) {
    const uint64_t i = base + (uint64_t)j * 64 + lane;
    const bool in = i < n, g = in && c[j] > T, e = in && c[j] == T;
    const unsigned long long mg = __ballot(g), me = __ballot(e);
    const uint64_t Gi = G + (uint64_t)__popcll(mg & below), Ei = E + (uint64_t)__popcll(me & below);
    if (g || (e && Ei < ties)) {
      const uint64_t pos = Gi + (Ei < ties ? Ei : ties);
      if (bounds_ok(bnd, BND_TOPK_WRITE, pos)) sel[pos] = (uint32_t)i;
      if (k1 && key_is_hashed(k1[i])) bytes += slen[i];
    }
    G += (uint64_t)__popcll(mg);
    E += (uint64_t)__popcll(me);
  }
  if (k1) {
    bytes = wave_sum(bytes);
    if (lane == 0 && bytes) atomicAdd(&st->blob_bytes, bytes);
  }
}

// Order, up to TOPK_SMALL rows: one block; row i's place is the number of rows
// before it under (count descending, selection order ascending) — the pairs
// are distinct, so the places are a permutation.
__global__ void __launch_bounds__(TK_PICK_THREADS) wc_topk_rank(const uint64_t* __restrict__ cnt, uint64_t n,
                                                                const uint32_t* sel, uint32_t m, uint32_t* out,
                                                                Bounds bnd) {
  __shared__ uint64_t sc[TOPK_SMALL];
  for (uint32_t i = threadIdx.x; i < m; i += TK_PICK_THREADS) {
    const uint32_t r = sel[i];  // a row outside the table is reported, not read
    sc[i] = bounds_ok(Bounds{bnd.err, n}, BND_TOPK_RANK, r) ? cnt[r] : 0;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < m; i += TK_PICK_THREADS) {
    const uint64_t ci = sc[i];
    uint32_t place = 0;
    for (uint32_t j = 0; j < m; ++j) {
      const uint64_t cj = sc[j];
      place += (cj > ci) || (cj == ci && j < i);
    }
    if (bounds_ok(bnd, BND_TOPK_RANK, place)) out[place] = sel[i];
  }
}

// Order above TOPK_SMALL rows: keys of the stable radix sort, ascending ~count.
__global__ void wc_topk_keys(const uint64_t* __restrict__ cnt, uint64_t n, const uint32_t* sel, uint64_t m,
                             uint64_t* keys, uint32_t* vals, Bounds bnd) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t r = sel[i];  // a row outside the table is reported, not read
    keys[i] = bounds_ok(Bounds{bnd.err, n}, BND_TOPK_RANK, r) ? ~cnt[r] : ~0ull;
    vals[i] = r;
  }
}

// out[i] = row rows[i] of the table; len[i] = the bytes its word holds in the
// arena (0: an inline key) and src[i] their arena offset.
__global__ void wc_topk_gather(TopkSrc src, const uint32_t* rows, uint64_t m, TopkDst dst, Bounds bnd) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = rows[i];
    if (!bounds_ok(bnd, BND_TOPK_GATHER, i)) continue;
    if (r >= src.n) {  // a row outside the table: reported like a row past a buffer
      bounds_ok(Bounds{bnd.err, 0}, BND_TOPK_GATHER, r);
      continue;
    }
    const uint64_t k1 = src.k1[r];
    dst.k0[i] = src.k0[r];
    dst.k1[i] = k1;
    dst.cnt[i] = src.cnt[r];
    dst.first[i] = src.first[r];
    dst.src[i] = src.soff[r];
    dst.len[i] = key_is_hashed(k1) ? src.slen[r] : 0u;
  }
}

// One block: off[i] = the exclusive prefix of len (the word's place in the blob).
__global__ void __launch_bounds__(TK_PICK_THREADS) wc_topk_offsets(const uint32_t* len, uint64_t m, uint64_t* off) {
  __shared__ unsigned long long wtot[TK_PICK_THREADS / 64];
  const uint64_t per = (m + TK_PICK_THREADS - 1) / TK_PICK_THREADS;
  const uint64_t i0 = threadIdx.x * per < m ? threadIdx.x * per : m, i1 = i0 + per < m ? i0 + per : m;
  unsigned long long s = 0;
  for (uint64_t i = i0; i < i1; ++i) s += len[i];
  unsigned long long total;
  s = block_excl<TK_PICK_THREADS>(s, wtot, total);
  for (uint64_t i = i0; i < i1; ++i) {
    off[i] = s;
    s += len[i];
  }
}

// The words' bytes, arena -> blob: a wave takes 64 rows at a time and copies
// each arena word among them with all its lanes (one lane per word would
// crawl through a 70 KB word).  A word past the blob or the arena is skipped
// and reported.
__global__ void __launch_bounds__(TK_THREADS) wc_topk_words(const uint8_t* __restrict__ arena, uint64_t arena_bytes,
                                                            const uint64_t* src, const uint32_t* len,
                                                            const uint64_t* off, uint64_t m, uint8_t* blob,
                                                            Bounds bnd) {
  const int lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * TK_THREADS + threadIdx.x) >> 6;
  const uint64_t waves = (uint64_t)gridDim.x * TK_WAVES;
  for (uint64_t base = wave * 64; base < m; base += waves * 64) {
    const uint64_t i = base + lane;
    const uint32_t l = i < m ? len[i] : 0u;
    const uint64_t s = l ? src[i] : 0, o = l ? off[i] : 0;
    unsigned long long todo = __ballot(l != 0);
    while (todo) {
      const int w = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const uint32_t wl = __shfl(l, w);
      const uint64_t ws = __shfl(s, w), wo = __shfl(o, w);
      if (ws + wl > arena_bytes) {  // wave-uniform
        if (lane == 0) bounds_ok(Bounds{bnd.err, arena_bytes}, BND_TOPK_WORDS, ws + wl);
        continue;
      }
      if (!bounds_ok(Bounds{lane == 0 ? bnd.err : nullptr, bnd.cap}, BND_TOPK_WORDS, wo + wl - 1)) continue;
      for (uint32_t b = lane; b < wl; b += 64) blob[wo + b] = arena[ws + b];
    }
  }
}

inline uint32_t grid_for(uint64_t n, uint32_t per_block, uint32_t cap) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(cap, (n + per_block - 1) / per_block));
}

}  // namespace dev

static uint64_t topk_tiles(uint64_t n) { return std::max<uint64_t>(1, (n + dev::TK_TILE - 1) / dev::TK_TILE); }

// histogram [TK_BINS] | tile counts above T [tiles] | tile counts at T [tiles]
size_t topk_select_ws_bytes(uint64_t n) { return (size_t)dev::TK_BINS * 4 + 256 + 2 * (topk_tiles(n) * 4 + 256); }

void topk_select(const uint64_t* cnt, const uint64_t* k1, const uint32_t* slen, uint64_t n, uint64_t k, void* ws,
                 TopkState* st, uint32_t* sel, hipStream_t s, const Bounds& bnd) {
  WC_CHECK(n < (1ull << 32), "topk_select: at most 2^32 - 1 rows (row indices are 32-bit)");
  WC_CHECK(k <= n, "topk_select: k exceeds the row count");
  uint8_t* p = static_cast<uint8_t*>(ws);
  uint32_t* hist = reinterpret_cast<uint32_t*>(p);
  const uint64_t tiles = topk_tiles(n);
  uint32_t* blk_gt = reinterpret_cast<uint32_t*>(p + (size_t)dev::TK_BINS * 4 + 256);
  uint32_t* blk_eq = reinterpret_cast<uint32_t*>(p + (size_t)dev::TK_BINS * 4 + 256 + tiles * 4 + 256);
  WC_HIP_CHECK(hipMemsetAsync(st, 0, sizeof(TopkState), s));
  if (n == 0) return;
  WC_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)dev::TK_BINS * 4, s));
  // ~16 rows per thread, at most 4 blocks per CU: the fold costs a block up to TK_BINS global adds
  const uint32_t hgrid = dev::grid_for(n, dev::TK_THREADS * 16, 1024);
  hipLaunchKernelGGL(dev::wc_topk_hist<true>, dim3(hgrid), dim3(dev::TK_THREADS), 0, s, cnt, n, st, hist);
  if (k == 0) return;  // the sum alone
  hipLaunchKernelGGL(dev::wc_topk_pick<true>, dim3(1), dim3(dev::TK_PICK_THREADS), 0, s, st, hist, k);
  for (int r = 0; r < dev::TK_REFINE; ++r) {  // a pass with no open bits left exits at once
    hipLaunchKernelGGL(dev::wc_topk_hist<false>, dim3(hgrid), dim3(dev::TK_THREADS), 0, s, cnt, n, st, hist);
    hipLaunchKernelGGL(dev::wc_topk_pick<false>, dim3(1), dim3(dev::TK_PICK_THREADS), 0, s, st, hist, k);
  }
  hipLaunchKernelGGL(dev::wc_topk_count, dim3((uint32_t)tiles), dim3(dev::TK_THREADS), 0, s, cnt, n, st, blk_gt,
                     blk_eq);
  hipLaunchKernelGGL(dev::wc_topk_scan, dim3(1), dim3(dev::TK_PICK_THREADS), 0, s, blk_gt, blk_eq, (uint32_t)tiles);
  hipLaunchKernelGGL(dev::wc_topk_write, dim3((uint32_t)tiles), dim3(dev::TK_THREADS), 0, s, cnt, k1, slen, n, st,
                     blk_gt, blk_eq, sel, bnd);
}

// out [m] | above TOPK_SMALL: keys, tmp keys [m], values, tmp values [m], radix workspace
size_t topk_order_ws_bytes(uint64_t m) {
  const size_t mm = m ? m : 1;
  size_t b = mm * 4 + 256;
  if (m > TOPK_SMALL) b += 2 * (mm * 8 + 256) + 2 * (mm * 4 + 256) + radix_hist_words(m) * 4 + 256;
  return b;
}

const uint32_t* topk_order(const uint64_t* cnt, uint64_t n, const uint32_t* sel, uint64_t m, int bits, void* ws,
                           hipStream_t s, const Bounds& bnd) {
  uint8_t* p = static_cast<uint8_t*>(ws);
  auto take = [&](size_t b) {
    uint8_t* r = p;
    p += (b + 255) / 256 * 256;
    return r;
  };
  const size_t mm = m ? m : 1;
  uint32_t* out = reinterpret_cast<uint32_t*>(take(mm * 4));
  if (m == 0) return out;
  if (m <= TOPK_SMALL) {
    hipLaunchKernelGGL(dev::wc_topk_rank, dim3(1), dim3(dev::TK_PICK_THREADS), 0, s, cnt, n, sel, (uint32_t)m, out,
                       bnd);
    return out;
  }
  uint64_t* keys = reinterpret_cast<uint64_t*>(take(mm * 8));
  uint64_t* tkeys = reinterpret_cast<uint64_t*>(take(mm * 8));
  uint32_t* tvals = reinterpret_cast<uint32_t*>(take(mm * 4));
  uint32_t* hist = reinterpret_cast<uint32_t*>(take(radix_hist_words(m) * 4));
  hipLaunchKernelGGL(dev::wc_topk_keys, dim3(dev::grid_for(m, 256, 2048)), dim3(256), 0, s, cnt, n, sel, m, keys, out,
                     bnd);
  bool in_tmp = false;
  // counts < 2^bits: the low `bits` bits of ~count order them (the bits above are all ones)
  radix_sort_pairs(keys, out, tkeys, tvals, hist, m, std::max(1, std::min(bits, 64)), s, &in_tmp);
  return in_tmp ? tvals : out;
}

void topk_gather(const TopkSrc& src, const uint32_t* rows, uint64_t m, const TopkDst& dst, hipStream_t s,
                 const Bounds& bnd) {
  if (m == 0) return;
  hipLaunchKernelGGL(dev::wc_topk_gather, dim3(dev::grid_for(m, 256, 2048)), dim3(256), 0, s, src, rows, m, dst, bnd);
  hipLaunchKernelGGL(dev::wc_topk_offsets, dim3(1), dim3(dev::TK_PICK_THREADS), 0, s, dst.len, m, dst.off);
}

void topk_words(const uint8_t* arena, uint64_t arena_bytes, const TopkDst& dst, uint64_t m, uint8_t* blob,
                uint64_t blob_bytes, unsigned long long* err, hipStream_t s) {
  if (m == 0 || blob_bytes == 0) return;
  hipLaunchKernelGGL(dev::wc_topk_words, dim3(dev::grid_for(m, 64 * dev::TK_WAVES, 2048)), dim3(dev::TK_THREADS), 0, s,
                     arena, arena_bytes, dst.src, dst.len, dst.off, m, blob, Bounds{err, blob_bytes});
}

}  // namespace wc
