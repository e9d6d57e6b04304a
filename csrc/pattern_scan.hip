// Multi-pattern DFA scan over a message batch.
//
// Replaces the reference's per-message regex loops (redaction
// registry.ts findMatches, claim-detector.ts, knowledge-engine
// patterns.ts, governance policy regex conditions) with one kernel: each
// thread walks the packed DFA tables (vainplex_openclaw_amd/ops/dfa.py
// MultiDFA.pack) over its message and ORs per-state accept masks into a
// u64 hit mask per message.
//
// The tables (few hundred KB) stay L2-resident; the per-family byte->class
// maps are staged in LDS. The walk is a dependent-load chain, so we give
// every thread its own message and rely on wave-level parallelism (a
// 4096-message batch = 64 waves spread over the 256 CUs).
#include "common.hpp"

// meta row: (next_base in u16 units, state_base, n_classes, class_map_row)
extern "C" __global__ void dfa_scan_kernel(
    const uint8_t* __restrict__ bytes, const int32_t* __restrict__ offsets,
    const uint16_t* __restrict__ next_tab, const unsigned long long* __restrict__ accept,
    const unsigned long long* __restrict__ eof_mask,
    const uint8_t* __restrict__ class_maps, const int32_t* __restrict__ meta,
    int n_dfas, unsigned long long* __restrict__ hits, int n_msgs) {
  extern __shared__ uint8_t lds_class[];  // n_dfas * 256
  for (int i = threadIdx.x; i < n_dfas * 256; i += blockDim.x)
    lds_class[i] = class_maps[i];
  __syncthreads();

  int mi = blockIdx.x * blockDim.x + threadIdx.x;
  if (mi >= n_msgs) return;
  int32_t lo = offsets[mi], hi = offsets[mi + 1];
  unsigned long long mask = 0ull;
  for (int d = 0; d < n_dfas; ++d) {
    int32_t next_base = meta[4 * d + 0];
    int32_t state_base = meta[4 * d + 1];
    int32_t ncls = meta[4 * d + 2];
    const uint8_t* cmap = lds_class + 256 * meta[4 * d + 3];
    uint32_t state = 0;
    mask |= accept[state_base];
    for (int32_t p = lo; p < hi; ++p) {
      uint32_t cls = cmap[bytes[p]];
      state = next_tab[next_base + state * ncls + cls];
      mask |= accept[state_base + state];
    }
    mask |= eof_mask[state_base + state];
  }
  hits[mi] = mask;
}

// Variant scanning ALL families in one launch: families are just separate
// packed MultiDFAs laid out back to back; each owns a hit column.
// hits layout: [n_families, n_msgs], zero-filled by the caller.
//
// One thread per (message, sub-DFA): grid.x covers the messages, grid.y is
// the sub-DFA, so a block walks one table with one 256 B class map in LDS
// and the walks of a message run side by side instead of one after another
// (4096 messages x 28 sub-DFAs = 1792 waves, against 64 with a thread per
// message). A thread ORs its sub-DFA's mask into its family's column with a
// 64-bit atomic. The walk itself is a chain of dependent next_tab loads; the
// message bytes are kept off that chain: they are read in aligned 16-byte
// pieces, the next piece requested before the current one is walked.
//
// A piece that would reach outside [0, n_bytes) is put together from single
// byte loads of the message's own bytes, so nothing outside the buffer is
// ever read (the payload carries no padding).
#define DFA_MULTI_THREADS 128
#define DFA_PIECE 16

DEVINL uint4 dfa_load_piece(const uint8_t* __restrict__ bytes, int p, int lo, int hi,
                            int n_bytes) {
  if (p >= 0 && p + DFA_PIECE <= n_bytes) return *(const uint4*)(bytes + p);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int i = 0; i < DFA_PIECE; ++i) {
    const int a = p + i;
    if (a >= lo && a < hi) w[i >> 2] |= (uint32_t)bytes[a] << (8 * (i & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

extern "C" __global__ void __launch_bounds__(DFA_MULTI_THREADS) dfa_scan_multi_kernel(
    const uint8_t* __restrict__ bytes, const int32_t* __restrict__ offsets,
    const uint16_t* __restrict__ next_tab, const unsigned long long* __restrict__ accept,
    const unsigned long long* __restrict__ eof_mask,
    const uint8_t* __restrict__ class_maps, const int32_t* __restrict__ meta,
    const int32_t* __restrict__ family_dfa_ranges,  // [n_families, 2] (begin, end) into meta rows
    int n_families, unsigned long long* __restrict__ hits, int n_msgs,
    int n_bytes) {
  __shared__ uint8_t cmap[256];
  const int d = blockIdx.y;
  int fam = -1;
  for (int f = 0; f < n_families; ++f)
    if (d >= family_dfa_ranges[2 * f] && d < family_dfa_ranges[2 * f + 1]) fam = f;
  if (fam < 0) return;  // a sub-DFA no family claims: block-uniform
  const int32_t next_base = meta[4 * d + 0];
  const int32_t state_base = meta[4 * d + 1];
  const uint32_t ncls = (uint32_t)meta[4 * d + 2];
  const uint8_t* cmap_g = class_maps + 256 * meta[4 * d + 3];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) cmap[i] = cmap_g[i];
  __syncthreads();

  int mi = blockIdx.x * blockDim.x + threadIdx.x;
  if (mi >= n_msgs) return;
  int32_t lo = max(offsets[mi], 0), hi = min(offsets[mi + 1], n_bytes);
  const uint16_t* nt = next_tab + next_base;
  const unsigned long long* acc = accept + state_base;
  uint32_t state = 0;
  unsigned long long mask = acc[0];
  if (lo < hi) {
    // pieces are 16-byte aligned in memory, so the first one starts at or
    // before lo (possibly before the buffer: then it takes the byte path)
    const int mis = (int)((uintptr_t)bytes & 15);
    int p = lo - ((lo + mis) & 15);
    uint4 cur = dfa_load_piece(bytes, p, lo, hi, n_bytes);
    while (true) {
      const int pn = p + DFA_PIECE;
      const bool more = pn < hi;
      uint4 nxt = make_uint4(0, 0, 0, 0);
      if (more) nxt = dfa_load_piece(bytes, pn, lo, hi, n_bytes);
      const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
      // class lookups do not depend on the state: all 16 ahead of the walk
      uint32_t cls[DFA_PIECE];
#pragma unroll
      for (int i = 0; i < DFA_PIECE; ++i) cls[i] = cmap[(w[i >> 2] >> (8 * (i & 3))) & 0xFFu];
#pragma unroll
      for (int i = 0; i < DFA_PIECE; ++i) {
        const int a = p + i;
        if (a >= lo && a < hi) {
          state = nt[state * ncls + cls[i]];
          mask |= acc[state];
        }
      }
      if (!more) break;
      cur = nxt;
      p = pn;
    }
  }
  mask |= eof_mask[state_base + state];
  // hits is zero-filled by the caller; OR commutes, so the sum over the
  // family's sub-DFAs does not depend on the order the threads arrive in
  if (mask != 0ull) atomicOr(&hits[(size_t)fam * n_msgs + mi], mask);
}
