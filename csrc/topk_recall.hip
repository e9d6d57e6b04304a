// Fused cosine-scores + streaming top-k: the Membrane salience recall
// kernel (v3).
//
// Replaces the reference Membrane plugin's salience retrieval (external
// repo; config surface in brainplex configurator.ts:137-148) with an
// LDS-tiled MFMA scan over the HBM-resident embedding shard. Scores are
// never materialized to HBM (4096 x 50M f32 would be 800 GB of traffic
// per step): each block walks its swath of the [N, D] bf16 index,
// computes 256x256 score tiles with v_mfma_f32_16x16x32_bf16 and filters
// them against per-row running top-k thresholds straight from the
// accumulator registers.
//
// v3 structure (cdna_hip_programming.md §5, 256² template geometry):
// - 512 threads (8 waves, 2M x 4N wave grid), block tile BM=256 x BN=256,
//   BK=64. Per wave: 128x64 output = 8x4 fragments of 16x16, 32
//   independent f32x4 accumulators. 2x the queries per index pass vs the
//   v2 128-tile: halves both HBM re-reads and LDS staging per FLOP.
// - global_load_lds width-16 staging; LDS image [row][8 slots of 16 B]
//   with slot ^= (row>>1)&7 — each 16-lane ds_read_b128 group covers 16
//   distinct 16 B slots across its half of the 64-bank array:
//   conflict-free (the v2 swizzle generalized to 128 B rows).
// - double-buffered LDS, one vmcnt(0)+barrier pair per K-step.
// - candidates + per-row top-k values live in GLOBAL memory
//   ([qb][swath][BM][k], host-initialized to -1e30/-1) — LDS holds only
//   tiles + thresholds + the push queue. Pushes are threshold-filtered
//   from registers (STATIC m/n/r indexing only: a dynamic index into acc
//   spills all accumulators to scratch — measured 46x), drained by one
//   row-owner thread each.
// - XCD-aware grid: flat blockIdx -> (qb = f / S, swath = f % S) with S a
//   multiple of 8 puts every co-sweeping same-swath block group on one
//   XCD (dispatch assigns XCDs round-robin), so the swath stream is
//   shared through that XCD's L2 and the L3.
#include "common.hpp"

#define BM 256
#define BN 256
#define BK 32
#define NBUF 3
#define TK_THREADS 512
#define TOPK_MAX 32
#define QCAP 2048
#define AS1 __attribute__((address_space(1)))
#define AS3 __attribute__((address_space(3)))

// LDS tile addressing: row-major [rows][BK] bf16, 64 B per row = 4 slots
// of 16 B. Swizzle: slot' = slot ^ ((row>>2)&3). That would be
// conflict-free if ds_read_b128 were served in groups of 16 contiguous
// lanes. The real groups are {0-3,12-15,20-27}, {4-11,16-19,28-31} and the
// same +32 (common.hpp, kDsReadB128Groups): in each of them this XOR puts
// two row quads on the same sixteen banks, a 2-way conflict on every
// fragment read (static_assert in common.hpp). Kept for v1..v9 and the
// bf16/fp8/mx kernels, which are A/B baselines off the bench path.
DEVINL uint32_t lds_off_bytes(uint32_t row, uint32_t slot) {
  return (row * 4u + frag_swz_slot_contig(row, slot)) * 16u;
}

// The same image with the swizzle that is conflict-free on the real lane
// groups (frag_swz_slot, proven in common.hpp). SWZ selects the slot
// function: 0 = the contiguous-group XOR above, 1 = group-aware.
template <int SWZ>
DEVINL uint32_t swz_slot(uint32_t row, uint32_t slot) {
  if constexpr (SWZ) return frag_swz_slot(row, slot);
  else return frag_swz_slot_contig(row, slot);
}
template <int SWZ>
DEVINL uint32_t lds_off_bytes_swz(uint32_t row, uint32_t slot) {
  return (row * 4u + swz_slot<SWZ>(row, slot)) * 16u;
}

// Stage a [rows x BK] tile into LDS via global_load_lds. Destination is
// linear in piece index (the hardware adds lane*16 to the wave-uniform
// base); the swizzle is applied on the SOURCE slot (involution with the
// read side).
DEVINL void stage_tile(const bf16* __restrict__ src, long long ld,
                       long long row0, long long row_max, int k0,
                       bf16* lds_base, int tile_rows) {
  int n_pieces = tile_rows * 4;  // 16 B pieces
  int w = wave_id();
  int lane = lane_id();
  for (int piece0 = w * WAVE; piece0 < n_pieces; piece0 += TK_THREADS) {
    int piece = piece0 + lane;
    uint32_t r = piece >> 2;
    uint32_t slot = piece & 3;
    uint32_t src_slot = slot ^ ((r >> 2u) & 3u);
    long long gr = row0 + r;
    if (gr >= row_max) gr = row_max - 1;  // clamp: garbage filtered later
    const bf16* p = src + gr * ld + k0 + src_slot * 8;
    int piece0_u = __builtin_amdgcn_readfirstlane(piece0);
    auto ldst = (AS3 char*)lds_base + piece0_u * 16;
    __builtin_amdgcn_global_load_lds(
        (const AS1 void*)p, (AS3 void*)ldst, 16, 0, 0);
  }
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_recall_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ X,
                   int nq, int nx, int D, int k, int n_swaths,
                   float* __restrict__ cand_scores,
                   int32_t* __restrict__ cand_ids,
                   // threshold mode (theta != nullptr): append every score
                   // > theta[row] to a per-query global candidate buffer —
                   // no queue, no drain, no per-tile barriers. cand_scores/
                   // cand_ids are then [nq][cap]; tc_n[nq] counts appends.
                   const float* __restrict__ theta,
                   int32_t* __restrict__ tc_n, int cap,
                   // owner filter (both nullptr = off): a (query, row) pair
                   // is eligible iff qowner[query] < 0 or xowner[row] ==
                   // qowner[query]; ineligible scores are dropped before
                   // the append / push
                   const int32_t* __restrict__ xowner,
                   const int32_t* __restrict__ qowner) {
  // Triple-buffered Q+X K-tiles: staging runs TWO K-steps ahead of
  // compute, synchronized with counted s_waitcnt vmcnt(4) + raw
  // s_barrier. (__syncthreads() makes the compiler drain the whole
  // global_load_lds queue at every barrier — the ~20% stall the guide
  // documents — and a 1-deep double buffer forces vmcnt(0) anyway.)
  __shared__ bf16 lds_all[NBUF * (BM + BN) * BK];
#define QS(buf) (lds_all + (buf) * BM * BK)
#define XS(buf) (lds_all + NBUF * BM * BK + (buf) * BN * BK)
  __shared__ float row_min[BM];
  __shared__ int row_min_slot[BM];
  // top-k VALUES live in LDS: the drain's insert+min-rescan is then a
  // pure-LDS dependent chain instead of serial L2 round trips (measured
  // ~2.4 us per insert through global memory). Ids go straight to
  // global (write-only); scores are written out once per block at the
  // end of the sweep.
  __shared__ float topk_vals[BM][TOPK_MAX];
  __shared__ float q_score[QCAP];
  __shared__ uint32_t q_meta[QCAP];  // (row<<16) | col_in_tile
  __shared__ int q_count;
  __shared__ int q_overflow;
  // conservative per-half-block threshold minima (rows 0-127 / 128-255):
  // a wave whose 128 accumulator values all fall below its half's min
  // skips the entire push scan for the tile (steady-state pushes are
  // rare; the scan's fixed cost measured ~half of kernel time)
  __shared__ float block_tmin[2];
  __shared__ int tmin_dirty;
  __shared__ int32_t row_owner[BM];  // owner filter: -1 = sees every row

  int S = n_swaths;
  int qb = blockIdx.x / S;      // same-swath groups land on one XCD
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x) {
    // threshold mode reuses row_min as the per-row fixed threshold
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
    row_min_slot[i] = 0;
    row_owner[i] = (qowner != nullptr && row0 + i < nq) ? qowner[row0 + i] : -1;
  }
  for (int i = threadIdx.x; i < BM * TOPK_MAX; i += blockDim.x)
    topk_vals[i / TOPK_MAX][i % TOPK_MAX] = -1e30f;
  if (threadIdx.x == 0) {
    q_count = 0; q_overflow = 0; tmin_dirty = 0;
    block_tmin[0] = -1e30f; block_tmin[1] = -1e30f;
  }
  __syncthreads();

  int wid = wave_id();              // 0..7
  int wm = wid >> 2, wn = wid & 3;  // 2 x 4 wave grid
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;             // 0..3 -> 16 B k-group within 32 elems
  int nk = D / BK;
  // candidate slice this block owns: [qb][swath][BM][k]
  size_t cbase = (((size_t)qb * S) + swath) * (size_t)BM * k;

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    // prologue: 2 K-tiles in flight (each stage = 4 glds per lane:
    // 2 for the Q tile + 2 for the X tile)
    stage_tile(Q, D, row0, nq, 0, QS(0), BM);
    stage_tile(X, D, x0, (long long)nx, 0, XS(0), BN);
    stage_tile(Q, D, row0, nq, BK, QS(1), BM);
    stage_tile(X, D, x0, (long long)nx, BK, XS(1), BN);
    for (int kt = 0; kt < nk; ++kt) {
      int cur = kt % NBUF;
      // stage(kt) landed when only stage(kt+1)'s 4 glds are outstanding
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      // raw barrier: (a) stage(kt) visible block-wide, (b) every wave is
      // done computing kt-1, so its buffer ((kt+2) % NBUF) is free.
      // Safe without the __syncthreads() fence: all LDS reads of kt-1
      // were consumed by mfma issue before this point.
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nk) {
        int pre = (kt + 2) % NBUF;
        stage_tile(Q, D, row0, nq, (kt + 2) * BK, QS(pre), BM);
        stage_tile(X, D, x0, (long long)nx, (kt + 2) * BK, XS(pre), BN);
      }
      // Fragment loads as ONE inline-asm block: a plain ds_read after
      // global_load_lds makes the memory legalizer insert s_waitcnt
      // vmcnt(0) (it cannot prove the read targets an already-landed
      // buffer), which drains the 2-deep prefetch every K-step — the
      // exact stall the guide's "inline-asm K-loop" path removes. The
      // swizzle term (lrow>>2)&3 is invariant across fragments (row
      // deltas are multiples of 16), so fragments sit at base + n*1024.
      uint32_t base_x = (uint32_t)(size_t)XS(cur)
                        + lds_off_bytes(wn * 64 + lrow, kgrp);
      uint32_t base_q = (uint32_t)(size_t)QS(cur)
                        + lds_off_bytes(wm * 128 + lrow, kgrp);
      // two 6-read asm blocks (xf[4]+qf[0..1], then qf[2..7]) halve the
      // peak early-clobber register footprint vs one 12-read block; the
      // first mfma quads overlap the second block's LDS latency
      bf16x8 xf[4], qf[8];
      asm volatile(
          "ds_read_b128 %0, %6\n\t"
          "ds_read_b128 %1, %6 offset:1024\n\t"
          "ds_read_b128 %2, %6 offset:2048\n\t"
          "ds_read_b128 %3, %6 offset:3072\n\t"
          "ds_read_b128 %4, %7\n\t"
          "ds_read_b128 %5, %7 offset:1024\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
            "=&v"(qf[0]), "=&v"(qf[1])
          : "v"(base_x), "v"(base_q));
      asm volatile(
          "ds_read_b128 %0, %6 offset:2048\n\t"
          "ds_read_b128 %1, %6 offset:3072\n\t"
          "ds_read_b128 %2, %6 offset:4096\n\t"
          "ds_read_b128 %3, %6 offset:5120\n\t"
          "ds_read_b128 %4, %6 offset:6144\n\t"
          "ds_read_b128 %5, %6 offset:7168\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(qf[2]), "=&v"(qf[3]), "=&v"(qf[4]), "=&v"(qf[5]),
            "=&v"(qf[6]), "=&v"(qf[7])
          : "v"(base_q));
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qf[m], xf[n], acc[m][n], 0, 0, 0);
#pragma unroll
      for (int m = 2; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qf[m], xf[n], acc[m][n], 0, 0, 0);
    }
    // drain remaining staging and make the last compute visible before
    // the push phase reuses LDS-adjacent state
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {  // scan-only diagnosis mode: keep acc live, skip top-k
      if (acc[0][0][0] > 1e29f) cand_scores[cbase] = acc[0][0][0];
      continue;
    }
    if (theta != nullptr) {
      // threshold mode: fixed per-row thresholds (LDS), rare global
      // atomic appends, zero epilogue barriers
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
            float v = acc[m][n][r];
            if (!(v > row_min[row])) continue;
            long long grow = row0 + row;
            if (grow >= nq) continue;
            long long col = x0 + wn * 64 + n * 16 + (lane & 15);
            if (col >= x_end) continue;
            if (xowner != nullptr) {
              int32_t qo = row_owner[row];
              if (qo >= 0 && xowner[col] != qo) continue;
            }
            int pos = atomicAdd(&tc_n[grow], 1);
            if (pos < cap) {
              cand_scores[grow * cap + pos] = v;
              cand_ids[grow * cap + pos] = int32_t(col);
            }
          }
      continue;
    }
    // ---- streaming top-k from the accumulators -------------------------
    // lane holds acc[m][n][r] at row = wm*128 + m*16 + (lane>>4)*4 + r,
    //                         col = wn*64  + n*16 + (lane&15)
    // Rounds: push survivors into the queue; drain by row-owner threads;
    // repeat if the queue overflowed (only plausible on the first tiles).
    // wave early-out: max over this lane's 128 values (registers only),
    // reduced across the wave, vs the conservative min of the wave's
    // row thresholds — steady-state tiles push nothing and skip the
    // whole scan
    float vmax = -1e30f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) vmax = fmaxf(vmax, acc[m][n][r]);
    for (int off = 32; off; off >>= 1) vmax = fmaxf(vmax, __shfl_down(vmax, off));
    vmax = __shfl(vmax, 0);
    bool wave_skip = !(vmax > block_tmin[wm]);
    unsigned long long pend0 = ~0ull, pend1 = ~0ull;  // 128 pending bits
    for (int round = 0; ; ++round) {
      unsigned long long still0 = 0ull, still1 = 0ull;
      if (!wave_skip)
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int vi = (m & 3) * 16 + n * 4 + r;
            unsigned long long bit = 1ull << vi;
            if (!(((m < 4) ? pend0 : pend1) & bit)) continue;
            int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
            if ((row0 + row) >= nq) continue;
            long long col = x0 + wn * 64 + n * 16 + (lane & 15);
            if (col >= x_end) continue;
            float v = acc[m][n][r];
            if (!(v > row_min[row])) continue;
            if (xowner != nullptr) {
              int32_t qo = row_owner[row];
              if (qo >= 0 && xowner[col] != qo) continue;
            }
            int idx = atomicAdd(&q_count, 1);
            if (idx < QCAP) {
              q_score[idx] = v;
              q_meta[idx] = (uint32_t(row) << 16) | uint32_t(col - x0);
            } else {
              if (m < 4) still0 |= bit; else still1 |= bit;
              atomicExch(&q_overflow, 1);
            }
          }
      __syncthreads();
      if (q_count == 0) { __syncthreads(); break; }  // uniform: no pushes
      // drain: thread t < BM owns row t; candidate state is in GLOBAL
      // memory (block-private slice, L2-hot)
      int total = min(q_count, QCAP);
      if (threadIdx.x < BM) {
        int my_row = threadIdx.x;
        float rmin = row_min[my_row];
        int rslot = row_min_slot[my_row];
        float* vals = topk_vals[my_row];
        int32_t* ci = cand_ids + cbase + (size_t)my_row * k;
        bool touched = false;
        for (int i = 0; i < total; ++i) {
          uint32_t meta = q_meta[i];
          if (int(meta >> 16) != my_row) continue;
          float v = q_score[i];
          if (v > rmin) {
            vals[rslot] = v;
            ci[rslot] = int32_t(x0 + (meta & 0xFFFFu));  // write-only
            float mn = vals[0];
            int ms = 0;
            for (int j = 1; j < k; ++j)
              if (vals[j] < mn) { mn = vals[j]; ms = j; }
            rmin = mn;
            rslot = ms;
            touched = true;
          }
        }
        if (touched) {
          row_min[my_row] = rmin;
          row_min_slot[my_row] = rslot;
          tmin_dirty = 1;  // any-writer, same value
        }
      }
      __syncthreads();
      int of = q_overflow;
      __syncthreads();  // all reads of q_overflow done before the reset
      if (threadIdx.x == 0) { q_count = 0; q_overflow = 0; }
      pend0 = still0;
      pend1 = still1;
      if (!of) break;   // of is uniform (LDS): no divergence
      __syncthreads();  // reset visible before next round's pushes
    }
    __syncthreads();
    if (tmin_dirty) {
      if (threadIdx.x < 2) {
        float mn = row_min[threadIdx.x * 128];
        for (int j = 1; j < 128; ++j)
          mn = fminf(mn, row_min[threadIdx.x * 128 + j]);
        block_tmin[threadIdx.x] = mn;
      }
      __syncthreads();  // tmin visible before the next tile's skip test
      if (threadIdx.x == 0) tmin_dirty = 0;
    }
  }
  // scores out: one pass from LDS (ids were streamed during drains);
  // threshold mode wrote its buffers inline
  if (theta == nullptr && k > 0)
    for (int i = threadIdx.x; i < BM * k; i += blockDim.x)
      cand_scores[cbase + (size_t)(i / k) * k + (i % k)] = topk_vals[i / k][i % k];
}

// Merge per-swath candidates into final [nq][k] (one wave per query).
extern "C" __global__ void topk_merge_kernel(
    const float* __restrict__ cand_scores, const int32_t* __restrict__ cand_ids,
    int nq, int k, int n_swaths, float* __restrict__ out_scores,
    int32_t* __restrict__ out_ids) {
  int q = blockIdx.x * (blockDim.x / WAVE) + wave_id();
  if (q >= nq) return;
  int lane = lane_id();
  int qb = q / BM, row = q % BM;
  int total = n_swaths * k;
  float my_s[16];
  int32_t my_i[16];
  int per_lane = (total + WAVE - 1) / WAVE;
  for (int j = 0; j < per_lane; ++j) {
    int idx = j * WAVE + lane;
    if (idx < total) {
      int sw = idx / k, slot = idx % k;
      size_t base = (((size_t)qb * n_swaths) + sw) * BM * k + (size_t)row * k;
      my_s[j] = cand_scores[base + slot];
      my_i[j] = cand_ids[base + slot];
    } else {
      my_s[j] = -1e30f;
      my_i[j] = -1;
    }
  }
  for (int sel = 0; sel < k; ++sel) {
    float best = -1e30f;
    int bj = -1;
    for (int j = 0; j < per_lane; ++j)
      if (my_s[j] > best) { best = my_s[j]; bj = j; }
    float wbest = best;
    int wlane = lane;
    for (int off = 32; off; off >>= 1) {
      float o = __shfl_down(wbest, off);
      int ol = __shfl_down(wlane, off);
      if (o > wbest) { wbest = o; wlane = ol; }
    }
    wbest = __shfl(wbest, 0);
    wlane = __shfl(wlane, 0);
    if (lane == wlane) {
      out_scores[(size_t)q * k + sel] = wbest;
      out_ids[(size_t)q * k + sel] = (bj >= 0) ? my_i[bj] : -1;
      if (bj >= 0) my_s[bj] = -1e30f;
    }
  }
}

// ===========================================================================
// fp8 scan variant: stage-1 of the two-stage recall. Index + queries are
// OCP e4m3 (pre-scaled x8 so typical unit-vector components sit in the
// normal range); scores rank candidates only — stage-2 rescores the
// overfetched top-k2 exactly in bf16 (ops/gpu.py topk_recall_two_stage).
//
// Same geometry and byte layout as the bf16 kernel: BK_F8 = 64 fp8
// elements = the SAME 64 B rows / 4 x 16 B slots / swizzle, so
// stage_tile and the asm ds_read block carry over. Each staged tile
// feeds TWO v_mfma_f32_16x16x32_fp8_fp8 sub-steps; a lane's 16 B
// fragment holds the i64 operands for both k-halves of its slot pair
// (sub-step s reads slots {2s, 2s+1}; lane kgrp selects slot s*2 +
// (kgrp>>1), i64 half kgrp&1).
// ===========================================================================

typedef long long i64x2 __attribute__((ext_vector_type(2)));
#define BK_F8 64
#define NBUF_F8 3

DEVINL void stage_tile8(const uint8_t* __restrict__ src, long long ld,
                        long long row0, long long row_max, int k0,
                        bf16* lds_base, int tile_rows) {
  // identical piece layout: 64 B rows = 4 x 16 B swizzled slots
  stage_tile((const bf16*)src, ld / 2, row0, row_max, k0 / 2, lds_base, tile_rows);
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_recall_fp8_kernel(const uint8_t* __restrict__ Q, const uint8_t* __restrict__ X,
                   int nq, int nx, int D, int k, int n_swaths,
                   float* __restrict__ cand_scores,
                   int32_t* __restrict__ cand_ids,
                   // threshold mode (theta != nullptr): append every score
                   // > theta[row] to a per-query global candidate buffer —
                   // no queue, no drain, no per-tile barriers. cand_scores/
                   // cand_ids are then [nq][cap]; tc_n[nq] counts appends.
                   const float* __restrict__ theta,
                   int32_t* __restrict__ tc_n, int cap) {
  __shared__ bf16 lds_all[NBUF_F8 * (BM + BN) * (BK_F8 / 2)];
#define QS8(buf) (lds_all + (buf) * BM * (BK_F8 / 2))
#define XS8(buf) (lds_all + NBUF_F8 * BM * (BK_F8 / 2) + (buf) * BN * (BK_F8 / 2))
  __shared__ float row_min[BM];
  __shared__ int row_min_slot[BM];
  __shared__ float topk_vals[BM][TOPK_MAX];  // LDS candidate values
  __shared__ float q_score[QCAP];
  __shared__ uint32_t q_meta[QCAP];
  __shared__ int q_count;
  __shared__ int q_overflow;
  __shared__ float block_tmin[2];  // see bf16 kernel comment
  __shared__ int tmin_dirty;

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x) {
    // threshold mode reuses row_min as the per-row fixed threshold
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
    row_min_slot[i] = 0;
  }
  for (int i = threadIdx.x; i < BM * TOPK_MAX; i += blockDim.x)
    topk_vals[i / TOPK_MAX][i % TOPK_MAX] = -1e30f;
  if (threadIdx.x == 0) {
    q_count = 0; q_overflow = 0; tmin_dirty = 0;
    block_tmin[0] = -1e30f; block_tmin[1] = -1e30f;
  }
  __syncthreads();

  int wid = wave_id();
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int half = kgrp & 1;            // i64 half within the 16 B fragment
  int nk = D / BK_F8;
  size_t cbase = (((size_t)qb * S) + swath) * (size_t)BM * k;

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    for (int p = 0; p < 2 && p < nk; ++p) {
      stage_tile8(Q, D, row0, nq, p * BK_F8, QS8(p), BM);
      stage_tile8(X, D, x0, (long long)nx, p * BK_F8, XS8(p), BN);
    }
    for (int kt = 0; kt < nk; ++kt) {
      int cur = kt % NBUF_F8;
      // stage(kt) landed when only stage(kt+1)'s 4 glds are outstanding
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (kt + 2 < nk) {
        int pre = (kt + 2) % NBUF_F8;
        stage_tile8(Q, D, row0, nq, (kt + 2) * BK_F8, QS8(pre), BM);
        stage_tile8(X, D, x0, (long long)nx, (kt + 2) * BK_F8, XS8(pre), BN);
      }
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {  // k-halves 0..31, 32..63
        uint32_t slot = sub * 2 + (kgrp >> 1);
        uint32_t base_x = (uint32_t)(size_t)XS8(cur)
                          + lds_off_bytes(wn * 64 + lrow, slot);
        uint32_t base_q = (uint32_t)(size_t)QS8(cur)
                          + lds_off_bytes(wm * 128 + lrow, slot);
        bf16x8 xf[4], qf[8];
        asm volatile(
            "ds_read_b128 %0, %12\n\t"
            "ds_read_b128 %1, %12 offset:1024\n\t"
            "ds_read_b128 %2, %12 offset:2048\n\t"
            "ds_read_b128 %3, %12 offset:3072\n\t"
            "ds_read_b128 %4, %13\n\t"
            "ds_read_b128 %5, %13 offset:1024\n\t"
            "ds_read_b128 %6, %13 offset:2048\n\t"
            "ds_read_b128 %7, %13 offset:3072\n\t"
            "ds_read_b128 %8, %13 offset:4096\n\t"
            "ds_read_b128 %9, %13 offset:5120\n\t"
            "ds_read_b128 %10, %13 offset:6144\n\t"
            "ds_read_b128 %11, %13 offset:7168\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
              "=&v"(qf[0]), "=&v"(qf[1]), "=&v"(qf[2]), "=&v"(qf[3]),
              "=&v"(qf[4]), "=&v"(qf[5]), "=&v"(qf[6]), "=&v"(qf[7])
            : "v"(base_x), "v"(base_q));
        long long xv[4], qv[8];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          i64x2 t = __builtin_bit_cast(i64x2, xf[n]);
          xv[n] = half ? t.y : t.x;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          i64x2 t = __builtin_bit_cast(i64x2, qf[m]);
          qv[m] = half ? t.y : t.x;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
                qv[m], xv[n], acc[m][n], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[cbase] = acc[0][0][0];
      continue;
    }
    if (theta != nullptr) {
      // threshold mode: fixed per-row thresholds (LDS), rare global
      // atomic appends, zero epilogue barriers
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
            float v = acc[m][n][r];
            if (!(v > row_min[row])) continue;
            long long grow = row0 + row;
            if (grow >= nq) continue;
            long long col = x0 + wn * 64 + n * 16 + (lane & 15);
            if (col >= x_end) continue;
            int pos = atomicAdd(&tc_n[grow], 1);
            if (pos < cap) {
              cand_scores[grow * cap + pos] = v;
              cand_ids[grow * cap + pos] = int32_t(col);
            }
          }
      continue;
    }
    // ---- streaming top-k (identical to the bf16 kernel) ----------------
    // wave early-out: max over this lane's 128 values (registers only),
    // reduced across the wave, vs the conservative min of the wave's
    // row thresholds — steady-state tiles push nothing and skip the
    // whole scan
    float vmax = -1e30f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) vmax = fmaxf(vmax, acc[m][n][r]);
    for (int off = 32; off; off >>= 1) vmax = fmaxf(vmax, __shfl_down(vmax, off));
    vmax = __shfl(vmax, 0);
    bool wave_skip = !(vmax > block_tmin[wm]);
    unsigned long long pend0 = ~0ull, pend1 = ~0ull;
    for (int round = 0; ; ++round) {
      unsigned long long still0 = 0ull, still1 = 0ull;
      if (!wave_skip)
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int vi = (m & 3) * 16 + n * 4 + r;
            unsigned long long bit = 1ull << vi;
            if (!(((m < 4) ? pend0 : pend1) & bit)) continue;
            int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
            if ((row0 + row) >= nq) continue;
            long long col = x0 + wn * 64 + n * 16 + (lane & 15);
            if (col >= x_end) continue;
            float v = acc[m][n][r];
            if (!(v > row_min[row])) continue;
            int idx = atomicAdd(&q_count, 1);
            if (idx < QCAP) {
              q_score[idx] = v;
              q_meta[idx] = (uint32_t(row) << 16) | uint32_t(col - x0);
            } else {
              if (m < 4) still0 |= bit; else still1 |= bit;
              atomicExch(&q_overflow, 1);
            }
          }
      __syncthreads();
      if (q_count == 0) { __syncthreads(); break; }  // uniform: no pushes
      int total = min(q_count, QCAP);
      if (threadIdx.x < BM) {
        int my_row = threadIdx.x;
        float rmin = row_min[my_row];
        int rslot = row_min_slot[my_row];
        float* vals = topk_vals[my_row];
        int32_t* ci = cand_ids + cbase + (size_t)my_row * k;
        bool touched = false;
        for (int i = 0; i < total; ++i) {
          uint32_t meta = q_meta[i];
          if (int(meta >> 16) != my_row) continue;
          float v = q_score[i];
          if (v > rmin) {
            vals[rslot] = v;
            ci[rslot] = int32_t(x0 + (meta & 0xFFFFu));  // write-only
            float mn = vals[0];
            int ms = 0;
            for (int j = 1; j < k; ++j)
              if (vals[j] < mn) { mn = vals[j]; ms = j; }
            rmin = mn;
            rslot = ms;
            touched = true;
          }
        }
        if (touched) {
          row_min[my_row] = rmin;
          row_min_slot[my_row] = rslot;
          tmin_dirty = 1;  // any-writer, same value
        }
      }
      __syncthreads();
      int of = q_overflow;
      __syncthreads();
      if (threadIdx.x == 0) { q_count = 0; q_overflow = 0; }
      pend0 = still0;
      pend1 = still1;
      if (!of) break;
      __syncthreads();
    }
    __syncthreads();
    if (tmin_dirty) {
      if (threadIdx.x < 2) {
        float mn = row_min[threadIdx.x * 128];
        for (int j = 1; j < 128; ++j)
          mn = fminf(mn, row_min[threadIdx.x * 128 + j]);
        block_tmin[threadIdx.x] = mn;
      }
      __syncthreads();  // tmin visible before the next tile's skip test
      if (threadIdx.x == 0) tmin_dirty = 0;
    }
  }
  if (theta == nullptr && k > 0)
    for (int i = threadIdx.x; i < BM * k; i += blockDim.x)
      cand_scores[cbase + (size_t)(i / k) * k + (i % k)] = topk_vals[i / k][i % k];
}

// ===========================================================================
// MX-scaled threshold scan: the fp8 scan rebuilt on
// v_mfma_scale_f32_16x16x128_f8f6f4 with unit e8m0 scales (0x7F = x1), so
// it consumes the SAME pre-scaled e4m3 index bytes. K=128 per issue is
// 2.25x the non-scaled fp8 MFMA rate (4661 vs 2075 TF/s peak), and each
// staged byte feeds exactly one ds_read instead of two — the fp8 scan
// measured at 67% of its MFMA issue peak, so issue pressure, not bytes,
// was the next wall.
//
// Staging is unchanged (64 B rows / 4 swizzled 16 B slots, stage_tile8,
// counted-vmcnt GLDS pipeline) but tiles are consumed in PAIRS: a lane's
// 32 B operand (k = kgrp*32 + [0,32)) is source slots {s0, s0+1} of tile
// (pair, kgrp>>1) with s0 = (kgrp&1)*2. The swizzle term ((row>>2)&3) is
// lrow-only (fragment row deltas are multiples of 16), so each matrix
// needs two base addresses (lo/hi slot) and fragments sit at +1024 asm
// offsets, exactly like the bf16 kernel's read blocks. NBUF_MX=4 x
// (BM+BN) x 64 B = 128 KB LDS (threshold mode carries no top-k state);
// prefetch is one pair (= two tiles, 8 per-lane glds) deep:
// s_waitcnt vmcnt(8). Threshold mode + the k<0 scan-only diagnostic.
// ===========================================================================

#define NBUF_MX 4
typedef int v8i_mx __attribute__((ext_vector_type(8)));

DEVINL v8i_mx mx_frag(bf16x8 lo, bf16x8 hi) {
  int4 l = __builtin_bit_cast(int4, lo), h = __builtin_bit_cast(int4, hi);
  v8i_mx f;
  f[0] = l.x; f[1] = l.y; f[2] = l.z; f[3] = l.w;
  f[4] = h.x; f[5] = h.y; f[6] = h.z; f[7] = h.w;
  return f;
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_mx_kernel(const uint8_t* __restrict__ Q, const uint8_t* __restrict__ X,
                    int nq, int nx, int D, int k, int n_swaths,
                    float* __restrict__ cand_scores,
                    int32_t* __restrict__ cand_ids,
                    const float* __restrict__ theta,
                    int32_t* __restrict__ tc_n, int cap) {
  __shared__ bf16 lds_mx[NBUF_MX * (BM + BN) * BK];
#define QSM(buf) (lds_mx + (buf) * BM * BK)
#define XSM(buf) (lds_mx + NBUF_MX * BM * BK + (buf) * BN * BK)
  __shared__ float row_min[BM];

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x)
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
  __syncthreads();

  int wid = wave_id();
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;             // k-block (of 32) within the 128 pair
  int th = kgrp >> 1;               // which tile of the pair holds it
  int s0 = (kgrp & 1) * 2;          // source slot pair base within that tile
  int np = D / (2 * BK_F8);         // K pairs of 128
  size_t cbase = (((size_t)qb * S) + swath) * (size_t)BM * k;
  const int unit_scale = 0x7F7F7F7F;  // e8m0 biased-127 exponent = x1.0

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    // prologue: two PAIRS (four tiles) in flight = 16 per-lane glds
    for (int t = 0; t < 4 && t < 2 * np; ++t) {
      stage_tile8(Q, D, row0, nq, t * BK_F8, QSM(t & 3), BM);
      stage_tile8(X, D, x0, (long long)nx, t * BK_F8, XSM(t & 3), BN);
    }
    for (int p = 0; p < np; ++p) {
      // pair p landed when at most pair p+1's 8 glds are outstanding;
      // on the final pair nothing else is in flight, so count to zero
      if (p + 1 < np)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      int buf = (2 * p + th) & 3;
      uint32_t r3 = ((uint32_t)lrow >> 2u) & 3u;
      uint32_t off_lo = ((uint32_t)s0 ^ r3) * 16u;
      uint32_t off_hi = (((uint32_t)s0 + 1u) ^ r3) * 16u;
      uint32_t xrow = (uint32_t)(wn * 64 + lrow) * 64u;
      uint32_t qrow = (uint32_t)(wm * 128 + lrow) * 64u;
      uint32_t xlo = (uint32_t)(size_t)XSM(buf) + xrow + off_lo;
      uint32_t xhi = (uint32_t)(size_t)XSM(buf) + xrow + off_hi;
      uint32_t qlo = (uint32_t)(size_t)QSM(buf) + qrow + off_lo;
      uint32_t qhi = (uint32_t)(size_t)QSM(buf) + qrow + off_hi;
      bf16x8 xl[4], xh[4], ql[8], qh[8];
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:1024\n\t"
          "ds_read_b128 %2, %8 offset:2048\n\t"
          "ds_read_b128 %3, %8 offset:3072\n\t"
          "ds_read_b128 %4, %9\n\t"
          "ds_read_b128 %5, %9 offset:1024\n\t"
          "ds_read_b128 %6, %9 offset:2048\n\t"
          "ds_read_b128 %7, %9 offset:3072\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(xl[0]), "=&v"(xl[1]), "=&v"(xl[2]), "=&v"(xl[3]),
            "=&v"(xh[0]), "=&v"(xh[1]), "=&v"(xh[2]), "=&v"(xh[3])
          : "v"(xlo), "v"(xhi));
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:1024\n\t"
          "ds_read_b128 %2, %8 offset:2048\n\t"
          "ds_read_b128 %3, %8 offset:3072\n\t"
          "ds_read_b128 %4, %9\n\t"
          "ds_read_b128 %5, %9 offset:1024\n\t"
          "ds_read_b128 %6, %9 offset:2048\n\t"
          "ds_read_b128 %7, %9 offset:3072\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(ql[0]), "=&v"(ql[1]), "=&v"(ql[2]), "=&v"(ql[3]),
            "=&v"(qh[0]), "=&v"(qh[1]), "=&v"(qh[2]), "=&v"(qh[3])
          : "v"(qlo), "v"(qhi));
      asm volatile(
          "ds_read_b128 %0, %8 offset:4096\n\t"
          "ds_read_b128 %1, %8 offset:5120\n\t"
          "ds_read_b128 %2, %8 offset:6144\n\t"
          "ds_read_b128 %3, %8 offset:7168\n\t"
          "ds_read_b128 %4, %9 offset:4096\n\t"
          "ds_read_b128 %5, %9 offset:5120\n\t"
          "ds_read_b128 %6, %9 offset:6144\n\t"
          "ds_read_b128 %7, %9 offset:7168\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(ql[4]), "=&v"(ql[5]), "=&v"(ql[6]), "=&v"(ql[7]),
            "=&v"(qh[4]), "=&v"(qh[5]), "=&v"(qh[6]), "=&v"(qh[7])
          : "v"(qlo), "v"(qhi));
      // every wave now holds pair p in registers; after this barrier the
      // pair's buffers are dead and pair p+2 can stage into them while
      // the MFMAs run (tiles t and t+4 share a buffer: NBUF_MX = 4)
      __builtin_amdgcn_s_barrier();
      if (2 * p + 4 < 2 * np) {
        stage_tile8(Q, D, row0, nq, (2 * p + 4) * BK_F8, QSM((2 * p + 4) & 3), BM);
        stage_tile8(X, D, x0, (long long)nx, (2 * p + 4) * BK_F8, XSM((2 * p + 4) & 3), BN);
        stage_tile8(Q, D, row0, nq, (2 * p + 5) * BK_F8, QSM((2 * p + 5) & 3), BM);
        stage_tile8(X, D, x0, (long long)nx, (2 * p + 5) * BK_F8, XSM((2 * p + 5) & 3), BN);
      }
      v8i_mx xv[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) xv[n] = mx_frag(xl[n], xh[n]);
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        v8i_mx qv = mx_frag(ql[m], qh[m]);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              qv, xv[n], acc[m][n], 0, 0, 0, unit_scale, 0, unit_scale);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {  // scan-only diagnosis mode
      if (acc[0][0][0] > 1e29f) cand_scores[cbase] = acc[0][0][0];
      continue;
    }
    // threshold appends (identical to the fp8 kernel's threshold branch)
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
          float v = acc[m][n][r];
          if (!(v > row_min[row])) continue;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          }
        }
  }
}

// ===========================================================================
// MX fp8xfp4 threshold scan: Q stays e4m3 (cbsz=0, unit scales); X is
// MXFP4 — e2m1 nibbles (two per byte, low nibble = even k) with one
// e8m0 scale per 32-element block (blgp=4). The scan is at the GLDS
// transport ceiling, so halving the X bytes (64 B per 128-k row + 32 B
// of scales per full row) buys what no MFMA-side change can.
//
// Geometry: Q staging identical to topk_scan_mx_kernel. X4 rows are
// D/2 bytes; one 128-k PAIR of X is a single 64 B-row tile (4 swizzled
// slots), so a lane's B fragment is ONE ds_read_b128 at slot kgrp —
// the bf16 kernel's X read pattern. Scales are staged once per x-tile
// (BN x D/32 bytes, linear rows) and read per pair as ds_read_u8.
// Per-pair staging = 6 per-lane glds (Q 2x2 + X4 2): s_waitcnt vmcnt(6).
// ===========================================================================

#define MX4_SMAX 64  // max D/32 scale bytes per row (D <= 2048)

DEVINL void stage_scale_rows(const uint8_t* __restrict__ src, int sb,
                             long long row0, long long row_max,
                             uint8_t* lds_base, int tile_rows) {
  // scale sheet: tile_rows x sb bytes, staged as LINEAR bytes (no
  // swizzle: the consumers are byte reads). A piece that starts past the
  // array's last whole piece is taken from that last piece, so every byte
  // of a live row comes from its own place and garbage scales only ever
  // land on rows the epilogue bound-checks away. That needs a piece that
  // never straddles the array's end: 16 B pieces when rows are whole
  // 16 B multiples (sb % 16 == 0; row0*sb is 16-aligned, row0 being a
  // multiple of 256), dword pieces otherwise (sb is always a multiple of
  // 4). The sheet is a multiple of 64 pieces either way, so whole waves
  // issue. The dword path is off the production depths (D = 512, 1024).
  long long base = row0 * (long long)sb;
  long long total = row_max * (long long)sb;
  int w = wave_id();
  int lane = lane_id();
  if ((sb & 15) == 0) {
    long long last = total - 16;
    int n_pieces = tile_rows * sb / 16;
    for (int piece0 = w * WAVE; piece0 < n_pieces; piece0 += TK_THREADS) {
      int piece = piece0 + lane;
      long long off = base + (long long)piece * 16;
      if (off > last) off = last;
      int piece0_u = __builtin_amdgcn_readfirstlane(piece0);
      auto ldst = (AS3 char*)lds_base + piece0_u * 16;
      __builtin_amdgcn_global_load_lds((const AS1 void*)(src + off),
                                       (AS3 void*)ldst, 16, 0, 0);
    }
  } else {
    long long last = total - 4;
    int n_pieces = tile_rows * sb / 4;
    for (int piece0 = w * WAVE; piece0 < n_pieces; piece0 += TK_THREADS) {
      int piece = piece0 + lane;
      long long off = base + (long long)piece * 4;
      if (off > last) off = last;
      int piece0_u = __builtin_amdgcn_readfirstlane(piece0);
      auto ldst = (AS3 char*)lds_base + piece0_u * 4;
      __builtin_amdgcn_global_load_lds((const AS1 void*)(src + off),
                                       (AS3 void*)ldst, 4, 0, 0);
    }
  }
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_mx4_kernel(const uint8_t* __restrict__ Q, const uint8_t* __restrict__ X4,
                     const uint8_t* __restrict__ XS,
                     int nq, int nx, int D, int k, int n_swaths,
                     float* __restrict__ cand_scores,
                     int32_t* __restrict__ cand_ids,
                     const float* __restrict__ theta,
                     int32_t* __restrict__ tc_n, int cap) {
  __shared__ bf16 lds_q4[NBUF_MX * BM * BK];          // 64 KB
  __shared__ bf16 lds_x4[2 * BN * BK];                // 32 KB (2 pair-bufs)
  __shared__ uint8_t lds_xs[BN * MX4_SMAX];           // 16 KB scale sheet
  __shared__ float row_min[BM];
#define QS4(buf) (lds_q4 + (buf) * BM * BK)
#define XS4(buf) (lds_x4 + (buf) * BN * BK)

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x)
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
  __syncthreads();

  int wid = wave_id();
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int th = kgrp >> 1;
  int s0 = (kgrp & 1) * 2;
  int np = D / (2 * BK_F8);
  int sb = D / 32;                  // scale bytes per X row
  size_t cbase = (((size_t)qb * S) + swath) * (size_t)BM * k;
  const int unit_scale = 0x7F7F7F7F;
  long long x4_ld = D / 4;          // X4 row length in bf16 units (D/2 bytes)

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    // prologue: scale sheet + two pairs in flight (1 + 2x6 glds)
    stage_scale_rows(XS, sb, x0, (long long)nx, lds_xs, BN);
    for (int pp = 0; pp < 2 && pp < np; ++pp) {
      stage_tile8(Q, D, row0, nq, (2 * pp) * BK_F8, QS4((2 * pp) & 3), BM);
      stage_tile8(Q, D, row0, nq, (2 * pp + 1) * BK_F8, QS4((2 * pp + 1) & 3), BM);
      stage_tile((const bf16*)X4, x4_ld, x0, (long long)nx, pp * 32, XS4(pp & 1), BN);
    }
    for (int p = 0; p < np; ++p) {
      if (p + 1 < np)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      int buf = (2 * p + th) & 3;
      uint32_t r3 = ((uint32_t)lrow >> 2u) & 3u;
      uint32_t off_lo = ((uint32_t)s0 ^ r3) * 16u;
      uint32_t off_hi = (((uint32_t)s0 + 1u) ^ r3) * 16u;
      uint32_t qrow = (uint32_t)(wm * 128 + lrow) * 64u;
      uint32_t qlo = (uint32_t)(size_t)QS4(buf) + qrow + off_lo;
      uint32_t qhi = (uint32_t)(size_t)QS4(buf) + qrow + off_hi;
      // X fragment: one b128 at slot kgrp of the pair-row
      uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
      uint32_t xaddr = (uint32_t)(size_t)XS4(p & 1)
                       + lds_off_bytes(xrow_base, (uint32_t)kgrp);
      // per-n scale byte: lds_xs[row * sb + p*4 + kgrp]
      uint32_t saddr = (uint32_t)(size_t)lds_xs + xrow_base * (uint32_t)sb
                       + (uint32_t)(p * 4 + kgrp);
      uint32_t sstride = 16u * (uint32_t)sb;
      bf16x8 xf[4], ql[8], qh[8];
      uint32_t sv[4];
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:1024\n\t"
          "ds_read_b128 %2, %8 offset:2048\n\t"
          "ds_read_b128 %3, %8 offset:3072\n\t"
          "ds_read_u8 %4, %9\n\t"
          "ds_read_u8 %5, %10\n\t"
          "ds_read_u8 %6, %11\n\t"
          "ds_read_u8 %7, %12\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
            "=&v"(sv[0]), "=&v"(sv[1]), "=&v"(sv[2]), "=&v"(sv[3])
          : "v"(xaddr), "v"(saddr), "v"(saddr + sstride),
            "v"(saddr + 2 * sstride), "v"(saddr + 3 * sstride));
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:1024\n\t"
          "ds_read_b128 %2, %8 offset:2048\n\t"
          "ds_read_b128 %3, %8 offset:3072\n\t"
          "ds_read_b128 %4, %9\n\t"
          "ds_read_b128 %5, %9 offset:1024\n\t"
          "ds_read_b128 %6, %9 offset:2048\n\t"
          "ds_read_b128 %7, %9 offset:3072\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(ql[0]), "=&v"(ql[1]), "=&v"(ql[2]), "=&v"(ql[3]),
            "=&v"(qh[0]), "=&v"(qh[1]), "=&v"(qh[2]), "=&v"(qh[3])
          : "v"(qlo), "v"(qhi));
      asm volatile(
          "ds_read_b128 %0, %8 offset:4096\n\t"
          "ds_read_b128 %1, %8 offset:5120\n\t"
          "ds_read_b128 %2, %8 offset:6144\n\t"
          "ds_read_b128 %3, %8 offset:7168\n\t"
          "ds_read_b128 %4, %9 offset:4096\n\t"
          "ds_read_b128 %5, %9 offset:5120\n\t"
          "ds_read_b128 %6, %9 offset:6144\n\t"
          "ds_read_b128 %7, %9 offset:7168\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(ql[4]), "=&v"(ql[5]), "=&v"(ql[6]), "=&v"(ql[7]),
            "=&v"(qh[4]), "=&v"(qh[5]), "=&v"(qh[6]), "=&v"(qh[7])
          : "v"(qlo), "v"(qhi));
      // all of pair p is in registers: free its buffers for pair p+2
      __builtin_amdgcn_s_barrier();
      if (2 * p + 4 < 2 * np) {
        stage_tile8(Q, D, row0, nq, (2 * p + 4) * BK_F8, QS4((2 * p + 4) & 3), BM);
        stage_tile8(Q, D, row0, nq, (2 * p + 5) * BK_F8, QS4((2 * p + 5) & 3), BM);
        stage_tile((const bf16*)X4, x4_ld, x0, (long long)nx, (p + 2) * 32,
                   XS4(p & 1), BN);
      }
      v8i_mx xv[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        int4 l = __builtin_bit_cast(int4, xf[n]);
        v8i_mx f;
        f[0] = l.x; f[1] = l.y; f[2] = l.z; f[3] = l.w;
        f[4] = 0; f[5] = 0; f[6] = 0; f[7] = 0;
        xv[n] = f;
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        v8i_mx qv = mx_frag(ql[m], qh[m]);
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              qv, xv[n], acc[m][n], 0 /*A fp8*/, 4 /*B fp4*/,
              0, unit_scale, 0, (int)sv[n]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[cbase] = acc[0][0][0];
      continue;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
          float v = acc[m][n][r];
          if (!(v > row_min[row])) continue;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          }
        }
  }
}

// ===========================================================================
// Full-MXFP4 threshold scan: BOTH operands e2m1 with per-lane-group
// e8m0 scales (cbsz=4, blgp=4). Per-pair staging drops to 4 per-lane
// glds (Q4 16 KB + X4 16 KB), Q fragment reads halve to one b128 per
// m-tile, and register pressure falls ~70 VGPRs vs the fp8-Q variant.
// The A-operand fp4 layout was probed identical to B
// (tools/probe_fp4map.hip): the same fragment permutation and scale
// grouping apply, so queries go through the same to_fp4_mx quantizer.
// Scores carry NO static prescale (the e8m0 block scales hold the
// magnitudes): theta is used at x1.
// ===========================================================================

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                     const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                     int nq, int nx, int D, int k, int n_swaths,
                     float* __restrict__ cand_scores,
                     int32_t* __restrict__ cand_ids,
                     const float* __restrict__ theta,
                     int32_t* __restrict__ tc_n, int cap) {
  // 4 pair-bufs x 16 KB each side: staging runs THREE pairs ahead
  // (stage target (p+3)%4 is disjoint from pairs p..p+2). Scale sheets
  // shrink to 32 B/row, capping this kernel at D = 1024 (the binding
  // routes larger D to the fp8xfp4 kernel).
  __shared__ bf16 lds_q[4 * BM * BK];
  __shared__ bf16 lds_x[4 * BN * BK];
  __shared__ uint8_t lds_qs[BM * 32];
  __shared__ uint8_t lds_xs2[BN * 32];
  __shared__ float row_min[BM];
#define QP4(buf) (lds_q + (buf) * BM * BK)
#define XP4(buf) (lds_x + (buf) * BN * BK)

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x)
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
  __syncthreads();

  int wid = wave_id();
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int np = D / (2 * BK_F8);
  int sb = D / 32;
  size_t cbase = (((size_t)qb * S) + swath) * (size_t)BM * k;
  long long p4_ld = D / 4;  // packed row length in bf16 units

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    stage_scale_rows(QS, sb, row0, (long long)nq, lds_qs, BM);
    stage_scale_rows(XS, sb, x0, (long long)nx, lds_xs2, BN);
    for (int pp = 0; pp < 3 && pp < np; ++pp) {
      stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, pp * 32, QP4(pp), BM);
      stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, pp * 32, XP4(pp), BN);
    }
    for (int p = 0; p < np; ++p) {
      // pairs p+1, p+2 may still be in flight (4 glds each)
      if (p + 2 < np)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (p + 1 < np)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // stage three pairs ahead: target (p+3)%4 touches only the buffer
      // consumed at pair p-1, so the single barrier suffices
      if (2 * p + 6 < 2 * np) {
        stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, (p + 3) * 32,
                   QP4((p + 3) & 3), BM);
        stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, (p + 3) * 32,
                   XP4((p + 3) & 3), BN);
      }
      uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
      uint32_t qrow_base = (uint32_t)(wm * 128 + lrow);
      uint32_t xaddr = (uint32_t)(size_t)XP4(p & 3)
                       + lds_off_bytes(xrow_base, (uint32_t)kgrp);
      uint32_t qaddr = (uint32_t)(size_t)QP4(p & 3)
                       + lds_off_bytes(qrow_base, (uint32_t)kgrp);
      uint32_t sst = 16u * (uint32_t)sb;
      uint32_t xs_a = (uint32_t)(size_t)lds_xs2 + xrow_base * (uint32_t)sb
                      + (uint32_t)(p * 4 + kgrp);
      uint32_t qs_a = (uint32_t)(size_t)lds_qs + qrow_base * (uint32_t)sb
                      + (uint32_t)(p * 4 + kgrp);
      bf16x8 xf[4], qf[8];
      uint32_t xs_v[4], qs_v[8];
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:1024\n\t"
          "ds_read_b128 %2, %8 offset:2048\n\t"
          "ds_read_b128 %3, %8 offset:3072\n\t"
          "ds_read_u8 %4, %9\n\t"
          "ds_read_u8 %5, %10\n\t"
          "ds_read_u8 %6, %11\n\t"
          "ds_read_u8 %7, %12\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
            "=&v"(xs_v[0]), "=&v"(xs_v[1]), "=&v"(xs_v[2]), "=&v"(xs_v[3])
          : "v"(xaddr), "v"(xs_a), "v"(xs_a + sst), "v"(xs_a + 2 * sst),
            "v"(xs_a + 3 * sst));
      asm volatile(
          "ds_read_b128 %0, %16\n\t"
          "ds_read_b128 %1, %16 offset:1024\n\t"
          "ds_read_b128 %2, %16 offset:2048\n\t"
          "ds_read_b128 %3, %16 offset:3072\n\t"
          "ds_read_b128 %4, %16 offset:4096\n\t"
          "ds_read_b128 %5, %16 offset:5120\n\t"
          "ds_read_b128 %6, %16 offset:6144\n\t"
          "ds_read_b128 %7, %16 offset:7168\n\t"
          "ds_read_u8 %8, %17\n\t"
          "ds_read_u8 %9, %18\n\t"
          "ds_read_u8 %10, %19\n\t"
          "ds_read_u8 %11, %20\n\t"
          "ds_read_u8 %12, %21\n\t"
          "ds_read_u8 %13, %22\n\t"
          "ds_read_u8 %14, %23\n\t"
          "ds_read_u8 %15, %24\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(qf[0]), "=&v"(qf[1]), "=&v"(qf[2]), "=&v"(qf[3]),
            "=&v"(qf[4]), "=&v"(qf[5]), "=&v"(qf[6]), "=&v"(qf[7]),
            "=&v"(qs_v[0]), "=&v"(qs_v[1]), "=&v"(qs_v[2]), "=&v"(qs_v[3]),
            "=&v"(qs_v[4]), "=&v"(qs_v[5]), "=&v"(qs_v[6]), "=&v"(qs_v[7])
          : "v"(qaddr), "v"(qs_a), "v"(qs_a + sst), "v"(qs_a + 2 * sst),
            "v"(qs_a + 3 * sst), "v"(qs_a + 4 * sst), "v"(qs_a + 5 * sst),
            "v"(qs_a + 6 * sst), "v"(qs_a + 7 * sst));
      v8i_mx xv[4], qv[8];
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        int4 l = __builtin_bit_cast(int4, xf[n]);
        v8i_mx f; f[0] = l.x; f[1] = l.y; f[2] = l.z; f[3] = l.w;
        f[4] = 0; f[5] = 0; f[6] = 0; f[7] = 0;
        xv[n] = f;
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        int4 l = __builtin_bit_cast(int4, qf[m]);
        v8i_mx f; f[0] = l.x; f[1] = l.y; f[2] = l.z; f[3] = l.w;
        f[4] = 0; f[5] = 0; f[6] = 0; f[7] = 0;
        qv[m] = f;
      }
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
              qv[m], xv[n], acc[m][n], 4 /*A fp4*/, 4 /*B fp4*/,
              0, (int)qs_v[m], 0, (int)xs_v[n]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[cbase] = acc[0][0][0];
      continue;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
          float v = acc[m][n][r];
          if (!(v > row_min[row])) continue;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          }
        }
  }
}


// ===========================================================================
// fp4x4 threshold scan v2: software-pipelined fragment reads. v1 reads
// all 24 LDS fragments, drains lgkmcnt(0) twice, then bursts 32 MFMAs —
// with only 2 waves/SIMD the drain serializes LDS latency against the
// MFMA pipe (measured 2.15 PF/s vs the instruction's 8.9 PF/s ceiling,
// tools/probe_mfma_rate). v2 issues the X fragments + the first two Q
// fragments, then per m-group overlaps the NEXT Q-fragment read with
// the current 4-MFMA burst, waiting lgkmcnt(2) instead of 0; ordering
// is pinned by "+v" passthroughs of the registers each wait guarantees.
// Zero-padding of the unused high halves of the fp4 operands is dropped
// (cbsz/blgp=4 consume 4 dwords; the probe's decode map covers only
// those) — that removes ~96 v_mov per pair from the hot loop.
// ===========================================================================

// Transposed, 40 B-padded scale staging for the v2 scan: LDS byte
// [row*40 + kgrp*8 + p] = global scale byte [row][4p + kgrp]. The
// per-pair consumers then read ONE conflict-free ds_read_b64 per
// fragment per x-tile (16 lanes x 40 B stride covers 16 distinct even
// bank residues) instead of 12 bank-conflicted ds_read_u8 per pair —
// PMC showed 6.0e9 LDS conflict cycles (~5 replays/read) on the u8 path.
#define SCALE_PITCH 40
DEVINL void stage_scale_rows_t(const uint8_t* __restrict__ src, int sb,
                               long long row0, long long row_max,
                               uint8_t* lds_base, int tile_rows) {
  int nd = sb >> 2;  // dwords per row actually present (np)
  for (int task = threadIdx.x; task < tile_rows * 4; task += TK_THREADS) {
    int row = task >> 2, kg = task & 3;
    long long gr = row0 + row;
    if (gr >= row_max) gr = row_max - 1;
    const uint8_t* rp = src + gr * (long long)sb;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < nd)
        lo |= (uint32_t)rp[q * 4 + kg] << (8 * q);
      if (q + 4 < nd)
        hi |= (uint32_t)rp[(q + 4) * 4 + kg] << (8 * q);
    }
    uint8_t* dst = lds_base + row * SCALE_PITCH + kg * 8;
    *(uint32_t*)dst = lo;
    *(uint32_t*)(dst + 4) = hi;
  }
}

DEVINL uint32_t scale_byte(uint32_t lo, uint32_t hi, int p) {
  uint32_t d = (p & 4) ? hi : lo;
  return (d >> (8 * (p & 3))) & 0xffu;
}

DEVINL v8i_mx fp4_frag(bf16x8 raw) {
  int4 l = __builtin_bit_cast(int4, raw);
  v8i_mx f;
  f[0] = l.x; f[1] = l.y; f[2] = l.z; f[3] = l.w;
  // f[4..7] intentionally uninitialized: fp4 operands (cbsz/blgp=4)
  // consume only the low 4 dwords of the 8-dword tuple
  return f;
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_v2_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                        const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                        int nq, int nx, int D, int k, int n_swaths,
                        float* __restrict__ cand_scores,
                        int32_t* __restrict__ cand_ids,
                        const float* __restrict__ theta,
                        int32_t* __restrict__ tc_n, int cap) {
  __shared__ bf16 lds_q[4 * BM * BK];
  __shared__ bf16 lds_x[4 * BN * BK];
  __shared__ uint8_t lds_qs[BM * SCALE_PITCH];
  __shared__ uint8_t lds_xs2[BN * SCALE_PITCH];
  __shared__ float row_min[BM];

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x)
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
  __syncthreads();

  int wid = wave_id();
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int np = D / (2 * BK_F8);
  int sb = D / 32;
  long long p4_ld = D / 4;

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    stage_scale_rows_t(QS, sb, row0, (long long)nq, lds_qs, BM);
    stage_scale_rows_t(XS, sb, x0, (long long)nx, lds_xs2, BN);
    __syncthreads();  // transposed ds_writes visible before any read
    // per-x-tile scale registers: one b64 per fragment, conflict-free
    uint32_t xs_lo[4], xs_hi[4], qs_lo[8], qs_hi[8];
    {
      uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
      uint32_t qrow_base = (uint32_t)(wm * 128 + lrow);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const uint8_t* a = lds_xs2 + (xrow_base + 16u * n) * SCALE_PITCH + kgrp * 8;
        xs_lo[n] = *(const uint32_t*)a;
        xs_hi[n] = *(const uint32_t*)(a + 4);
      }
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const uint8_t* a = lds_qs + (qrow_base + 16u * m) * SCALE_PITCH + kgrp * 8;
        qs_lo[m] = *(const uint32_t*)a;
        qs_hi[m] = *(const uint32_t*)(a + 4);
      }
    }
    for (int pp = 0; pp < 3 && pp < np; ++pp) {
      stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, pp * 32, QP4(pp), BM);
      stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, pp * 32, XP4(pp), BN);
    }
    for (int p = 0; p < np; ++p) {
      if (p + 2 < np)
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (p + 1 < np)
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (2 * p + 6 < 2 * np) {
        stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, (p + 3) * 32,
                   QP4((p + 3) & 3), BM);
        stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, (p + 3) * 32,
                   XP4((p + 3) & 3), BN);
      }
      uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
      uint32_t qrow_base = (uint32_t)(wm * 128 + lrow);
      uint32_t xaddr = (uint32_t)(size_t)XP4(p & 3)
                       + lds_off_bytes(xrow_base, (uint32_t)kgrp);
      uint32_t qaddr = (uint32_t)(size_t)QP4(p & 3)
                       + lds_off_bytes(qrow_base, (uint32_t)kgrp);
      bf16x8 xf[4], qf[8];
      // per-pair scale bytes extracted from the hoisted b64 registers
      uint32_t xsb[4], qsb[8];
#pragma unroll
      for (int n = 0; n < 4; ++n) xsb[n] = scale_byte(xs_lo[n], xs_hi[n], p);
#pragma unroll
      for (int m = 0; m < 8; ++m) qsb[m] = scale_byte(qs_lo[m], qs_hi[m], p);
      // prologue: X fragments + Q fragments 0,1; lgkmcnt(1) leaves
      // exactly qf1 in flight
      asm volatile(
          "ds_read_b128 %0, %6\n\t"
          "ds_read_b128 %1, %6 offset:1024\n\t"
          "ds_read_b128 %2, %6 offset:2048\n\t"
          "ds_read_b128 %3, %6 offset:3072\n\t"
          "ds_read_b128 %4, %7\n\t"
          "ds_read_b128 %5, %7 offset:1024\n\t"
          "s_waitcnt lgkmcnt(1)"
          : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
            "=&v"(qf[0]), "=&v"(qf[1])
          : "v"(xaddr), "v"(qaddr));
      v8i_mx xv[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) xv[n] = fp4_frag(xf[n]);

#define FP4V2_MFMA_GROUP(mm)                                                  \
  {                                                                           \
    v8i_mx qv = fp4_frag(qf[mm]);                                             \
    _Pragma("unroll") for (int n = 0; n < 4; ++n)                             \
        acc[mm][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(        \
            qv, xv[n], acc[mm][n], 4, 4, 0, (int)qsb[mm], 0, (int)xsb[n]);    \
  }
// issue fragment mm+2 while group mm computes; the lgkmcnt(1) then
// guarantees fragment mm+1, whose registers pass through to pin order
#define FP4V2_READ_NEXT(mm)                                                   \
  asm volatile(                                                               \
      "ds_read_b128 %0, %2\n\t"                                               \
      "s_waitcnt lgkmcnt(1)"                                                  \
      : "=&v"(qf[(mm) + 2]), "+v"(qf[(mm) + 1])                               \
      : "v"(qaddr + ((mm) + 2) * 1024u));

      FP4V2_MFMA_GROUP(0)
      FP4V2_READ_NEXT(0)
      FP4V2_MFMA_GROUP(1)
      FP4V2_READ_NEXT(1)
      FP4V2_MFMA_GROUP(2)
      FP4V2_READ_NEXT(2)
      FP4V2_MFMA_GROUP(3)
      FP4V2_READ_NEXT(3)
      FP4V2_MFMA_GROUP(4)
      FP4V2_READ_NEXT(4)
      FP4V2_MFMA_GROUP(5)
      FP4V2_READ_NEXT(5)
      FP4V2_MFMA_GROUP(6)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(qf[7]));
      FP4V2_MFMA_GROUP(7)
#undef FP4V2_MFMA_GROUP
#undef FP4V2_READ_NEXT
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[0] = acc[0][0][0];
      continue;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
          float v = acc[m][n][r];
          if (!(v > row_min[row])) continue;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          }
        }
  }
}

// ===========================================================================
// fp4x4 threshold scan v3: 2-pair barrier intervals. v1 pays one full
// s_barrier + vmcnt gate per K-pair (np=8 at D=1024); the measured gap
// to the MFMA floor is per-pair overhead amortized over a 32-MFMA burst
// (NOTES-NEXT). v3 keeps v1's fragment reads and MFMA body but consumes
// TWO consecutive pairs per barrier interval: one vmcnt wait + one
// barrier per 64 MFMAs. Buffer discipline: interval p consumes buffers
// p&3,(p+1)&3 and stages pairs p+2,p+3 into (p+2)&3,(p+3)&3 — disjoint,
// and the interval-entry barrier keeps the previous interval's readers
// ahead of this interval's overwrites (same invariant as v1, half the
// barriers). No extra VGPR: fragments for the two pairs are read
// sequentially, not held concurrently.
// ===========================================================================

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_v3_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                        const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                        int nq, int nx, int D, int k, int n_swaths,
                        float* __restrict__ cand_scores,
                        int32_t* __restrict__ cand_ids,
                        const float* __restrict__ theta,
                        int32_t* __restrict__ tc_n, int cap) {
  __shared__ bf16 lds_q[4 * BM * BK];
  __shared__ bf16 lds_x[4 * BN * BK];
  __shared__ uint8_t lds_qs[BM * 32];
  __shared__ uint8_t lds_xs2[BN * 32];
  __shared__ float row_min[BM];
#define QP4A(buf) (lds_q + (buf) * BM * BK)
#define XP4A(buf) (lds_x + (buf) * BN * BK)

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x)
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
  __syncthreads();

  int wid = wave_id();
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int np = D / (2 * BK_F8);
  int sb = D / 32;
  size_t cbase = (((size_t)qb * S) + swath) * (size_t)BM * k;
  long long p4_ld = D / 4;

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    stage_scale_rows(QS, sb, row0, (long long)nq, lds_qs, BM);
    stage_scale_rows(XS, sb, x0, (long long)nx, lds_xs2, BN);
    // prologue: stage the first interval's two pairs
    for (int pp = 0; pp < 2 && pp < np; ++pp) {
      stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, pp * 32, QP4A(pp), BM);
      stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, pp * 32, XP4A(pp), BN);
    }
    for (int p = 0; p < np; p += 2) {
      int pe = min(p + 2, np);
      // all outstanding glds are exactly this interval's pairs
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // stage the NEXT interval (pairs p+2, p+3) into the buffers the
      // PREVIOUS interval consumed; overlaps this interval's compute
      for (int s = p + 2; s < min(np, p + 4); ++s) {
        stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, s * 32,
                   QP4A(s & 3), BM);
        stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, s * 32,
                   XP4A(s & 3), BN);
      }
      for (int pc = p; pc < pe; ++pc) {
        uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
        uint32_t qrow_base = (uint32_t)(wm * 128 + lrow);
        uint32_t xaddr = (uint32_t)(size_t)XP4A(pc & 3)
                         + lds_off_bytes(xrow_base, (uint32_t)kgrp);
        uint32_t qaddr = (uint32_t)(size_t)QP4A(pc & 3)
                         + lds_off_bytes(qrow_base, (uint32_t)kgrp);
        uint32_t sst = 16u * (uint32_t)sb;
        uint32_t xs_a = (uint32_t)(size_t)lds_xs2 + xrow_base * (uint32_t)sb
                        + (uint32_t)(pc * 4 + kgrp);
        uint32_t qs_a = (uint32_t)(size_t)lds_qs + qrow_base * (uint32_t)sb
                        + (uint32_t)(pc * 4 + kgrp);
        bf16x8 xf[4], qf[8];
        uint32_t xs_v[4], qs_v[8];
        asm volatile(
            "ds_read_b128 %0, %8\n\t"
            "ds_read_b128 %1, %8 offset:1024\n\t"
            "ds_read_b128 %2, %8 offset:2048\n\t"
            "ds_read_b128 %3, %8 offset:3072\n\t"
            "ds_read_u8 %4, %9\n\t"
            "ds_read_u8 %5, %10\n\t"
            "ds_read_u8 %6, %11\n\t"
            "ds_read_u8 %7, %12\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
              "=&v"(xs_v[0]), "=&v"(xs_v[1]), "=&v"(xs_v[2]), "=&v"(xs_v[3])
            : "v"(xaddr), "v"(xs_a), "v"(xs_a + sst), "v"(xs_a + 2 * sst),
              "v"(xs_a + 3 * sst));
        asm volatile(
            "ds_read_b128 %0, %16\n\t"
            "ds_read_b128 %1, %16 offset:1024\n\t"
            "ds_read_b128 %2, %16 offset:2048\n\t"
            "ds_read_b128 %3, %16 offset:3072\n\t"
            "ds_read_b128 %4, %16 offset:4096\n\t"
            "ds_read_b128 %5, %16 offset:5120\n\t"
            "ds_read_b128 %6, %16 offset:6144\n\t"
            "ds_read_b128 %7, %16 offset:7168\n\t"
            "ds_read_u8 %8, %17\n\t"
            "ds_read_u8 %9, %18\n\t"
            "ds_read_u8 %10, %19\n\t"
            "ds_read_u8 %11, %20\n\t"
            "ds_read_u8 %12, %21\n\t"
            "ds_read_u8 %13, %22\n\t"
            "ds_read_u8 %14, %23\n\t"
            "ds_read_u8 %15, %24\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(qf[0]), "=&v"(qf[1]), "=&v"(qf[2]), "=&v"(qf[3]),
              "=&v"(qf[4]), "=&v"(qf[5]), "=&v"(qf[6]), "=&v"(qf[7]),
              "=&v"(qs_v[0]), "=&v"(qs_v[1]), "=&v"(qs_v[2]), "=&v"(qs_v[3]),
              "=&v"(qs_v[4]), "=&v"(qs_v[5]), "=&v"(qs_v[6]), "=&v"(qs_v[7])
            : "v"(qaddr), "v"(qs_a), "v"(qs_a + sst), "v"(qs_a + 2 * sst),
              "v"(qs_a + 3 * sst), "v"(qs_a + 4 * sst), "v"(qs_a + 5 * sst),
              "v"(qs_a + 6 * sst), "v"(qs_a + 7 * sst));
        v8i_mx xv[4], qv[8];
#pragma unroll
        for (int n = 0; n < 4; ++n) xv[n] = fp4_frag(xf[n]);
#pragma unroll
        for (int m = 0; m < 8; ++m) qv[m] = fp4_frag(qf[m]);
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                qv[m], xv[n], acc[m][n], 4 /*A fp4*/, 4 /*B fp4*/,
                0, (int)qs_v[m], 0, (int)xs_v[n]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[cbase] = acc[0][0][0];
      continue;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
          float v = acc[m][n][r];
          if (!(v > row_min[row])) continue;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          }
        }
  }
}


// ===========================================================================
// fp4x4 threshold scan v7: v3's tile geometry, LDS image, 2-pair
// intervals, fragment reads and MFMA body, with the per-tile work around
// the K-loop cut down:
//  - any-hit fast path: the lane's 32 thresholds come in as 8
//    ds_read_b128 (rows wm*128 + m*16 + (lane>>4)*4 + r are contiguous in
//    r), max over n per (m, r), one wave-uniform branch on the ballot. A
//    wave with no score above its thresholds (>90 % of wave-tiles at
//    production theta) skips the 128-element compare/append loop. The
//    loop itself is v3's, so the hit condition stays exactly v > theta and
//    clamped rows/columns of ragged tiles are still filtered there.
//  - hoisted staging addresses: a lane stages the same two rows of every
//    pair, so its two byte offsets (clamped row * ld + swizzled slot) are
//    computed once per block for Q and once per tile for X; each glds is
//    then wave-uniform 64-bit base (row0*ld + pair*64) + 32-bit lane
//    offset. Offsets span at most 256 rows * 512 B; the base carries the
//    index size.
//  - the Q scale sheet is identical for the whole block: staged once in
//    the block prologue instead of once per tile. The first tile's
//    interval-0 vmcnt(0) + barrier orders it before its first reader.
// The per-row candidate-pointer arithmetic (grow * cap, 64-bit) lives in
// the slow path only; with it out of the block-lifetime registers the
// kernel holds no scratch at all (v3: 41 VGPR + 20 SGPR spills).
// Tile boundary: as in v3 the trailing barrier orders every wave's last
// fragment/scale reads (each asm read block ends in lgkmcnt(0)) before
// the next tile's head restages pair buffers 0,1 and the X scale sheet —
// for np <= 2 those are the very buffers the last interval read. Issuing
// that head BEFORE the epilogue (so it flies under it) was measured and
// taken out: with the fast path the epilogue is too short to hide
// anything and the scan got 3 % slower (profiles/README.md).
// ===========================================================================

// byte offsets of the two 16 B pieces a lane stages per pair tile
// ([256 rows][4 slots], piece = w*64 + i*512 + lane), rows clamped to
// the tile's live rows (garbage rows are filtered in the epilogue)
DEVINL void stage_row_offsets(uint32_t w, uint32_t lane, uint32_t rows_live,
                              uint32_t ld_bytes, uint32_t off[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    uint32_t piece = w * WAVE + i * TK_THREADS + lane;
    uint32_t r = piece >> 2;
    uint32_t slot = piece & 3;
    uint32_t src_slot = slot ^ ((r >> 2u) & 3u);
    if (r >= rows_live) r = rows_live - 1;
    off[i] = r * ld_bytes + src_slot * 16u;
  }
}

// the same offsets with the source slot picked by swz_slot<SWZ>, the
// staging side of lds_off_bytes_swz<SWZ>. A lane's four-lane set still
// reads one whole 64 B row segment: coalescing does not depend on SWZ.
template <int SWZ>
DEVINL void stage_row_offsets_swz(uint32_t w, uint32_t lane, uint32_t rows_live,
                                  uint32_t ld_bytes, uint32_t off[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    uint32_t piece = w * WAVE + i * TK_THREADS + lane;
    uint32_t r = piece >> 2;
    uint32_t src_slot = swz_slot<SWZ>(r, piece & 3);
    if (r >= rows_live) r = rows_live - 1;
    off[i] = r * ld_bytes + src_slot * 16u;
  }
}

// stage one pair tile: base is wave-uniform (tile row0 * ld + pair * 64)
DEVINL void stage_tile_off(const uint8_t* __restrict__ base,
                           const uint32_t off[2], bf16* lds_base, uint32_t w) {
  auto ldst = (AS3 char*)lds_base + w * (WAVE * 16);
  __builtin_amdgcn_global_load_lds((const AS1 void*)(base + off[0]),
                                   (AS3 void*)ldst, 16, 0, 0);
  __builtin_amdgcn_global_load_lds((const AS1 void*)(base + off[1]),
                                   (AS3 void*)(ldst + TK_THREADS * 16), 16, 0, 0);
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_v7_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                        const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                        int nq, int nx, int D, int k, int n_swaths,
                        float* __restrict__ cand_scores,
                        int32_t* __restrict__ cand_ids,
                        const float* __restrict__ theta,
                        int32_t* __restrict__ tc_n, int cap) {
  __shared__ bf16 lds_q[4 * BM * BK];
  __shared__ bf16 lds_x[4 * BN * BK];
  __shared__ uint8_t lds_qs[BM * 32];
  __shared__ uint8_t lds_xs2[BN * 32];
  __shared__ __attribute__((aligned(16))) float row_min[BM];
#define QP4E(buf) (lds_q + (buf) * BM * BK)
#define XP4E(buf) (lds_x + (buf) * BN * BK)

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);
  if (x_begin >= x_end) return;

  for (int i = threadIdx.x; i < BM; i += blockDim.x)
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
  __syncthreads();

  int wid = wave_id();
  uint32_t wu = (uint32_t)__builtin_amdgcn_readfirstlane(wid);
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int np = D / (2 * BK_F8);
  int sb = D / 32;
  uint32_t ldb = (uint32_t)(D / 2);  // row pitch in bytes

  uint32_t qoff[2], xoff[2];
  const uint8_t* qbase = Q4 + row0 * (long long)ldb;
  stage_row_offsets(wu, (uint32_t)lane, (uint32_t)min((long long)BM, nq - row0),
                    ldb, qoff);

  // stage pair s of the Q block and of x tile xt into buffer s & 3
  auto stage_pair = [&](long long xt, int s) {
    stage_tile_off(qbase + s * 64, qoff, QP4E(s & 3), wu);
    stage_tile_off(X4 + xt * (long long)ldb + s * 64, xoff, XP4E(s & 3), wu);
  };
  // x tile xt's scale sheet + first interval
  auto stage_head = [&](long long xt) {
    stage_row_offsets(wu, (uint32_t)lane, (uint32_t)min((long long)BN, nx - xt),
                      ldb, xoff);
    stage_scale_rows(XS, sb, xt, (long long)nx, lds_xs2, BN);
    stage_pair(xt, 0);
    if (np > 1) stage_pair(xt, 1);
  };

  stage_scale_rows(QS, sb, row0, (long long)nq, lds_qs, BM);

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    stage_head(x0);
    for (int p = 0; p < np; p += 2) {
      int pe = min(p + 2, np);
      // all outstanding glds are exactly this interval's pairs (plus,
      // at p == 0, the tile's X scale sheet and once the Q scale sheet)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // stage the NEXT interval (pairs p+2, p+3) into the buffers the
      // PREVIOUS interval consumed; overlaps this interval's compute
      if (p + 2 < np) stage_pair(x0, p + 2);
      if (p + 3 < np) stage_pair(x0, p + 3);
      for (int pc = p; pc < pe; ++pc) {
        uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
        uint32_t qrow_base = (uint32_t)(wm * 128 + lrow);
        uint32_t xaddr = (uint32_t)(size_t)XP4E(pc & 3)
                         + lds_off_bytes(xrow_base, (uint32_t)kgrp);
        uint32_t qaddr = (uint32_t)(size_t)QP4E(pc & 3)
                         + lds_off_bytes(qrow_base, (uint32_t)kgrp);
        uint32_t sst = 16u * (uint32_t)sb;
        uint32_t xs_a = (uint32_t)(size_t)lds_xs2 + xrow_base * (uint32_t)sb
                        + (uint32_t)(pc * 4 + kgrp);
        uint32_t qs_a = (uint32_t)(size_t)lds_qs + qrow_base * (uint32_t)sb
                        + (uint32_t)(pc * 4 + kgrp);
        bf16x8 xf[4], qf[8];
        uint32_t xs_v[4], qs_v[8];
        asm volatile(
            "ds_read_b128 %0, %8\n\t"
            "ds_read_b128 %1, %8 offset:1024\n\t"
            "ds_read_b128 %2, %8 offset:2048\n\t"
            "ds_read_b128 %3, %8 offset:3072\n\t"
            "ds_read_u8 %4, %9\n\t"
            "ds_read_u8 %5, %10\n\t"
            "ds_read_u8 %6, %11\n\t"
            "ds_read_u8 %7, %12\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
              "=&v"(xs_v[0]), "=&v"(xs_v[1]), "=&v"(xs_v[2]), "=&v"(xs_v[3])
            : "v"(xaddr), "v"(xs_a), "v"(xs_a + sst), "v"(xs_a + 2 * sst),
              "v"(xs_a + 3 * sst));
        asm volatile(
            "ds_read_b128 %0, %16\n\t"
            "ds_read_b128 %1, %16 offset:1024\n\t"
            "ds_read_b128 %2, %16 offset:2048\n\t"
            "ds_read_b128 %3, %16 offset:3072\n\t"
            "ds_read_b128 %4, %16 offset:4096\n\t"
            "ds_read_b128 %5, %16 offset:5120\n\t"
            "ds_read_b128 %6, %16 offset:6144\n\t"
            "ds_read_b128 %7, %16 offset:7168\n\t"
            "ds_read_u8 %8, %17\n\t"
            "ds_read_u8 %9, %18\n\t"
            "ds_read_u8 %10, %19\n\t"
            "ds_read_u8 %11, %20\n\t"
            "ds_read_u8 %12, %21\n\t"
            "ds_read_u8 %13, %22\n\t"
            "ds_read_u8 %14, %23\n\t"
            "ds_read_u8 %15, %24\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(qf[0]), "=&v"(qf[1]), "=&v"(qf[2]), "=&v"(qf[3]),
              "=&v"(qf[4]), "=&v"(qf[5]), "=&v"(qf[6]), "=&v"(qf[7]),
              "=&v"(qs_v[0]), "=&v"(qs_v[1]), "=&v"(qs_v[2]), "=&v"(qs_v[3]),
              "=&v"(qs_v[4]), "=&v"(qs_v[5]), "=&v"(qs_v[6]), "=&v"(qs_v[7])
            : "v"(qaddr), "v"(qs_a), "v"(qs_a + sst), "v"(qs_a + 2 * sst),
              "v"(qs_a + 3 * sst), "v"(qs_a + 4 * sst), "v"(qs_a + 5 * sst),
              "v"(qs_a + 6 * sst), "v"(qs_a + 7 * sst));
        v8i_mx xv[4], qv[8];
#pragma unroll
        for (int n = 0; n < 4; ++n) xv[n] = fp4_frag(xf[n]);
#pragma unroll
        for (int m = 0; m < 8; ++m) qv[m] = fp4_frag(qf[m]);
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                qv[m], xv[n], acc[m][n], 4 /*A fp4*/, 4 /*B fp4*/,
                0, (int)qs_v[m], 0, (int)xs_v[n]);
      }
    }
    // nothing is in flight here (the last interval staged nothing); the
    // barrier orders every wave's last fragment reads before the next
    // tile's head overwrites buffers 0,1 and the X scale sheet
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // the lane's 32 thresholds, th[m][r] = row_min[wm*128 + m*16 +
    // (lane>>4)*4 + r]
    f32x4 th[8];
    {
      uint32_t ta = (uint32_t)(size_t)row_min
                    + (uint32_t)(wm * 128 + (lane >> 4) * 4) * 4u;
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:64\n\t"
          "ds_read_b128 %2, %8 offset:128\n\t"
          "ds_read_b128 %3, %8 offset:192\n\t"
          "ds_read_b128 %4, %8 offset:256\n\t"
          "ds_read_b128 %5, %8 offset:320\n\t"
          "ds_read_b128 %6, %8 offset:384\n\t"
          "ds_read_b128 %7, %8 offset:448\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(th[0]), "=&v"(th[1]), "=&v"(th[2]), "=&v"(th[3]),
            "=&v"(th[4]), "=&v"(th[5]), "=&v"(th[6]), "=&v"(th[7])
          : "v"(ta));
    }
    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[0] = acc[0][0][0];
      continue;
    }
    // any-hit test: fmax drops a NaN score exactly as v > theta does
    bool hit = false;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = __builtin_fmaxf(
            __builtin_fmaxf(acc[m][0][r], acc[m][1][r]),
            __builtin_fmaxf(acc[m][2][r], acc[m][3][r]));
        hit |= mx > th[m][r];
      }
    if (__builtin_amdgcn_ballot_w64(hit) == 0) continue;
    // slow path. lq is laundered per tile so the 32 per-row candidate
    // pointers (grow * cap, 64-bit) are formed here, on the rare hit,
    // not hoisted into block-lifetime registers and scratch
    int lq = lane >> 4;
    asm volatile("" : "+v"(lq));
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[m][n][r];
          if (!(v > th[m][r])) continue;
          int row = wm * 128 + m * 16 + lq * 4 + r;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          }
        }
  }
}

// ===========================================================================
// fp4x4 threshold scan v9: v7 with the per-pair scale-byte reads gone.
// v7 fetches a lane's 12 block scales of every pair with 12 ds_read_u8 from
// row-major byte sheets; rows r, r+4, r+8, r+12 of a fragment share a bank
// there (4-way). v9 keeps both sheets transposed in LDS, one dword per
// (row, 4-pair group, kgrp) whose byte (pc & 3) is the scale of pair pc,
// reads the lane's 12 dwords once per four pairs and lets the MFMA pick
// the byte: op_sel = pc & 3 on both scale operands, a compile-time
// constant because the pair loop is unrolled in groups of four. No VALU
// touches a scale byte.
//  - sheet layout: dword index row*10 + grp*4 + kgrp (grp = pc >> 2), row
//    pitch 40 B. ds_read_b32 is served in 32-lane groups with bank =
//    dword index mod 32 (MI355X_MICROARCH.md, LDS table). A group is the
//    fragment's 16 rows x two kgrp values (kgrp, kgrp + 1); row*10 mod 32
//    over 16 consecutive rows is 0,10,20,30,8,18,28,6,16,26,4,14,24,2,12,
//    22 — the 16 even residues, each once — and the kgrp pair adds 0/1
//    (or 2/3), so the 32 lanes hit 32 distinct banks: conflict-free. The
//    fragment base row (multiple of 16) and grp*4 shift all lanes alike.
//  - staging: glds cannot transpose bytes, so a sheet goes through
//    registers. Thread t owns half row (row = t & 255, grp = t >> 8, so
//    grp is wave-uniform): one global_load_dwordx4 of the half row when
//    rows are whole 16 B pieces (np = 4, 8), else one dword load per
//    dword that exists (min(4, np - 4*grp), block-uniform branch), rows
//    past the array's end clamped as v7's staging clamps them, 8 v_perm_b32
//    for the 4x4 byte transpose, two ds_write_b64. Q sheet: once per block, ahead of the
//    prologue barrier. X sheet: single buffer, written at the tile head
//    from registers loaded one tile earlier (the first tile's in the
//    prologue); the load for the next tile is issued right behind the
//    write, ahead of the tile's first glds, as an ordinary load and is
//    landed by the interval-0 vmcnt(0) the kernel executes anyway
//    (writing behind the glds instead measured 1 % slower). The previous tile's trailing barrier has
//    retired every reader of the old sheet; the interval waits carry
//    lgkmcnt(0) so the writes are done before the interval-0 barrier.
//    No new barrier, no new vmcnt wait.
//    For np not 4 or 8 the per-dword loads make the compiler drain vmcnt
//    at the tile head; those depths are off the production path.
//  - pair buffers (pc & 3) and op_sel coincide, so fragment and scale
//    reads address off two block-lifetime VGPRs each with immediate
//    offsets.
//  - counted lgkmcnt per m: with the byte reads gone a pair's read queue
//    is 12 in-order ds_read_b128 (behind the 12 scale dwords on the first
//    pair of a group). The four MFMAs of fragment row m start at
//    lgkmcnt(7 - m) instead of all 32 behind lgkmcnt(0), so Q1-7 land
//    under the MFMAs of the rows before them (measured -4.2 % on its own,
//    profiles/README.md).
// Intervals, barriers, vmcnt(0) placement, pair buffers, fragment reads,
// MFMA order and the epilogue are v7's: every accumulator sees the same
// operations in the same order, results are bit-identical.
// ===========================================================================

#define SCALE9_PITCH 40

typedef uint32_t u32x2_s9 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_s9 __attribute__((ext_vector_type(4)));

// the nd (0..4, wave-uniform) dwords of the half scale row at array byte
// offset o; w[pl] holds the four kgrp bytes of pair 4*grp + pl, absent
// pairs read as 0. whole16: sb % 16 == 0, the half row is one 16 B piece.
// A load that would start past the array's end (a row past the last live
// one) is moved onto the array's last piece, as stage_scale_rows does; a
// live row's bytes always come from their own place.
DEVINL u32x4_s9 scale9_load(const uint8_t* __restrict__ src, long long o,
                            long long total, int nd, bool whole16) {
  u32x4_s9 w = {0u, 0u, 0u, 0u};
  if (whole16) {
    __builtin_memcpy(&w, src + min(o, total - 16), 16);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nd) {
        uint32_t t;
        __builtin_memcpy(&t, src + min(o + 4 * i, total - 4), 4);
        w[i] = t;
      }
  }
  return w;
}

// 4x4 byte transpose (out[kg] byte pl = w[pl] byte kg) and the two 8 B
// writes of one half row. v_perm_b32 selector bytes index {b (0..3), a
// (4..7)} of __builtin_amdgcn_perm(a, b, sel).
DEVINL void scale9_write(u32x4_s9 w, uint32_t lds_addr) {
  uint32_t t0 = __builtin_amdgcn_perm(w[1], w[0], 0x05010400u);
  uint32_t t1 = __builtin_amdgcn_perm(w[1], w[0], 0x07030602u);
  uint32_t t2 = __builtin_amdgcn_perm(w[3], w[2], 0x05010400u);
  uint32_t t3 = __builtin_amdgcn_perm(w[3], w[2], 0x07030602u);
  u32x2_s9 lo, hi;
  lo[0] = __builtin_amdgcn_perm(t2, t0, 0x05040100u);
  lo[1] = __builtin_amdgcn_perm(t2, t0, 0x07060302u);
  hi[0] = __builtin_amdgcn_perm(t3, t1, 0x05040100u);
  hi[1] = __builtin_amdgcn_perm(t3, t1, 0x07060302u);
  asm volatile(
      "ds_write_b64 %0, %1\n\t"
      "ds_write_b64 %0, %2 offset:8"
      :: "v"(lds_addr), "v"(lo), "v"(hi) : "memory");
}

// one pair: pair buffer SEL, op_sel SEL. SCALES: this is the first pair of
// its 4-pair group and the read blocks also fetch the group's 12 scale
// dwords (sheet addresses xs_a / qs_a already carry grp*16).
template <int N>
DEVINL void fp4v9_wait(bf16x8& q) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(q) : "n"(N));
}

template <int SEL, bool SCALES>
DEVINL void fp4v9_pair(f32x4 (&acc)[8][4], uint32_t xaddr, uint32_t qaddr,
                       uint32_t xs_a, uint32_t qs_a, uint32_t (&xs_v)[4],
                       uint32_t (&qs_v)[8]) {
  constexpr int B = SEL * BM * BK * 2;  // pair buffer SEL, bytes
  constexpr int SP = 16 * SCALE9_PITCH;  // sheet bytes per 16-row fragment
  bf16x8 xf[4], qf[8];
  if constexpr (SCALES) {
    asm volatile(
        "ds_read_b32 %4, %9\n\t"
        "ds_read_b32 %5, %9 offset:%14\n\t"
        "ds_read_b32 %6, %9 offset:%15\n\t"
        "ds_read_b32 %7, %9 offset:%16\n\t"
        "ds_read_b128 %0, %8 offset:%10\n\t"
        "ds_read_b128 %1, %8 offset:%11\n\t"
        "ds_read_b128 %2, %8 offset:%12\n\t"
        "ds_read_b128 %3, %8 offset:%13"
        : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3]),
          "=&v"(xs_v[0]), "=&v"(xs_v[1]), "=&v"(xs_v[2]), "=&v"(xs_v[3])
        : "v"(xaddr), "v"(xs_a),
          "n"(B), "n"(B + 1024), "n"(B + 2048), "n"(B + 3072),
          "n"(SP), "n"(2 * SP), "n"(3 * SP));
    asm volatile(
        "ds_read_b32 %8, %17\n\t"
        "ds_read_b32 %9, %17 offset:%26\n\t"
        "ds_read_b32 %10, %17 offset:%27\n\t"
        "ds_read_b32 %11, %17 offset:%28\n\t"
        "ds_read_b32 %12, %17 offset:%29\n\t"
        "ds_read_b32 %13, %17 offset:%30\n\t"
        "ds_read_b32 %14, %17 offset:%31\n\t"
        "ds_read_b32 %15, %17 offset:%32\n\t"
        "ds_read_b128 %0, %16 offset:%18\n\t"
        "ds_read_b128 %1, %16 offset:%19\n\t"
        "ds_read_b128 %2, %16 offset:%20\n\t"
        "ds_read_b128 %3, %16 offset:%21\n\t"
        "ds_read_b128 %4, %16 offset:%22\n\t"
        "ds_read_b128 %5, %16 offset:%23\n\t"
        "ds_read_b128 %6, %16 offset:%24\n\t"
        "ds_read_b128 %7, %16 offset:%25\n\t"
        "s_waitcnt lgkmcnt(7)"
        : "=&v"(qf[0]), "=&v"(qf[1]), "=&v"(qf[2]), "=&v"(qf[3]),
          "=&v"(qf[4]), "=&v"(qf[5]), "=&v"(qf[6]), "=&v"(qf[7]),
          "=&v"(qs_v[0]), "=&v"(qs_v[1]), "=&v"(qs_v[2]), "=&v"(qs_v[3]),
          "=&v"(qs_v[4]), "=&v"(qs_v[5]), "=&v"(qs_v[6]), "=&v"(qs_v[7])
        : "v"(qaddr), "v"(qs_a),
          "n"(B), "n"(B + 1024), "n"(B + 2048), "n"(B + 3072),
          "n"(B + 4096), "n"(B + 5120), "n"(B + 6144), "n"(B + 7168),
          "n"(SP), "n"(2 * SP), "n"(3 * SP), "n"(4 * SP), "n"(5 * SP),
          "n"(6 * SP), "n"(7 * SP));
  } else {
    asm volatile(
        "ds_read_b128 %0, %4 offset:%5\n\t"
        "ds_read_b128 %1, %4 offset:%6\n\t"
        "ds_read_b128 %2, %4 offset:%7\n\t"
        "ds_read_b128 %3, %4 offset:%8"
        : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3])
        : "v"(xaddr),
          "n"(B), "n"(B + 1024), "n"(B + 2048), "n"(B + 3072));
    asm volatile(
        "ds_read_b128 %0, %8 offset:%9\n\t"
        "ds_read_b128 %1, %8 offset:%10\n\t"
        "ds_read_b128 %2, %8 offset:%11\n\t"
        "ds_read_b128 %3, %8 offset:%12\n\t"
        "ds_read_b128 %4, %8 offset:%13\n\t"
        "ds_read_b128 %5, %8 offset:%14\n\t"
        "ds_read_b128 %6, %8 offset:%15\n\t"
        "ds_read_b128 %7, %8 offset:%16\n\t"
        "s_waitcnt lgkmcnt(7)"
        : "=&v"(qf[0]), "=&v"(qf[1]), "=&v"(qf[2]), "=&v"(qf[3]),
          "=&v"(qf[4]), "=&v"(qf[5]), "=&v"(qf[6]), "=&v"(qf[7])
        : "v"(qaddr),
          "n"(B), "n"(B + 1024), "n"(B + 2048), "n"(B + 3072),
          "n"(B + 4096), "n"(B + 5120), "n"(B + 6144), "n"(B + 7168));
  }
  v8i_mx xv[4], qv[8];
#pragma unroll
  for (int n = 0; n < 4; ++n) xv[n] = fp4_frag(xf[n]);
  // the read queue is in order (scale dwords, X0-3, Q0-7) and the Q block
  // left lgkmcnt(7): all but Q1-7 are in. Group m's MFMAs start once Q_m
  // is: the wait passes qf[m] through, and the scheduling barrier keeps it
  // behind group m-1's MFMAs. Group 7's wait is lgkmcnt(0), so a pair
  // still ends with every one of its LDS reads retired.
#define FP4V9_GROUP(m)                                                        \
  {                                                                           \
    if constexpr ((m) > 0) {                                                  \
      __builtin_amdgcn_sched_barrier(0);                                      \
      fp4v9_wait<7 - (m)>(qf[m]);                                             \
    }                                                                         \
    qv[m] = fp4_frag(qf[m]);                                                  \
    _Pragma("unroll") for (int n = 0; n < 4; ++n)                             \
      acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(           \
          qv[m], xv[n], acc[m][n], 4 /*A fp4*/, 4 /*B fp4*/,                  \
          SEL, (int)qs_v[m], SEL, (int)xs_v[n]);                              \
  }
  FP4V9_GROUP(0) FP4V9_GROUP(1) FP4V9_GROUP(2) FP4V9_GROUP(3)
  FP4V9_GROUP(4) FP4V9_GROUP(5) FP4V9_GROUP(6) FP4V9_GROUP(7)
#undef FP4V9_GROUP
}

// ---------------------------------------------------------------------------
// v10: v9 on the group-aware fragment swizzle. v9's image uses slot ^
// ((row>>2)&3), conflict-free on contiguous 16-lane groups; on the real
// ds_read_b128 groups every fragment read is 2-way conflicted (8 LDS cycles
// instead of 4; SQ_LDS_BANK_CONFLICT residue of 12 reads x 4 cycles per
// wave-pair). v10 takes the slot from frag_swz_slot (common.hpp, proven
// there by static_assert) on both sides: the staging source slot
// (stage_row_offsets_swz) and the read address (lds_off_bytes_swz). The XOR
// term still depends on the row through (row>>2)&3 only, so the
// block-lifetime read addresses with immediate offsets survive, the glds
// destination stays lane-linear, and every accumulator sees the same
// operands in the same order: bit-identical to v9 and v1.
//
// One body serves five kernels, which differ in nothing else:
//   topk_scan_fp4_v9_kernel     SWZ = 0, unfiltered
//   topk_scan_fp4_v10_kernel    SWZ = 1, unfiltered
//   topk_scan_fp4_owned_kernel  SWZ = 1, owner-filtered (prologue, row-owner
//                               loads and two-gate epilogue described at
//                               the kernel)
//   topk_scan_fp4_hist_kernel, topk_scan_fp4_owned_hist_kernel
//                               the two above with HIST: a hit that finds
//                               its query's buffer full is counted in a
//                               per-query score histogram (hist_bin below)
//                               instead of vanishing. HIST = false compiles
//                               to the instructions it compiled to before
//                               the parameter existed.
// ---------------------------------------------------------------------------

typedef int32_t i32x4_own __attribute__((ext_vector_type(4)));

// Histogram of the hits that found the candidate buffer full (HIST bodies):
// HIST_NB bins of width w above theta, per query. edge(j) = fp32(fp64(j) *
// fp64(w) + fp64(theta)); bin(v) is the b with edge(b) < v <= edge(b + 1),
// the last bin open above. The bin is estimated from (v - theta) * inv_w,
// clamped as a float (fmax drops a NaN, fmin an inf) ahead of the int
// conversion, then moved by at most one bin against the two edges. The rule
// is ops.gpu.hist_bin_spec, bit for bit; j * w is exact in fp64, so a
// contracted fma gives the same edge as the spec's multiply and add.
#define HIST_NB 256

DEVINL float hist_edge(int j, float w, float theta) {
  return (float)((double)j * (double)w + (double)theta);
}

DEVINL int hist_bin(float v, float theta, float w, float inv_w) {
  float t = (v - theta) * inv_w;
  t = __builtin_fminf(__builtin_fmaxf(t, 0.0f), (float)(HIST_NB - 1));
  int b = (int)t;
  if (b > 0 && !(v > hist_edge(b, w, theta))) b -= 1;
  else if (b < HIST_NB - 1 && v > hist_edge(b + 1, w, theta)) b += 1;
  return b;
}

template <int SWZ, bool OWNED, bool HIST>
DEVINL void fp4_scan_body(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                          const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                          int nq, int nx, int D, int k, int n_swaths,
                          float* __restrict__ cand_scores,
                          int32_t* __restrict__ cand_ids,
                          const float* __restrict__ theta,
                          int32_t* __restrict__ tc_n, int cap,
                          const int32_t* __restrict__ xowner,
                          const int32_t* __restrict__ qowner,
                          // HIST only: hist[nq][HIST_NB] counts, by score
                          // bin, the hits that found the buffer full;
                          // hist_w / hist_iw are the per-query bin width
                          // and its reciprocal
                          int32_t* __restrict__ hist,
                          const float* __restrict__ hist_w,
                          const float* __restrict__ hist_iw) {
  __shared__ bf16 lds_q[4 * BM * BK];
  __shared__ bf16 lds_x[4 * BN * BK];
  __shared__ __attribute__((aligned(16))) uint8_t lds_qs[BM * SCALE9_PITCH];
  __shared__ __attribute__((aligned(16))) uint8_t lds_xs2[BN * SCALE9_PITCH];
  __shared__ __attribute__((aligned(16))) float row_min[BM];
  // owner filter only: query owners, -1 = unfiltered, -2 = garbage row
  __shared__ __attribute__((aligned(16))) int32_t row_owner[OWNED ? BM : 4];
#define QP4N(buf) (lds_q + (buf) * BM * BK)
#define XP4N(buf) (lds_x + (buf) * BN * BK)

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);
  if (x_begin >= x_end) return;

  int wid = wave_id();
  uint32_t wu = (uint32_t)__builtin_amdgcn_readfirstlane(wid);
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int np = D / (2 * BK_F8);
  int sb = D / 32;
  uint32_t ldb = (uint32_t)(D / 2);  // row pitch in bytes

  // scale sheets: this thread's half row (srow, sgrp) and how many of its
  // four dwords the row really has
  uint32_t srow = (wu & 3u) * WAVE + (uint32_t)lane;
  uint32_t sgrp = wu >> 2;
  int snd = min(4, np - 4 * (int)sgrp);  // <= 0: nothing to stage
  bool whole16 = (sb & 15) == 0;
  uint32_t ssheet = srow * SCALE9_PITCH + sgrp * 16u;
  // the half row of tile row srow of the X sheet tile at xt
  auto xs_load = [&](long long xt) {
    return scale9_load(XS, (xt + srow) * (long long)sb + sgrp * 16u,
                       (long long)nx * sb, snd, whole16);
  };
  u32x4_s9 xsr = {0u, 0u, 0u, 0u};
  if (snd > 0) {
    u32x4_s9 qsr = scale9_load(QS, (row0 + srow) * (long long)sb + sgrp * 16u,
                               (long long)nq * sb, snd, whole16);
    xsr = xs_load(x_begin);
    scale9_write(qsr, (uint32_t)(size_t)lds_qs + ssheet);
  }

  for (int i = threadIdx.x; i < BM; i += blockDim.x) {
    bool live = row0 + i < nq;
    row_min[i] = (theta != nullptr && live) ? theta[row0 + i] : -1e30f;
    if constexpr (OWNED) {
      int32_t qo = live ? qowner[row0 + i] : -2;
      row_owner[i] = (live && qo < 0) ? -1 : qo;
    }
  }
  __syncthreads();

  // owner filter: does any of this wave's 128 query rows see every row?
  bool wave_wild = false;
  if constexpr (OWNED)
    wave_wild = __builtin_amdgcn_ballot_w64(
        row_owner[wm * 128 + lane] == -1 || row_owner[wm * 128 + 64 + lane] == -1) != 0;

  uint32_t qoff[2], xoff[2];
  const uint8_t* qbase = Q4 + row0 * (long long)ldb;
  stage_row_offsets_swz<SWZ>(wu, (uint32_t)lane,
                             (uint32_t)min((long long)BM, nq - row0), ldb, qoff);

  // stage pair s of the Q block and of x tile xt into buffer s & 3
  auto stage_pair = [&](long long xt, int s) {
    stage_tile_off(qbase + s * 64, qoff, QP4N(s & 3), wu);
    stage_tile_off(X4 + xt * (long long)ldb + s * 64, xoff, XP4N(s & 3), wu);
  };
  // x tile xt's first interval
  auto stage_head = [&](long long xt) {
    stage_row_offsets_swz<SWZ>(wu, (uint32_t)lane,
                               (uint32_t)min((long long)BN, nx - xt), ldb, xoff);
    stage_pair(xt, 0);
    if (np > 1) stage_pair(xt, 1);
  };

  // block-lifetime read addresses: pair buffer 0 fragments and group 0
  // scale dwords of the lane's first fragment row
  uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
  uint32_t qrow_base = (uint32_t)(wm * 128 + lrow);
  uint32_t xaddr = (uint32_t)(size_t)lds_x
                   + lds_off_bytes_swz<SWZ>(xrow_base, (uint32_t)kgrp);
  uint32_t qaddr = (uint32_t)(size_t)lds_q
                   + lds_off_bytes_swz<SWZ>(qrow_base, (uint32_t)kgrp);
  uint32_t xs_a0 = (uint32_t)(size_t)lds_xs2 + xrow_base * SCALE9_PITCH
                   + (uint32_t)kgrp * 4u;
  uint32_t qs_a0 = (uint32_t)(size_t)lds_qs + qrow_base * SCALE9_PITCH
                   + (uint32_t)kgrp * 4u;

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    // owner filter: the lane's 4 row owners (columns n*16 + lrow); they fly
    // under the K-loop, landed by the interval-0 vmcnt(0). Columns past
    // x_end carry -3: matches nothing, not even an unfiltered query.
    int32_t xo[4] = {-3, -3, -3, -3};
    if constexpr (OWNED) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        long long col = x0 + wn * 64 + n * 16 + lrow;
        if (col < x_end) xo[n] = xowner[col];
      }
    }
    // this tile's X scale sheet from the registers loaded a tile ago,
    // then the next tile's half row into the same registers
    if (snd > 0) {
      scale9_write(xsr, (uint32_t)(size_t)lds_xs2 + ssheet);
      if (x0 + BN < x_end) xsr = xs_load(x0 + BN);
    }
    stage_head(x0);
    // pairs in op_sel groups of four; the two 2-pair intervals of a group
    // are v7's intervals p = 4g and p = 4g + 2
    for (int g = 0; 4 * g < np; ++g) {
      int p = 4 * g;
      uint32_t xs_a = xs_a0 + (uint32_t)g * 16u;
      uint32_t qs_a = qs_a0 + (uint32_t)g * 16u;
      uint32_t xs_v[4], qs_v[8];
      // all outstanding loads are exactly this interval's pairs (plus, at
      // p == 0, the next tile's X scale half row); lgkmcnt(0) retires the
      // tile head's sheet writes ahead of the barrier
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // stage the NEXT interval (pairs p+2, p+3) into the buffers the
      // PREVIOUS interval consumed; overlaps this interval's compute
      if (p + 2 < np) stage_pair(x0, p + 2);
      if (p + 3 < np) stage_pair(x0, p + 3);
      fp4v9_pair<0, true>(acc, xaddr, qaddr, xs_a, qs_a, xs_v, qs_v);
      if (p + 1 < np)
        fp4v9_pair<1, false>(acc, xaddr, qaddr, xs_a, qs_a, xs_v, qs_v);
      if (p + 2 >= np) break;
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (p + 4 < np) stage_pair(x0, p + 4);
      if (p + 5 < np) stage_pair(x0, p + 5);
      fp4v9_pair<2, false>(acc, xaddr, qaddr, xs_a, qs_a, xs_v, qs_v);
      if (p + 3 < np)
        fp4v9_pair<3, false>(acc, xaddr, qaddr, xs_a, qs_a, xs_v, qs_v);
    }
    // nothing is in flight here (the last interval staged nothing); the
    // barrier orders every wave's last fragment and scale reads (a pair
    // ends in lgkmcnt(0)) before the next tile's head overwrites buffers
    // 0,1 and the X scale sheet
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // the lane's 32 thresholds, th[m][r] = row_min[wm*128 + m*16 +
    // (lane>>4)*4 + r]
    f32x4 th[8];
    {
      uint32_t ta = (uint32_t)(size_t)row_min
                    + (uint32_t)(wm * 128 + (lane >> 4) * 4) * 4u;
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:64\n\t"
          "ds_read_b128 %2, %8 offset:128\n\t"
          "ds_read_b128 %3, %8 offset:192\n\t"
          "ds_read_b128 %4, %8 offset:256\n\t"
          "ds_read_b128 %5, %8 offset:320\n\t"
          "ds_read_b128 %6, %8 offset:384\n\t"
          "ds_read_b128 %7, %8 offset:448\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(th[0]), "=&v"(th[1]), "=&v"(th[2]), "=&v"(th[3]),
            "=&v"(th[4]), "=&v"(th[5]), "=&v"(th[6]), "=&v"(th[7])
          : "v"(ta));
    }
    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[0] = acc[0][0][0];
      continue;
    }
    // any-hit test: fmax drops a NaN score exactly as v > theta does
    bool hit = false;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float mx = __builtin_fmaxf(
            __builtin_fmaxf(acc[m][0][r], acc[m][1][r]),
            __builtin_fmaxf(acc[m][2][r], acc[m][3][r]));
        hit |= mx > th[m][r];
      }
    if (__builtin_amdgcn_ballot_w64(hit) == 0) continue;
    // owner filter: the lane's 32 query owners, qo[m][r] laid out like
    // th[m][r], read only behind the score gate
    i32x4_own qo[8];
    if constexpr (OWNED) {
      uint32_t oa = (uint32_t)(size_t)row_owner
                    + (uint32_t)(wm * 128 + (lane >> 4) * 4) * 4u;
      asm volatile(
          "ds_read_b128 %0, %8\n\t"
          "ds_read_b128 %1, %8 offset:64\n\t"
          "ds_read_b128 %2, %8 offset:128\n\t"
          "ds_read_b128 %3, %8 offset:192\n\t"
          "ds_read_b128 %4, %8 offset:256\n\t"
          "ds_read_b128 %5, %8 offset:320\n\t"
          "ds_read_b128 %6, %8 offset:384\n\t"
          "ds_read_b128 %7, %8 offset:448\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(qo[0]), "=&v"(qo[1]), "=&v"(qo[2]), "=&v"(qo[3]),
            "=&v"(qo[4]), "=&v"(qo[5]), "=&v"(qo[6]), "=&v"(qo[7])
          : "v"(oa));
      // gate 2: any (score > theta && owner match) in the wave. Scores of
      // foreign columns are replaced by -inf, then the test is gate 1's.
      if (!wave_wild) {
        bool hit2 = false;
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float mx = -__builtin_inff();
#pragma unroll
            for (int n = 0; n < 4; ++n)
              mx = __builtin_fmaxf(mx, qo[m][r] == xo[n] ? acc[m][n][r]
                                                        : -__builtin_inff());
            hit2 |= mx > th[m][r];
          }
        if (__builtin_amdgcn_ballot_w64(hit2) == 0) continue;
      }
    }
    // slow path, as v7: per-row candidate pointers formed only here
    int lq = lane >> 4;
    asm volatile("" : "+v"(lq));
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[m][n][r];
          if (!(v > th[m][r])) continue;
          if constexpr (OWNED)
            if (!(qo[m][r] == xo[n] || qo[m][r] == -1)) continue;
          int row = wm * 128 + m * 16 + lq * 4 + r;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          } else if constexpr (HIST) {
            // dropped hit: count it by score bin. Pointer and per-query
            // loads are formed here, behind the laundered row index, so
            // queries that fit their buffer pay nothing.
            int b = hist_bin(v, th[m][r], hist_w[grow], hist_iw[grow]);
            atomicAdd(&hist[grow * HIST_NB + b], 1);
          }
        }
  }
#undef QP4N
#undef XP4N
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_v9_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                        const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                        int nq, int nx, int D, int k, int n_swaths,
                        float* __restrict__ cand_scores,
                        int32_t* __restrict__ cand_ids,
                        const float* __restrict__ theta,
                        int32_t* __restrict__ tc_n, int cap) {
  fp4_scan_body<0, false, false>(Q4, QS, X4, XS, nq, nx, D, k, n_swaths,
                                 cand_scores, cand_ids, theta, tc_n, cap, nullptr,
                                 nullptr, nullptr, nullptr, nullptr);
}

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_v10_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                         const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                         int nq, int nx, int D, int k, int n_swaths,
                         float* __restrict__ cand_scores,
                         int32_t* __restrict__ cand_ids,
                         const float* __restrict__ theta,
                         int32_t* __restrict__ tc_n, int cap) {
  fp4_scan_body<1, false, false>(Q4, QS, X4, XS, nq, nx, D, k, n_swaths,
                                 cand_scores, cand_ids, theta, tc_n, cap, nullptr,
                                 nullptr, nullptr, nullptr, nullptr);
}

// v10 with the dropped-hit histogram (overflow="rescan" of the threshold
// recall): the same body, HIST = true. The only extra device code is the
// else of the buffer-full test in the slow path.
extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_hist_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                          const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                          int nq, int nx, int D, int k, int n_swaths,
                          float* __restrict__ cand_scores,
                          int32_t* __restrict__ cand_ids,
                          const float* __restrict__ theta,
                          int32_t* __restrict__ tc_n, int cap,
                          int32_t* __restrict__ hist,
                          const float* __restrict__ hist_w,
                          const float* __restrict__ hist_iw) {
  fp4_scan_body<1, false, true>(Q4, QS, X4, XS, nq, nx, D, k, n_swaths,
                                cand_scores, cand_ids, theta, tc_n, cap, nullptr,
                                nullptr, hist, hist_w, hist_iw);
}

// ===========================================================================
// fp4x4 threshold scan v5: v3's 2-pair intervals + tile-resident scales.
// Q block-scales are invariant across x tiles — staged transposed
// (SCALE_PITCH sheets) once per BLOCK, read as 8 conflict-free b64 per
// lane, then every pair derives its scale byte with VALU shifts. X
// scales load as 4 b64 per tile after the first interval barrier. This
// deletes all 12 per-pair ds_read_u8 (the PMC-measured 6.0e9
// bank-conflict replay cycles) at +24 VGPR of block-lifetime scalars.
// ===========================================================================

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_v5_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                        const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                        int nq, int nx, int D, int k, int n_swaths,
                        float* __restrict__ cand_scores,
                        int32_t* __restrict__ cand_ids,
                        const float* __restrict__ theta,
                        int32_t* __restrict__ tc_n, int cap) {
  __shared__ bf16 lds_q[4 * BM * BK];
  __shared__ bf16 lds_x[4 * BN * BK];
  __shared__ uint8_t lds_qs_t[BM * SCALE_PITCH];
  __shared__ uint8_t lds_xs_t[BN * SCALE_PITCH];
  __shared__ float row_min[BM];
#define QP4C(buf) (lds_q + (buf) * BM * BK)
#define XP4C(buf) (lds_x + (buf) * BN * BK)

  int S = n_swaths;
  int qb = blockIdx.x / S;
  int swath = blockIdx.x % S;
  long long row0 = (long long)qb * BM;

  long long per = ((long long)nx + S - 1) / S;
  per = ((per + BN - 1) / BN) * BN;
  long long x_begin = (long long)swath * per;
  long long x_end = min((long long)nx, x_begin + per);

  for (int i = threadIdx.x; i < BM; i += blockDim.x)
    row_min[i] = (theta != nullptr && row0 + i < nq) ? theta[row0 + i] : -1e30f;
  __syncthreads();

  int wid = wave_id();
  int wm = wid >> 2, wn = wid & 3;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = lane >> 4;
  int np = D / (2 * BK_F8);
  int sb = D / 32;
  size_t cbase = (((size_t)qb * S) + swath) * (size_t)BM * k;
  long long p4_ld = D / 4;

  // Q block scales are invariant across x tiles: stage the transposed
  // sheet once, read each lane's 8 m-row b64 slices once, and derive
  // per-pair scale bytes with VALU shifts — zero per-pair LDS traffic
  // (v1 paid 12 bank-conflicted ds_read_u8 per pair, PMC 6.0e9 replay
  // cycles).
  stage_scale_rows_t(QS, sb, row0, (long long)nq, lds_qs_t, BM);
  __syncthreads();
  uint32_t qslo[8], qshi[8];
  {
    uint32_t qrow_base0 = (uint32_t)(wm * 128 + (lane_id() & 15));
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const uint8_t* a = lds_qs_t + (qrow_base0 + m * 16) * SCALE_PITCH
                         + (lane_id() >> 4) * 8;
      qslo[m] = *(const uint32_t*)a;
      qshi[m] = *(const uint32_t*)(a + 4);
    }
  }

  for (long long x0 = x_begin; x0 < x_end; x0 += BN) {
    f32x4 acc[8][4] = {};
    uint32_t xslo[4], xshi[4];
    stage_scale_rows_t(XS, sb, x0, (long long)nx, lds_xs_t, BN);
    // prologue: stage the first interval's two pairs
    for (int pp = 0; pp < 2 && pp < np; ++pp) {
      stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, pp * 32, QP4C(pp), BM);
      stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, pp * 32, XP4C(pp), BN);
    }
    for (int p = 0; p < np; p += 2) {
      int pe = min(p + 2, np);
      // all outstanding glds are exactly this interval's pairs
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      // stage the NEXT interval (pairs p+2, p+3) into the buffers the
      // PREVIOUS interval consumed; overlaps this interval's compute
      for (int s = p + 2; s < min(np, p + 4); ++s) {
        stage_tile((const bf16*)Q4, p4_ld, row0, (long long)nq, s * 32,
                   QP4C(s & 3), BM);
        stage_tile((const bf16*)X4, p4_ld, x0, (long long)nx, s * 32,
                   XP4C(s & 3), BN);
      }
      if (p == 0) {
        // x scale sheet staged before the interval-0 barrier above
        uint32_t xrb = (uint32_t)(wn * 64 + lrow);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const uint8_t* a = lds_xs_t + (xrb + n * 16) * SCALE_PITCH + kgrp * 8;
          xslo[n] = *(const uint32_t*)a;
          xshi[n] = *(const uint32_t*)(a + 4);
        }
      }
      for (int pc = p; pc < pe; ++pc) {
        uint32_t xrow_base = (uint32_t)(wn * 64 + lrow);
        uint32_t qrow_base = (uint32_t)(wm * 128 + lrow);
        uint32_t xaddr = (uint32_t)(size_t)XP4C(pc & 3)
                         + lds_off_bytes(xrow_base, (uint32_t)kgrp);
        uint32_t qaddr = (uint32_t)(size_t)QP4C(pc & 3)
                         + lds_off_bytes(qrow_base, (uint32_t)kgrp);
        bf16x8 xf[4], qf[8];
        asm volatile(
            "ds_read_b128 %0, %4\n\t"
            "ds_read_b128 %1, %4 offset:1024\n\t"
            "ds_read_b128 %2, %4 offset:2048\n\t"
            "ds_read_b128 %3, %4 offset:3072"
            : "=&v"(xf[0]), "=&v"(xf[1]), "=&v"(xf[2]), "=&v"(xf[3])
            : "v"(xaddr));
        asm volatile(
            "ds_read_b128 %0, %8\n\t"
            "ds_read_b128 %1, %8 offset:1024\n\t"
            "ds_read_b128 %2, %8 offset:2048\n\t"
            "ds_read_b128 %3, %8 offset:3072\n\t"
            "ds_read_b128 %4, %8 offset:4096\n\t"
            "ds_read_b128 %5, %8 offset:5120\n\t"
            "ds_read_b128 %6, %8 offset:6144\n\t"
            "ds_read_b128 %7, %8 offset:7168\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(qf[0]), "=&v"(qf[1]), "=&v"(qf[2]), "=&v"(qf[3]),
              "=&v"(qf[4]), "=&v"(qf[5]), "=&v"(qf[6]), "=&v"(qf[7])
            : "v"(qaddr));
        v8i_mx xv[4], qv[8];
#pragma unroll
        for (int n = 0; n < 4; ++n) xv[n] = fp4_frag(xf[n]);
#pragma unroll
        for (int m = 0; m < 8; ++m) qv[m] = fp4_frag(qf[m]);
#pragma unroll
        for (int m = 0; m < 8; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                qv[m], xv[n], acc[m][n], 4 /*A fp4*/, 4 /*B fp4*/,
                0, (int)scale_byte(qslo[m], qshi[m], pc), 0,
                (int)scale_byte(xslo[n], xshi[n], pc));
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    if (k < 0) {
      if (acc[0][0][0] > 1e29f) cand_scores[cbase] = acc[0][0][0];
      continue;
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = wm * 128 + m * 16 + (lane >> 4) * 4 + r;
          float v = acc[m][n][r];
          if (!(v > row_min[row])) continue;
          long long grow = row0 + row;
          if (grow >= nq) continue;
          long long col = x0 + wn * 64 + n * 16 + (lane & 15);
          if (col >= x_end) continue;
          int pos = atomicAdd(&tc_n[grow], 1);
          if (pos < cap) {
            cand_scores[grow * cap + pos] = v;
            cand_ids[grow * cap + pos] = int32_t(col);
          }
        }
  }
}



// ===========================================================================
// fp4x4 threshold scan, owner-filtered (agent-isolated recall): the v10
// scan (fp4_scan_body: transposed scale sheets, op_sel, counted waits,
// group-aware fragment swizzle) with an owner-aware prologue and epilogue;
// tile geometry, staging and candidate-append format are the unfiltered
// kernel's. A (query, row) pair is eligible iff the query is
// unfiltered (qowner < 0) or xowner[row] == qowner[query].
//  - query owners: staged once per block into LDS (1 KB), -1 = unfiltered,
//    -2 = garbage row (grow >= nq, matches nothing). Read like the
//    thresholds, 8 ds_read_b128 per lane, only after the score gate passes.
//  - row owners: four per-lane global loads at the tile head (the lane's
//    columns n*16 + (lane&15)), landed by the first interval's vmcnt(0);
//    columns past x_end carry -3 (matches nothing, not even an unfiltered
//    query).
//  - gates: v7's score-only any-hit ballot first. Per-owner thresholds sit
//    lower than a whole-index threshold, so with many owners that gate
//    passes in most wave-tiles; a second ballot over (score > theta &&
//    owner match) keeps the 128-element compare/append loop for the
//    wave-tiles that really append. A wave whose 128 query rows include an
//    unfiltered query skips the second gate (block-lifetime flag): the
//    equality test cannot express "matches every row" and the loop is
//    exact either way.
// ===========================================================================

extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_owned_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                           const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                           int nq, int nx, int D, int k, int n_swaths,
                           float* __restrict__ cand_scores,
                           int32_t* __restrict__ cand_ids,
                           const float* __restrict__ theta,
                           int32_t* __restrict__ tc_n, int cap,
                           const int32_t* __restrict__ xowner,
                           const int32_t* __restrict__ qowner) {
  fp4_scan_body<1, true, false>(Q4, QS, X4, XS, nq, nx, D, k, n_swaths,
                                cand_scores, cand_ids, theta, tc_n, cap, xowner,
                                qowner, nullptr, nullptr, nullptr);
}

// the owner-filtered scan with the dropped-hit histogram
extern "C" __global__ void __launch_bounds__(TK_THREADS)
topk_scan_fp4_owned_hist_kernel(const uint8_t* __restrict__ Q4, const uint8_t* __restrict__ QS,
                                const uint8_t* __restrict__ X4, const uint8_t* __restrict__ XS,
                                int nq, int nx, int D, int k, int n_swaths,
                                float* __restrict__ cand_scores,
                                int32_t* __restrict__ cand_ids,
                                const float* __restrict__ theta,
                                int32_t* __restrict__ tc_n, int cap,
                                const int32_t* __restrict__ xowner,
                                const int32_t* __restrict__ qowner,
                                int32_t* __restrict__ hist,
                                const float* __restrict__ hist_w,
                                const float* __restrict__ hist_iw) {
  fp4_scan_body<1, true, true>(Q4, QS, X4, XS, nq, nx, D, k, n_swaths,
                               cand_scores, cand_ids, theta, tc_n, cap, xowner,
                               qowner, hist, hist_w, hist_iw);
}

