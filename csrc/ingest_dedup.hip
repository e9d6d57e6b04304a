// Near-duplicate detection for online ingest (gfx950): the two kernels
// behind PipelineConfig.ingest_dedup. The rule they implement is written
// down in Python, ops.gpu.reference_batch_first_similar and
// ops.gpu.reference_recall_dup_rows. Similarity is the plain dot product of
// bf16 feature rows with fp32 accumulation, which is what recall scores.
//
// batch_first_similar_kernel: first[i] = the smallest j < i with elig[i],
// elig[j], owner[i] == owner[j] and dot(F_i, F_j) >= tau. The host presets
// first[i] = i for an eligible row and -1 otherwise, so "no such j" needs
// no pass of its own: every candidate j is < i and lowers first[i] with an
// atomicMin, which also makes the result independent of scheduling.
//   F . F^T is computed over the lower triangle only, with the tile of
//   csrc/gemm_nt.hip: 128x128 per block, BK = 32, four waves in a 2x2 grid
//   of 64x64 sub-tiles, 4x4 fragments of v_mfma_f32_16x16x32_bf16, LDS
//   double buffered with 16 B of row padding. Block (bm, bn) covers rows i
//   of tile bm and columns j of tile bn; a block with bn > bm lies wholly
//   above the diagonal and returns at once, a diagonal block tests j < i
//   per element. The reduction to min j runs in the block first: a wave
//   that holds no accumulator >= tau skips the element loop altogether;
//   otherwise a lane folds its four column fragments of a row and lowers
//   an LDS row-min. After a barrier the block issues at most one global
//   atomicMin per row, so a batch of identical messages costs B * B/128
//   global atomics, not B^2 / 2.
//
// recall_dup_rows_kernel: for message i, the recalled row with the largest
// dot >= tau among ids[i, :k] (equal dots: the lowest id), or -1. One wave
// per message, the query row held in registers (D <= 2048: four uint4 per
// lane), every candidate row gathered with 16-byte loads, fp32 dot, wave
// reduction. An id outside [0, n_rows) is skipped before anything is
// loaded through it, and with owners a row of another owner is skipped
// before its vector is read, so the kernel stays in bounds whatever ids
// holds.
#include "common.hpp"

#include <climits>

#define DD_TILE 128
#define DD_BK 32
#define DD_PAD 8  // bf16 elements of row padding (16 B), as in gemm_nt.hip
#define DD_STRIDE (DD_BK + DD_PAD)
#define DD_THREADS 256

// [128 rows x 32 cols] bf16 tile into padded LDS: thread = (row, 32-B half),
// rows past `rows` are zero-filled (gemm_nt.hip stage_tile)
DEVINL void dd_stage_tile(const bf16* __restrict__ src, int ld, int row0,
                          int rows, int k0, bf16* lds) {
  int tid = threadIdx.x;
  int r = tid >> 1;
  int half = (tid & 1) * 16;
  bf16x8 v0 = {}, v1 = {};
  int gr = row0 + r;
  if (gr < rows) {
    const bf16* p = src + (size_t)gr * ld + k0 + half;
    v0 = *(const bf16x8*)(p);
    v1 = *(const bf16x8*)(p + 8);
  }
  *(bf16x8*)(lds + r * DD_STRIDE + half) = v0;
  *(bf16x8*)(lds + r * DD_STRIDE + half + 8) = v1;
}

extern "C" __global__ void __launch_bounds__(DD_THREADS)
batch_first_similar_kernel(const bf16* __restrict__ F,        // [B, D]
                           const uint8_t* __restrict__ elig,  // [B] 0/1
                           const int32_t* __restrict__ owner, // [B] or null
                           int B, int D, float tau,
                           int32_t* __restrict__ first) {     // [B], preset
  int bm = blockIdx.x;  // row tile (i)
  int bn = blockIdx.y;  // column tile (j)
  if (bn > bm) return;  // wholly above the diagonal: no j < i in it

  __shared__ bf16 As[2][DD_TILE * DD_STRIDE];
  __shared__ bf16 Bs[2][DD_TILE * DD_STRIDE];
  __shared__ int32_t own_s[2][DD_TILE];  // [0] rows i, [1] columns j
  __shared__ int32_t ok_s[2][DD_TILE];   // eligible and inside the batch
  __shared__ int32_t row_min[DD_TILE];

  int row0 = bm * DD_TILE, col0 = bn * DD_TILE;
  int tid = threadIdx.x;
  {
    int side = tid >> 7, l = tid & (DD_TILE - 1);
    int gi = (side ? col0 : row0) + l;
    bool ok = gi < B && elig[gi] != 0;
    ok_s[side][l] = ok;
    own_s[side][l] = (ok && owner != nullptr) ? owner[gi] : 0;
    if (side == 0) row_min[l] = INT_MAX;
  }

  int wid = wave_id();
  int wm = wid >> 1, wn = wid & 1;
  int lane = lane_id();
  int lrow = lane & 15;
  int kgrp = (lane >> 4) * 8;

  f32x4 acc[4][4] = {};

  dd_stage_tile(F, D, row0, B, 0, As[0]);
  dd_stage_tile(F, D, col0, B, 0, Bs[0]);
  __syncthreads();

  int nk = D / DD_BK;
  for (int kt = 0; kt < nk; ++kt) {
    int cur = kt & 1, nxt = cur ^ 1;
    if (kt + 1 < nk) {
      dd_stage_tile(F, D, row0, B, (kt + 1) * DD_BK, As[nxt]);
      dd_stage_tile(F, D, col0, B, (kt + 1) * DD_BK, Bs[nxt]);
    }
    bf16x8 afrag[4], bfrag[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      afrag[m] = *(const bf16x8*)(As[cur] + (wm * 64 + m * 16 + lrow) * DD_STRIDE + kgrp);
#pragma unroll
    for (int n = 0; n < 4; ++n)
      bfrag[n] = *(const bf16x8*)(Bs[cur] + (wn * 64 + n * 16 + lrow) * DD_STRIDE + kgrp);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n)
        acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[m], bfrag[n], acc[m][n], 0, 0, 0);
    __syncthreads();
  }

  // any-hit gate: most waves hold nothing above tau
  bool hit = false;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) hit |= acc[m][n][r] >= tau;

  if (__any(hit)) {
    // C layout: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int li = wm * 64 + m * 16 + (lane >> 4) * 4 + r;
        int i = row0 + li;
        if (!ok_s[0][li]) continue;
        int own_i = own_s[0][li];
        int best = INT_MAX;
#pragma unroll
        for (int n = 3; n >= 0; --n) {
          int lj = wn * 64 + n * 16 + lrow;
          int j = col0 + lj;
          if (acc[m][n][r] >= tau && j < i && ok_s[1][lj] && own_s[1][lj] == own_i)
            best = j;  // n descends, so the last one taken is the smallest j
        }
        if (best != INT_MAX) atomicMin(&row_min[li], best);
      }
    }
  }
  __syncthreads();
  // ok_s[0] implies row0 + l < B, and only such rows have a row_min
  if (tid < DD_TILE && row_min[tid] != INT_MAX) atomicMin(&first[row0 + tid], row_min[tid]);
}

DEVINL float dd_dot8(uint4 a, uint4 b, float s) {
  const uint32_t aw[4] = {a.x, a.y, a.z, a.w};
  const uint32_t bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    // a bf16 is the high half of an fp32
    s = fmaf(__uint_as_float(aw[w] << 16), __uint_as_float(bw[w] << 16), s);
    s = fmaf(__uint_as_float(aw[w] & 0xFFFF0000u), __uint_as_float(bw[w] & 0xFFFF0000u), s);
  }
  return s;
}

extern "C" __global__ void __launch_bounds__(256)
recall_dup_rows_kernel(const uint4* __restrict__ F,          // bf16 bits [B, D]
                       const int32_t* __restrict__ ids,      // [B, k]
                       const uint4* __restrict__ X,          // bf16 bits [n_rows, D]
                       const int32_t* __restrict__ xowner,   // [n_rows] or null
                       const int32_t* __restrict__ qowner,   // [B] or null (with xowner)
                       int B, int k, int D, int n_rows, float tau,
                       int32_t* __restrict__ dup_row,        // [B]
                       float* __restrict__ dup_dot) {        // [B]
  const int lane = threadIdx.x & 63;
  const int wave = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int n_waves = (int)(((long long)gridDim.x * blockDim.x) >> 6);
  const int row_q = D >> 3;  // uint4 per row, <= 256

  for (int i = wave; i < B; i += n_waves) {
    uint4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      q[u] = make_uint4(0, 0, 0, 0);
      if (lane + u * 64 < row_q) q[u] = F[(long long)i * row_q + lane + u * 64];
    }
    const int qo = xowner != nullptr ? qowner[i] : 0;
    float best = -INFINITY;
    int best_id = -1;
    for (int c = 0; c < k; ++c) {
      const int id = __builtin_amdgcn_readfirstlane(ids[(long long)i * k + c]);
      if ((unsigned)id >= (unsigned)n_rows) continue;  // -1, stale or foreign
      if (xowner != nullptr && xowner[id] != qo) continue;
      const uint4* px = X + (long long)id * row_q;
      uint4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        x[u] = make_uint4(0, 0, 0, 0);
        if (lane + u * 64 < row_q) x[u] = px[lane + u * 64];
      }
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) s = dd_dot8(q[u], x[u], s);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (s >= tau && (s > best || (s == best && id < best_id))) {
        best = s;
        best_id = id;
      }
    }
    if (lane == 0) {
      dup_row[i] = best_id;
      dup_dot[i] = best;
    }
  }
}
