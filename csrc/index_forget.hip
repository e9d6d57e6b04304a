// In-place row moves for forgetting in the live recall index (gfx950).
//
// Forgetting removes a set of live rows and keeps the live rows the
// contiguous prefix of every index buffer. The compaction rule is hole
// filling (ops.gpu.forget_plan): the dead rows below the new row count are
// the destinations, the live rows at or above it the sources, both
// ascending and equally many. Row order is NOT preserved; nothing depends
// on it, salience carries age. Sources and destinations are disjoint and
// the destinations unique, so the pairs need no ordering among themselves,
// no second copy of the index, no atomics and no block waits on another.
//
// One launch moves, for every pair j < m, row src[j] onto row dst[j] of
// every buffer it is given (a null buffer is left out):
//   - the bf16 index       [cap, D]     2*D bytes   uint4 per lane
//   - the fp4 codes X4     [cap, D/2]   D/2 bytes   uint4 per lane
//   - the e8m0 scales XS   [cap, D/32]  D/32 bytes  dwords (4 B at D = 128)
//   - owner (int32) and salience (fp32) [cap]       one dword each
//   - the memory ids (int64) [cap]                  one 8-byte word
// X4/XS have the row layout fp4_quantize_append_kernel writes: codes and
// scales are row-major per row, so a move is a byte copy. Copies are
// bitwise; every byte outside the rows named in dst stays as it is.
//
// Mapping: one wave per pair, pairs grid-strided over the waves. src[j] and
// dst[j] are wave-uniform (read once, kept in scalar registers), so the row
// bases are computed once per pair. A pair's loads are all issued before
// its first store. A pair with either index outside [0, cap) is skipped,
// as the append kernel leaves the destination of a bad source row alone:
// the kernel stays in bounds whatever src and dst hold. dst not unique, or
// not disjoint from src, gives an unspecified (but in-bounds) result.
//
// Needs D % 8 == 0 for the bf16 rows and D % 128 == 0, D <= 2048 for X4/XS
// (one uint4 of codes and one scale dword per lane at most).
#include <hip/hip_runtime.h>

#include <cstdint>

extern "C" __global__ __launch_bounds__(256)
void index_move_rows_kernel(
    const int32_t* __restrict__ src,  // [m]
    const int32_t* __restrict__ dst,  // [m]
    long long m, int cap, int D,
    uint4* index,        // bf16 bits [cap, D] or null
    uint4* X4,           // [cap, D/2] or null
    uint32_t* XS,        // [cap, D/32] or null (with X4)
    uint32_t* owner,     // int32 bits [cap] or null
    uint32_t* salience,  // fp32 bits [cap] or null
    uint2* ids)          // int64 bits [cap] or null
{
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
  const int row_q = D >> 3;    // uint4 per bf16 row
  const int code_q = D >> 5;   // uint4 per code row (<= 64)
  const int scale_w = D >> 7;  // dwords per scale row (<= 16)

  for (long long j = wave; j < m; j += n_waves) {
    const int s = __builtin_amdgcn_readfirstlane(src[j]);
    const int d = __builtin_amdgcn_readfirstlane(dst[j]);
    if ((unsigned)s >= (unsigned)cap || (unsigned)d >= (unsigned)cap) continue;

    // the short rows first: their loads stay in flight over the bf16 row
    uint4 code = make_uint4(0, 0, 0, 0);
    uint32_t scale = 0, own = 0, sal = 0;
    uint2 id = make_uint2(0, 0);
    if (X4 != nullptr) {
      if (lane < code_q) code = X4[(long long)s * code_q + lane];
      if (lane < scale_w) scale = XS[(long long)s * scale_w + lane];
    }
    if (lane == 0) {
      if (owner != nullptr) own = owner[s];
      if (salience != nullptr) sal = salience[s];
      if (ids != nullptr) id = ids[s];
    }

    if (index != nullptr) {
      const uint4* ps = index + (long long)s * row_q;
      uint4* pd = index + (long long)d * row_q;
      // 4 uint4 per lane in flight: a 4-KiB slice of the row per trip
      for (int c0 = lane; c0 < row_q; c0 += 256) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          v[u] = make_uint4(0, 0, 0, 0);
          if (c0 + u * 64 < row_q) v[u] = ps[c0 + u * 64];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (c0 + u * 64 < row_q) pd[c0 + u * 64] = v[u];
      }
    }

    if (X4 != nullptr) {
      if (lane < code_q) X4[(long long)d * code_q + lane] = code;
      if (lane < scale_w) XS[(long long)d * scale_w + lane] = scale;
    }
    if (lane == 0) {
      if (owner != nullptr) owner[d] = own;
      if (salience != nullptr) salience[d] = sal;
      if (ids != nullptr) ids[d] = id;
    }
  }
}
