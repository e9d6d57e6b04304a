// Find the rows that hold given memory ids (gfx950).
//
// The live recall index carries one int64 id per row (the ids column,
// written by fp4_quantize_append_kernel and moved by index_move_rows_kernel).
// Rows move at a forget, ids do not, so "which row holds id x now" is a
// search of the column. It is one pass over the column per chunk of wanted
// ids: no per-row temporaries, no host read.
//
// want is a chunk of m <= FIND_CHUNK ids, ascending and distinct (the
// wrapper sorts and de-duplicates), staged once per block in LDS (32 KB at
// the full chunk). Every row's id is first tested against the chunk's
// range [want[0], want[m-1]] and only then searched (branch-free lower
// bound, 12 LDS reads at the full chunk). A hit does
// atomicMax(&row_out[pos], row) into an output the caller prefilled with
// -1, so of several rows holding one id the highest wins, whatever the
// order the blocks run in. A negative id in the column matches nothing, so
// a negative wanted id is never found.
//
// The column is read 16 bytes per lane. A column view that starts on an odd
// element is only 8-byte aligned: its first element is peeled off, the
// rest is read as aligned pairs, and an odd last element is peeled off as
// well; lanes 0 and 1 of the first block take the two peeled elements.
#include <hip/hip_runtime.h>

#include <cstdint>

#define FIND_CHUNK 4096

extern "C" __global__ __launch_bounds__(256)
void index_find_ids_kernel(
    const long long* __restrict__ col,   // [n] ids of the live rows
    long long n,                         // < 2^31
    const long long* __restrict__ want,  // [m] ascending, distinct
    int m,                               // 1 <= m <= FIND_CHUNK
    int32_t* __restrict__ row_out)       // [m] prefilled with -1
{
  __shared__ long long s[FIND_CHUNK];
  for (int i = threadIdx.x; i < m; i += blockDim.x) s[i] = want[i];
  __syncthreads();
  const long long lo_id = s[0], hi_id = s[m - 1];

  auto probe = [&](long long v, long long row) {
    // lo_id may be negative; no negative id is ever found
    if (v < 0 || v < lo_id || v > hi_id) return;
    int lo = 0, len = m;
    while (len > 1) {
      const int half = len >> 1;
      lo = (s[lo + half] <= v) ? lo + half : lo;
      len -= half;
    }
    if (s[lo] == v) atomicMax(&row_out[lo], (int)row);
  };

  const long long head = ((reinterpret_cast<uintptr_t>(col) & 15) != 0 && n > 0) ? 1 : 0;
  const long long n_pairs = (n - head) >> 1;
  const longlong2* pairs = reinterpret_cast<const longlong2*>(col + head);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs;
       p += stride) {
    const longlong2 v = pairs[p];
    const long long row = head + 2 * p;
    probe(v.x, row);
    probe(v.y, row + 1);
  }
  if (blockIdx.x == 0) {
    const long long tail = head + 2 * n_pairs;  // n - 1 when one is left
    if (threadIdx.x == 0 && head) probe(col[0], 0);
    if (threadIdx.x == 1 && tail < n) probe(col[tail], tail);
  }
}
