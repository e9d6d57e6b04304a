// Fused bf16 -> MXFP4 quantize / index-append kernel (gfx950).
//
// One launch reads bf16 rows once and writes, per destination row:
//   - the packed e2m1 nibbles in the hardware fragment order of the fp4
//     scan's B operand (ops.gpu.fp4_perm128), X4 [*, D/2]
//   - the e8m0 group scales, XS [*, D/32]
//   - optionally the bf16 copy, the owner id, the initial salience and the
//     row's stable memory id (id_base + the batch position it came from)
// The output is bit-for-bit ops.gpu.to_fp4_mx (the torch oracle) on finite
// input; ops.gpu.fp4_mx_spec states the same integer rule in Python.
//
// Mapping: one lane per 16-element half-group, lanes in OUTPUT order. Lane
// h of a row (h in [0, D/16)) is chunk c = h>>3, group g = (h>>1)&3,
// half = h&1; it loads the 32 contiguous source bytes at element
// c*128 + (g&1)*64 + (g>>1)*16 + half*32 and stores 8 code bytes at
// h*8, so a wave's stores are contiguous and its loads cover whole 256-B
// chunks. The two halves of a scale group sit in lanes h and h^1 and
// exchange their max. D % 128 == 0 makes every row a multiple of 8 lanes,
// so a pair, and the 8 lanes of a chunk, never straddle a row or a wave.
//
// Scale rule (no log2): the group max as a bf16 bit pattern has exponent
// field E and mantissa M; for a normal max, ceil(log2(max/6)) is E-129
// when M <= 64 (max <= 1.5 * 2^(E-127)) and E-128 otherwise, clamped to
// [-127, 127]. A zero max gives e = 0, a subnormal max e = -127.
// Code rule: y = v * 2^-e (exact), magnitude code = number of e2m1
// midpoints strictly below |y| (ties take the lower code), sign bit iff
// y < 0 (fp32 compare, so a value that underflows to -0 has no sign bit).
#include <hip/hip_runtime.h>

#include <cstdint>

extern "C" __global__ __launch_bounds__(256)
void fp4_quantize_append_kernel(
    const uint16_t* __restrict__ feats,    // bf16 bits [m, D]
    const int32_t* __restrict__ src_idx,   // [n] or null (row i <- row i)
    int m, long long n, int D, long long dst_row0,
    uint16_t* __restrict__ index_dst,      // bf16 bits [cap, D] or null
    uint8_t* __restrict__ X4,              // [cap, D/2] or null
    uint8_t* __restrict__ XS,              // [cap, D/32] or null
    int32_t* __restrict__ owner_dst,       // [cap] or null
    const int32_t* __restrict__ owner_src, // [m] (with owner_dst)
    float* __restrict__ salience_dst,      // [cap] or null
    float salience_init,
    long long* __restrict__ id_dst,        // int64 [cap] or null
    long long id_base) {
  const int lpr = D >> 4;  // lanes per row
  const long long items = n * lpr;
  const long long stride = (long long)gridDim.x * blockDim.x;
  // trip count is uniform over the block: the shuffles below run with
  // every lane of the wave present
  for (long long base = (long long)blockIdx.x * blockDim.x; base < items;
       base += stride) {
    const bool active = base + threadIdx.x < items;
    // the 64-bit division is block-uniform; a lane adds a 32-bit one
    const long long row0 = base / lpr;
    const unsigned t = (unsigned)(base - row0 * lpr) + threadIdx.x;
    const long long i = row0 + t / (unsigned)lpr;
    const int h = (int)(t % (unsigned)lpr);
    long long src = i;
    if (src_idx != nullptr && active) src = src_idx[i];
    // a source row outside feats leaves its destination row untouched
    const bool ok = active && src >= 0 && src < m;
    const long long dst = dst_row0 + i;

    const int c = h >> 3, g = (h >> 1) & 3, half = h & 1;
    const int e0 = c * 128 + (g & 1) * 64 + (g >> 1) * 16 + half * 32;

    uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
    if (ok) {
      const uint4* p = reinterpret_cast<const uint4*>(feats + src * D + e0);
      lo = p[0];
      hi = p[1];
    }
    if (ok && index_dst != nullptr) {
      uint4* q = reinterpret_cast<uint4*>(index_dst + dst * D + e0);
      q[0] = lo;
      q[1] = hi;
    }
    if (ok && h == 0) {
      if (owner_dst != nullptr) owner_dst[dst] = owner_src[src];
      if (salience_dst != nullptr) salience_dst[dst] = salience_init;
      if (id_dst != nullptr) id_dst[dst] = id_base + src;
    }
    if (X4 == nullptr) continue;  // uniform

    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    // bf16 magnitudes order like their 15-bit patterns
    uint32_t amax = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t a = w[j] & 0x7fffu, b = (w[j] >> 16) & 0x7fffu;
      amax = max(amax, max(a, b));
    }
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));

    const int E = (int)(amax >> 7), M = (int)(amax & 0x7f);
    int e = (M <= 64) ? E - 129 : E - 128;
    e = e < -127 ? -127 : e;
    if (amax == 0) e = 0;
    // 2^-e; e <= 126 for any finite max, so the exponent field is >= 1
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);

    uint32_t codes[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t bits = (j & 1) ? (w[j >> 1] & 0xffff0000u) : (w[j >> 1] << 16);
      const float y = __uint_as_float(bits) * inv;
      const float a = fabsf(y);
      // midpoints strictly below a: 0.25, 0.75, 1.25, 1.75 are counted by
      // ceil(2a - 0.5), which is never below -0 and, a being a bf16 times a
      // power of two, rounds nowhere near an integer; the rest are compared
      uint32_t code = min((uint32_t)ceilf(fmaf(a, 2.0f, -0.5f)), 4u) +
                      (uint32_t)(a > 2.5f) + (uint32_t)(a > 3.5f) +
                      (uint32_t)(a > 5.0f);
      code |= (y < 0.0f) ? 8u : 0u;
      codes[j >> 3] |= code << ((j & 7) * 4);
    }
    if (ok)
      *reinterpret_cast<uint2*>(X4 + dst * (D >> 1) + (long long)h * 8) =
          make_uint2(codes[0], codes[1]);

    // the chunk's 4 scale bytes leave as one dword from its first lane
    const uint32_t sb = (uint32_t)(e + 127);
    const uint32_t s1 = (uint32_t)__shfl_down((int)sb, 2);
    const uint32_t s2 = (uint32_t)__shfl_down((int)sb, 4);
    const uint32_t s3 = (uint32_t)__shfl_down((int)sb, 6);
    if (ok && (h & 7) == 0)
      *reinterpret_cast<uint32_t*>(XS + dst * (D >> 5) + c * 4) =
          sb | (s1 << 8) | (s2 << 16) | (s3 << 24);
  }
}
