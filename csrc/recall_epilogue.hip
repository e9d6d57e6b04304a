// The two ends of threshold recall that sit around the index scan (gfx950),
// ops.gpu.topk_recall_threshold steps 1 and 3-4.
//
// row_moments_kernel: mean and correction=1 standard deviation of every row
// of the bf16 sample-score matrix, in ONE pass over it. One block per row,
// 16-byte loads. Sums are kept in fp64 and SHIFTED by the row's first
// element c: s1 = sum(x - c), s2 = sum((x - c)^2), mean = c + s1 / m, var =
// (s2 - s1^2 / m) / (m - 1). x - c is exact in fp64 for bf16 operands, and
// with the shift next to the data s2 and s1^2 / m differ by the row's own
// spread, so nothing cancels (a constant row gives exactly 0). The order of
// the sums is fixed: a thread's elements in address order, a butterfly over
// the wave, then the waves in order; no float atomics.
//
// select_rescore_kernel: one block per query turns the scan's candidate
// buffer into the final top-k. It loads the filled slots into LDS, keeps the
// `sel` best by scan score, gathers those rows of X with 16-byte loads and
// scores them exactly (bf16 x bf16 products are exact in fp32, fp32 sums),
// weights by salience and keeps the top k. Both selections rank by counting:
// an entry's place is the number of entries that beat it, where "beats" is
// (higher score, then lower row id, then lower slot), a total order, so the
// result does not depend on the order the scan's atomics filled the slots
// in, nor on scheduling. The dot of a row is summed per lane in address
// order and then by a butterfly over the wave, the same whichever wave takes
// the row. An id outside [0, nx) is never loaded through: it scores -1e30
// and comes out as id -1, which is also what fills positions past the valid
// candidates.
#include "common.hpp"

#define RM_THREADS 256

DEVINL double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

DEVINL double bf16_bits_f64(uint32_t hi16) { return (double)__uint_as_float(hi16); }

extern "C" __global__ void __launch_bounds__(RM_THREADS)
row_moments_kernel(const uint16_t* __restrict__ S,  // bf16 bits [nq, m]
                   int m, float* __restrict__ mu, float* __restrict__ sigma) {
  __shared__ double red[2][RM_THREADS / WAVE];
  const int tid = threadIdx.x;
  const uint16_t* row = S + (size_t)blockIdx.x * m;
  const double c = bf16_bits_f64((uint32_t)row[0] << 16);

  // [0, head) up to the first 16-byte boundary, nvec whole uint4, then a tail
  const int head = min(m, (int)(((16u - ((uintptr_t)row & 15u)) & 15u) >> 1));
  const int nvec = (m - head) >> 3;
  const int tail0 = head + nvec * 8;
  const uint4* body = (const uint4*)(row + head);

  double s1 = 0.0, s2 = 0.0;
  if (tid < head) {
    const double d = bf16_bits_f64((uint32_t)row[tid] << 16) - c;
    s1 += d;
    s2 = fma(d, d, s2);
  }
#pragma unroll 4
  for (int v = tid; v < nvec; v += RM_THREADS) {
    const uint4 q = body[v];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double d0 = bf16_bits_f64(w[i] << 16) - c;
      const double d1 = bf16_bits_f64(w[i] & 0xFFFF0000u) - c;
      s1 += d0;
      s2 = fma(d0, d0, s2);
      s1 += d1;
      s2 = fma(d1, d1, s2);
    }
  }
  if (tail0 + tid < m) {  // at most 7 elements
    const double d = bf16_bits_f64((uint32_t)row[tail0 + tid] << 16) - c;
    s1 += d;
    s2 = fma(d, d, s2);
  }

  s1 = wave_sum_f64(s1);
  s2 = wave_sum_f64(s2);
  if (lane_id() == 0) {
    red[0][wave_id()] = s1;
    red[1][wave_id()] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int w = 0; w < RM_THREADS / WAVE; ++w) {
      t1 += red[0][w];
      t2 += red[1][w];
    }
    const double dm = (double)m;
    const double var = m > 1 ? fmax(t2 - t1 * t1 / dm, 0.0) / (dm - 1.0) : NAN;
    mu[blockIdx.x] = (float)(c + t1 / dm);
    sigma[blockIdx.x] = (float)sqrt(var);
  }
}

#define SR_THREADS 256
#define SR_WAVES (SR_THREADS / WAVE)
#define SR_MAX_CAP 1024
#define SR_PER_THREAD (SR_MAX_CAP / SR_THREADS)
#define SR_MAX_ROW_Q 256  // uint4 per row: D <= 2048
#define SR_Q_PER_LANE (SR_MAX_ROW_Q / WAVE)
#define SR_NEG (-1e30f)

// entry (sj, ij) at slot j goes ahead of entry (sc, ic) at slot c
DEVINL bool sr_beats(float sj, int ij, int j, float sc, int ic, int c) {
  return sj > sc || (sj == sc && (ij < ic || (ij == ic && j < c)));
}

// place[u] = rank of entry tid + u * SR_THREADS among the n entries in LDS
DEVINL void sr_rank(const float* s, const int32_t* id, int n, int place[SR_PER_THREAD]) {
  float sc[SR_PER_THREAD];
  int ic[SR_PER_THREAD];
#pragma unroll
  for (int u = 0; u < SR_PER_THREAD; ++u) {
    const int c = threadIdx.x + u * SR_THREADS;
    sc[u] = c < n ? s[c] : 0.f;
    ic[u] = c < n ? id[c] : 0;
    place[u] = 0;
  }
  for (int j = 0; j < n; ++j) {
    const float sj = s[j];  // same address in every lane: an LDS broadcast
    const int ij = id[j];
#pragma unroll
    for (int u = 0; u < SR_PER_THREAD; ++u)
      place[u] += sr_beats(sj, ij, j, sc[u], ic[u], (int)threadIdx.x + u * SR_THREADS) ? 1 : 0;
  }
}

DEVINL void sr_unpack8(uint4 v, float f[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // a bf16 is the high half of an fp32
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
  }
}

extern "C" __global__ void __launch_bounds__(SR_THREADS)
select_rescore_kernel(const float* __restrict__ cs,       // [nq, cap]
                      const int32_t* __restrict__ ci,     // [nq, cap]
                      const int32_t* __restrict__ counts, // [nq], may exceed cap
                      const uint4* __restrict__ Q,        // bf16 bits [nq, D]
                      const uint4* __restrict__ X,        // bf16 bits [nx, D]
                      const float* __restrict__ salience, // [nx] or null
                      int cap, int sel, int k, int D, int nx,
                      float* __restrict__ out_s,          // [nq, k]
                      int32_t* __restrict__ out_i) {      // [nq, k]
  __shared__ float a_s[SR_MAX_CAP];    // candidates as scanned
  __shared__ int32_t a_i[SR_MAX_CAP];
  __shared__ float b_s[SR_MAX_CAP];    // the selected ones, then their exact scores
  __shared__ int32_t b_i[SR_MAX_CAP];

  const int q = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = wave_id();
  const int row_q = D >> 3;
  const int n = min(max(counts[q], 0), cap);

  for (int c = tid; c < n; c += SR_THREADS) {
    a_s[c] = cs[(size_t)q * cap + c];
    a_i[c] = ci[(size_t)q * cap + c];
  }
  __syncthreads();

  // 1. the sel best by scan score
  const int nsel = min(n, sel);
  int place[SR_PER_THREAD];
  sr_rank(a_s, a_i, n, place);
#pragma unroll
  for (int u = 0; u < SR_PER_THREAD; ++u) {
    const int c = tid + u * SR_THREADS;
    if (c < n && place[u] < nsel) b_i[place[u]] = a_i[c];
  }

  // the query row, converted once
  float qf[SR_Q_PER_LANE][8];
#pragma unroll
  for (int u = 0; u < SR_Q_PER_LANE; ++u) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (lane + u * WAVE < row_q) v = Q[(size_t)q * row_q + lane + u * WAVE];
    sr_unpack8(v, qf[u]);
  }
  __syncthreads();

  // 2. exact rescore: a wave per selected row, two rows in flight
  for (int r0 = wave * 2; r0 < nsel; r0 += SR_WAVES * 2) {
    int id[2];
    uint4 x[2][SR_Q_PER_LANE];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      id[t] = r0 + t < nsel ? b_i[r0 + t] : -1;
      if ((unsigned)id[t] >= (unsigned)nx) id[t] = -1;  // wave-uniform
      const uint4* px = X + (size_t)max(id[t], 0) * row_q;
#pragma unroll
      for (int u = 0; u < SR_Q_PER_LANE; ++u) {
        x[t][u] = make_uint4(0, 0, 0, 0);
        if (id[t] >= 0 && lane + u * WAVE < row_q) x[t][u] = px[lane + u * WAVE];
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < SR_Q_PER_LANE; ++u) {
        float xf[8];
        sr_unpack8(x[t][u], xf);
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(qf[u][i], xf[i], s);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0 && r0 + t < nsel) {
        if (id[t] >= 0 && salience != nullptr) s *= salience[id[t]];
        b_s[r0 + t] = id[t] >= 0 ? s : SR_NEG;
        b_i[r0 + t] = id[t];
      }
    }
  }
  __syncthreads();

  // 3. top k by exact score; the rest of the k positions are padding
  sr_rank(b_s, b_i, nsel, place);
#pragma unroll
  for (int u = 0; u < SR_PER_THREAD; ++u) {
    const int c = tid + u * SR_THREADS;
    if (c < nsel && place[u] < k) {
      out_s[(size_t)q * k + place[u]] = b_s[c];
      out_i[(size_t)q * k + place[u]] = b_i[c];
    }
  }
  for (int r = nsel + tid; r < k; r += SR_THREADS) {
    out_s[(size_t)q * k + r] = SR_NEG;
    out_i[(size_t)q * k + r] = -1;
  }
}
