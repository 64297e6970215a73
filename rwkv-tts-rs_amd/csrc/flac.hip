// flac.hip -- a FLAC encoder on the MI355X, for `format: "flac"` of the TTS routes: f32 PCM in, the
// frames of a mono 16-bit FLAC stream (RFC 9639, streamable subset, fixed block size) out, one-shot,
// batched (a rate, a block size and a scale per signal) and over exact stream windows. No reference
// counterpart: the reference sends WAV only.
//
// The contract is in include/rwkvtts.h: every output bit is defined, and the kernels
// are pinned bitwise to the numpy restatement (tests/flac_ref.py). All of it is integer arithmetic
// but the quantisation (three rounded f32 operations) and the Levinson-Durbin recursion (f64, one
// rounded operation at a time, on one lane).
//
// Work: k_flac_frame gives a workgroup to a block. It quantises the block into LDS and tries every
// subframe candidate by exact bit count: a lane per sample computes the residual and adds its 15
// shifted zigzag values into the sums of its finest Rice partition (LDS atomics); the sums of the
// coarser partition orders follow by pairwise adds, a lane per partition picks the best parameter,
// and lane 0 keeps the smallest candidate. The winner is written into a zeroed LDS frame buffer --
// code lengths, a workgroup prefix sum, then every sample ORs its stop bit and low bits in -- the
// CRC-16 is taken slice by slice and combined by multiplication with powers of x (it is linear), and
// the frame goes to a strided global slot with its length. k_flac_pack sums the lengths before each
// tile of 256 frames and copies the frames back to back; only the packed bytes cross to the host.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

namespace rwkvtts {

constexpr int kFlacThreads = 256;
constexpr int kFlacMaxB = 4096;
constexpr int kFlacFrameWords = (2 * kFlacMaxB + 16) / 4;  // the largest frame, 2 n + 16 bytes
constexpr int kFlacMaxLpc = 12, kFlacMaxK = 14, kFlacMaxPo = 8, kFlacPrecision = 12;
constexpr int kFlacTable = 256 + 512 + 1024 + 2048 + 4096;
constexpr int kFlacCands = 5 + kFlacMaxLpc;  // FIXED 0 .. 4, then LPC 1 .. 12
// A partition's 15 sums are a row of 17 words: an odd stride, so that lanes on neighbouring partitions
// (the atomics of the search, a lane per partition in the merges) fall on different LDS banks.
constexpr int kFlacRow = 17;
// A term zz >> k is capped here in the sums. A candidate with a capped term has more than 2^19 bits,
// above VERBATIM's at most 8 + 16 * 4096, so it never wins, and neither does a capped parameter or
// partition order inside the winner: the output is that of the exact sums. 4096 capped terms and the
// (k + 1) * n + 4 * 256 beside them stay below 2^32.
constexpr uint32_t kFlacTermCap = 1u << 19;

// One grid row of k_flac_frame: a window of whole blocks (and, with final, a short last one).
struct FlacJob {
  int64_t in_off, n;   // samples x[in_off, in_off + n)
  int64_t slot_off;    // bytes: frame b goes to slots[slot_off + b * (2 B + 16)]
  int64_t len_off;     // its length to lens[len_off + b]
  int64_t out_off;     // bytes: the packed frames start at out[out_off]
  int64_t nblocks;
  uint32_t first_frame;
  int32_t B, bs_code, rate_code, tab_off, lpc;
  float scale;
};

struct FlacRes {
  unsigned long long total;
  uint32_t min_frame, max_frame;
};

__host__ __device__ inline int flac_window_q15(int i, int n) {
  const long long d = 2ll * i - n + 1, D = (long long)n + 1;
  return (int)(32768ll - (32768ll * d * d) / (D * D));
}

__host__ __device__ inline int flac_utf8_len(uint32_t v) {
  return v < 0x80u ? 1 : v < 0x800u ? 2 : v < 0x10000u ? 3 : v < 0x200000u ? 4 : v < 0x4000000u ? 5 : 6;
}

__device__ inline int flac_order(int cand) { return cand < 5 ? cand : cand - 4; }

// The residual of sample i >= order. An LPC sum is at most 12 * 2048 * 32767 < 2^31 in magnitude, so
// the int64 accumulator of the contract fits int32, and so does every residual.
__device__ inline int flac_residual(const int* s, int i, int cand, const int* coef, int shift) {
  switch (cand) {
    case 0: return s[i];
    case 1: return s[i] - s[i - 1];
    case 2: return s[i] - 2 * s[i - 1] + s[i - 2];
    case 3: return s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
    case 4: return s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
    default: break;
  }
  const int p = cand - 4;
  int acc = 0;
  for (int j = 0; j < p; ++j) acc += coef[j] * s[i - 1 - j];
  return s[i] - (acc >> shift);
}

__device__ inline uint32_t flac_zigzag(int r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// S[p * kFlacRow + k] += min(zz >> k, cap) for every sample i >= order, p = i / plen.
__device__ inline void flac_accumulate(const int* s, int n, int cand, int order, const int* coef, int shift, int plen,
                                       uint32_t* S, int tid) {
  for (int i = tid; i < n; i += kFlacThreads) {
    if (i < order) continue;
    const uint32_t zz = flac_zigzag(flac_residual(s, i, cand, coef, shift));
    uint32_t* row = S + (i / plen) * kFlacRow;
#pragma unroll
    for (int k = 0; k <= kFlacMaxK; ++k) atomicAdd(&row[k], min(zz >> k, kFlacTermCap));
  }
}

// ORs the nb low bits of v (nb <= 32, v < 2^nb) into the frame buffer at bit pos, the most significant
// first; word w holds bits [32 w, 32 w + 32) with bit 32 w in its top.
__device__ inline void flac_put(uint32_t* buf, uint32_t pos, uint32_t v, int nb) {
  if (nb == 0) return;
  const uint32_t w = pos >> 5;
  const int end = (int)(pos & 31) + nb;
  if (w >= (uint32_t)kFlacFrameWords) return;  // (never: the winner is no larger than VERBATIM)
  if (end <= 32) {
    atomicOr(&buf[w], v << (32 - end));
  } else {
    atomicOr(&buf[w], v >> (end - 32));
    if (w + 1 < (uint32_t)kFlacFrameWords) atomicOr(&buf[w + 1], v << (64 - end));
  }
}

__device__ inline uint32_t flac_byte(const uint32_t* buf, int b) { return (buf[b >> 2] >> (24 - 8 * (b & 3))) & 0xffu; }

// a * b mod x^16 + x^15 + x^2 + 1 over GF(2).
__device__ inline uint32_t flac_mul16(uint32_t a, uint32_t b) {
  uint32_t out = 0;
  for (int bit = 15; bit >= 0; --bit) {
    out = ((out << 1) ^ ((out & 0x8000u) ? 0x18005u : 0u)) & 0xffffu;
    if ((b >> bit) & 1u) out ^= a;
  }
  return out;
}

// grid (blocks of the longest job, jobs).
__global__ __launch_bounds__(kFlacThreads) void k_flac_frame(const float* __restrict__ x, const int* __restrict__ tab,
                                                             const FlacJob* __restrict__ jobs,
                                                             uint8_t* __restrict__ slots, uint32_t* __restrict__ lens) {
  __shared__ int s_s[kFlacMaxB];                      // the block's samples
  __shared__ uint32_t s_S[((2 << kFlacMaxPo) - 1) * kFlacRow];  // the Rice sums of every partition order: order o
                                                      // at rows [2^o - 1, 2^(o+1) - 1); before the search the
                                                      // windowed samples, after it the winner's residuals
  __shared__ uint32_t s_buf[kFlacFrameWords];
  __shared__ uint32_t s_tot[kFlacMaxPo + 1];
  __shared__ unsigned long long s_R[kFlacMaxLpc + 1];
  __shared__ double s_a[kFlacMaxLpc], s_t[kFlacMaxLpc];
  __shared__ int s_c[kFlacMaxLpc * kFlacMaxLpc], s_shift[kFlacMaxLpc], s_valid[kFlacMaxLpc];
  __shared__ int s_varies, s_best_cand, s_best_o;
  __shared__ uint32_t s_best_bits, s_scan[kFlacThreads], s_total_bits, s_crc;
  __shared__ uint8_t s_k[1 << kFlacMaxPo];

  const FlacJob job = jobs[blockIdx.y];
  if ((int64_t)blockIdx.x >= job.nblocks) return;  // (uniform over the workgroup)
  const int tid = threadIdx.x;
  const int B = job.B;
  const int64_t first = (int64_t)blockIdx.x * B;
  const int n = (int)min((int64_t)B, job.n - first);
  const uint32_t frame_no = job.first_frame + blockIdx.x;

  // ---- quantise; zero the frame buffer
  for (int i = tid; i < n; i += kFlacThreads) {
    const float v = fminf(fmaxf(__fmul_rn(x[job.in_off + first + i], job.scale), -1.0f), 1.0f);
    s_s[i] = (int)__fmul_rn(v, 32767.0f);
  }
  for (int w = tid; w < kFlacFrameWords; w += kFlacThreads) s_buf[w] = 0;
  if (tid < kFlacMaxLpc) s_valid[tid] = 0;
  if (tid == 0) {
    s_varies = 0;
    s_best_cand = -1;  // VERBATIM
    s_best_o = 0;
    s_best_bits = 8u + 16u * (uint32_t)n;
    s_crc = 0;
  }
  __syncthreads();
  {
    const int s0 = s_s[0];
    bool varies = false;
    for (int i = tid; i < n; i += kFlacThreads) varies |= s_s[i] != s0;
    if (varies) s_varies = 1;
  }
  __syncthreads();
  const bool constant = s_varies == 0;

  // ---- LPC: windowed autocorrelation in int64, Levinson-Durbin in f64 on lane 0
  if (!constant && job.lpc && n >= 2) {
    int* v = (int*)s_S;
    for (int i = tid; i < n; i += kFlacThreads) {
      const int w = n == B ? tab[job.tab_off + i] : flac_window_q15(i, n);
      v[i] = (s_s[i] * w) >> 10;  // |s w| < 2^30
    }
    if (tid <= kFlacMaxLpc) s_R[tid] = 0;
    __syncthreads();
    const int m = min(kFlacMaxLpc, n - 1);
    for (int l = 0; l <= m; ++l) {
      long long acc = 0;
      for (int i = tid; i < n; i += kFlacThreads)
        if (i >= l) acc += (long long)v[i] * (long long)v[i - l];
      atomicAdd(&s_R[l], (unsigned long long)acc);
    }
    __syncthreads();
    if (tid == 0) {
      double E = (double)(long long)s_R[0];  // |R| <= 2^52: exact
      for (int i = 0; i < m; ++i) {
        if (!(E > 0.0)) break;
        double acc = (double)(long long)s_R[i + 1];
        for (int j = 0; j < i; ++j) acc = __dsub_rn(acc, __dmul_rn(s_a[j], (double)(long long)s_R[i - j]));
        const double k = __ddiv_rn(acc, E);
        for (int j = 0; j < i; ++j) s_t[j] = __dsub_rn(s_a[j], __dmul_rn(k, s_a[i - 1 - j]));
        for (int j = 0; j < i; ++j) s_a[j] = s_t[j];
        s_a[i] = k;
        E = __dmul_rn(E, __dsub_rn(1.0, __dmul_rn(k, k)));
        bool ok = true;
        double cmax = 0.0;
        for (int j = 0; j <= i; ++j) {
          const double f = fabs(s_a[j]);
          if (!(f < HUGE_VAL)) ok = false;  // (an infinity or a NaN)
          if (f > cmax) cmax = f;
        }
        if (!ok || !(cmax > 0.0)) continue;
        const int e = (int)((__double_as_longlong(cmax) >> 52) & 0x7ff) - 1022;  // 2^(e-1) <= cmax < 2^e
        const int shift = min(kFlacPrecision - 1 - e, 15);  // (a subnormal cmax: far above 15 either way)
        if (shift < 0) continue;
        const double scale = (double)(1 << shift);
        for (int j = 0; j <= i; ++j)
          s_c[i * kFlacMaxLpc + j] = (int)fmin(fmax(rint(__dmul_rn(s_a[j], scale)), -2048.0), 2047.0);
        s_shift[i] = shift;
        s_valid[i] = 1;
      }
    }
    __syncthreads();
  }

  // ---- the search: every candidate's exact size at every partition order
  const int of = min(kFlacMaxPo, __ffs(n) - 1);  // the finest partition order: 2^of divides n
  if (!constant) {
    for (int cand = 0; cand < kFlacCands; ++cand) {
      const int order = flac_order(cand);
      if (order >= n || (cand >= 5 && !s_valid[order - 1])) continue;  // (uniform)
      const int* coef = s_c + (cand >= 5 ? (order - 1) * kFlacMaxLpc : 0);
      const int shift = cand >= 5 ? s_shift[order - 1] : 0;
      uint32_t* fine = s_S + ((1 << of) - 1) * kFlacRow;
      for (int e = tid; e < (kFlacRow << of); e += kFlacThreads) fine[e] = 0;
      if (tid <= kFlacMaxPo) s_tot[tid] = 0;
      __syncthreads();
      flac_accumulate(s_s, n, cand, order, coef, shift, n >> of, fine, tid);
      __syncthreads();
      for (int o = of; o >= 0; --o) {
        if (tid < (1 << o)) {
          uint32_t* row = s_S + ((1 << o) - 1 + tid) * kFlacRow;
          if (o < of) {
            const uint32_t* child = s_S + ((2 << o) - 1 + 2 * tid) * kFlacRow;
            for (int k = 0; k <= kFlacMaxK; ++k) row[k] = child[k] + child[kFlacRow + k];
          }
          const uint32_t cnt = (uint32_t)((n >> o) - (tid == 0 ? order : 0));  // (an order past omax: unused)
          uint32_t best = 0xffffffffu;
          for (int k = 0; k <= kFlacMaxK; ++k) best = min(best, row[k] + (uint32_t)(k + 1) * cnt);
          atomicAdd(&s_tot[o], 4u + best);
        }
        __syncthreads();
      }
      if (tid == 0) {
        int omax = 0;
        while (omax < of && (n >> (omax + 1)) > order) ++omax;
        int bo = 0;
        for (int o = 1; o <= omax; ++o)
          if (s_tot[o] < s_tot[bo]) bo = o;
        const uint32_t bits = 8u + 16u * order + 6u + s_tot[bo] + (cand >= 5 ? 9u + (uint32_t)kFlacPrecision * order : 0u);
        if (bits < s_best_bits) s_best_bits = bits, s_best_cand = cand, s_best_o = bo;
      }
      __syncthreads();
    }
  }
  const int cand = constant ? -2 : s_best_cand;
  const int order = cand >= 0 ? flac_order(cand) : 0;
  const int po = s_best_o;
  const int plen = n >> po;
  const int* coef = s_c + (cand >= 5 ? (order - 1) * kFlacMaxLpc : 0);
  const int shift = cand >= 5 ? s_shift[order - 1] : 0;
  int* res = (int*)s_S;
  if (cand >= 0) {  // the winner's Rice parameters, then its residuals
    for (int e = tid; e < (kFlacRow << po); e += kFlacThreads) s_S[e] = 0;
    __syncthreads();
    flac_accumulate(s_s, n, cand, order, coef, shift, plen, s_S, tid);
    __syncthreads();
    if (tid < (1 << po)) {
      const uint32_t cnt = (uint32_t)(plen - (tid == 0 ? order : 0));
      uint32_t best = 0xffffffffu;
      int bk = 0;
      for (int k = 0; k <= kFlacMaxK; ++k) {
        const uint32_t b = s_S[tid * kFlacRow + k] + (uint32_t)(k + 1) * cnt;
        if (b < best) best = b, bk = k;
      }
      s_k[tid] = (uint8_t)bk;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kFlacThreads)
      if (i >= order) res[i] = flac_residual(s_s, i, cand, coef, shift);
    __syncthreads();
  }

  // ---- the frame: header and subframe header on lane 0, samples on every lane
  const int bs_code = n == B ? job.bs_code : (n <= 256 ? 6 : 7);
  const int hdr_len = 4 + flac_utf8_len(frame_no) + (bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0) + 1;
  const uint32_t sub0 = 8u * hdr_len;  // the subframe's first bit
  const uint32_t res0 = sub0 + 8u + 16u * order + (cand >= 5 ? 9u + (uint32_t)kFlacPrecision * order : 0u) + 6u;
  if (tid == 0) {
    uint8_t h[16];
    int len = 0;
    h[len++] = 0xff;
    h[len++] = 0xf8;
    h[len++] = (uint8_t)((bs_code << 4) | job.rate_code);
    h[len++] = 0x08;  // mono, 16 bits
    const int ul = flac_utf8_len(frame_no);
    if (ul == 1) {
      h[len++] = (uint8_t)frame_no;
    } else {
      h[len++] = (uint8_t)(((0xff << (8 - ul)) & 0xff) | (frame_no >> (6 * (ul - 1))));
      for (int j = ul - 2; j >= 0; --j) h[len++] = (uint8_t)(0x80u | ((frame_no >> (6 * j)) & 0x3fu));
    }
    if (bs_code == 6) h[len++] = (uint8_t)(n - 1);
    if (bs_code == 7) h[len++] = (uint8_t)((n - 1) >> 8), h[len++] = (uint8_t)((n - 1) & 0xff);
    uint32_t c = 0;
    for (int j = 0; j < len; ++j) {
      c ^= h[j];
      for (int b = 0; b < 8; ++b) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xffu : (c << 1) & 0xffu;
    }
    h[len++] = (uint8_t)c;
    for (int j = 0; j < len; ++j) flac_put(s_buf, 8u * j, h[j], 8);
    uint32_t pos = sub0;
    if (cand == -2) {
      flac_put(s_buf, pos, 0x00u, 8);
      flac_put(s_buf, pos + 8, (uint32_t)s_s[0] & 0xffffu, 16);
      s_total_bits = pos + 24;
    } else if (cand == -1) {
      flac_put(s_buf, pos, 0x02u, 8);
      s_total_bits = pos + 8 + 16u * n;
    } else {
      flac_put(s_buf, pos, cand < 5 ? (uint32_t)((8 | order) << 1) : (uint32_t)((32 | (order - 1)) << 1), 8);
      pos += 8;
      for (int j = 0; j < order; ++j, pos += 16) flac_put(s_buf, pos, (uint32_t)s_s[j] & 0xffffu, 16);
      if (cand >= 5) {
        flac_put(s_buf, pos, (uint32_t)(kFlacPrecision - 1), 4);
        flac_put(s_buf, pos + 4, (uint32_t)shift, 5);
        pos += 9;
        for (int j = 0; j < order; ++j, pos += kFlacPrecision)
          flac_put(s_buf, pos, (uint32_t)coef[j] & ((1u << kFlacPrecision) - 1), kFlacPrecision);
      }
      flac_put(s_buf, pos + 2, (uint32_t)po, 4);  // (coding method 00 before it)
    }
  }
  if (cand == -1) {
    for (int i = tid; i < n; i += kFlacThreads) flac_put(s_buf, sub0 + 8u + 16u * i, (uint32_t)s_s[i] & 0xffffu, 16);
  } else if (cand >= 0) {
    // lane t holds samples [t c, (t + 1) c): the lengths of its codes, a prefix sum, then the bits. A
    // partition's first code carries the partition's 4-bit parameter in front.
    const int c = (n + kFlacThreads - 1) / kFlacThreads;
    const int i0 = max(tid * c, order), i1 = min((tid + 1) * c, n);
    uint32_t mine = 0;
    for (int i = i0; i < i1; ++i) {
      const int p = i / plen, k = s_k[p];
      mine += (i == (p == 0 ? order : p * plen) ? 4u : 0u) + (flac_zigzag(res[i]) >> k) + 1u + (uint32_t)k;
    }
    s_scan[tid] = mine;
    __syncthreads();
    if (tid == 0) {
      uint32_t run = 0;
      for (int t = 0; t < kFlacThreads; ++t) {
        const uint32_t l = s_scan[t];
        s_scan[t] = run;
        run += l;
      }
      s_total_bits = res0 + run;
    }
    __syncthreads();
    uint32_t pos = res0 + s_scan[tid];
    for (int i = i0; i < i1; ++i) {
      const int p = i / plen, k = s_k[p];
      if (i == (p == 0 ? order : p * plen)) {
        flac_put(s_buf, pos, (uint32_t)k, 4);
        pos += 4;
      }
      const uint32_t zz = flac_zigzag(res[i]);
      pos += zz >> k;  // the unary zeros are in the buffer already
      flac_put(s_buf, pos, (1u << k) | (zz & ((1u << k) - 1)), k + 1);
      pos += (uint32_t)k + 1;
    }
  }
  __syncthreads();

  // ---- CRC-16 (initial value 0: linear), a slice per lane, then out
  const int stride = 2 * B + 16;
  const int nbytes = min((int)((s_total_bits + 7) >> 3), 2 * n + 14);  // (never the bound: the winner is no larger than VERBATIM)
  {
    const int sl = (nbytes + kFlacThreads - 1) / kFlacThreads;
    const int b0 = tid * sl, b1 = min(b0 + sl, nbytes);
    if (b0 < b1) {
      uint32_t c = 0;
      for (int b = b0; b < b1; ++b) {
        c ^= flac_byte(s_buf, b) << 8;
        for (int j = 0; j < 8; ++j) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xffffu : (c << 1) & 0xffffu;
      }
      uint32_t xp = 1, base = 0x0100u;  // x^(8 (nbytes - b1)) by square and multiply
      for (int mrem = nbytes - b1; mrem > 0; mrem >>= 1) {
        if (mrem & 1) xp = flac_mul16(xp, base);
        base = flac_mul16(base, base);
      }
      atomicXor(&s_crc, flac_mul16(c, xp));
    }
  }
  __syncthreads();
  if (tid == 0) flac_put(s_buf, 8u * nbytes, s_crc, 16);
  __syncthreads();
  const int len = nbytes + 2;
  uint32_t* out = (uint32_t*)(slots + job.slot_off + (int64_t)blockIdx.x * stride);  // (4-byte aligned: stride is)
  for (int w = tid; w < (len + 3) / 4; w += kFlacThreads) out[w] = __builtin_bswap32(s_buf[w]);
  if (tid == 0) lens[job.len_off + blockIdx.x] = (uint32_t)len;
}

// grid (tiles of 256 frames of the longest job, jobs): the lengths before the tile summed, the tile's
// own scanned, then a wave per frame copies.
__global__ __launch_bounds__(kFlacThreads) void k_flac_pack(const uint8_t* __restrict__ slots,
                                                            const uint32_t* __restrict__ lens,
                                                            const FlacJob* __restrict__ jobs, uint8_t* __restrict__ out,
                                                            FlacRes* __restrict__ results) {
  __shared__ unsigned long long s_pre, s_off[kFlacThreads];
  __shared__ uint32_t s_min, s_max, s_len[kFlacThreads];
  const FlacJob job = jobs[blockIdx.y];
  const int64_t tile0 = (int64_t)blockIdx.x * kFlacThreads;
  if (tile0 >= job.nblocks) return;  // (uniform)
  const int tid = threadIdx.x;
  if (tid == 0) s_pre = 0, s_min = 0xffffffffu, s_max = 0;
  __syncthreads();
  unsigned long long sum = 0;
  uint32_t mn = 0xffffffffu, mx = 0;
  for (int64_t f = tid; f < tile0; f += kFlacThreads) {
    const uint32_t l = lens[job.len_off + f];
    sum += l, mn = min(mn, l), mx = max(mx, l);
  }
  const uint32_t own = tile0 + tid < job.nblocks ? lens[job.len_off + tile0 + tid] : 0u;
  if (tile0 + tid < job.nblocks) mn = min(mn, own), mx = max(mx, own);
  s_len[tid] = own;
  atomicAdd(&s_pre, sum);
  atomicMin(&s_min, mn);
  atomicMax(&s_max, mx);
  __syncthreads();
  if (tid == 0) {
    unsigned long long off = s_pre;
    for (int t = 0; t < kFlacThreads; ++t) {
      s_off[t] = off;
      off += s_len[t];
    }
    if (tile0 + kFlacThreads >= job.nblocks) results[blockIdx.y] = FlacRes{off, s_min, s_max};
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const int64_t stride = 2 * (int64_t)job.B + 16;
  for (int t = wave; t < kFlacThreads && tile0 + t < job.nblocks; t += kFlacThreads / 64) {
    const uint8_t* src = slots + job.slot_off + (tile0 + t) * stride;
    uint8_t* dst = out + job.out_off + s_off[t];
    for (uint32_t b = lane; b < s_len[t]; b += 64) dst[b] = src[b];
  }
}

// ---- host ----------------------------------------------------------------------------------------
static int flac_rate_code(int rate) {
  switch (rate) {
    case 8000: return 4;
    case 16000: return 5;
    case 22050: return 6;
    case 24000: return 7;
    case 32000: return 8;
    case 44100: return 9;
    case 48000: return 10;
    default: return -1;
  }
}

// 256 -> 0 .. 4096 -> 4 (the header code is 8 + this); anything else -1.
static int flac_block_index(int64_t B) {
  for (int i = 0; i < 5; ++i)
    if (B == (256 << i)) return i;
  return -1;
}

static void flac_make_table(int32_t* out) {
  for (int b = 0; b < 5; ++b) {
    const int B = 256 << b;
    for (int i = 0; i < B; ++i) *out++ = flac_window_q15(i, B);
  }
}

struct FlacWin {
  const float* in;
  int64_t n_in, out_count;  // out_count: the window's blocks (stage_upload's "takes part")
  float scale;
  int rate_code, bidx, B, lpc;
  uint32_t first_frame;
  rwkvtts_flac_window* pub;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_flac : Stage<FlacJob, uint8_t, int32_t> {  // d_table: the five windows, 256 first
  DevBuf<uint8_t> d_slots;
  DevBuf<uint32_t> d_lens;
  DevBuf<FlacRes> d_res;
  std::vector<FlacRes> res;
};

extern "C" int rwkvtts_flac_table(int32_t block_size, int32_t* out) {
  RT_CHECK(flac_block_index(block_size) >= 0 && out, RWKVTTS_EINVAL,
           "flac_table: block_size must be 256, 512, 1024, 2048 or 4096, and out not null");
  for (int i = 0; i < block_size; ++i) out[i] = flac_window_q15(i, block_size);
  return RWKVTTS_OK;
}

extern "C" int64_t rwkvtts_flac_bound(int64_t n, int32_t block_size) {
  if (n < 0 || n > ((int64_t)1 << 40) || flac_block_index(block_size) < 0) return -1;
  return 2 * n + 16 * ((n + block_size - 1) / block_size);
}

extern "C" int rwkvtts_flac_streaminfo(int32_t sample_rate, int32_t block_size, int32_t min_frame, int32_t max_frame,
                                       int64_t total_samples, const uint8_t* md5, uint8_t* out) {
  RT_CHECK(out && flac_rate_code(sample_rate) >= 0 && flac_block_index(block_size) >= 0 && min_frame >= 0 &&
               max_frame >= min_frame && max_frame < (1 << 24) && total_samples >= 0 &&
               total_samples < ((int64_t)1 << 36),
           RWKVTTS_EINVAL, "flac_streaminfo: bad rate, block size, frame sizes or sample count");
  uint8_t* p = out;
  memcpy(p, "fLaC", 4), p += 4;
  *p++ = 0x80, *p++ = 0, *p++ = 0, *p++ = 34;  // the last metadata block, STREAMINFO, 34 bytes
  for (int rep = 0; rep < 2; ++rep) *p++ = (uint8_t)(block_size >> 8), *p++ = (uint8_t)block_size;
  for (int32_t v : {min_frame, max_frame}) *p++ = (uint8_t)(v >> 16), *p++ = (uint8_t)(v >> 8), *p++ = (uint8_t)v;
  const uint64_t v = ((uint64_t)sample_rate << 44) | ((uint64_t)15 << 36) | (uint64_t)total_samples;  // mono, 16 bits
  for (int b = 7; b >= 0; --b) *p++ = (uint8_t)(v >> (8 * b));
  if (md5)
    memcpy(p, md5, 16);
  else
    memset(p, 0, 16);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_flac_create(int device, const int32_t* table, rwkvtts_flac** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "flac_create: null output");
  *out = nullptr;
  rwkvtts_flac* v = nullptr;
  int rc = stage_create("flac_create", device, table, (size_t)kFlacTable, [&](int32_t* t) { flac_make_table(t); }, &v);
  if (rc) return rc;
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_flac_destroy(rwkvtts_flac* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  stage_free(v, {v->d_slots.p, v->d_lens.p, v->d_res.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_flac_kernel_ms(rwkvtts_flac* v, double* ms) { return stage_kernel_ms("flac_kernel_ms", v, ms); }

extern "C" int rwkvtts_flac_encode(rwkvtts_flac* v, rwkvtts_flac_window* w, int n) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "flac_encode: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("flac_encode", [&] {
    std::vector<FlacWin> ws;
    int rc = read_windows("flac_encode", w, n, ws, [](rwkvtts_flac_window* wi) {
      FlacWin f;
      f.in = wi->in, f.n_in = wi->n_in, f.scale = wi->scale;
      f.rate_code = flac_rate_code(wi->sample_rate), f.bidx = flac_block_index(wi->block_size), f.B = wi->block_size;
      f.lpc = (wi->flags & RWKVTTS_FLAC_NO_LPC) ? 0 : 1;
      f.first_frame = 0, f.out_count = 0, f.pub = wi;
      return f;
    });
    if (rc) return rc;
    // every window is checked before anything is launched or written
    int64_t tot_in = 0, tot_slots = 0, tot_blocks = 0, tot_out = 0, max_blocks = 0;
    size_t n_jobs = 0;
    for (FlacWin& f : ws) {
      const rwkvtts_flac_window* wi = f.pub;
      RT_CHECK(f.rate_code >= 0, RWKVTTS_EINVAL, "flac_encode: sample_rate is not one of the seven output rates");
      RT_CHECK(f.bidx >= 0, RWKVTTS_EINVAL, "flac_encode: block_size must be 256, 512, 1024, 2048 or 4096");
      RT_CHECK(f.n_in >= 0 && f.n_in <= ((int64_t)1 << 40) && (f.in || f.n_in == 0), RWKVTTS_EINVAL,
               "flac_encode: n_in out of range or null input");
      RT_CHECK(f.scale >= 0.0f && f.scale <= 3.4028234e38f, RWKVTTS_EINVAL,
               "flac_encode: scale must be finite and not negative");  // (NaN fails)
      RT_CHECK((wi->flags & RWKVTTS_FLAC_LAST) || f.n_in % f.B == 0, RWKVTTS_EINVAL,
               "flac_encode: a window that does not end the signal must hold whole blocks");
      const int64_t blocks = (f.n_in + f.B - 1) / f.B;
      RT_CHECK(wi->first_frame >= 0 && wi->first_frame + blocks <= ((int64_t)1 << 31), RWKVTTS_EINVAL,
               "flac_encode: first_frame + blocks passes 2^31");
      const int64_t cap = 2 * f.n_in + 16 * blocks;
      RT_CHECK(wi->out_cap >= cap && (wi->out || cap == 0), RWKVTTS_EINVAL,
               "flac_encode: out_cap is below rwkvtts_flac_bound (or out is null)");
      f.first_frame = (uint32_t)wi->first_frame;
      f.out_count = blocks;
      if (blocks == 0) continue;
      tot_in += f.n_in, tot_slots += blocks * (2 * (int64_t)f.B + 16), tot_blocks += blocks, tot_out += cap;
      max_blocks = std::max(max_blocks, blocks);
      ++n_jobs;
    }
    for (FlacWin& f : ws) f.pub->out_len = 0, f.pub->min_frame = 0, f.pub->max_frame = 0;
    if (n_jobs == 0) return RWKVTTS_OK;
    RT_CHECK(n_jobs <= 65535 && max_blocks <= 0x7fffffff, RWKVTTS_EINVAL, "flac_encode: too much for one launch");
    std::lock_guard<std::mutex> lock(v->mu);
    v->desc.clear();
    int64_t in_off = 0, slot_off = 0, len_off = 0, out_off = 0;
    for (const FlacWin& f : ws) {
      if (f.out_count == 0) continue;
      FlacJob j;
      j.in_off = in_off, j.n = f.n_in, j.slot_off = slot_off, j.len_off = len_off, j.out_off = out_off;
      j.nblocks = f.out_count, j.first_frame = f.first_frame;
      j.B = f.B, j.bs_code = 8 + f.bidx, j.rate_code = f.rate_code, j.tab_off = (256 << f.bidx) - 256, j.lpc = f.lpc;
      j.scale = f.scale;
      v->desc.push_back(j);
      in_off += f.n_in, slot_off += f.out_count * (2 * (int64_t)f.B + 16), len_off += f.out_count;
      out_off += 2 * f.n_in + 16 * f.out_count;
    }
    if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_slots.reserve((size_t)tot_slots)) ||
        (rc = v->d_lens.reserve((size_t)tot_blocks)) || (rc = v->d_res.reserve(n_jobs)) || (rc = stage_upload(v, ws)))
      return rc;
    hipExtLaunchKernelGGL(k_flac_frame, dim3((unsigned)max_blocks, (unsigned)n_jobs), dim3(kFlacThreads), 0, v->stream,
                          v->ev0, nullptr, 0u, v->d_in.p, v->d_table, v->d_desc.p, v->d_slots.p, v->d_lens.p);
    RT_HIP(hipGetLastError());
    const unsigned tiles = (unsigned)((max_blocks + kFlacThreads - 1) / kFlacThreads);
    hipExtLaunchKernelGGL(k_flac_pack, dim3(tiles, (unsigned)n_jobs), dim3(kFlacThreads), 0, v->stream, nullptr, v->ev1,
                          0u, v->d_slots.p, v->d_lens.p, v->d_desc.p, v->d_out.p, v->d_res.p);
    RT_HIP(hipGetLastError());
    v->res.assign(n_jobs, FlacRes{0, 0, 0});
    RT_HIP(hipMemcpyAsync(v->res.data(), v->d_res.p, n_jobs * sizeof(FlacRes), hipMemcpyDeviceToHost, v->stream));
    RT_HIP(hipStreamSynchronize(v->stream));  // the lengths first: only the packed bytes are copied
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, v->ev0, v->ev1) == hipSuccess) v->kernel_ms = (double)ms;
    size_t k = 0;
    for (const FlacWin& f : ws) {
      if (f.out_count == 0) continue;
      const FlacRes& r = v->res[k];
      const int64_t cap = 2 * f.n_in + 16 * f.out_count;
      RT_CHECK((int64_t)r.total <= cap, RWKVTTS_EHIP, "flac_encode: the packed length passes the bound");
      RT_HIP(hipMemcpyAsync(f.pub->out, v->d_out.p + v->desc[k].out_off, (size_t)r.total, hipMemcpyDeviceToHost,
                            v->stream));
      ++k;
    }
    RT_HIP(hipStreamSynchronize(v->stream));
    k = 0;
    for (const FlacWin& f : ws) {
      if (f.out_count == 0) continue;
      const FlacRes& r = v->res[k++];
      f.pub->out_len = (int64_t)r.total, f.pub->min_frame = (int32_t)r.min_frame, f.pub->max_frame = (int32_t)r.max_frame;
    }
    return RWKVTTS_OK;
  });
}
