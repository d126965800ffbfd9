// Labelled support sets, fp32, one build: a prototype bank that is filled once (ragged classes, any number of calls) and scored many times.
//  * proto_bank_accumulate: sum [way][D] += the support rows of each class, count [way] += their number, invalid += labels outside [0, way).
//    One workgroup per (class, 256-wide D slice) scans the label array: a class's rows are added in ascending support index on top of the
//    stored sum whatever the launch geometry - no floating-point atomics, bit-reproducible.
//  * proto_bank_finalize: proto = sum / count ('sqr', 'dot') and F.normalize of it with the 1e-12 clamp ('cos', meta_baseline.py:37-38);
//    empty [way] = 1 and a zero prototype where count == 0.  One wave per class.
//  * proto_bank_logits: utils.compute_logits (utils/__init__.py:78-101) of query [Q][D] against proto [way][D] as a tiled GEMM: a workgroup owns
//    64 queries and walks the class axis in tiles of 64, both operands staged through LDS in 32-wide K chunks, 4 x 4 outputs per thread in
//    registers (fp32 FMA; 'sqr' accumulates (q - p)^2 itself, the expanded |q|^2 + |p|^2 - 2 q.p form cancels).  A prototype element is read
//    from L2 / HBM once per query tile.  Optional pred [Q] = the first maximum of the row; an empty class scores -inf.
//  * proto_auc: the --sauc reduction (meta_tuning_sun_m/test_few_shot.py:95-112): per episode, cosine scores of the queries against the single
//    prototype of class 0 and their ROC-AUC as the pair count (#{pos > neg} + #{pos == neg} / 2) / (n_pos n_neg).  One workgroup per episode.
#include "fsvit_common.h"
#include "kernels.h"

namespace fsvit {

constexpr int PB_SLICE = 256;      // D elements per accumulate workgroup (one per thread)

template <typename L>
__global__ __launch_bounds__(PB_SLICE) void proto_bank_accumulate_kernel(const float* __restrict__ feat, const L* __restrict__ label, int S, int way, int D,
                                                                         float* __restrict__ sum, int* __restrict__ count, int* __restrict__ invalid) {
  __shared__ int n_class, n_bad;
  const int c = blockIdx.x, t = threadIdx.x, d = blockIdx.y * PB_SLICE + t;
  if (blockIdx.y == 0) {           // the class's count (and, in the workgroup of class 0, the labels no class takes): integer sums, any order
    if (t == 0) { n_class = 0; n_bad = 0; }
    __syncthreads();
    int mine = 0, bad = 0;
    for (int s = t; s < S; s += PB_SLICE) {
      const L l = label[s];
      mine += (l == (L)c);
      bad += (l < (L)0 || l >= (L)way);
    }
    if (mine) atomicAdd(&n_class, mine);
    if (bad && c == 0) atomicAdd(&n_bad, bad);
    __syncthreads();
    if (t == 0) {
      count[c] += n_class;
      if (c == 0 && n_bad) atomicAdd(invalid, n_bad);
    }
  }
  if (d >= D) return;
  float acc = sum[(size_t)c * D + d];
  for (int s = 0; s < S; ++s)
    if (label[s] == (L)c) acc += feat[(size_t)s * D + d];
  sum[(size_t)c * D + d] = acc;
}

int launch_proto_bank_accumulate(const float* feat, const void* label, int label_is_int64, int S, int way, int D, float* sum, int* count, int* invalid,
                                 hipStream_t s) {
  if (S <= 0) return 0;
  if (way < 1 || D < 1) return (int)hipErrorInvalidValue;
  const dim3 grid(way, (D + PB_SLICE - 1) / PB_SLICE);
  if (label_is_int64)
    hipLaunchKernelGGL(proto_bank_accumulate_kernel<long long>, grid, dim3(PB_SLICE), 0, s, feat, (const long long*)label, S, way, D, sum, count, invalid);
  else
    hipLaunchKernelGGL(proto_bank_accumulate_kernel<int>, grid, dim3(PB_SLICE), 0, s, feat, (const int*)label, S, way, D, sum, count, invalid);
  return (int)hipGetLastError();
}

__global__ __launch_bounds__(256) void proto_bank_finalize_kernel(const float* __restrict__ sum, const int* __restrict__ count, int way, int D, int method,
                                                                  float* __restrict__ proto, int* __restrict__ empty) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= way) return;
  const int n = count[c];
  const float* srow = sum + (size_t)c * D;
  float* prow = proto + (size_t)c * D;
  if (lane == 0) empty[c] = n <= 0;
  if (n <= 0) {
    for (int d = lane; d < D; d += 64) prow[d] = 0.f;
    return;
  }
  const float fn = (float)n;
  float inv = 1.0f;
  if (method == 0) {                                           // F.normalize(mean), eps 1e-12
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) { const float m = srow[d] / fn; ss += m * m; }
    inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  }
  for (int d = lane; d < D; d += 64) {
    const float m = srow[d] / fn;
    prow[d] = method == 0 ? m * inv : m;
  }
}

int launch_proto_bank_finalize(const float* sum, const int* count, int way, int D, int method, float* proto, int* empty, hipStream_t s) {
  if (way < 1 || D < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(proto_bank_finalize_kernel, dim3((way + 3) / 4), dim3(256), 0, s, sum, count, way, D, method, proto, empty);
  return (int)hipGetLastError();
}

// ---- logits: 64 x 64 output tile per step, K chunks of 32 through LDS, stored k-major so that a thread reads its 4 rows as one 16-byte word
constexpr int PB_TM = 64, PB_TN = 64, PB_KC = 32, PB_LD = 68;      // PB_LD: row pitch in floats (16-byte aligned, 4 banks off the 64-bank period)

// rows [row0, row0 + 64) x k [k0, k0 + 32) of a row-major [R][D] matrix -> tile[k][row]; rows >= R and k >= D read as zero (D % 4 == 0)
__device__ __forceinline__ void pb_stage(const float* __restrict__ src, int R, int D, int row0, int k0, float* __restrict__ tile, int t) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int r = p * 32 + (t >> 3), k = (t & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + r < R && k0 + k < D) v = *reinterpret_cast<const float4*>(src + (size_t)(row0 + r) * D + k0 + k);
    tile[(k + 0) * PB_LD + r] = v.x;
    tile[(k + 1) * PB_LD + r] = v.y;
    tile[(k + 2) * PB_LD + r] = v.z;
    tile[(k + 3) * PB_LD + r] = v.w;
  }
}

template <int METHOD>
__global__ __launch_bounds__(256) void proto_bank_logits_kernel(const float* __restrict__ query, const float* __restrict__ proto, const int* __restrict__ empty,
                                                                int Q, int way, int D, float temp, const float* __restrict__ temp_dev,
                                                                float* __restrict__ logits, int* __restrict__ pred) {
  __shared__ __attribute__((aligned(16))) float qs[PB_KC * PB_LD];
  __shared__ __attribute__((aligned(16))) float ps[PB_KC * PB_LD];
  __shared__ float qinv[PB_TM];
  if (temp_dev) temp = *temp_dev;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tx = t & 15, ty = t >> 4;                          // classes tx * 4 .. + 3, queries ty * 4 .. + 3 of the tile
  const int q0 = blockIdx.x * PB_TM;
  if (METHOD == 0) {                                           // F.normalize(query): 1 / max(|q|, 1e-12), one wave per row
    for (int r = wave; r < PB_TM; r += 4) {
      float ss = 0.f;
      if (q0 + r < Q) {
        const float* x = query + (size_t)(q0 + r) * D;
        for (int d = lane; d < D; d += 64) ss += x[d] * x[d];
      }
      ss = wave_sum(ss);
      if (lane == 0) qinv[r] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    }
    __syncthreads();
  }
  float best[4];
  int arg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { best[i] = -INFINITY; arg[i] = 0; }
  for (int c0 = 0; c0 < way; c0 += PB_TN) {
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < D; k0 += PB_KC) {
      __syncthreads();                                         // the previous chunk's reads are done
      pb_stage(query, Q, D, q0, k0, qs, t);
      pb_stage(proto, way, D, c0, k0, ps, t);
      __syncthreads();
#pragma unroll 8
      for (int k = 0; k < PB_KC; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(qs + k * PB_LD + ty * 4);
        const float4 b = *reinterpret_cast<const float4*>(ps + k * PB_LD + tx * 4);
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (METHOD == 1) { const float df = av[i] - bv[j]; acc[i][j] = fmaf(df, df, acc[i][j]); }
            else acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
          }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = q0 + ty * 4 + i;
      if (q >= Q) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + tx * 4 + j;
        if (c >= way) continue;
        float l = METHOD == 0 ? acc[i][j] * qinv[ty * 4 + i] * temp : (METHOD == 1 ? -acc[i][j] * temp : acc[i][j] * temp);
        if (empty && empty[c]) l = -INFINITY;
        logits[(size_t)q * way + c] = l;
        if (l > best[i]) { best[i] = l; arg[i] = c; }          // classes ascend within a thread: the first maximum of its own columns
      }
    }
  }
  if (pred) {                                                  // across the 16 threads of a row (lanes that differ in their low 4 bits): larger value, then lower index
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ob = __shfl_xor(best[i], o, 64);
        const int oa = __shfl_xor(arg[i], o, 64);
        if (ob > best[i] || (ob == best[i] && oa < arg[i])) { best[i] = ob; arg[i] = oa; }
      }
      const int q = q0 + ty * 4 + i;
      if (tx == 0 && q < Q) pred[q] = arg[i];
    }
  }
}

int launch_proto_bank_logits(const float* query, const float* proto, const int* empty, int Q, int way, int D, float temp, const float* temp_dev, int method,
                             float* logits, int* pred, hipStream_t s) {
  if (Q <= 0) return 0;
  if (way < 1 || D < 4 || D % 4 || method < 0 || method > 2) return (int)hipErrorInvalidValue;
  const dim3 grid((Q + PB_TM - 1) / PB_TM), block(256);
  if (method == 0) hipLaunchKernelGGL(proto_bank_logits_kernel<0>, grid, block, 0, s, query, proto, empty, Q, way, D, temp, temp_dev, logits, pred);
  else if (method == 1) hipLaunchKernelGGL(proto_bank_logits_kernel<1>, grid, block, 0, s, query, proto, empty, Q, way, D, temp, temp_dev, logits, pred);
  else hipLaunchKernelGGL(proto_bank_logits_kernel<2>, grid, block, 0, s, query, proto, empty, Q, way, D, temp, temp_dev, logits, pred);
  return (int)hipGetLastError();
}

// ---- --sauc: LDS = proto [D] | score [Q]
__global__ __launch_bounds__(256) void proto_auc_kernel(const float* __restrict__ feat_shot, const float* __restrict__ feat_query, int shot, int Q, int D,
                                                        float* __restrict__ auc, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int pairs2;                                       // 2 #{pos > neg} + #{pos == neg}
  float* proto = reinterpret_cast<float*>(smem);               // [D]
  float* sc = proto + D;                                       // [Q]
  const int e = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* fs = feat_shot + (size_t)e * shot * D;
  const float* fq = feat_query + (size_t)e * Q * D;
  if (t == 0) pairs2 = 0;
  for (int d = t; d < D; d += 256) {
    float s = 0.f;
    for (int k = 0; k < shot; ++k) s += fs[(size_t)k * D + d];
    proto[d] = s / (float)shot;
  }
  __syncthreads();
  float ss = 0.f;                                              // every wave forms the same |proto|^2 in the same order
  for (int d = lane; d < D; d += 64) ss += proto[d] * proto[d];
  const float pinv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  for (int q = wave; q < Q; q += 4) {
    const float* x = fq + (size_t)q * D;
    float qq = 0.f, qp = 0.f;
    for (int d = lane; d < D; d += 64) { qq += x[d] * x[d]; qp += x[d] * (proto[d] * pinv); }
    const float v = wave_sum(qp) * (1.0f / fmaxf(sqrtf(wave_sum(qq)), 1e-12f));
    if (lane == 0) {
      sc[q] = v;
      if (score) score[(size_t)e * Q + q] = v;
    }
  }
  __syncthreads();
  const int k = Q / 2;
  int mine = 0;
  for (int i = t; i < k * k; i += 256) {
    const float p = sc[i / k], n = sc[k + i % k];
    mine += p > n ? 2 : (p == n ? 1 : 0);
  }
  if (mine) atomicAdd(&pairs2, mine);
  __syncthreads();
  if (t == 0) auc[e] = (float)pairs2 / (2.0f * (float)k * (float)k);
}

int launch_proto_auc(const float* feat_shot, const float* feat_query, int E, int shot, int Q, int D, float* auc, float* score, hipStream_t s) {
  if (E <= 0) return 0;
  // Q <= 4096: the pair count 2 (Q / 2)^2 stays below 2^24, exact in fp32; with D <= 8192 the LDS is at most 48 KB
  if (shot < 1 || Q < 2 || Q % 2 || Q > 4096 || D < 1 || D > 8192) return (int)hipErrorInvalidValue;
  const size_t lds = ((size_t)D + Q) * sizeof(float);
  hipLaunchKernelGGL(proto_auc_kernel, dim3(E), dim3(256), lds, s, feat_shot, feat_query, shot, Q, D, auc, score);
  return (int)hipGetLastError();
}

}  // namespace fsvit
