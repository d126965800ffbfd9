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
//  * proto_bank_topk: the K <= 32 best classes of every row of that matrix (the order of a stable descending sort), their logits and the row's
//    log-sum-exp, without writing the matrix: the same tile body on a (query tile, class split) grid over segments of 1024 classes, a row's running
//    list in the 16 lanes that own the row, one (max, sum) pair per row and segment, then one wave per row merges the splits.  Bits do not depend on the split.
//  * proto_auc: the --sauc reduction (meta_tuning_sun_m/test_few_shot.py:95-112): per episode, cosine scores of the queries against the single
//    prototype of class 0 and their ROC-AUC as the pair count (#{pos > neg} + #{pos == neg} / 2) / (n_pos n_neg).  One workgroup per episode.
//  * proto_auc_gather: the same reduction over rows of a feature table [N][D] addressed by slot numbers (feature_table.py: every image is encoded
//    once); one device body serves both kernels.
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

// 1 / max(|q|, 1e-12) of the workgroup's 64 query rows ('cos': F.normalize(query)), one wave per row; ends in a barrier
__device__ __forceinline__ void pb_query_inv_norm(const float* __restrict__ query, int Q, int D, int q0, float* __restrict__ qinv, int lane, int wave) {
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

// The tile body of proto_bank_logits and proto_bank_topk: l[i][j] = the logit of query q0 + ty * 4 + i against class c0 + tx * 4 + j (t = ty * 16 + tx),
// one serial fmaf chain over D per output and the method's epilogue; -inf for an empty class.  Entries with q >= Q or c >= way hold no result.
template <int METHOD>
__device__ __forceinline__ void pb_tile_logits(const float* __restrict__ query, const float* __restrict__ proto, const int* __restrict__ empty, int Q, int way,
                                               int D, int q0, int c0, float temp, float* __restrict__ qs, float* __restrict__ ps,
                                               const float* __restrict__ qinv, int t, float (&l)[4][4]) {
  const int tx = t & 15, ty = t >> 4;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int k0 = 0; k0 < D; k0 += PB_KC) {
    __syncthreads();                                           // the previous chunk's reads are done
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
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + tx * 4 + j;
    const bool none = empty && c < way && empty[c];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = METHOD == 0 ? acc[i][j] * qinv[ty * 4 + i] * temp : (METHOD == 1 ? -acc[i][j] * temp : acc[i][j] * temp);
      l[i][j] = none ? -INFINITY : v;
    }
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
  if (METHOD == 0) pb_query_inv_norm(query, Q, D, q0, qinv, lane, wave);
  float best[4];
  int arg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { best[i] = -INFINITY; arg[i] = 0; }
  for (int c0 = 0; c0 < way; c0 += PB_TN) {
    float l[4][4];
    pb_tile_logits<METHOD>(query, proto, empty, Q, way, D, q0, c0, temp, qs, ps, qinv, t, l);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = q0 + ty * 4 + i;
      if (q >= Q) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + tx * 4 + j;
        if (c >= way) continue;
        logits[(size_t)q * way + c] = l[i][j];
        if (l[i][j] > best[i]) { best[i] = l[i][j]; arg[i] = c; }      // classes ascend within a thread: the first maximum of its own columns
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

// ---- top-k + log-sum-exp of every row without the [Q][way] matrix: the partial kernel on a (query tile, class split) grid, then a merge per row.
// Order of two (logit, class) entries everywhere below: the larger logit first, then the lower class - the order of a stable descending sort of the row.
constexpr int PB_SEG = 1024;             // classes per segment: the unit a split is made of, and the unit of the log-sum-exp chain
constexpr int PB_KMAX = 32;              // list length limit: a row's list lives in the 16 lanes of the row, two slots each
constexpr int PB_NONE = 0x7fffffff;      // class of a slot that holds nothing; with logit -inf it loses against every class, an empty one (-inf, c) included
constexpr int PB_MERGE_ROWS = 2;         // rows (waves) per merge workgroup: at most 2 * 64 * 32 * 8 bytes = 32 KB of LDS

__device__ __forceinline__ bool pb_better(float v, int c, float w, int d) { return v > w || (v == w && c < d); }

// (m, s) <- (m, s) + (om, os) where a pair stands for m + log(s); (-inf, 0) is the empty sum and no step forms inf - inf
__device__ __forceinline__ void pb_lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  if (nm == -INFINITY) return;
  s = s * expf(m - nm) + os * expf(om - nm);
  m = nm;
}

// Workspace (floats / ints, 4 bytes each): part_val [n_split][Q][K] | part_idx [n_split][Q][K] | seg_pair [Q][n_seg][2]
template <int METHOD>
__global__ __launch_bounds__(256) void proto_bank_topk_partial_kernel(const float* __restrict__ query, const float* __restrict__ proto, const int* __restrict__ empty,
                                                                      int Q, int way, int D, float temp, const float* __restrict__ temp_dev, int K, int n_seg,
                                                                      float* __restrict__ part_val, int* __restrict__ part_idx, float* __restrict__ seg_pair) {
  __shared__ __attribute__((aligned(16))) float qs[PB_KC * PB_LD];
  __shared__ __attribute__((aligned(16))) float ps[PB_KC * PB_LD];
  __shared__ float qinv[PB_TM];
  if (temp_dev) temp = *temp_dev;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tx = t & 15, ty = t >> 4;
  const int q0 = blockIdx.x * PB_TM;
  const int split = blockIdx.y, n_split = gridDim.y;
  const int seg_lo = split * n_seg / n_split, seg_hi = (split + 1) * n_seg / n_split;      // whole segments, every split at least one (n_split <= n_seg)
  if (METHOD == 0) pb_query_inv_norm(query, Q, D, q0, qinv, lane, wave);
  // Row ty * 4 + i belongs to the 16 lanes of one wave that share ty: its list is sorted, slot p in lane p & 15 (e0: p < 16, e1: p >= 16), and
  // (kv, kc) is a copy of slot K - 1 in all 16 lanes.  Nothing of it is in memory, so no wave ever waits for another outside the tile body.
  float e0v[4], e1v[4], kv[4];
  int e0c[4], e1c[4], kc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e0v[i] = e1v[i] = kv[i] = -INFINITY;
    e0c[i] = e1c[i] = kc[i] = PB_NONE;
  }
  const int k_lane = (K - 1) & 15, k_slot = (K - 1) >> 4;
  const int n_ins = K < PB_TN ? K : PB_TN;
  for (int seg = seg_lo; seg < seg_hi; ++seg) {
    float m[4], s[4];                                          // this thread's classes of the segment, ascending: fixed by the position in the segment alone
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] = -INFINITY; s[i] = 0.f; }
    const int c_end = (seg + 1) * PB_SEG < way ? (seg + 1) * PB_SEG : way;
    for (int c0 = seg * PB_SEG; c0 < c_end; c0 += PB_TN) {
      float l[4][4];
      pb_tile_logits<METHOD>(query, proto, empty, Q, way, D, q0, c0, temp, qs, ps, qinv, t, l);
      int cls[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + tx * 4 + j;
        cls[j] = c < way ? c : PB_NONE;
        if (c >= way) {
#pragma unroll
          for (int i = 0; i < 4; ++i) l[i][j] = -INFINITY;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float tm = fmaxf(fmaxf(l[i][0], l[i][1]), fmaxf(l[i][2], l[i][3]));
        if (tm > m[i]) { s[i] *= expf(m[i] - tm); m[i] = tm; }
        if (m[i] > -INFINITY) {
#pragma unroll
          for (int j = 0; j < 4; ++j) s[i] += expf(l[i][j] - m[i]);      // an empty class adds exp(-inf) = 0
        }
        const bool live = q0 + ty * 4 + i < Q;
        float cv[4];
        int ci[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { cv[j] = live ? l[i][j] : -INFINITY; ci[j] = live ? cls[j] : PB_NONE; }
        for (int n = 0; n < n_ins; ++n) {                      // each pass inserts the best entry left in the tile; after K of them the rest cannot enter
          float bv = -INFINITY;
          int bc = PB_NONE;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (pb_better(cv[j], ci[j], bv, bc)) { bv = cv[j]; bc = ci[j]; }
          if (!__any(pb_better(bv, bc, kv[i], kc[i]))) break;  // no row of this wave has an entry that beats its K-th: the common case
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            if (pb_better(ov, oc, bv, bc)) { bv = ov; bc = oc; }
          }
          const bool ins = pb_better(bv, bc, kv[i], kc[i]);    // the same in the 16 lanes of the row
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (ins && ci[j] == bc) { cv[j] = -INFINITY; ci[j] = PB_NONE; }
          // slot p keeps its entry if that is better than the new one, takes the new one if slot p - 1 is better than it, else takes slot p - 1's
          const float p0v = __shfl_up(e0v[i], 1, 16), w1v = __shfl_up(e1v[i], 1, 16), w0v = __shfl(e0v[i], 15, 16);
          const int p0c = __shfl_up(e0c[i], 1, 16), w1c = __shfl_up(e1c[i], 1, 16), w0c = __shfl(e0c[i], 15, 16);
          const float p1v = tx == 0 ? w0v : w1v;
          const int p1c = tx == 0 ? w0c : w1c;
          if (ins && !pb_better(e0v[i], e0c[i], bv, bc)) {
            const bool here = tx == 0 || pb_better(p0v, p0c, bv, bc);
            e0v[i] = here ? bv : p0v;
            e0c[i] = here ? bc : p0c;
          }
          if (ins && !pb_better(e1v[i], e1c[i], bv, bc)) {
            const bool here = pb_better(p1v, p1c, bv, bc);
            e1v[i] = here ? bv : p1v;
            e1c[i] = here ? bc : p1c;
          }
          kv[i] = __shfl(k_slot ? e1v[i] : e0v[i], k_lane, 16);
          kc[i] = __shfl(k_slot ? e1c[i] : e0c[i], k_lane, 16);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {                              // the 16 lanes of the row, a fixed tree; lane tx == 0 holds the segment's pair
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float om = __shfl_xor(m[i], o, 64), os = __shfl_xor(s[i], o, 64);
        pb_lse_merge(m[i], s[i], om, os);
      }
      const int q = q0 + ty * 4 + i;
      if (tx == 0 && q < Q) {
        seg_pair[((size_t)q * n_seg + seg) * 2 + 0] = m[i];
        seg_pair[((size_t)q * n_seg + seg) * 2 + 1] = s[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = q0 + ty * 4 + i;
    if (q >= Q) continue;
    const size_t base = ((size_t)split * Q + q) * K;
    if (tx < K) { part_val[base + tx] = e0v[i]; part_idx[base + tx] = e0c[i]; }
    if (tx + 16 < K) { part_val[base + tx + 16] = e1v[i]; part_idx[base + tx + 16] = e1c[i]; }
  }
}

// One wave per row: lane j walks the sorted list of split j (n_split <= 64), K times the best head of all lists is taken; the segment pairs are folded
// in ascending segment order.  LDS: val [rows][n_split * K] | idx [rows][n_split * K].
__global__ __launch_bounds__(64 * PB_MERGE_ROWS) void proto_bank_topk_merge_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                                                   const float* __restrict__ seg_pair, int Q, int K, int n_split, int n_seg,
                                                                                   float* __restrict__ values, int* __restrict__ indices, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = blockIdx.x * PB_MERGE_ROWS + wave;
  const int n = n_split * K;
  float* lv = reinterpret_cast<float*>(smem) + wave * n;
  int* lc = reinterpret_cast<int*>(smem) + PB_MERGE_ROWS * n + wave * n;
  if (q < Q)
    for (int e = lane; e < n; e += 64) {
      const size_t src = ((size_t)(e / K) * Q + q) * K + e % K;
      lv[e] = part_val[src];
      lc[e] = part_idx[src];
    }
  __syncthreads();
  if (q >= Q) return;
  int head = 0;
  for (int r = 0; r < K; ++r) {
    float v = -INFINITY;
    int c = PB_NONE;
    if (lane < n_split && head < K) { v = lv[lane * K + head]; c = lc[lane * K + head]; }
    float bv = v;
    int bc = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oc = __shfl_xor(bc, o, 64);
      if (pb_better(ov, oc, bv, bc)) { bv = ov; bc = oc; }
    }
    if (c == bc && bc != PB_NONE) ++head;                      // the splits hold disjoint classes: one lane advances
    if (lane == 0) {
      values[(size_t)q * K + r] = bv;
      indices[(size_t)q * K + r] = bc == PB_NONE ? -1 : bc;    // a rank beyond `way`: (-inf, -1)
    }
  }
  if (lse) {
    float pm = -INFINITY, psum = 0.f;
    if (lane < n_seg) { pm = seg_pair[((size_t)q * n_seg + lane) * 2]; psum = seg_pair[((size_t)q * n_seg + lane) * 2 + 1]; }
    float m = -INFINITY, s = 0.f;
    for (int g = 0; g < n_seg; ++g) pb_lse_merge(m, s, __shfl(pm, g, 64), __shfl(psum, g, 64));
    if (lane == 0) lse[q] = m == -INFINITY ? -INFINITY : m + logf(s);
  }
}

size_t proto_bank_topk_workspace_bytes(int Q, int way, int K, int n_split) {
  const size_t n_seg = ((size_t)way + PB_SEG - 1) / PB_SEG;
  return ((size_t)n_split * Q * K * 2 + (size_t)Q * n_seg * 2) * sizeof(float);
}

int launch_proto_bank_topk(const float* query, const float* proto, const int* empty, int Q, int way, int D, float temp, const float* temp_dev, int method, int K,
                           int n_split, float* values, int* indices, float* lse, void* ws, hipStream_t s) {
  if (Q <= 0) return 0;
  const int n_seg = (way + PB_SEG - 1) / PB_SEG;
  if (way < 1 || D < 4 || D % 4 || method < 0 || method > 2 || K < 1 || K > PB_KMAX || n_split < 1 || n_split > n_seg || n_seg > 64 || !ws)
    return (int)hipErrorInvalidValue;
  float* part_val = static_cast<float*>(ws);
  int* part_idx = reinterpret_cast<int*>(part_val + (size_t)n_split * Q * K);
  float* seg_pair = part_val + (size_t)n_split * Q * K * 2;
  const dim3 grid((Q + PB_TM - 1) / PB_TM, n_split), block(256);
  if (method == 0)
    hipLaunchKernelGGL(proto_bank_topk_partial_kernel<0>, grid, block, 0, s, query, proto, empty, Q, way, D, temp, temp_dev, K, n_seg, part_val, part_idx, seg_pair);
  else if (method == 1)
    hipLaunchKernelGGL(proto_bank_topk_partial_kernel<1>, grid, block, 0, s, query, proto, empty, Q, way, D, temp, temp_dev, K, n_seg, part_val, part_idx, seg_pair);
  else
    hipLaunchKernelGGL(proto_bank_topk_partial_kernel<2>, grid, block, 0, s, query, proto, empty, Q, way, D, temp, temp_dev, K, n_seg, part_val, part_idx, seg_pair);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  const size_t lds = (size_t)PB_MERGE_ROWS * n_split * K * (sizeof(float) + sizeof(int));
  hipLaunchKernelGGL(proto_bank_topk_merge_kernel, dim3((Q + PB_MERGE_ROWS - 1) / PB_MERGE_ROWS), dim3(64 * PB_MERGE_ROWS), lds, s, part_val, part_idx, seg_pair,
                     Q, K, n_split, n_seg, values, indices, lse);
  return (int)hipGetLastError();
}

// ---- --sauc: LDS = proto [D] | score [Q]
// The arithmetic of one episode, shared by the two kernels below: shot_row(k) / query_row(q) give the address of a feature row [D] of episode blockIdx.x -
// contiguous rows in proto_auc_kernel, rows of a feature table in proto_auc_gather_kernel; everything after the address is the same instruction
// sequence, so the two kernels give the same bits for the same rows.  smem: [D] + [Q] floats; pairs2: one int of LDS, 2 #{pos > neg} + #{pos == neg}.
template <typename ShotRow, typename QueryRow>
__device__ __forceinline__ void proto_auc_body(ShotRow shot_row, QueryRow query_row, unsigned char* smem, int* pairs2, int shot, int Q, int D,
                                               float* __restrict__ auc, float* __restrict__ score) {
  float* proto = reinterpret_cast<float*>(smem);               // [D]
  float* sc = proto + D;                                       // [Q]
  const int e = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) *pairs2 = 0;
  for (int d = t; d < D; d += 256) {
    float s = 0.f;
    for (int k = 0; k < shot; ++k) s += shot_row(k)[d];
    proto[d] = s / (float)shot;
  }
  __syncthreads();
  float ss = 0.f;                                              // every wave forms the same |proto|^2 in the same order
  for (int d = lane; d < D; d += 64) ss += proto[d] * proto[d];
  const float pinv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  for (int q = wave; q < Q; q += 4) {
    const float* x = query_row(q);
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
  if (mine) atomicAdd(pairs2, mine);
  __syncthreads();
  if (t == 0) auc[e] = (float)*pairs2 / (2.0f * (float)k * (float)k);
}

__global__ __launch_bounds__(256) void proto_auc_kernel(const float* __restrict__ feat_shot, const float* __restrict__ feat_query, int shot, int Q, int D,
                                                        float* __restrict__ auc, float* __restrict__ score) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int pairs2;
  const float* fs = feat_shot + (size_t)blockIdx.x * shot * D;
  const float* fq = feat_query + (size_t)blockIdx.x * Q * D;
  proto_auc_body([=](int k) { return fs + (size_t)k * D; }, [=](int q) { return fq + (size_t)q * D; }, smem, &pairs2, shot, Q, D, auc, score);
}

// The same reduction over rows gathered from a feature table [N][D]: shot_slots [E][shot] (the shots of class 0), query_slots [E][Q] (positives first).
// A slot outside [0, N) never becomes an address: its row is read from slot 0, *invalid is raised by one per such entry (integer adds, any order) and
// the episode's auc and score are written as NaN.
template <typename L>
__global__ __launch_bounds__(256) void proto_auc_gather_kernel(const float* __restrict__ table, const L* __restrict__ shot_slots,
                                                               const L* __restrict__ query_slots, int N, int shot, int Q, int D, float* __restrict__ auc,
                                                               float* __restrict__ score, int* __restrict__ invalid) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int pairs2, n_bad;
  const int e = blockIdx.x, t = threadIdx.x;
  const L* es = shot_slots + (size_t)e * shot;
  const L* eq = query_slots + (size_t)e * Q;
  if (t == 0) n_bad = 0;
  __syncthreads();
  int mine = 0;
  for (int i = t; i < shot; i += 256) mine += (es[i] < (L)0 || es[i] >= (L)N);
  for (int i = t; i < Q; i += 256) mine += (eq[i] < (L)0 || eq[i] >= (L)N);
  if (mine) atomicAdd(&n_bad, mine);
  __syncthreads();
  const int bad = n_bad;
  auto row = [=](const L* slots, int i) {
    const L s = slots[i];
    return table + (size_t)((s < (L)0 || s >= (L)N) ? (L)0 : s) * D;
  };
  proto_auc_body([=](int k) { return row(es, k); }, [=](int q) { return row(eq, q); }, smem, &pairs2, shot, Q, D, auc, score);
  if (!bad) return;                                            // (uniform over the workgroup)
  __syncthreads();                                             // the body's own stores to this episode's outputs come first
  const float nan = __builtin_nanf("");
  if (score)
    for (int i = t; i < Q; i += 256) score[(size_t)e * Q + i] = nan;
  if (t == 0) {
    auc[e] = nan;
    atomicAdd(invalid, bad);
  }
}

// Q <= 4096: the pair count 2 (Q / 2)^2 stays below 2^24, exact in fp32; with D <= 8192 the LDS is at most 48 KB
static bool proto_auc_dims(int shot, int Q, int D) { return shot >= 1 && Q >= 2 && Q % 2 == 0 && Q <= 4096 && D >= 1 && D <= 8192; }

int launch_proto_auc(const float* feat_shot, const float* feat_query, int E, int shot, int Q, int D, float* auc, float* score, hipStream_t s) {
  if (E <= 0) return 0;
  if (!proto_auc_dims(shot, Q, D)) return (int)hipErrorInvalidValue;
  const size_t lds = ((size_t)D + Q) * sizeof(float);
  hipLaunchKernelGGL(proto_auc_kernel, dim3(E), dim3(256), lds, s, feat_shot, feat_query, shot, Q, D, auc, score);
  return (int)hipGetLastError();
}

int launch_proto_auc_gather(const float* table, int N, int D, const void* shot_slots, const void* query_slots, int idx_is_int64, int E, int shot, int Q,
                            float* auc, float* score, int* invalid, hipStream_t s) {
  if (E <= 0) return 0;
  if (N < 1 || !proto_auc_dims(shot, Q, D)) return (int)hipErrorInvalidValue;
  const size_t lds = ((size_t)D + Q) * sizeof(float);
  if (idx_is_int64)
    hipLaunchKernelGGL(proto_auc_gather_kernel<long long>, dim3(E), dim3(256), lds, s, table, (const long long*)shot_slots, (const long long*)query_slots, N,
                       shot, Q, D, auc, score, invalid);
  else
    hipLaunchKernelGGL(proto_auc_gather_kernel<int>, dim3(E), dim3(256), lds, s, table, (const int*)shot_slots, (const int*)query_slots, N, shot, Q, D, auc,
                       score, invalid);
  return (int)hipGetLastError();
}

}  // namespace fsvit
