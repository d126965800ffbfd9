// DeepEMD head (meta_tuning_sun_d/Models/models/Network.py:48-175, emd_utils.py:65-76): a query is scored against a class by the earth mover's
// distance between the token maps of the two images.  fp32 throughout, in every numerics mode (the token map arrives as fp32).
//  * emd_prep_kernel: per token the channel mean, the centred vector (normalize_feature 'center', :143-146) scaled by 1 / max(|x|, 1e-8)
//    (F.cosine_similarity's clamp: a constant token gives similarity 0), and per image the token mean of the UN-centred map
//    (adaptive_avg_pool2d in get_weight_vector, which runs before the centring, :70-74).
//  * emd_pair_kernel: one wavefront per (query, proto) problem, four problems per workgroup.  Cost c = 1 - cosine similarity [query node][proto node]
//    (:151-167) and both weight vectors (:48-65, emd_utils.py:69-73) are formed in registers / LDS, the transportation problem is solved exactly in
//    place, and logit = temperature / N * sum (1 - c) F (:118-124).  The similarity map never reaches HBM.
//  * emd_gather_kernel: the same problems (emd_pair_wave) over rows of a token-map table addressed by slot numbers (feature_table.TokenTable: every
//    image is encoded and prepared once, fsvit_emd_table_prep); the class side is a table row (1-shot) or a dense per-episode map (the 5-shot SFC).
//  * emd_solve_wave: successive shortest augmenting paths with node potentials, one lane per node (rows on lanes 0 .. N-1, columns on lanes 32 .. 32+N-1),
//    from a starting dual (column minima) and a greedy starting flow on its tight arcs.
//    Every loop has a static bound (augmentations <= 8 N, Dijkstra steps <= 2 N + 1, path trace <= N + 1); a problem that reaches one writes status 1
//    and stops.  No block barrier anywhere: the waves of a workgroup run problems of different lengths.
//  * emd_bwd_kernel: flows are constants (the reference's `solver: opencv` semantics, :118-120): dS = dlogit * temperature / N * F.  One workgroup per
//    image looping over its partners, no atomics, deterministic.
//  * emd_sfc_kernel: the 5-shot SFC fine-tune (get_sfc, :83-107) as one on-device loop, one workgroup per episode: per mini-batch update the SFC's
//    nodes, the problems of the mini-batch (emd_pair_wave, the body emd_pair_kernel runs too), dlogits, the backward onto the SFC and the momentum
//    update, separated by block barriers that every wave reaches.  Opt-in (DeepEMD(sfc_fused=True)); the default route calls the kernels above.
//  * emd_bank_accumulate_kernel / emd_bank_finalize_kernel / emd_rerank_kernel: a labelled support set (models/emd_bank.TokenBank).  Per class the sum
//    of its support maps and their count; from them the class map, its prepared nodes (emd_prep_token / emd_prep_pooled) and a unit-length token mean for
//    a cosine shortlist; then per query only the shortlisted (query, class) problems (emd_pair_wave), ranked in the launch that solves them.
#include "fsvit_common.h"
#include "kernels.h"
#include "../../include/fsvit.h"

namespace fsvit {

constexpr int EMD_PITCH = 33;                      // N + 1 at N = 32: row scans and column scans of c / F are both bank-conflict free
constexpr int EMD_TILE = 32 * EMD_PITCH;
constexpr int EMD_WAVES = 4;
constexpr float EMD_SNAP = 1e-6f;                  // residual supply / demand / reverse flow below this is zero
constexpr float EMD_INF = 3.0e38f;

// Wave-wide minimum of non-negative keys on the DPP network (no LDS crossbar round trips: this sits on the critical path of every Dijkstra step):
// prefix minimum inside each row of 16 (row_shr 1, 2, 4, 8), lane 15 of rows 0 / 2 into rows 1 / 3 (row_bcast15), lane 31 into rows 2 / 3
// (row_bcast31); lane 63 then holds the minimum.  Lanes a step does not reach keep EMD_INF as the incoming value.
// (The keys are non-negative floats, never -0: their bit patterns order like unsigned integers, and the unsigned minimum with its identity as the
// incoming value folds into one v_min_u32 with a DPP operand per step.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned emd_dpp_min(unsigned v) {
  const unsigned in = (unsigned)__builtin_amdgcn_update_dpp((int)0xffffffffu, (int)v, CTRL, ROW_MASK, 0xf, false);
  return v < in ? v : in;
}
__device__ __forceinline__ float emd_lane_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ int emd_lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }      // l is wave-uniform at every call
__device__ __forceinline__ float emd_wave_min(float key) {
  unsigned v = __builtin_bit_cast(unsigned, key);
  v = emd_dpp_min<0x111, 0xf>(v);
  v = emd_dpp_min<0x112, 0xf>(v);
  v = emd_dpp_min<0x114, 0xf>(v);
  v = emd_dpp_min<0x118, 0xf>(v);
  v = emd_dpp_min<0x142, 0xa>(v);
  v = emd_dpp_min<0x143, 0xc>(v);
  return __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_readlane((int)v, 63));
}

// c, F: this wave's [32][EMD_PITCH] tiles in LDS (c zero outside N x N, F all zero); rem: this lane's supply (row lanes) or demand (column lanes).
// Returns the status; F holds the optimal flow.  Potentials: reduced cost of the forward arc i -> j is c_ij + pu_i - pv_j, of the reverse arc
// j -> i (present where F_ij > 0) its negative; both are clamped at 0 against fp32 rounding.
__device__ __forceinline__ int emd_solve_wave(const float* c, float* F, const int N, float rem, const int lane, int* naug_out) {
  const bool is_row = lane < 32;
  const int me = lane & 31;
  const bool valid = me < N;
  if (!valid) rem = 0.f;
  float pot = 0.f;
  int status = 0, it = 0;
  const int max_aug = 8 * N;
  // Starting dual and flow: pv_j = min_i c_ij keeps every forward arc at a non-negative reduced cost and the arcs that attain the minimum at 0; each
  // column in turn then hands its demand to its cheapest row while that row has supply left.  Flow sits only on arcs of reduced cost 0, which is all the
  // searches below need; N short uniform steps save about a third of them.
  {
    float cmin = EMD_INF;
    int arg = 0;
    for (int i = 0; i < N; ++i) {
      const float v = c[i * EMD_PITCH + me];
      if (v < cmin) { cmin = v; arg = i; }
    }
    if (!is_row && valid) pot = cmin;
    for (int j = 0; j < N; ++j) {
      const int r = emd_lane_i(arg, 32 + j) & 31;
      const float d = fminf(emd_lane_f(rem, r), emd_lane_f(rem, 32 + j));
      if (d > 0.f) {
        if (lane == 0) F[r * EMD_PITCH + j] = d;
        if (lane == r || lane == 32 + j) {
          const float x = rem - d;
          rem = x < EMD_SNAP ? 0.f : x;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  for (; it < max_aug; ++it) {
    const unsigned long long src_mask = __ballot(is_row && rem > 0.f);
    const unsigned long long dem_mask = __ballot(!is_row && rem > 0.f);
    if (!src_mask || !dem_mask) break;
    // multi-source Dijkstra from the rows with supply left, until the first column with demand left
    float dist = (is_row && rem > 0.f) ? 0.f : EMD_INF;
    bool vis = false;
    int par = -1, tgt = -1;
    float D = 0.f;
    for (int step = 0; step <= 2 * N; ++step) {
      const float key = (valid && !vis) ? dist : EMD_INF;
      const float dmin = emd_wave_min(key);
      if (!(dmin < EMD_INF)) break;
      const unsigned long long ties = __ballot(key == dmin);
      const unsigned long long hit = ties & dem_mask;
      if (hit) { tgt = __ffsll((long long)hit) - 1 - 32; D = dmin; break; }
      if (!ties) break;                                       // (a NaN key: cannot happen with finite costs; never index with ffs(0) - 1)
      const int u = __ffsll((long long)ties) - 1;
      if (lane == u) vis = true;
      const bool urow = u < 32;
      const int ui = u & 31;
      const float pu = emd_lane_f(pot, u);
      const int idx = urow ? ui * EMD_PITCH + me : me * EMD_PITCH + ui;      // < EMD_TILE for every lane
      const float cv = c[idx], fv = F[idx];
      const float rc = fmaxf((urow ? cv : -cv) + pu - pot, 0.f);
      const float nd = dmin + rc;
      const bool can = valid && !vis && (is_row != urow) && (urow || fv > 0.f);
      if (can && nd < dist) { dist = nd; par = ui; }
    }
    if (tgt < 0) { status = 1; break; }
    tgt &= 31;
    if (vis) pot += dist - D;
    // bottleneck along the path: demand left at the target, reverse flows, supply left at the source
    int cur = tgt, src = -1;
    float delta = emd_lane_f(rem, 32 + tgt);
    for (int k = 0; k <= N; ++k) {
      const int i = emd_lane_i(par, 32 + cur) & 31;
      const int pj = emd_lane_i(par, i);
      if (pj < 0) { src = i; delta = fminf(delta, emd_lane_f(rem, i)); break; }
      delta = fminf(delta, F[i * EMD_PITCH + (pj & 31)]);
      cur = pj & 31;
    }
    if (src < 0 || !(delta > 0.f)) { status = 1; break; }
    cur = tgt;
    for (int k = 0; k <= N; ++k) {
      const int i = emd_lane_i(par, 32 + cur) & 31;
      const int pj = emd_lane_i(par, i);
      if (lane == 0) F[i * EMD_PITCH + cur] += delta;
      if (pj < 0) break;
      if (lane == 0) {
        const float f = F[i * EMD_PITCH + (pj & 31)] - delta;
        F[i * EMD_PITCH + (pj & 31)] = f < EMD_SNAP ? 0.f : f;
      }
      cur = pj & 31;
    }
    if (lane == src || lane == 32 + tgt) {
      const float r = rem - delta;
      rem = r < EMD_SNAP ? 0.f : r;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // lane 0's flow updates before the next search reads them
  }
  if (status == 0) {
    const bool more = __ballot(is_row && rem > 0.f) != 0ull && __ballot(!is_row && rem > 0.f) != 0ull;
    if (it >= max_aug && more) status = 1;                     // augmentation bound
    float left = rem;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) left = fmaxf(left, __shfl_xor(left, o, 64));
    if (left > 1e-3f) status = 1;                              // supply without demand (or the reverse): the weight sums differ
  }
  if (naug_out && lane == 0) *naug_out = it;
  return status;
}

__global__ __launch_bounds__(64 * EMD_WAVES) void emd_solve_kernel(const float* __restrict__ cost, const float* __restrict__ w1, const float* __restrict__ w2,
                                                                   int B, int N, float* __restrict__ flow, int* __restrict__ status, int* __restrict__ naug) {
  __shared__ float lds[EMD_WAVES][2][EMD_TILE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * EMD_WAVES + wave;
  if (b >= B) return;
  float* c = lds[wave][0];
  float* F = lds[wave][1];
  const float* cb = cost + (size_t)b * N * N;
  for (int idx = lane; idx < EMD_TILE; idx += 64) {
    const int a = idx / EMD_PITCH, bb = idx - a * EMD_PITCH;
    c[idx] = (a < N && bb < N) ? cb[a * N + bb] : 0.f;
    F[idx] = 0.f;
  }
  const int me = lane & 31;
  float rem = 0.f;
  if (me < N) rem = lane < 32 ? w1[(size_t)b * N + me] : w2[(size_t)b * N + me];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const int st = emd_solve_wave(c, F, N, rem, lane, naug ? naug + b : nullptr);
  float* fb = flow + (size_t)b * N * N;
  for (int idx = lane; idx < EMD_TILE; idx += 64) {
    const int a = idx / EMD_PITCH, bb = idx - a * EMD_PITCH;
    if (a < N && bb < N) fb[a * N + bb] = F[idx];
  }
  if (lane == 0) status[b] = st;
}

// One token on one wave: x [C] -> xh [C] = (x - channel mean) / max(|x - mean|, 1e-8); returns the inverse norm.
__device__ __forceinline__ float emd_prep_token(const float* x, float* xh, const int C, const int lane) {
  float s = 0.f;
  for (int k = lane; k < C; k += 64) s += x[k];
  const float mean = wave_sum(s) / (float)C;
  float ss = 0.f;
  for (int k = lane; k < C; k += 64) { const float d = x[k] - mean; ss += d * d; }
  const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-8f);
  for (int k = lane; k < C; k += 64) xh[k] = (x[k] - mean) * inv;
  return inv;
}
// Channel k of the token mean of the un-centred map x [N][C]
__device__ __forceinline__ float emd_prep_pooled(const float* x, const int N, const int C, const int k) {
  float s = 0.f;
  for (int n = 0; n < N; ++n) s += x[n * C + k];
  return s / (float)N;
}

// tok [n_img][N][C] -> xhat [n_img][N][C], pooled [n_img][C], rn [n_img][N] (rn may be null: only the backward reads it)
__global__ __launch_bounds__(256) void emd_prep_kernel(const float* __restrict__ shot_tok, const float* __restrict__ query_tok, int n_shot, int N, int C,
                                                       float* __restrict__ xhat, float* __restrict__ pooled, float* __restrict__ rn) {
  const int img = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* x = img < n_shot ? shot_tok + (size_t)img * N * C : query_tok + (size_t)(img - n_shot) * N * C;
  float* xh = xhat + (size_t)img * N * C;
  for (int n = wave; n < N; n += 4) {
    const float inv = emd_prep_token(x + n * C, xh + n * C, C, lane);
    if (rn && lane == 0) rn[(size_t)img * N + n] = inv;
  }
  for (int k = threadIdx.x; k < C; k += 256) pooled[(size_t)img * C + k] = emd_prep_pooled(x, N, C, k);
}

// One (query image, proto image) problem on one wave.  tq / tp: the token maps [N][C], xq / xp: their prepared nodes, gq / gp: their token means [C];
// c, F: this wave's LDS tiles.  Builds the cost tile and both weight vectors, solves, and returns sum (1 - c) F (the logit before its scale); F holds the
// flow, st the solver's status.
__device__ __forceinline__ float emd_pair_wave(const float* tq, const float* tp, const float* xq, const float* xp, const float* gq, const float* gp,
                                               const int N, const int C, float* c, float* F, const int lane, int& st) {
  for (int idx = lane; idx < EMD_TILE; idx += 64) F[idx] = 0.f;
  if (lane < 32) c[lane * EMD_PITCH + 32] = 0.f;
  // c[a][b] = 1 - <xhat_q[a], xhat_p[b]>: lane (la, lb) of an 8 x 8 grid owns a = la + 8 r, b = lb + 8 s
  {
    const int la = lane >> 3, lb = lane & 7;
    const float *qa[4], *pb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      qa[r] = xq + (size_t)min(la + 8 * r, N - 1) * C;
      pb[r] = xp + (size_t)min(lb + 8 * r, N - 1) * C;
    }
    float acc[4][4] = {};
    for (int k = 0; k < C; k += 4) {
      f32x4 va[4], vb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        va[r] = *reinterpret_cast<const f32x4*>(qa[r] + k);
        vb[r] = *reinterpret_cast<const f32x4*>(pb[r] + k);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          acc[r][s] += va[r][0] * vb[s][0] + va[r][1] * vb[s][1] + va[r][2] * vb[s][2] + va[r][3] * vb[s][3];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int a = la + 8 * r, b = lb + 8 * s;
        c[a * EMD_PITCH + b] = (a < N && b < N) ? 1.0f - acc[r][s] : 0.f;
      }
  }
  // weights: w1[a] = relu(<query token a, pooled proto>) + 1e-3 on the row lanes, w2[b] = relu(<proto token b, pooled query>) + 1e-3 on the column lanes
  const int me = lane & 31;
  const bool is_row = lane < 32, valid = me < N;
  float w = 0.f;
  for (int n = 0; n < N; ++n) {
    float s1 = 0.f, s2 = 0.f;
    for (int k = lane * 4; k < C; k += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(tq + (size_t)n * C + k), g = *reinterpret_cast<const f32x4*>(gp + k);
      const f32x4 b = *reinterpret_cast<const f32x4*>(tp + (size_t)n * C + k), h = *reinterpret_cast<const f32x4*>(gq + k);
      s1 += a[0] * g[0] + a[1] * g[1] + a[2] * g[2] + a[3] * g[3];
      s2 += b[0] * h[0] + b[1] * h[1] + b[2] * h[2] + b[3] * h[3];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == n) w = s1;
    if (lane == 32 + n) w = s2;
  }
  w = valid ? fmaxf(w, 0.f) + 1e-3f : 0.f;                       // get_weight_vector (:64)
  w = valid ? fmaxf(w, 0.f) + 1e-5f : 0.f;                       // emd_inference_opencv (emd_utils.py:69-70)
  const float srow = wave_sum(is_row ? w : 0.f), scol = wave_sum(is_row ? 0.f : w);
  w *= (float)N / (is_row ? srow : scol);                        // both sum to N (emd_utils.py:72-73)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  st = emd_solve_wave(c, F, N, w, lane, nullptr);
  float s = 0.f;
  for (int idx = lane; idx < EMD_TILE; idx += 64) s += (1.0f - c[idx]) * F[idx];
  return wave_sum(s);
}
// F (this wave's LDS tile) -> fb [N][N], two rows per pass
__device__ __forceinline__ void emd_store_flow(const float* F, float* fb, const int N, const int lane) {
  const int b = lane & 31;
  for (int a = lane >> 5; a < N; a += 2)
    if (b < N) fb[a * N + b] = F[a * EMD_PITCH + b];
}

__global__ __launch_bounds__(64 * EMD_WAVES) void emd_pair_kernel(const float* __restrict__ shot_tok, const float* __restrict__ query_tok,
                                                                  const float* __restrict__ xhat, const float* __restrict__ pooled, int E, int P, int Q,
                                                                  int N, int C, float scale, float* __restrict__ logits, float* __restrict__ flow,
                                                                  int* __restrict__ status) {
  __shared__ float lds[EMD_WAVES][2][EMD_TILE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long prob = (long long)blockIdx.x * EMD_WAVES + wave;
  if (prob >= (long long)E * Q * P) return;
  const int p = (int)(prob % P);
  const long long eq = prob / P;                 // e * Q + q
  const int e = (int)(eq / Q);
  const size_t ip = (size_t)e * P + p, iq = (size_t)E * P + (size_t)eq;      // image indices in the workspace (protos first)
  float* c = lds[wave][0];
  float* F = lds[wave][1];
  int st;
  const float s = emd_pair_wave(query_tok + (size_t)eq * N * C, shot_tok + ip * N * C, xhat + iq * N * C, xhat + ip * N * C, pooled + iq * C, pooled + ip * C, N, C,
                                c, F, lane, st);
  if (lane == 0) {
    logits[prob] = s * scale;
    status[prob] = st;
  }
  if (flow) emd_store_flow(F, flow + (size_t)prob * N * N, N, lane);
}

// The problems of emd_pair_kernel over rows of a token-map table (tok / xhat [n_slots][N][C], pooled [n_slots][C], prepared once per image by
// fsvit_emd_table_prep): query (e, q) is the table row query_slots[e][q]; the class side is the row proto_slots[e][p], or - with proto_slots null - the
// dense map proto_tok[e][p] with its nodes in pxhat / ppool [E * P] (prepared by this launch).  A slot outside [0, n_slots) never becomes an address:
// the problems it takes part in write a NaN logit and status 0 and read nothing, and *invalid is raised by one per such entry of either slot array
// (by the problem at p == 0 for a query entry, at q == 0 for a proto entry; integer adds, any order).
template <typename L>
__global__ __launch_bounds__(64 * EMD_WAVES) void emd_gather_kernel(const float* __restrict__ tok, const float* __restrict__ xhat, const float* __restrict__ pooled,
                                                                    int n_slots, const L* __restrict__ query_slots, const L* __restrict__ proto_slots,
                                                                    const float* __restrict__ proto_tok, const float* __restrict__ pxhat,
                                                                    const float* __restrict__ ppool, int E, int P, int Q, int N, int C, float scale,
                                                                    float* __restrict__ logits, int* __restrict__ status, int* __restrict__ invalid) {
  __shared__ float lds[EMD_WAVES][2][EMD_TILE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long prob = (long long)blockIdx.x * EMD_WAVES + wave;
  if (prob >= (long long)E * Q * P) return;
  const int p = (int)(prob % P);
  const long long eq = prob / P;                 // e * Q + q
  const int e = (int)(eq / Q);
  const int q = (int)(eq - (long long)e * Q);
  const size_t ip = (size_t)e * P + p;
  const L qs = query_slots[eq], ps = proto_slots ? proto_slots[ip] : (L)0;
  const bool qbad = qs < (L)0 || qs >= (L)n_slots, pbad = ps < (L)0 || ps >= (L)n_slots;      // wave-uniform
  if (qbad || pbad) {
    if (lane == 0) {
      logits[prob] = __builtin_nanf("");
      status[prob] = 0;
      const int n_bad = (qbad && p == 0 ? 1 : 0) + (pbad && q == 0 ? 1 : 0);
      if (n_bad) atomicAdd(invalid, n_bad);
    }
    return;                                      // (no barrier in this kernel: the other waves of the workgroup go on)
  }
  const size_t NC = (size_t)N * C;
  const float* tp = proto_slots ? tok + (size_t)ps * NC : proto_tok + ip * NC;
  const float* xp = proto_slots ? xhat + (size_t)ps * NC : pxhat + ip * NC;
  const float* gp = proto_slots ? pooled + (size_t)ps * C : ppool + ip * C;
  float* c = lds[wave][0];
  float* F = lds[wave][1];
  int st;
  const float s = emd_pair_wave(tok + (size_t)qs * NC, tp, xhat + (size_t)qs * NC, xp, pooled + (size_t)qs * C, gp, N, C, c, F, lane, st);
  if (lane == 0) {
    logits[prob] = s * scale;
    status[prob] = st;
  }
}

// One workgroup per image (protos first, then queries), one wave per token.  d xhat = sum over partners and their tokens of g * F * partner xhat
// (g = dlogit * temperature / N), then back through x / max(|x|, 1e-8): rn (d xhat - xhat <xhat, d xhat>), then through the centring: minus the channel mean.
__global__ __launch_bounds__(256) void emd_bwd_kernel(const float* __restrict__ xhat, const float* __restrict__ rn, const float* __restrict__ dlogits,
                                                      const float* __restrict__ flow, int E, int P, int Q, int N, int C, float scale,
                                                      float* __restrict__ d_shot, float* __restrict__ d_query) {
  const int img = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool is_proto = img < E * P;
  const int e = is_proto ? img / P : (img - E * P) / Q;
  const int self = is_proto ? img - e * P : (img - E * P) - e * Q;            // p or q
  const int n_part = is_proto ? Q : P;
  float* out = is_proto ? d_shot + (size_t)img * N * C : d_query + (size_t)(img - E * P) * N * C;
  const float* xh = xhat + (size_t)img * N * C;
  for (int n = wave; n < N; n += 4) {
    float dot = 0.f;
    for (int k = lane * 4; k < C; k += 256) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < n_part; ++j) {
        const int q = is_proto ? j : self, p = is_proto ? self : j;
        const size_t pair = ((size_t)e * Q + q) * P + p;
        const float g = dlogits[pair] * scale;
        const float* fp = flow + pair * N * N;
        const float* oh = xhat + (is_proto ? (size_t)E * P + (size_t)e * Q + q : (size_t)e * P + p) * N * C;
        for (int m = 0; m < N; ++m) {
          const float f = is_proto ? fp[m * N + n] : fp[n * N + m];          // F[query node][proto node]
          if (f != 0.f) acc += (g * f) * *reinterpret_cast<const f32x4*>(oh + (size_t)m * C + k);
        }
      }
      const f32x4 x = *reinterpret_cast<const f32x4*>(xh + (size_t)n * C + k);
      dot += acc[0] * x[0] + acc[1] * x[1] + acc[2] * x[2] + acc[3] * x[3];
      *reinterpret_cast<f32x4*>(out + (size_t)n * C + k) = acc;
    }
    dot = wave_sum(dot);
    const float inv = rn[(size_t)img * N + n];
    float msum = 0.f;
    for (int k = lane * 4; k < C; k += 256) {                   // each lane re-reads only what it wrote itself
      const f32x4 x = *reinterpret_cast<const f32x4*>(xh + (size_t)n * C + k);
      f32x4 v = *reinterpret_cast<f32x4*>(out + (size_t)n * C + k);
      v = (v - x * dot) * inv;
      msum += v[0] + v[1] + v[2] + v[3];
      *reinterpret_cast<f32x4*>(out + (size_t)n * C + k) = v;
    }
    const float mean = wave_sum(msum) / (float)C;
    for (int k = lane * 4; k < C; k += 256) {
      f32x4 v = *reinterpret_cast<f32x4*>(out + (size_t)n * C + k);
      *reinterpret_cast<f32x4*>(out + (size_t)n * C + k) = v - mean;
    }
  }
}

// ---- the 5-shot SFC fine-tune (Network.py:83-107) on the device.  One workgroup owns one episode for n_steps mini-batch updates: the mini-batch's
// support images are the queries of the head, the SFC's `way` maps its protos.  Per step four phases, each closed by a block barrier that every wave
// reaches (no wave returns early, no barrier sits under a condition): prepare the SFC's nodes; one problem per (slot, class) and wave, EMD_SFC_WAVES at a
// time, each wave at most ceil(problems / EMD_SFC_WAVES) (emd_pair_wave: the arithmetic of emd_pair_kernel), flows and logits to the episode's workspace; dlogits; the backward onto the SFC (one wave per
// SFC token, fixed summation order, no atomics) with torch.optim.SGD's update of that token in place.  Nothing is handed between workgroups.
#ifndef FSVIT_EMD_SFC_WAVES
#define FSVIT_EMD_SFC_WAVES 16                     // 16 x 2 tiles = 135 KB of LDS, <= 128 VGPRs per lane (DESIGN.md 4f has the measurement against 8)
#endif
constexpr int EMD_SFC_WAVES = FSVIT_EMD_SFC_WAVES;

// An episode's workspace, in floats.  The arrays read 16 bytes at a time come first (each a multiple of 64 floats long); `stride` is a multiple of 4.
struct EmdSfcLayout {
  size_t sup_xhat, sfc_xhat, grad, sup_pool, sfc_pool, sfc_rn, flow, logit, dl, stride;
  __host__ __device__ EmdSfcLayout(int way, int n, int bs, int N, int C) {
    const size_t NC = (size_t)N * C;
    sup_xhat = 0;                                    // [n][N][C]    prepared nodes of the support images (constant over the fine-tune)
    sfc_xhat = sup_xhat + (size_t)n * NC;            // [way][N][C]  prepared nodes of the SFC, this step
    grad = sfc_xhat + (size_t)way * NC;              // [way][N][C]  d xhat, then d sfc
    sup_pool = grad + (size_t)way * NC;              // [n][C]       token means of the un-centred support maps
    sfc_pool = sup_pool + (size_t)n * C;             // [way][C]
    sfc_rn = sfc_pool + (size_t)way * C;             // [way][N]     inverse norms of the SFC's centred tokens
    flow = sfc_rn + (size_t)way * N;                 // [bs][way][N][N]
    logit = flow + (size_t)bs * way * N * N;         // [bs][way]
    dl = logit + (size_t)bs * way;                   // [bs][way]    dlogit * temperature / N
    stride = (dl + (size_t)bs * way + 3) & ~(size_t)3;
  }
};

// support [E][n][N][C], label [n], ids [n_steps][E][bs]; sfc, buf [E][way][N][C] in / out; status_count [E] in / out.  E = gridDim.x.
// (sfc, buf and the workspace carry no __restrict__: waves of the workgroup hand them to one another across the barriers.)
__global__ __launch_bounds__(64 * EMD_SFC_WAVES) void emd_sfc_kernel(const float* __restrict__ support, const int* __restrict__ label,
                                                                     const int* __restrict__ ids, int n_steps, int first, int way, int n, int bs, int N, int C,
                                                                     float scale, float lr, float momentum, float gmul, float* sfc_all, float* buf_all,
                                                                     int* status_count, float* ws_all) {
  __shared__ float lds[EMD_SFC_WAVES][2][EMD_TILE];
  __shared__ int bad[EMD_SFC_WAVES];
  __shared__ int next_prob;                                        // phase 2's problem counter
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;      // wave-uniform values stay in scalar registers
  const int e = blockIdx.x, E = gridDim.x;
  const int NC = N * C;                                            // the entry bounds an episode's workspace, so every index below, by 2^31
  const EmdSfcLayout L(way, n, bs, N, C);
  const float* sup = support + (size_t)e * n * NC;
  float* sfc = sfc_all + (size_t)e * way * NC;
  float* buf = buf_all + (size_t)e * way * NC;
  float* ws = ws_all + (size_t)e * L.stride;
  float *sup_xhat = ws + L.sup_xhat, *sfc_xhat = ws + L.sfc_xhat, *grad = ws + L.grad, *sup_pool = ws + L.sup_pool, *sfc_pool = ws + L.sfc_pool;
  float *sfc_rn = ws + L.sfc_rn, *flow = ws + L.flow, *logit = ws + L.logit, *dl = ws + L.dl;
  float* c = lds[wave][0];
  float* F = lds[wave][1];
  const int probs = bs * way, rounds = (probs + EMD_SFC_WAVES - 1) / EMD_SFC_WAVES;
  int nbad = 0;
  // the support images' nodes and token means: once per launch
  for (int i = wave; i < n * N; i += EMD_SFC_WAVES) emd_prep_token(sup + (size_t)i * C, sup_xhat + (size_t)i * C, C, lane);
  for (int i = tid; i < n * C; i += 64 * EMD_SFC_WAVES) {
    const int img = i / C;
    sup_pool[i] = emd_prep_pooled(sup + (size_t)img * NC, N, C, i - img * C);
  }
  for (int t = 0; t < n_steps; ++t) {
    const int* slot = ids + ((size_t)t * E + e) * bs;             // a slot outside [0, n) is empty: skipped, never an address
    // The lane index of phases 1, 3 and 4 is re-made opaque every step: otherwise their per-lane addresses are hoisted out of the step loop, live across
    // the solver of phase 2 (which needs all 128 registers of a 16-wave workgroup), and spilled.
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int tl = wave * 64 + ln;
    // 1. the SFC's nodes
    for (int i = wave; i < way * N; i += EMD_SFC_WAVES) {
      const float inv = emd_prep_token(sfc + (size_t)i * C, sfc_xhat + (size_t)i * C, C, ln);
      if (ln == 0) sfc_rn[i] = inv;
    }
    for (int i = tl; i < way * C; i += 64 * EMD_SFC_WAVES) {
      const int p = i / C;
      sfc_pool[i] = emd_prep_pooled(sfc + (size_t)p * NC, N, C, i - p * C);
    }
    if (tl == 0) next_prob = 0;
    __syncthreads();
    // 2. problem (slot q, class p) = q * way + p.  A wave that is done takes the next problem off a counter in LDS, at most `rounds` of them (enough for
    // all: EMD_SFC_WAVES * rounds >= probs), so the problems of the last round go to the waves whose first solves were short.  Which wave solves
    // which problem changes nothing: every result goes to the problem's own place in the workspace.  No wave waits for another here.
    for (int r = 0; r < rounds; ++r) {
      int prob = 0;
      if (ln == 0) prob = atomicAdd(&next_prob, 1);
      prob = __builtin_amdgcn_readfirstlane(prob);
      if (prob >= probs) break;
      const int q = prob / way, p = prob - q * way;
      const int id = __builtin_amdgcn_readfirstlane(slot[q]);
      if (id >= 0 && id < n) {
        int st, lp = ln;
        asm volatile("" : "+v"(lp));                              // (and per problem, as in emd_pair_kernel: the tile's row offsets are not kept either)
        const float s = emd_pair_wave(sup + (size_t)id * NC, sfc + (size_t)p * NC, sup_xhat + (size_t)id * NC, sfc_xhat + (size_t)p * NC,
                                      sup_pool + (size_t)id * C, sfc_pool + (size_t)p * C, N, C, c, F, lp, st);
        nbad += st;                                               // a problem at a loop bound still leaves a finite logit and a flow
        if (lp == 0) logit[prob] = s * scale;
        emd_store_flow(F, flow + (size_t)prob * N * N, N, lp);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");    // the tiles are reused by this wave's next problem
      }
    }
    __syncthreads();
    // 3. dl = (softmax(logits over way) - onehot(label)) / (slots in use) * temperature / N
    int b = 0;
    for (int q = 0; q < bs; ++q) b += (slot[q] >= 0 && slot[q] < n) ? 1 : 0;
    for (int q = tl; q < bs; q += 64 * EMD_SFC_WAVES) {
      const int id = slot[q];
      if (id >= 0 && id < n) {
        const int lab = label[id];
        const float* lg = logit + (size_t)q * way;
        float mx = lg[0], sum = 0.f;
        for (int p = 1; p < way; ++p) mx = fmaxf(mx, lg[p]);
        for (int p = 0; p < way; ++p) sum += expf(lg[p] - mx);
        for (int p = 0; p < way; ++p) dl[(size_t)q * way + p] = (expf(lg[p] - mx) / sum - (p == lab ? 1.0f : 0.f)) / (float)b * scale;
      }
    }
    __syncthreads();
    // 4. backward onto the SFC and the update, token (p, nn) = i on one wave: d xhat = sum over slots and their tokens of dl * F[m][nn] * xhat_q[m], then
    // rn (d xhat - xhat <xhat, d xhat>), minus the channel mean (emd_bwd_kernel's proto side); buf = grad on the first update of a fine-tune, else
    // momentum * buf + (1 - dampening) * grad; sfc -= lr * buf
    const bool start = first != 0 && t == 0;
    for (int i = wave; i < way * N; i += EMD_SFC_WAVES) {
      const int p = i / N, nn = i - p * N;
      const float* xh = sfc_xhat + (size_t)i * C;
      float* gr = grad + (size_t)i * C;
      float dot = 0.f;
      for (int k0 = 0; k0 < C; k0 += 256) {                       // (a uniform trip count: every lane takes part in the ballots below)
        const int k = k0 + ln * 4;
        const bool on = k < C;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < bs; ++q) {
          const int id = slot[q];
          if (id < 0 || id >= n) continue;
          const float g = dl[(size_t)q * way + p];
          const float* oh = sup_xhat + (size_t)id * NC;
          // column nn of F[support node][SFC node], one support node per lane; a flow has at most 2 N - 1 non-zero entries, so a column has few:
          // they are taken in ascending m (a fixed summation order)
          const float fcol = ln < N ? flow[((size_t)q * way + p) * N * N + ln * N + nn] : 0.f;
          unsigned long long mask = __ballot(fcol != 0.f);
          for (int j = 0; j < N && mask; ++j) {
            const int m = __ffsll((long long)mask) - 1;            // < N: only lanes below N can be set
            mask &= mask - 1;
            const float f = emd_lane_f(fcol, m);
            if (on) acc += (g * f) * *reinterpret_cast<const f32x4*>(oh + (size_t)m * C + k);
          }
        }
        if (on) {
          const f32x4 x = *reinterpret_cast<const f32x4*>(xh + k);
          dot += acc[0] * x[0] + acc[1] * x[1] + acc[2] * x[2] + acc[3] * x[3];
          *reinterpret_cast<f32x4*>(gr + k) = acc;
        }
      }
      dot = wave_sum(dot);
      const float inv = sfc_rn[i];
      float msum = 0.f;
      for (int k = ln * 4; k < C; k += 256) {                   // each lane re-reads only what it wrote itself
        const f32x4 x = *reinterpret_cast<const f32x4*>(xh + k);
        f32x4 v = *reinterpret_cast<f32x4*>(gr + k);
        v = (v - x * dot) * inv;
        msum += v[0] + v[1] + v[2] + v[3];
        *reinterpret_cast<f32x4*>(gr + k) = v;
      }
      const float mean = wave_sum(msum) / (float)C;
      for (int k = ln * 4; k < C; k += 256) {
        const f32x4 g = *reinterpret_cast<f32x4*>(gr + k) - mean;
        f32x4 m = g;
        if (!start) m = *reinterpret_cast<f32x4*>(buf + (size_t)i * C + k) * momentum + g * gmul;
        *reinterpret_cast<f32x4*>(buf + (size_t)i * C + k) = m;
        *reinterpret_cast<f32x4*>(sfc + (size_t)i * C + k) = *reinterpret_cast<f32x4*>(sfc + (size_t)i * C + k) - m * lr;
      }
    }
    __syncthreads();
  }
  if (lane == 0) bad[wave] = nbad;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < EMD_SFC_WAVES; ++w) s += bad[w];
    status_count[e] += s;
  }
}

size_t emd_sfc_workspace_bytes(int E, int way, int n, int bs, int N, int C) {
  return (size_t)E * EmdSfcLayout(way, n, bs, N, C).stride * sizeof(float);
}

int launch_emd_sfc_steps(const float* support, const int* label, const int* ids, int n_steps, int first, int E, int way, int n, int bs, int N, int C,
                         float temperature, float lr, float momentum, float dampening, float* sfc, float* buf, int* status_count, void* ws, hipStream_t s) {
  if (E <= 0 || n_steps <= 0) return 0;
  return launch(emd_sfc_kernel, dim3(E), dim3(64 * EMD_SFC_WAVES), 0, s, support, label, ids, n_steps, first, way, n, bs, N, C, temperature / (float)N, lr,
                momentum, 1.0f - dampening, sfc, buf, status_count, reinterpret_cast<float*>(ws));
}

size_t emd_head_workspace_bytes(int E, int P, int Q, int N, int C) {
  const size_t n_img = (size_t)E * ((size_t)P + (size_t)Q);
  return n_img * ((size_t)N * C + (size_t)C + (size_t)N) * sizeof(float);
}

static void emd_workspace_split(void* ws, int E, int P, int Q, int N, int C, float*& xhat, float*& pooled, float*& rn) {
  const size_t n_img = (size_t)E * ((size_t)P + (size_t)Q);
  xhat = reinterpret_cast<float*>(ws);
  pooled = xhat + n_img * N * C;
  rn = pooled + n_img * C;
}

int launch_emd_solve(const float* cost, const float* w1, const float* w2, int B, int N, float* flow, int* status, int* naug, hipStream_t s) {
  if (B <= 0) return 0;
  return launch(emd_solve_kernel, dim3((B + EMD_WAVES - 1) / EMD_WAVES), dim3(64 * EMD_WAVES), 0, s, cost, w1, w2, B, N, flow, status, naug);
}

int launch_emd_head_forward(const float* shot_tok, const float* query_tok, int E, int P, int Q, int N, int C, float temperature, float* logits, float* flow,
                            int* status, void* ws, hipStream_t s) {
  if (E <= 0 || P <= 0 || Q <= 0) return 0;
  float *xhat, *pooled, *rn;
  emd_workspace_split(ws, E, P, Q, N, C, xhat, pooled, rn);
  int rc = launch(emd_prep_kernel, dim3(E * (P + Q)), dim3(256), 0, s, shot_tok, query_tok, E * P, N, C, xhat, pooled, rn);
  if (rc) return rc;
  const long long probs = (long long)E * Q * P;
  return launch(emd_pair_kernel, dim3((unsigned)((probs + EMD_WAVES - 1) / EMD_WAVES)), dim3(64 * EMD_WAVES), 0, s, shot_tok, query_tok, xhat, pooled, E, P, Q, N,
                C, temperature / (float)N, logits, flow, status);
}

// Nodes and token means of n_img table rows: emd_prep_kernel over one array of maps, no rn (the table route is forward-only)
int launch_emd_table_prep(const float* tok, int n_img, int N, int C, float* xhat, float* pooled, hipStream_t s) {
  if (n_img <= 0) return 0;
  return launch(emd_prep_kernel, dim3(n_img), dim3(256), 0, s, tok, (const float*)nullptr, n_img, N, C, xhat, pooled, (float*)nullptr);
}

// the dense-prototype form keeps the E * P prepared prototypes in the workspace: the layout of the dense head's with no queries
size_t emd_head_gather_workspace_bytes(int E, int P, int N, int C) { return emd_head_workspace_bytes(E, P, 0, N, C); }

template <typename L>
static int launch_emd_gather_as(const float* tok, const float* xhat, const float* pooled, int n_slots, const void* query_slots, const void* proto_slots,
                                const float* proto_tok, const float* pxhat, const float* ppool, int E, int P, int Q, int N, int C, float scale, float* logits,
                                int* status, int* invalid, hipStream_t s) {
  const long long probs = (long long)E * Q * P;
  return launch(emd_gather_kernel<L>, dim3((unsigned)((probs + EMD_WAVES - 1) / EMD_WAVES)), dim3(64 * EMD_WAVES), 0, s, tok, xhat, pooled, n_slots,
                (const L*)query_slots, (const L*)proto_slots, proto_tok, pxhat, ppool, E, P, Q, N, C, scale, logits, status, invalid);
}

int launch_emd_head_gather(const float* tok, const float* xhat, const float* pooled, int n_slots, const void* query_slots, const void* proto_slots,
                           int slots_are_int64, const float* proto_tok, int E, int P, int Q, int N, int C, float temperature, float* logits, int* status,
                           int* invalid, void* ws, hipStream_t s) {
  if (E <= 0 || P <= 0 || Q <= 0) return 0;
  float *pxhat = nullptr, *ppool = nullptr, *rn = nullptr;
  if (proto_tok) {
    emd_workspace_split(ws, E, P, 0, N, C, pxhat, ppool, rn);
    int rc = launch(emd_prep_kernel, dim3(E * P), dim3(256), 0, s, proto_tok, (const float*)nullptr, E * P, N, C, pxhat, ppool, rn);
    if (rc) return rc;
  }
  const float scale = temperature / (float)N;
  return slots_are_int64 ? launch_emd_gather_as<long long>(tok, xhat, pooled, n_slots, query_slots, proto_slots, proto_tok, pxhat, ppool, E, P, Q, N, C, scale,
                                                           logits, status, invalid, s)
                         : launch_emd_gather_as<int>(tok, xhat, pooled, n_slots, query_slots, proto_slots, proto_tok, pxhat, ppool, E, P, Q, N, C, scale, logits,
                                                     status, invalid, s);
}

// ---- a labelled support set for the head: a bank of class token maps (models/emd_bank.TokenBank), and the exact re-rank of a shortlist of classes.
// Accumulate: proto_bank_accumulate_kernel's scheme over rows of N * C floats (its entry stops at D = 8192): one workgroup per (class, 256-wide slice)
// scans the label array, so a class's rows are added in ascending support index on top of the stored sum whatever the launch geometry - no
// floating-point atomics, and two calls over a split give the bits of one.
constexpr int EMD_BANK_SLICE = 256;

template <typename L>
__global__ __launch_bounds__(EMD_BANK_SLICE) void emd_bank_accumulate_kernel(const float* __restrict__ tok, const L* __restrict__ label, int S, int n_classes,
                                                                             int D, float* __restrict__ sum, int* __restrict__ count,
                                                                             int* __restrict__ invalid) {
  __shared__ int n_class, n_bad;
  const int c = blockIdx.x, t = threadIdx.x, d = blockIdx.y * EMD_BANK_SLICE + t;
  if (blockIdx.y == 0) {           // the class's count (and, in the workgroup of class 0, the labels no class takes): integer sums, any order
    if (t == 0) { n_class = 0; n_bad = 0; }
    __syncthreads();
    int mine = 0, bad = 0;
    for (int s = t; s < S; s += EMD_BANK_SLICE) {
      const L l = label[s];
      mine += (l == (L)c);
      bad += (l < (L)0 || l >= (L)n_classes);
    }
    if (mine) atomicAdd(&n_class, mine);
    if (bad && c == 0) atomicAdd(&n_bad, bad);
    __syncthreads();
    if (t == 0) {
      count[c] += n_class;
      if (c == 0 && n_bad) atomicAdd(invalid, n_bad);
    }
  }
  if (d >= D) return;              // (after the barriers above: uniform over the workgroups with blockIdx.y == 0, which all reach them)
  float acc = sum[(size_t)c * D + d];
  for (int s = 0; s < S; ++s)
    if (label[s] == (L)c) acc += tok[(size_t)s * D + d];      // a label outside [0, n_classes) equals no c: its row is never read
  sum[(size_t)c * D + d] = acc;
}

int launch_emd_bank_accumulate(const float* tok, const void* label, int label_is_int64, int S, int n_classes, int N, int C, float* sum, int* count,
                               int* invalid, hipStream_t s) {
  if (S <= 0) return 0;
  const int D = N * C;
  const dim3 grid(n_classes, (D + EMD_BANK_SLICE - 1) / EMD_BANK_SLICE);
  return label_is_int64 ? launch(emd_bank_accumulate_kernel<long long>, grid, dim3(EMD_BANK_SLICE), 0, s, tok, (const long long*)label, S, n_classes, D, sum,
                                 count, invalid)
                        : launch(emd_bank_accumulate_kernel<int>, grid, dim3(EMD_BANK_SLICE), 0, s, tok, (const int*)label, S, n_classes, D, sum, count, invalid);
}

// Finalize, one workgroup per class: tok = sum / count, then what emd_prep_kernel makes of that map (emd_prep_token / emd_prep_pooled: the same
// bodies on the same values, so the bits of fsvit_emd_table_prep), and proto = pooled / max(|pooled|, 1e-12), the class's row for the cosine shortlist.
// A class without examples: empty = 1 and zero rows everywhere.  (tok, xhat and pooled carry no __restrict__: written and read back in this launch.)
__global__ __launch_bounds__(256) void emd_bank_finalize_kernel(const float* __restrict__ sum, const int* __restrict__ count, int N, int C, float* tok_all,
                                                                float* xhat_all, float* pooled_all, float* __restrict__ proto_all,
                                                                int* __restrict__ empty) {
  const int cls = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int NC = N * C;
  const int n = count[cls];
  const float* srow = sum + (size_t)cls * NC;
  float* tok = tok_all + (size_t)cls * NC;
  float* xhat = xhat_all + (size_t)cls * NC;
  float* pooled = pooled_all + (size_t)cls * C;
  float* proto = proto_all + (size_t)cls * C;
  if (tid == 0) empty[cls] = n <= 0;
  if (n <= 0) {                                                  // uniform over the workgroup, before its first barrier
    for (int i = tid; i < NC; i += 256) { tok[i] = 0.f; xhat[i] = 0.f; }
    for (int k = tid; k < C; k += 256) { pooled[k] = 0.f; proto[k] = 0.f; }
    return;
  }
  const float fn = (float)n;
  for (int t = wave; t < N; t += 4) {
    for (int k = lane; k < C; k += 64) tok[t * C + k] = srow[t * C + k] / fn;      // emd_prep_token's lane pattern: a lane reads back its own stores
    emd_prep_token(tok + t * C, xhat + t * C, C, lane);
  }
  __syncthreads();
  for (int k = tid; k < C; k += 256) pooled[k] = emd_prep_pooled(tok, N, C, k);
  __syncthreads();
  float ss = 0.f;                                                // every wave forms the same |pooled|^2 in the same order
  for (int k = lane; k < C; k += 64) ss += pooled[k] * pooled[k];
  const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  for (int k = tid; k < C; k += 256) proto[k] = pooled[k] * inv;
}

int launch_emd_bank_finalize(const float* sum, const int* count, int n_classes, int N, int C, float* tok, float* xhat, float* pooled, float* proto, int* empty,
                             hipStream_t s) {
  return launch(emd_bank_finalize_kernel, dim3(n_classes), dim3(256), 0, s, sum, count, N, C, tok, xhat, pooled, proto, empty);
}

// Re-rank: query q against the classes cand[q][0 .. M) of the bank, one workgroup per query.  Wave w solves candidates w, w + EMD_WAVES, ..
// (emd_pair_wave: the problems, and the bits, of emd_gather_kernel on the same prepared rows) and leaves each logit in LDS; after the one block barrier
// wave 0 ranks the M values, one lane per candidate.  Every wave reaches that barrier: no wave returns early and the barrier sits under no condition
// (the discipline of emd_sfc_kernel; emd_gather_kernel, which has no barrier, returns early for a bad slot - this kernel must not).
// A candidate: -1 is an empty slot; an entry < -1 or >= n_classes raises *invalid by one and is an empty slot from then on - it never becomes an address;
// an empty slot and a class flagged `empty` score -inf and are not solved.  Order of the ranked list: the larger logit, then the lower class, then the
// lower candidate position, an empty slot (class -1: it holds nothing) after every class - the tail convention of proto_bank_topk, whose lists are the
// usual candidates.  prob = softmax over the finite entries of the row's M logits.
__device__ __forceinline__ bool emd_rank_before(float v, unsigned c, int i, float w, unsigned d, int j) {      // class -1 compares as 0xffffffff
  return v > w || (v == w && (c < d || (c == d && i < j)));
}

__global__ __launch_bounds__(64 * EMD_WAVES) void emd_rerank_kernel(const float* __restrict__ qtok, const float* __restrict__ qxhat,
                                                                    const float* __restrict__ qpooled, const float* __restrict__ btok,
                                                                    const float* __restrict__ bxhat, const float* __restrict__ bpooled,
                                                                    const int* __restrict__ empty, int n_classes, const int* __restrict__ cand, int M, int K,
                                                                    int N, int C, float scale, float* __restrict__ logits, int* __restrict__ classes,
                                                                    float* __restrict__ values, float* __restrict__ prob, int* __restrict__ status_count,
                                                                    int* __restrict__ invalid) {
  __shared__ float lds[EMD_WAVES][2][EMD_TILE];
  __shared__ float lg[32];                                       // the row's logits in candidate order (M <= 32)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const size_t q = blockIdx.x, NC = (size_t)N * C;
  const int* cq = cand + q * M;
  float* c = lds[wave][0];
  float* F = lds[wave][1];
  for (int m = wave; m < M; m += EMD_WAVES) {
    int cl = __builtin_amdgcn_readfirstlane(cq[m]);
    if (cl < -1 || cl >= n_classes) {
      if (lane == 0) atomicAdd(invalid, 1);
      cl = -1;
    }
    float v = -INFINITY;
    if (cl >= 0 && !__builtin_amdgcn_readfirstlane(empty[cl])) {                // wave-uniform: all 64 lanes enter the solver together
      int st;
      const float s = emd_pair_wave(qtok + q * NC, btok + (size_t)cl * NC, qxhat + q * NC, bxhat + (size_t)cl * NC, qpooled + q * C, bpooled + (size_t)cl * C,
                                    N, C, c, F, lane, st);
      v = s * scale;
      if (st && lane == 0) atomicAdd(status_count, 1);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the tiles are reused by this wave's next problem
    }
    if (lane == 0) lg[m] = v;
  }
  __syncthreads();
  if (wave == 0) {                                                // (no barrier below this line)
    const bool on = lane < M;
    const int raw = on ? cq[lane] : -1;
    const int cls = (raw < -1 || raw >= n_classes) ? -1 : raw;
    const float v = on ? lg[lane] : -INFINITY;
    int rank = 0;
    for (int i = 0; i < M; ++i) {                                 // M uniform steps: how many candidates come before this lane's
      const float vi = emd_lane_f(v, i);
      const int ci = emd_lane_i(cls, i);
      rank += emd_rank_before(vi, (unsigned)ci, i, v, (unsigned)cls, lane) ? 1 : 0;
    }
    const float mx = wave_max(v);                                 // lanes >= M hold -inf
    const float e = (v > -INFINITY) ? expf(v - mx) : 0.f;         // (mx is finite wherever v is)
    const float den = wave_sum(e);
    const float p = e > 0.f ? e / den : 0.f;
    if (on) {
      if (logits) logits[q * M + lane] = v;
      if (rank < K) {
        classes[q * K + rank] = cls;
        values[q * K + rank] = v;
        prob[q * K + rank] = p;
      }
    }
  }
}

int launch_emd_rerank(const float* qtok, const float* qxhat, const float* qpooled, int Q, const float* btok, const float* bxhat, const float* bpooled,
                      const int* empty, int n_classes, const int* cand, int M, int N, int C, float temperature, int K, float* logits, int* classes,
                      float* values, float* prob, int* status_count, int* invalid, hipStream_t s) {
  if (Q <= 0) return 0;
  return launch(emd_rerank_kernel, dim3(Q), dim3(64 * EMD_WAVES), 0, s, qtok, qxhat, qpooled, btok, bxhat, bpooled, empty, n_classes, cand, M, K, N, C,
                temperature / (float)N, logits, classes, values, prob, status_count, invalid);
}

int launch_emd_head_backward(const float* shot_tok, const float* query_tok, const float* dlogits, const float* flow, int E, int P, int Q, int N, int C,
                             float temperature, float* d_shot, float* d_query, void* ws, hipStream_t s) {
  if (E <= 0 || P <= 0 || Q <= 0) return 0;
  float *xhat, *pooled, *rn;
  emd_workspace_split(ws, E, P, Q, N, C, xhat, pooled, rn);
  int rc = launch(emd_prep_kernel, dim3(E * (P + Q)), dim3(256), 0, s, shot_tok, query_tok, E * P, N, C, xhat, pooled, rn);
  if (rc) return rc;
  return launch(emd_bwd_kernel, dim3(E * (P + Q)), dim3(256), 0, s, xhat, rn, dlogits, flow, E, P, Q, N, C, temperature / (float)N, d_shot, d_query);
}

}  // namespace fsvit

int fsvit_set_error(int code, const char* fmt, ...);      // engine.hip (library-internal, C++ linkage)

#define EMD_FAIL(...) return fsvit_set_error(FSVIT_ERR_ARG, __VA_ARGS__)

static const char* emd_shape_bad(int E, int P, int Q, int N, int C) {
  if (E < 0 || P < 0 || Q < 0) return "negative E / P / Q";
  if (N < 1 || N > 32) return "N must be 1 .. 32 (one lane per node)";
  if (C < 64 || C % 64) return "C must be a positive multiple of 64";
  if ((long long)E * ((long long)P + Q) > (1ll << 24) || (long long)E * P * Q > (1ll << 28)) return "too many images / problems for one launch";
  return nullptr;
}

extern "C" size_t fsvit_emd_head_workspace_bytes(int E, int P, int Q, int N, int C) {
  if (emd_shape_bad(E, P, Q, N, C)) return 0;
  return fsvit::emd_head_workspace_bytes(E, P, Q, N, C);
}

extern "C" int fsvit_emd_head_forward(const float* shot_tok, const float* query_tok, int E, int P, int Q, int N, int C, float temperature, float* logits,
                                      float* flow_or_null, int* status, void* workspace, size_t workspace_bytes, void* stream) {
  if (!shot_tok || !query_tok || !logits || !status || !workspace) EMD_FAIL("fsvit_emd_head_forward: null argument");
  if (const char* why = emd_shape_bad(E, P, Q, N, C)) EMD_FAIL("fsvit_emd_head_forward: E = %d, P = %d, Q = %d, N = %d, C = %d: %s", E, P, Q, N, C, why);
  if (!(temperature - temperature == 0.0f)) EMD_FAIL("fsvit_emd_head_forward: temperature is not finite");
  if (workspace_bytes < fsvit::emd_head_workspace_bytes(E, P, Q, N, C))
    return fsvit_set_error(FSVIT_ERR_WORKSPACE, "fsvit_emd_head_forward: workspace of %zu bytes, %zu needed", workspace_bytes,
                           fsvit::emd_head_workspace_bytes(E, P, Q, N, C));
  int rc = fsvit::launch_emd_head_forward(shot_tok, query_tok, E, P, Q, N, C, temperature, logits, flow_or_null, status, workspace, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_head_forward: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int fsvit_emd_head_backward(const float* shot_tok, const float* query_tok, const float* dlogits, const float* flow, int E, int P, int Q, int N,
                                       int C, float temperature, float* d_shot_tok, float* d_query_tok, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  if (!shot_tok || !query_tok || !dlogits || !flow || !d_shot_tok || !d_query_tok || !workspace) EMD_FAIL("fsvit_emd_head_backward: null argument");
  if (const char* why = emd_shape_bad(E, P, Q, N, C)) EMD_FAIL("fsvit_emd_head_backward: E = %d, P = %d, Q = %d, N = %d, C = %d: %s", E, P, Q, N, C, why);
  if (!(temperature - temperature == 0.0f)) EMD_FAIL("fsvit_emd_head_backward: temperature is not finite");
  if (workspace_bytes < fsvit::emd_head_workspace_bytes(E, P, Q, N, C))
    return fsvit_set_error(FSVIT_ERR_WORKSPACE, "fsvit_emd_head_backward: workspace of %zu bytes, %zu needed", workspace_bytes,
                           fsvit::emd_head_workspace_bytes(E, P, Q, N, C));
  int rc = fsvit::launch_emd_head_backward(shot_tok, query_tok, dlogits, flow, E, P, Q, N, C, temperature, d_shot_tok, d_query_tok, workspace,
                                           (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_head_backward: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int fsvit_emd_table_prep(const float* tok, int n_img, int N, int C, float* xhat, float* pooled, void* stream) {
  if (!tok || !xhat || !pooled) EMD_FAIL("fsvit_emd_table_prep: null argument");
  if (const char* why = emd_shape_bad(1, n_img, 0, N, C)) EMD_FAIL("fsvit_emd_table_prep: n_img = %d, N = %d, C = %d: %s", n_img, N, C, why);
  int rc = fsvit::launch_emd_table_prep(tok, n_img, N, C, xhat, pooled, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_table_prep: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" size_t fsvit_emd_head_gather_workspace_bytes(int E, int P, int N, int C) {
  if (emd_shape_bad(E, P, 0, N, C)) return 0;
  return fsvit::emd_head_gather_workspace_bytes(E, P, N, C);
}

extern "C" int fsvit_emd_head_gather(const float* tok, const float* xhat, const float* pooled, int n_slots, const void* query_slots,
                                     const void* proto_slots_or_null, int slots_are_int64, const float* proto_tok_or_null, int E, int P, int Q, int N, int C,
                                     float temperature, float* logits, int* status, int* invalid, void* workspace_or_null, size_t workspace_bytes,
                                     void* stream) {
  if (!tok || !xhat || !pooled || !query_slots || !logits || !status || !invalid) EMD_FAIL("fsvit_emd_head_gather: null argument");
  if (!proto_slots_or_null == !proto_tok_or_null) EMD_FAIL("fsvit_emd_head_gather: exactly one of proto_slots and proto_tok must be given");
  if (n_slots < 1) EMD_FAIL("fsvit_emd_head_gather: n_slots = %d", n_slots);
  if (const char* why = emd_shape_bad(E, P, Q, N, C)) EMD_FAIL("fsvit_emd_head_gather: E = %d, P = %d, Q = %d, N = %d, C = %d: %s", E, P, Q, N, C, why);
  if (!(temperature - temperature == 0.0f)) EMD_FAIL("fsvit_emd_head_gather: temperature is not finite");
  if (proto_tok_or_null) {
    const size_t need = fsvit::emd_head_gather_workspace_bytes(E, P, N, C);
    if (!workspace_or_null || workspace_bytes < need)
      return fsvit_set_error(FSVIT_ERR_WORKSPACE, "fsvit_emd_head_gather: workspace of %zu bytes, %zu needed", workspace_or_null ? workspace_bytes : (size_t)0,
                             need);
  }
  int rc = fsvit::launch_emd_head_gather(tok, xhat, pooled, n_slots, query_slots, proto_slots_or_null, slots_are_int64, proto_tok_or_null, E, P, Q, N, C,
                                         temperature, logits, status, invalid, workspace_or_null, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_head_gather: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

// ---- token-map bank and shortlist re-rank: limits as fsvit.h states them
static const char* emd_bank_shape_bad(int n_classes, int N, int C) {
  if (n_classes < 1 || n_classes > 65536) return "n_classes must be 1 .. 65536";
  if (N < 1 || N > 32) return "N must be 1 .. 32 (one lane per node)";
  if (C < 64 || C % 64 || C > 16384) return "C must be a positive multiple of 64, at most 16384";
  return nullptr;
}

extern "C" int fsvit_emd_bank_accumulate(const float* tok, const void* labels, int label_is_int64, int S, int n_classes, int N, int C, float* sum, int* count,
                                         int* invalid, void* stream) {
  if (S < 0 || S > (1 << 24)) EMD_FAIL("fsvit_emd_bank_accumulate: S = %d is outside [0, 2^24]", S);
  if (const char* why = emd_bank_shape_bad(n_classes, N, C)) EMD_FAIL("fsvit_emd_bank_accumulate: n_classes = %d, N = %d, C = %d: %s", n_classes, N, C, why);
  if (S == 0) return 0;                                          // nothing is touched (an empty array has no address to hand over)
  if (!tok || !labels || !sum || !count || !invalid) EMD_FAIL("fsvit_emd_bank_accumulate: null argument");
  int rc = fsvit::launch_emd_bank_accumulate(tok, labels, label_is_int64, S, n_classes, N, C, sum, count, invalid, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_bank_accumulate: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int fsvit_emd_bank_finalize(const float* sum, const int* count, int n_classes, int N, int C, float* tok, float* xhat, float* pooled, float* proto,
                                       int* empty, void* stream) {
  if (!sum || !count || !tok || !xhat || !pooled || !proto || !empty) EMD_FAIL("fsvit_emd_bank_finalize: null argument");
  if (const char* why = emd_bank_shape_bad(n_classes, N, C)) EMD_FAIL("fsvit_emd_bank_finalize: n_classes = %d, N = %d, C = %d: %s", n_classes, N, C, why);
  int rc = fsvit::launch_emd_bank_finalize(sum, count, n_classes, N, C, tok, xhat, pooled, proto, empty, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_bank_finalize: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int fsvit_emd_rerank(const float* query_tok, const float* query_xhat, const float* query_pooled, int Q, const float* bank_tok,
                                const float* bank_xhat, const float* bank_pooled, const int* bank_empty, int n_classes, const int* cand, int M, int N, int C,
                                float temperature, int K, float* logits_or_null, int* classes, float* values, float* prob, int* status_count, int* invalid,
                                void* stream) {
  if (Q < 0 || Q > (1 << 24)) EMD_FAIL("fsvit_emd_rerank: Q = %d is outside [0, 2^24]", Q);
  if (M < 1 || M > 32 || K < 1 || K > M) EMD_FAIL("fsvit_emd_rerank: K = %d, M = %d: 1 <= K <= M <= 32 (one lane per candidate)", K, M);
  if (const char* why = emd_bank_shape_bad(n_classes, N, C)) EMD_FAIL("fsvit_emd_rerank: n_classes = %d, N = %d, C = %d: %s", n_classes, N, C, why);
  if (!(temperature - temperature == 0.0f)) EMD_FAIL("fsvit_emd_rerank: temperature is not finite");
  if (Q == 0) return 0;                                          // nothing is touched (an empty array has no address to hand over)
  if (!query_tok || !query_xhat || !query_pooled || !bank_tok || !bank_xhat || !bank_pooled || !bank_empty || !cand || !classes || !values || !prob ||
      !status_count || !invalid)
    EMD_FAIL("fsvit_emd_rerank: null argument");
  int rc = fsvit::launch_emd_rerank(query_tok, query_xhat, query_pooled, Q, bank_tok, bank_xhat, bank_pooled, bank_empty, n_classes, cand, M, N, C, temperature,
                                    K, logits_or_null, classes, values, prob, status_count, invalid, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_rerank: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

static const char* emd_sfc_shape_bad(int E, int way, int n, int bs, int N, int C) {
  if (E < 0 || E > 65535) return "E must be 0 .. 65535 (one workgroup per episode)";
  if (way < 1 || n < 1 || bs < 1) return "way, n and bs must be at least 1";
  if (N < 1 || N > 32) return "N must be 1 .. 32 (one lane per node)";
  if (C < 64 || C % 64) return "C must be a positive multiple of 64";
  // ((n + 2 way) N C + (n + way) C + way N + bs way (N N + 2) floats per episode, in floating point so that the test itself cannot wrap)
  const double per = ((double)n + 2.0 * way) * N * C + ((double)n + way) * C + (double)way * N + (double)bs * way * (N * N + 2);
  if (per > 2147483000.0) return "an episode's workspace exceeds 2^31 floats";
  return nullptr;
}

extern "C" size_t fsvit_emd_sfc_workspace_bytes(int E, int way, int n, int bs, int N, int C) {
  if (emd_sfc_shape_bad(E, way, n, bs, N, C)) return 0;
  return fsvit::emd_sfc_workspace_bytes(E, way, n, bs, N, C);
}

extern "C" int fsvit_emd_sfc_steps(const float* support, const int* label, const int* ids, int n_steps, int first, int E, int way, int n, int bs, int N, int C,
                                   float temperature, float lr, float momentum, float dampening, float* sfc, float* buf, int* status_count, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!support || !label || !ids || !sfc || !buf || !status_count || !workspace) EMD_FAIL("fsvit_emd_sfc_steps: null argument");
  if (const char* why = emd_sfc_shape_bad(E, way, n, bs, N, C))
    EMD_FAIL("fsvit_emd_sfc_steps: E = %d, way = %d, n = %d, bs = %d, N = %d, C = %d: %s", E, way, n, bs, N, C, why);
  if (n_steps < 0) EMD_FAIL("fsvit_emd_sfc_steps: n_steps = %d", n_steps);
  for (const float v : {temperature, lr, momentum, dampening})
    if (!(v - v == 0.0f)) EMD_FAIL("fsvit_emd_sfc_steps: temperature, lr, momentum or dampening is not finite");
  const size_t need = fsvit::emd_sfc_workspace_bytes(E, way, n, bs, N, C);
  if (workspace_bytes < need)
    return fsvit_set_error(FSVIT_ERR_WORKSPACE, "fsvit_emd_sfc_steps: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  int rc = fsvit::launch_emd_sfc_steps(support, label, ids, n_steps, first, E, way, n, bs, N, C, temperature, lr, momentum, dampening, sfc, buf, status_count,
                                       workspace, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "fsvit_emd_sfc_steps: %s", hipGetErrorString((hipError_t)rc));
  return 0;
}

static int emd_solve_entry(const char* fn, const float* cost, const float* w1, const float* w2, int B, int N, float* flow, int* status, int* naug, void* stream) {
  if (!cost || !w1 || !w2 || !flow || !status) EMD_FAIL("%s: null argument", fn);
  if (B < 0 || B > (1 << 28)) EMD_FAIL("%s: B = %d", fn, B);
  if (N < 1 || N > 32) EMD_FAIL("%s: N = %d: N must be 1 .. 32 (one lane per node)", fn, N);
  int rc = fsvit::launch_emd_solve(cost, w1, w2, B, N, flow, status, naug, (hipStream_t)stream);
  if (rc) return fsvit_set_error(rc, "%s: %s", fn, hipGetErrorString((hipError_t)rc));
  return 0;
}

extern "C" int fsvit_op_emd_solve(const float* cost, const float* w1, const float* w2, int B, int N, float* flow, int* status, void* stream) {
  return emd_solve_entry("fsvit_op_emd_solve", cost, w1, w2, B, N, flow, status, nullptr, stream);
}

extern "C" int fsvit_op_emd_solve_counts(const float* cost, const float* w1, const float* w2, int B, int N, float* flow, int* status, int* n_augment,
                                         void* stream) {
  if (!n_augment) EMD_FAIL("fsvit_op_emd_solve_counts: null argument");
  return emd_solve_entry("fsvit_op_emd_solve_counts", cost, w1, w2, B, N, flow, status, n_augment, stream);
}
