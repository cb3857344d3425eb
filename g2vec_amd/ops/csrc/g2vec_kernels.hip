// g2vec_amd native kernels for AMD Instinct MI355X (gfx950, CDNA4).
//
// Hand-written HIP; no CUDA compatibility layers. Wavefront = 64 lanes
// throughout. Kernels (SURVEY 2.10 K-table in parentheses):
//
//   walk_kernel                 (K10) biased non-revisiting CSR walk, wave per walk, LDS hash-set visited
//   cbow_fwd_scalar_kernel      (K1+K2+K3+K8 collapsed) o_p = sum s_g + sigmoid-CE loss/correct/dlogit
//   cbow_eval_counts_kernel     fused eval: per-split correct counts + next-epoch train dlogits
//   cbow_eval_counts_lds_kernel same body with the s table staged in LDS (opt-in)
//   fold_partials_kernel        one-block fold of [n_blocks, 2] count partials
//   fold_partials_rows_kernel   the same fold for K evals' partial tables, block per table
//   cbow_eval_counts_rep_kernel<NT,VEC>  the eval body for R replicas (s_R [G, R]): one id load, R gathers
//   fold_partials_rep_kernel    per-replica fold of its [n_blocks, R, 2] partials
//   scatter_do_rep_kernel<NT,VEC>  c_R = X^T dO_R over the same plan, replica-minor
//   adam_rank1_rep_kernel / fold_gw_adam_rep_kernel / gemv_rows_rep_kernel<HPL>
//                               the fused tail and the GEMV with a replica grid dimension
//   scatter_do_det_kernel       (K6 collapsed) c = X^T dO by gene-sorted segments, atomic-free
//   adam_rank1_kernel           (K7) TF1 Adam, rank-1 grad c (x) who; optional dW_ho partials
//   fold_gw_adam_kernel         folds those partials and applies the W_ho Adam update
//   adam_dense_kernel           (K7) TF1 Adam, materialized grad
//   cbow_fwd_kernel<WT,HPL>     (K1+K2+K3+K8 general) row-gather forward, f32/bf16/fp16 W_ih, H stored
//   cbow_bwd_rows_det_kernel<HPL> (K6 general) per-gene-segment dW row reduce, atomic-free
//   pcc_edges_kernel            (K11) per-edge |PCC| dot product over samples
//   corr_gemm_kernel            (K11 dense) C = Z Z^T / S on v_mfma_f32_16x16x4_f32, LDS tiles
//   gemv_rows_kernel<HPL>       s = W @ x, wave per row
//   gemv_cols_kernel<CPT>       per-block partials of W^T c
//   fold_cols_kernel            folds the gemv_cols partials, wave per column
//   f32_to_bf16_kernel          round-to-nearest-even cast, NaN kept quiet
//   trunc_normal_kernel         (K9) seeded +-2 sigma truncated-normal fill
//   eval_scan_kernel            instance-parallel eval: segmented scan to per-window piece sums
//   eval_finish_kernel          thread-per-path fold of the pieces, counts + train dlogits
//   kmeans_step_kernel<HPL>     (step 5) fused Lloyd iteration: assign + per-block sums/counts/inertia
//   kmeans_fold_kernel          folds those partials, writes sums/counts/n_changed/inertia and C'
//   kmeans_mind2_kernel<HPL>    (step 5) k-means++ support: d2 = min(d2, |x - c|^2)
//   row_norms_kernel<HPL>       (step 6) d-score: f64-accumulated row L2 norms
//   t_scores_kernel             (step 6) |pooled t| per gene column, f64 two-pass
//   rank_columns_kernel         average ranks per gene column (ties included), LDS-tiled pair counting
//   ranksum_scores_kernel       (step 6) same body: rank-sum |z| and AUC per gene from int64 sums
//   col_moments_kernel          (step 6) f64 column sums of x and x*x for the permutation null
//   perm_t_stats_kernel         (step 6) t^2 per (relabelling, gene) on v_mfma_f32_16x16x4_f32
//   perm_t_counts_kernel        same body: per-gene exceed counts + per-relabelling max, no G x B output
//   knn_tile_kernel             nearest genes: [Q,h] x [h,G] on the same MFMA, fused per-row top-k
//   knn_merge_kernel            folds the per-block top-k lists of a candidate split
//   row_sqnorms_kernel          f64-accumulated squared row norms, any h % 4 == 0
//   cds_tile_kernel<KC>         silhouettes: the same product, per-cluster f64 distance sums per row
//   cds_fold_kernel             adds the per-block sums of a candidate split in ascending order
//
// The templates are instantiated by their launch sites in bindings.hip, the
// one translation unit that includes this file.
//
// Reference behaviour being reimplemented (not copied): mathcom/G2Vec
// G2Vec.py:328-346 (walk), :238-251 (CBOW fwd/loss/acc), :245-246 (Adam),
// :354-368 (PCC).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <cstdint>

// Debug build (G2VEC_DEBUG=1 at setup time): device-side bounds asserts in
// the index-following kernels (SURVEY 5.2 — the debug tier of the race/
// sanitizer story; host-side ASAN comes from the same flag's -fsanitize
// on the bindings TU).
#ifdef G2VEC_DEBUG
#define G2V_ASSERT(cond) \
  do { if (!(cond)) __builtin_trap(); } while (0)
#else
#define G2V_ASSERT(cond) do { } while (0)
#endif

#define WAVE 64

// ---------------------------------------------------------------- RNG / hash
// Must stay bit-identical to g2vec_amd/ops/cpu_ref.py::splitmix64/gene_hash.
__device__ __forceinline__ uint64_t sm64_next(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ULL;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double u01_from(uint64_t r) {
  return (double)(r >> 11) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ uint64_t gene_hash_dev(uint32_t g) {
  uint64_t s = (uint64_t)g * 0xBF58476D1CE4E5B9ULL + 0x9E3779B97F4A7C15ULL;
  return sm64_next(s);
}

// ---------------------------------------------------------------- wave utils
__device__ __forceinline__ int uni(int v) {
  return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ float unif(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// T: float everywhere on the training path; int / double in the k-means
// folds (counts, f64 inertia). One shuffle tree for all of them.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  return __shfl(v, 0);
}

// wave reduction with a PROVABLY-uniform (SGPR) result: downstream
// branches compile to scalar branches instead of exec-mask dances, and
// dependent integer math lands on the free scalar pipe
__device__ __forceinline__ float wave_sum_uni(float v) {
  for (int o = 32; o; o >>= 1) v += __shfl_down(v, o);
  return unif(v);   // lane 0 holds the total; full EXEC here
}

__device__ __forceinline__ float wave_incl_scan(float v) {
  const int lane = threadIdx.x & (WAVE - 1);
  for (int o = 1; o < WAVE; o <<= 1) {
    float t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// fold two per-thread accumulators over a 256-thread block (wave-reduce,
// then 4 wave slots in LDS); thread 0 writes the two totals to out2[0..1].
// The one fold order every count kernel shares.
__device__ __forceinline__ void block_fold2(float c0, float c1,
                                            float* __restrict__ out2) {
  c0 = wave_sum(c0);
  c1 = wave_sum(c1);
  __shared__ float sm[8];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  if (lane == 0) { sm[wib] = c0; sm[4 + wib] = c1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out2[0] = sm[0] + sm[1] + sm[2] + sm[3];
    out2[1] = sm[4] + sm[5] + sm[6] + sm[7];
  }
}

__device__ __forceinline__ float bf16_to_f32(uint16_t b) {
  union { float f; uint32_t u; } x;
  x.u = ((uint32_t)b) << 16;
  return x.f;
}

// tag types so the gather kernel can distinguish the two 16-bit formats
struct bf16_bits { uint16_t v; };
struct fp16_bits { uint16_t v; };

__device__ __forceinline__ float to_f32(const bf16_bits b) {
  return bf16_to_f32(b.v);
}
__device__ __forceinline__ float to_f32(const fp16_bits h) {
  return __half2float(*(const __half*)&h.v);
}
__device__ __forceinline__ float to_f32(const float f) { return f; }

__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
  union { float f; uint32_t u; } x;
  x.f = f;
  // NaN passes through as a quiet NaN of the same sign: the rounding add
  // below would carry a large payload out of the exponent (0x7FFFFFFF ->
  // 0x8000 = -0.0) or round a small one down to inf (0x7F800001 -> 0x7F80)
  if ((x.u & 0x7FFFFFFFu) > 0x7F800000u)
    return (uint16_t)((x.u >> 16) | 0x0040u);
  // round-to-nearest-even like torch's .bfloat16()
  uint32_t lsb = (x.u >> 16) & 1u;
  x.u += 0x7FFFu + lsb;
  return (uint16_t)(x.u >> 16);
}

// ================================================================= K10: walks
// One 64-lane wave per walk. Visited-set membership is an O(1) LDS
// open-addressing hash set (the naive O(path_len) visited-list scan per
// candidate left the CUs ~12% busy — latency-bound on the scan chain,
// measured via SQ_BUSY_CYCLES). For deg <= 64 the whole CSR row lives in
// one register per lane, so sampling is a single pass: masked weight ->
// wave sum -> wave prefix scan -> ballot pick. Matches the reference walk
// semantics exactly (G2Vec.py:328-346); the RNG stream is the framework's
// own (counter-based splitmix64, bit-shared with the CPU oracle).
#define HSET_EMPTY 0xFFFFFFFFu

__device__ __forceinline__ void hset_insert(uint32_t* tab, uint32_t tmask,
                                            uint32_t v) {
  uint32_t h = (v * 2654435761u) & tmask;
  for (;;) {
    const uint32_t c = tab[h];
    if (c == v) return;
    if (c == HSET_EMPTY) { tab[h] = v; return; }
    h = (h + 1) & tmask;
  }
}

__device__ __forceinline__ bool hset_contains(const uint32_t* tab,
                                              uint32_t tmask, uint32_t v) {
  uint32_t h = (v * 2654435761u) & tmask;
  for (;;) {
    const uint32_t c = tab[h];
    if (c == v) return true;
    if (c == HSET_EMPTY) return false;
    h = (h + 1) & tmask;
  }
}

// Rows with <= 4*64 neighbors sample entirely from registers (weights
// cached across the total/selection passes). Note: a packed int2
// {col,weight} layout was measured 19% SLOWER than separate col/weight
// arrays — CSR row starts have arbitrary parity, so half the dwordx2
// loads are 4-byte-misaligned.
#define WCHUNKS 4

extern "C" __global__ void __launch_bounds__(256)
walk_kernel(const int* __restrict__ row_ptr, const int* __restrict__ col_idx,
            const float* __restrict__ wgt, const int* __restrict__ sources,
            int n_src, long long n_walks, int num_rep, int len_path, int tsize,
            uint64_t seed, int* __restrict__ out_nodes,
            int* __restrict__ out_len, long long* __restrict__ out_hash) {
  extern __shared__ int smem[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = uni(threadIdx.x >> 6);       // wave-in-block (SGPR)
  const int wpb = blockDim.x >> 6;             // waves per block
  int* vis = smem + wib * len_path;            // ordered path (output)
  uint32_t* tab = (uint32_t*)(smem + wpb * len_path) + wib * tsize;
  const uint32_t tmask = (uint32_t)tsize - 1;

  for (long long walk = (long long)blockIdx.x * wpb + wib; walk < n_walks;
       walk += (long long)gridDim.x * wpb) {
    const int rep = (int)(walk / n_src);
    const int src = uni(sources[walk % n_src]);
    // RNG keyed on the GLOBAL (source, repetition): DP-sharded generation
    // is bitwise-identical to single-process (C5 rank invariance)
    const uint64_t gid = (uint64_t)src * (uint64_t)num_rep + (uint64_t)rep;
    uint64_t state = seed ^ (uint64_t)(gid * 0x94D049BB133111EBULL + 1ULL);
    (void)sm64_next(state);                    // warm draw (CPU oracle parity)
    int cur = src;
    int plen = 0;
    uint64_t hash = 0;
    for (int i = lane; i < tsize; i += WAVE) tab[i] = HSET_EMPTY;

    for (int step = 0; step < len_path; ++step) {
      G2V_ASSERT(plen < len_path && cur >= 0);
      if (lane == 0) {
        vis[plen] = cur;
        // ONE lane inserts: a 64-lane same-address LDS store serializes its
        // lane group and the LDS array is shared by all 32 waves of the CU
        hset_insert(tab, tmask, (uint32_t)cur);
      }
      ++plen;
      hash += gene_hash_dev((uint32_t)cur);
      const int s = row_ptr[cur], e = row_ptr[cur + 1];
      const int deg = e - s;
      if (deg <= 0) break;

      if (deg <= WAVE) {
        // leanest path (the common case): one candidate per lane
        const int j = lane;
        int cand = -1;
        float w = 0.f;
        if (j < deg) {
          cand = col_idx[s + j];
          w = wgt[s + j];
          if (hset_contains(tab, tmask, (uint32_t)cand)) w = 0.f;
        }
        // one scan serves both the total (its lane-63 element) and the
        // selection — 6 fewer dependent ds_bpermute per step
        const float scan = wave_incl_scan(w);
        const float tot = unif(__shfl(scan, WAVE - 1));
        const uint64_t r = sm64_next(state);   // drawn even on dead end
        if (!(tot > 0.f)) break;
        const float target = (float)(u01_from(r) * (double)tot);
        const bool hit = (w > 0.f) && (scan > target) && (scan - w <= target);
        const unsigned long long mh = __ballot(hit);
        int lane_sel;
        if (mh != 0ULL) {
          lane_sel = __ffsll((long long)mh) - 1;
        } else {
          const unsigned long long mp = __ballot(w > 0.f);
          lane_sel = 63 - __clzll((long long)mp);
        }
        cur = uni(__shfl(cand, lane_sel));
      } else if (deg <= WCHUNKS * WAVE) {
        // register path: the whole row (<= 4 chunks of 64) is loaded once,
        // membership-masked once, and both the total and the selection use
        // the cached registers — one dwordx2 load + one hash probe per
        // candidate per STEP, nothing re-read.
        const int nchunk = (deg + WAVE - 1) >> 6;
        float wreg[WCHUNKS];
        int creg[WCHUNKS];
        float partial = 0.f;
#pragma unroll
        for (int k = 0; k < WCHUNKS; ++k) {
          wreg[k] = 0.f;
          creg[k] = -1;
          const int j = (k << 6) + lane;
          if (k < nchunk && j < deg) {
            const int cc = col_idx[s + j];
            creg[k] = cc;
            float w = wgt[s + j];
            if (hset_contains(tab, tmask, (uint32_t)cc)) w = 0.f;
            wreg[k] = w;
            partial += w;
          }
        }
        const float tot = wave_sum_uni(partial);
        const uint64_t r = sm64_next(state);   // drawn even on dead end
        if (!(tot > 0.f)) break;
        const float target = (float)(u01_from(r) * (double)tot);
        int chosen_cand = -1;
        float base = 0.f;
        unsigned long long any_pos = 0ULL;
        int last_pos_cand = -1;
        for (int k = 0; k < nchunk; ++k) {
          const float w = wreg[k];
          const float scan = wave_incl_scan(w);
          const float chunk_tot = unif(__shfl(scan, WAVE - 1));
          const bool hit = (w > 0.f) && (base + scan > target) &&
                           (base + scan - w <= target);
          const unsigned long long m = __ballot(hit);
          if (m != 0ULL) {
            chosen_cand = uni(__shfl(creg[k], __ffsll((long long)m) - 1));
            break;
          }
          const unsigned long long mp = __ballot(w > 0.f);
          if (mp != 0ULL) {
            any_pos = 1;
            last_pos_cand = uni(__shfl(creg[k], 63 - __clzll((long long)mp)));
          }
          base += chunk_tot;
        }
        if (chosen_cand < 0) {
          // rounding tail: target >= running total -> last unvisited
          if (!any_pos) break;                 // cannot happen when tot > 0
          chosen_cand = last_pos_cand;
        }
        cur = chosen_cand;
      } else {
        // chunked fallback for very-high-degree nodes (> 256 neighbors)
        float partial = 0.f;
        for (int j = lane; j < deg; j += WAVE) {
          const int cc = col_idx[s + j];
          float w = wgt[s + j];
          if (hset_contains(tab, tmask, (uint32_t)cc)) w = 0.f;
          partial += w;
        }
        const float tot = wave_sum_uni(partial);
        const uint64_t r = sm64_next(state);
        if (!(tot > 0.f)) break;
        const float target = (float)(u01_from(r) * (double)tot);
        int chosen = -1;
        float base = 0.f;
        for (int j0 = 0; j0 < deg; j0 += WAVE) {
          const int j = j0 + lane;
          float w = 0.f;
          if (j < deg) {
            const int cc = col_idx[s + j];
            w = wgt[s + j];
            if (hset_contains(tab, tmask, (uint32_t)cc)) w = 0.f;
          }
          const float scan = wave_incl_scan(w);
          const float chunk_tot = unif(__shfl(scan, WAVE - 1));
          const bool hit = (j < deg) && (w > 0.f) &&
                           (base + scan > target) && (base + scan - w <= target);
          const unsigned long long m = __ballot(hit);
          if (m != 0ULL) { chosen = j0 + (__ffsll((long long)m) - 1); break; }
          base += chunk_tot;
        }
        if (chosen < 0) {
          for (int j0 = ((deg - 1) / WAVE) * WAVE; j0 >= 0 && chosen < 0;
               j0 -= WAVE) {
            const int j = j0 + lane;
            float w = 0.f;
            if (j < deg) {
              const int cc = col_idx[s + j];
              w = wgt[s + j];
              if (hset_contains(tab, tmask, (uint32_t)cc)) w = 0.f;
            }
            const unsigned long long m = __ballot(w > 0.f);
            if (m != 0ULL) chosen = j0 + (63 - __clzll((long long)m));
          }
          if (chosen < 0) break;               // cannot happen when tot > 0
        }
        cur = uni(col_idx[s + chosen]);
      }
    }

    long long outb = walk * (long long)len_path;
    for (int k = lane; k < len_path; k += WAVE)
      out_nodes[outb + k] = (k < plen) ? vis[k] : -1;
    if (lane == 0) {
      out_len[walk] = plen;
      out_hash[walk] = (long long)hash;
    }
  }
}

// ===================================================== fast path: scalar CBOW
// o_p = sum_{g in p} s_g; loss = sigmoid-CE(o, y); correct = (o>0)==y;
// dO = (sigmoid(o)-y)*inv_b. One 16-LANE SUB-WAVE per path (4 paths per
// wavefront): paths average ~21 genes, so a full 64-lane wave left 2/3 of
// its lanes idle in both the gather and the reduce, and a thread-per-path
// variant serialized on gather latency (1.5x slower at 1M genes).
#define SUBW 16

__device__ __forceinline__ float subwave_sum16(float v) {
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;                       // every lane of the 16-group has the sum
}

// The per-path epilogue, in one place: the CPU oracle matches these three
// expressions bit for bit, and the fast and general paths must not fork.
__device__ __forceinline__ float sigmoid_ce(float o, float y) {
  return fmaxf(o, 0.f) - o * y + log1pf(expf(-fabsf(o)));
}
__device__ __forceinline__ float is_correct(float o, float y) {
  return ((o > 0.f ? 1.f : 0.f) == y) ? 1.f : 0.f;
}
__device__ __forceinline__ float dlogit(float o, float y, float inv_b) {
  return (1.f / (1.f + expf(-o)) - y) * inv_b;
}

extern "C" __global__ void __launch_bounds__(256)
cbow_fwd_scalar_kernel(const float* __restrict__ s, const int* __restrict__ genes,
                       const int* __restrict__ offs, const float* __restrict__ labels,
                       long long P, float inv_b, float* __restrict__ loss,
                       float* __restrict__ correct, float* __restrict__ dO) {
  const int sublane = threadIdx.x & (SUBW - 1);
  const int subs_per_block = blockDim.x / SUBW;
  const int sub = threadIdx.x / SUBW;
  for (long long p = (long long)blockIdx.x * subs_per_block + sub; p < P;
       p += (long long)gridDim.x * subs_per_block) {
    const int lo = offs[p], hi = offs[p + 1];
    float partial = 0.f;
    for (int i = lo + sublane; i < hi; i += SUBW) partial += s[genes[i]];
    const float o = subwave_sum16(partial);
    if (sublane == 0) {
      const float y = labels[p];
      loss[p] = sigmoid_ce(o, y);
      correct[p] = is_correct(o, y);
      if (dO) dO[p] = dlogit(o, y, inv_b);
    }
  }
}

// eval-only variant: nothing stored per path; the two splits' correct
// counts (train = paths < p_split of the concatenated set, val = rest)
// accumulate per wave, reduce in-block, and write ATOMIC-FREE per-block
// partials; a one-block second pass folds them (a same-two-words atomic
// fan-in measured ~11 ns per serialized add — 10k blocks cost 200 us).
// One body for both entry points below: st is the s table, in global
// memory or staged in LDS, and everything else — per-path math and
// accumulation order — is the same code, hence bitwise-equal outputs.
// subs_per_block = blockDim.x / SUBW is read by the entry point: only in a
// __global__ function does the compiler fold blockDim to one scalar load.
//
// The gather is latency-bound (id load -> dependent s load, ~0.7 TB/s of
// id traffic at the ex shape), so a path is walked in ROUNDS of EVAL_U x 16
// instances: EVAL_U independent nontemporal id loads back to back, then
// EVAL_U gathers, then the adds — in ascending i per lane, the exact
// sequence of `partial += st[genes[i]]` (cbow_fwd_scalar_kernel defines
// that order). A slot past hi re-loads the path's last id (in range) and
// is dropped by a select, never by adding 0.0f (-0.0f must survive). The
// next path's offs/label loads are issued ahead of the current path's
// rounds. An empty path runs no round: no id load, no gather.
// EVAL_U = 5 covers len_path 80 in one round (registers: docs/KERNELS.md).
#ifndef EVAL_U
#define EVAL_U 5
#endif

__device__ __forceinline__ void
eval_counts_body(const float* __restrict__ st, const int* __restrict__ genes,
                 const int* __restrict__ offs, const float* __restrict__ labels,
                 long long P, long long p_split, float* __restrict__ partials,
                 float* __restrict__ dO, float inv_b, int subs_per_block) {
  const int sublane = threadIdx.x & (SUBW - 1);
  const int sub = threadIdx.x / SUBW;
  const long long stride = (long long)gridDim.x * subs_per_block;
  float c0 = 0.f, c1 = 0.f;                    // sublane-0 accumulators
  long long p = (long long)blockIdx.x * subs_per_block + sub;
  int lo = 0, hi = 0;
  float y = 0.f;
  if (p < P) { lo = offs[p]; hi = offs[p + 1]; y = labels[p]; }
  while (p < P) {
    const long long pn = p + stride;
    // next path's bounds + label, in flight during this path's rounds.
    // Unconditional (index clamped to the last path): behind a branch the
    // compiler's wait for lo/hi below would also wait for these loads.
    const long long pc = pn < P ? pn : P - 1;
    const int lo_n = offs[pc], hi_n = offs[pc + 1];
    const float y_n = labels[pc];
    float partial = 0.f;
    for (int i0 = lo + sublane; i0 - sublane < hi; i0 += EVAL_U * SUBW) {
      int id[EVAL_U];
      float sv[EVAL_U];
#pragma unroll
      for (int u = 0; u < EVAL_U; ++u) {
        const int i = i0 + u * SUBW;
        id[u] = __builtin_nontemporal_load(&genes[i < hi ? i : hi - 1]);
      }
#pragma unroll
      for (int u = 0; u < EVAL_U; ++u) sv[u] = st[id[u]];
#pragma unroll
      for (int u = 0; u < EVAL_U; ++u)
        partial = (i0 + u * SUBW < hi) ? partial + sv[u] : partial;
    }
    const float o = subwave_sum16(partial);
    if (sublane == 0) {
      const float corr = is_correct(o, y);
      if (p < p_split) c0 += corr; else c1 += corr;
      // fused next-epoch forward: this eval's s IS the next epoch's
      // pre-update s, so emit the train-split dO here and the standalone
      // forward kernel disappears from steady-state epochs (the s-gather
      // over the train paths runs ONCE per weight version, not twice)
      if (dO && p < p_split) dO[p] = dlogit(o, y, inv_b);
    }
    p = pn; lo = lo_n; hi = hi_n; y = y_n;
  }
  block_fold2(c0, c1, partials + 2 * blockIdx.x);
}

extern "C" __global__ void __launch_bounds__(256)
cbow_eval_counts_kernel(const float* __restrict__ s, const int* __restrict__ genes,
                        const int* __restrict__ offs, const float* __restrict__ labels,
                        long long P, long long p_split,
                        float* __restrict__ partials,
                        float* __restrict__ dO, float inv_b) {
  eval_counts_body(s, genes, offs, labels, P, p_split, partials, dO, inv_b,
                   blockDim.x / SUBW);
}

// LDS-staged variant: at ex_* scale the whole s table is 30 KB, but the
// subwave gathers above are TA-throughput bound — a 64-lane gather over a
// 30 KB range touches ~40-60 distinct L1 lines, serialized in the CU's
// one texture/addressing unit. Staging s in LDS turns each gather into a
// ds_read (32-bank parallel, ~2-4x conflict factor), so the block pays
// one coalesced G-float stage (L2-broadcast: every block reads the same
// table) and then gathers at LDS rate. The host picks this kernel when
// G*4 fits the LDS budget and caps the grid so each resident block
// amortizes its stage over many paths.
extern "C" __global__ void __launch_bounds__(256)
cbow_eval_counts_lds_kernel(const float* __restrict__ s,
                            const int* __restrict__ genes,
                            const int* __restrict__ offs,
                            const float* __restrict__ labels,
                            long long P, long long p_split,
                            float* __restrict__ partials,
                            float* __restrict__ dO, float inv_b, int G) {
  extern __shared__ float s_lds[];
  for (int g = threadIdx.x; g < G; g += blockDim.x) s_lds[g] = s[g];
  __syncthreads();
  eval_counts_body(s_lds, genes, offs, labels, P, p_split, partials, dO,
                   inv_b, blockDim.x / SUBW);
}

extern "C" __global__ void __launch_bounds__(256)
fold_partials_kernel(const float* __restrict__ partials, int n_blocks,
                     float* __restrict__ counts) {
  float c0 = 0.f, c1 = 0.f;
  for (int b = threadIdx.x; b < n_blocks; b += blockDim.x) {
    c0 += partials[2 * b];
    c1 += partials[2 * b + 1];
  }
  block_fold2(c0, c1, counts);
}

// The same fold for a block of K evals at once: partials [K, n_blocks, 2],
// counts [K, 2], block k folds row k exactly as fold_partials_kernel would.
// The K-epoch block graph parks each epoch's partials in its own row and
// folds them with this one launch instead of one per epoch.
extern "C" __global__ void __launch_bounds__(256)
fold_partials_rows_kernel(const float* __restrict__ partials, int n_blocks,
                          float* __restrict__ counts) {
  partials += (long long)blockIdx.x * n_blocks * 2;
  float c0 = 0.f, c1 = 0.f;
  for (int b = threadIdx.x; b < n_blocks; b += blockDim.x) {
    c0 += partials[2 * b];
    c1 += partials[2 * b + 1];
  }
  block_fold2(c0, c1, counts + 2 * blockIdx.x);
}

// ================================== replica-batched fast path (R <= REP_MAX)
// R independently initialised models train on ONE path set: ids, offsets,
// labels and the scatter plan are shared, the tables carry the replica
// index innermost (s_R [G, R], dO_R [P, R], c_R [G, R]). A kernel handles
// NT tiles of four replicas: one id load serves all of them and the four
// values of a tile are one 16-byte gather. VEC = (R % 4 == 0, 16-byte
// aligned base); otherwise four scalar loads whose replica index is clamped
// to R - 1 — in range, and the surplus sums are never stored. Per replica
// every kernel performs the single-model kernel's additions in the
// single-model kernel's order, so each output is bitwise the single op's.
#define REP_MAX 32
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__device__ __forceinline__ f32x4 rep_gather4(const float* __restrict__ tab,
                                             int row, int R, int t) {
  if (VEC)
    return ((const f32x4*)tab)[(long long)row * (R >> 2) + t];
  const float* p = tab + (long long)row * R;
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = 4 * t + k;
    o[k] = p[r < R ? r : R - 1];
  }
  return o;
}

// Batched eval_counts_body: same sub-wave-per-path walk, same rounds, the
// same select-not-add-zero handling of slots past hi. After the 16-lane
// reduce every lane holds every replica's o, so the epilogue is spread over
// the lanes: sublane j owns replicas j and j + 16 (is_correct, dlogit, the
// coalesced dO_R store and the two count accumulators). The block fold goes
// through LDS to per-block partials [gridDim.x, R, 2]; counts are integers
// below 2^24, so their fold order is free.
template <int NT, bool VEC>
__global__ void __launch_bounds__(256)
cbow_eval_counts_rep_kernel(const float* __restrict__ s_R,
                            const int* __restrict__ genes,
                            const int* __restrict__ offs,
                            const float* __restrict__ labels,
                            long long P, long long p_split, int R,
                            float* __restrict__ partials,
                            float* __restrict__ dO_R, float inv_b) {
  constexpr int NR = NT * 4;
  constexpr int NK = NR > SUBW ? 2 : 1;        // replicas owned per sublane
  const int subs_per_block = blockDim.x / SUBW;
  const int sublane = threadIdx.x & (SUBW - 1);
  const int sub = threadIdx.x / SUBW;
  const long long stride = (long long)gridDim.x * subs_per_block;
  float c0[NK], c1[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) { c0[k] = 0.f; c1[k] = 0.f; }
  long long p = (long long)blockIdx.x * subs_per_block + sub;
  int lo = 0, hi = 0;
  float y = 0.f;
  if (p < P) { lo = offs[p]; hi = offs[p + 1]; y = labels[p]; }
  while (p < P) {
    const long long pn = p + stride;
    const long long pc = pn < P ? pn : P - 1;
    const int lo_n = offs[pc], hi_n = offs[pc + 1];
    const float y_n = labels[pc];
    float part[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) part[r] = 0.f;
    for (int i0 = lo + sublane; i0 - sublane < hi; i0 += EVAL_U * SUBW) {
      int id[EVAL_U];
#pragma unroll
      for (int u = 0; u < EVAL_U; ++u) {
        const int i = i0 + u * SUBW;
        id[u] = __builtin_nontemporal_load(&genes[i < hi ? i : hi - 1]);
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4 sv[EVAL_U];
#pragma unroll
        for (int u = 0; u < EVAL_U; ++u)
          sv[u] = rep_gather4<VEC>(s_R, id[u], R, t);
#pragma unroll
        for (int u = 0; u < EVAL_U; ++u)
#pragma unroll
          for (int k = 0; k < 4; ++k)
            part[4 * t + k] = (i0 + u * SUBW < hi)
                                  ? part[4 * t + k] + sv[u][k]
                                  : part[4 * t + k];
      }
    }
    float o[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) o[k] = 0.f;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const float orr = subwave_sum16(part[r]);
      if ((r & (SUBW - 1)) == sublane) o[r / SUBW] = orr;
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int r = sublane + k * SUBW;
      if (r < R) {
        const float corr = is_correct(o[k], y);
        if (p < p_split) c0[k] += corr; else c1[k] += corr;
        if (dO_R && p < p_split) dO_R[p * R + r] = dlogit(o[k], y, inv_b);
      }
    }
    p = pn; lo = lo_n; hi = hi_n; y = y_n;
  }
  // block fold: slot [2k + split][thread]; thread (k, split, j) sums the
  // block's sub-waves for replica j + 16k
  __shared__ float sm[4 * 256];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    sm[(2 * k) * 256 + threadIdx.x] = c0[k];
    sm[(2 * k + 1) * 256 + threadIdx.x] = c1[k];
  }
  __syncthreads();
  if (threadIdx.x < 2 * NK * SUBW) {
    const int which = threadIdx.x / SUBW;      // 2k + split
    const int r = sublane + (which >> 1) * SUBW;
    float tot = 0.f;
    for (int sb = 0; sb < subs_per_block; ++sb)
      tot += sm[which * 256 + sb * SUBW + sublane];
    if (r < R)
      partials[((long long)blockIdx.x * R + r) * 2 + (which & 1)] = tot;
  }
}

// one block per replica folds its [n_blocks, 2] column of the partials
extern "C" __global__ void __launch_bounds__(256)
fold_partials_rep_kernel(const float* __restrict__ partials, int n_blocks,
                         int R, float* __restrict__ counts_R) {
  const int r = blockIdx.x;
  float c0 = 0.f, c1 = 0.f;
  for (int b = threadIdx.x; b < n_blocks; b += blockDim.x) {
    c0 += partials[((long long)b * R + r) * 2];
    c1 += partials[((long long)b * R + r) * 2 + 1];
  }
  block_fold2(c0, c1, counts_R + 2 * r);
}

// =============================================== fast path: c = X^T dO (det.)
// One wave per gene segment (instances pre-sorted by gene, plan built once
// per path set). Fixed tree-reduction order -> bitwise reproducible.
//
// The order, per lane l of a segment [lo, hi) (scatter_do_rep_kernel spells
// it as two loops): slot k is instance lo + l + 64k; group q = slots
// 4q..4q+3 is FULL for the lane iff lo + l + 256q + 192 < hi; a full group
// adds slot 4q+j into p_j, ascending q; every remaining slot goes into p0,
// ascending, after the full groups; then wave_sum((p0 + p1) + (p2 + p3)).
// A lane's full groups precede its other slots, so walking the slots once in
// ascending order with the accumulator chosen per slot is that order.
//
// A segment is walked in ROUNDS of SCAT_U slots: SCAT_U id loads back to
// back, SCAT_U gathers, then the adds in slot order, so a round costs two
// memory round trips however many slots it has. SCAT_U is a multiple of 4,
// so slot u of a round belongs to p_(u % 4) statically. A slot past hi
// re-loads index hi - 1 (in range) and is dropped by a select, never by
// adding 0.0f. The gene comes with the segment bounds and c[gene] is fetched
// before the rounds. An empty segment runs no round.
// Measured at the ex shape (profiles/README.md, "Epoch chain, second cut"):
// the id loads are PLAIN loads — the 10 MB plan stays resident in the XCD
// L2s from one epoch to the next, and nontemporal id loads cost 3 us per
// launch (12.8 against 9.7 us); loading the next segment's bounds ahead,
// as the eval does for paths, gained nothing, because the launch gives every
// segment its own wave up to 4M segments, so the loop is a plain grid
// stride.
#ifndef SCAT_U
#define SCAT_U 8
#endif
static_assert(SCAT_U >= 4 && SCAT_U % 4 == 0, "SCAT_U: whole groups of 4");

extern "C" __global__ void __launch_bounds__(256)
scatter_do_det_kernel(const int* __restrict__ inst_path,
                      const int* __restrict__ seg_start,
                      const int* __restrict__ seg_gene, int n_seg,
                      const float* __restrict__ dO, float* __restrict__ c) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (long long sidx = (long long)blockIdx.x * wpb + wib; sidx < n_seg;
       sidx += (long long)gridDim.x * wpb) {
    const int lo = seg_start[sidx], hi = seg_start[sidx + 1];
    const int gene = seg_gene[sidx];
    const float c_old = c[gene];
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    // rem = instances left from this lane's first slot of the round
    // (<= 0: none); the round runs while its lane-0 slot is inside
    int i0 = lo + lane;
    for (int rem = hi - i0; rem + lane > 0;
         rem -= SCAT_U * WAVE, i0 += SCAT_U * WAVE) {
      int ip[SCAT_U];
      float d[SCAT_U];
#pragma unroll
      for (int u = 0; u < SCAT_U; ++u)
        ip[u] = inst_path[i0 + (u * WAVE < rem ? u * WAVE : rem - 1)];
#pragma unroll
      for (int u = 0; u < SCAT_U; ++u) d[u] = dO[ip[u]];
#pragma unroll
      for (int q = 0; q < SCAT_U / 4; ++q) {
        const int k = 4 * q * WAVE;                // group's first slot offset
        const bool full = k + 3 * WAVE < rem;
        p0 = (k < rem) ? p0 + d[4 * q] : p0;
        p1 = full ? p1 + d[4 * q + 1] : p1;
        p0 = (!full && k + WAVE < rem) ? p0 + d[4 * q + 1] : p0;
        p2 = full ? p2 + d[4 * q + 2] : p2;
        p0 = (!full && k + 2 * WAVE < rem) ? p0 + d[4 * q + 2] : p0;
        p3 = full ? p3 + d[4 * q + 3] : p3;
      }
    }
    const float v = wave_sum((p0 + p1) + (p2 + p3));
    if (lane == 0) c[gene] = c_old + v;      // += so slab-blocked passes
                                             // accumulate (c starts zeroed;
                                             // launches are stream-ordered,
                                             // so still deterministic)
  }
}

// Batched scatter_do_det_kernel: c_R [G, R] += X^T dO_R over the same plan.
// Lane <-> instance as in the single kernel, so each inst_path entry is
// loaded once for all replicas; per replica the four unroll accumulators,
// their (p0 + p1) + (p2 + p3) join and the wave_sum tree are the single
// kernel's. Lane r then adds replica r's total into c_R (one coalesced
// R-float row per segment).
template <int NT, bool VEC>
__global__ void __launch_bounds__(256)
scatter_do_rep_kernel(const int* __restrict__ inst_path,
                      const int* __restrict__ seg_start,
                      const int* __restrict__ seg_gene, int n_seg,
                      const float* __restrict__ dO_R, int R,
                      float* __restrict__ c_R) {
  constexpr int NR = NT * 4;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (long long sidx = (long long)blockIdx.x * wpb + wib; sidx < n_seg;
       sidx += (long long)gridDim.x * wpb) {
    const int lo = seg_start[sidx], hi = seg_start[sidx + 1];
    float acc[4][NR];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[q][r] = 0.f;
    int i = lo + lane;
    for (; i + 3 * WAVE < hi; i += 4 * WAVE) {
      int ip[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) ip[q] = inst_path[i + q * WAVE];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4 d[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = rep_gather4<VEC>(dO_R, ip[q], R, t);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[q][4 * t + k] += d[q][k];
      }
    }
    for (; i < hi; i += WAVE) {
      const int ip = inst_path[i];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 d = rep_gather4<VEC>(dO_R, ip, R, t);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[0][4 * t + k] += d[k];
      }
    }
    float mine = 0.f;                          // lane r keeps replica r's sum
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const float v = wave_sum((acc[0][r] + acc[1][r]) +
                               (acc[2][r] + acc[3][r]));
      if (lane == r) mine = v;
    }
    if (lane < R) c_R[(long long)seg_gene[sidx] * R + lane] += mine;
  }
}

// ============================================================== K7: TF1 Adam
// theta -= lr_t * m / (sqrt(v) + eps); lr_t precomputed on host.
// rank-1 variant forms grad[g*h+j] = c[g] * who[j] on the fly (the linear
// CBOW's dW_ih is rank-1, see models/cbow.py) — no G*h grad tensor exists.

extern "C" __global__ void __launch_bounds__(256)
adam_rank1_kernel(float* __restrict__ W, float* __restrict__ m,
                  float* __restrict__ v, const float* __restrict__ c,
                  const float* __restrict__ who, long long G, int h,
                  const float* __restrict__ lr_t_ptr, float b1, float b2,
                  float eps, float* __restrict__ gw_partials) {
  // gw_partials != nullptr: ALSO emit this block's partial of
  // dW_ho = W_pre^T c ([gridDim.x, h] layout) — the fused epilogue reads
  // the pre-update W rows this kernel loads anyway, removing the
  // separate gemv_cols pass (a full W read) and its fold launch.
  // Deterministic: each thread accumulates its own grid-stride rows in
  // order, then fixed ascending-lrow LDS tree per block, then the fold
  // kernel sums blocks ascending.
  const float lr_t = lr_t_ptr[0];   // device-read so hipGraph replays see
                                    // the per-step bias-corrected value
  f32x4* W4 = (f32x4*)W; f32x4* m4 = (f32x4*)m; f32x4* v4 = (f32x4*)v;
  const f32x4* who4 = (const f32x4*)who;
  const int h4 = h / 4;
  // row-major indexing: the flat-index variant paid a 64-bit div+mod per
  // f32x4; here each thread owns a fixed column group and strides over
  // rows (one div/mod per THREAD at setup, multiply-add per iteration)
  const int rpb = blockDim.x / h4;             // rows per block (h <= 1024)
  const int lrow = (int)threadIdx.x / h4;      // this thread's row-in-block
  const int j4 = (int)threadIdx.x - lrow * h4; // and column group
  const f32x4 wj = who4[j4];
  f32x4 gw_acc = {0.f, 0.f, 0.f, 0.f};
  for (long long g = (long long)blockIdx.x * rpb + lrow; g < G;
       g += (long long)gridDim.x * rpb) {
    const long long i = g * h4 + j4;
    const float cg = c[g];
    // W/m/v are pure streams (no reuse inside an epoch): nontemporal
    // ld/st keeps them from evicting the gather tables in the XCD L2s
    f32x4 mm = __builtin_nontemporal_load(&m4[i]);
    f32x4 vv = __builtin_nontemporal_load(&v4[i]);
    f32x4 ww = __builtin_nontemporal_load(&W4[i]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (gw_partials) gw_acc[k] += cg * ww[k];   // pre-update W row
      const float grad = cg * wj[k];
      mm[k] = b1 * mm[k] + (1.f - b1) * grad;
      vv[k] = b2 * vv[k] + (1.f - b2) * grad * grad;
      ww[k] -= lr_t * mm[k] / (sqrtf(vv[k]) + eps);
    }
    __builtin_nontemporal_store(mm, &m4[i]);
    __builtin_nontemporal_store(vv, &v4[i]);
    __builtin_nontemporal_store(ww, &W4[i]);
  }
  if (gw_partials) {
    // per-block fold: slots [rpb][h] in LDS, summed ascending lrow
    __shared__ float gw_slots[256 * 4];          // rpb * h = 1024 floats
    float* slot = gw_slots + (lrow * h4 + j4) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) slot[k] = gw_acc[k];
    __syncthreads();
    if (lrow == 0) {
      f32x4 tot = {0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < rpb; ++r) {
        const float* sl = gw_slots + (r * h4 + j4) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[k] += sl[k];
      }
      float* out = gw_partials + (long long)blockIdx.x * h + j4 * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = tot[k];
    }
  }
}

// fold the adam_rank1 gw partials and apply the TF1-Adam update to W_ho
// in the same launch. One WAVE per column: lanes stride the block
// partials (fixed stride + fixed shuffle tree -> deterministic); the
// single-block variant was latency-bound at ~1k dependent loads/column.
// Lane l sums rows l, l + 64, ... ascending (fold_gw_adam_rep_kernel spells
// the plain loop); the strided row loads are issued FOLD_U at a time before
// their adds — 16 covers the 1024-block cap of the fused launch in one
// round — a slot past n_blocks re-loading the last row and dropped by a
// select. mO/vO/who are fetched ahead of the fold.
#define FOLD_U 16

extern "C" __global__ void __launch_bounds__(256)
fold_gw_adam_kernel(const float* __restrict__ partials, int n_blocks, int h,
                    float* __restrict__ who, float* __restrict__ mO,
                    float* __restrict__ vO,
                    const float* __restrict__ lr_t_ptr, float b1, float b2,
                    float eps) {
  const float lr_t = lr_t_ptr[0];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (int i = blockIdx.x * wpb + wib; i < h; i += gridDim.x * wpb) {
    const float mO_i = mO[i], vO_i = vO[i], who_i = who[i];
    float g = 0.f;
    for (int b0 = lane; b0 - lane < n_blocks; b0 += FOLD_U * WAVE) {
      float pv[FOLD_U];
#pragma unroll
      for (int u = 0; u < FOLD_U; ++u) {
        const int b = b0 + u * WAVE;
        pv[u] = partials[(long long)(b < n_blocks ? b : n_blocks - 1) * h + i];
      }
#pragma unroll
      for (int u = 0; u < FOLD_U; ++u)
        g = (b0 + u * WAVE < n_blocks) ? g + pv[u] : g;
    }
    g = wave_sum(g);
    if (lane == 0) {
      const float mm = b1 * mO_i + (1.f - b1) * g;
      const float vv = b2 * vO_i + (1.f - b2) * g * g;
      mO[i] = mm;
      vO[i] = vv;
      who[i] = who_i - lr_t * mm / (sqrtf(vv) + eps);
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
adam_dense_kernel(float* __restrict__ W, float* __restrict__ m,
                  float* __restrict__ v, const float* __restrict__ grad,
                  long long n, const float* __restrict__ lr_t_ptr, float b1,
                  float b2, float eps) {
  const float lr_t = lr_t_ptr[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const float g = grad[i];
    float mm = b1 * m[i] + (1.f - b1) * g;
    float vv = b2 * v[i] + (1.f - b2) * g * g;
    m[i] = mm; v[i] = vv;
    W[i] -= lr_t * mm / (sqrtf(vv) + eps);
  }
}

// ====================================== general path: row-gather CBOW forward
// One wave per path; h/64 embedding columns per lane (contiguous, vector
// loads); f32 accumulate; H stored for the general backward; loss/acc/dO
// fused into the same pass (the reference recomputed the forward 3x per
// epoch and shipped 2.5 GB/epoch host->device, SURVEY 3.2 — here everything
// is resident and fused).
template <typename WT, int HPL>
__global__ void __launch_bounds__(256)
cbow_fwd_kernel(const WT* __restrict__ W, const float* __restrict__ who,
                const int* __restrict__ genes, const int* __restrict__ offs,
                const float* __restrict__ labels, long long P, float inv_b,
                int h, float* __restrict__ H, float* __restrict__ loss,
                float* __restrict__ correct, float* __restrict__ dO,
                int act) {
  // act: 0 = linear (reference semantics, G2Vec.py:238-240); 1 = ReLU on
  // the hidden vector (opt-in non-linear successor; H stores the
  // PRE-activation so the backward recovers the mask)
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int col0 = lane * HPL;
  for (long long p = (long long)blockIdx.x * wpb + wib; p < P;
       p += (long long)gridDim.x * wpb) {
    const int lo = offs[p], hi = offs[p + 1];
    float acc[HPL];
#pragma unroll
    for (int k = 0; k < HPL; ++k) acc[k] = 0.f;
    for (int i = lo; i < hi; ++i) {
      const long long g = genes[i];
      G2V_ASSERT(g >= 0);
      const WT* row = W + g * (long long)h + col0;
      WT tmp[HPL];
      __builtin_memcpy(tmp, row, HPL * sizeof(WT));  // one wide load
#pragma unroll
      for (int k = 0; k < HPL; ++k) acc[k] += to_f32(tmp[k]);
    }
    float op = 0.f;
    float wv[HPL];
    __builtin_memcpy(wv, who + col0, HPL * sizeof(float));
#pragma unroll
    for (int k = 0; k < HPL; ++k)
      op += (act ? fmaxf(acc[k], 0.f) : acc[k]) * wv[k];
    const float o = wave_sum(op);
    if (H) {
      float* hrow = H + p * (long long)h + col0;
      __builtin_memcpy(hrow, acc, HPL * sizeof(float));
    }
    if (lane == 0) {
      const float y = labels[p];
      loss[p] = sigmoid_ce(o, y);
      correct[p] = is_correct(o, y);
      if (dO) dO[p] = dlogit(o, y, inv_b);
    }
  }
}

// ======================================= general path: dW_ih scatter backward
// Deterministic, atomic-free: instances are pre-sorted by gene (the same
// ScatterPlan as the fast path's c-reduction); one wave per gene segment
// accumulates its instances' dH rows in registers and writes the dW row
// once. dH_p = dO_p * who is recomputed per instance — for a non-linear
// successor, swap that line for a load from a materialized dH[P, h].
// (The v1 atomicAdd-per-touched-row kernel spent 2.1 ms/epoch on hub-gene
// contention at ex_* scale; this is ~100x less.)
template <int HPL>
__global__ void __launch_bounds__(256)
cbow_bwd_rows_det_kernel(const float* __restrict__ who,
                         const int* __restrict__ inst_path,
                         const int* __restrict__ seg_start,
                         const int* __restrict__ seg_gene, int n_seg,
                         const float* __restrict__ dO, int h,
                         float* __restrict__ dW,
                         const float* __restrict__ Hpre) {
  // Hpre != nullptr: ReLU backward — dH_p = dO_p * who (.) 1[Hpre_p > 0]
  // (one extra wide load per instance; linear path passes nullptr)
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int col0 = lane * HPL;
  float wv[HPL];
  __builtin_memcpy(wv, who + col0, HPL * sizeof(float));
  for (long long s = (long long)blockIdx.x * wpb + wib; s < n_seg;
       s += (long long)gridDim.x * wpb) {
    const int lo = seg_start[s], hi = seg_start[s + 1];
    float acc[HPL];
#pragma unroll
    for (int k = 0; k < HPL; ++k) acc[k] = 0.f;
    if (Hpre) {
      for (int i = lo; i < hi; ++i) {
        const long long pi = inst_path[i];
        const float g = dO[pi];
        float hrow[HPL];
        __builtin_memcpy(hrow, Hpre + pi * (long long)h + col0,
                         HPL * sizeof(float));
#pragma unroll
        for (int k = 0; k < HPL; ++k)
          acc[k] += (hrow[k] > 0.f) ? g * wv[k] : 0.f;
      }
    } else {
      for (int i = lo; i < hi; ++i) {
        const float g = dO[inst_path[i]];     // general shape: dH row source
#pragma unroll
        for (int k = 0; k < HPL; ++k) acc[k] += g * wv[k];
      }
    }
    float* row = dW + (long long)seg_gene[s] * h + col0;
    __builtin_memcpy(row, acc, HPL * sizeof(float));
  }
}

// =================================================== K11: per-edge PCC weight
// zt: f32 [G, S] z-scored rows; one wave per edge, lane-strided dot.
// PCC = dot / S; 0-variance genes have zero rows (graph.py) -> pcc 0.
extern "C" __global__ void __launch_bounds__(256)
pcc_edges_kernel(const float* __restrict__ zt, const int* __restrict__ edges,
                 long long E, int S, float inv_s, float* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (long long e = (long long)blockIdx.x * wpb + wib; e < E;
       e += (long long)gridDim.x * wpb) {
    const long long a = edges[2 * e], b = edges[2 * e + 1];
    const float* za = zt + a * S;
    const float* zb = zt + b * S;
    float partial = 0.f;
    for (int i = lane; i < S; i += WAVE) partial += za[i] * zb[i];
    const float d = wave_sum(partial);
    if (lane == 0) out[e] = fabsf(d * inv_s);
  }
}

// ============================================== K11 dense: MFMA f32 corr GEMM
// C = Zt Zt^T / S on v_mfma_f32_16x16x4_f32 (exact f32 at the FP32 matrix
// rate — no xf32 on gfx950, see cdna_hip_programming.md §3). 64x64 tile per
// 4-wave block (each wave one 32x32 sub-tile = 2x2 16x16 fragments), both
// operand tiles staged once in LDS (K = S <= 320 fits the 160 KiB budget).
extern "C" __global__ void __launch_bounds__(256)
corr_gemm_kernel(const float* __restrict__ zt, float* __restrict__ C,
                 int G, int S, int S4, float inv_s) {
#if defined(__gfx950__)
  extern __shared__ float lds[];
  float* At = lds;                 // [64][S4]
  float* Bt = lds + 64 * S4;       // [64][S4]
  const int ntile = (G + 63) / 64;
  const int ti = blockIdx.x / ntile;
  const int tj = blockIdx.x % ntile;
  const int i0 = ti * 64, j0 = tj * 64;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  // stage: each thread strides over the 64 x S4 tiles
  for (int idx = threadIdx.x; idx < 64 * S4; idx += blockDim.x) {
    const int r = idx / S4, k = idx % S4;
    At[idx] = (i0 + r < G && k < S) ? zt[(long long)(i0 + r) * S + k] : 0.f;
    Bt[idx] = (j0 + r < G && k < S) ? zt[(long long)(j0 + r) * S + k] : 0.f;
  }
  __syncthreads();

  const int wr = wid >> 1, wc = wid & 1;       // 2x2 wave grid -> 32x32 each
  f32x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4)(0.f);

  const int fr = lane & 15;                     // fragment row/col lane index
  const int kk = lane >> 4;                     // k sub-index 0..3
  for (int k0 = 0; k0 < S4; k0 += 4) {
    float av[2], bv[2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
      av[a] = At[(wr * 32 + a * 16 + fr) * S4 + k0 + kk];
#pragma unroll
    for (int b = 0; b < 2; ++b)
      bv[b] = Bt[(wc * 32 + b * 16 + fr) * S4 + k0 + kk];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b],
                                                         acc[a][b], 0, 0, 0);
  }
  // C/D map (16x16): col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int ci = i0 + wr * 32 + a * 16 + (lane >> 4) * 4 + reg;
        const int cj = j0 + wc * 32 + b * 16 + (lane & 15);
        if (ci < G && cj < G)
          C[(long long)ci * G + cj] = acc[a][b][reg] * inv_s;
      }
#endif
}

// ============================================== hot-path GEMVs (own kernels)
// rocBLAS gemvn on the tall-skinny [G, h] x [h] shape ran at ~2% of HBM
// bandwidth (18.6 ms for the 1M x 512 s = W_ih @ W_ho). One wave per row,
// h/64 contiguous columns per lane, wave-reduce: HBM-roofline instead.
// clear != nullptr: the row's wave also stores clear[g] = 0.0f. The epoch
// body passes its c buffer: this GEMV runs after Adam, the only reader of
// c, and before the next scatter, so c is zero again without a fill node.
template <int HPL>
__global__ void __launch_bounds__(256)
gemv_rows_kernel(const float* __restrict__ W, const float* __restrict__ x,
                 long long G, int h, float* __restrict__ out,
                 float* __restrict__ clear) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int col0 = lane * HPL;
  float xv[HPL];
  __builtin_memcpy(xv, x + col0, HPL * sizeof(float));
  for (long long g = (long long)blockIdx.x * wpb + wib; g < G;
       g += (long long)gridDim.x * wpb) {
    float acc[HPL];
    __builtin_memcpy(acc, W + g * (long long)h + col0, HPL * sizeof(float));
    float p = 0.f;
#pragma unroll
    for (int k = 0; k < HPL; ++k) p += acc[k] * xv[k];
    const float o = wave_sum(p);
    if (lane == 0) {
      out[g] = o;
      if (clear) clear[g] = 0.0f;
    }
  }
}


// out[j] = sum_g c[g] * W[g, j] (the dW_ho = W_ih^T c reduction): each
// block accumulates a row range into a private [h] partial; a second pass
// folds the partials (atomic-free).
template <int CPT>   // columns per thread = max(1, h/256)
__global__ void __launch_bounds__(256)
gemv_cols_kernel(const float* __restrict__ W, const float* __restrict__ c,
                 long long G, int h, float* __restrict__ partials) {
  const int col0 = threadIdx.x * CPT;
  if (col0 >= h) return;            // h < 256: surplus threads idle
  float acc[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) acc[k] = 0.f;
  const long long rows_per_blk = (G + gridDim.x - 1) / gridDim.x;
  const long long lo = (long long)blockIdx.x * rows_per_blk;
  const long long hi = (lo + rows_per_blk < G) ? lo + rows_per_blk : G;
  for (long long g = lo; g < hi; ++g) {
    const float cg = c[g];
    float wv[CPT];
    __builtin_memcpy(wv, W + g * (long long)h + col0, CPT * sizeof(float));
#pragma unroll
    for (int k = 0; k < CPT; ++k) acc[k] += cg * wv[k];
  }
  float* p = partials + (long long)blockIdx.x * h + col0;
  __builtin_memcpy(p, acc, CPT * sizeof(float));
}

extern "C" __global__ void __launch_bounds__(256)
fold_cols_kernel(const float* __restrict__ partials, int n_blocks, int h,
                 float* __restrict__ out) {
  // one wave per column, lane-strided over the block partials (a serial
  // per-thread loop over ~1k uncoalesced partial rows measured ~150 us)
  const int lane = threadIdx.x & (WAVE - 1);
  const int col = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (col >= h) return;
  float a = 0.f;
  for (int b = lane; b < n_blocks; b += WAVE)
    a += partials[(long long)b * h + col];
  a = wave_sum(a);
  if (lane == 0) out[col] = a;
}

// ============================ replica-batched fused tail and GEMV (see REP_MAX)
// blockIdx.y = replica r over the single launch's per-replica geometry;
// W/m/v [R, G, h], who/mO/vO [R, h], c_R and s_R [G, R] (read / written at
// stride R), gw_partials [R, gridDim.x, h]. The three kernels restate
// adam_rank1_kernel (fused form), fold_gw_adam_kernel and gemv_rows_kernel
// expression by expression, so the compiler contracts the same FMAs and
// each replica's result is bitwise the single kernel's;
// tests/test_gpu_replicates.py holds them to it. They deliberately share no
// body with the single entry points: routed through a common body those
// compiled to the same instructions in another order, so the single
// kernels keep their text and, with it, their instruction streams
// (docs/KERNELS.md).
extern "C" __global__ void __launch_bounds__(256)
adam_rank1_rep_kernel(float* __restrict__ W, float* __restrict__ m,
                      float* __restrict__ v, const float* __restrict__ c_R,
                      const float* __restrict__ who, long long G, int h,
                      int R, const float* __restrict__ lr_t_ptr, float b1,
                      float b2, float eps, float* __restrict__ gw_partials) {
  const long long r = blockIdx.y;
  const float lr_t = lr_t_ptr[0];
  f32x4* W4 = (f32x4*)(W + r * G * h);
  f32x4* m4 = (f32x4*)(m + r * G * h);
  f32x4* v4 = (f32x4*)(v + r * G * h);
  const f32x4* who4 = (const f32x4*)(who + r * h);
  const float* c = c_R + r;
  const int h4 = h / 4;
  const int rpb = blockDim.x / h4;             // rows per block (h <= 1024)
  const int lrow = (int)threadIdx.x / h4;      // this thread's row-in-block
  const int j4 = (int)threadIdx.x - lrow * h4; // and column group
  const f32x4 wj = who4[j4];
  f32x4 gw_acc = {0.f, 0.f, 0.f, 0.f};
  for (long long g = (long long)blockIdx.x * rpb + lrow; g < G;
       g += (long long)gridDim.x * rpb) {
    const long long i = g * h4 + j4;
    const float cg = c[g * R];
    f32x4 mm = __builtin_nontemporal_load(&m4[i]);
    f32x4 vv = __builtin_nontemporal_load(&v4[i]);
    f32x4 ww = __builtin_nontemporal_load(&W4[i]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gw_acc[k] += cg * ww[k];                 // pre-update W row
      const float grad = cg * wj[k];
      mm[k] = b1 * mm[k] + (1.f - b1) * grad;
      vv[k] = b2 * vv[k] + (1.f - b2) * grad * grad;
      ww[k] -= lr_t * mm[k] / (sqrtf(vv[k]) + eps);
    }
    __builtin_nontemporal_store(mm, &m4[i]);
    __builtin_nontemporal_store(vv, &v4[i]);
    __builtin_nontemporal_store(ww, &W4[i]);
  }
  // per-block fold: slots [rpb][h] in LDS, summed ascending lrow
  __shared__ float gw_slots[256 * 4];          // rpb * h = 1024 floats
  float* slot = gw_slots + (lrow * h4 + j4) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) slot[k] = gw_acc[k];
  __syncthreads();
  if (lrow == 0) {
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < rpb; ++q) {
      const float* sl = gw_slots + (q * h4 + j4) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) tot[k] += sl[k];
    }
    float* out = gw_partials + (r * gridDim.x + blockIdx.x) * h + j4 * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = tot[k];
  }
}

extern "C" __global__ void __launch_bounds__(256)
fold_gw_adam_rep_kernel(const float* __restrict__ partials, int n_blocks,
                        int h, float* __restrict__ who,
                        float* __restrict__ mO, float* __restrict__ vO,
                        const float* __restrict__ lr_t_ptr, float b1,
                        float b2, float eps) {
  const long long r = blockIdx.y;
  partials += r * n_blocks * h;
  who += r * h; mO += r * h; vO += r * h;
  const float lr_t = lr_t_ptr[0];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (int i = blockIdx.x * wpb + wib; i < h; i += gridDim.x * wpb) {
    float g = 0.f;
    for (int b = lane; b < n_blocks; b += WAVE)
      g += partials[(long long)b * h + i];
    g = wave_sum(g);
    if (lane == 0) {
      const float mm = b1 * mO[i] + (1.f - b1) * g;
      const float vv = b2 * vO[i] + (1.f - b2) * g * g;
      mO[i] = mm;
      vO[i] = vv;
      who[i] -= lr_t * mm / (sqrtf(vv) + eps);
    }
  }
}

template <int HPL>
__global__ void __launch_bounds__(256)
gemv_rows_rep_kernel(const float* __restrict__ W, const float* __restrict__ x,
                     long long G, int h, int R, float* __restrict__ out) {
  const long long r = blockIdx.y;
  W += r * G * h;
  x += r * h;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  const int col0 = lane * HPL;
  float xv[HPL];
  __builtin_memcpy(xv, x + col0, HPL * sizeof(float));
  for (long long g = (long long)blockIdx.x * wpb + wib; g < G;
       g += (long long)gridDim.x * wpb) {
    float acc[HPL];
    __builtin_memcpy(acc, W + g * (long long)h + col0, HPL * sizeof(float));
    float p = 0.f;
#pragma unroll
    for (int k = 0; k < HPL; ++k) p += acc[k] * xv[k];
    const float o = wave_sum(p);
    if (lane == 0) out[g * R + r] = o;
  }
}

// =============================================================== bf16 cast
extern "C" __global__ void __launch_bounds__(256)
f32_to_bf16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out,
                   long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    out[i] = f32_to_bf16(in[i]);
}

// ======================================================= K9: trunc-normal init
// Seeded device truncated normal (+-2 sigma, rejection-resampled) — the
// reference init semantics (tf.truncated_normal, G2Vec.py:234-235)
// computed entirely on-device: the host rejection loop materialized
// multi-GB intermediates at the 1M x 512 config (round-1 verdict item 6).
// Counter-based: element i draws from its own splitmix64 stream, so the
// result is independent of the launch geometry and bit-stable across
// runs; the CPU oracle (cpu_ref.trunc_normal) mirrors the algorithm.
extern "C" __global__ void trunc_normal_kernel(float* __restrict__ out,
                                               long long n, float std,
                                               uint64_t seed) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i < n; i += stride) {
    uint64_t state =
        seed ^ (uint64_t)((uint64_t)i * 0x94D049BB133111EBULL + 1ULL);
    (void)sm64_next(state);                  // warm draw (stream decorrelation)
    float x;
    do {                                     // P(reject) ~ 4.6%/draw
      const double u1 = u01_from(sm64_next(state));
      const double u2 = u01_from(sm64_next(state));
      // Box-Muller (cosine branch); u1 clamped away from log(0)
      const double r = sqrt(-2.0 * log(u1 > 1e-300 ? u1 : 1e-300));
      x = (float)(r * cos(6.283185307179586 * u2));
    } while (fabsf(x) > 2.0f);
    out[i] = x * std;
  }
}

// ================================= fast path: instance-parallel fused eval
// The subwave-per-path eval kernel is latency-bound: ~21-gene paths give
// each 16-lane group a 2-iteration dependent gather chain and idle lanes
// (26 us over 1.5M instances at ex_* scale). This pair streams the flat
// CSR instance space instead: every lane gathers ONE s value, a 64-lane
// segmented inclusive scan (head flags at path boundaries) produces
// per-path piece sums per 64-instance window, and a thread-per-path
// finish kernel folds each path's <= cap pieces (fixed ascending window
// order -> deterministic), computes correctness counts for the two
// splits, and emits the train split's next-epoch dlogits (same fusion
// as cbow_eval_counts_kernel). Wave windows are aligned: every wave
// covers instances [w*64, w*64+64).
extern "C" __global__ void __launch_bounds__(256)
eval_scan_kernel(const float* __restrict__ s, const int* __restrict__ genes,
                 const int* __restrict__ pathid, const int* __restrict__ offs,
                 long long nnz, int cap, float* __restrict__ piece,
                 int g_lds) {
  // g_lds > 0: the whole s table is staged into LDS once per
  // (persistent, grid-strided) block — random 4-byte s-gathers become
  // ds_read ops instead of 64-way-divergent L1 line lookups, the
  // measured wall of the gather at <= 48 KB tables
  extern __shared__ float s_lds[];
  const float* st = s;
  if (g_lds > 0) {
    for (int g = threadIdx.x; g < g_lds; g += blockDim.x) s_lds[g] = s[g];
    __syncthreads();
    st = s_lds;
  }
  const int lane = threadIdx.x & (WAVE - 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       i - lane < nnz; i += stride) {           // whole wave iterates together
    const bool act = i < nnz;
    const int pid = act ? pathid[i] : -1;
    float val = act ? st[genes[i]] : 0.f;
    const int pid_up = __shfl_up(pid, 1);
    int f = (lane == 0) || (pid != pid_up);     // head of a window piece
    const int head = f;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {        // segmented inclusive scan
      const float tv = __shfl_up(val, o);
      const int tf = __shfl_up(f, o);
      if (lane >= o) {
        if (!f) val += tv;
        f = f | tf;
      }
    }
    const int head_down = __shfl_down(head, 1);
    const bool last = (lane == WAVE - 1) || head_down;
    if (act && last) {
      const long long w = i >> 6;
      const long long w0 = (long long)offs[pid] >> 6;
      piece[(long long)pid * cap + (w - w0)] = val;
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
eval_finish_kernel(const float* __restrict__ piece, const int* __restrict__ offs,
                   const float* __restrict__ labels, long long P,
                   long long p_split, int cap, float* __restrict__ partials,
                   float* __restrict__ dO, float inv_b) {
  float c0 = 0.f, c1 = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       p < P; p += stride) {
    const int lo = offs[p], hi = offs[p + 1];
    const long long w0 = (long long)lo >> 6;
    const long long w1 = ((long long)hi - 1) >> 6;
    float o = 0.f;
    const float* pp = piece + (long long)p * cap;
    for (long long w = w0; w <= w1; ++w) o += pp[w - w0];
    const float y = labels[p];
    const float corr = is_correct(o, y);
    if (p < p_split) {
      c0 += corr;
      if (dO) dO[p] = dlogit(o, y, inv_b);
    } else {
      c1 += corr;
    }
  }
  block_fold2(c0, c1, partials + 2 * blockIdx.x);
}

// ==================================== steps 5-6: L-group k-means and scoring
// Row tile of the wave-per-row kernels below: a lane owns HPL = h/64
// columns as NCH chunks of VEC <= 4 floats, chunk c at column
// (c*64 + lane)*VEC. Every wave instruction then reads 64 consecutive
// 4..16-byte pieces: a fully coalesced global load, and a conflict-free
// ds_read when the row lives in LDS (lane*64 B strides would put four lanes
// of each ds_read_b128 lane group on one bank). Rows must be 16-byte
// aligned (the bindings check the base; h is a multiple of 64): the
// alignment promise is what lets LDS rows move as ds_read/write_b128.
template <int HPL>
__device__ __forceinline__ void row_load(const float* row, int lane,
                                         float (&x)[HPL]) {
  constexpr int VEC = HPL < 4 ? HPL : 4;
  row = (const float*)__builtin_assume_aligned(row, VEC * sizeof(float));
#pragma unroll
  for (int c = 0; c < HPL / VEC; ++c)
    __builtin_memcpy(&x[c * VEC], row + (c * WAVE + lane) * VEC,
                     VEC * sizeof(float));
}

template <int HPL>
__device__ __forceinline__ void row_store(float* row, int lane,
                                          const float (&x)[HPL]) {
  constexpr int VEC = HPL < 4 ? HPL : 4;
  row = (float*)__builtin_assume_aligned(row, VEC * sizeof(float));
#pragma unroll
  for (int c = 0; c < HPL / VEC; ++c)
    __builtin_memcpy(row + (c * WAVE + lane) * VEC, &x[c * VEC],
                     VEC * sizeof(float));
}

// |x - c|^2 as the direct sum of squared differences (no |x|^2 - 2xc + |c|^2
// expansion: dyadic inputs stay exact and nothing cancels)
template <int HPL>
__device__ __forceinline__ float row_dist2(const float (&x)[HPL],
                                           const float (&c)[HPL]) {
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < HPL; ++i) {
    const float d = x[i] - c[i];
    p += d * d;
  }
  return wave_sum(p);
}

#define KM_MAX_K 8
#define KM_PCNT (KM_MAX_K + 1)     // per-block ints: counts[8], n_changed

// One fused Lloyd iteration. One wave per row (two adjacent rows per pass),
// grid-strided. Dynamic LDS,
// 5*k*h floats: the k centroids (block-resident) and one [k][h] sum
// accumulator PER WAVE. A row's label is wave-uniform, so the wave adds the
// row into its own accumulator's label row with plain LDS read-add-write:
// no atomics, and X is read once for assign + update. Counts, n_changed and
// the f64 inertia ride in wave-uniform registers. Epilogue: the 4 waves'
// accumulators are summed in ascending wave order into this block's
// partial; kmeans_fold_kernel folds the blocks. Every order is fixed by
// (G, grid), so a step is bitwise reproducible.
// prev/labels may alias (a row's wave reads prev[g] before writing
// labels[g]); neither is __restrict__.
template <int HPL>
__global__ void __launch_bounds__(256)
kmeans_step_kernel(const float* __restrict__ X, const float* __restrict__ C,
                   const int* prev, int* labels, long long G, int h, int k,
                   float* __restrict__ psums, int* __restrict__ pcnt,
                   double* __restrict__ pinert) {
  extern __shared__ __attribute__((aligned(16))) float km_lds[];
  const int kh = k * h;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = uni(threadIdx.x >> 6);
  const int wpb = blockDim.x >> 6;             // 4: the epilogue assumes it
  float* cen = km_lds;                         // [k][h]
  float* acc = km_lds + (1 + wib) * kh;        // this wave's [k][h]
  for (int i = threadIdx.x; i < kh; i += blockDim.x) cen[i] = C[i];
  for (int i = threadIdx.x; i < wpb * kh; i += blockDim.x)
    km_lds[kh + i] = 0.f;
  __syncthreads();

  int cnt[KM_MAX_K];
#pragma unroll
  for (int j = 0; j < KM_MAX_K; ++j) cnt[j] = 0;
  int changed = 0;
  double inert = 0.0;
  // two adjacent rows per wave and pass: both loads are in flight together
  // and the two rows' reduction chains interleave (one row per pass ran at
  // the latency of load + k shuffle trees, well under the HBM rate)
  for (long long g = ((long long)blockIdx.x * wpb + wib) * 2; g < G;
       g += (long long)gridDim.x * wpb * 2) {
    const bool two = g + 1 < G;                // wave-uniform
    float xa[HPL], xb[HPL], cv[HPL];
    row_load<HPL>(X + g * (long long)h, lane, xa);
    row_load<HPL>(X + (two ? g + 1 : g) * (long long)h, lane, xb);
    float besta = 0.f, bestb = 0.f;
    int ja = 0, jb = 0;
    for (int j = 0; j < k; ++j) {
      row_load<HPL>(cen + j * h, lane, cv);
      const float da = row_dist2<HPL>(xa, cv);
      const float db = row_dist2<HPL>(xb, cv);
      if (j == 0 || da < besta) { besta = da; ja = j; }  // ties: lowest index
      if (j == 0 || db < bestb) { bestb = db; jb = j; }
    }
    ja = uni(ja);
    jb = uni(jb);
    G2V_ASSERT(ja >= 0 && ja < k && jb >= 0 && jb < k);
    float* arow = acc + ja * h;
    row_load<HPL>(arow, lane, cv);
#pragma unroll
    for (int i = 0; i < HPL; ++i) cv[i] += xa[i];
    row_store<HPL>(arow, lane, cv);
#pragma unroll
    for (int j = 0; j < KM_MAX_K; ++j) cnt[j] += (ja == j) ? 1 : 0;
    changed += (prev[g] != ja) ? 1 : 0;
    inert += (double)besta;
    if (lane == 0) labels[g] = ja;
    if (two) {                                 // row g + 1, after row g
      arow = acc + jb * h;
      row_load<HPL>(arow, lane, cv);
#pragma unroll
      for (int i = 0; i < HPL; ++i) cv[i] += xb[i];
      row_store<HPL>(arow, lane, cv);
#pragma unroll
      for (int j = 0; j < KM_MAX_K; ++j) cnt[j] += (jb == j) ? 1 : 0;
      changed += (prev[g + 1] != jb) ? 1 : 0;
      inert += (double)bestb;
      if (lane == 0) labels[g + 1] = jb;
    }
  }
  __syncthreads();                             // all rows in, cen[] is dead

  float* ps = psums + (long long)blockIdx.x * kh;
  for (int i = threadIdx.x; i < kh; i += blockDim.x) {
    const float* a = km_lds + kh + i;
    ps[i] = ((a[0] + a[kh]) + a[2 * kh]) + a[3 * kh];
  }
  // the wave scalars go through the dead centroid region (kh >= 64 floats;
  // 4 doubles + 4*9 ints = 44): the block may own all 160 KiB of LDS as
  // dynamic memory (k*h = 8192), which leaves no room for a static array
  double* sd = (double*)cen;                   // [4]
  int* si = (int*)cen + 2 * 4;                 // [4][KM_PCNT]
  if (lane == 0) {
    sd[wib] = inert;
#pragma unroll
    for (int j = 0; j < KM_MAX_K; ++j) si[wib * KM_PCNT + j] = cnt[j];
    si[wib * KM_PCNT + KM_MAX_K] = changed;
  }
  __syncthreads();
  if (threadIdx.x < KM_PCNT) {
    const int j = threadIdx.x;
    pcnt[(long long)blockIdx.x * KM_PCNT + j] =
        si[j] + si[KM_PCNT + j] + si[2 * KM_PCNT + j] + si[3 * KM_PCNT + j];
  }
  if (threadIdx.x == KM_PCNT)
    pinert[blockIdx.x] = ((sd[0] + sd[1]) + sd[2]) + sd[3];
}

// Folds the per-block partials of kmeans_step_kernel. One wave per sums
// element, like fold_cols_kernel: lane l takes blocks l, l+64, ... in
// ascending order, then the fixed shuffle tree. The element's wave also
// folds its cluster's count and writes C' = sum / float(count) in fp32 (an
// empty cluster keeps its old row); wave 0 folds n_changed and the f64
// inertia. C_new may alias C_old: element e is read and written by the same
// lane.
extern "C" __global__ void __launch_bounds__(256)
kmeans_fold_kernel(const float* __restrict__ psums,
                   const int* __restrict__ pcnt,
                   const double* __restrict__ pinert, int n_blocks, int k,
                   int h, const float* C_old, float* C_new,
                   float* __restrict__ sums, int* __restrict__ counts,
                   int* __restrict__ n_changed, double* __restrict__ inertia) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wpb = blockDim.x >> 6;
  const int kh = k * h;
  for (int e = blockIdx.x * wpb + (threadIdx.x >> 6); e < kh;
       e += gridDim.x * wpb) {
    const int j = e / h;
    float s = 0.f;
    int c = 0;
    for (int b = lane; b < n_blocks; b += WAVE) {
      s += psums[(long long)b * kh + e];
      c += pcnt[(long long)b * KM_PCNT + j];
    }
    s = wave_sum(s);
    c = wave_sum(c);
    if (lane == 0) {
      sums[e] = s;
      C_new[e] = (c > 0) ? s / (float)c : C_old[e];
      if (e == j * h) counts[j] = c;
    }
    if (e == 0) {
      int ch = 0;
      double in = 0.0;
      for (int b = lane; b < n_blocks; b += WAVE) {
        ch += pcnt[(long long)b * KM_PCNT + KM_MAX_K];
        in += pinert[b];
      }
      ch = wave_sum(ch);
      in = wave_sum(in);
      if (lane == 0) { n_changed[0] = ch; inertia[0] = in; }
    }
  }
}

// k-means++ D^2 sampling support: d2[g] = min(d2[g], |x_g - c|^2) for one
// new centre c[h] (same row tile and distance as kmeans_step_kernel).
template <int HPL>
__global__ void __launch_bounds__(256)
kmeans_mind2_kernel(const float* __restrict__ X, const float* __restrict__ c,
                    long long G, int h, float* __restrict__ d2) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  float cv[HPL];
  row_load<HPL>(c, lane, cv);
  for (long long g = (long long)blockIdx.x * wpb + wib; g < G;
       g += (long long)gridDim.x * wpb) {
    float x[HPL];
    row_load<HPL>(X + g * (long long)h, lane, x);
    const float d = row_dist2<HPL>(x, cv);
    if (lane == 0) d2[g] = fminf(d2[g], d);
  }
}

// d-score: out[g] = sqrt(sum_j W[g, j]^2), accumulated in f64 and rounded
// to fp32 once.
template <int HPL>
__global__ void __launch_bounds__(256)
row_norms_kernel(const float* __restrict__ W, long long G, int h,
                 float* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (long long g = (long long)blockIdx.x * wpb + wib; g < G;
       g += (long long)gridDim.x * wpb) {
    float x[HPL];
    row_load<HPL>(W + g * (long long)h, lane, x);
    double p = 0.0;
#pragma unroll
    for (int i = 0; i < HPL; ++i) p += (double)x[i] * (double)x[i];
    p = wave_sum(p);
    if (lane == 0) out[g] = (float)sqrt(p);
  }
}

// t-score: |pooled-variance two-sample t| per gene column of expr[S, G]
// (row-major, samples x genes), label 0 (good) vs 1 (poor); other labels
// are left out. One THREAD per gene, so each sample row is a coalesced read
// across genes. Two passes over the column in f64: group means, then the
// sums of squared deviations; then the formula of scoring.t_scores. 0 when
// d1 <= 0 or a group has fewer than 2 samples. Sample labels are staged in
// LDS tile by tile (any S) and read as broadcasts.
#define TS_TILE 1024

extern "C" __global__ void __launch_bounds__(256)
t_scores_kernel(const float* __restrict__ expr, const int* __restrict__ labels,
                int S, long long G, float* __restrict__ out) {
  __shared__ int lab[TS_TILE];
  for (long long g0 = (long long)blockIdx.x * blockDim.x; g0 < G;
       g0 += (long long)gridDim.x * blockDim.x) {
    const long long g = g0 + threadIdx.x;
    const bool act = g < G;
    int n0 = 0, n1 = 0;
    double m0 = 0.0, m1 = 0.0, q0 = 0.0, q1 = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      double a0 = 0.0, a1 = 0.0;
      for (int t0 = 0; t0 < S; t0 += TS_TILE) {
        const int nt = (S - t0 < TS_TILE) ? S - t0 : TS_TILE;
        __syncthreads();                       // readers of the last tile done
        for (int i = threadIdx.x; i < nt; i += blockDim.x)
          lab[i] = labels[t0 + i];
        __syncthreads();
        if (act) {
          const float* col = expr + (long long)t0 * G + g;
#pragma unroll 4
          for (int i = 0; i < nt; ++i) {
            const int l = lab[i];
            const double v = (double)col[(long long)i * G];
            if (pass == 0) {
              a0 += (l == 0) ? v : 0.0;
              a1 += (l == 1) ? v : 0.0;
              n0 += (l == 0) ? 1 : 0;
              n1 += (l == 1) ? 1 : 0;
            } else {
              const double d0 = v - m0, d1 = v - m1;
              a0 += (l == 0) ? d0 * d0 : 0.0;
              a1 += (l == 1) ? d1 * d1 : 0.0;
            }
          }
        }
      }
      if (pass == 0) {
        m0 = (n0 > 0) ? a0 / (double)n0 : 0.0;
        m1 = (n1 > 0) ? a1 / (double)n1 : 0.0;
      } else {
        q0 = a0;
        q1 = a1;
      }
    }
    if (act) {
      float t = 0.f;
      if (n0 >= 2 && n1 >= 2) {
        const double nx = (double)n0, ny = (double)n1;
        const double sx = sqrt(q0 / (nx - 1.0)), sy = sqrt(q1 / (ny - 1.0));
        const double d1 = sqrt(((nx - 1.0) * sx * sx + (ny - 1.0) * sy * sy) /
                               (nx + ny - 2.0));
        const double d2 = sqrt(1.0 / nx + 1.0 / ny);
        if (d1 > 0.0) t = (float)fabs((m0 - m1) / d1 / d2);
      }
      out[g] = t;
    }
  }
}

// ===================================== rank statistics: average ranks, rank sum
// For gene column g of expr[S, G] and sample i, the doubled average rank is
// the integer
//   R2 = 2 * #{j : x_j < x_i} + #{j : x_j == x_i} + 1
//      = 1 + sum_j ((x_j < x_i) + (x_j <= x_i))          (self included)
// with IEEE compares (-0.0 ties +0.0, +-inf are ordinary values; NaN is
// refused by the caller). rank = R2 / 2 is a half-integer <= S: exact in f32
// for S < 2^23.
//
// One body for the two kernels below. A 256-thread block owns RK_TG = 64
// consecutive genes, lane l of every wave on gene g0 + l, so each sample row
// piece is one coalesced 256-byte read and no cross-lane step exists. Wave w
// keeps RK_IB of its own x_i in registers (samples i0 + w * RK_IB + b of the
// current i-pass of RK_IB * RK_WAVES samples) and walks j over a
// [RK_SJ samples][RK_TG genes] LDS tile: tile[j * RK_TG + lane] is one
// conflict-free ds_read_b32 that feeds RK_IB compare pairs. S is arbitrary:
// a column longer than RK_SJ is walked j-tile by j-tile, re-staged for every
// i-pass (the re-read hits L2: 1 staged element per RK_IB * RK_WAVES pair
// tests); a column that fits is staged once per gene tile. 32 KiB of LDS per
// block. Gene tiles are grid-strided.
//
// SCORES = false writes ranks[i, g] = 0.5f * R2.
// SCORES = true writes no ranks: per gene it sums, as 64-bit INTEGERS,
//   w2 = sum_i R2_i * m_i         ( = 2 W1, m = labels, 0/1 only)
//   q4 = sum_i (R2_i - (S + 1))^2 ( = 4 SSR, tie-corrected by construction)
// per wave, folds the RK_WAVES partials through LDS (integer adds: any order
// gives the same bits) and finishes in f64 with one rounding to f32:
//   z   = |w2/2 - n1 (S+1)/2| / sqrt(n1 n0 / (S (S-1)) * q4/4)
//   auc = (w2/2 - n1 (n1+1)/2) / (n1 n0)
// z = 0 and auc = 0.5 when q4 == 0 or a group has fewer than 2 samples (the
// rule of t_scores_kernel). q4 <= S^3 / 3 fits int64 for S <= 2^21, which the
// binding enforces for this entry point.
#define RK_TG 64                   // genes per block tile (one wave wide)
#define RK_SJ 128                  // samples per staged j-tile
#define RK_IB 8                    // x_i held in registers per wave
#define RK_WAVES 4
#define RK_MAX_BLOCKS 16384        // grid cap; further gene tiles are strided

template <bool SCORES>
__device__ __forceinline__ void rank_body(
    const float* __restrict__ expr, const int* __restrict__ labels, int S,
    long long G, int n1, float* __restrict__ ranks, float* __restrict__ z,
    float* __restrict__ auc) {
  __shared__ float tile[RK_SJ * RK_TG];
  __shared__ long long fold[SCORES ? 2 * RK_WAVES * RK_TG : 1];
  const int lane = threadIdx.x & (WAVE - 1);
  const int w = uni(threadIdx.x >> 6);
  const bool one_tile = S <= RK_SJ;
  const long long n_gt = (G + RK_TG - 1) / RK_TG;
  for (long long gt = blockIdx.x; gt < n_gt; gt += gridDim.x) {
    const long long g = gt * RK_TG + lane;
    const bool act = g < G;
    const long long gc = act ? g : G - 1;      // dead lanes re-read the last gene
    long long w2 = 0, q4 = 0;
    for (int i0 = 0; i0 < S; i0 += RK_IB * RK_WAVES) {
      const int iw = i0 + w * RK_IB;           // this wave's first sample
      float xi[RK_IB];
      int r2[RK_IB];
#pragma unroll
      for (int b = 0; b < RK_IB; ++b) {
        const int ic = (iw + b < S) ? iw + b : S - 1;
        G2V_ASSERT(ic >= 0 && ic < S && gc >= 0 && gc < G);
        xi[b] = expr[(long long)ic * G + gc];
        r2[b] = 1;
      }
      for (int t0 = 0; t0 < S; t0 += RK_SJ) {
        const int nt = (S - t0 < RK_SJ) ? S - t0 : RK_SJ;
        if (!one_tile || i0 == 0) {
          __syncthreads();                     // readers of the last tile done
          for (int j = w; j < nt; j += RK_WAVES) {
            G2V_ASSERT(t0 + j < S && j * RK_TG + lane < RK_SJ * RK_TG);
            tile[j * RK_TG + lane] = expr[(long long)(t0 + j) * G + gc];
          }
          __syncthreads();
        }
        if (iw < S) {                          // wave-uniform
#pragma unroll 4
          for (int j = 0; j < nt; ++j) {
            const float v = tile[j * RK_TG + lane];
#pragma unroll
            for (int b = 0; b < RK_IB; ++b)
              r2[b] += (int)(v < xi[b]) + (int)(v <= xi[b]);
          }
        }
      }
#pragma unroll
      for (int b = 0; b < RK_IB; ++b) {
        const int i = iw + b;
        if (i < S) {                           // wave-uniform
          G2V_ASSERT(r2[b] >= 2 && r2[b] <= 2 * S);
          if (SCORES) {
            const long long d = (long long)r2[b] - ((long long)S + 1);
            w2 += labels[i] ? (long long)r2[b] : 0LL;
            q4 += d * d;
          } else if (act) {
            ranks[(long long)i * G + g] = 0.5f * (float)r2[b];
          }
        }
      }
    }
    if (SCORES) {
      __syncthreads();                         // the last fold's reader is done
      fold[w * RK_TG + lane] = w2;
      fold[(RK_WAVES + w) * RK_TG + lane] = q4;
      __syncthreads();
      if (w == 0 && act) {
        long long W2 = 0, Q4 = 0;
#pragma unroll
        for (int k = 0; k < RK_WAVES; ++k) {
          W2 += fold[k * RK_TG + lane];
          Q4 += fold[(RK_WAVES + k) * RK_TG + lane];
        }
        const double n1d = (double)n1, n0d = (double)(S - n1), Sd = (double)S;
        float zf = 0.f, af = 0.5f;
        if (Q4 > 0 && n1 >= 2 && S - n1 >= 2) {
          const double W1 = 0.5 * (double)W2;
          const double var = n1d * n0d / (Sd * (Sd - 1.0)) * (0.25 * (double)Q4);
          zf = (float)(fabs(W1 - 0.5 * n1d * (Sd + 1.0)) / sqrt(var));
          af = (float)((W1 - 0.5 * n1d * (n1d + 1.0)) / (n1d * n0d));
        }
        z[g] = zf;
        auc[g] = af;
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(256)
rank_columns_kernel(const float* __restrict__ expr, int S, long long G,
                    float* __restrict__ ranks) {
  rank_body<false>(expr, nullptr, S, G, 0, ranks, nullptr, nullptr);
}

extern "C" __global__ void __launch_bounds__(256)
ranksum_scores_kernel(const float* __restrict__ expr,
                      const int* __restrict__ labels, int S, long long G,
                      int n1, float* __restrict__ z, float* __restrict__ auc) {
  rank_body<true>(expr, labels, S, G, n1, nullptr, z, auc);
}

// ============================== step 6: label-permutation null of the pooled t
// For a 0/1 mask m over the S samples (poor group m == 1, n1 = sum m,
// n0 = S - n1) and gene g of expr[S, G]:
//   s1 = sum_s x m      q1 = sum_s (x x) m     f32 accumulate (MFMA)
//   T  = sum_s x        Q  = sum_s (x x)       f64 accumulate of the f32 values
//   s0 = T - s1, q0 = Q - q1                   f64 from here on
//   ss = (q1 - s1 s1 / n1) + (q0 - s0 s0 / n0),  pooled = ss / (S - 2)
//   d  = s0 / n0 - s1 / n1
//   stat = pooled > 0 ? d d / pooled / (1/n1 + 1/n0) : 0          ( = t^2 )
// A relabelling EXCEEDS when stat >= stat_obs * (1 - 2^-30): the factor only
// merges values equal in exact arithmetic but ulps apart in evaluation.

// T and Q per gene column. One THREAD per gene (each sample row a coalesced
// read, as in t_scores_kernel); x*x is one f32 multiply, like the q1 operand.
extern "C" __global__ void __launch_bounds__(256)
col_moments_kernel(const float* __restrict__ expr, int S, long long G,
                   double* __restrict__ T, double* __restrict__ Q) {
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < G;
       g += (long long)gridDim.x * blockDim.x) {
    double t = 0.0, q = 0.0;
    const float* col = expr + g;
#pragma unroll 4
    for (int s = 0; s < S; ++s) {
      const float v = col[(long long)s * G];
      const float v2 = v * v;
      t += (double)v;
      q += (double)v2;
    }
    T[g] = t;
    Q[g] = q;
  }
}

#define PT_TILE 64                 // genes x relabellings per block
#define PT_KC 64                   // samples per LDS-staged K chunk
#define PT_NLD (PT_TILE * PT_KC / 256)   // staged elements per thread and tile
#define PT_LDX (PT_TILE + 16)      // x tile [k][gene]: stride = 16 mod 32 banks
#define PT_LDM (PT_KC + 2)         // mask tile [relabelling][k]: stride = 2 mod 32

__device__ __forceinline__ double perm_t_stat(double s1, double q1, double T,
                                              double Q, double n1, double n0,
                                              double dof, double inv_n) {
  const double s0 = T - s1, q0 = Q - q1;
  const double ss = (q1 - s1 * s1 / n1) + (q0 - s0 * s0 / n0);
  const double pooled = ss / dof;
  const double d = s0 / n0 - s1 / n1;
  return pooled > 0.0 ? d * d / pooled / inv_n : 0.0;
}

// One body for the two entry points below, so the stat of a (gene, mask)
// pair is the same code and the same bits in both modes.
// 64 genes x 64 relabellings per 256-thread block; wave w owns the 32x32
// sub-tile (w>>1, w&1) as 2x2 fragments of v_mfma_f32_16x16x4_f32, each with
// an s1 and a q1 accumulator (8 independent MFMA chains per wave). The q1
// A-operand is av*av formed in-register: no x^2 tile anywhere. K runs over S
// in PT_KC-sample chunks staged in LDS (x tile k-major, as expr rows are
// gene-contiguous; u8 masks widened to f32 once, at the stage), zero-padded
// to a multiple of 4. The global loads of the NEXT chunk (or of the next
// relabelling tile's first chunk) are issued into registers before the MFMA
// loop of the current one and land in LDS after it, so their latency hides
// behind the matrix work. blockIdx.x is the gene tile; the block walks the
// relabelling tiles blockIdx.y, +gridDim.y, ...
// stat_out != null: stats mode, stat_out[b, g] = stat.
// else counts mode: counts[g] += #{b : stat >= thr_g}, maxstat[b] =
// max(maxstat[b], max_g stat) through integer atomics (order-independent;
// non-negative doubles order like their u64 bit patterns), both zeroed by
// the host first.
__device__ __forceinline__ void
perm_t_body(const float* __restrict__ expr, const uint8_t* __restrict__ masks,
            const double* __restrict__ T, const double* __restrict__ Q,
            const double* __restrict__ stat_obs, int S, long long G,
            long long B, int n1i, double* __restrict__ stat_out,
            int* __restrict__ counts,
            unsigned long long* __restrict__ maxstat) {
#if defined(__gfx950__)
  __shared__ float Xs[PT_KC * PT_LDX];
  __shared__ float Ms[PT_TILE * PT_LDM];
  __shared__ double Tq[3][PT_TILE];            // T, Q, exceed threshold

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, kk = lane >> 4;
  const long long g0 = (long long)blockIdx.x * PT_TILE;
  const double n1 = (double)n1i, n0 = (double)(S - n1i);
  const double dof = (double)(S - 2), inv_n = 1.0 / n1 + 1.0 / n0;

  if (threadIdx.x < PT_TILE) {
    const long long g = g0 + threadIdx.x;
    const bool in = g < G;
    Tq[0][threadIdx.x] = in ? T[g] : 0.0;
    Tq[1][threadIdx.x] = in ? Q[g] : 0.0;
    Tq[2][threadIdx.x] =
        (in && stat_obs) ? stat_obs[g] * (1.0 - 0x1p-30) : 0.0;
  }

  int cnt[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) cnt[a][r] = 0;

  // staging registers: element (hi, lo) = (4 * i + wid, lane) of the 64 x 64
  // chunk; hi is the sample of the x tile and the relabelling of the mask
  // tile, lo the gene resp. the sample. Out-of-range elements load as zero.
  float xr[PT_NLD];
  uint8_t mr[PT_NLD];
  auto prefetch = [&](long long pb0, int ps0) {
#pragma unroll
    for (int i = 0; i < PT_NLD; ++i) {
      const int hi = 4 * i + wid;
      xr[i] = (ps0 + hi < S && g0 + lane < G)
          ? expr[(long long)(ps0 + hi) * G + g0 + lane] : 0.f;
      mr[i] = (pb0 + hi < B && ps0 + lane < S)
          ? masks[(pb0 + hi) * S + ps0 + lane] : (uint8_t)0;
    }
  };

  const long long nbt = (B + PT_TILE - 1) / PT_TILE;
  if ((long long)blockIdx.y < nbt) prefetch((long long)blockIdx.y * PT_TILE, 0);
  for (long long bt = blockIdx.y; bt < nbt; bt += gridDim.y) {
    const long long b0 = bt * PT_TILE;
    f32x4 acs[2][2], acq[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        acs[a][b] = (f32x4)(0.f);
        acq[a][b] = (f32x4)(0.f);
      }

    for (int s0 = 0; s0 < S; s0 += PT_KC) {
      const int kc = (S - s0 < PT_KC) ? S - s0 : PT_KC;
      const int kc4 = (kc + 3) & ~3;
      __syncthreads();                   // readers of the last chunk done
#pragma unroll
      for (int i = 0; i < PT_NLD; ++i) {
        const int hi = 4 * i + wid;
        Xs[hi * PT_LDX + lane] = xr[i];
        Ms[hi * PT_LDM + lane] = (float)mr[i];
      }
      __syncthreads();
      if (s0 + PT_KC < S)
        prefetch(b0, s0 + PT_KC);
      else if (bt + gridDim.y < nbt)
        prefetch((bt + gridDim.y) * PT_TILE, 0);
      for (int k0 = 0; k0 < kc4; k0 += 4) {
        float av[2], aq[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          av[a] = Xs[(k0 + kk) * PT_LDX + wr * 32 + a * 16 + fr];
          aq[a] = av[a] * av[a];
        }
#pragma unroll
        for (int b = 0; b < 2; ++b)
          bv[b] = Ms[(wc * 32 + b * 16 + fr) * PT_LDM + k0 + kk];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            acs[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                av[a], bv[b], acs[a][b], 0, 0, 0);
            acq[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                aq[a], bv[b], acq[a][b], 0, 0, 0);
          }
      }
    }

    // C/D map (16x16): col = lane&15 (relabelling), row = (lane>>4)*4 + reg
    // (gene). Padded genes and relabellings are computed and dropped here.
    double cmax[2] = {0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gl = wr * 32 + a * 16 + kk * 4 + reg;
        const bool g_in = g0 + gl < G;
        const double Tg = Tq[0][gl], Qg = Tq[1][gl], thr = Tq[2][gl];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const long long bb = b0 + wc * 32 + b * 16 + fr;
          const double st = perm_t_stat((double)acs[a][b][reg],
                                        (double)acq[a][b][reg], Tg, Qg, n1,
                                        n0, dof, inv_n);
          const bool live = g_in && bb < B;
          if (stat_out) {
            if (live) stat_out[bb * G + g0 + gl] = st;
          } else {
            cnt[a][reg] += (live && st >= thr) ? 1 : 0;
            cmax[b] = (live && st > cmax[b]) ? st : cmax[b];
          }
        }
      }
    if (!stat_out) {
      // column max: over the 4 lane groups that hold one relabelling
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        double m = cmax[b];
        m = fmax(m, __shfl_xor(m, 16));
        m = fmax(m, __shfl_xor(m, 32));
        const long long bb = b0 + wc * 32 + b * 16 + fr;
        if (kk == 0 && bb < B && m > 0.0)
          atomicMax(&maxstat[bb], (unsigned long long)__double_as_longlong(m));
      }
    }
  }
  if (!stat_out) {
    // exceed counts: over the 16 lanes that share a gene row
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        int c = cnt[a][reg];
        for (int o = 1; o < 16; o <<= 1) c += __shfl_xor(c, o);
        const long long g = g0 + wr * 32 + a * 16 + kk * 4 + reg;
        if (fr == 0 && g < G && c) atomicAdd(&counts[g], c);
      }
  }
#endif
}

extern "C" __global__ void __launch_bounds__(256)
perm_t_stats_kernel(const float* __restrict__ expr,
                    const uint8_t* __restrict__ masks,
                    const double* __restrict__ T, const double* __restrict__ Q,
                    int S, long long G, long long B, int n1,
                    double* __restrict__ stat_out) {
  perm_t_body(expr, masks, T, Q, nullptr, S, G, B, n1, stat_out, nullptr,
              nullptr);
}

extern "C" __global__ void __launch_bounds__(256)
perm_t_counts_kernel(const float* __restrict__ expr,
                     const uint8_t* __restrict__ masks,
                     const double* __restrict__ T, const double* __restrict__ Q,
                     const double* __restrict__ stat_obs, int S, long long G,
                     long long B, int n1, int* __restrict__ counts,
                     unsigned long long* __restrict__ maxstat) {
  perm_t_body(expr, masks, T, Q, stat_obs, S, G, B, n1, nullptr, counts,
              maxstat);
}

// ===================================== nearest genes: fused MFMA GEMM + top-k
// For every query row q of Xq f32[Q, h]: the k candidates g of X f32[G, h]
// with the largest dot(Xq[q], X[g]), g != q_index[q], in the TOTAL order
// "value descending, equal values by ascending candidate index" (-0.0 ==
// +0.0 is a tie). The dot is the MFMA's k-ordered f32 chain. Nothing of size
// Q x G is written: a score tile lives in LDS just long enough to be
// compared with each row's current k-th entry.
//
// The selection keeps a row's sorted list one entry per lane of a wave
// (k <= 64; all 64 lanes hold entries, the first k are the result). Empty
// entries are (-inf, KN_EMPTY): every real candidate is ahead of them. As
// the order is total and candidate indices are distinct, the top k of a set
// do not depend on the order of the inserts or on how the candidates were
// split over blocks: results are bitwise equal for every launch split.
#define KN_TILE 64                 // queries x candidates per block and tile
#define KN_KC 64                   // columns of h per LDS-staged K chunk
#define KN_LD (KN_KC + 2)          // operand tiles [row][k]: stride = 2 mod 32
#define KN_LDS (KN_TILE + 4)       // score tile [query][cand]: 4 rows = 16 mod 32
#define KN_NLD (KN_TILE * KN_KC / 4 / 256)   // staged float4 per thread and tile
#define KN_EMPTY 0x7fffffff

__device__ __forceinline__ bool knn_ahead(float av, int ai, float bv, int bi) {
  return av > bv || (av == bv && ai < bi);
}

// The value a wave-uniform lane l holds: v_readlane_b32, no trip through
// the LDS crossbar as __shfl (ds_bpermute) takes.
__device__ __forceinline__ int knn_lane(int v, int l) {
  return __builtin_amdgcn_readlane(v, l);
}
__device__ __forceinline__ float knn_lane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Offer every lane's candidate (v, g), live where pend, to the list
// (lv, li). A ballot of zero against the k-th entry is the common case; the
// survivors go in one at a time: position = number of entries ahead of the
// candidate (a prefix, the list is sorted), entries behind it move up a lane.
__device__ __forceinline__ void knn_insert(float& lv, int& li, float v, int g,
                                           bool pend, int k, int lane) {
  float tv = knn_lane(lv, k - 1);
  int ti = knn_lane(li, k - 1);
  pend = pend && knn_ahead(v, g, tv, ti);
  unsigned long long m = __ballot(pend);
  while (m) {
    const int b = __ffsll(m) - 1;
    const float cv = knn_lane(v, b);
    const int cg = knn_lane(g, b);
    const int p = __popcll(__ballot(knn_ahead(lv, li, cv, cg)));
    const float uv = __shfl_up(lv, 1);
    const int ui = __shfl_up(li, 1);
    if (lane == p) {
      lv = cv;
      li = cg;
    } else if (lane > p) {
      lv = uv;
      li = ui;
    }
    tv = knn_lane(lv, k - 1);
    ti = knn_lane(li, k - 1);
    pend = pend && lane != b && knn_ahead(v, g, tv, ti);
    m = __ballot(pend);
  }
}

// 64 queries (blockIdx.x) against the candidate tiles blockIdx.y,
// +gridDim.y, ...; wave w owns the 32x32 sub-tile (w>>1, w&1) as 2x2
// fragments of v_mfma_f32_16x16x4_f32, A = queries, B = candidates (both
// rows x K with K contiguous: the stage is 16-byte loads, 16 lanes per row).
// K runs over h in KN_KC chunks, zero-filled past h; the loads of the next
// chunk (or of the next tile's first) are issued into registers before the
// MFMA loop and land in LDS after it. After a tile's last chunk the scores
// go to LDS over the dead operand tiles and wave w selects for query rows
// 16w .. 16w+15, one candidate per lane.
// out_idx / out_val are [Q, gridDim.y, k]: the final result when
// gridDim.y == 1, else the partial lists knn_merge_kernel folds.
extern "C" __global__ void __launch_bounds__(256)
knn_tile_kernel(const float* __restrict__ Xq, const float* __restrict__ X,
                const int* __restrict__ q_index, long long Q, long long G,
                int h, int k, int* __restrict__ out_idx,
                float* __restrict__ out_val) {
#if defined(__gfx950__)
  __shared__ __attribute__((aligned(16))) float lds[2 * KN_TILE * KN_LD];
  float* As = lds;
  float* Bs = lds + KN_TILE * KN_LD;
  float* Sc = lds;                             // [64][KN_LDS] <= both tiles

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, kk = lane >> 4;
  const long long q0 = (long long)blockIdx.x * KN_TILE;

  // lane r < 16 holds the excluded candidate of query row 16 * wid + r
  int self_r = -1;
  if (q_index && lane < 16 && q0 + 16 * wid + lane < Q)
    self_r = q_index[q0 + 16 * wid + lane];

  float lv[16];
  int li[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    lv[r] = -INFINITY;
    li[r] = KN_EMPTY;
  }

  // staging registers: float4 (row, c4) = (16 * i + tid / 16, tid % 16) of
  // the 64 x 64 chunk of either operand. h % 4 == 0, so a float4 lies
  // entirely inside a row or entirely past it.
  f32x4 ar[KN_NLD], br[KN_NLD];
  const int srow = threadIdx.x >> 4, sc4 = (threadIdx.x & 15) * 4;
  auto prefetch = [&](long long pc0, int pk0) {
#pragma unroll
    for (int i = 0; i < KN_NLD; ++i) {
      const int row = 16 * i + srow;
      const bool kin = pk0 + sc4 < h;
      ar[i] = (kin && q0 + row < Q)
          ? *(const f32x4*)(Xq + (q0 + row) * h + pk0 + sc4) : (f32x4)(0.f);
      br[i] = (kin && pc0 + row < G)
          ? *(const f32x4*)(X + (pc0 + row) * h + pk0 + sc4) : (f32x4)(0.f);
    }
  };

  const long long nct = (G + KN_TILE - 1) / KN_TILE;
  if ((long long)blockIdx.y < nct) prefetch((long long)blockIdx.y * KN_TILE, 0);
  for (long long ct = blockIdx.y; ct < nct; ct += gridDim.y) {
    const long long c0 = ct * KN_TILE;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4)(0.f);

    for (int k0 = 0; k0 < h; k0 += KN_KC) {
      const int kc = (h - k0 < KN_KC) ? h - k0 : KN_KC;    // multiple of 4
      __syncthreads();          // readers of the last chunk / score tile done
#pragma unroll
      for (int i = 0; i < KN_NLD; ++i) {
        float* pa = As + (16 * i + srow) * KN_LD + sc4;    // 8-byte aligned
        float* pb = Bs + (16 * i + srow) * KN_LD + sc4;
        pa[0] = ar[i][0]; pa[1] = ar[i][1]; pa[2] = ar[i][2]; pa[3] = ar[i][3];
        pb[0] = br[i][0]; pb[1] = br[i][1]; pb[2] = br[i][2]; pb[3] = br[i][3];
      }
      __syncthreads();
      if (k0 + KN_KC < h)
        prefetch(c0, k0 + KN_KC);
      else if (ct + gridDim.y < nct)
        prefetch((ct + gridDim.y) * KN_TILE, 0);
      for (int kq = 0; kq < kc; kq += 4) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
          av[a] = As[(wr * 32 + a * 16 + fr) * KN_LD + kq + kk];
#pragma unroll
        for (int b = 0; b < 2; ++b)
          bv[b] = Bs[(wc * 32 + b * 16 + fr) * KN_LD + kq + kk];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }

    // C/D map (16x16): col = lane&15 (candidate), row = (lane>>4)*4 + reg
    // (query). Padded rows and candidates are computed and masked below.
    __syncthreads();                     // operand tiles dead in every wave
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          Sc[(wr * 32 + a * 16 + kk * 4 + reg) * KN_LDS + wc * 32 + b * 16 +
             fr] = acc[a][b][reg];
    __syncthreads();

    const long long g = c0 + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 16 * wid + r;
      const int self = knn_lane(self_r, r);
      const bool live = q0 + row < Q && g < G && g != (long long)self;
      knn_insert(lv[r], li[r], Sc[row * KN_LDS + lane], (int)g, live, k, lane);
    }
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long q = q0 + 16 * wid + r;
    if (q < Q && lane < k) {
      const long long o = (q * gridDim.y + blockIdx.y) * k + lane;
      out_idx[o] = li[r] == KN_EMPTY ? -1 : li[r];
      out_val[o] = lv[r];
    }
  }
#endif
}

// One wave per query: fold its gy partial lists [Q, gy, k] into idx / val
// [Q, k] with the insert routine of the tile kernel (empty entries carry
// index -1 and are skipped).
extern "C" __global__ void __launch_bounds__(256)
knn_merge_kernel(const int* __restrict__ part_idx,
                 const float* __restrict__ part_val, long long Q, int gy,
                 int k, int* __restrict__ idx, float* __restrict__ val) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  for (long long q = (long long)blockIdx.x * 4 + wid; q < Q;
       q += (long long)gridDim.x * 4) {
    float lv = -INFINITY;
    int li = KN_EMPTY;
    // the query's gy lists are one contiguous run of gy * k entries: 64 at
    // a time, whatever k is, the next 64 loaded before the current insert
    const long long n = (long long)gy * k;
    const int* pi = part_idx + q * n;
    const float* pv = part_val + q * n;
    int g = lane < n ? pi[lane] : -1;
    float v = lane < n ? pv[lane] : 0.f;
    for (long long e0 = 0; e0 < n; e0 += WAVE) {
      const long long e = e0 + WAVE + lane;
      const int g_next = e < n ? pi[e] : -1;
      const float v_next = e < n ? pv[e] : 0.f;
      knn_insert(lv, li, v, g, g >= 0, k, lane);
      g = g_next;
      v = v_next;
    }
    if (lane < k) {
      idx[q * k + lane] = li == KN_EMPTY ? -1 : li;
      val[q * k + lane] = lv;
    }
  }
}

// ============================ L-group silhouettes: fused MFMA distance sums
// D[q, c] = sum over the rows g of X f32[G, h] with labels[g] == c and
// g != q_index[q] of d(q, g) = sqrtf(max(nq[q] + nx[g] - 2 dot(Xq[q], X[g]),
// 0)), d in f32, the sums in f64. The dot is knn_tile_kernel's k-ordered
// MFMA chain; nq / nx are the rows' squared norms (row_sqnorms_kernel).
// Nothing of size Q x G is written, and there are no atomics: every sum is
// added in one fixed order, so a result is bitwise equal run to run for a
// given launch split.

// out[g] = sum_j X[g, j]^2: row_norms_kernel's f64 accumulation and single
// rounding to f32, unrooted and for any h % 4 == 0 (16-byte pieces, a lane
// takes every 64th).
extern "C" __global__ void __launch_bounds__(256)
row_sqnorms_kernel(const float* __restrict__ X, long long G, int h,
                   float* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wib = threadIdx.x >> 6;
  const int wpb = blockDim.x >> 6;
  for (long long g = (long long)blockIdx.x * wpb + wib; g < G;
       g += (long long)gridDim.x * wpb) {
    const float* row = X + g * (long long)h;
    double p = 0.0;
    for (int j = lane * 4; j < h; j += WAVE * 4) {
      const f32x4 x = *(const f32x4*)(row + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) p += (double)x[i] * (double)x[i];
    }
    p = wave_sum(p);
    if (lane == 0) out[g] = (float)p;
  }
}

// The stage, the register prefetch and the K loop are knn_tile_kernel's,
// repeated here rather than shared (knn_tile_kernel's text and register
// budget stay as they are; docs/KERNELS.md). The epilogue differs: once the
// 64 x 64 dots lie in LDS, wave w reduces query rows 16w .. 16w+15 with lane
// (fr, kk) = (lane & 15, lane >> 4) owning row 16w + fr and the candidates
// 4i + kk, i = 0 .. 15, of the tile: KC f64 accumulators per lane, a
// select-add of d or +0.0 per cluster. Masked entries (candidates past G,
// which carry label -1, and a query's own index) select +0.0; padded query
// rows are accumulated and never written. After the walk the four kk groups
// of a row are added by a fixed xor tree.
// out is [Q, gridDim.y, k] f64: D itself when gridDim.y == 1, else the
// partials cds_fold_kernel adds.
template <int KC>
__global__ void __launch_bounds__(256)
cds_tile_kernel(const float* __restrict__ Xq, const float* __restrict__ X,
                const int* __restrict__ labels, const float* __restrict__ nq,
                const float* __restrict__ nx, const int* __restrict__ q_index,
                long long Q, long long G, int h, int k,
                double* __restrict__ out) {
#if defined(__gfx950__)
  __shared__ __attribute__((aligned(16))) float lds[2 * KN_TILE * KN_LD];
  __shared__ int lab_s[KN_TILE];
  __shared__ float nx_s[KN_TILE];
  float* As = lds;
  float* Bs = lds + KN_TILE * KN_LD;
  float* Sc = lds;                             // [64][KN_LDS] <= both tiles

  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, kk = lane >> 4;
  const long long q0 = (long long)blockIdx.x * KN_TILE;

  // this lane's query row: its squared norm and excluded candidate
  const long long qrow = q0 + 16 * wid + fr;
  const float nq_r = qrow < Q ? nq[qrow] : 0.f;
  const long long self = (q_index && qrow < Q) ? q_index[qrow] : -1;

  double acc_d[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) acc_d[c] = 0.0;

  f32x4 ar[KN_NLD], br[KN_NLD];
  const int srow = threadIdx.x >> 4, sc4 = (threadIdx.x & 15) * 4;
  auto prefetch = [&](long long pc0, int pk0) {
#pragma unroll
    for (int i = 0; i < KN_NLD; ++i) {
      const int row = 16 * i + srow;
      const bool kin = pk0 + sc4 < h;
      ar[i] = (kin && q0 + row < Q)
          ? *(const f32x4*)(Xq + (q0 + row) * h + pk0 + sc4) : (f32x4)(0.f);
      br[i] = (kin && pc0 + row < G)
          ? *(const f32x4*)(X + (pc0 + row) * h + pk0 + sc4) : (f32x4)(0.f);
    }
  };

  const long long nct = (G + KN_TILE - 1) / KN_TILE;
  if ((long long)blockIdx.y < nct) prefetch((long long)blockIdx.y * KN_TILE, 0);
  for (long long ct = blockIdx.y; ct < nct; ct += gridDim.y) {
    const long long c0 = ct * KN_TILE;
    // the tile's labels and norms, one candidate per thread of wave 0; they
    // land in LDS with the scores
    int lab_c = -1;
    float nx_c = 0.f;
    if (threadIdx.x < KN_TILE && c0 + threadIdx.x < G) {
      lab_c = labels[c0 + threadIdx.x];
      nx_c = nx[c0 + threadIdx.x];
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4)(0.f);

    for (int k0 = 0; k0 < h; k0 += KN_KC) {
      const int kc = (h - k0 < KN_KC) ? h - k0 : KN_KC;    // multiple of 4
      __syncthreads();          // readers of the last chunk / score tile done
#pragma unroll
      for (int i = 0; i < KN_NLD; ++i) {
        float* pa = As + (16 * i + srow) * KN_LD + sc4;    // 8-byte aligned
        float* pb = Bs + (16 * i + srow) * KN_LD + sc4;
        pa[0] = ar[i][0]; pa[1] = ar[i][1]; pa[2] = ar[i][2]; pa[3] = ar[i][3];
        pb[0] = br[i][0]; pb[1] = br[i][1]; pb[2] = br[i][2]; pb[3] = br[i][3];
      }
      __syncthreads();
      if (k0 + KN_KC < h)
        prefetch(c0, k0 + KN_KC);
      else if (ct + gridDim.y < nct)
        prefetch((ct + gridDim.y) * KN_TILE, 0);
      for (int kq = 0; kq < kc; kq += 4) {
        float av[2], bv[2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
          av[a] = As[(wr * 32 + a * 16 + fr) * KN_LD + kq + kk];
#pragma unroll
        for (int b = 0; b < 2; ++b)
          bv[b] = Bs[(wc * 32 + b * 16 + fr) * KN_LD + kq + kk];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }

    // C/D map (16x16): col = lane&15 (candidate), row = (lane>>4)*4 + reg
    __syncthreads();                     // operand tiles dead in every wave
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          Sc[(wr * 32 + a * 16 + kk * 4 + reg) * KN_LDS + wc * 32 + b * 16 +
             fr] = acc[a][b][reg];
    if (threadIdx.x < KN_TILE) {
      lab_s[threadIdx.x] = lab_c;
      nx_s[threadIdx.x] = nx_c;
    }
    __syncthreads();

    const float* srow_p = Sc + (16 * wid + fr) * KN_LDS;
#pragma unroll 4
    for (int i = 0; i < KN_TILE / 4; ++i) {
      const int j = 4 * i + kk;
      const int lab = (c0 + j == self) ? -1 : lab_s[j];
      const float d2 = nq_r + nx_s[j] - 2.f * srow_p[j];
      const double d = (double)sqrtf(fmaxf(d2, 0.f));
#pragma unroll
      for (int c = 0; c < KC; ++c) acc_d[c] += (lab == c) ? d : 0.0;
    }
  }

#pragma unroll
  for (int c = 0; c < KC; ++c) {
    double v = acc_d[c];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (kk == 0 && qrow < Q && c < k)
      out[(qrow * gridDim.y + blockIdx.y) * k + c] = v;
  }
#endif
}

// D[q, c] = the gy partials part[q, 0 .. gy-1, c] added in ascending y; one
// thread per element of D.
extern "C" __global__ void __launch_bounds__(256)
cds_fold_kernel(const double* __restrict__ part, long long n, int gy, int k,
                double* __restrict__ D) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (long long)gridDim.x * blockDim.x) {
    const long long q = e / k;
    const int c = (int)(e - q * k);
    const double* p = part + q * gy * (long long)k + c;
    double s = 0.0;
    for (int y = 0; y < gy; ++y) s += p[(long long)y * k];
    D[e] = s;
  }
}
