// Ragged fused encoder forward (hidden 50, seq_len 50, 8 waves, two workgroups per CU): the arithmetic of
// srfrd_encoder_fwd_kernel.inc done only for the rows a LEFT-PADDED sequence really has.
//
// A padded position (id 0) is an exact-zero row at every block input and its block output is masked to zero again
// (reference SRFR_model.py:98-99, :121): as a QUERY row it contributes nothing.  As a KEY row it does count - the reference
// passes no key-padding mask (SRFR_model.py:112) - but every LEADING pad is the same key: k = b_k, v = b_v (x = 0), visible
// to every real query.  So the t0 leading pads of a sequence are merged into ONE representative key row (the last of them,
// position t0 - 1) that enters the softmax with multiplicity t0:
//     Z_i = t0 e^{s_i,rep - m} + sum_{valid j <= i} e^{s_ij - m},   o_i = c_i / (1 - p) P_i,rep b_v + sum_j drop(P_ij) v_j
// with c_i = the number of kept ones among the t0 attention-dropout coordinates (i, 0 .. t0 - 1) - the masks stay the
// coordinate hash of srfrd_rng.h, element for element what the full kernel draws.  Same sums in another order: fp32
// rounding-level differences against the full kernel (1e-7), the 1e-4 parity bar against the oracle unchanged.
//
// LDS rows are addressed in TILE coordinates: position t lives in row t + kRagSH (= 12), so that the END of the sequence
// (row 61) sits in the last 16-row MFMA tile and a sequence of n valid positions occupies ceil((n + 1 + 2) / 16) row tiles
// from the bottom - all GEMMs, LayerNorms, the softmax and the FFN run on row tiles mt0 .. 3 only, mt0 = (t0 - 1 + 12) / 16.
// Rows of a computed tile in front of the first valid position ("dead" rows: leading pads, or rows 0..11 that no position
// maps to) go through the arithmetic as zero inputs with keep = 0; as keys they are masked out of the softmax.
//
// Training checkpoints are written for the rows of the computed tiles only (the ragged backward,
// srfrd_encoder_bwd_ragged_kernel.inc, reads exactly those); the probability checkpoint of a row carries c_i P_i,rep in
// the representative's column and t0 P_i,rep in column LP - 1 (spare: L < LP).  The launchers pair this kernel with the
// ragged backward ONLY (encoder_plan pairs them): every other backward reads full-row checkpoints.
//
// Sequence -> workgroup assignment: static (b = blockIdx.x, += gridDim.x) or, when the launch carries the batch's lengths
// (EncArgs::sched, srfrd_seq_order), by LENGTH ORDER: workgroup x takes the sequence of rank perm(x) (rag_take) so that the
// two workgroups sharing a CU's SIMDs hold a long and a short sequence - a launch is as slow as its slowest CU.  Outputs
// are indexed by sequence: results do not depend on the assignment.
namespace SRFRD_NS {

constexpr int kRagSH = 12;          // LDS row of position 0 (LP - R of the backward's 52-row slots: both kernels agree)

// This thread's share of the batch's first-item positions (srfrd_seq_order's output): 512-sequence chunks held in registers
// (B <= 1024; larger batches: identity order, see rag_take).  A kernel requests them as its FIRST instructions, so that the
// round trip runs beside the LayerNorm-parameter fill instead of behind it.
constexpr int kRagChunks = 2;
struct RagT0 {
  int v[kRagChunks];
};
__device__ __forceinline__ bool rag_ordered(const EncArgs& a) { return a.sched != nullptr && a.sched_mode != 0 && a.B <= 512 * kRagChunks; }
__device__ __forceinline__ RagT0 rag_load_t0(const EncArgs& a, int tid) {
  RagT0 t;
#pragma unroll
  for (int c = 0; c < kRagChunks; ++c) {
    const int b = c * 512 + tid;
    t.v[c] = (rag_ordered(a) && c * 512 < a.B) ? a.sched[kSchedT0 + min(b, a.B - 1)] : 0;
  }
  return t;
}

// The sequence of rank `want` in the order (t0 ascending, index ascending), selected from the B first-item positions
// (tv: rag_load_t0) by all 512 threads of the workgroup; scr: >= 96 LDS words, free for the duration.  t0 <= 63.
__device__ __forceinline__ int rag_select(const RagT0& t0v, int B, int want, lds_i* scr, int tid) {
  lds_i* hist = scr;            // [64]
  lds_i* wcnt = scr + 64;       // [8] flagged lanes per wave of the current chunk
  lds_i* res = scr + 80;        // [0] bucket, [1] rank inside the bucket, [2] result
  const int lane = tid & 63, wave = tid >> 6;
  constexpr int NCH = kRagChunks;
  int tv[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) tv[c] = t0v.v[c];
  if (tid < 64) hist[tid] = 0;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int b = c * 512 + tid;
    if (b < B) __hip_atomic_fetch_add(&hist[min(max(tv[c], 0), 63)], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  if (wave == 0) {
    // inclusive prefix over the 64 buckets (one per lane), then the first bucket whose prefix exceeds `want`
    int incl = hist[lane];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const unsigned long long m = __ballot(want < incl);
    const int k = m ? (int)__builtin_ctzll(m) : 63;
    const int excl = __shfl(incl, k, 64) - __shfl(hist[lane], k, 64);
    if (lane == 0) { res[0] = k; res[1] = want - excl; res[2] = 0; }
  }
  __syncthreads();
  const int k = res[0], r = res[1];
  int seen = 0;                 // sequences of bucket k in the chunks before this one
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c * 512 >= B) break;                      // (uniform)
    const int b = c * 512 + tid;
    const bool f = b < B && min(max(tv[c], 0), 63) == k;
    const unsigned long long m = __ballot(f);
    if (lane == 0) wcnt[wave] = (int)__builtin_popcountll(m);
    __syncthreads();
    int before = seen, total = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const int cw = wcnt[w];
      if (w < wave) before += cw;
      total += cw;
    }
    const int mine = before + (int)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (f && mine == r) res[2] = b;
    seen += total;
    __syncthreads();
  }
  return res[2];
}

// One workgroup's next sequence (wave-uniform; -1: none left).  Length order: the first G workgroups (one per CU, in dispatch
// order) take the G longest sequences, the next G the shortest ascending - the workgroup that joins the longest sequence's CU
// brings the shortest one - everything else in descending order.
__device__ __forceinline__ int rag_want(int x, int G, int B) { return x < G ? x : (x < 2 * G ? B - 1 - (x - G) : x - G); }
__device__ __forceinline__ int rag_take(const EncArgs& a, lds_i* scr, int iter, int tid, const RagT0& t0v) {
  const int x = (int)blockIdx.x + iter * (int)gridDim.x;
  if (x >= a.B) return -1;
  if (!rag_ordered(a)) return x;
  return rag_select(t0v, a.B, rag_want(x, a.sched[kSchedG], a.B), scr, tid);
}

// The batch's first-item positions WITHOUT srfrd_seq_order's launch (srfrd_encoder_train_ranked): every workgroup reads the
// whole id plane itself - B * 50 ids, flat, 16 bytes (two ids) per lane: thread t takes the pairs t, t + 512, ... (coalesced: a
// wave reads 128 consecutive ids; 8-byte loads run at 0.6 of this rate) - and all it keeps of an id is whether it is zero.  A
// round costs a wave two compares and four lane writes: the ballots of its 25 rounds collect in four registers (lane j: round
// j) and go to LDS in one store each, where they form two bitmaps in pair order - bit q of the first: id 2 q is not zero, of
// the second: id 2 q + 1.  A sequence's 50 ids are the pairs 25 b .. 25 b + 24; thread b takes those 25 bits from either bitmap
// and counts the zeros in front.  All loads of the first 512 sequences are requested before anything waits; zero_fill() - the
// caller's LDS fill, which must cover bm - runs in their shadow.  bm: kRagRankWords LDS words, left zeroed again.  Ends WITHOUT
// a barrier: the caller's next one orders the last stores.  Same values as srfrd_seq_order writes (50 for a sequence of pads; a
// zero behind the first item is no pad), so rag_select picks the same sequences.  B <= 512 * kRagChunks; ids 16-byte aligned.
constexpr int kRagRankHalf = kRagChunks * 512 * 25 / 32 + 2;      // words of one bitmap (+ 2: a window is read as two words)
constexpr int kRagRankWords = 2 * kRagRankHalf;
// v_writelane_b32 (value, lane, old): clang has the read builtin only; the intrinsic by its own name
extern "C" __device__ int srfrd_writelane(int, int, int) __asm("llvm.amdgcn.writelane.i32");
typedef long long RagIdPair __attribute__((ext_vector_type(2)));
template <class ZF>
__device__ __forceinline__ RagT0 rag_rank_batch(const int64_t* __restrict__ ids, int B, lds_i* bm, int tid, const ZF& zero_fill) {
  constexpr int L = 50, NJ = L / 2;              // 512 sequences are NJ rounds of 512 id pairs
  static_assert(NJ <= 64 && kRagRankWords <= 4 * 512, "one lane per round; four words per thread to clear");
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n2 = B * NJ;                         // id pairs of the plane
  const RagIdPair* __restrict__ pairs = reinterpret_cast<const RagIdPair*>(ids);
  RagIdPair v[NJ];
  auto request = [&](int c) {
    if ((c + 1) * NJ * 512 <= n2) {              // (uniform) 512 whole sequences: nothing to clamp
      const unsigned off = (unsigned)tid << 4;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        v[j] = *reinterpret_cast<const RagIdPair*>(reinterpret_cast<const char*>(pairs + (c * NJ + j) * 512) + off);
    } else {
      // (a round's first pair and the pairs left from there are scalars, the lane's share a 32-bit byte offset.  Clamped: every
      // address is one of the plane's; what a lane behind the batch reads lands in bits behind the last sequence's, which
      // nobody looks at)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int first = min((c * NJ + j) * 512, n2 - 1);
        const unsigned off = (unsigned)min(tid, n2 - 1 - first) << 4;
        v[j] = *reinterpret_cast<const RagIdPair*>(reinterpret_cast<const char*>(pairs + first) + off);
      }
      asm volatile("");                          // (keeps the two forms apart: merged, every load waits for a selected 64-bit address)
    }
  };
  auto collect = [&](int c) {
    int e_lo = 0, e_hi = 0, o_lo = 0, o_hi = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const unsigned long long me = __ballot(v[j].x != 0), mo = __ballot(v[j].y != 0);
      e_lo = srfrd_writelane((int)(unsigned)me, j, e_lo);
      e_hi = srfrd_writelane((int)(unsigned)(me >> 32), j, e_hi);
      o_lo = srfrd_writelane((int)(unsigned)mo, j, o_lo);
      o_hi = srfrd_writelane((int)(unsigned)(mo >> 32), j, o_hi);
    }
    if (lane < NJ) {                             // pairs ((c NJ + lane) 8 + wave) 64 ..: that 64-bit word of either bitmap
      const int w = (((c * NJ + lane) << 3) + wave) << 1;
      bm[w] = e_lo;
      bm[w + 1] = e_hi;
      bm[kRagRankHalf + w] = o_lo;
      bm[kRagRankHalf + w + 1] = o_hi;
    }
  };
  request(0);
  __builtin_amdgcn_sched_barrier(0);
  zero_fill();
  __syncthreads();
  collect(0);
#pragma unroll 1
  for (int c = 1; c < kRagChunks; ++c)
    if (c * 512 < B) {                           // (uniform)
      request(c);
      collect(c);
    }
  __syncthreads();
  RagT0 t;
#pragma unroll
  for (int c = 0; c < kRagChunks; ++c) {
    const int b = c * 512 + tid;
    int t0 = L;
    if (b < B) {                                 // bits 25 b .. 25 b + 24 of either bitmap
      const int w = (b * NJ) >> 5, sh = (b * NJ) & 31;
      const unsigned long long we = ((unsigned long long)(unsigned)bm[w + 1] << 32) | (unsigned)bm[w];
      const unsigned long long wo = ((unsigned long long)(unsigned)bm[kRagRankHalf + w + 1] << 32) | (unsigned)bm[kRagRankHalf + w];
      const unsigned xe = (unsigned)(we >> sh) & ((1u << NJ) - 1u), xo = (unsigned)(wo >> sh) & ((1u << NJ) - 1u);
      const int pe = xe ? 2 * __builtin_ctz(xe) : L, po = xo ? 2 * __builtin_ctz(xo) + 1 : L;
      t0 = min(pe, po);
    }
    t.v[c] = t0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i * 512 + tid < kRagRankWords) bm[i * 512 + tid] = 0;
  return t;
}

// softplus on the hardware exp / log (1e-7 absolute: the loss is compared at 1e-4; log1pf / expf expand to ~200 instructions
// that every lane of the head pass executes)
__device__ __forceinline__ float softplus_fast(float z) { return fmaxf(z, 0.f) + __logf(1.0f + __expf(-fabsf(z))); }

// What the fused masked BCE's logit gradients (bce_dlogits: srfrd_enc_bwd_head.h) send back into the head: one definition for
// the backward's head and the train kernel's forward head (SEAM_), so that both contract the same way.
// d hidden[t][c] of a column with target rows: the upstream gradient (0 under the fused BCE) plus dp * (positive row) +
// dn * (negative row)
__device__ __forceinline__ float head_dh(float up, float dp, float pv, float dn, float nv) {
  up += dp * pv + dn * nv;
  return up;
}
// head_dh(0, ...) as the backward's instantiation of kind K_ computes it.  Under -ffp-contract=fast hipcc contracts the
// expression above by its surroundings: in SRFRN's backward to fma(dn, nv, fma(dp, pv, up)), in the other kinds' to two rounded
// products and their sum.  The train kernel's forward head stands elsewhere, so it pins the form (the empty asm keeps a rounded
// product from being fused again); tests/test_gpu_fused_train.py and tests/test_gpu_train_seam.py hold the one-launch step to
// the two-launch step bit for bit, for every kind.
template <int K_>
__device__ __forceinline__ float head_dh_as_backward(float dp, float pv, float dn, float nv) {
  float a = dp * pv;
  asm volatile("" : "+v"(a));
  if constexpr (K_ == SRFRD_SRFRN) return __builtin_fmaf(dn, nv, a);
  float b = dn * nv;
  asm volatile("" : "+v"(b));
  return a + b;
}
// h * (target row element) as the stand-alone forward rounds it into LDS before the logit sums read it: the train kernel keeps
// the row there instead and multiplies in the sum (the empty asm keeps the product out of an fma with the running sum)
__device__ __forceinline__ float seam_product(float h, float v) {
  float p = h * v;
  asm volatile("" : "+v"(p));
  return p;
}
// ... and the two rows' item-table contributions: dp * h, dn * h
__device__ __forceinline__ float head_contrib(float dl, float h) { return dl * h; }
// Head range of the backward: the first position of the 16-row tiles that hold position min(th, krp), th the first position
// with an upstream gradient, krp the representative key.  tile0: the first tile, pos0: its first position.
struct RagHead {
  int tile0, pos0;
};
__device__ __forceinline__ RagHead rag_head_range(int th, int krp) {
  const int hp = th < krp ? th : krp;
  RagHead r;
  r.tile0 = (hp + kRagSH) >> 4;
  const int rh0 = r.tile0 << 4;
  r.pos0 = rh0 > kRagSH ? rh0 - kRagSH : 0;
  return r;
}

// Packed-weight GEMM group for the ragged kernels: gemm_group_packed (srfrd_dev.h) with
//   * an optional SECOND product accumulated into the same tiles (C = A1 W1 + A2 W2: the backward's dx = dk Wk + dv Wv without
//     a store and a read-modify-write in between),
//   * epi runs for columns < ncols only, under one lane-level branch;
//   * pre(r, c): one LDS value per output element requested BEFORE the MFMA chain (the residual a forward epilogue adds, the
//     ReLU mask, the destination of a += epilogue) and handed to epi(r, c, acc, pre): the epilogue itself then holds only
//     stores - with a read inside it hipcc keeps read -> wait -> store order for each of the tile's eight elements.
// Rows: (mt + j * mstride_tiles) * 16 + 4 lq + e, column 16 nt + li; k = 4 * ksteps <= 64.
struct NoPost {
  __device__ __forceinline__ void operator()(int, int, const float (&)[4]) const {}
};
template <int G, bool TWO, class AL, class AL2, class PRE, class EPI, class POST = NoPost>
__device__ __forceinline__ void rgemm_packed(int mt, int mstride_tiles, int nt, int ksteps, int ncols, const AL& a, const WFrag& w,
                                             const AL2& a2, const WFrag& w2, const PRE& pre, const EPI& epi, int lane,
                                             const POST& post = POST{}) {
  const int li = lane & 15, lq = lane >> 4;
  const int c = (nt << 4) + li;
  float pv[G][4];
#pragma unroll
  for (int j = 0; j < G; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) pv[j][e] = pre(((mt + j * mstride_tiles) << 4) + (lq << 2) + e, c);
  f32x4 acc[G];
#pragma unroll
  for (int j = 0; j < G; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int mrow = (mt << 4) + li, mstride = mstride_tiles << 4;
#pragma unroll
  for (int pass = 0; pass < (TWO ? 2 : 1); ++pass) {
    float av[4][G];
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < ksteps)
#pragma unroll
        for (int j = 0; j < G; ++j) av[s][j] = pass == 0 ? a(mrow + j * mstride, 4 * s + lq) : a2(mrow + j * mstride, 4 * s + lq);
#pragma unroll
    for (int kc = 0; kc < kPackKC; ++kc) {
      const int nst = ksteps - 4 * kc;
      if (nst > 0) {
        const int nnext = nst - 4;
        float an[4][G];
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < nnext)
#pragma unroll
            for (int j = 0; j < G; ++j)
              an[s][j] = pass == 0 ? a(mrow + j * mstride, ((kc + 1) << 4) + 4 * s + lq) : a2(mrow + j * mstride, ((kc + 1) << 4) + 4 * s + lq);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (s < nst)
#pragma unroll
            for (int j = 0; j < G; ++j)
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][j], pass == 0 ? w.q[kc][s] : w2.q[kc][s], acc[j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int j = 0; j < G; ++j) av[s][j] = an[s][j];
      }
    }
  }
  const float bias = TWO ? w.bias + w2.bias : w.bias;
  if (c < ncols) {            // ONE exec-mask region for the lane's eight elements (the column is the lane's, not the element's)
#pragma unroll
    for (int j = 0; j < G; ++j) {
      // epi may return the element's stored value; post(first row, c, values[4]) then sees the lane's four consecutive rows of
      // the tile together (the forward's checkpoint stores: one offset, three immediates)
      const int rb = ((mt + j * mstride_tiles) << 4) + (lq << 2);
      float gv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if constexpr (std::is_void_v<decltype(epi(rb, c, 0.f, 0.f))>) { epi(rb + e, c, acc[j][e] + bias, pv[j][e]); gv[e] = 0.f; }
        else gv[e] = epi(rb + e, c, acc[j][e] + bias, pv[j][e]);
      }
      post(rb, c, gv);
    }
  }
}
struct NoPre {
  __device__ __forceinline__ float operator()(int, int) const { return 0.f; }
};

// row tiles [m0, m0 + mtn) of the operand, mtn <= 4: wave (strip nt = wave & 3, g = wave >> 2) owns tiles m0 + g, m0 + g + 2
template <class AL, class PRE, class EPI, class POST = NoPost>
__device__ __forceinline__ void rag_packed(int m0, int mtn, int ksteps, int ncols, const AL& a, const WFrag& w, const PRE& pre,
                                           const EPI& epi, int lane, int wave, const POST& post = POST{}) {
  const int nt = wave & 3, g = wave >> 2;
  if (g + 2 < mtn) rgemm_packed<2, false>(m0 + g, 2, nt, ksteps, ncols, a, w, a, w, pre, epi, lane, post);
  else if (g < mtn) rgemm_packed<1, false>(m0 + g, 2, nt, ksteps, ncols, a, w, a, w, pre, epi, lane, post);
}
template <class AL, class AL2, class PRE, class EPI>
__device__ __forceinline__ void rag_packed2(int m0, int mtn, int ksteps, int ncols, const AL& a, const WFrag& w, const AL2& a2,
                                            const WFrag& w2, const PRE& pre, const EPI& epi, int lane, int wave) {
  const int nt = wave & 3, g = wave >> 2;
  if (g + 2 < mtn) rgemm_packed<2, true>(m0 + g, 2, nt, ksteps, ncols, a, w, a2, w2, pre, epi, lane);
  else if (g < mtn) rgemm_packed<1, true>(m0 + g, 2, nt, ksteps, ncols, a, w, a2, w2, pre, epi, lane);
}

// Two products that share the A operand (k = x Wk^T + bk and v = x Wv^T + bv): the A fragments are read from LDS once and
// feed both weights' accumulator chains (2 G independent chains per wave).  epi(r, c, value_1, value_2).
template <int G, class AL, class EPI, class POST>
__device__ __forceinline__ void rgemm_packed_dual(int mt, int mstride_tiles, int nt, int ksteps, int ncols, const AL& a, const WFrag& w1,
                                                  const WFrag& w2, const EPI& epi, int lane, const POST& post) {
  const int li = lane & 15, lq = lane >> 4;
  const int c = (nt << 4) + li;
  f32x4 acc1[G], acc2[G];
#pragma unroll
  for (int j = 0; j < G; ++j) { acc1[j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc2[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int mrow = (mt << 4) + li, mstride = mstride_tiles << 4;
  float av[4][G];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < ksteps)
#pragma unroll
      for (int j = 0; j < G; ++j) av[s][j] = a(mrow + j * mstride, 4 * s + lq);
#pragma unroll
  for (int kc = 0; kc < kPackKC; ++kc) {
    const int nst = ksteps - 4 * kc;
    if (nst > 0) {
      const int nnext = nst - 4;
      float an[4][G];
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < nnext)
#pragma unroll
          for (int j = 0; j < G; ++j) an[s][j] = a(mrow + j * mstride, ((kc + 1) << 4) + 4 * s + lq);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if (s < nst)
#pragma unroll
          for (int j = 0; j < G; ++j) {
            acc1[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][j], w1.q[kc][s], acc1[j], 0, 0, 0);
            acc2[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][j], w2.q[kc][s], acc2[j], 0, 0, 0);
          }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < G; ++j) av[s][j] = an[s][j];
    }
  }
  if (c < ncols) {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const int rb = ((mt + j * mstride_tiles) << 4) + (lq << 2);
      float g1[4], g2[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        g1[e] = acc1[j][e] + w1.bias;
        g2[e] = acc2[j][e] + w2.bias;
        epi(rb + e, c, g1[e], g2[e]);
      }
      post(rb, c, g1, g2);
    }
  }
}
template <class AL, class EPI, class POST>
__device__ __forceinline__ void rag_packed_dual(int m0, int mtn, int ksteps, int ncols, const AL& a, const WFrag& w1, const WFrag& w2,
                                                const EPI& epi, int lane, int wave, const POST& post) {
  const int nt = wave & 3, g = wave >> 2;
  if (g + 2 < mtn) rgemm_packed_dual<2>(m0 + g, 2, nt, ksteps, ncols, a, w1, w2, epi, lane, post);
  else if (g < mtn) rgemm_packed_dual<1>(m0 + g, 2, nt, ksteps, ncols, a, w1, w2, epi, lane, post);
}

// causal softmax over key rows [kr, r] of query rows [rq0, LP); see the header.  S in tile coordinates [LP][SLD].
// Eight lanes per row; lane m owns the eight CONSECUTIVE key positions 8 m .. 8 m + 7 (tile columns 12 + 8 m ..): a lane reads and
// writes its part of the row as four 8-byte LDS accesses and its part of the probability checkpoint as two 16-byte stores
// (a wave covers eight consecutive checkpoint rows: 2 KB contiguous) - instead of eight 4-byte accesses each at stride 8.
// Lane 7 (positions 56 .. 63: beyond the sequence) only joins the reductions.  Tile columns 0 .. 11 are never written: the P v
// product starts at column 12.
typedef __attribute__((address_space(3))) f32x2 lds_f2r;
__device__ __forceinline__ void rag_softmax(lds_f* S, int rq0, int r0, int v0, int kr, int t0, int row_end, const DropSite& ds,
                                            float* gsave, int tid) {
  constexpr int LP = 64, SLD = 66, SH = kRagSH;
  const int m8 = (tid & 7) << 3;                  // first key position of this lane
  const int r = rq0 + (tid >> 3);                 // 512 threads: 64 rows in one pass
  if (r >= LP) return;
  lds_f2r* row2 = reinterpret_cast<lds_f2r*>(S + r * SLD + SH + m8);
  const bool own = m8 < 56;                       // lanes 0 .. 6 hold columns of the matrix
  const int npair = m8 == 48 ? 2 : 4;             // (lane 6: tile columns 60 .. 63 exist, 64 .. 67 do not)
  const int ip = r - SH;                          // position of the query
  float4* g4 = (gsave != nullptr && own && ip >= 0 && r < row_end) ? reinterpret_cast<float4*>(gsave + ip * LP + m8) : nullptr;
  if (r < v0 || r >= row_end) {                   // dead query row: zeros (its P v must stay finite)
    if (own) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < npair) row2[i] = f32x2{0.f, 0.f};
    }
    if (g4 != nullptr) { g4[0] = make_float4(0.f, 0.f, 0.f, 0.f); g4[1] = make_float4(0.f, 0.f, 0.f, 0.f); }
    return;
  }
  const bool rep = t0 >= 1;
  const int krp = kr - SH;                        // first key position
  float x[8];
  if (own) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { const f32x2 t = row2[i < npair ? i : 0]; x[2 * i] = t.x; x[2 * i + 1] = t.y; }
  }
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int pj = m8 + i;
    x[i] = (own && pj >= krp && pj <= ip) ? x[i] : -INFINITY;
    mx = fmaxf(mx, x[i]);
  }
  mx = row_max(mx);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int pj = m8 + i;
    const float e = (own && pj >= krp && pj <= ip) ? __expf(x[i] - mx) : 0.f;
    x[i] = e;
    s += (rep && pj == krp) ? e * (float)t0 : e;
  }
  s = row_sum(s);
  const float inv = 1.0f / s;
  // kept ones among the attention-dropout coordinates (ip, 0 .. t0 - 1) of the merged pads
  float cnt = (float)t0;
  if (ds.on && rep) {
    int c = 0;
    for (int jj = tid & 7; jj < t0; jj += 8) c += drop_mul(ds, ip, jj) != 0.f ? 1 : 0;
    cnt = row_sum((float)c);
  }
  if (!own) return;
  const float scale = ds.on ? ds.scale : 1.0f;
  float pv[8], gs[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int pj = m8 + i;
    const float p = x[i] * inv;                   // exact zero outside [krp, ip]
    if (rep && pj == krp) {
      const float pm = p * cnt;
      if (gsave != nullptr) gsave[ip * LP + LP - 1] = p * (float)t0;
      pv[i] = pm * scale;
      gs[i] = pm;
    } else {
      const float mul = drop_mul(ds, ip, pj);
      pv[i] = p * mul;
      gs[i] = mul != 0.f ? p : -p;                // (p = 0 outside the live range: +-0)
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < npair) row2[i] = f32x2{pv[2 * i], pv[2 * i + 1]};
  if (g4 != nullptr) {
    g4[0] = make_float4(gs[0], gs[1], gs[2], gs[3]);
    g4[1] = make_float4(gs[4], gs[5], gs[6], gs[7]);
  }
}

// What the train kernel's forward hands its backward in registers (SEAM_), beside the LDS rows it leaves in place: the head's
// first position, the leading pads, and - in lane t < 64 of the first wave - the ids and SRFRN's logit gradients of position t.
struct RagSeam {
  int th, t0;
  int id, pid, nid, fk, pfk, nfk;
  float dp, dn;
};
// ... and in LDS: the last block's output stays in the backward's slot 0 (the forward's position-indexed x is that address
// range), d hidden is written to the backward's slot kRagSeamG, which rag_bwd_seq<.., SEAM_> takes for sG.
constexpr int kRagSlot = 52 * 54;   // floats of one backward slot
constexpr int kRagSeamG = 3;

// LDS working set of the ragged forward for one sequence.  The forward kernel lays it out behind its per-row arrays, the
// train kernel (srfrd_encoder_train_ragged.hip) over the same floats as the backward's slots: see rag_fwd_seq's callers.
struct RagFwdLds {
  lds_f *bXS, *bQN, *bQ, *bK, *bV;  // [LP][SLD] (x, and the scores over it), then four [LP][DS]; kSlack readable behind bV
  lds_i* s_in;                      // all four in tile coordinates (row = position + SH)
  lds_f* s_keep;
  lds_i *s_pid, *s_nid;
  lds_f* s_misc;                    // 64 floats
  lds_f* s_ln;                      // LayerNorm parameters (fill_ln_cache)
};

// The ragged forward of sequence b by the whole workgroup (512 threads), from its ids to its hidden states, logits, BCE
// partial sums and (training) checkpoints; ends with a workgroup barrier.  tid: the laundered thread index (see launder),
// wave: its wave (uniform).
// SEAM_ (the train kernel, fused BCE; m laid over the backward's slots as encoder_train_ragged_kernel does): the head also does
// the first part of the backward's head while the target rows, the hidden rows and the logits are at hand - the logit
// gradients, d hidden -> the backward's LDS slot kRagSeamG (its head range) and, as its last action, the target rows'
// item-table contributions (float atomics, or the rows of a.contrib) - and leaves the last block's output where it is.
// Returns what the backward takes over in registers (RagSeam; zeros without SEAM_).
template <int K_, int T_, int DI_, bool SEAM_ = false>
__device__ __forceinline__ RagSeam rag_fwd_seq(const EncArgs& a, const RagFwdLds& m, int b, int& tid, int wave, uint32_t seed) {
  static_assert(!SEAM_ || T_ != 0, "the head seam belongs to the training forward");
  const Dims& ly = a.dm;
  constexpr int D = 50, L = 50, LP = 64, DK = 52, DS = 54, SLD = 66, NT = 4, MT = 4, SH = kRagSH;
  constexpr int nw = 8, nthr = 512;
  static_assert(SH + L <= LP && (SH & 3) == 0, "tile coordinates");
  const int lane0 = threadIdx.x & 63;
  lds_f* bXS = m.bXS;
  lds_f* bQN = m.bQN;
  lds_f* bQ = m.bQ;
  lds_f* bK = m.bK;
  lds_f* bV = m.bV;
  lds_i* s_in = m.s_in;
  lds_f* s_keep = m.s_keep;
  lds_i* s_pid = m.s_pid;
  lds_i* s_nid = m.s_nid;
  lds_f* s_misc = m.s_misc;
  lds_f* s_ln = m.s_ln;
  const float* P = a.dense;
  const ItemTable table{a.table, a.table16};
  constexpr bool TR_ = T_ != 0;
  const bool has_pos = TR_ || a.pos_ids != nullptr, has_neg = TR_ || a.neg_ids != nullptr;
  const bool drop_on = TR_ || a.drop_on != 0, do_save = TR_ || a.save_x != nullptr, do_loss = TR_ || a.loss_part != nullptr;
  const int kind = K_ >= 0 ? K_ : ly.kind;
  const bool is_sas = kind == SRFRD_SASREC;
  const bool has_fake = kind == SRFRD_SRFR || kind == SRFRD_SRFRN;
  const bool is_srfu = kind >= SRFRD_SRFU_B;
  constexpr int di = DI_, dfk = D - DI_;
  constexpr int dout = (K_ == SRFRD_SRFR) ? DI_ : D;
  const float sqrtD = sqrtf((float)di);
  const float qscale = a.qscale;
  auto pk = [&](int mat, int form) {
    return PackedB{reinterpret_cast<const float4*>(a.packed) + ((int64_t)mat * 2 + form) * (kPackFloats / 4)};
  };

  asm volatile("" : "+v"(tid));
  const int64_t rowbase = (int64_t)b * L;
  const uint32_t seq = (uint32_t)(a.seq0 + b);
  if (tid < LP) {
    const int t = tid - SH;
    const bool in = t >= 0 && t < L;
    const int id = in ? clamp_id(a.in_ids[rowbase + t], ly.n_items) : 0;
    s_in[tid] = id;
    s_keep[tid] = id != 0 ? 1.f : 0.f;
    s_pid[tid] = (in && has_pos) ? clamp_id(a.pos_ids[rowbase + t], ly.n_items) : 0;
    s_nid[tid] = (in && has_neg) ? clamp_id(a.neg_ids[rowbase + t], ly.n_items) : 0;
  }
  if (is_srfu && wave == 1) {
    const int lab = user_label_wave(kind, a.fk_ids ? a.fk_ids + rowbase : nullptr, L, ly.n_labels);
    if (lane0 == 0) ((lds_i*)s_misc)[0] = lab;
  }
  __syncthreads();
  // ---- the sequence's rows: v0 = first non-pad row, kr = first key row (the representative of the t0 leading pads)
  int v0;
  {
    const unsigned long long nz = __ballot(s_in[tid & 63] != 0);
    v0 = nz ? (int)__builtin_ctzll(nz) : SH + L;
    if (a.ragged_off) v0 = SH;
    v0 = __builtin_amdgcn_readfirstlane(v0);
  }
  const int t0 = v0 - SH;
  const int kr = t0 >= 1 ? v0 - 1 : v0;
  const int mt0 = kr >> 4, r0 = mt0 << 4, mtn = MT - mt0;
  const int tstart = r0 > SH ? r0 - SH : 0;               // first position of the computed tiles

  // ---- embedding: gather + position (+ side channel) + pad mask          (SURVEY 3.4 steps 1-4)
  {
    const DropSite dsE = drop_site(drop_on && is_sas, seed, SITE_EMB, seq, a.drop_thr, a.drop_scale);
    const int lab = is_srfu ? ((lds_i*)s_misc)[0] : 0;
    // rows of the computed tiles that no position maps to (0 .. SH - 1 in front, SH + L .. LP - 1 behind): zeros
    if (r0 < SH)
      for (int i = tid; i < (SH - r0) * DS; i += nthr) bXS[r0 * DS + i] = 0.f;
    for (int i = tid; i < (LP - SH - L) * DS; i += nthr) bXS[(SH + L) * DS + i] = 0.f;
    int t = tstart + tid / D, c = tid - (tid / D) * D;
    constexpr int dt = nthr / D, dc = nthr - dt * D;
    for (; t < L;) {
      const int id = s_in[t + SH];
      float v;
      if (has_fake) {
        if (c < di) v = table((int64_t)id * di + c) + P[ly.off_pos + t * di + c];
        else v = P[ly.off_side + ((a.fk_ids ? clamp_id(a.fk_ids[rowbase + t], 2) : 0)) * dfk + (c - di)];
      } else {
        v = table((int64_t)id * di + c);
        if (is_sas) v *= sqrtD;
        v += P[ly.off_pos + t * di + c];
        if (is_srfu) v += P[ly.off_side + lab * D + c];
        if (is_sas) v *= drop_mul(dsE, t, c);
      }
      v *= s_keep[t + SH];
      bXS[(t + SH) * DS + c] = v;
      if (do_save) a.save_x[x_off(0, b, ly.n_blocks, L, D) + t * D + c] = v;
      t += dt; c += dc;
      if (c >= D) { c -= D; ++t; }
    }
  }
  __syncthreads();

  for (int i = 0; i < ly.n_blocks; ++i) {
    const BlkOff o = blk_off(ly.blk0 + i * ly.blk_stride, D);
    launder(bXS); launder(bQN); launder(bQ); launder(bK); launder(bV);
    // (nothing derived from the lane index may be lifted out of the block loop: hipcc otherwise precomputes every per-lane
    // epilogue address of the block once, runs out of registers and spills them)
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    // ranking (last_only): the LAST block computes its query-side rows for the tile of position L - 1 only
    const bool lo = !TR_ && a.last_only != 0 && i == ly.n_blocks - 1;
    const int mq0 = lo ? (L - 1 + SH) >> 4 : mt0, rq0 = mq0 << 4, mqn = MT - mq0;
    const AuxOff ax = aux_off(i, b, ly.n_blocks, L, LP, D, 1);
    float* sv_r = do_save ? a.save_aux + ax.r : nullptr;
    float* sv_o = do_save ? a.save_aux + ax.o : nullptr;
    float* sv_p = do_save ? a.save_aux + ax.p : nullptr;
    float* sv_q = do_save ? a.save_aux + ax.q : nullptr;
    float* sv_k = do_save ? a.save_aux + ax.k : nullptr;
    float* sv_v = do_save ? a.save_aux + ax.v : nullptr;
    // Epilogues (rgemm_packed): one lane-level branch on the column, LDS stores straight-line, checkpoint stores per row group
    // checkpoint rows of one lane's four consecutive tile rows rb .. rb + 3 (positions rb - SH ..): scalar plane base + one
    // 32-bit offset + immediates when all four are positions of the sequence (every row group but rows 0 .. 11 and 60 .. 63)
    auto gstore4 = [&](float* plane, int rb, int c, const float (&v)[4]) {
      const int p0 = rb - SH;
      const unsigned off = (unsigned)(p0 * D + c);
      if (p0 >= 0 && p0 + 3 < L) {
        plane[off] = v[0]; plane[off + D] = v[1]; plane[off + 2 * D] = v[2]; plane[off + 3 * D] = v[3];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((unsigned)(p0 + e) < (unsigned)L) plane[(unsigned)((p0 + e) * D + c)] = v[e];
      }
    };
    const WFrag wq = load_wfrag(pk(i * 6 + 0, 0), P + o.in_b, D, NT, tid);
    const WFrag wk = load_wfrag(pk(i * 6 + 1, 0), P + o.in_b + D, D, NT, tid);
    const WFrag wv = load_wfrag(pk(i * 6 + 2, 0), P + o.in_b + 2 * D, D, NT, tid);
    ln_rows(nw, bXS + rq0 * DS, bQN + rq0 * DS, LP - rq0, DS, D, s_ln + (4 * i + 0) * 64, s_ln + (4 * i + 1) * 64);
    __syncthreads();
    // q = (LN(x) Wq^T + bq) * sqrt(1/d_h);  k = x Wk^T + bk;  v = x Wv^T + bv       (rows of tiles mt0 .. 3)
    rag_packed(mq0, mqn, DK >> 2, D, Mat{bQN, DS}, wq, NoPre{}, [&](int r, int c, float v, float) {
      bQ[r * DS + c] = v * qscale;
      return v * qscale;
    }, lane, wave, [&](int rb, int c, const float (&gv)[4]) { if (sv_q) gstore4(sv_q, rb, c, gv); });
    rag_packed_dual(mt0, mtn, DK >> 2, D, Mat{bXS, DS}, wk, wv, [&](int r, int c, float vk, float vv) {
      bK[r * DS + c] = vk;
      bV[r * DS + c] = vv;
    }, lane, wave, [&](int rb, int c, const float (&gk)[4], const float (&gv)[4]) {
      if (sv_k) { gstore4(sv_k, rb, c, gk); gstore4(sv_v, rb, c, gv); }
    });
    const WFrag wo = load_wfrag(pk(i * 6 + 3, 0), P + o.out_b, D, NT, tid);
    const WFrag w1 = load_wfrag(pk(i * 6 + 4, 0), P + o.c1_b, D, NT, tid);
    __syncthreads();
    // S = q k^T on the lower-triangular tiles of [mq0, 4) x [mt0, 4) (x is dead: S overlays it), dealt round-robin
    {
      const int li = lane & 15, lq = lane >> 4;
      if (lo) {
        for (int u = wave; u < mtn; u += nw)
          gemm_group<0, 1>(0, 1, u << 4, DK, Mat{bQ + rq0 * DS, DS}, MatT{bK + r0 * DS, DS},
                           [&](int r, int c, float v) { bXS[(r + rq0) * SLD + c + r0] = v; }, li, lq);
      } else {
        const int ntri = (mtn * (mtn + 1)) >> 1;
        for (int u = wave; u < ntri; u += nw) {
          const int m = u >= 6 ? 3 : (u >= 3 ? 2 : (u >= 1 ? 1 : 0)), n = u - ((m * (m + 1)) >> 1);
          gemm_group<0, 1>(m, 1, n << 4, DK, Mat{bQ + r0 * DS, DS}, MatT{bK + r0 * DS, DS},
                           [&](int r, int c, float v) { bXS[(r + r0) * SLD + c + r0] = v; }, li, lq);
        }
      }
    }
    __syncthreads();
    {
      const DropSite dsA = drop_site(drop_on, seed, site_attn(i), seq, a.drop_thr, a.drop_scale);
      // Key-padding mask (srfrd_layout::flags): the t0 merged pads are no key - the softmax runs as for a sequence whose first
      // key is its first valid position (no representative, no multiplicity term), which leaves exact zeros in the
      // representative's checkpoint column (c_i P_i,rep); column LP - 1 (t0 P_i,rep, which only a row with a representative
      // writes) gets its zeros here: the ragged backward reads both, and every merged-key term it forms from them vanishes.
      // (SRFRD_RAGGED_FULL_ROWS walks the pads as rows of their own, t0 = 0: they are counted again here, and the pad QUERY
      // rows become dead rows - zero probabilities, finite.)  Without the flag the call is the one it was.
      int v0m = v0, krm = kr, t0m = t0;
      if (ly.flags & SRFRD_LAYOUT_MASK_PAD_KEYS) {
        int vt = v0;
        if (a.ragged_off) {
          const unsigned long long nz = __ballot(s_in[tid & 63] != 0);
          vt = __builtin_amdgcn_readfirstlane(nz ? (int)__builtin_ctzll(nz) : SH + L);
        }
        if (vt > SH) { v0m = vt; krm = vt; t0m = 0; }
        if (sv_p != nullptr && t0 >= 1 && tid >= t0 && tid < L) sv_p[tid * LP + LP - 1] = 0.f;
      }
      rag_softmax(bXS, rq0, r0, v0m, krm, t0m, SH + L, dsA, sv_p, tid);
    }
    __syncthreads();
    // o = P v  (q is dead: o overlays it); tile m of the queries meets key tiles <= m: the pairs {0,3}, {1,2} cost the same
    {
      const int li = lane & 15, lq = lane >> 4;
      const int nt = wave & 3, g = wave >> 2;
      auto epi_o = [&](int r_, int c, float v) {
        const int r = r_ + rq0;
        if (c < D) {          // (not an rgemm_packed epilogue: the column guard is its own)
          bQ[r * DS + c] = v;
          if (sv_o && (unsigned)(r - SH) < (unsigned)L) sv_o[(unsigned)((r - SH) * D + c)] = v;
        }
      };
      if (lo) {
        if (g == 0) {
          const int kk0 = r0 > SH ? r0 : SH;
          gemm_group<0, 1>(0, 1, nt << 4, LP - kk0, Mat{bXS + rq0 * SLD + kk0, SLD}, Mat{bV + kk0 * DS, DS}, epi_o, li, lq);
        }
      } else {
        // (k from tile column max(r0, 12): columns 0 .. 11 of tile 0 are keys no position maps to - the softmax leaves them
        // unwritten; with the shifted base a query tile's k-range ends up to 12 columns past its diagonal tile: exact zeros)
        const int kk0 = r0 > SH ? r0 : SH;
        const Mat Ap{bXS + r0 * SLD + kk0, SLD};
        const Mat Bv{bV + kk0 * DS, DS};
        const int kend = LP - kk0;
        // relative query tiles of this wave: mtn 4: {0,3} | {1,2};  3: {2} | {0,1};  2: {1} | {0};  1: {0} | -
        int ma, mb;
        if (mtn == 4) { ma = g == 0 ? 0 : 1; mb = g == 0 ? 3 : 2; }
        else if (mtn == 3) { ma = g == 0 ? 2 : 0; mb = g == 0 ? -1 : 1; }
        else if (mtn == 2) { ma = g == 0 ? 1 : 0; mb = -1; }
        else { ma = g == 0 ? 0 : -1; mb = -1; }
        if (ma >= 0) gemm_group<2, 1>(ma, 1, nt << 4, kend, Ap, Bv, epi_o, li, lq);
        if (mb >= 0) gemm_group<2, 1>(mb, 1, nt << 4, kend, Ap, Bv, epi_o, li, lq);
      }
    }
    __syncthreads();
    // h1 = LN(x) + (o Wo^T + bo)
    rag_packed(mq0, mqn, DK >> 2, D, Mat{bQ, DS}, wo, [&](int r, int c) { return bQN[r * DS + c]; }, [&](int r, int c, float v, float res) {
      const float h = res + v;
      bXS[r * DS + c] = h;
      return h;
    }, lane, wave, [&](int rb, int c, const float (&gv)[4]) { if (do_save) gstore4(a.save_h1 + h1_off(i, b, ly.n_blocks, L, D), rb, c, gv); });
    __syncthreads();
    ln_rows(nw, bXS + rq0 * DS, bQN + rq0 * DS, LP - rq0, DS, D, s_ln + (4 * i + 2) * 64, s_ln + (4 * i + 3) * 64);
    __syncthreads();
    // PW-FFN: y = (drop2(relu(drop1(h2 W1^T + b1)) W2^T + b2) + h2) * keep
    const DropSite ds1 = drop_site(drop_on, seed, site_ffn1(i), seq, a.drop_thr, a.drop_scale);
    const DropSite ds2 = drop_site(drop_on, seed, site_ffn2(i), seq, a.drop_thr, a.drop_scale);
    const WFrag w2 = load_wfrag(pk(i * 6 + 5, 0), P + o.c2_b, D, NT, tid);
    rag_packed(mq0, mqn, DK >> 2, D, Mat{bQN, DS}, w1, NoPre{}, [&](int r, int c, float v, float) {
      const float h = fmaxf(v * drop_mul(ds1, r - SH, c), 0.f);
      bQ[r * DS + c] = h;
      return h;
    }, lane, wave, [&](int rb, int c, const float (&gv)[4]) { if (sv_r) gstore4(sv_r, rb, c, gv); });
    __syncthreads();
    rag_packed(mq0, mqn, DK >> 2, D, Mat{bQ, DS}, w2, [&](int r, int c) { return bQN[r * DS + c]; }, [&](int r, int c, float v, float res) {
      const float y = (v * drop_mul(ds2, r - SH, c) + res) * s_keep[r];
      bXS[r * DS + c] = y;
      return y;
    }, lane, wave, [&](int rb, int c, const float (&gv)[4]) { if (do_save) gstore4(a.save_x + x_off(i + 1, b, ly.n_blocks, L, D), rb, c, gv); });
    __syncthreads();
  }

  // ---- head: (last_conv) -> last LayerNorm -> hidden, pos/neg logits, BCE partial sums        (every position: a padded
  // row's hidden state is LayerNorm(0 or b_lc), its logits against the table's row 0 - outputs the reference has too)
  const bool lo_h = !TR_ && a.last_only != 0;
  int seam_th = 0;
  RagSeam hs = {};
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  if (!lo_h && r0 > SH) {                    // the positions in front of the computed tiles: exact zeros (S overlaid them)
    for (int i = tid; i < (r0 - SH) * DS; i += nthr) bXS[SH * DS + i] = 0.f;
    __syncthreads();
  }
  lds_f* xp = bXS + SH * DS;                 // position-indexed views
  lds_f* qnp = bQN + SH * DS;
  const lds_f* hin = xp;
  const int p0h = lo_h ? L - 1 : 0;          // first position the head computes
  if (kind == SRFRD_SRFR) {
    const WFrag wl = load_wfrag(pk(ly.n_blocks * 6, 0), P + ly.off_lc_b, di, (di + 15) >> 4, tid);
    const int mh0 = lo_h ? MT - 1 : 0;
    // (three strips of 45 columns: load_wfrag dealt strip wave % 3 to this wave; waves 0 .. 5 = 3 strips x 2 row-tile groups)
    {
      constexpr int nst = (di + 15) >> 4;
      const int nt = wave % nst, g = wave / nst;
      const int mtn_h = MT - mh0;
      auto epi = [&](int r_, int c, float v) { if (c < di) bQ[(r_ + (mh0 << 4)) * DS + c] = v; };
      if (g < 2) {
        if (g + 2 < mtn_h) gemm_group_packed<2>(g, 2, nt, DK >> 2, Mat{bXS + (mh0 << 4) * DS, DS}, wl, epi, lane);
        else if (g < mtn_h) gemm_group_packed<1>(g, 2, nt, DK >> 2, Mat{bXS + (mh0 << 4) * DS, DS}, wl, epi, lane);
      }
    }
    __syncthreads();
    hin = bQ + SH * DS;
  }
  ln_rows(nw, hin + p0h * DS, qnp + p0h * DS, L - p0h, DS, dout, s_ln + (4 * ly.n_blocks) * 64, s_ln + (4 * ly.n_blocks + 1) * 64);
  __syncthreads();
  if (lo_h) {
    for (int c = tid; c < dout; c += nthr) a.hidden[(int64_t)b * dout + c] = qnp[(L - 1) * DS + c];
  } else {
    const bool srfrn = kind == SRFRD_SRFRN;
    lds_f* kp = bK + SH * DS;
    lds_f* vp = bV + SH * DS;
    lds_f* s_dp = bXS + LP * DS;               // SEAM_: the logit gradients by position, behind the [LP][DS] view of x
    lds_f* s_dn = s_dp + LP;
    static_assert(LP * DS + 2 * LP <= LP * SLD, "logit gradients inside the x / scores matrix");
    {
      int t = tid / dout, c = tid - t * dout;
      constexpr int dt = nthr / dout, dc = nthr - dt * dout;
      for (; t < L;) {
        const float h = qnp[t * DS + c];
        a.hidden[(rowbase + t) * dout + c] = h;
        if (has_pos) {
          const float pv = c < di ? table((int64_t)s_pid[t + SH] * di + c)
                                  : (srfrn ? P[ly.off_side + clamp_id(a.pos_fk[rowbase + t], 2) * dfk + (c - di)] : 0.f);
          // (SEAM_: the row itself waits there - the logit pass forms the product - and x stays whole for the backward)
          kp[t * DS + c] = SEAM_ ? pv : h * pv;
        }
        if (has_neg) {
          const float nv = c < di ? table((int64_t)s_nid[t + SH] * di + c)
                                  : (srfrn ? P[ly.off_side + clamp_id(a.neg_fk[rowbase + t], 2) * dfk + (c - di)] : 0.f);
          vp[t * DS + c] = SEAM_ ? nv : h * nv;
        }
        t += dt; c += dc;
        if (c >= dout) { c -= dout; ++t; }
      }
    }
    __syncthreads();
    float sp = 0.f, sn = 0.f, cnt = 0.f;
    const int q = tid & (kRL - 1);
    for (int t = tid / kRL; t < L; t += nthr / kRL) {
      float ap = 0.f, an = 0.f;
#pragma unroll
      for (int j = 0; j < kQC; ++j) {
        const int c = q + kRL * j;
        if (c < dout) {
          if constexpr (SEAM_) {               // the stand-alone forward's rounded products, summed as it sums them
            const float h = qnp[t * DS + c];
            ap += seam_product(h, kp[t * DS + c]);
            an += seam_product(h, vp[t * DS + c]);
          } else {
            if (has_pos) ap += kp[t * DS + c];
            if (has_neg) an += vp[t * DS + c];
          }
        }
      }
      const float pl = row_sum(ap), nl = row_sum(an);
      if (q == 0) {
        if (has_pos) a.pos_logits[rowbase + t] = pl;
        if (has_neg) a.neg_logits[rowbase + t] = nl;
        if constexpr (SEAM_) {
          float dp = 0.f, dn = 0.f;
          bce_dlogits(s_pid[t + SH], pl, nl, dp, dn);
          s_dp[t] = dp;
          s_dn[t] = dn;
        }
        if (do_loss && s_pid[t + SH] != 0) {     // trainer.py:36-38: both terms indexed by pos != 0
          sp += softplus_fast(-pl);
          sn += softplus_fast(nl);
          cnt += 1.f;
        }
      }
    }
    if (do_loss) {
      sp = wave_sum(sp); sn = wave_sum(sn); cnt = wave_sum(cnt);
      if (lane == 0) {
        s_misc[8 + wave * 3 + 0] = sp;
        s_misc[8 + wave * 3 + 1] = sn;
        s_misc[8 + wave * 3 + 2] = cnt;
      }
      __syncthreads();
      if (tid < 3) {
        float s = 0.f;
        for (int w = 0; w < nw; ++w) s += s_misc[8 + w * 3 + tid];
        a.loss_part[(int64_t)b * 3 + tid] = s;
      }
    }
    if constexpr (SEAM_) {
      // (the barrier of the loss sums stands between the logit gradients' stores and these reads)
      const int l0 = tid & 63;
      const unsigned long long ng = __ballot(l0 < L && (s_in[l0 + SH] != 0 || s_dp[l0] != 0.f || s_dn[l0] != 0.f));
      seam_th = ng ? (int)__builtin_ctzll(ng) : L;
      if (a.ragged_off) seam_th = 0;
      seam_th = __builtin_amdgcn_readfirstlane(seam_th);
      const int ph0 = rag_head_range(seam_th, t0 >= 1 ? t0 - 1 : 0).pos0;
      hs.th = seam_th;
      hs.t0 = t0;
      if (has_fake && tid < L) {             // (requested in front of the atomics: the memory queue retires in order)
        hs.fk = a.fk_ids ? clamp_id(a.fk_ids[rowbase + tid], 2) : 0;
        hs.pfk = a.pos_fk ? clamp_id(a.pos_fk[rowbase + tid], 2) : 0;
        hs.nfk = a.neg_fk ? clamp_id(a.neg_fk[rowbase + tid], 2) : 0;
      }
      // d hidden of the head range goes where the backward reads it: its slot kRagSeamG, position-indexed like xp - over the
      // last_conv output / q matrix, which is dead (the rows it reads wait in kp / vp, the hidden rows in qnp)
      lds_f* sgp = xp + kRagSeamG * kRagSlot;
      const int B = a.B;
      int t = ph0 + tid / dout, c = tid - (tid / dout) * dout;
      constexpr int dt = nthr / dout, dc = nthr - dt * dout;
      for (; t < L;) {
        const float dp = s_dp[t], dn = s_dn[t];
        float dh = 0.f;
        if (c < di || srfrn) dh = head_dh_as_backward<K_>(dp, kp[t * DS + c], dn, vp[t * DS + c]);
        sgp[t * DS + c] = dh;
        if (c < di) {
          const float h = qnp[t * DS + c];
          const int pid = s_pid[t + SH], nid = s_nid[t + SH];
          if (a.contrib != nullptr) {          // deterministic mode: see srfrd_encoder_bwd_kernel.inc
            a.contrib[(((int64_t)0 * B + b) * L + t) * di + c] = pid != 0 ? head_contrib(dp, h) : 0.f;
            a.contrib[(((int64_t)1 * B + b) * L + t) * di + c] = nid != 0 ? head_contrib(dn, h) : 0.f;
          } else {
            if (pid != 0 && dp != 0.f) atomicAdd(&a.grad_table[(int64_t)pid * di + c], head_contrib(dp, h));
            if (nid != 0 && dn != 0.f) atomicAdd(&a.grad_table[(int64_t)nid * di + c], head_contrib(dn, h));
          }
        }
        t += dt; c += dc;
        if (c >= dout) { c -= dout; ++t; }
      }
      if (a.contrib != nullptr)              // (the sorted reduction reads every row of the batch: rows in front of the head are zeros)
        for (int idx = tid; idx < ph0 * di; idx += nthr) {
          a.contrib[(((int64_t)0 * B + b) * L) * di + idx] = 0.f;
          a.contrib[(((int64_t)1 * B + b) * L) * di + idx] = 0.f;
        }
      // the ids, position-indexed as the backward holds them (lanes 0 .. L - 1 of the first wave; zeros behind)
      if (tid < L) {
        hs.id = s_in[tid + SH];
        hs.pid = s_pid[tid + SH];
        hs.nid = s_nid[tid + SH];
        if constexpr (K_ == SRFRD_SRFRN) {   // (only its side-channel sums still read the logit gradients)
          hs.dp = s_dp[tid];
          hs.dn = s_dn[tid];
        }
      }
    }
  }
  __syncthreads();
  return hs;
}

template <int K_, int T_, int DI_>
__global__ void __launch_bounds__(512, 4) encoder_fwd_ragged_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  constexpr int D = 50, L = 50, LP = 64, DS = 54, SLD = 66;
  constexpr int nthr = 512;
  int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  constexpr int szA = LP * DS, szX = LP * SLD;
  const int tailsz = 4 * LP + 64 + ln_cache_floats(ly.n_blocks);
  const RagT0 t0v = rag_load_t0(a, tid);
  lds_f* c_cur = (lds_f*)smem;
  auto carve = [&](int64_t n) -> lds_f* { lds_f* p = c_cur; c_cur += n; return p; };
  {
    Geom g = make_geom(L, D);
    const int total = (int)fwd_lds_floats(g, ly.n_blocks);
    for (int i = tid; i < total; i += nthr) ((lds_f*)smem)[i] = 0.f;
  }
  lds_f* tail = carve(tailsz);
  RagFwdLds m;
  m.bXS = carve(szX);
  m.bQN = carve(szA);
  m.bQ = carve(szA);
  m.bK = carve(szA);
  m.bV = carve(szA + kSlack);
  m.s_in = (lds_i*)tail;
  m.s_keep = tail + LP;
  m.s_pid = (lds_i*)(tail + 2 * LP);
  m.s_nid = (lds_i*)(tail + 3 * LP);
  m.s_misc = tail + 4 * LP;
  lds_f* s_ln = m.s_misc + 64;
  m.s_ln = s_ln;
  __syncthreads();
  fill_ln_cache(s_ln, a.dense, ly);
  const uint32_t seed = a.seed_dev ? *a.seed_dev : a.seed;

  STAMP_INIT
  for (int iter = 0;; ++iter) {
    const int b = __builtin_amdgcn_readfirstlane(rag_take(a, (lds_i*)m.bXS, iter, tid, t0v));      // (bXS: free between sequences)
    if (b < 0) break;
    rag_fwd_seq<K_, T_, DI_>(a, m, b, tid, wave, seed);
  }
}

}  // namespace SRFRD_NS
