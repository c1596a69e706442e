// Kernel template of the fused encoder backward pass; included by srfrd_encoder_bwd.hip (LDS-resident build)
// and srfrd_encoder_bwd_long.hip (SRFRD_BUF_GLOBAL build).
namespace SRFRD_NS {


// ================================================================================================
// backward
// ================================================================================================
// column sums over rows < L of an LDS matrix, added into a slab vector by ONE wave (fixed owner => the
// read-modify-write on the slab is race-free and order-deterministic)
__device__ __forceinline__ void colsum_to_slab(int owner_wave, const lds_f* buf, int ld, int rows, int cols, float* dst) {
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) != owner_wave) return;
  const int lane = threadIdx.x & 63;
  if (lane < cols) {
    float s = 0.f;
    for (int t = 0; t < rows; ++t) s += buf[t * ld + lane];
    dst[lane] += s;
  }
}

// D_, LP_, NW_ > 0: geometry and wave count fixed at compile time (strides become immediates, tile loops
// resolve statically); 0: read at run time (the generic instantiation covers every other shape).
template <int D_, int LP_, int NW_, int L_ = 0, int K_ = -1, int T_ = 0, int DI_ = 0>
__global__ void __launch_bounds__(NW_ > 0 ? NW_ * 64 : 512) encoder_bwd_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = NW_ > 0 ? NW_ : (int)(blockDim.x >> 6), nthr = nw << 6;
  const int L = L_ > 0 ? L_ : a.L;       // (L_: the reference's default maxlen = 50 gets loop bounds and k-ranges at compile time)
  const int D = D_ > 0 ? D_ : ly.D;
  const int LP = LP_ > 0 ? LP_ : ((L + 15) & ~15);
  const int DK = (D + 3) & ~3, DS = DK + 2, SLD = LP + 2, NT = (D + 15) >> 4, MT = LP >> 4;
  const int LK = (L + 3) & ~3;           // token k-range of the gradient GEMMs: rows >= L of every gradient matrix are zero
  Geom g;
  g.L = L; g.LP = LP; g.D = D; g.DK = DK; g.DS = DS; g.SLD = SLD; g.NT = NT; g.MT = MT;
  // global -> LDS block copies: one chunk (one memory round trip) covers a whole [L][D] block in the specialised shapes
  constexpr bool CV2 = D_ > 0 && (D_ & 1) == 0;
  constexpr int CIT = D_ > 0 ? (LP_ * (CV2 ? D_ / 2 : D_) + NW_ * 64 - 1) / (NW_ * 64) : 4;
  constexpr int PIT = D_ > 0 ? (LP_ * LP_ / 2 + NW_ * 64 - 1) / (NW_ * 64) : 4;      // the [L][LP] probability block, in pairs
  const int szA = LP * DS, szS = imax(LP * SLD, szA);
  const int tailsz = (kHeadRows + 1) * LP + 64 + 2 * ln_cache_floats(ly.n_blocks);
#ifdef SRFRD_BUF_GLOBAL
  // long-sequence build: buffers are taken from LDS while they fit (in priority order), then from the workgroup's
  // slice of the global scratch; pointers are generic, the hardware routes each flat access by aperture
  float* c_lds = (float*)smem;
  int64_t c_left = a.lds_floats;
  float* c_glb = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
  auto carve = [&](int64_t n) -> lds_f* {
    if (n <= c_left) { float* p = c_lds; c_lds += n; c_left -= n; return p; }
    float* p = c_glb; c_glb += n; return p;
  };
  for (int i = tid; i < a.lds_floats; i += nthr) ((float*)smem)[i] = 0.f;
  for (int64_t i = tid; i < a.scratch_stride; i += nthr) c_glb[i] = 0.f;
#else
  lds_f* c_cur = (lds_f*)smem;
  auto carve = [&](int64_t n) -> lds_f* { lds_f* p = c_cur; c_cur += n; return p; };
  {
    const int total = (int)bwd_lds_floats(g, ly.n_blocks);
    for (int i = tid; i < total; i += nthr) ((lds_f*)smem)[i] = 0.f;
  }
#endif
  lds_f* tail = carve(tailsz);
  lds_f *bX, *bQN, *bQ, *bK, *bV, *bO, *bG, *bT, *S1, *S2;
  bX = carve(szA); bQN = carve(szA); bQ = carve(szA); bK = carve(szA);
  bV = carve(szA); bO = carve(szA); bG = carve(szA); bT = carve(szA + kSlack);
  S1 = carve(szS); S2 = carve(szS + kSlack);
  lds_i* s_in = (lds_i*)(tail + kRowIn * LP);
  lds_f* s_keep = tail + kRowKeep * LP;
  lds_i* s_pid = (lds_i*)(tail + kRowPid * LP);
  lds_i* s_nid = (lds_i*)(tail + kRowNid * LP);
  lds_i* s_fk = (lds_i*)(tail + kRowFk * LP);
  lds_i* s_pfk = (lds_i*)(tail + kRowPfk * LP);
  lds_i* s_nfk = (lds_i*)(tail + kRowNfk * LP);
  lds_f* s_dpl = tail + kRowDpl * LP;
  lds_f* s_dnl = tail + kRowDnl * LP;
  lds_f* s_misc = tail + (kHeadRows + 1) * LP;        // 64
  lds_f* s_ln = s_misc + 64;             // LayerNorm parameter cache
  lds_f* s_lng = s_ln + ln_cache_floats(ly.n_blocks);   // LayerNorm parameter-gradient accumulators (same indexing)
  __syncthreads();
  fill_ln_cache(s_ln, a.dense, ly);
  const float* P = a.dense;
  // T_ = 1: fused training step (targets present, fused BCE, no upstream hidden gradient, dropout on, no debug taps):
  // the run-time "is this pointer null / is this mode on" questions are answered at compile time
  constexpr bool TR_ = T_ != 0;
  const bool has_pos = TR_ || a.pos_ids != nullptr, has_neg = TR_ || a.neg_ids != nullptr;
  const bool drop_on = TR_ || a.drop_on != 0, fused = TR_ || a.fused_bce != 0;
  const float* up_hidden = TR_ ? nullptr : a.d_hidden;
  const int kind = K_ >= 0 ? K_ : ly.kind;
  const bool is_sas = kind == SRFRD_SASREC;
  const bool has_fake = kind == SRFRD_SRFR || kind == SRFRD_SRFRN;
  const bool is_srfu = kind >= SRFRD_SRFU_B;
  // DI_: item width at compile time (DI_ == D_: SASRec / SRFU kinds, no side channel; DI_ < D_ with K_ = SRFR / SRFRN:
  // the reference's default 45 + 5 split) - the (position, channel) walks below divide by these
  constexpr int DIc = DI_ > 0 ? DI_ : (K_ == SRFRD_SASREC && D_ > 0 ? D_ : 0);
  const int di = DIc > 0 ? DIc : ly.d_item, dfk = DIc > 0 ? D_ - DIc : ly.d_fake;
  const int dout = DIc > 0 ? (K_ == SRFRD_SRFR ? DIc : D_) : ly.d_out;
  const float sqrtD = sqrtf((float)di);
  const float qscale = a.qscale;
  const uint32_t seed = a.seed_dev ? *a.seed_dev : a.seed;
  const int B = a.B;
  // packed weight of matrix `mat` (block*6 + {Wq,Wk,Wv,Wo,W1,W2}; n_blocks*6 = last_conv); form 0: x W^T, 1: dy W
  auto pk = [&](int mat, int form) {
    return PackedB{reinterpret_cast<const float4*>(a.packed) + ((int64_t)mat * 2 + form) * (kPackFloats / 4)};
  };
  float* slab = a.grad_slabs + (int64_t)blockIdx.x * ly.n_dense;
  const bool fold_bias = (D & 15) != 0;       // a spare padded column exists in the last n-tile
  // Bias gradients ride in the dW GEMMs: every matrix that is the X operand of one (block input, LayerNorm outputs,
  // FFN activation, attention output) carries 1.0 in column D of its rows < L, so column D of dY^T [X | 1] is the
  // column sum of dY.  The column is invisible elsewhere: k = D.. of every packed weight is zero, every epilogue and
  // row pass stops at D, and no gradient matrix ever meets another one's column D in a product.
  auto ones_col = [&](lds_f* buf) {
    if (fold_bias)
      for (int t = tid; t < L; t += nthr) buf[t * DS + D] = 1.0f;
  };
  // Column sums over the positions of a sequence for the small side tables (fake / user-label embeddings): output p is
  // owned by wave p % nw, its lanes take the positions, one butterfly reduction, one no-return add by lane 0 - a fixed
  // adder and a fixed order per slab element.  (A single wave walking the positions one by one and doing a global
  // load-add-store per output was ~20 k cycles per sequence with every other wave parked at the barrier.)
  auto side_sums = [&](int n_out, auto term, auto dst_off) {
    for (int p = wave; p < n_out; p += nw) {
      float sacc = 0.f;
      for (int t = lane; t < L; t += 64) sacc += term(p, t);
      sacc = wave_sum(sacc);
      if (lane == 0) atomicAdd(&slab[dst_off(p)], sacc);
    }
  };
  // Slab initialisation.  Every weight / bias / LayerNorm gradient entry is fully overwritten (the first sequence of the
  // workgroup stores instead of accumulating; LayerNorm entries are flushed from LDS at the end), so only the entries
  // that are accumulated with += from the start - position table, side table, and the biases when they are not folded
  // into the dW GEMMs - need zeros: 10 KB instead of 140 KB per workgroup.
  for (int64_t i = tid; i < (fold_bias ? (int64_t)ly.blk0 : (int64_t)ly.n_dense); i += nthr) slab[i] = 0.f;
  __syncthreads();
  const float keep_scale = drop_on ? a.drop_scale : 1.0f;

  STAMP_INIT
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t rowbase = (int64_t)b * L;
    const uint32_t seq = (uint32_t)(a.seq0 + b);
    const int rmw = b != (int)blockIdx.x;      // first sequence of this workgroup: the slab is still all zero
    // the last block's output is requested first and lands in LDS after the id pass: one round trip for both
    // (specialised shapes only: there one G2L covers the block; the generic kernel copies in chunks further down)
    const float* last_x = a.c_save_x + x_off(ly.n_blocks, b, ly.n_blocks, L, D);
    G2L<CIT, CV2> g_last;
    if constexpr (D_ > 0) g_last.load(last_x, L, D, nthr);
    // post-attention checkpoint of the block the loop below starts with: in flight while the logits / last-LayerNorm
    // backward runs; each iteration requests the next block's ahead of time in the same way
    G2L<CIT, CV2> g_h1, g_r;
    if constexpr (D_ > 0) {
      g_h1.load(a.c_save_h1 + h1_off(ly.n_blocks - 1, b, ly.n_blocks, L, D), L, D, nthr);
      g_r.load(a.c_save_aux + aux_off(ly.n_blocks - 1, b, ly.n_blocks, L, LP, D, D_ == 0 ? ly.n_heads : 1).r, L, D, nthr);
    }
    for (int t = tid; t < LP; t += nthr) {
      const bool in = t < L;
      const int id = in ? clamp_id(a.in_ids[rowbase + t], ly.n_items) : 0;
      const int pid = (in && has_pos) ? clamp_id(a.pos_ids[rowbase + t], ly.n_items) : 0;
      const int nid = (in && has_neg) ? clamp_id(a.neg_ids[rowbase + t], ly.n_items) : 0;
      s_in[t] = id;
      s_keep[t] = id != 0 ? 1.f : 0.f;
      s_pid[t] = pid;
      s_nid[t] = nid;
      s_fk[t] = (in && a.fk_ids) ? clamp_id(a.fk_ids[rowbase + t], 2) : 0;
      s_pfk[t] = (in && a.pos_fk) ? clamp_id(a.pos_fk[rowbase + t], 2) : 0;
      s_nfk[t] = (in && a.neg_fk) ? clamp_id(a.neg_fk[rowbase + t], 2) : 0;
      float dp = 0.f, dn = 0.f;
      if (in) {
        if (fused) {
          const float pl = a.c_pl[rowbase + t], nl = a.c_nl[rowbase + t];     // (not behind `pid != 0`: same round trip)
          bce_dlogits(pid, pl, nl, dp, dn);
        } else {
          if (a.d_pos) dp = a.d_pos[rowbase + t];
          if (a.d_neg) dn = a.d_neg[rowbase + t];
        }
      }
      s_dpl[t] = dp;
      s_dnl[t] = dn;
    }
    if (is_srfu && wave == 0) {
      const int lab = user_label_wave(kind, a.fk_ids ? a.fk_ids + rowbase : nullptr, L, ly.n_labels);
      if (lane == 0) ((lds_i*)s_misc)[0] = lab;
    }
    // final block output (input of last_conv / last LayerNorm) -> bX ; gradient pad rows must be exact zeros
    if constexpr (D_ > 0) g_last.store(bX, DS, L, D, nthr);
    else copy_g2l<CIT, CV2>(bX, DS, last_x, L, D, nthr);
    ones_col(bX);
    for (int i = tid; i < (LP - L) * DS; i += nthr) bG[L * DS + i] = 0.f;
    __syncthreads();

    const lds_f* lnin = bX;
    if (kind == SRFRD_SRFR) {
      const WFrag wl = load_wfrag(pk(ly.n_blocks * 6, 0), P + ly.off_lc_b, di, (di + 15) >> 4);
      gemm_packed(nw, MT, (di + 15) >> 4, DK, Mat{bX, DS}, wl, [&](int r, int c, float v) { if (c < di) bQ[r * DS + c] = v; });
      __syncthreads();
      lnin = bQ;
    }
    // ---- logits backward.  Pass 1: dh -> bG and the hidden rows -> bT.  Threads walk (position, channel) linearly, so a
    // wave reads each gathered item row as one contiguous 4*d_item-byte segment (the rows sit anywhere in the table).
    {
      const bool srfrn = kind == SRFRD_SRFRN;
      const int n = L * dout;
      constexpr int GIT = D_ > 0 ? (LP_ * D_ + NW_ * 64 - 1) / (NW_ * 64) : 4;      // d_out <= D
      const float* hid = a.c_hidden + rowbase * dout;
      const float* dhid = up_hidden ? up_hidden + rowbase * dout : nullptr;
      // (two instantiations of the chunk loop, chosen by a kernel-uniform test: the fp32 form keeps its single selected-address
      // load per gather; the bf16-shadow form loads 2-byte item elements)
      auto chunks = [&](auto bf16_shadow) {
        constexpr bool H = decltype(bf16_shadow)::value;
        for (int base = 0; base < n; base += GIT * nthr) {
          // every gather of the chunk is in flight before the first use (clamped indices, selected addresses: no branch)
          float hv[GIT], dv[GIT], pv[GIT], nv[GIT];
#pragma unroll
          for (int u = 0; u < GIT; ++u) {
            const int i = min(base + u * nthr + tid, n - 1);
            const int t = i / dout, c = i - t * dout;
            const bool item = c < di;
            const int prow = item ? s_pid[t] : s_pfk[t], nrow = item ? s_nid[t] : s_nfk[t];
            const int w = item ? di : dfk, cc = item ? c : c - di;
            const bool use = item || srfrn;
            hv[u] = hid[i];
            dv[u] = dhid ? dhid[i] : 0.f;
            if constexpr (H) {
              const float* side = P + ly.off_side;
              const float ps = side[(use && !item) ? prow * dfk + cc : 0], ns = side[(use && !item) ? nrow * dfk + cc : 0];
              const uint16_t ph = a.table16[item ? (int64_t)prow * di + cc : 0], nh = a.table16[item ? (int64_t)nrow * di + cc : 0];
              pv[u] = item ? bf16_to_f32(ph) : ps;
              nv[u] = item ? bf16_to_f32(nh) : ns;
            } else {
              const float* src = item ? a.table : P + ly.off_side;
              pv[u] = src[use ? (int64_t)prow * w + cc : 0];
              nv[u] = src[use ? (int64_t)nrow * w + cc : 0];
            }
          }
#pragma unroll
          for (int u = 0; u < GIT; ++u) {
            const int i = base + u * nthr + tid;
            if (i < n) {
              const int t = i / dout, c = i - t * dout;
              float dh = dv[u];
              if (c < di || srfrn) {
                if (has_pos) dh += s_dpl[t] * pv[u];
                if (has_neg) dh += s_dnl[t] * nv[u];
              }
              bT[t * DS + c] = hv[u];
              bG[t * DS + c] = dh;
            }
          }
        }
      };
      if (a.table16 != nullptr) chunks(std::true_type{});
      else chunks(std::false_type{});
      if (dout < D)                                    // SRFR: channels d_out..D-1 of the LN input gradient are zero
        for (int idx = tid; idx < L * (D - dout); idx += nthr) {
          const int tt = idx / (D - dout), cc = dout + idx - tt * (D - dout);
          bG[tt * DS + cc] = 0.f;
        }
    }
    __syncthreads();
    // Pass 2: item-table scatter (float atomics, no return), again linear in (position, channel): every wave-instruction
    // adds to at most two contiguous row segments - the shape the memory-side atomic units run at full rate for.
    // Row 0 (padding_idx) receives none.
    {
      int t = tid / di, c = tid - t * di;
      const int dt = nthr / di, dc = nthr - dt * di;
      for (; t < L; ) {
        const float h = bT[t * DS + c];
        const float dp = s_dpl[t], dn = s_dnl[t];
        const int pid = s_pid[t], nid = s_nid[t];
        if (a.contrib != nullptr) {
          // deterministic mode: every (target kind, sequence, position) owns a row of `contrib`; srfrd_table_reduce sums
          // the rows of one item in a fixed order afterwards (zeros where there is nothing to add)
          a.contrib[(((int64_t)0 * B + b) * L + t) * di + c] = (has_pos && pid != 0) ? dp * h : 0.f;
          a.contrib[(((int64_t)1 * B + b) * L + t) * di + c] = (has_neg && nid != 0) ? dn * h : 0.f;
        } else {
          if (has_pos && pid != 0 && dp != 0.f) atomicAdd(&a.grad_table[(int64_t)pid * di + c], dp * h);
          if (has_neg && nid != 0 && dn != 0.f) atomicAdd(&a.grad_table[(int64_t)nid * di + c], dn * h);
        }
        t += dt; c += dc;
        if (c >= di) { c -= di; ++t; }
      }
    }
    if (kind == SRFRD_SRFRN && (has_pos || has_neg))      // fake_embed rows 1 (fake) and 2 (real); row 0 is padding_idx
      side_sums(2 * dfk, [&](int p, int t) {
        const int dq = dfk > 0 ? dfk : 1, f = 1 + p / dq, c = p - (f - 1) * dq;
        const float w = (s_pfk[t] == f ? s_dpl[t] : 0.f) + (s_nfk[t] == f ? s_dnl[t] : 0.f);
        return w * bT[t * DS + di + c];
      }, [&](int p) { return ly.off_side + dfk + p; });
    // ---- last LayerNorm backward: dx -> bK, g * xhat -> bO; dgamma / dbeta as ones-row GEMMs on the matrix cores
    ln_bwd_rows<false>(nw, bG, lnin, bK, bO, L, LP, DS, dout, s_ln + (4 * ly.n_blocks) * 64);
    __syncthreads();
    gemm_tiles<0>(nw, 1, (dout + 15) >> 4, LK, OnesRow{}, Mat{bG, DS},
                  [=](int r, int c, float v) { if (r == 0 && c < dout) s_lng[(4 * ly.n_blocks + 1) * 64 + c] += v; });
    gemm_tiles<0>(nw, 1, (dout + 15) >> 4, LK, OnesRow{}, Mat{bO, DS},
                  [=](int r, int c, float v) { if (r == 0 && c < dout) s_lng[(4 * ly.n_blocks + 0) * 64 + c] += v; });
    // no barrier: the buffers these two column-sum GEMMs read (old bG, bO) are not written before the next barrier
    { lds_f* t_ = bG; bG = bK; bK = t_; }
    if (kind == SRFRD_SRFR) {             // hc = hf Wlc^T + blc
      gemm_slab(nw, (di + 15) >> 4, NT, LK, MatT{bG, DS}, Mat{bX, DS},
                SlabWB{slab, ly.off_lc_w, fold_bias ? ly.off_lc_b : -1, di, D, rmw});
      if (!fold_bias) colsum_to_slab(0, bG, DS, L, di, slab + ly.off_lc_b);
      const WFrag wln = load_wfrag(pk(ly.n_blocks * 6, 1), nullptr, 0, NT);
      gemm_packed(nw, MT, NT, (di + 3) & ~3, Mat{bG, DS}, wln, [&](int r, int c, float v) { if (c < D) bT[r * DS + c] = v; });
      __syncthreads();
      lds_f* t_ = bG; bG = bT; bT = t_;
    }
    if constexpr (!TR_) tap(a, b, 0, bG, L, D, DS);

    for (int i = ly.n_blocks - 1; i >= 0; --i) {
      const BlkOff o = blk_off(ly.blk0 + i * ly.blk_stride, D);
      const int tb = 1 + 4 * i;
      const DropSite ds2 = drop_site(drop_on, seed, site_ffn2(i), seq, a.drop_thr, a.drop_scale);
      launder(bX); launder(bQN); launder(bQ); launder(bK); launder(bV); launder(bO); launder(bG); launder(bT);
      launder(S1); launder(S2);
      const AuxOff ax = aux_off(i, b, ly.n_blocks, L, LP, D, D_ == 0 ? ly.n_heads : 1);
      // ================= FFN half: y = (drop2(a2) + h2) * keep, a2 = r W2^T + b2, r = relu(drop1(h2 W1^T + b1))
      // (r comes back from the forward's checkpoint: no W1 GEMM, no drop1 hash here)
      const WFrag w2n = load_wfrag(pk(i * 6 + 5, 1), nullptr, 0, NT);
      const WFrag w1n = load_wfrag(pk(i * 6 + 4, 1), nullptr, 0, NT);
      const SlabWB sl_w2{slab, o.c2_w, fold_bias ? o.c2_b : -1, D, D, rmw};
      const SlabWB sl_w1{slab, o.c1_w, fold_bias ? o.c1_b : -1, D, D, rmw};
      {
        for (int idx = tid; idx < L * D; idx += nthr) {
          const int t = idx / D, c = idx - t * D;
          bG[t * DS + c] *= s_keep[t];
        }
        if constexpr (D_ > 0) {
          g_h1.store(bX, DS, L, D, nthr);
          g_r.store(bQ, DS, L, D, nthr);
        } else {
          copy_g2l<CIT, CV2>(bX, DS, a.c_save_h1 + h1_off(i, b, ly.n_blocks, L, D), L, D, nthr);
          copy_g2l<CIT, CV2>(bQ, DS, a.c_save_aux + ax.r, L, D, nthr);
        }
        ones_col(bQ);
        ones_col(bQN);
      }
      __syncthreads();
      ln_rows(nw, bX, bQN, L, DS, D, s_ln + (4 * i + 2) * 64, s_ln + (4 * i + 3) * 64);      // h2
      for (int idx = tid; idx < LP * D; idx += nthr) {                             // dA2 = drop2'(dy)
        const int t = idx / D, c = idx - t * D;
        bK[t * DS + c] = t < L ? bG[t * DS + c] * drop_mul(ds2, t, c) : 0.f;
      }
      __syncthreads();
      // attention checkpoints (sign-coded probabilities, attention output): requested a phase before S1 / bO take them
      G2L<PIT, true> g_p;
      G2L<CIT, CV2> g_o;
      if constexpr (D_ > 0) {
        g_p.load(a.c_save_aux + ax.p, L, LP, nthr);
        g_o.load(a.c_save_aux + ax.o, L, D, nthr);
      }
      // (within a phase the register-operand GEMMs run first and the slab GEMMs last: a wait for a weight fragment
      // issued behind slab stores would also wait for the stores' acknowledgement - vmcnt retires in order)
      SlabPre pre_w2 = slab_preload(nw, NT, NT, sl_w2);       // old dW2 tiles: land under the packed GEMM below
      gemm_packed(nw, MT, NT, DK, Mat{bK, DS}, w2n, [&](int r, int c, float v) {
        if (c < D) bV[r * DS + c] = bQ[r * DS + c] > 0.f ? v * keep_scale : 0.f;               // dA1
      });
      gemm_slab(nw, NT, NT, LK, MatT{bK, DS}, Mat{bQ, DS}, sl_w2, pre_w2);                   // dW2 += dA2^T r (+ db2)
      if (!fold_bias) colsum_to_slab(0, bK, DS, L, D, slab + o.c2_b);
      __syncthreads();
      if constexpr (D_ > 0) {
        g_p.store(S1, SLD, L, LP, nthr);
        g_o.store(bO, DS, L, D, nthr);
      } else {
        copy_g2l<PIT, true>(S1, SLD, a.c_save_aux + ax.p, L, LP, nthr);
        copy_g2l<CIT, CV2>(bO, DS, a.c_save_aux + ax.o, L, D, nthr);
      }
      ones_col(bO);
      for (int idx = tid; idx < (LP - L) * SLD; idx += nthr) S1[L * SLD + idx] = 0.f;     // (S1 last held dk: pad rows)
      // block input (attention half): requested two phases before bX is free to take it
      const float* blk_x = a.c_save_x + x_off(i, b, ly.n_blocks, L, D);
      G2L<CIT, CV2> g_x;
      if constexpr (D_ > 0) g_x.load(blk_x, L, D, nthr);
      SlabPre pre_w1 = slab_preload(nw, NT, NT, sl_w1);
      gemm_packed(nw, MT, NT, DK, Mat{bV, DS}, w1n, [&](int r, int c, float v) { if (c < D) bG[r * DS + c] += v; });   // dh2 = dy + dA1 W1
      gemm_slab(nw, NT, NT, LK, MatT{bV, DS}, Mat{bQN, DS}, sl_w1, pre_w1);                  // dW1 += dA1^T h2 (+ db1)
      if (!fold_bias) colsum_to_slab(1 % nw, bV, DS, L, D, slab + o.c1_b);
      __syncthreads();
      // q (scaled), k, v of the forward: requested here, two short phases before bQ / bK / bV are free to take them
      G2L<CIT, CV2> g_q, g_k, g_v;
      if constexpr (D_ > 0) {
        g_v.load(a.c_save_aux + ax.v, L, D, nthr);
        g_q.load(a.c_save_aux + ax.q, L, D, nthr);
        g_k.load(a.c_save_aux + ax.k, L, D, nthr);
      }
      ln_bwd_rows<false>(nw, bG, bX, bT, bV, L, LP, DS, D, s_ln + (4 * i + 2) * 64);               // dh1 -> bT
      __syncthreads();
      gemm_tiles<0>(nw, 1, NT, LK, OnesRow{}, Mat{bG, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 3) * 64 + c] += v; });
      gemm_tiles<0>(nw, 1, NT, LK, OnesRow{}, Mat{bV, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 2) * 64 + c] += v; });
      { lds_f* t_ = bG; bG = bT; bT = t_; }        // (no barrier: see the last-LayerNorm column sums above)
      if constexpr (!TR_) tap(a, b, tb + 0, bG, L, D, DS);
      // ================= attention half: h1 = LN1(x) + o Wo^T + bo, o = drop(P) v  (P, o from the checkpoint)
      if constexpr (D_ > 0) g_x.store(bX, DS, L, D, nthr);
      else copy_g2l<CIT, CV2>(bX, DS, blk_x, L, D, nthr);
      ones_col(bX);
      __syncthreads();
      const WFrag won = load_wfrag(pk(i * 6 + 3, 1), nullptr, 0, NT);
      const SlabWB sl_wo{slab, o.out_w, fold_bias ? o.out_b : -1, D, D, rmw};
      if constexpr (D_ > 0) {
        g_v.store(bV, DS, L, D, nthr);
        g_q.store(bQ, DS, L, D, nthr);
        g_k.store(bK, DS, L, D, nthr);
      } else {
        copy_g2l<CIT, CV2>(bV, DS, a.c_save_aux + ax.v, L, D, nthr);
        copy_g2l<CIT, CV2>(bQ, DS, a.c_save_aux + ax.q, L, D, nthr);
        copy_g2l<CIT, CV2>(bK, DS, a.c_save_aux + ax.k, L, D, nthr);
      }
      ln_rows(nw, bX, bQN, L, DS, D, s_ln + (4 * i + 0) * 64, s_ln + (4 * i + 1) * 64);      // LN1(x): X operand of dWq
      __syncthreads();
      // one phase: do = dh1 Wo and dWo (q / k / v came back from the checkpoint)
      SlabPre pre_wo = slab_preload(nw, NT, NT, sl_wo);
      const SlabWB sl_wq{slab, o.in_w, fold_bias ? o.in_b : -1, D, D, rmw};
      const SlabWB sl_wk{slab, o.in_w + D * D, fold_bias ? o.in_b + D : -1, D, D, rmw};
      const SlabWB sl_wv{slab, o.in_w + 2 * D * D, fold_bias ? o.in_b + 2 * D : -1, D, D, rmw};
      gemm_packed(nw, MT, NT, DK, Mat{bG, DS}, won, [&](int r, int c, float v) { if (c < D) bT[r * DS + c] = v; });    // do = dh1 Wo
      // (requested only now: a wait for `won` behind these would have been a wait for them as well)
      const WFrag wqn = load_wfrag(pk(i * 6 + 0, 1), nullptr, 0, NT);
      const WFrag wkn = load_wfrag(pk(i * 6 + 1, 1), nullptr, 0, NT);
      const WFrag wvn = load_wfrag(pk(i * 6 + 2, 1), nullptr, 0, NT);
      gemm_slab(nw, NT, NT, LK, MatT{bG, DS}, Mat{bO, DS}, sl_wo, pre_wo);                   // dWo += dh1^T o (+ dbo)
      if (!fold_bias) colsum_to_slab(2 % nw, bG, DS, L, D, slab + o.out_b);
      __syncthreads();
      // H > 1 (generic instantiation only): the heads take turns in S1 / S2.  Head h owns columns [c0, c1): dv_h overlays
      // o's columns (dead), dPd_h = do_h v_h^T reads do with the other heads' columns as zero, dk_h = dS_h^T q_h overlays
      // v_h (dead once dPd_h exists) and, one barrier later, dq_h = dS_h k_h overlays q_h.  do stays whole until the last
      // head is through, so dx is then built in ITS buffer: (dq, dk, dv, dx) = (bQ, bV, bO, bT) instead of (bT, S1, bO, bQ).
      const int H = D_ == 0 ? ly.n_heads : 1;
      lds_f *dQb = bT, *dKb = S1, *dXb = bQ;       // (single head: P is dead by then, dk overlays it as [LP][DS])
      if (H > 1) {
        const int dh = D / H;
        for (int h = 0; h < H; ++h) {
          const int c0 = h * dh, c1 = c0 + dh;
          if (h > 0) {
            copy_g2l<PIT, true>(S1, SLD, a.c_save_aux + ax.p + (int64_t)h * L * LP, L, LP, nthr);
            __syncthreads();
          }
          gemm_tiles<3>(nw, MT, NT, LK, MatTPos{S1, SLD}, Mat{bT, DS},
                        [&](int r, int c, float v) { if (c >= c0 && c < c1) bO[r * DS + c] = v * keep_scale; });
          gemm_tiles<1>(nw, MT, MT, DK, MatCols{bT, DS, c0, c1}, MatT{bV, DS}, [&](int r, int c, float v) { S2[r * SLD + c] = v; });
          __syncthreads();
          softmax_bwd_rows(nw, S2, S1, L, SLD, LP, keep_scale);
          __syncthreads();
          gemm_tiles<3>(nw, MT, NT, LK, MatT{S2, SLD}, Mat{bQ, DS},
                        [&](int r, int c, float v) { if (c >= c0 && c < c1) bV[r * DS + c] = v; });             // dk_h
          __syncthreads();
          gemm_tiles<2>(nw, MT, NT, LK, Mat{S2, SLD}, Mat{bK, DS},
                        [&](int r, int c, float v) { if (c >= c0 && c < c1) bQ[r * DS + c] = v * qscale; });    // dq_h
          __syncthreads();
        }
        dQb = bQ; dKb = bV; dXb = bT;
      } else {
      gemm_tiles<3>(nw, MT, NT, LK, MatTPos{S1, SLD}, Mat{bT, DS},
                    [&](int r, int c, float v) { if (c < D) bO[r * DS + c] = v * keep_scale; });
      gemm_tiles<1>(nw, MT, MT, DK, Mat{bT, DS}, MatT{bV, DS}, [&](int r, int c, float v) { S2[r * SLD + c] = v; });
      __syncthreads();
      softmax_bwd_rows(nw, S2, S1, L, SLD, LP, keep_scale);          // dS = P * (dP - sum_j dP_j P_j), dP = mask * dPd
      __syncthreads();
      gemm_tiles<2>(nw, MT, NT, LK, Mat{S2, SLD}, Mat{bK, DS},                             // (dS is zero for keys >= L)
                    [&](int r, int c, float v) { if (c < D) bT[r * DS + c] = v * qscale; });   // dq (pre-scale; do is dead)
      gemm_tiles<3>(nw, MT, NT, LK, MatT{S2, SLD}, Mat{bQ, DS},
                    [&](int r, int c, float v) { if (c < D) dKb[r * DS + c] = v; });           // dk = dS^T q
      __syncthreads();
      }
      SlabPre pre_wq = slab_preload(nw, NT, NT, sl_wq);
      SlabPre pre_wk = slab_preload(nw, NT, NT, sl_wk);
      SlabPre pre_wv = slab_preload(nw, NT, NT, sl_wv);
      gemm_packed(nw, MT, NT, DK, Mat{dQb, DS}, wqn, [&](int r, int c, float v) { if (c < D) bG[r * DS + c] += v; });   // dLN1 = dh1 + dq Wq
      gemm_packed(nw, MT, NT, DK, Mat{dKb, DS}, wkn, [&](int r, int c, float v) { if (c < D) dXb[r * DS + c] = v; });   // dx  = dk Wk
      gemm_packed(nw, MT, NT, DK, Mat{bO, DS}, wvn, [&](int r, int c, float v) { if (c < D) dXb[r * DS + c] += v; });   //     + dv Wv
      slab_ready(pre_wq); slab_ready(pre_wk); slab_ready(pre_wv);     // (before the first slab store of the phase)
      gemm_slab(nw, NT, NT, LK, MatT{dQb, DS}, Mat{bQN, DS}, sl_wq, pre_wq);                  // dWq (+ dbq)
      gemm_slab(nw, NT, NT, LK, MatT{dKb, DS}, Mat{bX, DS}, sl_wk, pre_wk);                  // dWk (+ dbk)
      gemm_slab(nw, NT, NT, LK, MatT{bO, DS}, Mat{bX, DS}, sl_wv, pre_wv);                   // dWv (+ dbv)
      if (!fold_bias) {
        colsum_to_slab(0, dQb, DS, L, D, slab + o.in_b);
        colsum_to_slab(1 % nw, dKb, DS, L, D, slab + o.in_b + D);
        colsum_to_slab(2 % nw, bO, DS, L, D, slab + o.in_b + 2 * D);
      }
      __syncthreads();
      if constexpr (D_ > 0)
        if (i > 0) {                               // the next block's FFN checkpoints, two phases ahead
          g_h1.load(a.c_save_h1 + h1_off(i - 1, b, ly.n_blocks, L, D), L, D, nthr);
          g_r.load(a.c_save_aux + aux_off(i - 1, b, ly.n_blocks, L, LP, D, D_ == 0 ? ly.n_heads : 1).r, L, D, nthr);
        }
      ln_bwd_rows<true>(nw, bG, bX, dXb, S2, L, LP, DS, D, s_ln + (4 * i + 0) * 64);               //     + LN1 bwd
      __syncthreads();
      gemm_tiles<0>(nw, 1, NT, LK, OnesRow{}, Mat{bG, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 1) * 64 + c] += v; });
      gemm_tiles<0>(nw, 1, NT, LK, OnesRow{}, Mat{S2, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 0) * 64 + c] += v; });
      // No barrier here either, so the buffer the first column sum is still reading (old bG) must not be one the next
      // block writes before ITS first barrier (it stores the FFN activation into bQ right away): the new gradient becomes
      // bG, the dead dq / do buffer becomes bQ, and old bG retires to bT, which is not written for several phases.
      // (A plain bG <-> bQ swap here let waves 4-7, which have no column-sum tile, overwrite old bG under waves 0-3.)
      if (H > 1) { lds_f* t_ = bG; bG = bT; bT = t_; }
      else { lds_f* t_ = bG; bG = bQ; bQ = bT; bT = t_; }
      if constexpr (!TR_) tap(a, b, tb + 1, bG, L, D, DS);
    }

    // ---- embedding backward: item rows (atomics), position table, side channel
    {
      const DropSite dsE = drop_site(drop_on && is_sas, seed, SITE_EMB, seq, a.drop_thr, a.drop_scale);
      {
        int t = tid / di, c = tid - t * di;
        const int dt = nthr / di, dc = nthr - dt * di;
        for (; t < L; ) {
          float gv = bG[t * DS + c] * s_keep[t];
          if (is_sas) gv *= drop_mul(dsE, t, c);
          const int id = s_in[t];
          if (a.contrib != nullptr) a.contrib[(((int64_t)2 * B + b) * L + t) * di + c] = id != 0 ? (is_sas ? gv * sqrtD : gv) : 0.f;
          else if (id != 0) atomicAdd(&a.grad_table[(int64_t)id * di + c], is_sas ? gv * sqrtD : gv);
          // no-return atomic instead of a load-add-store: nothing waits for the old value.  (t, c) is owned by the
          // same thread for every sequence of the workgroup, so the order of the additions is fixed.
          atomicAdd(&slab[ly.off_pos + t * di + c], gv);
          t += dt; c += dc;
          if (c >= di) { c -= di; ++t; }
        }
      }
      if (has_fake)
        side_sums(2 * dfk, [&](int p, int t) {
          const int dq = dfk > 0 ? dfk : 1, f = 1 + p / dq, c = p - (f - 1) * dq;
          return s_fk[t] == f ? bG[t * DS + di + c] * s_keep[t] : 0.f;
        }, [&](int p) { return ly.off_side + dfk + p; });
      if (is_srfu) {
        const int lab = ((lds_i*)s_misc)[0];
        side_sums(D, [&](int c, int t) { return bG[t * DS + c] * s_keep[t]; }, [&](int c) { return ly.off_side + lab * D + c; });
      }
    }
    __syncthreads();
  }
  // LayerNorm parameter gradients: LDS accumulators -> slab (same vector indexing as the parameter cache)
  for (int idx = tid; idx < (4 * ly.n_blocks + 2) * 64; idx += nthr) {
    const int vec = idx >> 6, c = idx & 63;
    if (vec < 4 * ly.n_blocks) {
      const BlkOff o = blk_off(ly.blk0 + (vec >> 2) * ly.blk_stride, D);
      const int sel = vec & 3;
      if (c < D) slab[(sel == 0 ? o.ln1_w : sel == 1 ? o.ln1_b : sel == 2 ? o.ln2_w : o.ln2_b) + c] = s_lng[idx];
    } else if (c < dout) {
      slab[(vec == 4 * ly.n_blocks ? ly.off_ll_w : ly.off_ll_b) + c] = s_lng[idx];
    }
  }
}

}  // namespace SRFRD_NS
