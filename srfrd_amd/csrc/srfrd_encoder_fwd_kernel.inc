// Kernel template of the fused encoder forward pass; included by srfrd_encoder_fwd.hip (LDS-resident build)
// and srfrd_encoder_fwd_long.hip (SRFRD_BUF_GLOBAL build).
namespace SRFRD_NS {


// ================================================================================================
// forward
// ================================================================================================
// D_, LP_, NW_ > 0: geometry and wave count fixed at compile time (strides become immediates, tile loops
// resolve statically); 0: read at run time (the generic instantiation covers every other shape).
template <int D_, int LP_, int NW_, int L_ = 0, int K_ = -1, int T_ = 0, int DI_ = 0>
__global__ void __launch_bounds__(NW_ > 0 ? NW_ * 64 : 512, NW_ == 8 ? (LP_ <= 64 ? 4 : 2) : 1) encoder_fwd_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = NW_ > 0 ? NW_ : (int)(blockDim.x >> 6), nthr = nw << 6;
  const int L = L_ > 0 ? L_ : a.L;       // (L_: the reference's default maxlen = 50 gets loop bounds and k-ranges at compile time)
  const int D = D_ > 0 ? D_ : ly.D;
  const int LP = LP_ > 0 ? LP_ : ((L + 15) & ~15);
  const int DK = (D + 3) & ~3, DS = DK + 2, SLD = LP + 2, NT = (D + 15) >> 4, MT = LP >> 4;
  Geom g;
  g.L = L; g.LP = LP; g.D = D; g.DK = DK; g.DS = DS; g.SLD = SLD; g.NT = NT; g.MT = MT;
  const int szA = LP * DS, szX = imax(szA, LP * SLD);
  const int tailsz = 4 * LP + 64 + ln_cache_floats(ly.n_blocks);
#ifdef SRFRD_BUF_GLOBAL
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
    const int total = (int)fwd_lds_floats(g, ly.n_blocks);
    for (int i = tid; i < total; i += nthr) ((lds_f*)smem)[i] = 0.f;
  }
#endif
  lds_f* tail = carve(tailsz);
  lds_f *bXS, *bQN, *bQ, *bK, *bV;
#ifdef SRFRD_BUF_GLOBAL
  // (the activation matrices take the LDS share first; the scores and the input go to scratch when it runs out)
  bQN = carve(szA); bQ = carve(szA); bK = carve(szA); bV = carve(szA + kSlack);
  bXS = carve(szX + kSlack);
#else
  bXS = carve(szX); bQN = carve(szA); bQ = carve(szA); bK = carve(szA); bV = carve(szA + kSlack);
#endif
  lds_i* s_in = (lds_i*)tail;
  lds_f* s_keep = tail + LP;
  lds_i* s_pid = (lds_i*)(tail + 2 * LP);
  lds_i* s_nid = (lds_i*)(tail + 3 * LP);
  lds_f* s_misc = tail + 4 * LP;          // 64 floats
  lds_f* s_ln = s_misc + 64;              // LayerNorm parameter cache
  __syncthreads();
  fill_ln_cache(s_ln, a.dense, ly);

  const float* P = a.dense;
  const ItemTable table{a.table, a.table16};
  // T_ = 1: fused training step (targets, checkpoints and loss sums all requested, dropout on, no debug taps): the
  // run-time "is this pointer null / is this mode on" questions are answered at compile time
  constexpr bool TR_ = T_ != 0;
  const bool has_pos = TR_ || a.pos_ids != nullptr, has_neg = TR_ || a.neg_ids != nullptr;
  const bool drop_on = TR_ || a.drop_on != 0, do_save = TR_ || a.save_x != nullptr, do_loss = TR_ || a.loss_part != nullptr;
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

  STAMP_INIT
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t rowbase = (int64_t)b * L;
    const uint32_t seq = (uint32_t)(a.seq0 + b);
    for (int t = tid; t < LP; t += nthr) {
      const int id = t < L ? clamp_id(a.in_ids[rowbase + t], ly.n_items) : 0;
      s_in[t] = id;
      s_keep[t] = id != 0 ? 1.f : 0.f;
      s_pid[t] = (t < L && has_pos) ? clamp_id(a.pos_ids[rowbase + t], ly.n_items) : 0;
      s_nid[t] = (t < L && has_neg) ? clamp_id(a.neg_ids[rowbase + t], ly.n_items) : 0;
    }
    if (is_srfu && wave == 0) {
      const int lab = user_label_wave(kind, a.fk_ids ? a.fk_ids + rowbase : nullptr, L, ly.n_labels);
      if (lane == 0) ((lds_i*)s_misc)[0] = lab;
    }
    __syncthreads();

    // ---- embedding: gather + position (+ side channel) + pad mask          (SURVEY 3.4 steps 1-4)
    {
      const DropSite dsE = drop_site(drop_on && is_sas, seed, SITE_EMB, seq, a.drop_thr, a.drop_scale);
      const int lab = is_srfu ? ((lds_i*)s_misc)[0] : 0;
      // threads walk (position, channel) linearly: a wave reads each gathered item row as one contiguous segment
      int t = tid / D, c = tid - t * D;
      const int dt = nthr / D, dc = nthr - dt * D;
      for (; t < L;) {
        const int id = s_in[t];
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
        v *= s_keep[t];
        bXS[t * DS + c] = v;
        if (do_save) a.save_x[x_off(0, b, ly.n_blocks, L, D) + t * D + c] = v;
        t += dt; c += dc;
        if (c >= D) { c -= D; ++t; }
      }
    }
    __syncthreads();
    if constexpr (!TR_) tap(a, b, 0, bXS, L, D, DS);

    for (int i = 0; i < ly.n_blocks; ++i) {
      const BlkOff o = blk_off(ly.blk0 + i * ly.blk_stride, D);
      const int tb = 1 + 8 * i;
      launder(bXS); launder(bQN); launder(bQ); launder(bK); launder(bV);
      // Inference for ranking (last_only): only the last position's state leaves the kernel, so the LAST block computes
      // its queries, attention rows, output projection and FFN for the one 16-row tile that holds position L - 1 (keys
      // and values still for every position).  Row for row the arithmetic is that of the full block: same results.
      const bool lo = !TR_ && a.last_only != 0 && i == ly.n_blocks - 1;
      const int mt0 = lo ? (L - 1) >> 4 : 0, r0 = mt0 << 4, mtn = lo ? 1 : MT;
      // training checkpoints of this block beyond its input and post-attention residual (srfrd_aux_floats)
      const AuxOff ax = aux_off(i, b, ly.n_blocks, L, LP, D, D_ == 0 ? ly.n_heads : 1);
      float* sv_r = do_save ? a.save_aux + ax.r : nullptr;
      float* sv_o = do_save ? a.save_aux + ax.o : nullptr;
      float* sv_p = do_save ? a.save_aux + ax.p : nullptr;
      float* sv_q = do_save ? a.save_aux + ax.q : nullptr;
      float* sv_k = do_save ? a.save_aux + ax.k : nullptr;
      float* sv_v = do_save ? a.save_aux + ax.v : nullptr;
      // weight fragments are requested one phase ahead of the GEMM that consumes them
      const WFrag wq = load_wfrag(pk(i * 6 + 0, 0), P + o.in_b, D, NT);
      const WFrag wk = load_wfrag(pk(i * 6 + 1, 0), P + o.in_b + D, D, NT);
      const WFrag wv = load_wfrag(pk(i * 6 + 2, 0), P + o.in_b + 2 * D, D, NT);
      ln_rows(nw, bXS, bQN, L, DS, D, s_ln + (4 * i + 0) * 64, s_ln + (4 * i + 1) * 64);
      __syncthreads();
      if constexpr (!TR_) tap(a, b, tb + 0, bQN, L, D, DS);
      // q = (LN(x) Wq^T + bq) * sqrt(1/d_h);  k = x Wk^T + bk;  v = x Wv^T + bv
      gemm_packed(nw, mtn, NT, DK, Mat{bQN + r0 * DS, DS}, wq, [&](int r_, int c, float v) {
        const int r = r_ + r0;
        if (c < D) {
          bQ[r * DS + c] = v * qscale;
          if (sv_q && r < L) sv_q[r * D + c] = v * qscale;
        }
      });
      gemm_packed(nw, MT, NT, DK, Mat{bXS, DS}, wk, [&](int r, int c, float v) {
        if (c < D) {
          bK[r * DS + c] = v;
          if (sv_k && r < L) sv_k[r * D + c] = v;
        }
      });
      gemm_packed(nw, MT, NT, DK, Mat{bXS, DS}, wv, [&](int r, int c, float v) {
        if (c < D) {
          bV[r * DS + c] = v;
          if (sv_v && r < L) sv_v[r * D + c] = v;
        }
      });
      const WFrag wo = load_wfrag(pk(i * 6 + 3, 0), P + o.out_b, D, NT);
      const WFrag w1 = load_wfrag(pk(i * 6 + 4, 0), P + o.c1_b, D, NT);
      __syncthreads();
      if constexpr (!TR_) tap(a, b, tb + 1, bQ, L, D, DS);
      if constexpr (!TR_) tap(a, b, tb + 2, bK, L, D, DS);
      if constexpr (!TR_) tap(a, b, tb + 3, bV, L, D, DS);
      // H > 1 (generic instantiation only): the heads take turns in the S buffer.  Head h owns columns [c0, c1) of q / k / v:
      // S_h = q_h k_h^T with the other heads' columns of q read as zero, its own dropout mask and probability checkpoint,
      // and o_h = P_h v lands in the head's columns of the q buffer (q_h is dead by then, the other heads' q untouched).
      const int H = D_ == 0 ? ly.n_heads : 1;
      if (H > 1) {
        const int dh = D / H;
        for (int h = 0; h < H; ++h) {
          const int c0 = h * dh, c1 = c0 + dh;
          if (lo) gemm_tiles<0>(nw, 1, mt0 + 1, DK, MatCols{bQ + r0 * DS, DS, c0, c1}, MatT{bK, DS}, [&](int r, int c, float v) { bXS[(r + r0) * SLD + c] = v; });
          else gemm_tiles<1>(nw, MT, MT, DK, MatCols{bQ, DS, c0, c1}, MatT{bK, DS}, [&](int r, int c, float v) { bXS[r * SLD + c] = v; });
          __syncthreads();
          {
            const DropSite dsA = drop_site(drop_on, seed, site_attn(i, h), seq, a.drop_thr, a.drop_scale);
            if (ly.flags & SRFRD_LAYOUT_MASK_PAD_KEYS) mask_pad_keys(nw, bXS, L, SLD, r0, first_live(s_keep, L));
            softmax_rows<true>(nw, bXS, L, SLD, LP, dsA, nullptr, sv_p ? sv_p + (int64_t)h * L * LP : nullptr, r0);
          }
          __syncthreads();
          if (lo) gemm_tiles<0>(nw, 1, NT, (L + 3) & ~3, Mat{bXS + r0 * SLD, SLD}, Mat{bV, DS}, [&](int r, int c, float v) {
            if (c >= c0 && c < c1) bQ[(r + r0) * DS + c] = v;
          });
          else gemm_tiles<2>(nw, MT, NT, (L + 3) & ~3, Mat{bXS, SLD}, Mat{bV, DS}, [&](int r, int c, float v) {
            if (c >= c0 && c < c1) {
              bQ[r * DS + c] = v;
              if (sv_o && r < L) sv_o[r * D + c] = v;
            }
          });
          __syncthreads();
        }
      } else {
      // S = q k^T on the lower-triangular tiles (x is dead: S overlays it)
      if (lo) gemm_tiles<0>(nw, 1, mt0 + 1, DK, Mat{bQ + r0 * DS, DS}, MatT{bK, DS}, [&](int r, int c, float v) { bXS[(r + r0) * SLD + c] = v; });
      else gemm_tiles<1>(nw, MT, MT, DK, Mat{bQ, DS}, MatT{bK, DS}, [&](int r, int c, float v) { bXS[r * SLD + c] = v; });
      __syncthreads();
      // causal softmax (+ attention dropout); keys j > r get exact zeros up to LP
      {
        const DropSite dsA = drop_site(drop_on, seed, site_attn(i), seq, a.drop_thr, a.drop_scale);
        // key-padding mask (srfrd_layout::flags): the leading pads, counted from the pad mask the id load left in LDS, leave
        // the keys of the live rows.  Without the flag nothing runs here and the softmax is the one it was.
        if (ly.flags & SRFRD_LAYOUT_MASK_PAD_KEYS) mask_pad_keys(nw, bXS, L, SLD, r0, first_live(s_keep, L));
        softmax_rows<true>(nw, bXS, L, SLD, LP, dsA, nullptr, sv_p, r0);
      }
      __syncthreads();
      if constexpr (!TR_) tap(a, b, tb + 4, bXS, L, L, SLD);
      // o = P v  (q is dead: o overlays it)
      if (lo) gemm_tiles<0>(nw, 1, NT, (L + 3) & ~3, Mat{bXS + r0 * SLD, SLD}, Mat{bV, DS}, [&](int r, int c, float v) {
        if (c < D) bQ[(r + r0) * DS + c] = v;
      });
      else gemm_tiles<2>(nw, MT, NT, (L + 3) & ~3, Mat{bXS, SLD}, Mat{bV, DS}, [&](int r, int c, float v) {     // (P is zero for keys >= L)
        if (c < D) {
          bQ[r * DS + c] = v;
          if (sv_o && r < L) sv_o[r * D + c] = v;
        }
      });
      __syncthreads();
      }
      // h1 = LN(x) + (o Wo^T + bo)
      gemm_packed(nw, mtn, NT, DK, Mat{bQ + r0 * DS, DS}, wo, [&](int r_, int c, float v) {
        const int r = r_ + r0;
        if (c < D) {
          const float h = bQN[r * DS + c] + v;
          bXS[r * DS + c] = h;
          if (do_save && r < L) a.save_h1[h1_off(i, b, ly.n_blocks, L, D) + r * D + c] = h;
        }
      });
      __syncthreads();
      if constexpr (!TR_) tap(a, b, tb + 5, bXS, L, D, DS);
      ln_rows(nw, bXS + r0 * DS, bQN + r0 * DS, L - r0, DS, D, s_ln + (4 * i + 2) * 64, s_ln + (4 * i + 3) * 64);
      __syncthreads();
      if constexpr (!TR_) tap(a, b, tb + 6, bQN, L, D, DS);
      // PW-FFN: y = (drop2(relu(drop1(h2 W1^T + b1)) W2^T + b2) + h2) * keep
      const DropSite ds1 = drop_site(drop_on, seed, site_ffn1(i), seq, a.drop_thr, a.drop_scale);
      const DropSite ds2 = drop_site(drop_on, seed, site_ffn2(i), seq, a.drop_thr, a.drop_scale);
      const WFrag w2 = load_wfrag(pk(i * 6 + 5, 0), P + o.c2_b, D, NT);
      gemm_packed(nw, mtn, NT, DK, Mat{bQN + r0 * DS, DS}, w1, [&](int r_, int c, float v) {
        const int r = r_ + r0;
        if (c < D) {
          const float h = fmaxf(v * drop_mul(ds1, r, c), 0.f);
          bQ[r * DS + c] = h;
          if (sv_r && r < L) sv_r[r * D + c] = h;
        }
      });
      __syncthreads();
      gemm_packed(nw, mtn, NT, DK, Mat{bQ + r0 * DS, DS}, w2, [&](int r_, int c, float v) {
        const int r = r_ + r0;
        if (c < D) {
          const float y = (v * drop_mul(ds2, r, c) + bQN[r * DS + c]) * s_keep[r];
          bXS[r * DS + c] = y;
          if (do_save && r < L) a.save_x[x_off(i + 1, b, ly.n_blocks, L, D) + r * D + c] = y;
        }
      });
      __syncthreads();
      if constexpr (!TR_) tap(a, b, tb + 7, bXS, L, D, DS);
    }

    // ---- head: (last_conv) -> last LayerNorm -> hidden, pos/neg logits, BCE partial sums
    const lds_f* hin = bXS;
    const bool lo_h = !TR_ && a.last_only != 0;
    const int r0h = lo_h ? ((L - 1) >> 4) << 4 : 0;
    if (kind == SRFRD_SRFR) {
      const WFrag wl = load_wfrag(pk(ly.n_blocks * 6, 0), P + ly.off_lc_b, di, (di + 15) >> 4);
      gemm_packed(nw, lo_h ? 1 : MT, (di + 15) >> 4, DK, Mat{bXS + r0h * DS, DS}, wl,
                  [&](int r, int c, float v) { if (c < di) bQ[(r + r0h) * DS + c] = v; });
      __syncthreads();
      hin = bQ;
    }
    ln_rows(nw, hin + r0h * DS, bQN + r0h * DS, L - r0h, DS, dout, s_ln + (4 * ly.n_blocks) * 64, s_ln + (4 * ly.n_blocks + 1) * 64);
    __syncthreads();
    if (lo_h) {
      for (int c = tid; c < dout; c += nthr) a.hidden[(int64_t)b * dout + c] = bQN[(L - 1) * DS + c];
    } else {
      // pass 1 (linear in (position, channel), coalesced row gathers): hidden out, h * E[pos] -> bK, h * E[neg] -> bV
      const bool srfrn = kind == SRFRD_SRFRN;
      {
        int t = tid / dout, c = tid - t * dout;
        const int dt = nthr / dout, dc = nthr - dt * dout;
        for (; t < L;) {
          const float h = bQN[t * DS + c];
          a.hidden[(rowbase + t) * dout + c] = h;
          if (has_pos)
            bK[t * DS + c] = h * (c < di ? table((int64_t)s_pid[t] * di + c)
                                         : (srfrn ? P[ly.off_side + clamp_id(a.pos_fk[rowbase + t], 2) * dfk + (c - di)] : 0.f));
          if (has_neg)
            bV[t * DS + c] = h * (c < di ? table((int64_t)s_nid[t] * di + c)
                                         : (srfrn ? P[ly.off_side + clamp_id(a.neg_fk[rowbase + t], 2) * dfk + (c - di)] : 0.f));
          t += dt; c += dc;
          if (c >= dout) { c -= dout; ++t; }
        }
      }
      __syncthreads();
      // pass 2 (one DPP quad per position): row sums -> logits, BCE partial sums
      float sp = 0.f, sn = 0.f, cnt = 0.f;
      const int q = tid & (kRL - 1);
      for (int t = tid / kRL; t < L; t += nthr / kRL) {
        float ap = 0.f, an = 0.f;
#pragma unroll
        for (int j = 0; j < kQC; ++j) {
          const int c = q + kRL * j;
          if (c < dout) {
            if (has_pos) ap += bK[t * DS + c];
            if (has_neg) an += bV[t * DS + c];
          }
        }
        const float pl = row_sum(ap), nl = row_sum(an);
        if (q == 0) {
          if (has_pos) a.pos_logits[rowbase + t] = pl;
          if (has_neg) a.neg_logits[rowbase + t] = nl;
          if (do_loss && s_pid[t] != 0) {     // trainer.py:36-38: both terms indexed by pos != 0
            sp += softplus_f(-pl);
            sn += softplus_f(nl);
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
    }
    __syncthreads();
  }
}

}  // namespace SRFRD_NS
