// Fused encoder backward for sequences whose first-generation working set (8 + 2 LDS matrices of LP rows: 295 KB at
// seq_len 100) does not fit a CU: the same arithmetic in SIX uniform LDS slots of R = round4(L) rows ([100][54] floats =
// 21.6 KB each, 130 KB + tail at L = 100), so BASELINE configs[3] (seq_len 100) runs LDS-resident instead of through the
// global-scratch build.
//
//  * every matrix is placed by liveness; checkpoints (block input, LayerNorm input, FFN activation, q, k, v, attention
//    output, sign-coded probabilities) are requested a phase or two ahead (G2L registers) and land in a slot when their
//    consumer runs;
//  * the attention backward walks the queries in CHUNKS of 48 rows (the last one up to 52): the score-shaped matrices
//    P_c, dS_c [chunk][R + 2] fit ONE slot, and they share it - the softmax backward
//          dS_ij = P_ij (dP_ij - delta_i),   delta_i = sum_j dP_ij P_ij = do_i . o_i
//    takes delta from the attention-output checkpoint (with dropout: dP = mask / (1 - p) * dPd and o = (mask / (1 - p) * P) v,
//    so the identity holds term by term), which turns the row pass into the epilogue of the dPd = do v^T tiles: they wait
//    in accumulator registers across one barrier and overwrite P_c element by element;
//  * dv = sum_c drop(P_c)^T do_c and dk = sum_c dS_c^T q_c accumulate in registers across the chunks (a wave owns a
//    16-column strip and every second key tile), dq_c = dS_c k overwrites the rows of do it came from.
//
// Rows R.. of an MFMA A operand read past the slot into the next slot (or the tail): whatever they hold only reaches
// output rows >= R, which no epilogue stores.  Rows L..R-1 of every matrix that serves as a k-operand over tokens are
// exact zeros (checkpoint stores zero them, GEMM outputs inherit them from zero A rows - no bias in the backward).
//
// Scope: hidden 50, 8 waves, one workgroup per CU; fused BCE or upstream logit / hidden gradients (the autograd path); no
// debug taps (those run srfrd_encoder_bwd_long.hip).
namespace SRFRD_NS {

// (kSlotWaves, slots_R, slots_lds_floats: srfrd_enc_common.h, where the kernel plan reads them)
constexpr int kChunkRows = 48;         // query rows of an attention-backward chunk (three 16-row tiles)

__host__ __device__ constexpr int slots_chunks(int L) { return slots_R(L) <= kChunkRows + 4 ? 1 : (slots_R(L) - 4 + kChunkRows - 1) / kChunkRows; }

template <int D_, int L_, int K_, int DI_, bool RMW_>
__global__ void __launch_bounds__(kSlotWaves * 64, (L_ <= 52 ? 4 : 2)) encoder_bwd_slots_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  constexpr int nw = kSlotWaves, nthr = nw * 64;
  constexpr int L = L_, D = D_, LP = (L_ + 15) & ~15;
  constexpr int DK = (D + 3) & ~3, DS = DK + 2, NT = (D + 15) >> 4, MT = LP >> 4;
  constexpr int R = slots_R(L_);               // rows of a slot = token k-range of the gradient GEMMs
  constexpr int SZ = R * DS;
  constexpr int SLD = R + 2;                   // row stride of a score chunk (even, (SLD / 2) odd: the [row][k] view is conflict-free)
  constexpr int NCH = slots_chunks(L_);
  constexpr int CRL = R - kChunkRows * (NCH - 1);          // rows of the last chunk
  constexpr int CRMAX = NCH > 1 ? (CRL > kChunkRows ? CRL : kChunkRows) : CRL;
  static_assert(CRMAX * SLD <= SZ && CRMAX <= 64, "a score chunk must fit a [R][DS] slot");
  static_assert(MT <= 8 && NT == 4, "tile ownership below: 8 waves = 4 column strips x 2 row-tile parities");
  int tid = threadIdx.x;                    // (re-laundered per sequence and block: see the sequence loop)
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  // global -> LDS block copies: one G2L (one memory round trip) covers a whole [L][D] block
  constexpr bool CV2 = (D_ & 1) == 0;
  constexpr int CIT = (R * (CV2 ? D_ / 2 : D_) + nthr - 1) / nthr;
  constexpr int PIT = (CRMAX * (R / 2) + nthr - 1) / nthr;          // a [chunk][R] window of the probability block, in pairs
  lds_f* base = (lds_f*)smem;
  {
    const int total = (int)slots_lds_floats(L, D, ly.n_blocks);
    for (int i = tid; i < total; i += nthr) base[i] = 0.f;
  }
  lds_f* slot[6];
#pragma unroll
  for (int s = 0; s < 6; ++s) slot[s] = base + s * SZ;
  lds_f* tail = base + 6 * SZ;
  lds_i* s_in = (lds_i*)(tail + kRowIn * LP);
  lds_f* s_keep = tail + kRowKeep * LP;
  lds_i* s_pid = (lds_i*)(tail + kRowPid * LP);
  lds_i* s_nid = (lds_i*)(tail + kRowNid * LP);
  lds_i* s_fk = (lds_i*)(tail + kRowFk * LP);
  lds_i* s_pfk = (lds_i*)(tail + kRowPfk * LP);
  lds_i* s_nfk = (lds_i*)(tail + kRowNfk * LP);
  lds_f* s_dpl = tail + kRowDpl * LP;
  lds_f* s_dnl = tail + kRowDnl * LP;
  lds_f* s_delta = tail + kHeadRows * LP;        // do_i . o_i of the block being walked
  lds_f* s_misc = tail + (kHeadRows + 2) * LP;        // 64
  lds_f* s_ln = s_misc + 64;             // LayerNorm parameter cache
  lds_f* s_lng = s_ln + ln_cache_floats(ly.n_blocks);   // LayerNorm parameter-gradient accumulators (same indexing)
  __syncthreads();
  fill_ln_cache(s_ln, a.dense, ly);
  const float* P = a.dense;
  const bool drop_on = a.drop_on != 0;
  const int rkind = K_ >= 0 ? K_ : ly.kind;
  const bool is_sas = rkind == SRFRD_SASREC;
  const bool has_fake = rkind == SRFRD_SRFR || rkind == SRFRD_SRFRN;
  const bool is_srfu = rkind >= SRFRD_SRFU_B;
  constexpr int di = DI_, dfk = D_ - DI_;
  constexpr int dout = (K_ == SRFRD_SRFR) ? DI_ : D_;
  const float sqrtD = sqrtf((float)di);
  const float qscale = a.qscale;
  const uint32_t seed = a.seed_dev ? *a.seed_dev : a.seed;
  const int B = a.B;
  auto pk = [&](int mat, int form) {
    return PackedB{reinterpret_cast<const float4*>(a.packed) + ((int64_t)mat * 2 + form) * (kPackFloats / 4)};
  };
  float* slab = a.grad_slabs + (int64_t)blockIdx.x * ly.n_dense;
  constexpr bool fold_bias = (D & 15) != 0;      // a spare padded column exists in the last n-tile
  static_assert(fold_bias, "this kernel folds the bias gradients into the dW GEMMs (hidden width not a multiple of 16)");
  auto ones_col = [&](lds_f* buf) {
    for (int t = tid; t < L; t += nthr) buf[t * DS + D] = 1.0f;
  };
  auto zero_pad_rows = [&](lds_f* buf) {        // rows L..R-1: the zero padding of the token k-range
    if constexpr (R > L)
      for (int i = tid; i < (R - L) * DS; i += nthr) buf[L * DS + i] = 0.f;
  };
  auto side_sums = [&](int n_out, auto term, auto dst_off) {
    for (int p = wave; p < n_out; p += nw) {
      float sacc = 0.f;
      for (int t = lane; t < L; t += 64) sacc += term(p, t);
      sacc = wave_sum(sacc);
      if (lane == 0) atomicAdd(&slab[dst_off(p)], sacc);
    }
  };
  for (int64_t i = tid; i < (int64_t)ly.blk0; i += nthr) slab[i] = 0.f;      // position / side tables accumulate with +=
  __syncthreads();
  const float keep_scale = drop_on ? a.drop_scale : 1.0f;

  STAMP_INIT
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    // Nothing derived from the thread index may be lifted out of the sequence / block loops: LLVM otherwise keeps a
    // hundred per-thread offsets (G2L element positions, (row, column) walks) live across the whole kernel, runs out of
    // registers at the head of a sequence and serializes its loads behind spill reloads.
    asm volatile("" : "+v"(tid));
#ifdef SRFRD_STAMPS
    asm volatile("s_waitcnt vmcnt(0)");
    __syncthreads();
#endif
    const int64_t rowbase = (int64_t)b * L;
    const uint32_t seq = (uint32_t)(a.seq0 + b);
    const int rmw = RMW_ ? (b != (int)blockIdx.x) : 0;
    lds_f *sX = slot[0], *sQ = slot[1], *sG = slot[2], *sT = slot[3], *sK = slot[4], *sO = slot[5];
    const float* last_x = a.c_save_x + x_off(ly.n_blocks, b, ly.n_blocks, L, D);
    G2L<CIT, CV2> g_last;
    g_last.load(last_x, L, D, nthr);
    G2L<CIT, CV2> g_h1, g_r;
    g_h1.load(a.c_save_h1 + h1_off(ly.n_blocks - 1, b, ly.n_blocks, L, D), L, D, nthr);
    g_r.load(a.c_save_aux + aux_off(ly.n_blocks - 1, b, ly.n_blocks, L, LP, D).r, L, D, nthr);
    for (int t = tid; t < LP; t += nthr) {
      const bool in = t < L;
      const int id = in ? clamp_id(a.in_ids[rowbase + t], ly.n_items) : 0;
      const int pid = (in && a.pos_ids) ? clamp_id(a.pos_ids[rowbase + t], ly.n_items) : 0;
      const int nid = (in && a.neg_ids) ? clamp_id(a.neg_ids[rowbase + t], ly.n_items) : 0;
      s_in[t] = id;
      s_keep[t] = id != 0 ? 1.f : 0.f;
      s_pid[t] = pid;
      s_nid[t] = nid;
      s_fk[t] = (in && a.fk_ids) ? clamp_id(a.fk_ids[rowbase + t], 2) : 0;
      s_pfk[t] = (in && a.pos_fk) ? clamp_id(a.pos_fk[rowbase + t], 2) : 0;
      s_nfk[t] = (in && a.neg_fk) ? clamp_id(a.neg_fk[rowbase + t], 2) : 0;
      float dp = 0.f, dn = 0.f;
      if (in) {
        if (a.fused_bce) {                   // fused masked BCE (trainer.py:36-38): both terms indexed by pos != 0
          const float pl = a.c_pl[rowbase + t], nl = a.c_nl[rowbase + t];
          bce_dlogits(pid, pl, nl, dp, dn);
        } else {                             // upstream logit gradients (the autograd path)
          if (a.d_pos && a.pos_ids) dp = a.d_pos[rowbase + t];
          if (a.d_neg && a.neg_ids) dn = a.d_neg[rowbase + t];
        }
      }
      s_dpl[t] = dp;
      s_dnl[t] = dn;
    }
    if (is_srfu && wave == 0) {
      const int lab = user_label_wave(rkind, a.fk_ids ? a.fk_ids + rowbase : nullptr, L, ly.n_labels);
      if (lane == 0) ((lds_i*)s_misc)[0] = lab;
    }
#ifdef SRFRD_STAMPS
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0)");
    __syncthreads();
#endif
    g_last.store(sX, DS, L, D, nthr);
    zero_pad_rows(sX);
    ones_col(sX);
    zero_pad_rows(sG);
    __syncthreads();

    const lds_f* lnin = sX;
    if (K_ == SRFRD_SRFR) {               // hc = hf Wlc^T + blc -> sQ (input of the last LayerNorm)
      const WFrag wl = load_wfrag(pk(ly.n_blocks * 6, 0), P + ly.off_lc_b, di, (di + 15) >> 4);
      gemm_packed(nw, MT, (di + 15) >> 4, DK, Mat{sX, DS}, wl, [&](int r, int c, float v) { if (c < di && r < L) sQ[r * DS + c] = v; });
      __syncthreads();
      lnin = sQ;
    }
    // ---- logits backward.  Pass 1: dh -> sG and the hidden rows -> sT (linear (position, channel) walk: coalesced row gathers)
    {
      const bool srfrn = K_ == SRFRD_SRFRN;
      constexpr int n = L * dout;
      constexpr int GIT = (LP * D_ + nthr - 1) / nthr;
      constexpr int HALF = (GIT + 1) / 2;
      const float* hid = a.c_hidden + rowbase * dout;
      const float* dhid = a.d_hidden ? a.d_hidden + rowbase * dout : nullptr;      // upstream hidden-state gradient, if any
      // (the index arithmetic of the gathers starts HERE: left free, the scheduler lifts all of it above the barrier into the
      // id pass, runs out of registers there and pays for the spills with serialized reloads between the gathers)
      int tg = tid;
      asm volatile("" : "+v"(tg));
      auto chunks = [&](auto bf16_shadow) {
        constexpr bool H16 = decltype(bf16_shadow)::value;
        for (int base0 = 0; base0 < n; base0 += HALF * nthr) {
          float hv[HALF], pv[HALF], nv[HALF];
#pragma unroll
          for (int u = 0; u < HALF; ++u) {
            const int i = min(base0 + u * nthr + tg, n - 1);
            const int t = i / dout, c = i - t * dout;
            const bool item = c < di;
            const int prow = item ? s_pid[t] : s_pfk[t], nrow = item ? s_nid[t] : s_nfk[t];
            const int w = item ? di : dfk, cc = item ? c : c - di;
            const bool use = item || srfrn;
            hv[u] = hid[i];
            if constexpr (H16) {
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
          for (int u = 0; u < HALF; ++u) {
            const int i = base0 + u * nthr + tg;
            if (i < n) {
              const int t = i / dout, c = i - t * dout;
              float dh = dhid ? dhid[i] : 0.f;
              if (c < di || srfrn) dh += s_dpl[t] * pv[u] + s_dnl[t] * nv[u];
              sT[t * DS + c] = hv[u];
              sG[t * DS + c] = dh;
            }
          }
        }
      };
      if (a.table16 != nullptr) chunks(std::true_type{});
      else chunks(std::false_type{});
      head_zero_cols(sG, DS, L, dout, D, tid, nthr);
    }
    __syncthreads();
    // Pass 2: item-table scatter (float atomics, no return): at most two contiguous row segments per wave-instruction
    {
      int t = tid / di, c = tid - t * di;
      constexpr int dt = nthr / di, dc = nthr - dt * di;
      for (; t < L;) {
        const float h = sT[t * DS + c];
        const float dp = s_dpl[t], dn = s_dnl[t];
        const int pid = s_pid[t], nid = s_nid[t];
        if (a.contrib != nullptr) {          // deterministic mode: see srfrd_encoder_bwd_kernel.inc
          a.contrib[(((int64_t)0 * B + b) * L + t) * di + c] = pid != 0 ? dp * h : 0.f;
          a.contrib[(((int64_t)1 * B + b) * L + t) * di + c] = nid != 0 ? dn * h : 0.f;
        } else {
          if (pid != 0 && dp != 0.f) atomicAdd(&a.grad_table[(int64_t)pid * di + c], dp * h);
          if (nid != 0 && dn != 0.f) atomicAdd(&a.grad_table[(int64_t)nid * di + c], dn * h);
        }
        t += dt; c += dc;
        if (c >= di) { c -= di; ++t; }
      }
    }
    if (K_ == SRFRD_SRFRN)
      side_sums(2 * dfk, [&](int p, int t) {
        constexpr int dq = dfk > 0 ? dfk : 1;
        const int f = 1 + p / dq, c = p - (f - 1) * dq;
        const float w = (s_pfk[t] == f ? s_dpl[t] : 0.f) + (s_nfk[t] == f ? s_dnl[t] : 0.f);
        return w * sT[t * DS + di + c];
      }, [&](int p) { return ly.off_side + dfk + p; });
    // ---- last LayerNorm backward: dx -> sK, g * xhat -> sO; dgamma / dbeta as ones-row GEMMs
    ln_bwd_rows<false>(nw, sG, lnin, sK, sO, L, R, DS, dout, s_ln + (4 * ly.n_blocks) * 64);
    head_zero_cols(sK, DS, L, dout, D, tid, nthr);
    zero_pad_rows(sK);
    __syncthreads();
    gemm_tiles<0>(nw, 1, (dout + 15) >> 4, R, OnesRow{}, Mat{sG, DS},
                  [=](int r, int c, float v) { if (r == 0 && c < dout) s_lng[(4 * ly.n_blocks + 1) * 64 + c] += v; });
    gemm_tiles<0>(nw, 1, (dout + 15) >> 4, R, OnesRow{}, Mat{sO, DS},
                  [=](int r, int c, float v) { if (r == 0 && c < dout) s_lng[(4 * ly.n_blocks + 0) * 64 + c] += v; });
    __syncthreads();
    // running gradient G = sK from here
    lds_f* G = sK;
    lds_f* fr[5] = {sG, sO, sT, sQ, sX};
    if (K_ == SRFRD_SRFR) {               // hc = hf Wlc^T + blc: dWlc += G^T x_nb, G <- G Wlc
      gemm_slab(nw, (di + 15) >> 4, NT, R, MatT{G, DS}, Mat{sX, DS}, SlabWB{slab, ly.off_lc_w, ly.off_lc_b, di, D, rmw});
      const WFrag wln = load_wfrag(pk(ly.n_blocks * 6, 1), nullptr, 0, NT);
      lds_f* Gn = sG;
      gemm_packed(nw, MT, NT, (di + 3) & ~3, Mat{G, DS}, wln, [&](int r, int c, float v) { if (c < D && r < R) Gn[r * DS + c] = v; });
      __syncthreads();
      fr[0] = G;
      G = Gn;
    }

    for (int i = ly.n_blocks - 1; i >= 0; --i) {
      const BlkOff o = blk_off(ly.blk0 + i * ly.blk_stride, D);
      const DropSite ds2 = drop_site(drop_on, seed, site_ffn2(i), seq, a.drop_thr, a.drop_scale);
      const AuxOff ax = aux_off(i, b, ly.n_blocks, L, LP, D);
      asm volatile("" : "+v"(tid));
      // slot assignment of this block (G is live, fr[0..4] are free)
      lds_f *X = fr[0], *Rr = fr[1], *N = fr[2], *A2 = fr[3], *A1 = fr[4];
      launder(G); launder(X); launder(Rr); launder(N); launder(A2); launder(A1);
      // ================= FFN half: y = (drop2(a2) + h2) * keep, a2 = r W2^T + b2, r = relu(drop1(h2 W1^T + b1))
      const WFrag w2n = load_wfrag(pk(i * 6 + 5, 1), nullptr, 0, NT);
      const SlabWB sl_w2{slab, o.c2_w, o.c2_b, D, D, rmw};
      const SlabWB sl_w1{slab, o.c1_w, o.c1_b, D, D, rmw};
      // ---- F1: dy *= keep; checkpoints h1 -> X, r -> Rr
      for (int idx = tid; idx < L * D; idx += nthr) {
        const int t = idx / D, c = idx - t * D;
        G[t * DS + c] *= s_keep[t];
      }
      g_h1.store(X, DS, L, D, nthr);
      g_r.store(Rr, DS, L, D, nthr);
      zero_pad_rows(X); zero_pad_rows(Rr);
      ones_col(Rr);
      __syncthreads();
      // ---- F2: h2 = LN2(h1) -> N; dA2 = drop2'(dy) -> A2
      ln_rows(nw, X, N, L, DS, D, s_ln + (4 * i + 2) * 64, s_ln + (4 * i + 3) * 64);
      zero_pad_rows(N);
      ones_col(N);
      for (int idx = tid; idx < R * D; idx += nthr) {
        const int t = idx / D, c = idx - t * D;
        A2[t * DS + c] = t < L ? G[t * DS + c] * drop_mul(ds2, t, c) : 0.f;
      }
      __syncthreads();
      // ---- F3: dA1 = (dA2 W2) * relu' -> A1 ; dW2 += dA2^T r
      G2L<CIT, CV2> g_o, g_v, g_k;
      {
        SlabPre pre_w2 = RMW_ ? slab_preload(nw, NT, NT, sl_w2) : SlabPre{};
        gemm_packed(nw, MT, NT, DK, Mat{A2, DS}, w2n, [&](int r, int c, float v) {
          if (c < D && r < R) A1[r * DS + c] = Rr[r * DS + c] > 0.f ? v * keep_scale : 0.f;
        });
        gemm_slab(nw, NT, NT, R, MatT{A2, DS}, Mat{Rr, DS}, sl_w2, pre_w2);
      }
      const WFrag w1n = load_wfrag(pk(i * 6 + 4, 1), nullptr, 0, NT);
      g_o.load(a.c_save_aux + ax.o, L, D, nthr);
      __syncthreads();
      // ---- F4: dh2 = dy + dA1 W1 (in place) ; dW1 += dA1^T h2           (A2, Rr are free afterwards)
      {
        SlabPre pre_w1 = RMW_ ? slab_preload(nw, NT, NT, sl_w1) : SlabPre{};
        gemm_packed(nw, MT, NT, DK, Mat{A1, DS}, w1n, [&](int r, int c, float v) { if (c < D && r < R) G[r * DS + c] += v; });
        gemm_slab(nw, NT, NT, R, MatT{A1, DS}, Mat{N, DS}, sl_w1, pre_w1);
      }
      g_v.load(a.c_save_aux + ax.v, L, D, nthr);
      __syncthreads();
      // ---- F5: LN2 backward: dh1 -> H (= A2's slot), g * xhat -> GX (= Rr's slot)            (A1, N free after this)
      lds_f *H = A2, *GX = Rr;
      ln_bwd_rows<false>(nw, G, X, H, GX, L, R, DS, D, s_ln + (4 * i + 2) * 64);
      zero_pad_rows(H);
      g_k.load(a.c_save_aux + ax.k, L, D, nthr);
      __syncthreads();
      // ---- F6: column sums (dbeta2 from G, dgamma2 from GX); o -> O (= N's slot)
      lds_f* O = N;
      gemm_tiles<0>(nw, 1, NT, R, OnesRow{}, Mat{G, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 3) * 64 + c] += v; });
      gemm_tiles<0>(nw, 1, NT, R, OnesRow{}, Mat{GX, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 2) * 64 + c] += v; });
      g_o.store(O, DS, L, D, nthr);
      zero_pad_rows(O);
      ones_col(O);
      const WFrag won = load_wfrag(pk(i * 6 + 3, 1), nullptr, 0, NT);
      G2L<PIT, true> g_p;
      g_p.load2d(a.c_save_aux + ax.p, NCH > 1 ? kChunkRows : L, R, LP, nthr);       // chunk 0 of the sign-coded probabilities
      __syncthreads();
      // ================= attention half: h1 = LN1(x) + o Wo^T + bo, o = drop(P) v       (G, GX, X, A1 are free; dh1 = H)
      lds_f *DO = G, *V = GX, *Kk = X, *S = A1;
      const SlabWB sl_wo{slab, o.out_w, o.out_b, D, D, rmw};
      G2L<CIT, CV2> g_q, g_x;
      // ---- A1: do = dh1 Wo -> DO ; dWo += dh1^T o ; v -> V ; k -> Kk
      {
        SlabPre pre_wo = RMW_ ? slab_preload(nw, NT, NT, sl_wo) : SlabPre{};
        g_v.store(V, DS, L, D, nthr);
        g_k.store(Kk, DS, L, D, nthr);
        zero_pad_rows(V); zero_pad_rows(Kk);
        // (columns D..DK-1 of do are written too - exact zeros, the packed weight has none there: do meets v over k < DK in
        // the dPd tiles, and a slot may hold a previous tenant's ones column)
        gemm_packed(nw, MT, NT, DK, Mat{H, DS}, won, [&](int r, int c, float v) { if (c < DK && r < R) DO[r * DS + c] = v; });
        gemm_slab(nw, NT, NT, R, MatT{H, DS}, Mat{O, DS}, sl_wo, pre_wo);
      }
      g_q.load(a.c_save_aux + ax.q, L, D, nthr);
      __syncthreads();
      // ---- A2: delta_i = do_i . o_i ; P_0 -> S
      {
        const int q = tid & (kRL - 1);
        for (int r = tid / kRL; r < L; r += nthr / kRL) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < kQC; ++j) {
            const int c = q + kRL * j;
            if (c < D) s += DO[r * DS + c] * O[r * DS + c];
          }
          s = row_sum(s);
          if (q == 0) s_delta[r] = s;
        }
        g_p.store(S, SLD, NCH > 1 ? kChunkRows : L, R, nthr);
        if constexpr (NCH == 1 && R > L)
          for (int idx = tid; idx < (R - L) * SLD; idx += nthr) S[L * SLD + idx] = 0.f;
      }
      __syncthreads();
      lds_f* Q = O;                                 // o is dead: q takes its slot
      // dv / dk accumulators: strip nt = wave % 4, key tiles g, g + 2, g + 4, g + 6 (g = wave / 4)
      const int ant = wave & 3, ag = wave >> 2;
      f32x4 dv_acc[4], dk_acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { dv_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dk_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
      WFrag wqn;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int q0 = ch * kChunkRows;                                      // first query row of the chunk
        const int cr = ch == NCH - 1 ? CRL : kChunkRows;                     // its rows (a multiple of 4)
        const int q1 = q0 + cr;
        const int qt0 = q0 >> 4, qtn = (cr + 15) >> 4;                       // query tiles: first (global), count
        const int ktn = (q1 + 15) >> 4;                                      // key tiles that any query of the chunk sees
        // ---- C1: dv += drop(P_c)^T do_c (registers) ; dPd_c = do_c v^T (registers: tiles u = wave, wave + 8, ...)
        f32x4 dp_acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) dp_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int u = wave + j * nw;
          const int m = u / ktn, n = u - m * ktn;
          if (m < qtn && n <= qt0 + m) {
            f32x4 acc1[1] = {dp_acc[j]};
            mma_group<1>(acc1, Mat{DO + q0 * DS, DS}, MatT{V, DS}, (m << 4) + li, 0, (n << 4) + li, 0, DK, lq);
            dp_acc[j] = acc1[0];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kt = ag + 2 * j;
          if (kt < ktn) {
            f32x4 acc1[1] = {dv_acc[j]};
            const int k0 = imax(0, (kt << 4) - q0);
            mma_group<1>(acc1, MatTPos{S, SLD}, Mat{DO + q0 * DS, DS}, (kt << 4) + li, 0, (ant << 4) + li, k0, cr, lq);
            dv_acc[j] = acc1[0];
          }
        }
        if (ch == 0) {
          g_q.store(Q, DS, L, D, nthr);
          zero_pad_rows(Q);
        }
        G2L<PIT, true> g_pn;
        if (ch + 1 < NCH) g_pn.load2d(a.c_save_aux + ax.p + (int64_t)(q0 + kChunkRows) * LP, ch + 2 == NCH ? L - (q0 + kChunkRows) : kChunkRows, R, LP, nthr);
        __syncthreads();
        // ---- C2: dS_c = P_c * (mask / (1 - p) * dPd_c - delta) over P_c, element by element (own tiles)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int u = wave + j * nw;
          const int m = u / ktn, n = u - m * ktn;
          if (m < qtn && n <= qt0 + m) {
            const int col = (n << 4) + li;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = (m << 4) + (lq << 2) + e;
              if (q0 + r < L && col < R) {
                const float pm = S[r * SLD + col];
                const float dp = pm > 0.f ? dp_acc[j][e] * keep_scale : 0.f;
                S[r * SLD + col] = fabsf(pm) * (dp - s_delta[q0 + r]);
              }
            }
          }
        }
        if (ch == NCH - 1) {
          g_x.load(a.c_save_x + x_off(i, b, ly.n_blocks, L, D), L, D, nthr);
          wqn = load_wfrag(pk(i * 6 + 0, 1), nullptr, 0, NT);
        }
        __syncthreads();
        // ---- C3: dq_c = dS_c k * qscale -> rows q0.. of DO (do_c is dead) ; dk += dS_c^T q_c (registers)
        {
          const Mat As{S - q0 * SLD, SLD};                 // addressed by global query row
          for (int mt = qt0 + ag; mt < qt0 + qtn; mt += 2)
            gemm_group<2, 1>(mt, 2, ant << 4, R, As, Mat{Kk, DS},
                             [&](int r, int c, float v) { if (c < D && r < R) DO[r * DS + c] = v * qscale; }, li, lq);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kt = ag + 2 * j;
          if (kt < ktn) {
            f32x4 acc1[1] = {dk_acc[j]};
            const int k0 = imax(0, (kt << 4) - q0);
            mma_group<1>(acc1, MatT{S, SLD}, Mat{Q + q0 * DS, DS}, (kt << 4) + li, 0, (ant << 4) + li, k0, cr, lq);
            dk_acc[j] = acc1[0];
          }
        }
        __syncthreads();
        if (ch + 1 < NCH) {
          // ---- C4: P_{c+1} -> S
          const int nr = ch + 2 == NCH ? L - (q0 + kChunkRows) : kChunkRows;
          g_pn.store(S, SLD, nr, R, nthr);
          if (ch + 2 == NCH && CRL > nr)
            for (int idx = tid; idx < (CRL - nr) * SLD; idx += nthr) S[nr * SLD + idx] = 0.f;
          __syncthreads();
        }
      }
      // ---- A3: dv -> DV (= v's slot), dk -> DKm (= k's slot) ; x -> Xb (= S's slot) ; dLN1 = dh1 + dq Wq (in place in H)
      lds_f *DQ = DO, *DV = V, *DKm = Kk, *Xb = S, *DX = Q;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kt = ag + 2 * j;
        if (kt < MT) {
          const int c = (ant << 4) + li;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = (kt << 4) + (lq << 2) + e;
            if (r < R && c < D) {
              DV[r * DS + c] = dv_acc[j][e] * keep_scale;
              DKm[r * DS + c] = dk_acc[j][e];
            }
          }
        }
      }
      const SlabWB sl_wq{slab, o.in_w, o.in_b, D, D, rmw};
      const SlabWB sl_wk{slab, o.in_w + D * D, o.in_b + D, D, D, rmw};
      const SlabWB sl_wv{slab, o.in_w + 2 * D * D, o.in_b + 2 * D, D, D, rmw};
      g_x.store(Xb, DS, L, D, nthr);
      zero_pad_rows(Xb);
      ones_col(Xb);
      const WFrag wkn = load_wfrag(pk(i * 6 + 1, 1), nullptr, 0, NT);
      gemm_packed(nw, MT, NT, DK, Mat{DQ, DS}, wqn, [&](int r, int c, float v) { if (c < D && r < R) H[r * DS + c] += v; });
      const WFrag wvn = load_wfrag(pk(i * 6 + 2, 1), nullptr, 0, NT);
      __syncthreads();
      // ---- A4: dx = dk Wk + dv Wv -> DX (= q's slot) ; dWk += dk^T x ; dWv += dv^T x
      {
        SlabPre pre_wk = RMW_ ? slab_preload(nw, NT, NT, sl_wk) : SlabPre{};
        SlabPre pre_wv = RMW_ ? slab_preload(nw, NT, NT, sl_wv) : SlabPre{};
        gemm_packed(nw, MT, NT, DK, Mat{DKm, DS}, wkn, [&](int r, int c, float v) { if (c < D && r < R) DX[r * DS + c] = v; });
        gemm_packed(nw, MT, NT, DK, Mat{DV, DS}, wvn, [&](int r, int c, float v) { if (c < D && r < R) DX[r * DS + c] += v; });
        if (RMW_) { slab_ready(pre_wk); slab_ready(pre_wv); }
        gemm_slab(nw, NT, NT, R, MatT{DKm, DS}, Mat{Xb, DS}, sl_wk, pre_wk);
        gemm_slab(nw, NT, NT, R, MatT{DV, DS}, Mat{Xb, DS}, sl_wv, pre_wv);
      }
      if (i > 0) {                               // the next block's FFN checkpoints
        g_h1.load(a.c_save_h1 + h1_off(i - 1, b, ly.n_blocks, L, D), L, D, nthr);
        g_r.load(a.c_save_aux + aux_off(i - 1, b, ly.n_blocks, L, LP, D).r, L, D, nthr);
      }
      __syncthreads();
      // ---- A5: LN1(x) -> N1 (= dk's slot)                                              (DKm, DV free)
      lds_f* N1 = DKm;
      ln_rows(nw, Xb, N1, L, DS, D, s_ln + (4 * i + 0) * 64, s_ln + (4 * i + 1) * 64);
      zero_pad_rows(N1);
      ones_col(N1);
      __syncthreads();
      // ---- A6: dWq += dq^T LN1(x) ; LN1 backward: DX += dx(dLN1), g * xhat -> GX1 (= dv's slot)
      lds_f* GX1 = DV;
      {
        SlabPre pre_wq = RMW_ ? slab_preload(nw, NT, NT, sl_wq) : SlabPre{};
        ln_bwd_rows<true>(nw, H, Xb, DX, GX1, L, R, DS, D, s_ln + (4 * i + 0) * 64);
        gemm_slab(nw, NT, NT, R, MatT{DQ, DS}, Mat{N1, DS}, sl_wq, pre_wq);
      }
      __syncthreads();
      // ---- A7: column sums (dbeta1 from dLN1 = H, dgamma1 from GX1)
      gemm_tiles<0>(nw, 1, NT, R, OnesRow{}, Mat{H, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 1) * 64 + c] += v; });
      gemm_tiles<0>(nw, 1, NT, R, OnesRow{}, Mat{GX1, DS}, [=](int r, int c, float v) { if (r == 0 && c < D) s_lng[(4 * i + 0) * 64 + c] += v; });
      __syncthreads();
      // next block: G = DX; everything else is free
      G = DX;
      fr[0] = H; fr[1] = GX1; fr[2] = Xb; fr[3] = N1; fr[4] = DQ;
    }

    // ---- embedding backward: item rows (atomics), position table, side channel
    {
      const DropSite dsE = drop_site(drop_on && is_sas, seed, SITE_EMB, seq, a.drop_thr, a.drop_scale);
      {
        int t = tid / di, c = tid - t * di;
        constexpr int dt = nthr / di, dc = nthr - dt * di;
        for (; t < L;) {
          float gv = G[t * DS + c] * s_keep[t];
          if (is_sas) gv *= drop_mul(dsE, t, c);
          const int id = s_in[t];
          if (a.contrib != nullptr) a.contrib[(((int64_t)2 * B + b) * L + t) * di + c] = id != 0 ? (is_sas ? gv * sqrtD : gv) : 0.f;
          else if (id != 0) atomicAdd(&a.grad_table[(int64_t)id * di + c], is_sas ? gv * sqrtD : gv);
          atomicAdd(&slab[ly.off_pos + t * di + c], gv);
          t += dt; c += dc;
          if (c >= di) { c -= di; ++t; }
        }
      }
      if (has_fake)
        side_sums(2 * dfk, [&](int p, int t) {
          constexpr int dq = dfk > 0 ? dfk : 1;
          const int f = 1 + p / dq, c = p - (f - 1) * dq;
          return s_fk[t] == f ? G[t * DS + di + c] * s_keep[t] : 0.f;
        }, [&](int p) { return ly.off_side + dfk + p; });
      if (is_srfu) {
        const int lab = ((lds_i*)s_misc)[0];
        side_sums(D, [&](int c, int t) { return G[t * DS + c] * s_keep[t]; }, [&](int c) { return ly.off_side + lab * D + c; });
      }
    }
    __syncthreads();
  }
  // LayerNorm parameter gradients: LDS accumulators -> slab
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
