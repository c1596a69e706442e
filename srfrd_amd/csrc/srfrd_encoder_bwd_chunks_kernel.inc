// Fused encoder backward for seq_len 101..208 (BASELINE configs[4] trains at seq_len 200): the arithmetic of the slot-placed
// backward (srfrd_encoder_bwd_slots_kernel.inc) walked in ROW CHUNKS of 48 tokens, so that it stays LDS-resident where six
// whole-sequence slots (6 x 43 KB at seq_len 200) cannot.
//
// Every per-token operation of a block's backward - the FFN half, the output projection, the q / k / v projections, all
// LayerNorm passes - needs only its own rows; the weight gradients need a sum over rows; only the attention needs other
// rows (K and V of the whole sequence).  A block therefore runs as three passes over the chunks:
//   pass 1 (FFN half)       per chunk: dy -> dA2 -> dA1 -> dh2 -> LN2 backward -> dh1 (to scratch); dW2, dW1 accumulate
//   pass 2 (attention)      K, V of the sequence resident (2 x [L][54]); per 48-query chunk: do = dh1 Wo, delta = do . o,
//                           dPd = do v^T, dS folded into its epilogue over P_c, dq_c = dS_c k (to scratch); dv, dk and dWo
//                           accumulate in registers; at the end dv / dk take the places of v / k
//   pass 3 (projections)    per chunk: dLN1 = dh1 + dq Wq, dx = dk Wk + dv Wv + LN1 backward -> the next block's dy (to
//                           scratch); dWq, dWk, dWv accumulate
// The three full-length intermediates that cross passes (dy, dh1, dq: [L][50] each) live in the workgroup's slice of the
// caller's scratch (L2-resident, 120 KB); the weight-gradient tiles of a pass stay in accumulator registers across its
// chunks (initialised with the slab's old values, stored once).  LDS: K / V 86 KB + one [48][L + 2] score chunk 39 KB + two
// chunk slots, the per-token passes place their six chunk slots over the (then idle) K / V region: 157 KB.
//
// Scope: hidden 50, 8 waves, one workgroup per CU; fused BCE or upstream logit / hidden gradients (the autograd path); no
// debug taps.
namespace SRFRD_NS {

// (kCkWaves, kCkRows, chunks_lds_floats, chunks_scratch_floats: srfrd_enc_common.h, where the kernel plan reads them)

// the two row tiles of a (4 x 4 tile) weight gradient a wave owns (wave_tiles(8, 4, 4): strip wave % 4, tiles g, g + 2)
struct DwAcc {
  f32x4 t[2];
};
__device__ __forceinline__ DwAcc dw_init(const SlabWB& sl) {
  const SlabPre p = slab_preload(kCkWaves, 4, 4, sl);
  DwAcc a;
#pragma unroll
  for (int j = 0; j < 2; ++j) a.t[j] = f32x4{p.v[j][0], p.v[j][1], p.v[j][2], p.v[j][3]};
  return a;
}
// acc += A^T-view (m = feature of dY, k = token) x B (k = token, n = feature of X | 1), k < k_end
template <class AL, class BL>
__device__ __forceinline__ void dw_add(DwAcc& acc, const AL& a, const BL& b, int k_end) {
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
  const WaveTiles t = wave_tiles(kCkWaves, 4, 4);
  mma_group<2>(acc.t, a, b, (t.g << 4) + li, t.mgroups << 4, (t.nt << 4) + li, 0, k_end, lq);
}
__device__ __forceinline__ void dw_store(const SlabWB& sl, const DwAcc& acc) {
  const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
  const WaveTiles t = wave_tiles(kCkWaves, 4, 4);
  const SlabCol sc = slab_col(sl, (t.nt << 4) + li);
  if (sc.ok) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = ((t.g + j * t.mgroups) << 4) + (lq << 2) + e;
        if (r < sl.R) sl.base[(unsigned)(sc.col0 + r * sc.rs)] = acc.t[j][e];
      }
  }
}

template <int D_, int K_, int DI_, bool RMW_>
__global__ void __launch_bounds__(kCkWaves * 64) encoder_bwd_chunks_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  constexpr int nw = kCkWaves, nthr = nw * 64;
  constexpr int D = D_, DK = (D + 3) & ~3, DS = DK + 2, NT = (D + 15) >> 4;
  constexpr int CR = kCkRows, CT = CR >> 4, CSZ = CR * DS;
  const int L = a.L, LP = (L + 15) & ~15, LR = (L + 3) & ~3, SLD = LR + 2;
  const int NCH = (L + CR - 1) / CR;
  // The thread / lane index is re-laundered per sequence, pass and chunk (CK_RELANE): left alone, LLVM computes every
  // per-lane address of the kernel once, keeps hundreds live, spills them, and reloads each in front of its use (the 56
  // LDS addresses of the dv / dk write-out cost 22 us per block that way).
  int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int lane = tid & 63, li = lane & 15, lq = lane >> 4;
#define CK_RELANE() do { asm volatile("" : "+v"(tid)); lane = tid & 63; li = lane & 15; lq = lane >> 4; } while (0)
  constexpr bool CV2 = (D_ & 1) == 0;
  constexpr int CIT = (CR * (CV2 ? D_ / 2 : D_) + nthr - 1) / nthr;         // a [48][D] chunk block
  constexpr int BIT = (208 * (CV2 ? D_ / 2 : D_) + nthr - 1) / nthr;        // a whole [L][D] block (K, V), L <= 208
  constexpr int PIT = (CR * (208 / 2) + nthr - 1) / nthr;                   // a [48][L] window of the probabilities, in pairs
  lds_f* base = (lds_f*)smem;
  {
    const int total = (int)chunks_lds_floats(L, D, ly.n_blocks);
    for (int i = tid; i < total; i += nthr) base[i] = 0.f;
  }
  lds_f* regA = base;                          // K | V ([LR][DS] each); the FFN pass and the head lay six chunk slots from here
  lds_f* regB = regA + 2 * LR * DS;            // pool: score chunk [CR][SLD] + two chunk slots (regC), or five chunk slots
  lds_f* regC = regB + CR * SLD;
  const int pool = imax(CR * SLD + 2 * CSZ, 5 * CSZ);
  lds_f* tail = regB + pool;
  lds_i* s_in = (lds_i*)(tail + kRowIn * LP);
  lds_f* s_keep = tail + kRowKeep * LP;
  lds_i* s_pid = (lds_i*)(tail + kRowPid * LP);
  lds_i* s_nid = (lds_i*)(tail + kRowNid * LP);
  lds_i* s_fk = (lds_i*)(tail + kRowFk * LP);
  lds_i* s_pfk = (lds_i*)(tail + kRowPfk * LP);
  lds_i* s_nfk = (lds_i*)(tail + kRowNfk * LP);
  lds_f* s_dpl = tail + kRowDpl * LP;
  lds_f* s_dnl = tail + kRowDnl * LP;
  lds_f* s_delta = tail + kHeadRows * LP;
  lds_f* s_misc = tail + (kHeadRows + 2) * LP;        // 64
  lds_f* s_ln = s_misc + 64;
  lds_f* s_lng = s_ln + ln_cache_floats(ly.n_blocks);
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
  constexpr bool fold_bias = (D & 15) != 0;
  static_assert(fold_bias, "this kernel folds the bias gradients into the dW GEMMs (hidden width not a multiple of 16)");
  // scratch of this workgroup: dy, dh1, dq of the sequence ([LR][D] each, row-major)
  float* gbuf = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
  float* hbuf = gbuf + LR * D + 64;
  float* qbuf = hbuf + LR * D + 64;
  // rows of chunk c: [c * CR, min(L, (c + 1) * CR)); k-range of its token sums = rows rounded up to 4 (pad rows are zero)
  auto rows_of = [&](int c) { return min(L - c * CR, CR); };
  auto ones_col = [&](lds_f* buf, int rows) {
    for (int t = tid; t < rows; t += nthr) buf[t * DS + D] = 1.0f;
  };
  // a chunk slot holds [CR][DS]; rows >= `rows` up to CR are zeroed so that they are exact zeros in every token sum
  auto zero_tail_rows = [&](lds_f* buf, int rows) {
    for (int i = tid; i < (CR - rows) * DS; i += nthr) buf[rows * DS + i] = 0.f;
  };
  // chunk rows: scratch / checkpoint ([rows][D] contiguous) -> slot, slot -> scratch
  auto load_chunk = [&](lds_f* dst, const float* src, int rows) {
    copy_g2l<CIT, CV2>(dst, DS, src, rows, D, nthr);
    zero_tail_rows(dst, rows);
  };
  // the same copy split in two: request a chunk's rows early (registers), land them in the slot when it is free
  auto put_chunk = [&](const G2L<CIT, CV2>& g, lds_f* dst, int rows) {
    g.store(dst, DS, rows, D, nthr);
    zero_tail_rows(dst, rows);
  };
  auto store_chunk = [&](float* dst, const lds_f* src, int rows) {
    for (int idx = tid; idx < rows * D; idx += nthr) {
      const int t = idx / D, c = idx - t * D;
      dst[idx] = src[t * DS + c];
    }
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
    CK_RELANE();
    const int64_t rowbase = (int64_t)b * L;
    const uint32_t seq = (uint32_t)(a.seq0 + b);
    const int rmw = RMW_ ? (b != (int)blockIdx.x) : 0;
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
    __syncthreads();

    // ================= head, chunk by chunk: logits backward, item scatter, last LayerNorm backward -> dy (gbuf)
    {
      DwAcc wlc;
      const SlabWB sl_lc{slab, ly.off_lc_w, ly.off_lc_b, di, D, rmw};
      if (K_ == SRFRD_SRFR) wlc = dw_init(sl_lc);
      for (int c = 0; c < NCH; ++c) {
        CK_RELANE();
        const int r0 = c * CR, rows = rows_of(c), kr = (rows + 3) & ~3, ct = (rows + 15) >> 4;
        lds_f *sX = regA, *sQ = regA + CSZ, *sG = regA + 2 * CSZ, *sT = regA + 3 * CSZ, *sK = regA + 4 * CSZ, *sO = regA + 5 * CSZ;
        load_chunk(sX, a.c_save_x + x_off(ly.n_blocks, b, ly.n_blocks, L, D) + (int64_t)r0 * D, rows);
        ones_col(sX, rows);
        __syncthreads();
        const lds_f* lnin = sX;
        if (K_ == SRFRD_SRFR) {             // hc = hf Wlc^T + blc -> sQ (input of the last LayerNorm)
          const WFrag wl = load_wfrag(pk(ly.n_blocks * 6, 0), P + ly.off_lc_b, di, (di + 15) >> 4);
          gemm_packed(nw, ct, (di + 15) >> 4, DK, Mat{sX, DS}, wl, [&](int r, int cc, float v) { if (cc < di && r < rows) sQ[r * DS + cc] = v; });
          __syncthreads();
          lnin = sQ;
        }
        // pass 1: dh -> sG, hidden rows -> sT (linear (position, channel) walk: coalesced row gathers)
        {
          const bool srfrn = K_ == SRFRD_SRFRN;
          const int n = rows * dout;
          constexpr int GIT = (CR * D_ + nthr - 1) / nthr;
          const float* hid = a.c_hidden + (rowbase + r0) * dout;
          const float* dhid = a.d_hidden ? a.d_hidden + (rowbase + r0) * dout : nullptr;   // upstream hidden-state gradient, if any
          int tg = tid;
          asm volatile("" : "+v"(tg));
          auto chunks = [&](auto bf16_shadow) {
            constexpr bool H16 = decltype(bf16_shadow)::value;
            float hv[GIT], pv[GIT], nv[GIT];
#pragma unroll
            for (int u = 0; u < GIT; ++u) {
              const int i = min(u * nthr + tg, n - 1);
              const int t = i / dout, cc0 = i - t * dout;
              const bool item = cc0 < di;
              const int prow = item ? s_pid[r0 + t] : s_pfk[r0 + t], nrow = item ? s_nid[r0 + t] : s_nfk[r0 + t];
              const int w = item ? di : dfk, cc = item ? cc0 : cc0 - di;
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
            for (int u = 0; u < GIT; ++u) {
              const int i = u * nthr + tg;
              if (i < n) {
                const int t = i / dout, cc0 = i - t * dout;
                float dh = dhid ? dhid[i] : 0.f;
                if (cc0 < di || srfrn) dh += s_dpl[r0 + t] * pv[u] + s_dnl[r0 + t] * nv[u];
                sT[t * DS + cc0] = hv[u];
                sG[t * DS + cc0] = dh;
              }
            }
          };
          if (a.table16 != nullptr) chunks(std::true_type{});
          else chunks(std::false_type{});
          head_zero_cols(sG, DS, rows, dout, D, tid, nthr);
          zero_tail_rows(sG, rows);
        }
        __syncthreads();
        // pass 2: item-table scatter (float atomics, no return)
        {
          int t = tid / di, cc = tid - t * di;
          constexpr int dt = nthr / di, dc = nthr - dt * di;
          for (; t < rows;) {
            const float h = sT[t * DS + cc];
            const float dp = s_dpl[r0 + t], dn = s_dnl[r0 + t];
            const int pid = s_pid[r0 + t], nid = s_nid[r0 + t];
            if (a.contrib != nullptr) {
              a.contrib[(((int64_t)0 * B + b) * L + r0 + t) * di + cc] = pid != 0 ? dp * h : 0.f;
              a.contrib[(((int64_t)1 * B + b) * L + r0 + t) * di + cc] = nid != 0 ? dn * h : 0.f;
            } else {
              if (pid != 0 && dp != 0.f) atomicAdd(&a.grad_table[(int64_t)pid * di + cc], dp * h);
              if (nid != 0 && dn != 0.f) atomicAdd(&a.grad_table[(int64_t)nid * di + cc], dn * h);
            }
            t += dt; cc += dc;
            if (cc >= di) { cc -= di; ++t; }
          }
        }
        if (K_ == SRFRD_SRFRN)                // fake_embed rows of the targets (per chunk: partial sums, += in the slab)
          for (int p = wave; p < 2 * dfk; p += nw) {
            constexpr int dq = dfk > 0 ? dfk : 1;
            const int f = 1 + p / dq, cc = p - (f - 1) * dq;
            float sacc = 0.f;
            for (int t = lane; t < rows; t += 64) {
              const float w = (s_pfk[r0 + t] == f ? s_dpl[r0 + t] : 0.f) + (s_nfk[r0 + t] == f ? s_dnl[r0 + t] : 0.f);
              sacc += w * sT[t * DS + di + cc];
            }
            sacc = wave_sum(sacc);
            if (lane == 0) atomicAdd(&slab[ly.off_side + dfk + p], sacc);
          }
        // last LayerNorm backward: dx -> sK, g * xhat -> sO
        ln_bwd_rows<false>(nw, sG, lnin, sK, sO, rows, CR, DS, dout, s_ln + (4 * ly.n_blocks) * 64);
        head_zero_cols(sK, DS, rows, dout, D, tid, nthr);
        zero_tail_rows(sK, rows);
        __syncthreads();
        gemm_tiles<0>(nw, 1, (dout + 15) >> 4, kr, OnesRow{}, Mat{sG, DS},
                      [=](int r, int cc, float v) { if (r == 0 && cc < dout) s_lng[(4 * ly.n_blocks + 1) * 64 + cc] += v; });
        gemm_tiles<0>(nw, 1, (dout + 15) >> 4, kr, OnesRow{}, Mat{sO, DS},
                      [=](int r, int cc, float v) { if (r == 0 && cc < dout) s_lng[(4 * ly.n_blocks + 0) * 64 + cc] += v; });
        lds_f* Gc = sK;
        if (K_ == SRFRD_SRFR) {             // dWlc += G^T x_nb ; G <- G Wlc
          __syncthreads();                   // (the column sums above still read sG)
          dw_add(wlc, MatT{sK, DS}, Mat{sX, DS}, kr);
          const WFrag wln = load_wfrag(pk(ly.n_blocks * 6, 1), nullptr, 0, NT);
          gemm_packed(nw, ct, NT, (di + 3) & ~3, Mat{sK, DS}, wln, [&](int r, int cc, float v) { if (cc < D && r < CR) sG[r * DS + cc] = v; });
          Gc = sG;
        }
        __syncthreads();
        store_chunk(gbuf + r0 * D, Gc, rows);
        __syncthreads();
      }
      if (K_ == SRFRD_SRFR) dw_store(sl_lc, wlc);
      // (end of a pass: its scratch rows are read by the next pass - the stores are made to complete here; a workgroup
      // barrier alone orders LDS, not global memory, on this target)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }

    for (int i = ly.n_blocks - 1; i >= 0; --i) {
      const BlkOff o = blk_off(ly.blk0 + i * ly.blk_stride, D);
      const DropSite ds2 = drop_site(drop_on, seed, site_ffn2(i), seq, a.drop_thr, a.drop_scale);
      const AuxOff ax = aux_off(i, b, ly.n_blocks, L, LP, D);
      // ================= pass 1: FFN half.  y = (drop2(a2) + h2) * keep, a2 = r W2^T + b2, r = relu(drop1(h2 W1^T + b1))
      {
        const SlabWB sl_w2{slab, o.c2_w, o.c2_b, D, D, rmw};
        const SlabWB sl_w1{slab, o.c1_w, o.c1_b, D, D, rmw};
        DwAcc aw2 = dw_init(sl_w2), aw1 = dw_init(sl_w1);
        const WFrag w2n = load_wfrag(pk(i * 6 + 5, 1), nullptr, 0, NT);
        const WFrag w1n = load_wfrag(pk(i * 6 + 4, 1), nullptr, 0, NT);
        // (a chunk's rows are requested while the previous chunk is still being worked on and land when its slots are free)
        G2L<CIT, CV2> pg, px, pr;
        auto fetch1 = [&](int c) {
          const int r0 = c * CR, rows = rows_of(c);
          pg.load(gbuf + r0 * D, rows, D, nthr);
          px.load(a.c_save_h1 + h1_off(i, b, ly.n_blocks, L, D) + (int64_t)r0 * D, rows, D, nthr);
          pr.load(a.c_save_aux + ax.r + (int64_t)r0 * D, rows, D, nthr);
        };
        fetch1(0);
        for (int c = 0; c < NCH; ++c) {
          CK_RELANE();
          const int r0 = c * CR, rows = rows_of(c), kr = (rows + 3) & ~3, ct = (rows + 15) >> 4;
          lds_f *G = regA, *X = regA + CSZ, *Rr = regA + 2 * CSZ, *N = regA + 3 * CSZ, *A2 = regA + 4 * CSZ, *A1 = regA + 5 * CSZ;
          put_chunk(pg, G, rows);
          put_chunk(px, X, rows);
          put_chunk(pr, Rr, rows);
          ones_col(Rr, rows);
          __syncthreads();
          // h2 = LN2(h1) -> N ; dy *= keep (in place) ; dA2 = drop2'(dy) -> A2
          ln_rows(nw, X, N, rows, DS, D, s_ln + (4 * i + 2) * 64, s_ln + (4 * i + 3) * 64);
          zero_tail_rows(N, rows);
          ones_col(N, rows);
          for (int idx = tid; idx < CR * D; idx += nthr) {
            const int t = idx / D, cc = idx - t * D;
            const float g = t < rows ? G[t * DS + cc] * s_keep[r0 + t] : 0.f;
            G[t * DS + cc] = g;
            A2[t * DS + cc] = t < rows ? g * drop_mul(ds2, r0 + t, cc) : 0.f;
          }
          __syncthreads();
          // dA1 = (dA2 W2) * relu' -> A1 ; dW2 += dA2^T r
          gemm_packed(nw, ct, NT, DK, Mat{A2, DS}, w2n, [&](int r, int cc, float v) {
            if (cc < D && r < CR) A1[r * DS + cc] = Rr[r * DS + cc] > 0.f ? v * keep_scale : 0.f;
          });
          dw_add(aw2, MatT{A2, DS}, Mat{Rr, DS}, kr);
          __syncthreads();
          // dh2 = dy + dA1 W1 (in place) ; dW1 += dA1^T h2
          gemm_packed(nw, ct, NT, DK, Mat{A1, DS}, w1n, [&](int r, int cc, float v) { if (cc < D && r < CR) G[r * DS + cc] += v; });
          dw_add(aw1, MatT{A1, DS}, Mat{N, DS}, kr);
          __syncthreads();
          // LN2 backward: dh1 -> A2's slot, g * xhat -> Rr's slot
          lds_f *H = A2, *GX = Rr;
          ln_bwd_rows<false>(nw, G, X, H, GX, rows, CR, DS, D, s_ln + (4 * i + 2) * 64);
          if (c + 1 < NCH) fetch1(c + 1);
          __syncthreads();
          gemm_tiles<0>(nw, 1, NT, kr, OnesRow{}, Mat{G, DS}, [=](int r, int cc, float v) { if (r == 0 && cc < D) s_lng[(4 * i + 3) * 64 + cc] += v; });
          gemm_tiles<0>(nw, 1, NT, kr, OnesRow{}, Mat{GX, DS}, [=](int r, int cc, float v) { if (r == 0 && cc < D) s_lng[(4 * i + 2) * 64 + cc] += v; });
          store_chunk(hbuf + r0 * D, H, rows);
          __syncthreads();
        }
        dw_store(sl_w2, aw2);
        dw_store(sl_w1, aw1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
      // ================= pass 2: attention.  h1 = LN1(x) + o Wo^T + bo, o = drop(P) v   (P, o, q, k, v from the checkpoint)
      lds_f *Kb = regA, *Vb = regA + LR * DS;
      {
        CK_RELANE();
        const SlabWB sl_wo{slab, o.out_w, o.out_b, D, D, rmw};
        DwAcc awo = dw_init(sl_wo);
        copy_g2l<BIT, CV2>(Kb, DS, a.c_save_aux + ax.k, L, D, nthr);
        copy_g2l<BIT, CV2>(Vb, DS, a.c_save_aux + ax.v, L, D, nthr);
        for (int idx = tid; idx < (LR - L) * DS; idx += nthr) { Kb[L * DS + idx] = 0.f; Vb[L * DS + idx] = 0.f; }
        // dv / dk accumulators: strip nt = wave % 4, key tiles g, g + 2, ... (g = wave / 4): up to 7 of the 13 key tiles
        const int ant = wave & 3, ag = wave >> 2;
        f32x4 dv_acc[7], dk_acc[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) { dv_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dk_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        lds_f *S = regB, *DO = regC, *Qc = regC + CSZ;
        G2L<CIT, CV2> ph, po, pq;
        G2L<PIT, true> pp;
        auto fetch2 = [&](int ch) {
          const int q0 = ch * CR, rows = rows_of(ch);
          ph.load(hbuf + q0 * D, rows, D, nthr);
          po.load(a.c_save_aux + ax.o + (int64_t)q0 * D, rows, D, nthr);
        };
        fetch2(0);
        for (int ch = 0; ch < NCH; ++ch) {
          CK_RELANE();
          const int q0 = ch * CR, rows = rows_of(ch), cr = (rows + 3) & ~3, q1 = q0 + cr;
          const int qt0 = q0 >> 4, qtn = (cr + 15) >> 4, ct = qtn;
          const int ktn = (min(q0 + rows, L) + 15) >> 4;             // key tiles that any query of the chunk sees
          lds_f *Hc = Qc, *Oc = S;                                   // (dead before q_c / P_c take these places)
          // (Wo's fragments per chunk, not per pass: 53 registers that the dv / dk / dPd accumulators need in between)
          const WFrag won = load_wfrag(pk(i * 6 + 3, 1), nullptr, 0, NT, tid);
          put_chunk(ph, Hc, rows);
          put_chunk(po, Oc, rows);
          ones_col(Oc, rows);
          // the chunk's probabilities and queries: in flight under the do / dWo phase and the delta pass
          pp.load2d(a.c_save_aux + ax.p + (int64_t)q0 * LP, rows, LR, LP, nthr);
          pq.load(a.c_save_aux + ax.q + (int64_t)q0 * D, rows, D, nthr);
          __syncthreads();
          // do = dh1 Wo -> DO (columns D..DK-1 too: exact zeros) ; dWo += dh1^T o
          gemm_packed(nw, ct, NT, DK, Mat{Hc, DS}, won, [&](int r, int cc, float v) { if (cc < DK && r < CR) DO[r * DS + cc] = v; });
          dw_add(awo, MatT{Hc, DS}, Mat{Oc, DS}, cr);
          __syncthreads();
          // delta_i = do_i . o_i
          {
            const int q = tid & (kRL - 1);
            for (int r = tid / kRL; r < rows; r += nthr / kRL) {
              float s = 0.f;
#pragma unroll
              for (int j = 0; j < kQC; ++j) {
                const int cc = q + kRL * j;
                if (cc < D) s += DO[r * DS + cc] * Oc[r * DS + cc];
              }
              s = row_sum(s);
              if (q == 0) s_delta[r] = s;
            }
          }
          __syncthreads();
          // P_c -> S ([rows][LR] window of the sign-coded [L][LP] block) ; q_c -> Qc
          {
            pp.store(S, SLD, rows, LR, nthr);
            for (int idx = tid; idx < (cr - rows) * SLD; idx += nthr) S[rows * SLD + idx] = 0.f;
            put_chunk(pq, Qc, rows);
          }
          __syncthreads();
          // dv += drop(P_c)^T do_c (registers) ; dPd_c = do_c v^T (registers: tiles u = wave, wave + 8, ...)
          f32x4 dp_acc[5];
#pragma unroll
          for (int j = 0; j < 5; ++j) dp_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            const int u = wave + j * nw;
            const int m = u / ktn, n = u - m * ktn;
            if (m < qtn && n <= qt0 + m) {
              f32x4 acc1[1] = {dp_acc[j]};
              mma_group<1>(acc1, Mat{DO, DS}, MatT{Vb, DS}, (m << 4) + li, 0, (n << 4) + li, 0, DK, lq);
              dp_acc[j] = acc1[0];
            }
          }
#pragma unroll
          for (int j = 0; j < 7; ++j) {
            const int kt = ag + 2 * j;
            if (kt < ktn) {
              f32x4 acc1[1] = {dv_acc[j]};
              const int k0 = imax(0, (kt << 4) - q0);
              mma_group<1>(acc1, MatTPos{S, SLD}, Mat{DO, DS}, (kt << 4) + li, 0, (ant << 4) + li, k0, cr, lq);
              dv_acc[j] = acc1[0];
            }
          }
          __syncthreads();
          // dS_c = P_c * (mask / (1 - p) * dPd_c - delta) over P_c, element by element (own tiles)
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            const int u = wave + j * nw;
            const int m = u / ktn, n = u - m * ktn;
            if (m < qtn && n <= qt0 + m) {
              const int col = (n << 4) + li;
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int r = (m << 4) + (lq << 2) + e;
                if (r < rows && col < LR) {
                  const float pm = S[r * SLD + col];
                  const float dp = pm > 0.f ? dp_acc[j][e] * keep_scale : 0.f;
                  S[r * SLD + col] = fabsf(pm) * (dp - s_delta[r]);
                }
              }
            }
          }
          __syncthreads();
          // dq_c = dS_c k * qscale -> DO (do_c is dead) ; dk += dS_c^T q_c (registers)
          {
            const Mat As{S - q0 * SLD, SLD};                 // addressed by global query row
            lds_f* DOg = DO - q0 * DS;
            for (int mt = qt0 + ag; mt < qt0 + qtn; mt += 2)
              gemm_group<2, 1>(mt, 2, ant << 4, LR, As, Mat{Kb, DS},
                               [&](int r, int cc, float v) { if (cc < D && r < q0 + CR) DOg[r * DS + cc] = v * qscale; }, li, lq);
          }
#pragma unroll
          for (int j = 0; j < 7; ++j) {
            const int kt = ag + 2 * j;
            if (kt < ktn) {
              f32x4 acc1[1] = {dk_acc[j]};
              const int k0 = imax(0, (kt << 4) - q0);
              mma_group<1>(acc1, MatT{S, SLD}, Mat{Qc, DS}, (kt << 4) + li, 0, (ant << 4) + li, k0, cr, lq);
              dk_acc[j] = acc1[0];
            }
          }
          if (ch + 1 < NCH) fetch2(ch + 1);
          __syncthreads();
          store_chunk(qbuf + q0 * D, DO, rows);
          __syncthreads();
          (void)q1;
        }
        dw_store(sl_wo, awo);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        CK_RELANE();
        // dv -> V's place, dk -> K's place (rows < LR)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int kt = ag + 2 * j;
          const int cc = (ant << 4) + li;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = (kt << 4) + (lq << 2) + e;
            if (r < LR && cc < D) {
              Vb[r * DS + cc] = dv_acc[j][e] * keep_scale;
              Kb[r * DS + cc] = dk_acc[j][e];
            }
          }
        }
        __syncthreads();
      }
      // ================= pass 3: projections.  dLN1 = dh1 + dq Wq ; dx = dk Wk + dv Wv + LN1 backward -> next dy
      {
        const SlabWB sl_wq{slab, o.in_w, o.in_b, D, D, rmw};
        const SlabWB sl_wk{slab, o.in_w + D * D, o.in_b + D, D, D, rmw};
        const SlabWB sl_wv{slab, o.in_w + 2 * D * D, o.in_b + 2 * D, D, D, rmw};
        DwAcc awq = dw_init(sl_wq), awk = dw_init(sl_wk), awv = dw_init(sl_wv);
        G2L<CIT, CV2> pdq, ph3, px3;
        auto fetch3 = [&](int c) {
          const int r0 = c * CR, rows = rows_of(c);
          pdq.load(qbuf + r0 * D, rows, D, nthr);
          ph3.load(hbuf + r0 * D, rows, D, nthr);
          px3.load(a.c_save_x + x_off(i, b, ly.n_blocks, L, D) + (int64_t)r0 * D, rows, D, nthr);
        };
        fetch3(0);
        for (int c = 0; c < NCH; ++c) {
          CK_RELANE();
          const int r0 = c * CR, rows = rows_of(c), kr = (rows + 3) & ~3, ct = (rows + 15) >> 4;
          lds_f *DQ = regB, *H = regB + CSZ, *Xb = regB + 2 * CSZ, *DX = regB + 3 * CSZ, *N1 = regB + 4 * CSZ;
          const lds_f *DKc = Kb + r0 * DS, *DVc = Vb + r0 * DS;      // rows of the chunk in dk / dv (rows >= L are zero)
          put_chunk(pdq, DQ, rows);
          put_chunk(ph3, H, rows);
          put_chunk(px3, Xb, rows);
          ones_col(Xb, rows);
          const WFrag wqn = load_wfrag(pk(i * 6 + 0, 1), nullptr, 0, NT, tid);
          const WFrag wkn = load_wfrag(pk(i * 6 + 1, 1), nullptr, 0, NT, tid);
          __syncthreads();
          gemm_packed(nw, ct, NT, DK, Mat{DQ, DS}, wqn, [&](int r, int cc, float v) { if (cc < D && r < CR) H[r * DS + cc] += v; });
          const WFrag wvn = load_wfrag(pk(i * 6 + 2, 1), nullptr, 0, NT, tid);
          gemm_packed(nw, ct, NT, DK, Mat{DKc, DS}, wkn, [&](int r, int cc, float v) { if (cc < D && r < CR) DX[r * DS + cc] = r < rows ? v : 0.f; });
          gemm_packed(nw, ct, NT, DK, Mat{DVc, DS}, wvn, [&](int r, int cc, float v) { if (cc < D && r < rows) DX[r * DS + cc] += v; });
          dw_add(awk, MatT{DKc, DS}, Mat{Xb, DS}, kr);
          dw_add(awv, MatT{DVc, DS}, Mat{Xb, DS}, kr);
          ln_rows(nw, Xb, N1, rows, DS, D, s_ln + (4 * i + 0) * 64, s_ln + (4 * i + 1) * 64);
          zero_tail_rows(N1, rows);
          ones_col(N1, rows);
          __syncthreads();
          dw_add(awq, MatT{DQ, DS}, Mat{N1, DS}, kr);
          __syncthreads();
          // LN1 backward: DX += dx(dLN1), g * xhat -> GX1 (= dq's slot: dq is dead)
          lds_f* GX1 = DQ;
          ln_bwd_rows<true>(nw, H, Xb, DX, GX1, rows, CR, DS, D, s_ln + (4 * i + 0) * 64);
          if (c + 1 < NCH) fetch3(c + 1);
          __syncthreads();
          gemm_tiles<0>(nw, 1, NT, kr, OnesRow{}, Mat{H, DS}, [=](int r, int cc, float v) { if (r == 0 && cc < D) s_lng[(4 * i + 1) * 64 + cc] += v; });
          gemm_tiles<0>(nw, 1, NT, kr, OnesRow{}, Mat{GX1, DS}, [=](int r, int cc, float v) { if (r == 0 && cc < D) s_lng[(4 * i + 0) * 64 + cc] += v; });
          store_chunk(gbuf + r0 * D, DX, rows);
          __syncthreads();
        }
        dw_store(sl_wq, awq);
        dw_store(sl_wk, awk);
        dw_store(sl_wv, awv);
      }
    }
    // (the embedding backward reads the last chunk's dy rows from scratch one barrier after they were stored: make the
    // stores complete first - a workgroup barrier alone orders LDS, not global memory, here)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ================= embedding backward from gbuf: item rows (atomics), position table, side channel
    {
      const DropSite dsE = drop_site(drop_on && is_sas, seed, SITE_EMB, seq, a.drop_thr, a.drop_scale);
      CK_RELANE();
      {
        int t = tid / di, c = tid - t * di;
        constexpr int dt = nthr / di, dc = nthr - dt * di;
        for (; t < L;) {
          float gv = gbuf[t * D + c] * s_keep[t];
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
          return s_fk[t] == f ? gbuf[t * D + di + c] * s_keep[t] : 0.f;
        }, [&](int p) { return ly.off_side + dfk + p; });
      if (is_srfu) {
        const int lab = ((lds_i*)s_misc)[0];
        side_sums(D, [&](int c, int t) { return gbuf[t * D + c] * s_keep[t]; }, [&](int c) { return ly.off_side + lab * D + c; });
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

#undef CK_RELANE

}  // namespace SRFRD_NS
