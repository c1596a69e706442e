// Ragged fused encoder backward (hidden 50, seq_len 50, 8 waves, two workgroups per CU): the slot-placed backward of
// srfrd_encoder_bwd_slots_kernel.inc (six [52][54] LDS slots, matrices placed by liveness, one query chunk) walked only over
// the rows a LEFT-PADDED sequence really has - the counterpart of srfrd_encoder_fwd_ragged_kernel.inc, whose checkpoints
// (rows of the computed tiles only, the merged leading pads as one representative key) it reads.
//
// With t0 leading pads, v0 = t0 the first valid position and kr = t0 - 1 the representative key (or 0 when t0 = 0):
//   * per-token work (FFN half, projections, LayerNorm passes, dq) runs on the 16-row tiles mt0 .. 3, mt0 = (kr + 12) / 16,
//     in TILE coordinates: position t is tile row t + 12 (= slot row t: a slot holds tile rows 12 .. 63), so the end of the
//     sequence sits in the last tile.  GEMM operands are the slots' pointers biased by -12 rows; tile rows 0 .. 11 of tile 0
//     alias the previous slot (or a guard region): whatever they hold reaches only output rows no epilogue stores;
//   * sums over tokens (every weight gradient, dv, dk, the column sums) take k = max(16 mt0, 12) .. 63;
//   * the representative key row: P~_i,rep = c_i / (1 - p) P_i,rep is what multiplies do_i in dv (c_i P_i,rep is stored in the
//     probability checkpoint's column kr), and the t0 merged columns' score gradients add up to
//         dS_i,rep = P~_i,rep dPd_i,rep - (t0 P_i,rep) delta_i          (t0 P_i,rep: column LP - 1 of the checkpoint row)
//     so dq_i gets dS_i,rep b_k through the ordinary dS k product, and rows kr of dk / dv hold the TOTAL over the merged pads:
//     they reach b_k / b_v through the ones column of x (x[kr] = 0: no weight gradient), exactly what the pads contribute.
//   * the head (logits backward, last LayerNorm) starts at the first position that carries an upstream gradient - the first
//     non-zero target or input id (every position when a hidden-state gradient is given).
// Same sums in another order than the full kernel: fp32 rounding-level differences, the oracle bar unchanged.
namespace SRFRD_NS {

// (bwd_ragged_lds_floats: srfrd_enc_common.h, where the kernel plan reads it)

// LDS working set of the ragged backward: base = the 12-row guard in front of six [52][54] slots, 12 per-position arrays and
// 64 misc words (kRagBwdWork floats), then the LayerNorm parameters and their gradient accumulators wherever the caller
// put them (s_lng persists across the sequences of a workgroup).
struct RagBwdLds {
  lds_f* base;
  lds_f* s_ln;
  lds_f* s_lng;
};

// The ragged backward of sequence b (the workgroup's iter-th) by the whole workgroup (512 threads): reads the checkpoints
// of the ragged forward, scatters item-row gradients, accumulates the dense ones into this workgroup's slab and s_lng; ends
// with a workgroup barrier.  tid: the laundered thread index (see launder), wave: its wave (uniform).
// SEAM_ (the train kernel): rag_fwd_seq<.., SEAM_> of the same workgroup has done the head's first part and rag_seam_handoff
// has left the working set as this function's own first phase would: the last block's output in sX, d hidden in sG (slot
// kRagSeamG), the ids in the per-position arrays - nothing of it is read from global memory again; the target rows'
// item-table contributions are out already.  hs: what the forward returned.
template <int K_, int DI_, bool RMW_, bool SEAM_ = false>
__device__ __forceinline__ void rag_bwd_seq(const EncArgs& a, const RagBwdLds& m, int b, int iter, int& tid, int wave, uint32_t seed,
                                            const RagSeam& hs = RagSeam{}) {
  const Dims& ly = a.dm;
  constexpr int nw = 8, nthr = 512;
  constexpr int L = 50, D = 50, LP = 64, DK = 52, DS = 54, NT = 4, MT = 4;
  constexpr int R = 52, SZ = R * DS, SLD = R + 2, SH = kRagSH;
  static_assert(SH == LP - R && R * SLD <= SZ + 2 * R, "slot geometry");
  static_assert(kRagBwdWork == SH * DS + 6 * SZ + (kHeadRows + 4) * LP, "working set");
  constexpr bool CV2 = true;
  constexpr int CIT = (R * (D / 2) + nthr - 1) / nthr;
  constexpr int PIT = (R * (R / 2) + nthr - 1) / nthr;
  lds_f* slot[6];
#pragma unroll
  for (int s = 0; s < 6; ++s) slot[s] = m.base + SH * DS + s * SZ;
  lds_f* tail = m.base + SH * DS + 6 * SZ;
  lds_i* s_in = (lds_i*)(tail + kRowIn * LP);   // per-position arrays (position coordinates)
  lds_f* s_keep = tail + kRowKeep * LP;
  lds_i* s_pid = (lds_i*)(tail + kRowPid * LP);
  lds_i* s_nid = (lds_i*)(tail + kRowNid * LP);
  lds_i* s_fk = (lds_i*)(tail + kRowFk * LP);
  lds_i* s_pfk = (lds_i*)(tail + kRowPfk * LP);
  lds_i* s_nfk = (lds_i*)(tail + kRowNfk * LP);
  lds_f* s_dpl = tail + kRowDpl * LP;
  lds_f* s_dnl = tail + kRowDnl * LP;
  lds_f* s_delta = tail + kHeadRows * LP;
  lds_f* s_brep = tail + (kHeadRows + 1) * LP;        // t0 P_i,rep of the block being walked
  lds_f* s_dummy = tail + (kHeadRows + 2) * LP;       // 64 scratch words: where branch-free epilogues store what must not land anywhere
  lds_f* s_misc = tail + (kHeadRows + 3) * LP;        // 64
  lds_f* s_ln = m.s_ln;
  lds_f* s_lng = m.s_lng;
  const float* P = a.dense;
  const bool drop_on = a.drop_on != 0;
  const int rkind = K_ >= 0 ? K_ : ly.kind;
  const bool is_sas = rkind == SRFRD_SASREC;
  const bool has_fake = rkind == SRFRD_SRFR || rkind == SRFRD_SRFRN;
  const bool is_srfu = rkind >= SRFRD_SRFU_B;
  constexpr int di = DI_, dfk = D - DI_;
  constexpr int dout = (K_ == SRFRD_SRFR) ? DI_ : D;
  const float sqrtD = sqrtf((float)di);
  const float qscale = a.qscale;
  const int B = a.B;
  auto pk = [&](int mat, int form) {
    return PackedB{reinterpret_cast<const float4*>(a.packed) + ((int64_t)mat * 2 + form) * (kPackFloats / 4)};
  };
  // (one predicated store each: L and (R - L) * DS are below the workgroup size)
  static_assert(L <= nthr && (R - L) * DS <= nthr, "single-pass helpers");
  auto ones_col = [&](lds_f* buf) {
    if (tid < L) buf[tid * DS + D] = 1.0f;
  };
  auto zero_pad_rows = [&](lds_f* buf) {        // slot rows L .. R - 1 (tile rows 62, 63): the zero padding of every token sum
    if (tid < (R - L) * DS) buf[L * DS + tid] = 0.f;
  };
  const float keep_scale = drop_on ? a.drop_scale : 1.0f;

  asm volatile("" : "+v"(tid));
  float* slab = a.grad_slabs + (int64_t)blockIdx.x * ly.n_dense;
  const int rmw = RMW_ ? (iter != 0) : 0;
  if (iter == 0)
    for (int i = tid; i < ly.blk0; i += nthr) slab[i] = 0.f;      // position / side tables accumulate with +=
  const int64_t rowbase = (int64_t)b * L;
  const uint32_t seq = (uint32_t)(a.seq0 + b);
  const int lane0 = tid & 63;
  if (!SEAM_ && tid < LP) {
    const int t = tid;
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
      if (a.fused_bce) {                   // fused masked BCE
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
  if (is_srfu && wave == 1) {
    const int lab = user_label_wave(rkind, a.fk_ids ? a.fk_ids + rowbase : nullptr, L, ly.n_labels);
    if (lane0 == 0) ((lds_i*)s_misc)[0] = lab;       // (read after the blocks: any later barrier orders it)
  }
  if constexpr (!SEAM_) __syncthreads();
  // ---- the sequence's rows (wave-uniform): t0 leading pads; head range from the first position with an upstream gradient
  int t0, th;
  if constexpr (SEAM_) {
    t0 = hs.t0;
    th = hs.th;
  } else {
    const bool inr = lane0 < L;
    const unsigned long long nz = __ballot(inr && s_in[lane0] != 0);
    const unsigned long long ng = __ballot(inr && (s_in[lane0] != 0 || s_dpl[lane0] != 0.f || s_dnl[lane0] != 0.f));
    t0 = nz ? (int)__builtin_ctzll(nz) : L;
    th = ng ? (int)__builtin_ctzll(ng) : L;
    if (a.ragged_off) t0 = 0;
    if (a.d_hidden != nullptr || a.ragged_off) th = 0;
    t0 = __builtin_amdgcn_readfirstlane(t0);
    th = __builtin_amdgcn_readfirstlane(th);
  }
  const int krp = t0 >= 1 ? t0 - 1 : 0;                   // representative key (position)
  const int kr = krp + SH, v0 = t0 + SH;                   // ... and first valid row, in tile coordinates
  const int mt0 = kr >> 4, r0 = mt0 << 4, mtn = MT - mt0;
  const int p0 = r0 > SH ? r0 - SH : 0;                    // first position of the computed tiles
  const int k0 = p0 + SH;                                  // first token of the token sums (tile coordinates)
  // head: tiles from the first position with an upstream gradient (never behind the blocks' range)
  const RagHead hr = rag_head_range(th, krp);
  const int mh0 = hr.tile0, mhn = MT - mh0;
  const int ph0 = hr.pos0, kh0 = ph0 + SH;

  // (SEAM_: d hidden arrives in slot kRagSeamG, whose floats the forward's head no longer needs when it writes them)
  static_assert(kRagSlot == SZ && kRagSeamG == 3, "hand-off slot");
  lds_f *sX = slot[0], *sQ = slot[1], *sG = slot[SEAM_ ? 3 : 2], *sT = slot[SEAM_ ? 2 : 3], *sK = slot[4], *sO = slot[5];
  // GEMM epilogues are BRANCH-FREE: an element outside the matrix (column >= D of the last strip, or a tile row in front of
  // row 12 that aliases the previous slot) is stored to this scratch word instead of being skipped - with a branch per element
  // hipcc wraps each of a tile's eight stores (and the LDS read some of them need) in its own exec-mask region and waits for
  // every read on its own; straight-line code shares one row address and overlaps the reads
  lds_f* dummy = s_dummy;            // [64], indexed by the lane's column: no same-address store conflicts
  // (tile-coordinate view of a slot: tile row r = slot row r - SH)
#define TB(p) ((p) - SH * DS)
  G2L<CIT, CV2> g_last, g_h1, g_r;
  if constexpr (!SEAM_) g_last.load(a.c_save_x + x_off(ly.n_blocks, b, ly.n_blocks, L, D) + p0 * D, L - p0, D, nthr);
  g_h1.load(a.c_save_h1 + h1_off(ly.n_blocks - 1, b, ly.n_blocks, L, D) + p0 * D, L - p0, D, nthr);
  g_r.load(a.c_save_aux + aux_off(ly.n_blocks - 1, b, ly.n_blocks, L, LP, D).r + p0 * D, L - p0, D, nthr);
  if constexpr (SEAM_) {                // SRFRN: the hidden rows -> sT for the side-channel sums (everything else is in place)
    if constexpr (K_ == SRFRD_SRFRN) {
      constexpr bool V2 = dout % 2 == 0;    // (8-byte accesses: every head range starts at an even float offset)
      constexpr int HIT = (L * (V2 ? dout / 2 : dout) + nthr - 1) / nthr;
      G2L<HIT, V2> g_hid;
      g_hid.load(a.c_hidden + (rowbase + ph0) * dout, L - ph0, dout, nthr);
      g_hid.store(sT + ph0 * DS, DS, L - ph0, dout, nthr);
      __syncthreads();
    }
  } else {
    g_last.store(sX + p0 * DS, DS, L - p0, D, nthr);
    // (head rows in front of the blocks' range - pad positions that carry an upstream gradient - are exact zeros: the
    // forward did not write them)
    // (column D, the ones column, is left to ones_col below: eight rows x 64 columns per pass, no division)
    for (int r = ph0 + (tid >> 6); r < p0; r += nthr >> 6) {
      const int c = tid & 63;
      if (c < DS && c != D) sX[r * DS + c] = 0.f;
    }
    zero_pad_rows(sX);
    ones_col(sX);
    zero_pad_rows(sG);
    __syncthreads();
  }

  // (per-lane indices are re-derived from the laundered thread index per block: nothing computed from them may be lifted out
  // of the block loop - hipcc otherwise precomputes hundreds of per-lane addresses, spills them and reloads each before use)
  int lane = tid & 63, li = lane & 15, lq = lane >> 4;
#define RG_RELANE() do { asm volatile("" : "+v"(tid)); lane = tid & 63; li = lane & 15; lq = lane >> 4; } while (0)
  const int nt_w = wave & 3, g_w = wave >> 2;
  // ---- small GEMM helpers on tile coordinates (operands: biased pointers) ----------------------------------------------
  // weight gradient (4 x 4 tiles of features) += dY^T [X | 1] over tokens [kk0, 64): rows g_w, g_w + 2 of strip nt_w
  auto slab_gemm = [&](int kk0, auto amat, auto bmat, const SlabWB& sl, const SlabPre& pre) {
    f32x4 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j] = f32x4{pre.v[j][0], pre.v[j][1], pre.v[j][2], pre.v[j][3]};
    mma_group<2>(acc, amat, bmat, (g_w << 4) + li, 32, (nt_w << 4) + li, kk0, LP, lq);
    const SlabCol sc = slab_col(sl, (nt_w << 4) + li);
    if (sc.ok) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = ((g_w + 2 * j) << 4) + (lq << 2) + e;
          if (r < sl.R) sl.base[(unsigned)(sc.col0 + r * sc.rs)] = acc[j][e];
        }
    }
  };
  // column sums of tokens [kk0, 64) of a [.][DS] matrix -> += into an LDS vector (waves 0 .. 3, one strip each)
  auto col_sums = [&](int kk0, const lds_f* m_b, lds_f* dst, int ncol) {
    if (wave < NT) {
      f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
      mma_group<1>(acc, OnesRow{}, Mat{m_b, DS}, li, 0, (wave << 4) + li, kk0, LP, lq);
      const int c = (wave << 4) + li;
      if (lq == 0 && c < ncol) dst[c] += acc[0][0];
    }
  };
  auto side_sums = [&](int n_out, auto term, auto dst_off, int tlo) {
    for (int p = wave; p < n_out; p += nw) {
      float sacc = 0.f;
      for (int t = tlo + lane; t < L; t += 64) sacc += term(p, t);
      sacc = wave_sum(sacc);
      if (lane == 0) atomicAdd(&slab[dst_off(p)], sacc);
    }
  };

  const lds_f* lnin = sX;
  if (K_ == SRFRD_SRFR) {               // hc = hf Wlc^T + blc -> sQ (input of the last LayerNorm)
    const WFrag wl = load_wfrag(pk(ly.n_blocks * 6, 0), P + ly.off_lc_b, di, (di + 15) >> 4, tid);
    {                                   // (three strips: load_wfrag dealt strip wave % 3; waves 0 .. 5 = 3 strips x 2 row-tile groups)
      constexpr int nst = (di + 15) >> 4;
      const int nt3 = wave % nst, g3 = wave / nst;
      auto epi = [&](int r, int c, float v) { *((c < di && r >= SH && r < SH + L) ? &TB(sQ)[r * DS + c] : dummy + c) = v; };
      if (g3 < 2) {
        if (g3 + 2 < mhn) gemm_group_packed<2>(mh0 + g3, 2, nt3, DK >> 2, Mat{TB(sX), DS}, wl, epi, lane);
        else if (g3 < mhn) gemm_group_packed<1>(mh0 + g3, 2, nt3, DK >> 2, Mat{TB(sX), DS}, wl, epi, lane);
      }
    }
    __syncthreads();
    lnin = sQ;
  }
  // ---- logits backward.  Pass 1: dh -> sG and the hidden rows -> sT (positions ph0 .. L - 1, coalesced row gathers)
  if constexpr (!SEAM_) {
    const bool srfrn = K_ == SRFRD_SRFRN;
    const int n = (L - ph0) * dout;
    constexpr int GIT = (LP * D + nthr - 1) / nthr;
    constexpr int HALF = (GIT + 1) / 2;
    const float* hid = a.c_hidden + (rowbase + ph0) * dout;
    const float* dhid = a.d_hidden ? a.d_hidden + (rowbase + ph0) * dout : nullptr;
    int tg = tid;
    asm volatile("" : "+v"(tg));
    auto chunks = [&](auto bf16_shadow) {
      constexpr bool H16 = decltype(bf16_shadow)::value;
      for (int base0 = 0; base0 < n; base0 += HALF * nthr) {
        float hv[HALF], pv[HALF], nv[HALF];
#pragma unroll
        for (int u = 0; u < HALF; ++u) {
          const int i = min(base0 + u * nthr + tg, n - 1);
          const int tt = i / dout, c = i - tt * dout, t = ph0 + tt;
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
            const int tt = i / dout, c = i - tt * dout, t = ph0 + tt;
            float dh = dhid ? dhid[i] : 0.f;
            if (c < di || srfrn) dh = head_dh(dh, s_dpl[t], pv[u], s_dnl[t], nv[u]);
            sT[t * DS + c] = hv[u];
            sG[t * DS + c] = dh;
          }
        }
      }
    };
    if (a.table16 != nullptr) chunks(std::true_type{});
    else chunks(std::false_type{});
    if (dout < D)
      for (int idx = tid; idx < (L - ph0) * (D - dout); idx += nthr) {
        const int tt = idx / (D - dout), cc = dout + idx - tt * (D - dout);
        sG[(ph0 + tt) * DS + cc] = 0.f;
      }
  }
  if constexpr (!SEAM_) __syncthreads();
  // Pass 2: item-table scatter (float atomics, no return): at most two contiguous row segments per wave-instruction
  if constexpr (!SEAM_) {
    int t = ph0 + tid / di, c = tid - (tid / di) * di;
    constexpr int dt = nthr / di, dc = nthr - dt * di;
    for (; t < L;) {
      const float h = sT[t * DS + c];
      const float dp = s_dpl[t], dn = s_dnl[t];
      const int pid = s_pid[t], nid = s_nid[t];
      if (a.contrib != nullptr) {          // deterministic mode: see srfrd_encoder_bwd_kernel.inc
        a.contrib[(((int64_t)0 * B + b) * L + t) * di + c] = pid != 0 ? head_contrib(dp, h) : 0.f;
        a.contrib[(((int64_t)1 * B + b) * L + t) * di + c] = nid != 0 ? head_contrib(dn, h) : 0.f;
      } else {
        if (pid != 0 && dp != 0.f) atomicAdd(&a.grad_table[(int64_t)pid * di + c], head_contrib(dp, h));
        if (nid != 0 && dn != 0.f) atomicAdd(&a.grad_table[(int64_t)nid * di + c], head_contrib(dn, h));
      }
      t += dt; c += dc;
      if (c >= di) { c -= di; ++t; }
    }
    if (a.contrib != nullptr)              // (the sorted reduction reads every row of the batch: rows in front of the head are zeros)
      for (int idx = tid; idx < ph0 * di; idx += nthr) {
        a.contrib[(((int64_t)0 * B + b) * L) * di + idx] = 0.f;
        a.contrib[(((int64_t)1 * B + b) * L) * di + idx] = 0.f;
      }
  }
  if (K_ == SRFRD_SRFRN)
    side_sums(2 * dfk, [&](int p, int t) {
      constexpr int dq = dfk > 0 ? dfk : 1;
      const int f = 1 + p / dq, c = p - (f - 1) * dq;
      const float w = (s_pfk[t] == f ? s_dpl[t] : 0.f) + (s_nfk[t] == f ? s_dnl[t] : 0.f);
      return w * sT[t * DS + di + c];
    }, [&](int p) { return ly.off_side + dfk + p; }, ph0);
  // ---- last LayerNorm backward: dx -> sK, g * xhat -> sO; dgamma / dbeta as ones-row GEMMs
  ln_bwd_rows<false>(nw, sG + ph0 * DS, lnin + ph0 * DS, sK + ph0 * DS, sO + ph0 * DS, L - ph0, R - ph0, DS, dout,
                     s_ln + (4 * ly.n_blocks) * 64);
  if (dout < D)
    for (int idx = tid; idx < (L - ph0) * (D - dout); idx += nthr) {
      const int tt = idx / (D - dout), cc = dout + idx - tt * (D - dout);
      sK[(ph0 + tt) * DS + cc] = 0.f;
    }
  zero_pad_rows(sK);
  __syncthreads();
  col_sums(kh0, TB(sG), s_lng + (4 * ly.n_blocks + 1) * 64, dout);
  col_sums(kh0, TB(sO), s_lng + (4 * ly.n_blocks + 0) * 64, dout);
  __syncthreads();
  // running gradient G = sK from here
  lds_f* G = sK;
  lds_f* fr[5] = {sG, sO, sT, sQ, sX};
  if (K_ == SRFRD_SRFR) {               // hc = hf Wlc^T + blc: dWlc += G^T x_nb, G <- G Wlc
    {
      const SlabWB sl{slab, ly.off_lc_w, ly.off_lc_b, di, D, rmw};
      // (three row tiles of 45 features: the general helper - tiles g_w, g_w + 2 - covers them)
      SlabPre pre = RMW_ ? slab_preload(nw, NT, NT, sl) : SlabPre{};
      slab_gemm(kh0, MatT{TB(G), DS}, Mat{TB(sX), DS}, sl, pre);
    }
    const WFrag wln = load_wfrag(pk(ly.n_blocks * 6, 1), nullptr, 0, NT, tid);
    lds_f* Gn = sG;
    {
      auto epi = [&](int r, int c, float v) { *((c < D && r >= SH) ? &TB(Gn)[r * DS + c] : dummy + c) = v; };
      if (g_w + 2 < mhn) gemm_group_packed<2>(mh0 + g_w, 2, nt_w, ((di + 3) & ~3) >> 2, Mat{TB(G), DS}, wln, epi, lane);
      else if (g_w < mhn) gemm_group_packed<1>(mh0 + g_w, 2, nt_w, ((di + 3) & ~3) >> 2, Mat{TB(G), DS}, wln, epi, lane);
    }
    __syncthreads();
    fr[0] = G;
    G = Gn;
  }

  for (int i = ly.n_blocks - 1; i >= 0; --i) {
    const BlkOff o = blk_off(ly.blk0 + i * ly.blk_stride, D);
    const DropSite ds2 = drop_site(drop_on, seed, site_ffn2(i), seq, a.drop_thr, a.drop_scale);
    const AuxOff ax = aux_off(i, b, ly.n_blocks, L, LP, D);
    RG_RELANE();
    lds_f *X = fr[0], *Rr = fr[1], *N = fr[2], *A2 = fr[3], *A1 = fr[4];
    launder(G); launder(X); launder(Rr); launder(N); launder(A2); launder(A1);
    // ================= FFN half: y = (drop2(a2) + h2) * keep, a2 = r W2^T + b2, r = relu(drop1(h2 W1^T + b1))
    const WFrag w2n = load_wfrag(pk(i * 6 + 5, 1), nullptr, 0, NT, tid);
    const SlabWB sl_w2{slab, o.c2_w, o.c2_b, D, D, rmw};
    const SlabWB sl_w1{slab, o.c1_w, o.c1_b, D, D, rmw};
    // ---- F1: dy *= keep (rows in front of p0 are never read again) and dA2 = drop2'(dy) -> A2 in the same pass (eight rows x
    // 64 columns per step: no division); checkpoints h1 -> X, r -> Rr
    {
      const int c = tid & 63;
      if (c < D)
        for (int r = p0 + (tid >> 6); r < R; r += nthr >> 6) {
          const float g = r < L ? G[r * DS + c] * s_keep[r] : 0.f;
          if (r < L) G[r * DS + c] = g;
          A2[r * DS + c] = g * drop_mul(ds2, r, c);
        }
    }
    g_h1.store(X + p0 * DS, DS, L - p0, D, nthr);
    g_r.store(Rr + p0 * DS, DS, L - p0, D, nthr);
    zero_pad_rows(X); zero_pad_rows(Rr); zero_pad_rows(G);
    ones_col(Rr);
    __syncthreads();
    // ---- F2: h2 = LN2(h1) -> N
    ln_rows(nw, X + p0 * DS, N + p0 * DS, L - p0, DS, D, s_ln + (4 * i + 2) * 64, s_ln + (4 * i + 3) * 64);
    zero_pad_rows(N);
    ones_col(N);
    __syncthreads();
    // ---- F3: dA1 = (dA2 W2) * relu' -> A1 ; dW2 += dA2^T r
    G2L<CIT, CV2> g_o, g_v, g_k;
    {
      SlabPre pre_w2 = RMW_ ? slab_preload(nw, NT, NT, sl_w2) : SlabPre{};
      rag_packed(mt0, mtn, DK >> 2, D, Mat{TB(A2), DS}, w2n, [&](int r, int c) { return TB(Rr)[r * DS + c]; },
                 [&](int r, int c, float v, float act) {
        *(r >= SH ? &TB(A1)[r * DS + c] : dummy + c) = act > 0.f ? v * keep_scale : 0.f;
      }, lane, wave);
      slab_gemm(k0, MatT{TB(A2), DS}, Mat{TB(Rr), DS}, sl_w2, pre_w2);
    }
    const WFrag w1n = load_wfrag(pk(i * 6 + 4, 1), nullptr, 0, NT, tid);
    g_o.load(a.c_save_aux + ax.o + p0 * D, L - p0, D, nthr);
    __syncthreads();
    // ---- F4: dh2 = dy + dA1 W1 (in place) ; dW1 += dA1^T h2           (A2, Rr are free afterwards)
    {
      SlabPre pre_w1 = RMW_ ? slab_preload(nw, NT, NT, sl_w1) : SlabPre{};
      rag_packed(mt0, mtn, DK >> 2, D, Mat{TB(A1), DS}, w1n, [&](int r, int c) { return TB(G)[r * DS + c]; },
                 [&](int r, int c, float v, float old) { *(r >= SH ? &TB(G)[r * DS + c] : dummy + c) = old + v; }, lane, wave);
      slab_gemm(k0, MatT{TB(A1), DS}, Mat{TB(N), DS}, sl_w1, pre_w1);
    }
    g_v.load(a.c_save_aux + ax.v + p0 * D, L - p0, D, nthr);
    __syncthreads();
    // ---- F5: LN2 backward: dh1 -> H (= A2's slot), g * xhat -> GX (= Rr's slot)            (A1, N free after this)
    lds_f *H = A2, *GX = Rr;
    ln_bwd_rows<false>(nw, G + p0 * DS, X + p0 * DS, H + p0 * DS, GX + p0 * DS, L - p0, R - p0, DS, D, s_ln + (4 * i + 2) * 64);
    zero_pad_rows(H);
    g_k.load(a.c_save_aux + ax.k + p0 * D, L - p0, D, nthr);
    __syncthreads();
    // ---- F6: column sums (dbeta2 from G, dgamma2 from GX); o -> O (= N's slot)
    lds_f* O = N;
    col_sums(k0, TB(G), s_lng + (4 * i + 3) * 64, D);
    col_sums(k0, TB(GX), s_lng + (4 * i + 2) * 64, D);
    g_o.store(O + p0 * DS, DS, L - p0, D, nthr);
    zero_pad_rows(O);
    ones_col(O);
    const WFrag won = load_wfrag(pk(i * 6 + 3, 1), nullptr, 0, NT, tid);
    G2L<PIT, true> g_p;
    g_p.load2d(a.c_save_aux + ax.p + p0 * LP + p0, L - p0, R - p0, LP, nthr);     // rows / columns p0 .. of the sign-coded probabilities
    // t0 P_i,rep of the valid rows (column LP - 1 of their checkpoint row), requested here, stored in A2
    float brep_v = 0.f;
    if (tid < L && tid >= t0 && t0 >= 1) brep_v = a.c_save_aux[ax.p + tid * LP + LP - 1];
    __syncthreads();
    // ================= attention half: h1 = LN1(x) + o Wo^T + bo, o = drop(P) v       (G, GX, X, A1 are free; dh1 = H)
    lds_f *DO = G, *V = GX, *Kk = X, *S = A1;
    RG_RELANE();
    const SlabWB sl_wo{slab, o.out_w, o.out_b, D, D, rmw};
    G2L<CIT, CV2> g_q, g_x;
    // ---- A1: do = dh1 Wo -> DO ; dWo += dh1^T o ; v -> V ; k -> Kk
    {
      SlabPre pre_wo = RMW_ ? slab_preload(nw, NT, NT, sl_wo) : SlabPre{};
      g_v.store(V + p0 * DS, DS, L - p0, D, nthr);
      g_k.store(Kk + p0 * DS, DS, L - p0, D, nthr);
      zero_pad_rows(V); zero_pad_rows(Kk);
      rag_packed(mt0, mtn, DK >> 2, DK, Mat{TB(H), DS}, won, NoPre{},
                 [&](int r, int c, float v, float) { *(r >= SH ? &TB(DO)[r * DS + c] : dummy + c) = v; }, lane, wave);
      slab_gemm(k0, MatT{TB(H), DS}, Mat{TB(O), DS}, sl_wo, pre_wo);
    }
    g_q.load(a.c_save_aux + ax.q + p0 * D, L - p0, D, nthr);
    __syncthreads();
    // ---- A2: delta_i = do_i . o_i ; P -> S
    {
      const int q = tid & (kRL - 1);
      for (int r = p0 + tid / kRL; r < L; r += nthr / kRL) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < kQC; ++j) {
          const int c = q + kRL * j;
          if (c < D) s += DO[r * DS + c] * O[r * DS + c];
        }
        s = row_sum(s);
        if (q == 0) s_delta[r] = s;
      }
      g_p.store(S + p0 * SLD + p0, SLD, L - p0, R - p0, nthr);
      for (int idx = tid; idx < (R - L) * SLD; idx += nthr) S[L * SLD + idx] = 0.f;
      if (tid < L) s_brep[tid] = brep_v;
    }
    __syncthreads();
    lds_f* Q = O;                                 // o is dead: q takes its slot
    lds_f* S_b = S - SH * SLD - SH;               // tile-coordinate view of the scores: S_b[r * SLD + c], r, c in [12, 64)
    // dPd / dS tiles: the lower triangle of the [mt0, 4) x [mt0, 4) tiles, dealt round-robin (<= 2 per wave);
    // dv / dk accumulators: strip nt_w, key tiles mt0 + g_w, mt0 + g_w + 2
    f32x4 dv_acc[2], dk_acc[2], dp_acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) { dv_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dk_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; dp_acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int ntri = (mtn * (mtn + 1)) >> 1;
    // ---- C1: dv += drop(P)^T do (registers) ; dPd = do v^T (registers)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int u = wave + j * nw;
      if (u < ntri) {
        const int m = u >= 6 ? 3 : (u >= 3 ? 2 : (u >= 1 ? 1 : 0)), n = u - ((m * (m + 1)) >> 1);
        f32x4 acc1[1] = {dp_acc[j]};
        mma_group<1>(acc1, Mat{TB(DO), DS}, MatT{TB(V), DS}, ((mt0 + m) << 4) + li, 0, ((mt0 + n) << 4) + li, 0, DK, lq);
        dp_acc[j] = acc1[0];
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kt = mt0 + g_w + 2 * j;
      if (kt < MT) {
        f32x4 acc1[1] = {dv_acc[j]};
        const int kq0 = imax(kt << 4, k0);
        mma_group<1>(acc1, MatTPos{S_b, SLD}, Mat{TB(DO), DS}, (kt << 4) + li, 0, (nt_w << 4) + li, kq0, LP, lq);
        dv_acc[j] = acc1[0];
      }
    }
    g_q.store(Q + p0 * DS, DS, L - p0, D, nthr);
    zero_pad_rows(Q);
    __syncthreads();
    // ---- C2: dS = P * (mask / (1 - p) * dPd - delta) over P, element by element (own tiles); the representative column:
    //          dS_rep = (c P_rep) / (1 - p) dPd - (t0 P_rep) delta
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int u = wave + j * nw;
      if (u < ntri) {
        const int m = u >= 6 ? 3 : (u >= 3 ? 2 : (u >= 1 ? 1 : 0)), n = u - ((m * (m + 1)) >> 1);
        const int col = ((mt0 + n) << 4) + li;
        const bool is_rep = t0 >= 1 && col == kr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = ((mt0 + m) << 4) + (lq << 2) + e;
          const bool ok = r >= v0 && r < SH + L && col >= kr;
          const int ip = min(max(r, SH), SH + L - 1) - SH;                 // (clamped: the reads below are unconditional)
          lds_f* sp = &S_b[r * SLD + col];
          const float pm = *sp;
          const float dl = s_delta[ip];
          const float dsr = pm * keep_scale * dp_acc[j][e] - s_brep[ip] * dl;
          const float dso = fabsf(pm) * ((pm > 0.f ? dp_acc[j][e] * keep_scale : 0.f) - dl);
          *(ok ? sp : dummy + (col & 63)) = is_rep ? dsr : dso;
        }
      }
    }
    g_x.load(a.c_save_x + x_off(i, b, ly.n_blocks, L, D) + p0 * D, L - p0, D, nthr);
    const WFrag wqn = load_wfrag(pk(i * 6 + 0, 1), nullptr, 0, NT, tid);
    __syncthreads();
    // ---- C3: dq = dS k * qscale -> rows of DO (do is dead) ; dk += dS^T q (registers)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int mt = mt0 + g_w + 2 * j;
      if (mt < MT) {
        f32x4 acc1[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
        mma_group<1>(acc1, Mat{S_b, SLD}, Mat{TB(Kk), DS}, (mt << 4) + li, 0, (nt_w << 4) + li, k0, (mt + 1) << 4, lq);
        const int c = (nt_w << 4) + li;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = (mt << 4) + (lq << 2) + e;
          *((c < D && r >= SH) ? &TB(DO)[r * DS + c] : dummy + c) = acc1[0][e] * qscale;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kt = mt0 + g_w + 2 * j;
      if (kt < MT) {
        f32x4 acc1[1] = {dk_acc[j]};
        const int kq0 = imax(kt << 4, k0);
        mma_group<1>(acc1, MatT{S_b, SLD}, Mat{TB(Q), DS}, (kt << 4) + li, 0, (nt_w << 4) + li, kq0, LP, lq);
        dk_acc[j] = acc1[0];
      }
    }
    __syncthreads();
    // ---- A3: dv -> DV (= v's slot), dk -> DKm (= k's slot) ; x -> Xb (= S's slot) ; dLN1 = dh1 + dq Wq (in place in H)
    lds_f *DQ = DO, *DV = V, *DKm = Kk, *Xb = S, *DX = Q;
    RG_RELANE();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kt = mt0 + g_w + 2 * j;
      if (kt < MT) {
        const int c = (nt_w << 4) + li;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = (kt << 4) + (lq << 2) + e;
          const bool ok = r >= SH && c < D;
          *(ok ? &TB(DV)[r * DS + c] : dummy + c) = dv_acc[j][e] * keep_scale;
          *(ok ? &TB(DKm)[r * DS + c] : dummy + c) = dk_acc[j][e];
        }
      }
    }
    const SlabWB sl_wq{slab, o.in_w, o.in_b, D, D, rmw};
    const SlabWB sl_wk{slab, o.in_w + D * D, o.in_b + D, D, D, rmw};
    const SlabWB sl_wv{slab, o.in_w + 2 * D * D, o.in_b + 2 * D, D, D, rmw};
    g_x.store(Xb + p0 * DS, DS, L - p0, D, nthr);
    zero_pad_rows(Xb);
    ones_col(Xb);
    const WFrag wkn = load_wfrag(pk(i * 6 + 1, 1), nullptr, 0, NT, tid);
    rag_packed(mt0, mtn, DK >> 2, D, Mat{TB(DQ), DS}, wqn, [&](int r, int c) { return TB(H)[r * DS + c]; },
               [&](int r, int c, float v, float old) { *(r >= SH ? &TB(H)[r * DS + c] : dummy + c) = old + v; }, lane, wave);
    const WFrag wvn = load_wfrag(pk(i * 6 + 2, 1), nullptr, 0, NT, tid);
    __syncthreads();
    // ---- A4: dx = dk Wk + dv Wv -> DX (= q's slot) ; dWk += dk^T x ; dWv += dv^T x
    {
      SlabPre pre_wk = RMW_ ? slab_preload(nw, NT, NT, sl_wk) : SlabPre{};
      SlabPre pre_wv = RMW_ ? slab_preload(nw, NT, NT, sl_wv) : SlabPre{};
      rag_packed2(mt0, mtn, DK >> 2, D, Mat{TB(DKm), DS}, wkn, Mat{TB(DV), DS}, wvn, NoPre{},
                  [&](int r, int c, float v, float) { *(r >= SH ? &TB(DX)[r * DS + c] : dummy + c) = v; }, lane, wave);
      if (RMW_) { slab_ready(pre_wk); slab_ready(pre_wv); }
      slab_gemm(k0, MatT{TB(DKm), DS}, Mat{TB(Xb), DS}, sl_wk, pre_wk);
      slab_gemm(k0, MatT{TB(DV), DS}, Mat{TB(Xb), DS}, sl_wv, pre_wv);
    }
    if (i > 0) {                               // the next block's FFN checkpoints
      g_h1.load(a.c_save_h1 + h1_off(i - 1, b, ly.n_blocks, L, D) + p0 * D, L - p0, D, nthr);
      g_r.load(a.c_save_aux + aux_off(i - 1, b, ly.n_blocks, L, LP, D).r + p0 * D, L - p0, D, nthr);
    }
    __syncthreads();
    // ---- A5: LN1(x) -> N1 (= dk's slot)                                              (DKm, DV free)
    lds_f* N1 = DKm;
    ln_rows(nw, Xb + p0 * DS, N1 + p0 * DS, L - p0, DS, D, s_ln + (4 * i + 0) * 64, s_ln + (4 * i + 1) * 64);
    zero_pad_rows(N1);
    ones_col(N1);
    __syncthreads();
    // ---- A6: dWq += dq^T LN1(x) ; LN1 backward: DX += dx(dLN1), g * xhat -> GX1 (= dv's slot)
    lds_f* GX1 = DV;
    {
      SlabPre pre_wq = RMW_ ? slab_preload(nw, NT, NT, sl_wq) : SlabPre{};
      ln_bwd_rows<true>(nw, H + p0 * DS, Xb + p0 * DS, DX + p0 * DS, GX1 + p0 * DS, L - p0, R - p0, DS, D, s_ln + (4 * i + 0) * 64);
      slab_gemm(k0, MatT{TB(DQ), DS}, Mat{TB(N1), DS}, sl_wq, pre_wq);
    }
    __syncthreads();
    // ---- A7: column sums (dbeta1 from dLN1 = H, dgamma1 from GX1)
    col_sums(k0, TB(H), s_lng + (4 * i + 1) * 64, D);
    col_sums(k0, TB(GX1), s_lng + (4 * i + 0) * 64, D);
    __syncthreads();
    // next block: G = DX; everything else is free
    G = DX;
    fr[0] = H; fr[1] = GX1; fr[2] = Xb; fr[3] = N1; fr[4] = DQ;
  }

  // ---- embedding backward: item rows (atomics), position table, side channel      (positions p0 .. : pads carry keep = 0)
  RG_RELANE();
  {
    const DropSite dsE = drop_site(drop_on && is_sas, seed, SITE_EMB, seq, a.drop_thr, a.drop_scale);
    {
      int t = p0 + tid / di, c = tid - (tid / di) * di;
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
      if (a.contrib != nullptr)
        for (int idx = tid; idx < p0 * di; idx += nthr) a.contrib[(((int64_t)2 * B + b) * L) * di + idx] = 0.f;
    }
    if (has_fake)
      side_sums(2 * dfk, [&](int p, int t) {
        constexpr int dq = dfk > 0 ? dfk : 1;
        const int f = 1 + p / dq, c = p - (f - 1) * dq;
        return s_fk[t] == f ? G[t * DS + di + c] * s_keep[t] : 0.f;
      }, [&](int p) { return ly.off_side + dfk + p; }, p0);
    if (is_srfu) {
      const int lab = ((lds_i*)s_misc)[0];
      side_sums(D, [&](int c, int t) { return G[t * DS + c] * s_keep[t]; }, [&](int c) { return ly.off_side + lab * D + c; }, p0);
    }
  }
  __syncthreads();
  // LayerNorm parameter gradients of the sequences this workgroup has walked so far: LDS accumulators -> slab (the running
  // sums after every sequence: the last write stands)
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
  __syncthreads();
#undef TB
#undef RG_RELANE
}

// Between rag_fwd_seq<.., SEAM_> and rag_bwd_seq<.., SEAM_> of one sequence (the train kernel; a workgroup barrier on either
// side): every word of the working set (W floats) gets the value the backward's own first phase would have left in a
// zeroed one, except the rows the forward hands over, which stay:
//   * slot 0 (sX): rows p0 .. L - 1, columns < D - the last block's output, position-indexed at this very address.  The
//     forward left score data in its columns D .. DS - 1 and in rows L, L + 1: the ones column, zeros; rows in front of p0
//     (the head's rows ph0 .. p0 - 1 among them) are zeros, as a pad's row is;
//   * slot kRagSeamG (sG): rows ph0 .. L - 1, columns < d_out - d hidden, written by the forward's last pass;
//   * the nine per-position arrays (rag_bwd_seq's first nine, in its order) from hs, whole.
// So each word has one writer here, and the backward reads what a launch of its own would read.
template <int K_, int DI_>
__device__ __forceinline__ void rag_seam_handoff(const RagBwdLds& m, const RagSeam& hs, int W, int tid) {
  constexpr int nthr = 512, L = 50, D = 50, LP = 64, DS = 54, R = 52, SZ = R * DS, SH = kRagSH;
  constexpr int dout = (K_ == SRFRD_SRFR) ? DI_ : D;
  constexpr int oX = SH * DS, oG = oX + kRagSeamG * SZ, oT = oX + 6 * SZ, nT = kHeadRows * LP;
  lds_f* base = m.base;
  const int krp = hs.t0 >= 1 ? hs.t0 - 1 : 0;
  const int r0 = ((krp + SH) >> 4) << 4;
  const int p0 = r0 > SH ? r0 - SH : 0;
  const int ph0 = rag_head_range(hs.th, krp).pos0;
  auto zero = [&](int lo, int hi) {
    for (int i = lo + tid; i < hi; i += nthr) base[i] = 0.f;
  };
  zero(0, oX);
  zero(oX + SZ, oG);
  zero(oG + SZ, oT);
  zero(oT + nT, W);
  {                                      // the two slots with rows that stay: eight rows x 64 columns per pass, no division
    const int c = tid & 63;
    if (c < DS)
      for (int r = tid >> 6; r < R; r += nthr >> 6) {
        if (!(r >= p0 && r < L && c < D)) base[oX + r * DS + c] = (c == D && r < L) ? 1.0f : 0.f;
        if (!(r >= ph0 && r < L && c < dout)) base[oG + r * DS + c] = 0.f;
      }
  }
  if (tid < LP) {
    lds_f* tail = base + oT;
    lds_i* ti = (lds_i*)tail;
    ti[kRowIn * LP + tid] = hs.id;
    tail[kRowKeep * LP + tid] = hs.id != 0 ? 1.f : 0.f;
    ti[kRowPid * LP + tid] = hs.pid;
    ti[kRowNid * LP + tid] = hs.nid;
    ti[kRowFk * LP + tid] = hs.fk;
    ti[kRowPfk * LP + tid] = hs.pfk;
    ti[kRowNfk * LP + tid] = hs.nfk;
    tail[kRowDpl * LP + tid] = hs.dp;
    tail[kRowDnl * LP + tid] = hs.dn;
  }
}

template <int K_, int DI_, bool RMW_>
__global__ void __launch_bounds__(512, 4) encoder_bwd_ragged_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  constexpr int nthr = 512;
  int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const RagT0 t0v = rag_load_t0(a, tid);
  lds_f* base = (lds_f*)smem;
  {
    const int total = (int)bwd_ragged_lds_floats(ly.n_blocks);
    for (int i = tid; i < total; i += nthr) base[i] = 0.f;
  }
  lds_f* s_ln = base + kRagBwdWork;
  const RagBwdLds m{base, s_ln, s_ln + ln_cache_floats(ly.n_blocks)};
  __syncthreads();
  fill_ln_cache(s_ln, a.dense, ly);
  const uint32_t seed = a.seed_dev ? *a.seed_dev : a.seed;
  __syncthreads();

  STAMP_INIT
  for (int iter = 0;; ++iter) {
    const int b = __builtin_amdgcn_readfirstlane(rag_take(a, (lds_i*)(base + kRagSH * 54), iter, tid, t0v));      // (slot 0: free between sequences)
    if (b < 0) break;
    rag_bwd_seq<K_, DI_, RMW_>(a, m, b, iter, tid, wave, seed);
  }
}

}  // namespace SRFRD_NS
