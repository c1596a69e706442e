// Forward for sequences whose first-generation working set does not fit LDS (seq_len > 112: BASELINE configs[4],
// seq_len 200) - inference (MODE_ 0) and training (MODE_ 1): a wave OWNS 16-row token tiles and carries them through a
// block in registers.
//
// The first-generation forward assembles every GEMM output in LDS ([LP][LP] scores included: 175 KB at seq_len 200), so a
// long sequence ran its global-scratch build.  But every per-token operation - LayerNorm, the q / k / v / out
// projections, the residuals, the position-wise FFN - needs only its own row, and attention needs only K and V of the
// sequence.  Here:
//   * shared LDS holds K and V of the current block ([16 MT][54] each: 90 KB at seq_len 200) and nothing else;
//   * wave w owns the row tiles w and MT - 1 - w (causal attention of tile t costs t + 1 key tiles: the pairs cost the
//     same; one tile per wave while there are no more tiles than waves, i.e. up to seq_len 128), keeps their block input x
//     in accumulator layout in registers across blocks, and walks each through
//     LN -> q -> attention -> out-proj -> LN -> FFN with wave-private [16][54] LDS tiles for the accumulator -> A-operand
//     hand-over: two workgroup barriers per block (around the K / V rows), everything else in program order;
//   * the scores are computed TRANSPOSED (S^T = K q^T: key on the accumulator row, query on the lane), so the softmax of a
//     query is a reduction over the lane's own registers plus two cross-lane steps, and the probabilities are already the
//     A operand of P V (k index = the key each register holds; the V fragments are fetched in the same order): neither the
//     scores nor the probabilities ever leave the registers;
//   * LayerNorm runs on the accumulator layout (a row = the 16 lanes of a DPP row).
// last_only (ranking): the last block walks only the tile that holds position L - 1 (K / V still for every tile).
//
// Arithmetic: per-token GEMMs and q k^T use the first generation's k-order and weight fragments (identical products and
// sums); the LayerNorm / softmax reductions and the P V key order differ in association (1e-7 relative).
//
// MODE_ 0: eval-mode hidden states only (no dropout, no checkpoints, no target logits): the ranking forward.
// MODE_ 1: everything srfrd_encoder_fwd offers - dropout at the four sites (same coordinate hash), the backward's
//          checkpoints (the sign-coded probabilities leave the registers as 16-byte row pieces of the [L][LP] block, zeros
//          above the diagonal included), target logits and BCE partial sums: the TRAINING forward of long sequences.
// Scope: hidden width 50, 8 waves, seq_len <= 208.
namespace SRFRD_NS {

// (kRowWaves, kRowMaxTiles, rows_lds_floats: srfrd_enc_common.h, where the kernel plan reads them)

// sum / max over the 16 lanes of a DPP row (= the 16 columns a lane group holds of one accumulator row)
__device__ __forceinline__ float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // lane ^ 1
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // lane ^ 2
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // 7 - lane
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // 15 - lane
  return v;
}

// all four strips of a packed weight matrix (one product form) + the bias of this lane's columns
struct WAll {
  float4 q[4][kPackKC];
  float bias[4];
};
__device__ __forceinline__ WAll load_wall(PackedB b, const float* bias, int nbias, int lane) {
  const int li = lane & 15;
  WAll w;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
    for (int kc = 0; kc < kPackKC; ++kc) w.q[nt][kc] = b.chunk(nt, kc, lane);
    const int c = (nt << 4) + li;
    w.bias[nt] = (bias != nullptr && c < nbias) ? bias[c] : 0.f;
  }
  return w;
}

// acc[nt] = T[16 x K] * W strip nt, K = 4 * KSTEPS; T is this wave's [16][ld] LDS tile (row li, k contiguous)
template <int KSTEPS>
__device__ __forceinline__ void row_gemm(f32x4 (&acc)[4], const lds_f* T, int ld, const WAll& w, int li, int lq) {
  float a[KSTEPS];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) a[s] = T[li * ld + 4 * s + lq];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], w.q[nt][s >> 2][s & 3], acc[nt], 0, 0, 0);
}

template <int D_, int K_, int DI_, int MODE_>
__global__ void __launch_bounds__(kRowWaves * 64) encoder_fwd_rows_kernel(const EncArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const Dims& ly = a.dm;
  constexpr int nw = kRowWaves, nthr = nw * 64;
  constexpr int D = D_, DK = (D + 3) & ~3, DS = DK + 2, KS = DK / 4;
  const int L = a.L, LP = (L + 15) & ~15, MT = LP >> 4;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // The lane index is re-laundered at the head of every sequence, block and tile (RELANE): left alone, LLVM computes every
  // per-lane address of the kernel once (weight fragments of all matrices, gather indices, tile offsets), keeps hundreds
  // of them live, spills them, and then reloads each one in front of the load that needs it - serializing the gathers.
  int lane = tid & 63, li = lane & 15, lq = lane >> 4;
#define RELANE() do { asm volatile("" : "+v"(lane)); li = lane & 15; lq = lane >> 4; } while (0)
  lds_f* sK = (lds_f*)smem;
  lds_f* sV = sK + LP * DS;
  lds_f* T1 = sV + LP * DS + wave * (2 * 16 * DS);
  lds_f* T2 = T1 + 16 * DS;
  lds_f* tail = sV + LP * DS + nw * (2 * 16 * DS);
  lds_i* s_in = (lds_i*)tail;
  lds_f* s_keep = tail + LP;
  lds_i* s_fk = (lds_i*)(tail + 2 * LP);
  lds_i* s_pid = (lds_i*)(tail + 3 * LP);
  lds_i* s_nid = (lds_i*)(tail + 4 * LP);
  lds_f* s_misc = tail + 5 * LP;          // 64 floats
  lds_f* s_ln = s_misc + 64;
  {
    const int total = (int)rows_lds_floats(L, D, ly.n_blocks);
    for (int i = tid; i < total; i += nthr) ((lds_f*)smem)[i] = 0.f;
  }
  __syncthreads();
  fill_ln_cache(s_ln, a.dense, ly);
  const float* P = a.dense;
  const ItemTable table{a.table, a.table16};
  const int kind = K_ >= 0 ? K_ : ly.kind;
  const bool is_sas = kind == SRFRD_SASREC;
  const bool has_fake = kind == SRFRD_SRFR || kind == SRFRD_SRFRN;
  const bool is_srfu = kind >= SRFRD_SRFU_B;
  constexpr int di = DI_, dfk = D_ - DI_;
  constexpr int dout = (K_ == SRFRD_SRFR) ? DI_ : D_;
  const float sqrtD = sqrtf((float)di);
  const float qscale = a.qscale;
  const int B = a.B;
  constexpr bool TR = MODE_ != 0;
  const bool has_pos = TR && a.pos_ids != nullptr, has_neg = TR && a.neg_ids != nullptr;
  const bool drop_on = TR && a.drop_on != 0, do_save = TR && a.save_x != nullptr, do_loss = TR && a.loss_part != nullptr;
  const uint32_t seed = TR ? (a.seed_dev ? *a.seed_dev : a.seed) : 0u;
  auto pk = [&](int mat, int form) {
    return PackedB{reinterpret_cast<const float4*>(a.packed) + ((int64_t)mat * 2 + form) * (kPackFloats / 4)};
  };
  // row tiles of this wave: w alone while there are no more tiles than waves (seq_len <= 128), else w and MT - 1 - w
  const bool single = MT <= nw;
  const int tile0 = wave, tile1 = single ? -1 : MT - 1 - wave;
  const int n_own = single ? (wave < MT ? 1 : 0) : (tile0 > tile1 ? 0 : (tile0 == tile1 ? 1 : 2));
  // LayerNorm over dd columns of rows held in accumulator layout: x[nt][r] <-> (row0 + 4 lq + r, 16 nt + li)
  auto layer_norm = [&](f32x4 (&x)[4], int dd, const lds_f* w, const lds_f* bia) {
    const float invD = 1.0f / (float)dd;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) s += ((nt << 4) + li < dd) ? x[nt][r] : 0.f;
      const float mu = row16_sum(s) * invD;
      float v = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float d = ((nt << 4) + li < dd) ? x[nt][r] - mu : 0.f;
        x[nt][r] = d;
        v += d * d;
      }
      const float rstd = 1.0f / sqrtf(row16_sum(v) * invD + kLnEps);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int c = (nt << 4) + li;
        x[nt][r] = c < dd ? x[nt][r] * rstd * w[c] + bia[c] : 0.f;
      }
    }
  };
  // accumulator-layout rows -> a [16][DS] LDS tile (the A operand of the wave's next GEMM, or K / V rows)
  auto to_tile = [&](lds_f* T, const f32x4 (&x)[4]) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int c = (nt << 4) + li;
      if (c < DS)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[(4 * lq + r) * DS + c] = c < D ? x[nt][r] : 0.f;
    }
  };

  // accumulator-layout rows -> a row-major [L][ldd] global block of this sequence (rows < L, columns < dd)
  auto to_global = [&](float* dst, int ldd, int dd, int row0, const f32x4 (&x)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int R = row0 + 4 * lq + r;
      if (R < L)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int c = (nt << 4) + li;
          if (c < dd) dst[R * ldd + c] = x[nt][r];
        }
    }
  };

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t rowbase = (int64_t)b * L;
    const uint32_t seq = (uint32_t)(a.seq0 + b);
    RELANE();
    __syncthreads();                               // the previous sequence's readers of s_in / s_keep / sK / sV are done
    for (int t = tid; t < LP; t += nthr) {
      const int id = t < L ? clamp_id(a.in_ids[rowbase + t], ly.n_items) : 0;
      s_in[t] = id;
      s_keep[t] = id != 0 ? 1.f : 0.f;
      s_fk[t] = (t < L && a.fk_ids) ? clamp_id(a.fk_ids[rowbase + t], 2) : 0;
      if (TR) {
        s_pid[t] = (t < L && has_pos) ? clamp_id(a.pos_ids[rowbase + t], ly.n_items) : 0;
        s_nid[t] = (t < L && has_neg) ? clamp_id(a.neg_ids[rowbase + t], ly.n_items) : 0;
      }
    }
    if (is_srfu && wave == 0) {
      const int lab = user_label_wave(kind, a.fk_ids ? a.fk_ids + rowbase : nullptr, L, ly.n_labels);
      if (lane == 0) ((lds_i*)s_misc)[0] = lab;
    }
    __syncthreads();

    // ---- embedding (SURVEY 3.4 steps 1-4), straight into the accumulator layout of the owned tiles
    f32x4 xs[2][4];
    {
      const int lab = is_srfu ? ((lds_i*)s_misc)[0] : 0;
      const DropSite dsE = drop_site(drop_on && is_sas, seed, SITE_EMB, seq, a.drop_thr, a.drop_scale);
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const int row0 = (o == 0 ? tile0 : tile1) << 4;
        RELANE();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int R = row0 + 4 * lq + r;
          const int Rc = min(max(R, 0), L - 1);       // (rows >= L and unowned tiles: clamped addresses, zeroed below)
          const int id = s_in[Rc];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int c = (nt << 4) + li;
            float v = 0.f;
            if (c < D && o < n_own) {
              if (has_fake) {
                if (c < di) v = table((int64_t)id * di + c) + P[ly.off_pos + Rc * di + c];
                else v = P[ly.off_side + s_fk[Rc] * dfk + (c - di)];
              } else {
                v = table((int64_t)id * di + c);
                if (is_sas) v *= sqrtD;
                v += P[ly.off_pos + Rc * di + c];
                if (is_srfu) v += P[ly.off_side + lab * D + c];
                if (TR && is_sas) v *= drop_mul(dsE, Rc, c);
              }
              v *= (R < L) ? s_keep[Rc] : 0.f;
            }
            xs[o][nt][r] = v;
          }
        }
        if (do_save && o < n_own) to_global(a.save_x + x_off(0, b, ly.n_blocks, L, D), D, D, row0, xs[o]);
      }
    }

    for (int i = 0; i < ly.n_blocks; ++i) {
      const BlkOff o_ = blk_off(ly.blk0 + i * ly.blk_stride, D);
      const bool last = !TR && a.last_only != 0 && i == ly.n_blocks - 1;
      const AuxOff ax = aux_off(i, b, ly.n_blocks, L, LP, D);
      RELANE();
      // ---- k = x Wk^T + bk, v = x Wv^T + bv -> the shared K / V rows of the owned tiles
      {
        const WAll wk = load_wall(pk(i * 6 + 1, 0), P + o_.in_b + D, D, lane);
        // (weights are always requested BEFORE the checkpoint stores of the step that precedes their use: vmcnt retires in
        // order, so a wait for a load issued behind stores is a wait for the stores' acknowledgement as well)
        const WAll wv = load_wall(pk(i * 6 + 2, 0), P + o_.in_b + 2 * D, D, lane);
        __syncthreads();                           // every wave is done with the previous block's K / V
#pragma unroll
        for (int o = 0; o < 2; ++o)
          if (o < n_own) {
            const int row0 = (o == 0 ? tile0 : tile1) << 4;
            __builtin_amdgcn_wave_barrier();
            to_tile(T1 + o * 16 * DS, xs[o]);       // (T1 and T2 are adjacent: tile o of the pair goes to T1 / T2)
            __builtin_amdgcn_wave_barrier();
            f32x4 acc[4];
            row_gemm<KS>(acc, T1 + o * 16 * DS, DS, wk, li, lq);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[nt][r] += wk.bias[nt];
            to_tile(sK + row0 * DS, acc);
            if (do_save) to_global(a.save_aux + ax.k, D, D, row0, acc);
          }
#pragma unroll
        for (int o = 0; o < 2; ++o)
          if (o < n_own) {
            const int row0 = (o == 0 ? tile0 : tile1) << 4;
            f32x4 acc[4];
            row_gemm<KS>(acc, T1 + o * 16 * DS, DS, wv, li, lq);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[nt][r] += wv.bias[nt];
            to_tile(sV + row0 * DS, acc);
            if (do_save) to_global(a.save_aux + ax.v, D, D, row0, acc);
          }
        __syncthreads();                           // K, V of every row are in place
      }
      // ---- the owned tiles, one after the other: LN1 -> q -> attention -> out-proj -> LN2 -> FFN
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const int t = o == 0 ? tile0 : tile1;
        if (o >= n_own || (last && t != MT - 1)) continue;
        const int row0 = t << 4;
        f32x4 (&x)[4] = xs[o];
        RELANE();
        WAll w = load_wall(pk(i * 6 + 0, 0), P + o_.in_b, D, lane);          // Wq
        f32x4 n1[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) n1[nt] = x[nt];
        layer_norm(n1, D, s_ln + (4 * i + 0) * 64, s_ln + (4 * i + 1) * 64);
        __builtin_amdgcn_wave_barrier();
        to_tile(T2, n1);
        __builtin_amdgcn_wave_barrier();
        f32x4 acc[4];
        row_gemm<KS>(acc, T2, DS, w, li, lq);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[nt][r] = (acc[nt][r] + w.bias[nt]) * qscale;
        __builtin_amdgcn_wave_barrier();
        to_tile(T2, acc);                          // q
        if (do_save) to_global(a.save_aux + ax.q, D, D, row0, acc);
        __builtin_amdgcn_wave_barrier();
        // ---- S^T = K q^T on the key tiles ct <= t: register r of s[ct] is (key 16 ct + 4 lq + r, query row0 + li)
        {
          f32x4 s[kRowMaxTiles];
          float aq[KS];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) aq[ks] = T2[li * DS + 4 * ks + lq];
#pragma unroll
          for (int ct = 0; ct < kRowMaxTiles; ++ct) {
            s[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ct <= t) {
              float bk[KS];
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) bk[ks] = sK[((ct << 4) + li) * DS + 4 * ks + lq];
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) s[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(bk[ks], aq[ks], s[ct], 0, 0, 0);
            }
          }
          // causal softmax of query R = row0 + li over its keys j <= R (registers of this lane and of lanes li + 16 lq')
          const int R = row0 + li;
          // key-padding mask (srfrd_layout::flags): the leading pads, counted from the pad mask of the id load; a pad query
          // row keeps its keys (finite, masked to zero behind the FFN)
          const int kt0 = (ly.flags & SRFRD_LAYOUT_MASK_PAD_KEYS) ? first_live(s_keep, L) : 0;
          const int klo = R >= kt0 ? kt0 : 0;      // first key of the row
          float m = -INFINITY;
#pragma unroll
          for (int ct = 0; ct < kRowMaxTiles; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int j = (ct << 4) + (lq << 2) + r;
              const bool on = ct <= t && j >= klo && j <= R;
              s[ct][r] = on ? s[ct][r] : -INFINITY;
              m = fmaxf(m, s[ct][r]);
            }
          m = fmaxf(m, __shfl_xor(m, 16, 64));
          m = fmaxf(m, __shfl_xor(m, 32, 64));
          float sum = 0.f;
#pragma unroll
          for (int ct = 0; ct < kRowMaxTiles; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float e = s[ct][r] == -INFINITY ? 0.f : __expf(s[ct][r] - m);
              s[ct][r] = e;
              sum += e;
            }
          sum += __shfl_xor(sum, 16, 64);
          sum += __shfl_xor(sum, 32, 64);
          const float inv = 1.0f / sum;
          if (TR) {
            // probabilities, attention dropout and the backward's checkpoint: a lane holds four consecutive keys of its query
            // per key tile - one 16-byte store into row R of the [L][LP] block, sign-coded with the mask (dropped = negated);
            // the tiles above the diagonal are written as zeros (the backward reads whole rows)
            const DropSite dsA = drop_site(drop_on, seed, site_attn(i), seq, a.drop_thr, a.drop_scale);
            float* prow = do_save ? a.save_aux + ax.p + (int64_t)R * LP + (lq << 2) : nullptr;
#pragma unroll
            for (int ct = 0; ct < kRowMaxTiles; ++ct) {
              float4 pv = {0.f, 0.f, 0.f, 0.f};
              if (ct <= t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const float p = s[ct][r] * inv;
                  const float mul = drop_mul(dsA, R, (ct << 4) + (lq << 2) + r);
                  (&pv.x)[r] = mul != 0.f ? p : -p;
                  s[ct][r] = p * mul;
                }
              }
              if (do_save && R < L && (ct << 4) < LP) {
                if ((L & 1) == 0) *reinterpret_cast<float4*>(prow + (ct << 4)) = pv;      // (16-byte aligned iff L is even)
                else { prow[(ct << 4) + 0] = pv.x; prow[(ct << 4) + 1] = pv.y; prow[(ct << 4) + 2] = pv.z; prow[(ct << 4) + 3] = pv.w; }
              }
            }
          }
          RELANE();
          w = load_wall(pk(i * 6 + 3, 0), P + o_.out_b, D, lane);             // Wo: in flight under P v (requested only now: the
                                                                        // 64 fragment registers would not fit beside the scores' GEMM)
          // ---- o = P v: k-step (ct, r) takes P(query li, key 16 ct + 4 lq + r) from the lane's own register
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ct = 0; ct < kRowMaxTiles; ++ct)
            if (ct <= t) {
              float bv[4][4];
#pragma unroll
              for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) bv[r][nt] = sV[((ct << 4) + (lq << 2) + r) * DS + (nt << 4) + li];
#pragma unroll
              for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                  acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(TR ? s[ct][r] : s[ct][r] * inv, bv[r][nt], acc[nt], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();
        to_tile(T1, acc);                          // o
        if (do_save) to_global(a.save_aux + ax.o, D, D, row0, acc);
        __builtin_amdgcn_wave_barrier();
        // ---- h1 = n1 + (o Wo^T + bo); n2 = LN2(h1)
        row_gemm<KS>(acc, T1, DS, w, li, lq);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) n1[nt][r] = ((nt << 4) + li < D) ? n1[nt][r] + acc[nt][r] + w.bias[nt] : 0.f;
        RELANE();
        w = load_wall(pk(i * 6 + 4, 0), P + o_.c1_b, D, lane);                // W1
        if (do_save) to_global(a.save_h1 + h1_off(i, b, ly.n_blocks, L, D), D, D, row0, n1);
        layer_norm(n1, D, s_ln + (4 * i + 2) * 64, s_ln + (4 * i + 3) * 64);          // n2
        __builtin_amdgcn_wave_barrier();
        to_tile(T2, n1);
        __builtin_amdgcn_wave_barrier();
        // ---- PW-FFN: r = relu(drop1(n2 W1^T + b1)) ; y = (drop2(r W2^T + b2) + n2) * keep
        const DropSite ds1 = drop_site(drop_on, seed, site_ffn1(i), seq, a.drop_thr, a.drop_scale);
        const DropSite ds2 = drop_site(drop_on, seed, site_ffn2(i), seq, a.drop_thr, a.drop_scale);
        row_gemm<KS>(acc, T2, DS, w, li, lq);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float h = acc[nt][r] + w.bias[nt];
            if (TR) h *= drop_mul(ds1, row0 + 4 * lq + r, (nt << 4) + li);
            acc[nt][r] = ((nt << 4) + li < D) ? fmaxf(h, 0.f) : 0.f;
          }
        RELANE();
        w = load_wall(pk(i * 6 + 5, 0), P + o_.c2_b, D, lane);                // W2
        if (do_save) to_global(a.save_aux + ax.r, D, D, row0, acc);
        __builtin_amdgcn_wave_barrier();
        to_tile(T1, acc);
        __builtin_amdgcn_wave_barrier();
        row_gemm<KS>(acc, T1, DS, w, li, lq);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int Rr = min(row0 + 4 * lq + r, LP - 1);
          const float keep = s_keep[Rr];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int c = (nt << 4) + li;
            float y = acc[nt][r] + w.bias[nt];
            if (TR) y *= drop_mul(ds2, row0 + 4 * lq + r, c);
            x[nt][r] = c < D ? (y + n1[nt][r]) * keep : 0.f;
          }
        }
        if (do_save) to_global(a.save_x + x_off(i + 1, b, ly.n_blocks, L, D), D, D, row0, x);
      }
    }

    // ---- head: (last_conv) -> last LayerNorm -> hidden (all rows, or position L - 1 only), target logits, BCE partial sums
    float lsum[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int t = o == 0 ? tile0 : tile1;
      if (o >= n_own || (a.last_only != 0 && t != MT - 1)) continue;
      const int row0 = t << 4;
      f32x4 (&x)[4] = xs[o];
      if (K_ == SRFRD_SRFR) {
        const WAll wl = load_wall(pk(ly.n_blocks * 6, 0), P + ly.off_lc_b, di, lane);
        __builtin_amdgcn_wave_barrier();
        to_tile(T1, x);
        __builtin_amdgcn_wave_barrier();
        f32x4 acc[4];
        row_gemm<KS>(acc, T1, DS, wl, li, lq);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) x[nt][r] = ((nt << 4) + li < di) ? acc[nt][r] + wl.bias[nt] : 0.f;
      }
      layer_norm(x, dout, s_ln + (4 * ly.n_blocks) * 64, s_ln + (4 * ly.n_blocks + 1) * 64);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int R = row0 + 4 * lq + r;
        if (a.last_only != 0 ? R == L - 1 : R < L)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int c = (nt << 4) + li;
            if (c < dout) a.hidden[(a.last_only != 0 ? (int64_t)b : rowbase + R) * dout + c] = x[nt][r];
          }
      }
      if (TR && (has_pos || has_neg)) {
        // target logits: row dot products against the gathered item rows (a row = the 16 lanes of a DPP row x 4 strips)
        const bool srfrn = kind == SRFRD_SRFRN;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int R = row0 + 4 * lq + r;
          const int Rc = min(R, L - 1);
          const int pid = s_pid[Rc], nid = s_nid[Rc];
          float ap = 0.f, an = 0.f;
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int c = (nt << 4) + li;
            if (c < dout) {
              const float h = x[nt][r];
              if (has_pos) ap += h * (c < di ? table((int64_t)pid * di + c)
                                             : (srfrn ? P[ly.off_side + clamp_id(a.pos_fk[rowbase + Rc], 2) * dfk + (c - di)] : 0.f));
              if (has_neg) an += h * (c < di ? table((int64_t)nid * di + c)
                                             : (srfrn ? P[ly.off_side + clamp_id(a.neg_fk[rowbase + Rc], 2) * dfk + (c - di)] : 0.f));
            }
          }
          const float pl = row16_sum(ap), nl = row16_sum(an);
          if (li == 0 && R < L) {
            if (has_pos) a.pos_logits[rowbase + R] = pl;
            if (has_neg) a.neg_logits[rowbase + R] = nl;
            if (do_loss && pid != 0) {               // trainer.py:36-38: both terms indexed by pos != 0
              lsum[0] += softplus_f(-pl);
              lsum[1] += softplus_f(nl);
              lsum[2] += 1.f;
            }
          }
        }
      }
    }
    if (do_loss) {
#pragma unroll
      for (int k = 0; k < 3; ++k) lsum[k] = wave_sum(lsum[k]);
      if (lane == 0) {
        s_misc[8 + wave * 3 + 0] = lsum[0];
        s_misc[8 + wave * 3 + 1] = lsum[1];
        s_misc[8 + wave * 3 + 2] = lsum[2];
      }
      __syncthreads();
      if (tid < 3) {
        float sacc = 0.f;
        for (int w = 0; w < nw; ++w) sacc += s_misc[8 + w * 3 + tid];
        a.loss_part[(int64_t)b * 3 + tid] = sacc;
      }
    }
  }
}

#undef RELANE

}  // namespace SRFRD_NS
