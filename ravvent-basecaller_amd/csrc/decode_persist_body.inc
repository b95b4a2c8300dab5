// The body of the persistent decode's kernels (decode.hip: k_dec_persist, k_dec_persist_1p, k_dec_persist_gru), included inside each of
// them.  In scope at the point of inclusion: the kernel's arguments (d, Wcat, Wtok, bdec, Wcat1, bdec1, Nh) and the compile-time W, NIT,
// D, ATT, NT and T = PersistTraits<...>, whose PARTS says how many f16 parts a weight of the Wc16 / Wl16 fragments has and whose GRU
// says that the one cell is a GRU (the gate phase alone differs: the four gate tiles of the cell product are then z, r and the two
// halves of the candidate, and `cS` holds h).
  extern __shared__ __align__(16) float dsm[];
  const PersistLds L(W, D, ATT, T::PARTS);
  _Float16* xim = reinterpret_cast<_Float16*>(dsm + L.xim);   // MXC only
  float* pqs = dsm + L.pq;  float* vat = dsm + L.vat;   // ATT == 1 only
  float* wcache = dsm + L.wcache;                        // CACHE only: rows 72 g + 104 + i of Wcat at [(8 g + i) * 512], g = 0..2
  float* attT = dsm + L.attT;  float* zb = dsm + L.zb;  float* cS = dsm + L.cS;
  float* qp = dsm + L.qp;  float* part = dsm + L.part;  float* ctxp = dsm + L.ctxp;  float* hcT = dsm + L.hcT;  float* att = dsm + L.att;
  float* ml = dsm + L.ml;  float* mg = dsm + L.mg;  float* lg = dsm + L.lg;  float* fold = dsm + L.fold;
  float* h0T = dsm + L.h0T;  float* cS1 = dsm + L.cS1;  float* b1s = dsm + L.b1s;  float* partU = ctxp;   // D == 2 only (FMA form: spans ctxp + fold)
  // (the matrix-pipe form takes the output layer from the Wl16 fragments: it only needs the bias here, and neither `qp` nor `att`)
  __shared__ __align__(16) float s_wfc[(T::MXC ? 0 : RV_MAX_VOCAB * T::FCW) + RV_MAX_VOCAB];
  __shared__ __align__(16) float s_nh[(D == 1 && !T::MXC) ? RV_MAX_VOCAB * T::FCW : 4];
  __shared__ float s_lprob[WB];
  __shared__ int s_fin[WB], s_len[WB], s_parent[WB], s_tok[WB], s_allfin;
  // moves: the call's records pointer and split index, parked here by the prologue.  Read from the kernel arguments inside the step
  // loop they would be hoisted and hold three more scalar registers through it, which the forms at the edge of the register file pay
  // for in spilled lanes; an LDS read per step holds none
  __shared__ float* s_moves;
  __shared__ int s_movesTr;
  __shared__ int s_qbig;                   // Bahdanau on the matrix pipe: some processed query of this step lies outside the fast form's range

  const int b = blockIdx.x, tid = threadIdx.x, Tm = d.Tm, V = d.V;
  const int lane = tid & 63, sub = lane & 15, sid = tid >> 4;
  const size_t row0 = (size_t)b * W;
  const int steps = d.L - 1;

  const int half = sub >> 3, s8 = sub & 7;
  float4 kr[T::MXS ? 1 : T::NP][4], ur[T::MX ? 1 : NIT][2];
  float4 kb[T::MXS ? T::NTT : 1][4][2], ub[T::MX ? NIT : 1][2];
  unsigned livebits = 0;
  // the default form projects its chunk's memory itself when the call hands it enc_out (persist_project_memory); d.values is unused then
  bool fused = false;
  if constexpr (T::FUSE) {
    fused = d.enc_rows != nullptr;
    if (fused) persist_project_memory<NIT>(d, b, dsm, kb, ub, livebits);
  }
  if (!fused) {
    if constexpr (T::MXS) persist_load_keys_mx<T>(d, b, tid, kb, livebits);
    if constexpr (T::MX) {     // (inline) U' as B fragments: wave wv0 owns units 16 wv0 .. + 15
      const float* cbase = d.values + (size_t)b * Tm * RV_E;
      const int l16 = lane & 15, kq = lane >> 4, wv0 = tid >> 6;
#pragma unroll
      for (int ks = 0; ks < NIT; ++ks) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = cbase[(size_t)min(32 * ks + 8 * kq + j, Tm - 1) * RV_E + RV_U + 16 * wv0 + l16];
        split_f16x8(v, d.mx_uscale, ub[ks][0], ub[ks][1]);
      }
    }
  }
  // ---- (inline) forms that score on fp32 key rows.  Keys: the 16
  //      lanes of a stream hold TWO rows at a time, lanes 0-7 row sid + 32 (2p), lanes 8-15 row sid + 32 (2p + 1), 16 columns each, so
  //      that a score is an 8-lane reduction and one pass over the registers scores two rows.  U' (the context side, unless it sits
  //      on the matrix pipe): every lane 8 columns of each of the stream's rows.
  if constexpr (!T::MXS) {
    const float* cbase = d.values + (size_t)b * Tm * RV_E;
    const uint8_t* mrow = d.mask + (size_t)b * Tm;
#pragma unroll
    for (int p = 0; p < T::NP; ++p) {
      const int tc = min(sid + 32 * (2 * p + half), Tm - 1);
      const float* q = cbase + (size_t)tc * RV_E + 16 * s8;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        kr[p][m] = *reinterpret_cast<const float4*>(q + 4 * m);
        if (T::BAH) {   // Bahdanau: tanh(k + pq) = 1 - 2 / (1 + exp2((k + pq) * 2 log2 e)): the keys carry the factor from here on
          kr[p][m].x *= 2.0f * LOG2E; kr[p][m].y *= 2.0f * LOG2E; kr[p][m].z *= 2.0f * LOG2E; kr[p][m].w *= 2.0f * LOG2E;
        }
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int t = sid + 32 * it, tc = min(t, Tm - 1);
      if constexpr (!T::MX) {
        const float* q = cbase + (size_t)tc * RV_E + RV_U + 4 * sub;
#pragma unroll
        for (int m = 0; m < 2; ++m) ur[it][m] = *reinterpret_cast<const float4*>(q + 64 * m);
      }
      if (t < Tm && mrow[tc]) livebits |= 1u << it;       // _maybe_mask_score: padded steps never score
    }
  }
  bool kbig = false;
  if constexpr (T::BAH && T::MXC) {          // Bahdanau beside the matrix pipe: the resident keys k' become E_k = 2^k' unless one of the chunk is out of range
    kbig = __syncthreads_or(persist_keys_out_of_range<T>(kr) ? 1 : 0) != 0;
    if (!kbig) persist_keys_to_exp2<T>(kr);
  }
  // ---- decoder initial state: zeros; start tokens; log_probs = [0, -inf, ...] (SURVEY.md A.5)
  // The cell's matrix-vector product of a step is taken on the PREVIOUS step's beams, before they are re-ordered (it only
  // needs their attention vector and h); the gate math then picks up the partial sums and the cell state of its parent
  // beam.  Zero initial state: partial sums 0, parents = identity.
  if (!T::MXC) {
    for (int i = tid; i < RV_U * WB; i += NT) attT[i] = 0.f;
    for (int i = tid; i < RV_U * WB; i += NT) hcT[i] = 0.f;
  }
  for (int i = tid; i < 2 * W * RV_U; i += NT) cS[i] = 0.f;
  for (int i = tid; i < (T::MXC ? W * T::ZS : 4 * W * RV_G); i += NT) part[i] = 0.f;
  if (T::MXC) for (int i = tid; i < (T::MXC2 ? 3072 : 2048); i += NT) dsm[L.xim + i] = 0.f;
  if (D > 1) {
    if (!T::MXC) for (int i = tid; i < RV_U * WB; i += NT) h0T[i] = 0.f;
    for (int i = tid; i < 2 * W * RV_U; i += NT) cS1[i] = 0.f;
    for (int i = tid; i < (T::MXC ? W * T::ZS : 3 * W * RV_G); i += NT) partU[i] = 0.f;
    b1s[tid] = bdec1[tid];
  }
  if (!T::MXC) {
    for (int i = tid; i < RV_U * V; i += NT) s_wfc[(i % V) * T::FCW + i / V] = d.W_fc[i];
    if (D == 1) for (int i = tid; i < RV_U * V; i += NT) s_nh[(i % V) * T::FCW + i / V] = Nh[i] * (1.0f / LOG2E);   // applied to qp = h * log2(e), the row-major copy of h
  }
  if (tid < V) s_wfc[T::BFC + tid] = d.b_fc[tid];
  if (T::MXC) {   // the output layer's fragments
    const uint4* src = reinterpret_cast<const uint4*>(d.Wl16);
    uint4* dst = reinterpret_cast<uint4*>(dsm + L.wl16);
    for (int i = tid; i < 8 * T::FR; i += NT) dst[i] = src[i];
  }
  if (T::MXC2) {  // the first MXC2_CACHE of wave 0's end-of-step pairs (cell 0's product, image order)
    const uint4* src = reinterpret_cast<const uint4*>(d.Wc16);
    uint4* dst = reinterpret_cast<uint4*>(wcache);
    for (int i = tid; i < MXC2_CACHE * 128; i += NT) dst[i] = src[i];
  } else if (T::MXC) {   // wave 0's 32 pairs, then the last NC pairs of waves 1-7: 2 KB each, in image order
    const uint4* src = reinterpret_cast<const uint4*>(d.Wc16);
    uint4* dst = reinterpret_cast<uint4*>(wcache);
    for (int i = tid; i < 32 * T::FR; i += NT) dst[i] = src[i];
    if constexpr (T::NC > 0)
      for (int i = tid; i < 7 * T::NC * T::FR; i += NT) dst[32 * T::FR + i] = src[(size_t)((1 + i / (T::NC * T::FR)) * 32 + 32 - T::NC) * T::FR + i % (T::NC * T::FR)];
  } else if (T::CACHE) {
    for (int i = tid; i < 24 * (RV_G / 4); i += NT) {
      const int r = i >> 7, c = i & 127;
      *reinterpret_cast<float4*>(&wcache[r * RV_G + 4 * c]) =
          *reinterpret_cast<const float4*>(Wcat + (size_t)(72 * (r >> 3) + 104 + (r & 7)) * RV_G + 4 * c);
    }
  }
  if (T::BAH && tid < RV_U) vat[tid] = d.v_att[tid] * (-2.0f * LOG2E);   // score = sum_j v_j tanh(.) = const - 2 sum_j v_j / (1 + exp(.)): softmax drops the constant
  if (tid < WB) {
    s_tok[tid] = (W == 1 && d.forced) ? persist_forced_tok(d, b, 0) : d.start_token; s_lprob[tid] = tid == 0 ? 0.f : -INFINITY;
    s_fin[tid] = 0; s_len[tid] = 0; s_parent[tid] = tid;
  }
  if (tid == 0) { s_allfin = 0; s_moves = d.step_moves; s_movesTr = d.Tr; }
  for (int i = tid; i < V * RV_G; i += NT) zb[i] = Wtok[i] + bdec[i & (RV_G - 1)];   // W_dec[one_hot(v)] + b, resident
  if (W == 1 && d.forced) for (int i = tid; i < RV_G; i += NT) zb[V * RV_G + i] = bdec[i];      // row V (V < RV_MAX_VOCAB: ravvent_hip.cpp, persist_form): no input row, persist_forced_tok
  __syncthreads();

  uint4 rbh[T::NR > 0 ? T::NR : 1], rbl[(T::NR > 0 && !T::P1) ? T::NR : 1];       // pairs 32 - NC - NR .. 32 - NC - 1 of this wave, resident for the whole decode
  if constexpr (T::NR > 0) persist_load_resident_pairs<T>(d, tid, rbh, rbl);
  int done_steps = steps;
  const int tid0 = tid;
  for (int step = 0; step < steps; ++step) {
    // Thread coordinates are re-derived from an opaque copy each step: otherwise every LDS / global address
    // of every phase is hoisted out of the loop and the hoisted values spill (the resident rows leave ~70 VGPRs).
    int tid = tid0;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wv = tid >> 6, sub = lane & 15, sid = tid >> 4, row = lane >> 4;
    int mvTr = 0;
    RV_STAMP(d, step, 0);
    if (T::BAH && T::MXC && tid == 0) s_qbig = 0;              // (set again, if at all, after the gates' barrier; last read before this step's last barrier)
    // ================= gates of this step: the cell product was taken at the end of the previous step on the parent beams
    const int cb = step & 1;                             // cell-state buffer holding the previous step's states
    // The chunk's resident rows are [keys | U'] = values . [W_mem | A_c] (A_c = the attention layer's context rows), built once
    // per slab by a GEMM: score_t = keys_t . h as in the reference (128-wide, no q' = W_mem h product per step), and the
    // attention vector = h . A_h + ctx' with ctx' = sum_t alpha_t U'_t (the context never has to pass through the attention
    // layer).  With ONE decoder cell the h part is folded into the weights at load time as well: the cell product of the
    // next step is [ctx' | h] . [W_a ; U + A_h W_a] and the logits are ctx' . W_fc + h . (A_h W_fc) + b, so no attention-layer
    // product is left in the step.  With two cells (cell 0 would need h_1 as a third input block) h . A_h stays explicit.
    float4 pw[8];                      // D == 2: this thread's whole slice of A_h = W_att[0:128] (8 rows x 4 columns), requested before the gate math
    auto ah_prefetch = [&]() {
      const float* wa = d.W_att + (size_t)(8 * (tid >> 5)) * RV_U + 4 * (tid & 31);
#pragma unroll
      for (int u = 0; u < 8; ++u) pw[u] = *reinterpret_cast<const float4*>(wa + (size_t)u * RV_U);
    };
    auto wq_prefetch = [&]() {           // ATT: this thread's slice of W_q (8 rows x 4 columns), requested before the gate math
      const float* wq = d.W_q + (size_t)(8 * (tid >> 5)) * RV_U + 4 * (tid & 31);
#pragma unroll
      for (int u = 0; u < 8; ++u) pw[u] = *reinterpret_cast<const float4*>(wq + (size_t)u * RV_U);
    };
    // Bahdanau + matrix pipe: this wave's B fragments of W_q (its 16 columns, K = 128: 4 k-steps x 2 parts), requested before the gate math
    uint4 wqf[(T::BAH && T::MXC) ? 8 : 1];
    if constexpr (T::BAH && T::MXC) {
      const uint4* wq = reinterpret_cast<const uint4*>(d.Wq16) + (size_t)wv * (8 * 64) + lane;
#pragma unroll
      for (int j = 0; j < 8; ++j) wqf[j] = wq[j * 64];
    } else if (T::BAH) wq_prefetch();
    if constexpr (T::MXC) {
      // W * 128 (beam, unit) items on 512 threads: waves 0-1 take two (W = 5).  Both items' operands are read first, then both are
      // computed, then stored: the second item rides in the first one's LDS and transcendental latencies instead of doubling the phase.
      // CELL 0: z = the end-of-step product of the PARENT beam + the token's row; CELL 1 (two cells): z = h_0 . W_1 of this beam (taken
      // right before) + h_1 . U_1 of the parent beam (end of the previous step) + b_1.  h goes to its segment of the A-fragment image:
      // one cell [ctx' | h]; two cells [ctx' | h_1 | h_0]; the top cell's h is the score query as well.
      auto mxc_gates = [&](auto cell_tag) {
        constexpr int CELL = decltype(cell_tag)::value;
        constexpr bool TOP = CELL == D - 1;
        constexpr int NITEM = (W * RV_U + NT - 1) / NT;
        float* cst = CELL == 0 ? cS : cS1;
        float z4[NITEM][4], cp[NITEM];
        bool ok[NITEM];
#pragma unroll
        for (int it = 0; it < NITEM; ++it) {
          const int idx = tid + it * NT;
          ok[it] = idx < W * RV_U;                             // wave-uniform (128 items per beam, 64 lanes per wave)
          const int w = ok[it] ? idx >> 7 : 0, u = idx & 127, pb = s_parent[w], tk = s_tok[w];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            if constexpr (T::GRU && NITEM == 1) continue;      // (a GRU thread with one item reads each operand where the gate math uses it)
            if constexpr (CELL == 0) z4[it][g] = part[pb * T::ZS + g * RV_U + u] + zb[tk * RV_G + g * RV_U + u];
            else z4[it][g] = (part[w * T::ZS + g * RV_U + u] + partU[pb * T::ZS + g * RV_U + u]) + b1s[g * RV_U + u];
          }
          if constexpr (!T::GRU || W > 5) cp[it] = cst[cb * W * RV_U + pb * RV_U + u];
        }
#pragma unroll
        for (int it = 0; it < NITEM; ++it) {
          if (!ok[it]) continue;
          const int idx = tid + it * NT, w = idx >> 7, u = idx & 127;
          float c2, hh;
          if constexpr (T::GRU) {
            // Keras GRU cell, reset_after: the tiles are z, r, candidate-input, candidate-recurrent (the last with b[1]_h from its token-table
            // row, so that the reset gate multiplies h . U_h + b[1]_h whole); hp = the parent's h, the cell's one state, kept in fp32 in `cS`.
            // The candidate first, then z and hp.  Up to W = 5 (at most waves 0-1 carry a second item) hp is read here, as late as its use,
            // and a thread with one item reads its tiles here too: the Bahdanau forms hold W_q's fragments across this phase, and with
            // the LSTM's order of reads k_dec_persist_gru<4,8,4> and <5,8,4> spill more than their LSTM forms; wider beams keep that
            // order, under which <7,8,4> spills no more than its LSTM form (tests/test_gru_persist_build.py holds every form to it)
            const int pb = s_parent[w];
            auto zt = [&](int g) {
              if constexpr (NITEM == 1) return part[pb * T::ZS + g * RV_U + u] + zb[s_tok[w] * RV_G + g * RV_U + u];
              else return z4[it][g];
            };
            const float cand = rv_tanh(fmaf(rv_sigmoid(zt(1)), zt(3), zt(2)));
            const float zg = rv_sigmoid(zt(0));
            float hp;
            if constexpr (W > 5) hp = cp[it]; else hp = cst[cb * W * RV_U + pb * RV_U + u];
            hh = fmaf(zg, hp - cand, cand);                    // z h + (1 - z) hh
            c2 = hh;
          } else {
            c2 = fmaf(rv_sigmoid(z4[it][1]), cp[it], rv_sigmoid(z4[it][0]) * rv_tanh(z4[it][2]));
            hh = rv_sigmoid(z4[it][3]) * rv_tanh(c2);
          }
          cst[(cb ^ 1) * W * RV_U + idx] = c2;
          {   // h as A fragments: h 2^14 in two f16 parts, k = 128 + u (top cell), 256 + u (cell 0 of two)
            const float sv = hh * 16384.f;
            const _Float16 hi = (_Float16)sv, lo = (_Float16)(sv - (float)hi);
            _Float16* xq = xim + ((((TOP ? 1 : 2) * RV_U + u) >> 3) * 16 + mx_row(w)) * 8 + (u & 7);
            xq[0] = hi; xq[8] = lo;
          }
          if constexpr (T::MXS && TOP) {   // the score query as MFMA A fragments: [k-block u / 8][row mx_row(w) (+ 1: low part)][u % 8] f16 of h log2(e) 2^14
            const float sv = (hh * LOG2E) * 16384.f;
            const _Float16 hi = (_Float16)sv, lo = (_Float16)(sv - (float)hi);
            _Float16* qa = reinterpret_cast<_Float16*>(fold) + ((u >> 3) * 16 + mx_row(w)) * 8 + (u & 7);
            qa[0] = hi; qa[8] = lo;
          }
        }
      };
      mxc_gates(std::integral_constant<int, 0>{});
      if constexpr (T::MXC2) {
        __syncthreads();
        // ---- cell 1's input product z_1a = h_0(new) . W_1 on the matrix pipe: every wave its 16 units x 4 gates, K = 128 (the h_0 segment
        //      of the image: k-steps 8..11), 16 pairs streamed from the W1c16 image through a window of 4; `part` (cell 0's z~, consumed by
        //      the gates above) takes the result, rows = this step's beams
        {
          const int l16 = lane & 15, kq = lane >> 4;
          const uint4* wimg = reinterpret_cast<const uint4*>(d.W1c16) + (size_t)wv * (32 * 128) + lane;
          const _Float16* xa = xim + (kq * 16 + l16) * 8;
          f4v acc[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = f4v{0.f, 0.f, 0.f, 0.f};
          uint4 bh[4], bl[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) { bh[i] = wimg[(2 * i) * 64]; bl[i] = wimg[(2 * i + 1) * 64]; }
#pragma unroll
          for (int p = 0; p < 16; ++p) {
            const h8 a = *reinterpret_cast<const h8*>(xa + (8 + (p >> 2)) * 512);
            acc[p & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, bl[p & 3]), acc[p & 3], 0, 0, 0);
            acc[p & 3] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, bh[p & 3]), acc[p & 3], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (p + 4 < 16) { bh[p & 3] = wimg[(2 * (p + 4)) * 64]; bl[p & 3] = wimg[(2 * (p + 4) + 1) * 64]; }
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < T::NI; ++i)
              if (kq + 4 * i < W) part[(kq + 4 * i) * T::ZS + RV_U * g + 16 * wv + l16] = (acc[g][2 * i] + acc[g][2 * i + 1]) * d.mx_c1descale;
        }
        __syncthreads();
        mxc_gates(std::integral_constant<int, 1>{});
      }
    } else {
      for (int idx = tid; idx < W * RV_U; idx += NT) {       // K-group sums in fixed order, gate math, cell update (SURVEY.md A.1)
        const int w = idx >> 7, u = idx & 127, pb = s_parent[w];
        float z4[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = g * RV_U + u;
          z4[g] = (((part[(0 * W + pb) * RV_G + col] + part[(1 * W + pb) * RV_G + col]) + part[(2 * W + pb) * RV_G + col]) +
                     part[(3 * W + pb) * RV_G + col]) + zb[s_tok[w] * RV_G + col];
        }
        const float c2 = fmaf(rv_sigmoid(z4[1]), cS[cb * W * RV_U + pb * RV_U + u], rv_sigmoid(z4[0]) * dec_gate_tanh<ATT>(z4[2]));
        const float hh = rv_sigmoid(z4[3]) * rv_tanh(c2);
        cS[(cb ^ 1) * W * RV_U + idx] = c2;
        if (D > 1) h0T[u * WB + w] = hh; else { hcT[u * WB + w] = hh; qp[idx] = hh * LOG2E; }
        if constexpr (T::MXS) {     // the score query as MFMA A fragments: [k-block u / 8][row mx_row(w) (+ 1: low part)][u % 8] f16 of h log2(e) 2^14
          const float sv = (hh * LOG2E) * 16384.f;
          const _Float16 hi = (_Float16)sv, lo = (_Float16)(sv - (float)hi);
          _Float16* qa = reinterpret_cast<_Float16*>(fold) + ((u >> 3) * 16 + mx_row(w)) * 8 + (u & 7);
          qa[0] = hi; qa[8] = lo;
        }
      }
    }
    __syncthreads();
    if (D > 1 && !T::MXC) {
      // ---- second cell: z_1 = h_0(new) . W_1 + [h_1(prev) . U_1 of the parent beam, taken at the end of the previous step] + b_1
      {
        const int c4 = tid & 127, kg = tid >> 7;           // 32 rows of W_1 per K group
        f2 acc[W][2];
#pragma unroll
        for (int w = 0; w < W; ++w) { acc[w][0] = f2{0.f, 0.f}; acc[w][1] = f2{0.f, 0.f}; }
        const float* wc = Wcat1 + (size_t)(32 * kg) * RV_G + 4 * c4;
        const float* xk = h0T + (32 * kg) * WB;
#pragma unroll 1
        for (int k0 = 0; k0 < 32; k0 += 8) {
          float4 wr[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) wr[i] = *reinterpret_cast<const float4*>(wc + (size_t)(k0 + i) * RV_G);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 8; ++i) beams_fma_row<W>(acc, wr[i], &xk[(k0 + i) * WB]);
        }
#pragma unroll
        for (int w = 0; w < W; ++w)
          *reinterpret_cast<float4*>(&part[(kg * W + w) * RV_G + 4 * c4]) = make_float4(acc[w][0].x, acc[w][0].y, acc[w][1].x, acc[w][1].y);
      }
      ah_prefetch();
      __syncthreads();
      for (int idx = tid; idx < W * RV_U; idx += NT) {
        const int w = idx >> 7, u = idx & 127, pb = s_parent[w];
        float z4[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = g * RV_U + u;
          const float zin = ((part[(0 * W + w) * RV_G + col] + part[(1 * W + w) * RV_G + col]) + part[(2 * W + w) * RV_G + col]) +
                            part[(3 * W + w) * RV_G + col];
          const float zrec = (partU[(0 * W + pb) * RV_G + col] + partU[(1 * W + pb) * RV_G + col]) + partU[(2 * W + pb) * RV_G + col];
          z4[g] = (zin + zrec) + b1s[col];
        }
        const float c2 = fmaf(rv_sigmoid(z4[1]), cS1[cb * W * RV_U + pb * RV_U + u], rv_sigmoid(z4[0]) * rv_tanh(z4[2]));
        const float hh = rv_sigmoid(z4[3]) * rv_tanh(c2);
        cS1[(cb ^ 1) * W * RV_U + idx] = c2; hcT[u * WB + w] = hh; qp[idx] = hh * LOG2E;
      }
      __syncthreads();
    }
    if constexpr (T::BAH && T::MXC) {
      // ================= Bahdanau: processed query pq = h . W_q (BahdanauAttention.query_layer, no bias) on the matrix pipe: A = the h rows
      //   of the [ctx' | h] image (k-steps 4..7), B = this wave's 16 columns of W_q (Wq16, requested before the gate math): complete in the wave
      const int l16 = lane & 15, kq = lane >> 4;
      const _Float16* xa = xim + (kq * 16 + l16) * 8;
      f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const h8 a = *reinterpret_cast<const h8*>(xa + (4 + ks) * 512);
        a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, wqf[2 * ks]), a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, wqf[2 * ks + 1]), a1, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < T::NI; ++i)
        if (kq + 4 * i < W) {
          const float qv = tile_pair_sum(a0, a1, i) * (d.mx_qdescale * 2.0f * LOG2E);
          pqs[(kq + 4 * i) * RV_U + 16 * wv + l16] = qv;                       // q' ...
          fold[(kq + 4 * i) * RV_U + 16 * wv + l16] = __builtin_amdgcn_exp2f(fminf(fmaxf(qv, -126.f), 126.f));   // ... and E_q = 2^q' (`fold` holds no query image here)
          if (!(fabsf(qv) <= 60.f)) s_qbig = 1;
        }
      __syncthreads();
    } else if (T::BAH) {
      // ================= Bahdanau: processed query pq = h . W_q (BahdanauAttention.query_layer, no bias); thread = (4 columns,
      //   1 of 16 K groups of 8 rows), partial sums through `part` (free between the gates and the context phase)
      persist_h_times_rows<W>(part, hcT, pw, tid);
      __syncthreads();
      for (int i = tid; i < W * RV_U; i += NT) {
        const int w = i >> 7, col = i & 127;
        float s0 = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) s0 += part[(g * W + w) * RV_U + col];
        pqs[i] = s0 * (2.0f * LOG2E);
      }
      __syncthreads();
    }
    RV_STAMP(d, step, 2);
    // ================= (two cells) attention layer, h part: h . A_h ; thread = (4 columns, 1 of 16 K groups of 8 rows), one batch
    if (D > 1 && !T::MXC) persist_h_times_rows<W>(part, hcT, pw, tid);   // (the cell-product partial sums in `part` were consumed by the gates above)
    RV_STAMP(d, step, 3);

    if constexpr (T::MXS) {
      // ================= scores on the matrix pipe: rows = beams, columns = the 16 steps of a tile, K = 128 units.
      //   C/D map: lane l holds column l % 16 and rows 4 g + i (g = l / 16).  Beam w sits in rows mx_row(w), + 1 (its high and its low
      //   part: see mx_row), so that registers 0 + 1 hold beams 0-3 (one per 16-lane group, all 64 lanes busy) and 2 + 3 beams 4-7: the
      //   softmax below touches W <= 4 ? 1 : 2 values per tile.  A row of A only feeds its own row of C, so the rows of absent beams
      //   hold whatever the LDS image holds there, harmlessly.
      const int l16 = lane & 15, kq = lane >> 4;
      float sc[T::NTT][T::NI];
      persist_scores_mx<T>(d, tid, livebits, kb, sc, fold);

      RV_STAMP(d, step, 4);
      // ================= softmax over the chunk's T_m steps: per-wave (max, sum) of every beam, one fixed-order merge
      //   (raw v_exp_f32: arguments <= 0, a result below 2^-126 is an alignment of 0 either way)
      float mrow_[T::NI];
      persist_softmax_wave_mx<T>(tid, sc, mrow_, ml);

      RV_STAMP(d, step, 14);
      __syncthreads();
      RV_STAMP(d, step, 15);
      {
        // merge: lane (beam = lane / 8, wave g = lane % 8) takes one (max, sum) pair; 8-lane butterflies give every lane of the
        // group the beam's maximum and its total (the same instruction sequence in every wave: the same bits in every wave)
        const float mv = ml[(lane & 7) * WB + (lane >> 3)], lv = ml[(8 + (lane & 7)) * WB + (lane >> 3)];
        float Mgl = mv;
        Mgl = fmaxf(Mgl, dpp<0xB1>(Mgl)); Mgl = fmaxf(Mgl, dpp<0x4E>(Mgl)); Mgl = fmaxf(Mgl, dpp<0x141>(Mgl));
        float tl = mv == -INFINITY ? 0.f : lv * __builtin_amdgcn_exp2f(mv - Mgl);
        tl += dpp<0xB1>(tl); tl += dpp<0x4E>(tl); tl += dpp<0x141>(tl);
        // all-masked chunk: 0 / 0 = NaN like the reference
        const float rt = Mgl == -INFINITY ? __int_as_float(0x7fc00000) : __builtin_amdgcn_rcpf(tl);   // (v_rcp_f32: 1 ulp; the IEEE division is a dozen dependent instructions on this phase's critical path)
        // alignments -> A fragments of the context product: [k-block t / 8][row mx_row(beam) (+ 1: low part)][t % 8] f16 of alpha 2^14 (in `part`,
        // idle between the gates and the cell product at the end of the step)
        _Float16* aa = reinterpret_cast<_Float16*>(part);
        float Mg_[T::NI], rr_[T::NI];                                // (both beams' pairs fetched before either is used: one LDS round trip, not two)
#pragma unroll
        for (int i = 0; i < T::NI; ++i) {
          Mg_[i] = __int_as_float(__builtin_amdgcn_ds_bpermute(32 * (kq + 4 * i), __float_as_int(Mgl)));
          rr_[i] = __int_as_float(__builtin_amdgcn_ds_bpermute(32 * (kq + 4 * i), __float_as_int(rt)));
        }
#pragma unroll
        for (int i = 0; i < T::NI; ++i) {
          const int beam = kq + 4 * i;                         // its merged pair sits in lanes 8 beam .. 8 beam + 7
          const float Mg = Mg_[i], rr = rr_[i];
          const bool nanrow = rr != rr && beam < W;
          const float f = (beam >= W || mrow_[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mrow_[i] - Mg) * rr * 16384.f;
#pragma unroll
          for (int c = 0; c < T::NTT; ++c) {
            const int t = 16 * (wv + 8 * c) + l16;
            if (t < 32 * NIT) {
              const float av = nanrow ? rr : sc[c][i] * f;
              const _Float16 hi = (_Float16)av, lo = (_Float16)(av - (float)hi);
              _Float16* q = aa + ((t >> 3) * 16 + mx_row(beam)) * 8 + (t & 7);
              q[0] = hi; q[8] = lo;
            }
          }
        }
      }
      __syncthreads();
      if (d.persist_align) tap_align_image<W, false>(d, part, b, step, tid);
      RV_STAMP(d, step, 5);
    } else {
      // ================= scores from the resident key rows: lane w keeps beam w's score of the even row of a pair, lane 8 + w
      //   that of the odd row
      float sc[T::NP];
#pragma unroll
      for (int p = 0; p < T::NP; ++p) sc[p] = -INFINITY;
      if constexpr (T::BAH && T::MXC) {
        // score_t log2(e) = const + sum_j v'_j / (1 + 2^(k'_tj + q'_j)) (see the resident rows above): MODE 1 = E_k . E_q + 1, one reciprocal;
        // MODE 0 = the chunk kept k' (a key out of range); MODE 2 = this step has a query out of range
        auto bah_scores = [&](auto mode_tag) {
          constexpr int MODE = decltype(mode_tag)::value;
          const float* qsrc = MODE == 1 ? fold : pqs;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            float4 qv[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) qv[m] = *reinterpret_cast<const float4*>(&qsrc[w * RV_U + 16 * s8 + 4 * m]);
#pragma unroll
            for (int p = 0; p < T::NP; ++p) {
              f2 pp = f2{0.f, 0.f};
#pragma unroll
              for (int m = 0; m < 4; ++m) {
                const float4 vv = *reinterpret_cast<const float4*>(&vat[16 * s8 + 4 * m]);
                auto el = [&](float k, float q) -> float {
                  if constexpr (MODE == 1) return __builtin_amdgcn_rcpf(fmaf(k, q, 1.0f));
                  else if constexpr (MODE == 0) return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(k + q));
                  else return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(k) + q));
                };
                const float r0 = el(kr[p][m].x, qv[m].x), r1 = el(kr[p][m].y, qv[m].y), r2 = el(kr[p][m].z, qv[m].z), r3 = el(kr[p][m].w, qv[m].w);
                pp = __builtin_elementwise_fma(f2{vv.x, vv.y}, f2{r0, r1}, pp);
                pp = __builtin_elementwise_fma(f2{vv.z, vv.w}, f2{r2, r3}, pp);
              }
              float sw = pp.x + pp.y;
              sw += dpp<0xB1>(sw); sw += dpp<0x4E>(sw); sw += dpp<0x141>(sw);      // the 8 lanes of this half row
              const int it = 2 * p + half;
              sc[p] = (s8 == w && it < NIT && ((livebits >> it) & 1u)) ? sw : sc[p];
            }
          }
        };
        if (kbig) bah_scores(std::integral_constant<int, 0>{});
        else if (s_qbig) bah_scores(std::integral_constant<int, 2>{});
        else bah_scores(std::integral_constant<int, 1>{});
      } else {
#pragma unroll
        for (int w = 0; w < W; ++w) {
          float4 qv[4];
#pragma unroll
          for (int m = 0; m < 4; ++m) qv[m] = *reinterpret_cast<const float4*>(&(T::BAH ? pqs : qp)[w * RV_U + 16 * s8 + 4 * m]);
#pragma unroll
          for (int p = 0; p < T::NP; ++p) {
            f2 pp = f2{0.f, 0.f};
            if (T::BAH) {
              // Bahdanau, normalize = False: score_t = sum_j v_j tanh(keys_tj + pq_j) (SURVEY.md A.3); keys and pq carry 2 log2(e),
              // v carries -2 log2(e): score * log2(e) = const + sum_j v'_j / (1 + exp2(k'_tj + pq'_j)), the constant cancels in the softmax.
              // Raw v_exp_f32 (no denormal-range rescue: 1 + e does not see it; +inf gives rcp = 0 = tanh's limit)
#pragma unroll
              for (int m = 0; m < 4; ++m) {
                const float4 vv = *reinterpret_cast<const float4*>(&vat[16 * s8 + 4 * m]);
                const float r0 = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kr[p][m].x + qv[m].x));
                const float r1 = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kr[p][m].y + qv[m].y));
                const float r2 = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kr[p][m].z + qv[m].z));
                const float r3 = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kr[p][m].w + qv[m].w));
                pp = __builtin_elementwise_fma(f2{vv.x, vv.y}, f2{r0, r1}, pp);
                pp = __builtin_elementwise_fma(f2{vv.z, vv.w}, f2{r2, r3}, pp);
              }
            } else {
#pragma unroll
              for (int m = 0; m < 4; ++m) {
                pp = __builtin_elementwise_fma(f2{kr[p][m].x, kr[p][m].y}, f2{qv[m].x, qv[m].y}, pp);
                pp = __builtin_elementwise_fma(f2{kr[p][m].z, kr[p][m].w}, f2{qv[m].z, qv[m].w}, pp);
              }
            }
            float sw = pp.x + pp.y;
            sw += dpp<0xB1>(sw);    // quad_perm [1,0,3,2]
            sw += dpp<0x4E>(sw);    // quad_perm [2,3,0,1]
            sw += dpp<0x141>(sw);   // row_half_mirror: the other quad of this 8-lane half
            const int it = 2 * p + half;
            sc[p] = (s8 == w && it < NIT && ((livebits >> it) & 1u)) ? sw : sc[p];
          }
        }
      }
      RV_STAMP(d, step, 4);
      // ================= softmax over the chunk's T_m steps: per-stream (max, sum), one fixed-order merge per beam
      {
        float m = -INFINITY;
#pragma unroll
        for (int p = 0; p < T::NP; ++p) m = fmaxf(m, sc[p]);
        m = fmaxf(m, dpp<0x128>(m));                          // row_ror:8 -- the stream's other half
        float lsum = 0.f;
#pragma unroll
        for (int p = 0; p < T::NP; ++p) { sc[p] = exp2f(sc[p] - m); lsum += sc[p]; }   // stream without live rows: NaN, dropped below
        lsum += dpp<0x128>(lsum);
        if (sub < W) { ml[sid * WB + sub] = m; ml[(32 + sid) * WB + sub] = m == -INFINITY ? 0.f : lsum; }
        __syncthreads();
        if (wv < W) {
          const float ms = lane < 32 ? ml[lane * WB + wv] : -INFINITY;
          const float ls = lane < 32 ? ml[(32 + lane) * WB + wv] : 0.f;
          const float Mg = wave_max_fast(ms);
          const float tot = wave_sum_fast(ms == -INFINITY ? 0.f : ls * exp2f(ms - Mg));   // all-masked chunk: 0 -> NaN like the reference
          if (lane == 0) { mg[wv] = Mg; mg[WB + wv] = Mg == -INFINITY ? __int_as_float(0x7fc00000) : 1.0f / tot; }
        }
        __syncthreads();
        const float f = (s8 < W && m != -INFINITY) ? exp2f(m - mg[s8]) * mg[WB + s8] : 0.f;
        const float nanv = (s8 < W && mg[WB + s8] != mg[WB + s8]) ? mg[WB + s8] : 0.f;
#pragma unroll
        for (int p = 0; p < T::NP; ++p) sc[p] = m == -INFINITY ? nanv : sc[p] * f;   // alignments of beam s8 on this half's rows
        if constexpr (!T::MX) {
          if (d.persist_align && s8 < W) {     // tap (option persist_taps): the fp32 alignments the context sum below consumes
            int t0 = sid, w0 = s8;
            asm volatile("" : "+v"(t0), "+v"(w0));   // nothing of the tap is hoisted out of the step loop (no registers held while taps are off)
            float* out = d.persist_align + ((size_t)step * d.B + b) * W * Tm;   // (uniform base, 32-bit lane offset)
#pragma unroll
            for (int p = 0; p < T::NP; ++p) {
              const int it = 2 * p + half, t = t0 + 32 * it;
              if (it < NIT && t < Tm) out[(unsigned)(w0 * Tm + t)] = sc[p];
            }
          }
          if (float* mvp = persist_moves_arg(s_moves, s_movesTr, mvTr)) {        // moves: the same fp32 alignments, reduced.  Lane (stream t0, half, beam w0) adds its rows, the two
            // halves and the wave's four streams merge by butterflies (the beam stays in place), the eight waves through `ml`, idle
            // from the merge's barrier above to the next step's softmax, in wave order
            int t0 = sid, w0 = s8, hv = half, ln = lane, wq = wv;
            asm volatile("" : "+v"(t0), "+v"(w0), "+v"(hv), "+v"(ln), "+v"(wq));   // (as the tap: nothing held while the pointer is null)
            MoveAcc a = move_zero();
#pragma unroll
            for (int p = 0; p < T::NP; ++p) {
              const int it = 2 * p + hv, t = t0 + 32 * it;
              if (it < NIT && t < Tm) move_add(a, sc[p], t, mvTr);
            }
#pragma unroll
            for (int x = 8; x <= 32; x <<= 1) { const MoveAcc o = move_shfl_xor(a, x); move_merge(a, o); }
            if (ln < W) {
              float* r = ml + (wq * WB + w0) * RV_MOVE_COLS;
              r[0] = a.rm; r[1] = a.r1; r[2] = a.em; r[3] = a.e1; r[4] = a.pk; r[5] = __int_as_float(a.pt);
            }
            __syncthreads();
            if (ln < W && wq == 0) {
#pragma unroll 1
              for (int g = 1; g < 8; ++g) {
                const float* r = ml + (g * WB + w0) * RV_MOVE_COLS;
                move_merge(a, MoveAcc{r[0], r[1], r[2], r[3], r[4], __float_as_int(r[5])});
              }
              move_store(mvp + (((size_t)step * d.B + b) * W + w0) * RV_MOVE_COLS, a);
            }
          }
        }
      }
      RV_STAMP(d, step, 5);
      if constexpr (T::MX) {
        // ================= (Bahdanau on the matrix pipe) the alignments this lane holds -- beam s8 on rows t = sid + 32 (2 p + half) -- as the
        //   context product's A fragments: [k-block t / 8][row mx_row(beam) (+ 1: low part)][t % 8] f16 of alpha 2^14, in `part` (idle
        //   between the gates and the cell product at the end of the step); padded steps carry an alignment of exactly 0
        if (s8 < W) {
          _Float16* aa = reinterpret_cast<_Float16*>(part);
#pragma unroll
          for (int p = 0; p < T::NP; ++p) {
            const int it = 2 * p + half, t = sid + 32 * it;
            if (it < NIT) {
              const float av = sc[p] * 16384.f;
              const _Float16 hi = (_Float16)av, lo = (_Float16)(av - (float)hi);
              _Float16* q = aa + ((t >> 3) * 16 + mx_row(s8)) * 8 + (t & 7);
              q[0] = hi; q[8] = lo;
            }
          }
        }
        __syncthreads();
        if (d.persist_align) tap_align_image<W, true>(d, part, b, step, tid);
        if (float* mvp = persist_moves_arg(s_moves, s_movesTr, mvTr)) moves_from_image<W, NIT, W != 5>(d, mvp, mvTr, part, b, step, tid);
      } else {
        // ================= attention-layer context part = sum_t alpha_t * U'_t, one beam at a time (8-register accumulator)
        {
          float4* slab = reinterpret_cast<float4*>(fold + (size_t)wv * (4 * 2 * 16 * 4));
#pragma unroll
          for (int w = 0; w < W; ++w) {
            f2 a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = f2{0.f, 0.f};
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
              const float al = row_bcast16(sc[it >> 1], 8 * (it & 1) + w);
#pragma unroll
              for (int m = 0; m < 2; ++m) {
                a[2 * m] = __builtin_elementwise_fma(f2{al, al}, f2{ur[it][m].x, ur[it][m].y}, a[2 * m]);
                a[2 * m + 1] = __builtin_elementwise_fma(f2{al, al}, f2{ur[it][m].z, ur[it][m].w}, a[2 * m + 1]);
              }
            }
            // fold the wave's 4 streams (same columns) in ONE LDS round trip: every row parks its 2 column blocks, rows 0 and 1
            // then sum one block each over the 4 streams in fixed order.  DS operations of one wave execute in issue order, so
            // the reads see the writes without a wait in between.
#pragma unroll
            for (int m = 0; m < 2; ++m) slab[(row * 2 + m) * 16 + sub] = make_float4(a[2 * m].x, a[2 * m].y, a[2 * m + 1].x, a[2 * m + 1].y);
            asm volatile("" ::: "memory");
            if (row < 2) {
              const float4 p0 = slab[(0 * 2 + row) * 16 + sub], p1 = slab[(1 * 2 + row) * 16 + sub];
              const float4 p2 = slab[(2 * 2 + row) * 16 + sub], p3 = slab[(3 * 2 + row) * 16 + sub];
              *reinterpret_cast<float4*>(&ctxp[(wv * W + w) * RV_U + 4 * sub + 64 * row]) =
                  make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y, ((p0.z + p1.z) + p2.z) + p3.z, ((p0.w + p1.w) + p2.w) + p3.w);
            }
            asm volatile("" ::: "memory");
          }
        }
        __syncthreads();
        RV_STAMP(d, step, 6);
        for (int i = tid; i < W * RV_U; i += NT) {              // ctx' (8 waves, fixed order) [+ h . A_h (16 K groups) = attention vector when D == 2]
          const int w = i >> 7, col = i & 127;
          float s0 = 0.f;
          if (D > 1) {
#pragma unroll
            for (int g = 0; g < 16; ++g) s0 += part[(g * W + w) * RV_U + col];
          }
          float s1 = 0.f;
#pragma unroll
          for (int g = 0; g < 8; ++g) s1 += ctxp[(g * W + w) * RV_U + col];
          const float av = s0 + s1;
          att[i] = av; attT[col * WB + w] = av;
        }
        __syncthreads();
      }
    }
    if constexpr (T::MX) {
      const int l16 = lane & 15, kq = lane >> 4;
      // ================= attention-layer context part = sum_t alpha_t U'_t on the matrix pipe: rows = beams, this wave's 16 units,
      //   K = the chunk's steps; the product is complete in one wave (no partial sums to merge)
      {
        const _Float16* aa = reinterpret_cast<const _Float16*>(part) + (kq * 16 + l16) * 8;
        f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;           // against the high / the low part of U'
#pragma unroll
        for (int ks = 0; ks < NIT; ++ks) {
          const h8 a = *reinterpret_cast<const h8*>(aa + ks * 512);
          a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, ub[ks][0]), a0, 0, 0, 0);
          a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, ub[ks][1]), a1, 0, 0, 0);
        }
        float acc[2];                                      // beams kq, kq + 4
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = tile_pair_sum(a0, a1, i);
        RV_STAMP(d, step, 6);
        const int col = 16 * wv + l16;
#pragma unroll
        for (int i = 0; i < T::NI; ++i)
          if (kq + 4 * i < W) {
            const float av = acc[i] * d.mx_udescale;
            if constexpr (!T::MXC) att[(kq + 4 * i) * RV_U + col] = av;
            if constexpr (T::MXC) {   // ctx' as A fragments of the cell product: k = col, ctx' . mx_uscale (= acc 2^-14, below 2^14) in two f16 parts
              const float sv = acc[i] * (1.0f / 16384.f);
              const _Float16 hi = (_Float16)sv, lo = (_Float16)(sv - (float)hi);
              _Float16* xq = xim + ((col >> 3) * 16 + mx_row(kq + 4 * i)) * 8 + (col & 7);
              xq[0] = hi; xq[8] = lo;
            } else attT[col * WB + kq + 4 * i] = av;
          }
      }
      // moves: the alignment image is still whole here (`part` is next written behind this barrier), and the product's own registers are free
      if constexpr (T::MXS)
        if (float* mvp = persist_moves_arg(s_moves, s_movesTr, mvTr)) moves_from_image<W, NIT, true>(d, mvp, mvTr, part, b, step, tid);
      __syncthreads();
    }
    RV_STAMP(d, step, 8);
    // ================= logits = attention . W_fc + b_fc
    if constexpr (T::MXC) {
      // Matrix-pipe cell product: the logits are ONE 16-column tile over the beams' [ctx' | h] image (the cell product's A operand),
      // 24 MFMAs that wave 0 takes alone, B fragments from the LDS copy of the 16 KB Wl16 image (from L2 the same reads queue behind
      // the other waves' weight stream: 4.4 k cycles) -- the other waves go straight on to the cell product (they only need ctx' and
      // h): no logits phase and no barrier in front of the beam step.
      if (wv == 0) {
        const int l16 = lane & 15, kq = lane >> 4;
        const _Float16* xa = xim + (kq * 16 + l16) * 8;
        const uint4* wl = reinterpret_cast<const uint4*>(dsm + L.wl16) + lane;
        f4v a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          uint4 bh[4], bl[T::P1 ? 1 : 4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if constexpr (T::P1) bh[i] = wl[(4 * half + i) * 64];
            else { bh[i] = wl[(2 * (4 * half + i)) * 64]; bl[i] = wl[(2 * (4 * half + i) + 1) * 64]; }
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const h8 a = *reinterpret_cast<const h8*>(xa + (4 * half + i) * 512);
            a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, bh[i]), a0, 0, 0, 0);
            if constexpr (!T::P1) a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, bl[i]), a1, 0, 0, 0);   // (one-part: a1 stays +0, what a zero second part leaves)
          }
        }
        float acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i] = tile_pair_sum(a0, a1, i);
#pragma unroll
        for (int i = 0; i < T::NI; ++i)
          if (kq + 4 * i < W && l16 < V) lg[(kq + 4 * i) * RV_MAX_VOCAB + l16] = acc[i] * d.mx_ldescale + s_wfc[T::BFC + l16];
      }
    } else {
      const int o8 = tid >> 3, s8 = tid & 7;
      if (o8 < W * V) {                                     // whole 8-lane groups take the branch together
        const int w = o8 / V, v = o8 % V;
        // lane s8 takes k = 16 s8 .. 16 s8 + 15: four float4 of the attention vector against four of the weight row
        f2 pp = f2{0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const float4 a4 = *reinterpret_cast<const float4*>(&att[w * RV_U + 16 * s8 + 4 * m]);
          const float4 w4 = *reinterpret_cast<const float4*>(&s_wfc[v * T::FCW + 16 * s8 + 4 * m]);
          pp = __builtin_elementwise_fma(f2{a4.x, a4.y}, f2{w4.x, w4.y}, pp);
          pp = __builtin_elementwise_fma(f2{a4.z, a4.w}, f2{w4.z, w4.w}, pp);
        }
        if (D == 1) {                                       // + h . (A_h W_fc)
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const float4 a4 = *reinterpret_cast<const float4*>(&qp[w * RV_U + 16 * s8 + 4 * m]);
            const float4 w4 = *reinterpret_cast<const float4*>(&s_nh[v * T::FCW + 16 * s8 + 4 * m]);
            pp = __builtin_elementwise_fma(f2{a4.x, a4.y}, f2{w4.x, w4.y}, pp);
            pp = __builtin_elementwise_fma(f2{a4.z, a4.w}, f2{w4.z, w4.w}, pp);
          }
        }
        float p = pp.x + pp.y;
        p += dpp<0xB1>(p);    // quad_perm [1,0,3,2]
        p += dpp<0x4E>(p);    // quad_perm [2,3,0,1]
        p += dpp<0x141>(p);   // row_half_mirror: the other quad of this 8-lane group
        if (s8 == 0) lg[w * RV_MAX_VOCAB + v] = p + s_wfc[T::BFC + v];
      }
      __syncthreads();
    }
    RV_STAMP(d, step, 9);
    // ================= beam step (wave 0): log-softmax, finished masking, top-W, bookkeeping
    if (tid < 64) {
      const int w = lane / V, v = lane % V;
      const bool cand = lane < W * V;
      const size_t o = ((size_t)step * d.B + b) * W;
      float val = -INFINITY;
      if (d.greedy) {                  // GreedyEmbeddingSampler: argmax of the raw logits (W == 1)
        if (cand) { val = lg[v]; d.step_logits[((size_t)step * d.B + b) * V + v] = val; }
      } else if (cand) {
        if (d.step_logits) d.step_logits[(((size_t)step * d.B + b) * W + w) * V + v] = lg[w * RV_MAX_VOCAB + v];   // debug tap (option persist_taps)
        float lv[RV_MAX_VOCAB];                             // the beam's logits in two LDS reads; same order of operations as the loops
        *reinterpret_cast<float4*>(lv) = *reinterpret_cast<const float4*>(&lg[w * RV_MAX_VOCAB]);
        *reinterpret_cast<float4*>(lv + 4) = *reinterpret_cast<const float4*>(&lg[w * RV_MAX_VOCAB + 4]);
        float m = lv[0];
#pragma unroll
        for (int x = 1; x < RV_MAX_VOCAB; ++x) m = x < V ? fmaxf(m, lv[x]) : m;
        float ssum = 0.f, mine = lv[0];
#pragma unroll
        for (int x = 0; x < RV_MAX_VOCAB; ++x) { ssum += x < V ? __expf(lv[x] - m) : 0.f; mine = x == v ? lv[x] : mine; }
        const float lse = __logf(ssum);
        const bool fin = s_fin[w] != 0;
        const float lp = fin ? (v == d.end_token ? 0.f : -FLT_MAX) : (mine - m) - lse;
        val = s_lprob[w] + lp;
      }
      bool taken = !cand;
      int my_word = 0, my_par = 0; float my_val = 0.f;
      for (int k = 0; k < W; ++k) {
        const float mx = wave_max_fast(taken ? -INFINITY : val);
        const unsigned long long hit = __ballot(!taken && (val == mx || mx == -INFINITY));
        const int win = __ffsll((long long)hit) - 1;
        const float wval = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(val), win));
        if (lane == win) taken = true;
        if (lane == k) { my_word = win % V; my_par = win / V; my_val = wval; }
      }
      bool nf = false; int nl = 0;
      if (lane < W) {
        const bool pf = s_fin[my_par] != 0;
        nf = pf || my_word == d.end_token;
        nl = s_len[my_par] + (pf ? 0 : 1);
      }
      const unsigned long long fmask = __ballot(lane < W && nf);
      if (W == 1 && d.forced) {      // (one beam: the wider instantiations compile this branch away)
        // TrainingSampler with sequence_length = L - 1 for every row: the next input is the next label, sample_id is still the argmax of
        // the raw logits, and no chunk waits for or reports to another -- every chunk runs exactly L - 1 steps (s_fin, s_allfin stay 0)
        if (lane == 0) {
          d.step_ids[(size_t)step * d.B + b] = my_word;
          s_tok[0] = persist_forced_tok(d, b, step + 1); s_parent[0] = 0;
        }
      } else if (d.greedy) {
        // BasicDecoder without impute_finished: a finished row keeps sampling and the loop runs until EVERY row of the
        // slab has finished, so a chunk may only stop once all chunks have reported their first finished step
        // (nfin[0] = how many have, nfin[1] = the latest of those steps + 1) and it has itself recorded that many steps.
        if (lane == 0) {
          const bool pf = s_fin[0] != 0;
          d.step_ids[(size_t)step * d.B + b] = my_word;
          s_tok[0] = my_word; s_fin[0] = nf; s_parent[0] = 0;
          if (nf && !pf) { s_len[0] = step + 1; atomicMax(&d.nfin[1], step + 1); __threadfence(); atomicAdd(&d.nfin[0], 1); }
          // writer: atomicMax(step) -> fence -> atomicAdd(count); reader: count, ACQUIRE fence, then the step, so a reader that
          // sees every chunk counted also sees every chunk's first-finish step (the two words sit in different L2 channels).
          // The acquire fence is only paid once the count is complete (the last few steps of the slab).
          const int cnt = __hip_atomic_load(&d.nfin[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          int stop = 0;
          if (nf && cnt >= d.B) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const int sg = __hip_atomic_load(&d.nfin[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            stop = step + 1 >= sg;
          }
          s_allfin = stop;
        }
      } else {
      if (lane < W) {      // all reads of the old bookkeeping happened above (same wave, program order)
        d.step_ids[o + lane] = my_word; d.parent_ids[o + lane] = my_par; d.step_scores[o + lane] = my_val;
        s_tok[lane] = my_word; s_fin[lane] = nf; s_lprob[lane] = my_val; s_len[lane] = nl; s_parent[lane] = my_par;
      }
      if (lane == 0) s_allfin = __popcll(fmask) == W;
      }
      RV_STAMP(d, step, 11);      // end of the beam step (wave 0)
    }
    // ================= next step's cell product on THIS step's beams: z~[w] = [attention_w | h_w] . Wcat (the beam step above
    //   only decides which z~ each new beam inherits).  thread = (4 gate columns c4, K group kg); waves 1-7 start at once,
    //   wave 0 joins after the beam step, so K group 0 (waves 0-1) is the short one: rows 0-39 | 40-111 | 112-183 | 184-255.
    if constexpr (T::MXC2) {
      // Two cells on the matrix pipe.  End of the step, on THIS step's beams (the beam step only decides which rows each new beam inherits):
      //   cell 0's next product  z~_0 = [ctx' | h_1 | h_0] . [W_a ; A_h W_a ; U_0]   (K = 384: jobs 0..47, pair j = 4 ks + g of the Wc16 image)
      //   cell 1's recurrent one z~_1 = h_1 . U_1                                     (K = 128: jobs 48..63, pairs 16..31 of the W1c16 image)
      // -- the attention vector never exists: its h_1 . A_h half is folded into cell 0's rows 128..255 and into the output layer at
      // load time, its context half is the ctx' segment.  Wave wv owns units 16 wv .. 16 wv + 15 of all four gates of both products
      // (64 jobs of 2 KB); wave 0 -- output layer and beam step first -- finds its first MXC2_CACHE jobs in LDS.
      if (step + 1 < steps) {
        RV_STAMP_W1(d, step, 12);
        const int l16 = lane & 15, kq = lane >> 4;
        const uint4* w0img = reinterpret_cast<const uint4*>(d.Wc16) + (size_t)wv * (48 * 128) + lane;
        const uint4* w1img = reinterpret_cast<const uint4*>(d.W1c16) + (size_t)wv * (32 * 128) + 16 * 128 + lane;
        const _Float16* xa = xim + (kq * 16 + l16) * 8;
        constexpr int NB = 4;
        f4v acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = f4v{0.f, 0.f, 0.f, 0.f};
        auto src = [&](int j, int q) -> uint4 { return j < 48 ? w0img[(2 * j + q) * 64] : w1img[(2 * (j - 48) + q) * 64]; };
        auto mm = [&](int j, const uint4& vh, const uint4& vl) {
          const int ks = j < 48 ? (j >> 2) : 4 + ((j - 48) >> 2), g = j & 3;      // h_1 . U_1 reads the h_1 segment: k-steps 4..7
          const h8 a = *reinterpret_cast<const h8*>(xa + ks * 512);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, vl), acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, vh), acc[g], 0, 0, 0);
        };
        auto flush = [&](float* dst, float scale) {         // C/D: lane (column l16, kq): registers 0 + 1 = beam kq, 2 + 3 = beam kq + 4
#pragma unroll
          for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int i = 0; i < T::NI; ++i)
              if (kq + 4 * i < W) dst[(kq + 4 * i) * T::ZS + RV_U * g + 16 * wv + l16] = (acc[g][2 * i] + acc[g][2 * i + 1]) * scale;
            acc[g] = f4v{0.f, 0.f, 0.f, 0.f};
          }
        };
        auto stream = [&](auto first_tag) {
          constexpr int J0 = decltype(first_tag)::value;    // jobs J0..63 come from L2 through a window of NB
          uint4 bh[NB], bl[NB];
#pragma unroll
          for (int i = 0; i < NB; ++i) { bh[i] = src(J0 + i, 0); bl[i] = src(J0 + i, 1); }
          if constexpr (J0 > 0) {                            // (wave 0) the LDS-resident jobs first: the first requests are in flight meanwhile
            const uint4* wc = reinterpret_cast<const uint4*>(wcache) + lane;
            uint4 fh = wc[0], fl = wc[64];
#pragma unroll
            for (int j = 0; j < J0; ++j) {
              uint4 nh = fh, nl = fl;
              if (j + 1 < J0) { nh = wc[(2 * (j + 1)) * 64]; nl = wc[(2 * (j + 1) + 1) * 64]; }
              mm(j, fh, fl);
              fh = nh; fl = nl;
              __builtin_amdgcn_sched_barrier(0);
            }
          }
#pragma unroll
          for (int j = J0; j < 64; ++j) {
            mm(j, bh[(j - J0) % NB], bl[(j - J0) % NB]);
            __builtin_amdgcn_sched_barrier(0);
            if (j + NB < 64) { bh[(j - J0) % NB] = src(j + NB, 0); bl[(j - J0) % NB] = src(j + NB, 1); }
            if (j == 47) flush(part, d.mx_cdescale);
            __builtin_amdgcn_sched_barrier(0);
          }
          flush(partU, d.mx_c1descale);
        };
        if (wv == 0) stream(std::integral_constant<int, MXC2_CACHE>{});
        else stream(std::integral_constant<int, 0>{});
        RV_STAMP_W1(d, step, 13);
      }
    } else if constexpr (T::MXC) {
      // Matrix pipe: z~ [beams x 512] = x [beams x 256] . Wcat2 as split-f16 MFMAs.  Wave wv owns units 16 wv .. 16 wv + 15 of all
      // four gates over the whole K (no partial sums to merge): 32 (k-step, gate) pairs, each one B fragment pair (high, low
      // part; 2 KB per wave) streamed from the Wc16 image through a rolling window of NB pairs, the last NC pairs from LDS.  A = the
      // beams' [ctx' | h] image (rows = beam slots as in the scores), three exact part products per pair.
      if (step + 1 < steps) {
        RV_STAMP_W1(d, step, 12);
        const int l16 = lane & 15, kq = lane >> 4;
        const uint4* wimg = reinterpret_cast<const uint4*>(d.Wc16) + (size_t)wv * (32 * T::FR) + lane;   // pair p, part q: [(2 p + q) * 64]; one-part: [p * 64]
        const _Float16* xa = xim + (kq * 16 + l16) * 8;      // k-step ks: + 512 ks (both parts of a beam in rows mx_row, + 1)
        constexpr int NS = 32 - T::NC - T::NR, NB = 4;             // streamed pairs
        f4v acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = f4v{0.f, 0.f, 0.f, 0.f};
        auto mm = [&](int p, const uint4& vh, const uint4& vl) {
          const int ks = p >> 2, g = p & 3;
          const h8 a = *reinterpret_cast<const h8*>(xa + ks * 512);
          if constexpr (!T::P1) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, vl), acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, vh), acc[g], 0, 0, 0);
        };
        // One-part fragments (T::P1): the MFMA against the second part is the one left out -- against a zero part it adds +0 -- and every
        // gate's accumulator takes its k-steps in the order the two-part form of the same width takes them (wave 0: 0..7; the others: the
        // last mxc_nc(W) pairs first, then the rest in rising order), wherever a pair is kept.  So both forms agree bit for bit.
        // Wave 0 takes the output layer and the beam step first (4.7 k cycles); its columns' 32 pairs all sit in LDS (64 KB) and it takes
        // them afterwards, half a k-step (two gates) at a time with the next half's fragments requested before this half's MFMAs.  (As a
        // chain of whole k-steps, each waiting for its eight LDS reads -- round 3 -- the 32 pairs took 4.3 k cycles and the step ended
        // 1.5 k cycles after the streaming waves had finished: C3 launch 0.342 -> 0.325 ms, R 0.916 -> 0.842 on one box, round-robin.
        // Handing wave 0's columns to waves 1-4, one gate each between their own streamed pairs, measured SLOWER than either, 0.35 / 0.88:
        // the extra LDS round trips delay the streaming waves' next requests, and with T_m > 256 there is no register for a prefetch.)
        if constexpr (T::P1) {
          if (wv == 0) {                                     // a whole k-step (four gates, 4 KB) at a time, the next one's fragments requested first
            const uint4* wc = reinterpret_cast<const uint4*>(wcache) + lane;     // pair p = 4 ks + g: [p * 64]
            uint4 fr[2][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) fr[0][j] = wc[j * 64];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
              if (ks + 1 < 8) {
#pragma unroll
                for (int j = 0; j < 4; ++j) fr[(ks + 1) & 1][j] = wc[(4 * (ks + 1) + j) * 64];
              }
#pragma unroll
              for (int g = 0; g < 4; ++g) mm(4 * ks + g, fr[ks & 1][g], fr[ks & 1][g]);
              __builtin_amdgcn_sched_barrier(0);
            }
          } else {
            constexpr int NE = mxc_nc(W);                    // the pairs the two-part form takes first
            uint4 bh[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) bh[i] = wimg[i * 64];
            const uint4* wc = reinterpret_cast<const uint4*>(wcache) + 32 * 64 + (size_t)(wv - 1) * (T::NC * 64) + lane;   // pair 32 - NC + c: [c * 64]
#pragma unroll
            for (int c = T::NC - NE; c < T::NC; ++c) mm(32 - T::NC + c, wc[c * 64], wc[c * 64]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < NS; ++p) {
              mm(p, bh[p % NB], bh[p % NB]);
              __builtin_amdgcn_sched_barrier(0);
              if (p + NB < NS) bh[p % NB] = wimg[(p + NB) * 64];
              __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (T::NR > 0) {                       // the pairs that live in registers
#pragma unroll
              for (int r = 0; r < T::NR; ++r) mm(NS + r, rbh[r], rbh[r]);
            }
#pragma unroll
            for (int c = 0; c < T::NC - NE; ++c) mm(32 - T::NC + c, wc[c * 64], wc[c * 64]);      // the rest of the on-chip pairs
          }
        } else if (wv == 0) {
          const uint4* wc = reinterpret_cast<const uint4*>(wcache) + lane;       // pair p = 4 ks + g, part q: [(2 p + q) * 64]
          uint4 fr[2][4];                                    // [buffer][(g0 high, g0 low, g1 high, g1 low)]
#pragma unroll
          for (int j = 0; j < 4; ++j) fr[0][j] = wc[j * 64];
#pragma unroll
          for (int hs = 0; hs < 16; ++hs) {                  // half k-steps: k-step hs / 2, gates 2 (hs % 2), + 1
            if (hs + 1 < 16) {
#pragma unroll
              for (int j = 0; j < 4; ++j) fr[(hs + 1) & 1][j] = wc[(4 * (hs + 1) + j) * 64];
            }
            const h8 a = *reinterpret_cast<const h8*>(xa + (hs >> 1) * 512);
            const int g0 = 2 * (hs & 1);
            acc[g0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, fr[hs & 1][1]), acc[g0], 0, 0, 0);
            acc[g0 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, fr[hs & 1][3]), acc[g0 + 1], 0, 0, 0);
            acc[g0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, fr[hs & 1][0]), acc[g0], 0, 0, 0);
            acc[g0 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(h8, fr[hs & 1][2]), acc[g0 + 1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          uint4 bh[NB], bl[NB];
#pragma unroll
          for (int i = 0; i < NB; ++i) { bh[i] = wimg[(2 * i) * 64]; bl[i] = wimg[(2 * i + 1) * 64]; }
          {                                                  // the on-chip pairs first: the first requests are in flight meanwhile
            const uint4* wc = reinterpret_cast<const uint4*>(wcache) + 32 * 128 + (size_t)(wv - 1) * (T::NC * 128) + lane;
#pragma unroll
            for (int c = 0; c < T::NC; ++c) mm(32 - T::NC + c, wc[(2 * c) * 64], wc[(2 * c + 1) * 64]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int p = 0; p < NS; ++p) {
            mm(p, bh[p % NB], bl[p % NB]);
            __builtin_amdgcn_sched_barrier(0);
            if (p + NB < NS) { bh[p % NB] = wimg[(2 * (p + NB)) * 64]; bl[p % NB] = wimg[(2 * (p + NB) + 1) * 64]; }
            __builtin_amdgcn_sched_barrier(0);
          }
          if constexpr (T::NR > 0) {                            // the pairs that live in registers
#pragma unroll
            for (int r = 0; r < T::NR; ++r) mm(NS + r, rbh[r], rbl[r]);
          }
        }
        // C/D: lane (column l16, kq) holds rows 4 kq + i: registers 0 + 1 = beam kq (high- and low-part rows), 2 + 3 = beam kq + 4
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int i = 0; i < T::NI; ++i)
            if (kq + 4 * i < W) part[(kq + 4 * i) * T::ZS + RV_U * g + 16 * wv + l16] = (acc[g][2 * i] + acc[g][2 * i + 1]) * d.mx_cdescale;
        RV_STAMP_W1(d, step, 13);
      }
    } else if (step + 1 < steps) {
      const int c4 = tid & 127, kg = tid >> 7;
      // one cell: rows 0-39 | 40-111 | 112-183 | 184-255;  two cells: 64 rows each here, and K groups 1-3 also take the
      // second cell's recurrent product below (48 / 40 / 40 rows)
      const int kb = D > 1 ? 64 * kg : (kg == 0 ? 0 : 72 * kg - 32), ke = D > 1 ? kb + 64 : (kg == 0 ? 40 : kb + 72);
      f2 acc[W][2];
#pragma unroll
      for (int w = 0; w < W; ++w) { acc[w][0] = f2{0.f, 0.f}; acc[w][1] = f2{0.f, 0.f}; }
      const float* wc = Wcat + 4 * c4;
      auto fma_row = [&](const float4& wr, const float* xrow) { beams_fma_row<W>(acc, wr, xrow); };
      const bool cached = T::CACHE && kg > 0;                  // wave-uniform: K groups 1-3 find their last 8 rows in LDS
      const int ke_g = cached ? ke - 8 : ke;                // rows streamed from L2
      if (cached) {                                         // the rows that are already on chip
        const int kc = ke - 8;
        const float* xk = kc < RV_U ? attT + kc * WB : hcT + (kc - RV_U) * WB;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          fma_row(*reinterpret_cast<const float4*>(&wcache[((kg - 1) * 8 + i) * RV_G + 4 * c4]), xk + i * WB);
      }
#pragma unroll 1
      for (int k0 = kb; k0 < ke_g; k0 += 8) {               // batches never straddle row 128 (40, 112 and 184 are multiples of 8)
        float4 wr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wr[i] = *reinterpret_cast<const float4*>(wc + (size_t)(k0 + i) * RV_G);
        __builtin_amdgcn_sched_barrier(0);
        const float* xk = k0 < RV_U ? attT + k0 * WB : (D > 1 ? h0T : hcT) + (k0 - RV_U) * WB;
#pragma unroll
        for (int i = 0; i < 8; ++i) fma_row(wr[i], xk + i * WB);
      }
#pragma unroll
      for (int w = 0; w < W; ++w)
        *reinterpret_cast<float4*>(&part[(kg * W + w) * RV_G + 4 * c4]) = make_float4(acc[w][0].x, acc[w][0].y, acc[w][1].x, acc[w][1].y);
      if (D > 1 && kg > 0) {            // h_1 . U_1 of this step's beams (U_1 = rows 128..255 of Wcat1; h_1 = hcT's h rows)
        const int rb = kg == 1 ? 0 : 8 + 40 * (kg - 1), re = kg == 1 ? 48 : rb + 40;
#pragma unroll
        for (int w = 0; w < W; ++w) { acc[w][0] = f2{0.f, 0.f}; acc[w][1] = f2{0.f, 0.f}; }
        const float* wu = Wcat1 + (size_t)RV_U * RV_G + 4 * c4;
#pragma unroll 1
        for (int k0 = rb; k0 < re; k0 += 8) {
          float4 wr[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) wr[i] = *reinterpret_cast<const float4*>(wu + (size_t)(k0 + i) * RV_G);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int i = 0; i < 8; ++i) beams_fma_row<W>(acc, wr[i], &hcT[(k0 + i) * WB]);
        }
#pragma unroll
        for (int w = 0; w < W; ++w)
          *reinterpret_cast<float4*>(&partU[((kg - 1) * W + w) * RV_G + 4 * c4]) = make_float4(acc[w][0].x, acc[w][0].y, acc[w][1].x, acc[w][1].y);
      }
    }
    __syncthreads();
    RV_STAMP(d, step, 10);
    if (s_allfin) { done_steps = step + 1; break; }         // uniform: every thread reads the same LDS word
  }
  if (tid < W) { d.lengths[row0 + tid] = s_len[tid]; d.finished[row0 + tid] = (uint8_t)s_fin[tid]; }
  if (tid == 0) d.chunk_steps[b] = d.greedy ? (s_fin[0] ? s_len[0] : steps) : done_steps;   // greedy: the row's first finished step + 1
