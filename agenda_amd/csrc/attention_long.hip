// Recording cross-attention over several key tiles (97 .. 320 keys) for gfx950: the DAAM recorder for long and weighted prompts.
//
// attention.hip's recording kernels hold the whole key axis in one tile (Nk <= 96) because a recorded probability has to be final -- divided
// by the row sum over ALL keys -- when it is added into the accumulator.  Here the keys stream in tiles of 64, so every query tile makes two
// passes over them:
//   pass 1  streams the K tiles alone and keeps, per query, the running maximum m of the scaled logits and the sum l of exp(s - m);
//   pass 2  streams K and V, forms p = exp(s - m) with the FINAL m, adds p / l into the token-major rows rec[img][head][t][pixel] of that
//           tile's keys (one lane owns each (image, head, token, pixel): plain read-modify-write, no atomics, equal bits run to run) and
//           accumulates O^T += V^T . P^T with no rescale; O is divided by l once at the end.
// K is read twice: at most 320 rows per (batch row, head), resident in L2.  K + V of 320 keys at d = 160 do not fit the LDS, hence tiles.
//
// Same MFMA formulation as attention.hip (S^T = K . Q^T with the query on the lane, V^T through ds_read_b64_tr_b16) and the roundings of its
// recording kernels, which tests/_attn_model.py states with fold=False:
//   - q, k, v are bf16; the raw logits q . k accumulate in fp32 and are scaled by scale * log2(e) in fp32 (nothing folded into q);
//   - the unnormalised probabilities exp(s - m) are rounded to bf16 before P V (the recorded ones stay fp32: p * (1 / l));
//   - the output O / l is rounded to bf16.
// record_mode 1 only; rec_b0 / rec_T as there: batch rows below rec_b0 are computed but not recorded, token rows >= rec_T never touched
// (the buffer descriptor's range check drops them).
#include "kernels.h"

template <int D> struct LongCfg {
  static constexpr int KB = 2, KEYS = KB * 32;           // keys per tile
  static constexpr int KSTEPS = (D + 15) / 16;           // QK^T k-steps (d padded to 16)
  static constexpr int DBLK = (D + 31) / 32;             // PV output d-blocks (d padded to 32)
  static constexpr int KCH = KSTEPS * 2;                 // 16-B chunks per K row incl. zero pad
  static constexpr int KPITCH = ((KCH | 1)) * 16;        // odd #chunks -> conflict-free b128 row reads
  static constexpr int VPITCH = ((DBLK | 1)) * 64;       // odd multiple of 64 B -> conflict-free tr reads
  static constexpr int CH = D / 8;                       // real 16-B chunks per row
  static constexpr int LDS = KEYS * (KPITCH + VPITCH);   // one stage: K tile | V tile
};

template <int D>
__global__ __launch_bounds__(256, 1) void attn_long_kernel(const AttnP p) {
  using C = LongCfg<D>;
  constexpr int KB = C::KB, KEYS = C::KEYS, KSTEPS = C::KSTEPS, DBLK = C::DBLK, KPITCH = C::KPITCH, VPITCH = C::VPITCH, CH = C::CH;
  constexpr int NCHUNK = KEYS * CH;                      // 16-B chunks per K (or V) tile
  constexpr int LD_IT = (NCHUNK + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const sK = smem;
  char* const sV = smem + KEYS * KPITCH;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 31, hh = lane >> 5;
  // XCD-aware 1-D grid as in attention.hip: the query tiles of one (batch row, head) go to one XCD, whose L2 then serves both K passes
  const int nqt = p.nqt, nbh = p.B * p.H;
  int bh, qt;
  {
    const int id = blockIdx.x, x = id & 7, j = id >> 3;
    const int per = (nbh + 7) >> 3;
    const int lb = j / nqt;
    qt = j - lb * nqt;
    bh = x * per + lb;                                   // may exceed nbh for the last groups: exit
  }
  if (bh >= nbh) return;
  const int head = bh % p.H, b = bh / p.H;
  const int q0 = qt * 128 + wid * 32;
  const bf16_t* kp = p.k + b * p.sk + head * D;
  const bf16_t* vp = p.v + b * p.sv + head * D;

  // pad chunks (never overwritten by tile loads): zeros
  if constexpr (C::KCH > CH) {
    for (int i = tid; i < KEYS * (C::KCH - CH); i += 256) {
      const int r = i / (C::KCH - CH), cc = CH + i % (C::KCH - CH);
      *(u32x4*)(sK + r * KPITCH + cc * 16) = u32x4{0, 0, 0, 0};
    }
  }
  if constexpr (DBLK * 4 > CH) {
    for (int i = tid; i < KEYS * (DBLK * 4 - CH); i += 256) {
      const int r = i / (DBLK * 4 - CH), cc = CH + i % (DBLK * 4 - CH);
      *(u32x4*)(sV + r * VPITCH + cc * 16) = u32x4{0, 0, 0, 0};
    }
  }

  // Q fragments: lane (c, hh) holds Q[q0 + c][16s + 8hh .. +8]; rows >= Nq are zeros (computed, never stored or recorded)
  bf16x8 qf[KSTEPS];
  {
    const bf16_t* qp = p.q + b * p.sq + head * D;
    const int qrow = q0 + c;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const int d0 = 16 * s + 8 * hh;
      u32x4 v = u32x4{0, 0, 0, 0};
      if (qrow < p.Nq && d0 < D) v = *(const u32x4*)(qp + (long long)qrow * p.ldq + d0);
      qf[s] = __builtin_bit_cast(bf16x8, v);
    }
  }

  // K/V tile loads through buffer descriptors: rows >= Nk fall outside num_records and read as zeros
  u32x4 kreg[LD_IT], vreg[LD_IT];
  unsigned kvoff[LD_IT], vvoff[LD_IT];
#pragma unroll
  for (int it = 0; it < LD_IT; ++it) {
    const int idx = tid + it * 256;
    const int r = idx / CH, cc = idx - r * CH;
    kvoff[it] = (idx < NCHUNK) ? (unsigned)((r * p.ldk + cc * 8) * 2) : 0x80000000u;
    vvoff[it] = (idx < NCHUNK) ? (unsigned)((r * p.ldv + cc * 8) * 2) : 0x80000000u;
  }
  const unsigned k_bytes = (unsigned)(((long long)(p.Nk - 1) * p.ldk + D) * 2), v_bytes = (unsigned)(((long long)(p.Nk - 1) * p.ldv + D) * 2);
  const auto krs = __builtin_amdgcn_make_buffer_rsrc((void*)kp, 0, k_bytes, 0x00020000);
  const auto vrs = __builtin_amdgcn_make_buffer_rsrc((void*)vp, 0, v_bytes, 0x00020000);
  const int ntiles = (p.Nk + KEYS - 1) / KEYS;
  // step s of 2 * ntiles: pass s / ntiles over tile s % ntiles; pass 0 needs K alone
  auto gload = [&](int step) {
    const int tile = step >= ntiles ? step - ntiles : step;
    const unsigned ks_ = __builtin_amdgcn_readfirstlane((unsigned)(tile * KEYS * p.ldk * 2));
    const unsigned vs_ = __builtin_amdgcn_readfirstlane((unsigned)(tile * KEYS * p.ldv * 2));
#pragma unroll
    for (int it = 0; it < LD_IT; ++it) kreg[it] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, kvoff[it], ks_, 0));
    if (step >= ntiles) {
#pragma unroll
      for (int it = 0; it < LD_IT; ++it) vreg[it] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vrs, vvoff[it], vs_, 0));
    }
  };
  auto lstore = [&](int step) {
#pragma unroll
    for (int it = 0; it < LD_IT; ++it) {
      const int idx = tid + it * 256;
      const int r = idx / CH, cc = idx - r * CH;
      if (idx < NCHUNK) {
        *(u32x4*)(sK + r * KPITCH + cc * 16) = kreg[it];
        if (step >= ntiles) *(u32x4*)(sV + r * VPITCH + cc * 16) = vreg[it];
      }
    }
  };
  // S^T = K . Q^T of the staged tile; keys >= Nk (last tile only) become -inf
  auto scores = [&](int tile, f32x16 (&sacc)[KB]) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int s = 0; s < KSTEPS; ++s) {
        const bf16x8 a = *(const bf16x8*)(sK + (kb * 32 + c) * KPITCH + (2 * s + hh) * 16);
        if (s == 0) { const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                      sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], z, 0, 0, 0); }
        else sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], sacc[kb], 0, 0, 0);
      }
    }
    if ((tile + 1) * KEYS > p.Nk) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = tile * KEYS + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
          if (key >= p.Nk) sacc[kb][i] = -INFINITY;
        }
    }
  };

  const float sc = p.scale * 1.44269504088896340736f;     // exp(x) = exp2(x * log2 e)
  gload(0);

  // ---- pass 1: row maximum (log2 units, shared by the two half-waves of a query) and this lane's part of the row sum ----
  // tile 0 is full (Nk > 64), so m is finite from the first tile on and a masked key gives exp2(-inf) = 0
  float m_run = -INFINITY, l_run = 0.f;
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();                                      // every wave has read the previous tile
    lstore(t);
    __syncthreads();
    gload(t + 1);                                         // t + 1 == ntiles: tile 0 of pass 2, K and V
    f32x16 sacc[KB];
    scores(t, sacc);
    float mx = sacc[0][0];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sacc[kb][i]);
    const float m_new = fmaxf(m_run, xhalf_max(mx) * sc);
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) rs += __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], sc, -m_new));
    l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + rs;
    m_run = m_new;
  }
  const float inv = 1.0f / xhalf_sum(l_run);
  const float nm = -m_run;

  // ---- pass 2: final probabilities -> recorder rows, O^T += V^T . P^T ----
  f32x16 oacc[DBLK];
#pragma unroll
  for (int i = 0; i < DBLK; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) oacc[i][j] = 0.f;
  // V^T fragment addressing for ds_read_b64_tr_b16: lane supplies row (key), 4 columns
  const int gi = lane & 15;
  const int tr_row = (gi >> 2) + 4 * hh;
  const int tr_col = ((lane >> 4) & 1) * 16 + (gi & 3) * 4;
  const bool recl = p.record_mode == 1 && b >= p.rec_b0 && (q0 + c) < p.Nq;
  // wave-uniform base (this image / head slice), one 32-bit per-lane offset; num_records = rec_T * Nq * 4 B drops token rows >= rec_T
  float* rbase = p.rec + (long long)(b - p.rec_b0) * p.rec_img_stride + head * p.rec_head_stride;
  const auto rrs = __builtin_amdgcn_make_buffer_rsrc(recl ? rbase : p.rec, 0, recl ? (unsigned)p.rec_T * (unsigned)p.Nq * 4u : 0u, 0x00020000);
  const unsigned rowb = (unsigned)p.Nq * 4u;
  const unsigned voff0 = (unsigned)(q0 + c) * 4u + (unsigned)(4 * hh) * rowb;

  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();
    lstore(ntiles + t);
    __syncthreads();
    if (t + 1 < ntiles) gload(ntiles + t + 1);
    f32x16 sacc[KB];
    scores(t, sacc);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[kb][i] = __builtin_amdgcn_exp2f(fmaf(sacc[kb][i], sc, nm));
    if (recl && t * KEYS < p.rec_T) {
      // all old values of a key block are loaded first, then added, then stored: the RMW chains overlap
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const unsigned trow = (unsigned)(t * KEYS + kb * 32);
        float old[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
          old[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrs, voff0 + (trow + (unsigned)((i & 3) + 8 * (i >> 2))) * rowb, 0, 0));
#pragma unroll
        for (int i = 0; i < 16; ++i)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, old[i] + sacc[kb][i] * inv), rrs,
                                                voff0 + (trow + (unsigned)((i & 3) + 8 * (i >> 2))) * rowb, 0, 0);
      }
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (__bf16)sacc[kb][8 * s + j];
        const char* vb = sV + (kb * 32 + 16 * s + tr_row) * VPITCH + tr_col * 2;
#pragma unroll
        for (int db = 0; db < DBLK; ++db) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + db * 64));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + 8 * VPITCH + db * 64));
          const u32x2 lo2 = __builtin_bit_cast(u32x2, lo), hi2 = __builtin_bit_cast(u32x2, hi);
          const u32x4 a4 = u32x4{lo2[0], lo2[1], hi2[0], hi2[1]};
          oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a4), pf, oacc[db], 0, 0, 0);
        }
      }
  }

  // ---- O[query][d] = O^T / l ----
  const int qrow = q0 + c;
  if (qrow < p.Nq) {
    bf16_t* op = p.o + b * p.so + (long long)qrow * p.ldo + head * D;
#pragma unroll
    for (int db = 0; db < DBLK; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d0 = db * 32 + 8 * g + 4 * hh;
        if (d0 < D) {
          u32x2 pk;
          pk[0] = pack_bf2(oacc[db][4 * g + 0] * inv, oacc[db][4 * g + 1] * inv);
          pk[1] = pack_bf2(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv);
          *(u32x2*)(op + d0) = pk;
        }
      }
  }
}

template <int D>
static int launch_attn_long_d(const AttnP& p, hipStream_t st) {
  AttnP pp = p;
  pp.nqt = (p.Nq + 127) / 128;
  const int per = (p.B * p.H + 7) / 8;
  hipLaunchKernelGGL(attn_long_kernel<D>, dim3(8 * per * pp.nqt), dim3(256), LongCfg<D>::LDS, st, pp);
  HIP_CHECK_RET(hipGetLastError());
  return 0;
}

int launch_attention_long(const AttnP& p, hipStream_t st) {
  if (p.Nk <= 96 || p.Nk > ATTN_LONG_MAX_KEYS) { agd_set_error("attention_long: %d keys (97..%d)", p.Nk, ATTN_LONG_MAX_KEYS); return -1; }
  if (p.record_mode == 3) { agd_set_error("attention_long: head-group sums (record_mode 3) are not recorded beyond 96 keys"); return -1; }
  if (p.record_mode != 1) { agd_set_error("attention_long: record_mode %d (1: per-(image, head) rows)", p.record_mode); return -1; }
  if (p.mask) { agd_set_error("attention_long: recording together with an attention mask is not supported beyond 96 keys"); return -1; }
  if (p.causal || p.k2) { agd_set_error("attention_long: takes no causal order and no second K/V source"); return -1; }
  if (!p.rec || p.rec_T < 1 || p.rec_T > p.Nk || p.rec_b0 < 0 || p.rec_b0 > p.B) { agd_set_error("attention_long: recorder rows rec_T=%d (1..%d), rec_b0=%d (0..%d)", p.rec_T, p.Nk, p.rec_b0, p.B); return -1; }
  if ((p.ldq | p.ldk | p.ldv) & 7) { agd_set_error("attention_long: q/k/v pitches must be multiples of 8 elements"); return -1; }
  if (p.ldo & 3) { agd_set_error("attention_long: row pitches must be multiples of 4 elements"); return -1; }
  // the per-lane byte offsets are 32-bit and reach every key row of the last tile, recorded or not
  if ((unsigned long long)(ATTN_LONG_MAX_KEYS + 64) * (unsigned long long)p.Nq * 4ull > 0xFFFFFFFFull) { agd_set_error("attention_long: %d queries exceed the recorder's 32-bit row offsets", p.Nq); return -1; }
  switch (p.D) {
    case 32: return launch_attn_long_d<32>(p, st);
    case 40: return launch_attn_long_d<40>(p, st);
    case 64: return launch_attn_long_d<64>(p, st);
    case 80: return launch_attn_long_d<80>(p, st);
    case 128: return launch_attn_long_d<128>(p, st);
    case 160: return launch_attn_long_d<160>(p, st);
    default: agd_set_error("attention_long: unsupported head dim %d", p.D); return -1;
  }
}
