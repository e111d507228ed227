// Body of the key-tiled forward kernels of attn_long.hip, included once per kernel: the text between the braces, with STORE_P and
// STATS compile-time constants of the including kernel.  One text, so gt_attn_long_fwd_kernel<true / false> keep the device code
// they had before the STATS variant existed (an inlined shared function changed their register allocation; this does not).
  if (seed_dev) drop_seed ^= *seed_dev;
  __shared__ __attribute__((aligned(16))) bf16_t Vr[2 * 32 * VP];   // V ring: two [32][VP] tiles
  __shared__ __attribute__((aligned(16))) bf16_t Eks[32 * KP];      // rows >= 9 are zero
  __shared__ __attribute__((aligned(16))) bf16_t EvT[D * 16];       // EvT[d][r], r >= 9 zero
  __shared__ __attribute__((aligned(16))) float  QE[4 * 32 * NW];
  __shared__ __attribute__((aligned(16))) bf16_t PB[4 * 32 * 16];

  const int b = blockIdx.z, h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int len = lens[b];
  const size_t rbase = (size_t)gt_row_base(row0, b, Tp) + HALO;
  const int nv1 = gt_row_count(row0, b, Tp) - HALO - 1;          // see gt_attn_fwd_mfma_kernel
  auto RW = [&](int t) { return rbase + (size_t)(t < nv1 ? t : nv1); };

  for (int i = tid; i < 32 * D; i += 256) { const int rr = i / D, c = i - rr * D; Eks[rr * KP + c] = rr < NW ? f2bf(Ek[rr * D + c]) : (bf16_t)0; }
  for (int i = tid; i < D * 16; i += 256) { const int d = i >> 4, rr = i & 15; EvT[i] = rr < NW ? f2bf(Ev[rr * D + d]) : (bf16_t)0; }
  for (int i = tid; i < 4 * 32 * 16; i += 256) PB[i] = 0;
  const int nt = (T + 31) >> 5;                                  // key tiles that hold keys (uniform)
  uint4 vr[2];
  GT_TILE_LOAD(vr, v, ld, 0)
  GT_TILE_STORE(Vr, vr)
  __syncthreads();

  const int i0 = blockIdx.x * 128 + 32 * w;
  const bool active = i0 < T;                                    // wave-uniform
  const int i = i0 + r;
  const int ic = i < T ? i : T - 1;
  float* qe = QE + w * 32 * NW;
  bf16_t* pb = PB + w * 32 * 16;
  const float inv_sqrt = rsqrtf((float)D);

  bf16x8_t qf[6];
#pragma unroll
  for (int ks = 0; ks < 6; ++ks)
    qf[ks] = *reinterpret_cast<const bf16x8_t*>(q + RW(ic) * ld + h * D + ks * 16 + 8 * hh);
  if (active) {
    f32x16_t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) {
      const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(Eks + r * KP + ks * 16 + 8 * hh);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, qf[ks], acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) qe[r * NW + e + 4 * hh] = acc[e];
    if (hh == 0) qe[r * NW + 8] = acc[4];
  }
  __builtin_amdgcn_wave_barrier();

  // K fragments of key tile t: lane (key r of the tile, k-half hh); rows >= T are zero
  auto load_k = [&](int t, bf16x8_t* kf) {
    const int j = 32 * t + r;
    if (j < T) {
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) kf[ks] = *reinterpret_cast<const bf16x8_t*>(k + RW(j) * ld + h * D + ks * 16 + 8 * hh);
    } else {
      const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) kf[ks] = __builtin_bit_cast(bf16x8_t, z);
    }
  };
  // masked, scaled scores of one tile (element e <-> key 32t + (e&3) + 8(e>>2) + 4hh)
  auto scores = [&](int t, const bf16x8_t* kf, f32x16_t& st) {
#pragma unroll
    for (int e = 0; e < 16; ++e) st[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 6; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], st, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int j = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
      float sc = st[e];
      const int rel = j - i + WIN;
      if ((unsigned)rel <= 2u * WIN) sc += qe[r * NW + rel];
      sc *= inv_sqrt;
      if (j >= T) sc = -3.0e38f;                                 // not a key at all
      else if (j >= len || i >= len) sc = -1e4f;                 // masked_fill(mask == 0, -1e4), attentions.py:260
      st[e] = sc;
    }
  };

  // ---- pass 1 (no LDS operand, no barrier): online max / denominator over this lane's keys, then the lane halves merge
  float mx = -3.0e38f, den = 0.f;
  bf16x8_t kf[6], kn[6];
  if (active) {
    load_k(0, kf);
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      if (t + 1 < nt) load_k(t + 1, kn);
      f32x16_t st;
      scores(t, kf, st);
      float tm = st[0];
#pragma unroll
      for (int e = 1; e < 16; ++e) tm = fmaxf(tm, st[e]);
      const float mn = fmaxf(mx, tm);
      float add = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) add += __expf(st[e] - mn);
      den = den * __expf(mx - mn) + add;
      mx = mn;
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) kf[ks] = kn[ks];
    }
    const float mo = __shfl_xor(mx, 32), dn = __shfl_xor(den, 32);
    const float mm = fmaxf(mx, mo);
    den = den * __expf(mx - mm) + dn * __expf(mo - mm);
    mx = mm;
  }
  const float rden = active ? 1.0f / den : 0.f;
  if (STATS && active && hh == 0 && i < T)                        // every query row, padded ones included
    *reinterpret_cast<float2*>(Pout + (((size_t)b * H + h) * T + i) * 2) = make_float2(mx, rden);

  // ---- pass 2: P = softmax, dropout, O^T = V^T P^T (+ Ev^T band(P)^T); V tile t in ring slot t & 1
  float* prow = STORE_P ? Pout + (((size_t)b * H + h) * T + ic) * T : nullptr;
  const uint32_t drow = (uint32_t)((b * H + h) * T + i);
  const int li = lane & 15, qd = li >> 2, pp = li & 3, colhalf = ((lane >> 4) & 1) * 16;
  const bool vec = (T & 3) == 0;
  f32x16_t o[3];
#pragma unroll
  for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  }
  if (active) load_k(0, kf);
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      GT_TILE_LOAD(vr, v, ld, t + 1)
      if (active) load_k(t + 1, kn);
    }
    if (active) {
      const bf16_t* Vs = Vr + (t & 1) * 32 * VP;
      f32x16_t st;
      scores(t, kf, st);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int j0 = 32 * t + 8 * g + 4 * hh;
        float p4[4];
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) p4[e2] = __expf(st[4 * g + e2] - mx) * rden;
        if (STORE_P && i < T) {
          if (vec && j0 + 3 < T) *reinterpret_cast<float4*>(prow + j0) = make_float4(p4[0], p4[1], p4[2], p4[3]);
          else {
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) if (j0 + e2 < T) prow[j0 + e2] = p4[e2];
          }
        }
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
          const int j = j0 + e2;
          float pd = p4[e2];
          if (drop_thresh) pd = drop_keep(drop_seed, drow, j, drop_thresh) ? pd * drop_scale : 0.f;
          st[4 * g + e2] = pd;
          const int rel = j - i + WIN;
          if ((unsigned)rel <= 2u * WIN && j < T) pb[r * 16 + rel] = f2bf(pd);
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float f8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f8[e] = st[8 * s2 + e];
        const bf16x8_t pf = pack8(f8);
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) {
          const bf16_t* va = Vs + (16 * s2 + 4 * hh + qd) * VP + 32 * dt + colhalf + 4 * pp;
          const bf16x8_t af = tr_frag8(va, va + 8 * VP);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, pf, o[dt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 6; ++ks) kf[ks] = kn[ks];
    }
    if (t + 1 < nt) { GT_TILE_STORE(Vr + ((t + 1) & 1) * 32 * VP, vr) }
    __syncthreads();
  }
  if (!active) return;
  {
    const bf16x8_t bfp = *reinterpret_cast<const bf16x8_t*>(pb + r * 16 + 8 * hh);      // band(P)^T: k = rel
#pragma unroll
    for (int dt = 0; dt < 3; ++dt) {
      const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(EvT + (32 * dt + r) * 16 + 8 * hh);
      o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfp, o[dt], 0, 0, 0);
    }
  }
  if (i < T && i <= nv1) {
#pragma unroll
    for (int dt = 0; dt < 3; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = 32 * dt + 8 * g + 4 * hh;
        *reinterpret_cast<uint2*>(out + (rbase + i) * ldo + h * D + d) =
            make_uint2(pack2bf(o[dt][4 * g], o[dt][4 * g + 1]), pack2bf(o[dt][4 * g + 2], o[dt][4 * g + 3]));
      }
  }
