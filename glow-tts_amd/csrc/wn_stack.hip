// A whole WaveNet (all n = 4 gated layers of modules.WN.forward, modules.py:144-171) as ONE kernel, gfx950.
//
// csrc/wn_layer.hip runs one kernel per layer: a workgroup owns 64 rows and all channels, and between two layers every row
// tile needs 2 rows of its neighbours (k = 5), which is why the layers are separate launches (~2.5 us of launch gap, the first
// tile's load latency and the store drain at the kernel boundary per layer, on the decoder's dependent chain).  Here a workgroup
// RECOMPUTES that halo instead of exchanging it: it loads 68 rows of the WaveNet's input, computes layer 0 on 64 rows, layer 1
// is then exact on the inner 60, layer 2 on 56, layer 3 on 52 — the workgroup OWNS those 52 rows and stores only them; tiles
// advance by 52 rows (9 216..9 728 rows of cfg 2 -> 178..188 workgroups instead of 144..152: the extra 23 % of arithmetic runs on
// CUs that were idle).  The layer's input never leaves LDS ([68][192] bf16, ping-pong), the k=5 conv needs no K-slice staging
// and no barrier in its loop, and x_{i+1} is stored (for the weight gradients / the backward) without anyone waiting for it.
// A halo row is computed by two workgroups with the same arithmetic in the same order and the same dropout hash (seed, global
// row, column): what they produce is bit-identical, so the result equals the per-layer kernels' bit for bit.
//
// Per layer (as wn_layer.hip): stage 1  x_in = conv_k5(x): N = 384, K = 960; 4 waves x (64 rows x 96 columns); weights as MFMA-A
// fragments L2 -> registers (3-step ring), activations = MFMA-B from the LDS tile; gate epilogue in registers (bias, dropout,
// cond, tanh * sigmoid; T, S, acts -> HBM for the owned rows, acts -> LDS); stage 2  x_next = (x + acts @ W_res^T + b) * mask.
#include "common.h"
#include "internal.h"
#include "mfma_frag.h"
#include "../../include/glowtts_hip.h"

namespace {

constexpr int H = 192, TAPS = 5, NLMAX = 4;
constexpr int BM = 64;                        // rows computed per layer
constexpr int AP = H + 8;                     // LDS pitch (halfs): 400 B = 16 mod 128 -> conflict-free ds_read_b128
constexpr int XR = BM + TAPS - 1;             // 68 input rows
// Weight ring depths.  64-row form: forward 3 steps, backward 2 * 3 - 1 = 5 (half the fragments per step: twice the depth for the
// same registers).  Measured and settled (round 3) for the
// 32-row form (NBM = 1), whose spare accumulator registers could pay for deeper rings, at 5 120 rows: forward 56.6 / 58.4 / 58.4 us
// at depth 4 / 5 / 3, backward 73.7 / 68.2 us at depth 9 / 5 — what the 256 workgroups wait for is the L2 itself (each streams
// all 3.2 MB of weights: 0.8 GB per launch), not a ring step's round trip: the 32-row form keeps the 64-row depths.
constexpr int RING = 3, RING1 = RING;
constexpr int RB = 2 * RING - 1, RB1 = RB;
// Barriers are __syncthreads() (vmcnt(0) as well as lgkmcnt(0)).  One that waits for LDS traffic only measured (round 3, back to
// back) backward 86.6 us either way, forward 71.2 vs 67.9 us: the activation stores then sit in front of the next layer's weight
// loads on the in-order vmcnt counter and stall the conv loop instead of the barrier.
#ifndef WNS_PHASES
#define WNS_PHASES 0                          // dev: per-phase shader-clock stamps of wave 0 (tools/wn_stack_phases.py), 0 in every build that ships
#endif
#if WNS_PHASES
// [1024 workgroups][48] of wave 0, then (8-wave backward only) the same of wave 4, its SIMD partner
__device__ unsigned long long g_wns_ph[2 * 1024 * 48];
#define PH(i) do { if ((threadIdx.x == 0 || threadIdx.x == 256) && blockIdx.x < 1024)                                                \
                     g_wns_ph[((threadIdx.x >> 8) * 1024 + blockIdx.x) * 48 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define PH(i) do { } while (0)
#endif
constexpr int KK2 = H / 16;
constexpr int STACK_LDS = (2 * XR + BM) * AP * 2;                       // Xa, Xb [68][200] + At [64][200] = 80 000 B
constexpr int FWD_BIAS_FLOATS = NLMAX * 2 * H + (NLMAX - 1) * H;        // every layer's biases, staged once (see the forward kernel)
constexpr int FWD_AFF_FLOATS = 2 * NLMAX * H;                            // affine conditioning (COND == 2): w | b of cond_layer1, H * n each
constexpr int STACK_FWD_LDS = STACK_LDS + 2 * BM * AP * 2 + FWD_BIAS_FLOATS * 4;   // forward: + the saved tanh / sigmoid tiles [64][200] each + biases = 139 648 B
constexpr int STACK_FWD_LDS_AFF = STACK_FWD_LDS + FWD_AFF_FLOATS * 4;              // + 6 144 B
constexpr int CPR = H / 8;                                              // 16-byte chunks per row

// A pointer the optimiser cannot see through: the 180 fragment addresses of a layer depend only on a kernel argument and the
// lane, so LLVM hoists them to the kernel's entry block — 360 registers that then live (spilled) across every earlier layer.
template <typename T>
__device__ __forceinline__ const T* pinned(const T* p) { asm volatile("" : "+s"(p)); return p; }
// The wave index as a SCALAR that is a fresh value wherever it is asked for: the fragment offsets (functions of the wave's
// column / K share) are then scalar arithmetic next to each load (SGPR base + 32-bit lane offset addressing) instead of ~180
// vector values that common-subexpression elimination keeps alive from one layer to the next.
__device__ __forceinline__ int wave_scalar()
{
  int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  asm volatile("" : "+s"(w));
  return w;
}

template <typename T>
__device__ __forceinline__ T pick(T const (&arr)[NLMAX], int i)        // scalar selects: no dynamically indexed kernarg copy
{
  return i == 0 ? arr[0] : (i == 1 ? arr[1] : (i == 2 ? arr[2] : arr[3]));
}

// The forward keeps a RUNTIME layer loop: the compiler then forms the layer's 180 fragment offsets once (hoisted out of the loop,
// parked in the accumulation registers the MFMAs do not use) — measured 8 % faster than the straight-line, scalar-addressed form
// the backward kernel needs (its register budget has no room for them).
// COND / DROP are compile-time: as run-time (uniform) branches around the conditioning loads and the dropout hashes they cost a
// branch per element and a conservative `s_waitcnt vmcnt(0)` at every join.
// COND: 0 none; 1 rows of a cond tensor (per utterance: the speaker vector through cond_layer; or per row); 2 AFFINE per-frame
// conditioning formed here: modules.WNP (modules.py:316-343) conditions on cond_layer1(contour), a conv with ONE input channel —
// w[c] * contour[t] + b[c] — squeezed in time (modules.py:353-362): squeezed row m, column parity * O + c (O = H n) holds
// w[c] * contour[2 m + parity] + b[c], and layer i reads columns [2H i, 2H (i+1)).  Materialised, that is 6 KB of fp32 per row written
// by a host-side op and read back here; formed from the row's two contour values and the 2 x O parameters it is 8 bytes per row.
// NBM: 32-row blocks computed per layer — 2 (64-row tiles, 52 owned with 4 layers) or 1 (32-row tiles, 20 owned) for launches whose
// 64-row tiles would leave most of the chip idle (cfg 4 / cfg 5's 4-5 k rows: 90 workgroups on 256 CUs): 2.6 x the workgroups, each
// with half the MFMA rows but the same weight stream.  The LDS layout is the 64-row one either way; every row's arithmetic (K order,
// dropout hash, epilogue) is the same, so the results are bit-identical between the two forms.
// SAVE: the saved tanh / sigmoid halves and every x_i go to HBM for a backward (training); false = synthesis: acts only (the tiles
// those outputs pass through are then never written).  Built for COND 0 / 1 without dropout, where the arithmetic that produces acts
// compiles to the same instructions either way (equality is tested).  NOT built for COND == 2: whether `b + contour * w` becomes one
// fused operation or a multiply and an add is the compiler's choice per instantiation, and an acts-only <2, false, 2> differed from
// the saving one in the last bf16 bit of 16 of 4.9 M acts — the affine WaveNets of a synthesis pass run the saving kernel.
template <int COND, bool DROP, int NBM, bool SAVE = true>
__global__ __launch_bounds__(256) void gt_wn_stack_fwd_kernel(gt_wn_stack_fwd_args a, uint32_t drop_thresh, float drop_scale)
{
  constexpr int BMv = 32 * NBM, XRv = BMv + TAPS - 1;
  constexpr int RINGv = NBM == 1 ? RING1 : RING;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // (an atomicMin here, 188 workgroups on one address, sat in front of every weight fragment's wait)
  const unsigned long long t_begin = stamp_begin(a);
  PH(0);
  const uint32_t seed_x = a.seed_dev ? *a.seed_dev : 0u;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int n_layers = a.n_layers, R = a.R;
  const int halo = 2 * (n_layers - 1);                               // rows lost per side: 6 for 4 layers
  const int own = BMv - 2 * halo;                                    // rows this workgroup owns: 52 (NBM = 2) or 20
  const int s0 = blockIdx.x * own - halo;                            // global row of tile row 0
  bf16_t* Xc = reinterpret_cast<bf16_t*>(smem);
  bf16_t* Xn = Xc + XR * AP;
  bf16_t* At = Xn + XR * AP;
  bf16_t* Tl = At + BM * AP;                                         // saved tanh / sigmoid halves on their way out (see the gate epilogue)
  bf16_t* Sl = Tl + BM * AP;
  // Every layer's biases live in LDS from the start: read from global memory inside the epilogues (two float4 per 4 gate channels,
  // each waited for where it is used) they cost a full L2 round trip per (column block, channel group) — 5 k of a layer's 12 k
  // epilogue cycles (tools/wn_stack_phases.py).
  float* Bs = reinterpret_cast<float*>(Sl + BM * AP);                // [n][2H] in_layer biases | [n-1][H] residual biases
  constexpr int KS = H / 16, NBT = 2 * H / 32, NIT = 3 * TAPS;       // 12 k-steps per tap, 12 column blocks, 15 steps of 4 k-steps

  // Vector-memory operations retire IN ORDER on one counter (vmcnt): a wait for a weight fragment also waits for every store issued
  // before that load.  So the loads a layer needs first are issued BEFORE the stores that precede their use: the next layer's first
  // ring steps ahead of the T / S / acts / x_next stores, and layer 0's here, ahead of (and overlapping) the input tile's loads.
  uint4 ring[RINGv][4][3];
  float rm2;
  // Fragment addresses are left to the compiler: it forms the layer's per-lane offsets once, outside the layer loop, and every load
  // is then ONE instruction with an immediate offset.  Measured against scalar bases formed next to each load (`pinned`, as the
  // backward needs for its register budget: + 7 us per launch — one wave per SIMD issues in order, so every scalar instruction in
  // front of a load is time the matrix pipe idles), against buffer loads with the descriptor in SGPRs (+ 2.5 us), and against
  // pinning each load between two MFMAs (sched_group_barrier: + 5 us — a vector-memory instruction holds the wave's issue for
  // longer than the MFMA it was meant to hide behind): tools/stack_variants.sh, round 3.
  auto w_frag = [&](const bf16_t* W, int it, int ks, int bn) {
    const int kg = it / TAPS, tap = it - kg * TAPS;
    return ldfrag_global(W, (tap * NBT + 3 * wave + bn) * KS + kg * 4 + ks, lane);
  };
  auto w_load_l = [&](const bf16_t* W, int it, uint4 (&dst)[4][3]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int bn = 0; bn < 3; ++bn) dst[ks][bn] = w_frag(W, it, ks, bn);
  };
  // layer-0 input: rows s0 - 2 .. s0 + 65, all 192 channels (rows outside [0, R) read as zero); every layer's biases; the row
  // mask of the one row this lane finishes in every residual stage (32 * (wave >> 1) + r).  All of these loads are issued first,
  // then layer 0's first ring steps (a wait for the tile must not wait for the weights behind it), then the LDS writes.
  {
    const bf16_t* x0 = static_cast<const bf16_t*>(a.x0);
    constexpr int NX = (XR * CPR + 255) / 256, NB = (FWD_BIAS_FLOATS / 4 + 255) / 256;   // 7 and 3 per thread
    uint4 xin[NX];
    float4 bin[NB];
    float4 ain[(FWD_AFF_FLOATS / 4 + 255) / 256];
    if (COND == 2) {
      const int O = H * n_layers;
#pragma unroll
      for (int i = 0; i < (FWD_AFF_FLOATS / 4 + 255) / 256; ++i) {
        const int idx = threadIdx.x + 256 * i;                       // [w (O) | b (O)] as float4
        ain[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (idx < O / 4) ain[i] = reinterpret_cast<const float4*>(a.aff_w)[idx];
        else if (idx < 2 * O / 4) ain[i] = reinterpret_cast<const float4*>(a.aff_b)[idx - O / 4];
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int chunk = threadIdx.x + 256 * i, u = chunk / CPR, c8 = chunk - u * CPR, gm = s0 - 2 + u;
      xin[i] = make_uint4(0, 0, 0, 0);
      if (u < XRv && gm >= 0 && gm < R) xin[i] = *reinterpret_cast<const uint4*>(x0 + (size_t)gm * H + c8 * 8);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = threadIdx.x + 256 * i;
      bin[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (idx < NLMAX * 2 * H / 4) {
        const int l = idx / (2 * H / 4), o = idx - l * (2 * H / 4);
        if (l < n_layers) bin[i] = reinterpret_cast<const float4*>(pick(a.b_in, l))[o];
      } else if (idx < FWD_BIAS_FLOATS / 4) {
        const int q = idx - NLMAX * 2 * H / 4, l = q / (H / 4), o = q - l * (H / 4);
        if (l < n_layers - 1) bin[i] = reinterpret_cast<const float4*>(pick(a.b_res, l))[o];
      }
    }
    {
      const int m = s0 + 32 * (wave >> 1) + r;
      rm2 = (m >= 0 && m < R) ? a.rowmask[m] : 0.0f;
    }
    {
      const bf16_t* W10 = static_cast<const bf16_t*>(a.w_in[0]);
#pragma unroll
      for (int p = 0; p < RINGv - 1; ++p) w_load_l(W10, p, ring[p]);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int chunk = threadIdx.x + 256 * i, u = chunk / CPR, c8 = chunk - u * CPR;
      if (u < XRv) *reinterpret_cast<uint4*>(Xc + u * AP + c8 * 8) = xin[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = threadIdx.x + 256 * i;
      if (idx < FWD_BIAS_FLOATS / 4) reinterpret_cast<float4*>(Bs)[idx] = bin[i];
    }
    if (COND == 2) {
#pragma unroll
      for (int i = 0; i < (FWD_AFF_FLOATS / 4 + 255) / 256; ++i) {
        const int idx = threadIdx.x + 256 * i;
        if (idx < 2 * H * n_layers / 4) reinterpret_cast<float4*>(Bs + FWD_BIAS_FLOATS)[idx] = ain[i];
      }
    }
    if (threadIdx.x < 4 * 24) {                                       // the next tile's rows 0, 1, 66, 67 are never produced
      const int q = threadIdx.x / 24, c8 = threadIdx.x - q * 24, u = q < 2 ? q : XRv - 4 + q;
      *reinterpret_cast<uint4*>(Xn + u * AP + c8 * 8) = make_uint4(0, 0, 0, 0);
    }
  }
  __syncthreads();
  PH(1);

  // per-utterance conditioning: the utterance of this lane's two rows (one binary search each, once per launch)
  int cb[NBM] = {};
  float sg[NBM][2] = {};                          // COND == 2: the two contour values (even / odd frame) of this lane's two rows
  if (COND == 1) {
#pragma unroll
    for (int bm = 0; bm < NBM; ++bm) {
      const int m = s0 + 32 * bm + r, mc = m < 0 ? 0 : (m >= R ? R - 1 : m);
      cb[bm] = a.B > 0 ? gt_row_batch(a.row0, a.B, mc, a.Tp) : mc;
    }
  }
  if (COND == 2) {
#pragma unroll
    for (int bm = 0; bm < NBM; ++bm) {
      const int m = s0 + 32 * bm + r;
      if (m >= 0 && m < R) { const float2 v = *reinterpret_cast<const float2*>(a.aff_sig + 2 * (size_t)m); sg[bm][0] = v.x; sg[bm][1] = v.y; }
    }
  }

  for (int layer = 0; layer < n_layers; ++layer) {
    const bool last = layer == n_layers - 1;
    const bf16_t* W1 = static_cast<const bf16_t*>(pick(a.w_in, layer));
    const bf16_t* W2 = static_cast<const bf16_t*>(pick(a.w_res, layer));
    const float* bias1 = Bs + layer * 2 * H;
    const float* bias2 = Bs + NLMAX * 2 * H + layer * H;
    bf16_t* Tt = static_cast<bf16_t*>(pick(a.gate_t, layer));
    bf16_t* Ss = static_cast<bf16_t*>(pick(a.gate_s, layer));
    bf16_t* xo = static_cast<bf16_t*>(pick(a.x_out, layer));
    const uint32_t seed = (a.drop_seed + (uint32_t)layer) ^ seed_x;

    f32x16_t acc[3][NBM];
    acc_zero(acc);

    auto w_load = [&](int it, uint4 (&dst)[4][3]) { w_load_l(W1, it, dst); };
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int kg = it / TAPS, tap = it - kg * TAPS;
      w_load(it + RINGv - 1 < NIT ? it + RINGv - 1 : NIT - 1, ring[(it + RINGv - 1) % RINGv]);
      __builtin_amdgcn_sched_barrier(0);       // keep the prefetch RINGv - 1 steps ahead
      const bf16_t* xsb = Xc + (r + tap) * AP + 8 * h + kg * 64;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        bf16x8_t bx[NBM];
#pragma unroll
        for (int bm = 0; bm < NBM; ++bm) bx[bm] = *reinterpret_cast<const bf16x8_t*>(xsb + 32 * bm * AP + ks * 16);
#pragma unroll
        for (int bn = 0; bn < 3; ++bn)
#pragma unroll
          for (int bm = 0; bm < NBM; ++bm)
            acc[bn][bm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(asfrag(ring[it % RINGv][ks][bn]), bx[bm], acc[bn][bm], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }

    PH(2 + 6 * layer);
    // the thread index as a value formed HERE: the copy loops' per-thread addresses and the epilogue's 24 per-channel hash bases
    // are otherwise computed in front of the layer loop and carried (spilled) across the K loops
    int tid_e = threadIdx.x;
    asm volatile("" : "+v"(tid_e));
    const int r_e = tid_e & 31, h_e = (tid_e >> 5) & 1, wave_e = tid_e >> 6;
    // second-stage weights start flying now, under the gate epilogue
    const int wn2 = wave & 1, wm2 = wave >> 1;
    const bool st2 = wm2 < NBM;                // the residual stage's 2 x 2 waves are (row block, column half): NBM = 1 leaves two of them out
    constexpr int R2 = KK2 / 2;
    uint4 ring2[R2][3];
    if (!last && st2) {
#pragma unroll
      for (int kk = 0; kk < R2; ++kk)
#pragma unroll
        for (int bn = 0; bn < 3; ++bn) ring2[kk][bn] = ldfrag_global(W2, (3 * wn2 + bn) * KK2 + kk, lane);
    }

    // gate epilogue in registers (see wn_layer.hip): block 3*wave + bn holds [16 tanh | 16 sigmoid] of channels 16*(3*wave+bn)..+15
    bf16_t* acts = static_cast<bf16_t*>(a.acts) + layer * H;
    const float* cond = COND == 1 ? a.cond + (size_t)layer * 2 * H : nullptr;
    // affine conditioning of this layer: column 2H * layer of the squeezed cond_layer1 output = parity par, parameters off ..
    const int aff_O = H * n_layers, aff_par = (2 * H * layer) / aff_O, aff_off = (2 * H * layer) - aff_par * aff_O;
    const float* Aw = Bs + FWD_BIAS_FLOATS + aff_off;
    const float* Ab = Aw + aff_O;
#pragma unroll
    for (int bn = 0; bn < 3; ++bn)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int c = 16 * (3 * wave_e + bn) + 8 * g + 4 * h_e;
        const float4 bt = *reinterpret_cast<const float4*>(bias1 + c), bs = *reinterpret_cast<const float4*>(bias1 + H + c);
        const float btv[4] = {bt.x, bt.y, bt.z, bt.w}, bsv[4] = {bs.x, bs.y, bs.z, bs.w};
#pragma unroll
        for (int bm = 0; bm < NBM; ++bm) {
          const int t = 32 * bm + r_e, m = s0 + t;
          float ctv[4] = {}, csv[4] = {};
          if (COND == 1) {
            const float* cp = cond + (size_t)cb[bm] * a.ldc + c;
            const float4 ct = *reinterpret_cast<const float4*>(cp), cs = *reinterpret_cast<const float4*>(cp + H);
            ctv[0] = ct.x; ctv[1] = ct.y; ctv[2] = ct.z; ctv[3] = ct.w; csv[0] = cs.x; csv[1] = cs.y; csv[2] = cs.z; csv[3] = cs.w;
          }
          if (COND == 2) {
            const float pv = aff_par ? sg[bm][1] : sg[bm][0];
            const float4 wt = *reinterpret_cast<const float4*>(Aw + c), ws = *reinterpret_cast<const float4*>(Aw + H + c);
            const float4 bt2 = *reinterpret_cast<const float4*>(Ab + c), bs2 = *reinterpret_cast<const float4*>(Ab + H + c);
            // torch.addcmul(b, contour, w) of the host-side form: b + contour * w, one rounding each way it is written
            ctv[0] = bt2.x + pv * wt.x; ctv[1] = bt2.y + pv * wt.y; ctv[2] = bt2.z + pv * wt.z; ctv[3] = bt2.w + pv * wt.w;
            csv[0] = bs2.x + pv * ws.x; csv[1] = bs2.y + pv * ws.y; csv[2] = bs2.z + pv * ws.z; csv[3] = bs2.w + pv * ws.w;
          }
          float tt[4], ss[4], aa[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float vt = acc[bn][bm][4 * g + j] + btv[j], vs = acc[bn][bm][4 * g + j + 8] + bsv[j];
            if (DROP) {                              // x_in = drop(conv(x)) (modules.py:153)
              bool kt, ks;
              drop_keep_gate(seed, m, c + j, drop_thresh16(drop_thresh), kt, ks);
              vt = kt ? vt * drop_scale : 0.0f;
              vs = ks ? vs * drop_scale : 0.0f;
            }
            vt += ctv[j]; vs += csv[j];
            tt[j] = tanhf_(vt); ss[j] = sigmoidf_(vs); aa[j] = tt[j] * ss[j];
          }
          // T, S and acts leave through LDS: straight from the MFMA layout a store instruction writes 16 bytes to each of 32
          // rows (2.6 M partial-line requests per launch, the "17 us of stores" of DESIGN 4.9); the tiles below go out as whole rows
          if (SAVE) {
            *reinterpret_cast<uint2*>(Tl + t * AP + c) = pack4(tt[0], tt[1], tt[2], tt[3]);
            *reinterpret_cast<uint2*>(Sl + t * AP + c) = pack4(ss[0], ss[1], ss[2], ss[3]);
          }
          *reinterpret_cast<uint2*>(At + t * AP + c) = pack4(aa[0], aa[1], aa[2], aa[3]);
        }
      }
    PH(3 + 6 * layer);
    __syncthreads();                                                   // At, Tl, Sl complete
    PH(4 + 6 * layer);
    auto store_gate_tiles = [&]() {
      // the rows this workgroup owns are ONE contiguous block of T / S (and 384-byte pieces of the acts rows): 16 bytes per lane,
      // consecutive lanes on consecutive addresses; all the LDS reads first, then the stores (as a rolled loop every chunk paid its
      // own LDS round trip)
      constexpr int NC = (BM * CPR + 255) / 256, NP = 2;               // <= 6 chunks per thread and tile, in passes of NP
#pragma unroll 1
      for (int i0 = 0; i0 < NC; i0 += NP) {
        uint4 vt[NP], vs[NP], va[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int idx = tid_e + 256 * (i0 + i), row = idx / CPR, c8 = idx - row * CPR, t = halo + row;
          vt[i] = vs[i] = va[i] = make_uint4(0, 0, 0, 0);
          if (idx < own * CPR) {
            if (SAVE) { vt[i] = *reinterpret_cast<const uint4*>(Tl + t * AP + c8 * 8); vs[i] = *reinterpret_cast<const uint4*>(Sl + t * AP + c8 * 8); }
            va[i] = *reinterpret_cast<const uint4*>(At + t * AP + c8 * 8);
          }
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int idx = tid_e + 256 * (i0 + i), row = idx / CPR, c8 = idx - row * CPR, m = s0 + halo + row;
          if (idx < own * CPR && m < R) {
            if (SAVE) {
              *reinterpret_cast<uint4*>(Tt + (size_t)m * H + c8 * 8) = vt[i];
              *reinterpret_cast<uint4*>(Ss + (size_t)m * H + c8 * 8) = vs[i];
            }
            *reinterpret_cast<uint4*>(acts + (size_t)m * a.ldacts + c8 * 8) = va[i];
          }
        }
      }
    };
    if (last) store_gate_tiles();
    if (last) break;

    // stage 2: x_next = (x + acts @ W_res^T + b_res) * mask -> the next layer's LDS tile (+ HBM for the owned rows)
    f32x16_t acc2[3];
    acc_zero(acc2);
    if (st2) {
      const bf16_t* ab = At + (32 * wm2 + r) * AP + 8 * h;
#pragma unroll
      for (int kk = 0; kk < KK2; ++kk) {
        const bf16x8_t bfm = *reinterpret_cast<const bf16x8_t*>(ab + kk * 16);
#pragma unroll
        for (int bn = 0; bn < 3; ++bn) {
          acc2[bn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(asfrag(ring2[kk % R2][bn]), bfm, acc2[bn], 0, 0, 0);
          if (R2 < KK2 && kk + R2 < KK2) ring2[kk % R2][bn] = ldfrag_global(W2, (3 * wn2 + bn) * KK2 + kk + R2, lane);
        }
      }
    }
    PH(5 + 6 * layer);
    {                                          // the next layer's first ring steps, ahead of the x_next stores
      const bf16_t* W1n = static_cast<const bf16_t*>(pick(a.w_in, layer + 1));
#pragma unroll
      for (int p = 0; p < RINGv - 1; ++p) w_load_l(W1n, p, ring[p]);
    }
    store_gate_tiles();                        // T, S, acts: the tiles are untouched until the next layer's epilogue
    if (st2) {
      const int t = 32 * wm2 + r;
      const float rm = rm2;
#pragma unroll
      for (int bn = 0; bn < 3; ++bn)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = 32 * (3 * wn2 + bn) + 8 * g + 4 * h;
          const float4 b2 = *reinterpret_cast<const float4*>(bias2 + n);
          float xv[4];
          unpack4(*reinterpret_cast<const uint2*>(Xc + (t + 2) * AP + n), xv);
          const uint2 v = pack4((acc2[bn][4 * g] + b2.x + xv[0]) * rm, (acc2[bn][4 * g + 1] + b2.y + xv[1]) * rm,
                                (acc2[bn][4 * g + 2] + b2.z + xv[2]) * rm, (acc2[bn][4 * g + 3] + b2.w + xv[3]) * rm);
          *reinterpret_cast<uint2*>(Xn + (t + 2) * AP + n) = v;
        }
    }
    __syncthreads();                                                   // the next layer's input is complete; Xc and At are free
    PH(6 + 6 * layer);
    bf16_t* tmp = Xc; Xc = Xn; Xn = tmp;
    if (SAVE) {                                                      // x_next of the owned rows, whole rows from the finished tile
      constexpr int NC = (BM * CPR + 255) / 256, NP = 3;
#pragma unroll 1
      for (int i0 = 0; i0 < NC; i0 += NP) {
        uint4 vx[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int idx = tid_e + 256 * (i0 + i), row = idx / CPR, c8 = idx - row * CPR;
          vx[i] = make_uint4(0, 0, 0, 0);
          if (idx < own * CPR) vx[i] = *reinterpret_cast<const uint4*>(Xc + (halo + row + 2) * AP + c8 * 8);
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int idx = tid_e + 256 * (i0 + i), row = idx / CPR, c8 = idx - row * CPR, m = s0 + halo + row;
          if (idx < own * CPR && m < R) *reinterpret_cast<uint4*>(xo + (size_t)m * H + c8 * 8) = vx[i];
        }
      }
    }
    if (threadIdx.x < 4 * 24) {                                        // rows 0, 1, 66, 67 of the tile after next
      const int q = threadIdx.x / 24, c8 = threadIdx.x - q * 24, u = q < 2 ? q : XRv - 4 + q;
      *reinterpret_cast<uint4*>(Xn + u * AP + c8 * 8) = make_uint4(0, 0, 0, 0);
    }
    PH(7 + 6 * layer);
  }
  PH(40);
  stamp_end(a, t_begin);
}

// ------------------------------------------------------------------------------------------------ backward
// The mirror: the gate backward of the top layer (row-local, from the skip-path gradient), then for j = n-1 .. 0 the k=5 data
// gradient of in_layer_j on the d pre_j tile -> dX_j (+ the residual-path gradient dX_{j+1}, * mask), and below it the
// residual 1x1's data gradient + skip-path gradient + gate backward -> d pre_{j-1}.  The first conv reads an exact 68-row
// tile, each of the other n-1 loses 2 rows per side: the workgroup owns the same 64 - 4 (n-1) rows as the forward.
//   stage 1: N = 192, K = 5 * 384: 12 accumulation streams (6 blocks of 32 columns x 2 K parities, all rows of the tile), 3 per SIMD;
//            the partial sums of the two parities are exchanged through LDS
//   stage 2: N = 192, K = 192 on the dX tile: per SIMD (row half, column half) = 32 rows x 96 columns
// 512 threads, 8 waves, two per SIMD (the LDS tiles allow one workgroup per CU).  Waves w and w + 4 (SIMD partners in practice)
// split their SIMD's 3 column blocks 2 + 1: wave w takes blocks 0, 1 of the SIMD's column half, wave w + 4 block 2, both on the same
// K parity, so one LDS operand read feeds 2 blocks and every weight fragment is still fetched ONCE per workgroup (a row-block split
// would fetch each fragment twice: the L2 -> VGPR weight stream costs as much vector-memory issue as the MFMAs, wn_layer.hip).  Every
// output element is the same MFMA chain in the same order as with 4 waves (and as the per-layer kernels): bit-identical results.
// Each wave then fits in 256 VGPR + AGPR; with one wave per SIMD nothing hid the exchange, the epilogues or the copy loops.  Measured at
// cfg 2's rows (tools/wn_layer_bench.py stack, back to back): 88.1 -> 74.5-75.2 us per launch; in the step 90.0 -> 74.4 us.
constexpr int BWD_THREADS = 512;
constexpr int DP = 2 * H + 8;                 // d pre tile pitch (halfs): 784 B = 16 mod 128
constexpr int EX_BYTES = 4 * 3 * 16 * 64 * 4; // partial-sum exchange [4 SIMDs][3 blocks][16][64 lanes] fp32: aliases the d pre tile
constexpr int BWD_DT = XR * DP * 2;           // 53 312 B
static_assert(EX_BYTES <= BWD_DT, "the exchange buffer lives in the d pre tile");
constexpr int SBWD_LDS = BWD_DT + 4 * BM * AP * 2;       // d pre tile | dX tile | skip-gradient, tanh, sigmoid staging tiles = 155 712 B

template <bool DROP>
__device__ __forceinline__ void gate_bwd4(const float (&dd)[4], const float (&t)[4], const float (&s)[4], uint32_t seed, int m, int n,
                                          uint32_t thresh, float scale, uint2& pt, uint2& ps, uint2& ct, uint2& cs)
{
  float gt[4], gs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { gt[j] = dd[j] * s[j] * (1.0f - t[j] * t[j]); gs[j] = dd[j] * t[j] * s[j] * (1.0f - s[j]); }
  ct = pack4(gt[0], gt[1], gt[2], gt[3]); cs = pack4(gs[0], gs[1], gs[2], gs[3]);      // before the dropout mask: d cond
  if (DROP) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bool kt, ks;
      drop_keep_gate(seed, m, n + j, drop_thresh16(thresh), kt, ks);
      gt[j] = kt ? gt[j] * scale : 0.0f;
      gs[j] = ks ? gs[j] * scale : 0.0f;
    }
  }
  pt = pack4(gt[0], gt[1], gt[2], gt[3]); ps = pack4(gs[0], gs[1], gs[2], gs[3]);
}

constexpr int B_NS = 2 * H / 64, B_NIT = B_NS * TAPS, B_KS = 2 * H / 16, B_NBT = H / 32;  // 6 slices, 30 steps, 24 k-steps per tap, 6 blocks

// NB column blocks per wave: 2 (waves 0-3, blocks 0 and 1 of the SIMD's column half) or 1 (waves 4-7, block 2)
template <int NB> constexpr int bwd_b0() { return NB == 2 ? 0 : 2; }

// step `it` of a data-gradient conv's weight stream: this SIMD's column half (wn) and K parity (wk), this wave's NB blocks
template <int NB>
__device__ __forceinline__ void bwd_w_load(const bf16_t* W1, int it, int wn, int wk, int lane, uint4 (&dst)[2][NB])
{
  const int slice = it / TAPS, tap = it - slice * TAPS;
  const bf16_t* Wt = pinned(W1 + (size_t)((tap * B_NBT + 3 * wn + bwd_b0<NB>()) * B_KS + slice * 4 + 2 * wk) * 512);
#pragma unroll
  for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
    for (int bn = 0; bn < NB; ++bn) dst[k2][bn] = ldfrag_global(Wt, bn * B_KS + k2, lane);
}
// the first RB - 1 steps: issued by the PREVIOUS step (or the kernel's head) ahead of its stores — vmcnt retires in order, so a
// wait for these fragments would otherwise also wait for every store issued before them (see the forward kernel)
template <int RBv, int NB>
__device__ __forceinline__ void bwd_ring_prologue(const void* w, int lane, uint4 (&ring)[RBv][2][NB])
{
  const int simd = wave_scalar() & 3, wn = simd & 1, wk = simd >> 1;
  const bf16_t* W1 = pinned(static_cast<const bf16_t*>(w));
#pragma unroll
  for (int p = 0; p < RBv - 1; ++p) bwd_w_load<NB>(W1, p, wn, wk, lane, ring[p]);
}

// one step j of the chain (compile-time j: every pointer is a kernel argument, every fragment address is formed where it is used)
template <int J, bool COND, bool DROP, int NBM, int NB>
__device__ __forceinline__ void bwd_step(const gt_wn_stack_bwd_args& a, uint32_t drop_thresh, float drop_scale, uint32_t seed_x,
                                         bf16_t* Dt, float* Ex, bf16_t* At, int s0, int halo,
                                         uint4 (&ring)[NBM == 1 ? RB1 : RB][2][NB], float rm)
{
  // the thread index as a value formed HERE (see the forward's tid_e): formed once for the kernel, the per-lane addresses derived
  // from it are carried (spilled) from step to step
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int simd = wave_scalar() & 3;
  const int wn = simd & 1, wk = simd >> 1;     // stage 1: column half, K parity;  afterwards wk doubles as the row half
  constexpr int B0 = bwd_b0<NB>();             // this wave's first block of the column half
  constexpr int BMv = 32 * NBM;                // rows of the tile (NBM: see the forward kernel)
  constexpr int RBv = NBM == 1 ? RB1 : RB;
  const bool act = wk < NBM;                   // NBM = 1: one row block — the waves of K parity 1 hand their sums over and sit the rest out
  const int n_layers = a.n_layers, R = a.R;
  const bf16_t* via = static_cast<const bf16_t*>(a.via_skip);
  constexpr int NIT = B_NIT;
  const bf16_t* W1 = pinned(static_cast<const bf16_t*>(a.w_in_d[J]));
  f32x16_t acc[NB][NBM];                       // (written out: through acc_zero this kernel comes out scheduled differently)
#pragma unroll
  for (int bn = 0; bn < NB; ++bn)
#pragma unroll
    for (int bm = 0; bm < NBM; ++bm)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[bn][bm][e] = 0.0f;
  auto w_load = [&](int it, uint4 (&dst)[2][NB]) { bwd_w_load<NB>(W1, it, wn, wk, lane, dst); };
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int slice = it / TAPS, tap = it - slice * TAPS;
    w_load(it + RBv - 1 < NIT ? it + RBv - 1 : NIT - 1, ring[(it + RBv - 1) % RBv]);
    __builtin_amdgcn_sched_barrier(0);
    const bf16_t* xsb = Dt + (r + tap) * DP + 8 * h + slice * 64 + 32 * wk;
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      bf16x8_t bx[NBM];
#pragma unroll
      for (int bm = 0; bm < NBM; ++bm) bx[bm] = *reinterpret_cast<const bf16x8_t*>(xsb + 32 * bm * DP + k2 * 16);
#pragma unroll
      for (int bn = 0; bn < NB; ++bn)
#pragma unroll
        for (int bm = 0; bm < NBM; ++bm)
          acc[bn][bm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(asfrag(ring[it % RBv][k2][bn]), bx[bm], acc[bn][bm], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  PH(2 + 8 * (3 - J));
  // second-stage weights (the layer below): this wave's NB blocks of the SIMD's 96 columns (wn), rows 32*wk
  constexpr int JL = J > 0 ? J - 1 : 0;
  const bf16_t* W2 = pinned(static_cast<const bf16_t*>(a.w_res_d[JL]));
  // All of them before the stage-2 loop (reloaded inside it they arrived after it needed them): the first half now, the second once
  // the stage-1 accumulators are dead (all at once, next to those and the gate operands below, they spill)
  uint4 ring2[KK2][NB];
  auto w2_load = [&](int k0, int k1) {
    if (J > 0 && act) {
#pragma unroll
      for (int kk = k0; kk < k1; ++kk)
#pragma unroll
        for (int bn = 0; bn < NB; ++bn) ring2[kk][bn] = ldfrag_global(W2, (3 * wn + B0 + bn) * KK2 + kk, lane);
    }
  };
  w2_load(0, KK2 / 2);
  // the gate backward's three row operands (skip-path gradient, saved tanh, saved sigmoid of layer j-1, all 64 rows of the tile) are
  // fetched as whole rows — read in the MFMA layout, every load instruction touched 16 bytes in each of 32 rows — and handed to the
  // epilogue through LDS; they are issued here, ahead of this step's stores
  constexpr int JLp = J > 0 ? J - 1 : 0;
  constexpr int NPRE = (BM * CPR + BWD_THREADS - 1) / BWD_THREADS;   // 3 chunks per thread and operand
  uint4 pre[3][NPRE];
  if (J > 0) {
    const bf16_t* Tg = static_cast<const bf16_t*>(a.gate_t[JLp]);
    const bf16_t* Sg = static_cast<const bf16_t*>(a.gate_s[JLp]);
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int idx = tid + BWD_THREADS * i, row = idx / CPR, c8 = idx - row * CPR, mm = s0 + row;
      pre[0][i] = pre[1][i] = pre[2][i] = make_uint4(0, 0, 0, 0);
      if (row < BMv && mm >= 0 && mm < R) {
        pre[0][i] = *reinterpret_cast<const uint4*>(via + (size_t)mm * a.ldvs + JLp * H + c8 * 8);
        pre[1][i] = *reinterpret_cast<const uint4*>(Tg + (size_t)mm * H + c8 * 8);
        pre[2][i] = *reinterpret_cast<const uint4*>(Sg + (size_t)mm * H + c8 * 8);
      }
    }
  }
  __syncthreads();                            // every wave is done with the d pre tile: the exchange buffer may overwrite it

  // K parities meet: a wave keeps row block bm == wk and hands the other one to the wave of the same blocks and the other parity
  if (NBM == 2 || wk) {
    float* mine = Ex + (simd * 3 + B0) * (16 * 64);
#pragma unroll
    for (int bn = 0; bn < NB; ++bn)
#pragma unroll
      for (int e = 0; e < 16; ++e) mine[(bn * 16 + e) * 64 + lane] = (NBM == 2 && !wk) ? acc[bn][NBM - 1][e] : acc[bn][0][e];
  }
  __syncthreads();
  f32x16_t sum[NB];
  if (act) {
    const float* theirs = Ex + ((simd ^ 2) * 3 + B0) * (16 * 64);
#pragma unroll
    for (int bn = 0; bn < NB; ++bn)
#pragma unroll
      for (int e = 0; e < 16; ++e) sum[bn][e] = ((NBM == 2 && wk) ? acc[bn][NBM - 1][e] : acc[bn][0][e]) + theirs[(bn * 16 + e) * 64 + lane];
  }
  w2_load(KK2 / 2, KK2);
  PH(3 + 8 * (3 - J));
  // dX_j = (conv^T(d pre_j) + dX_{j+1}) * mask -> HBM (owned rows) and the stage-2 tile (which still holds dX_{j+1})
  const int t = 32 * wk + r, m = s0 + t;
  const bool mine_row = act && t >= halo && t < BMv - halo && m < R;
  if (act) {
#pragma unroll
    for (int bn = 0; bn < NB; ++bn)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = 32 * (3 * wn + B0 + bn) + 8 * g + 4 * h;
        float ad[4] = {};
        if (J < n_layers - 1) unpack4(*reinterpret_cast<const uint2*>(At + t * AP + n), ad);
        const uint2 v = pack4((sum[bn][4 * g] + ad[0]) * rm, (sum[bn][4 * g + 1] + ad[1]) * rm,
                              (sum[bn][4 * g + 2] + ad[2]) * rm, (sum[bn][4 * g + 3] + ad[3]) * rm);
        *reinterpret_cast<uint2*>(At + t * AP + n) = v;
      }
  }
  __syncthreads();
  PH(4 + 8 * (3 - J));
  auto store_dx = [&]() {
    // dX_j of the owned rows leaves as whole rows from the finished tile (the MFMA layout gives a store 16 bytes in each of 32 rows)
    bf16_t* dx = static_cast<bf16_t*>(a.dx[J]);
    const int own = BMv - 2 * halo;
    constexpr int NC = (BM * CPR + BWD_THREADS - 1) / BWD_THREADS;
    uint4 vx[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int idx = tid + BWD_THREADS * i, row = idx / CPR, c8 = idx - row * CPR;
      vx[i] = make_uint4(0, 0, 0, 0);
      if (idx < own * CPR) vx[i] = *reinterpret_cast<const uint4*>(At + (halo + row) * AP + c8 * 8);
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int idx = tid + BWD_THREADS * i, row = idx / CPR, c8 = idx - row * CPR, mm = s0 + halo + row;
      if (idx < own * CPR && mm < R) *reinterpret_cast<uint4*>(dx + (size_t)mm * H + c8 * 8) = vx[i];
    }
  };
  if (J == 0) { store_dx(); return; }                               // bottom: dX_0 is the gradient at the WaveNet's input

  // d acts_{j-1} = dX_j W_res + skip-path gradient -> gate backward -> d pre_{j-1}: the next tile (+ HBM for the owned rows)
  bf16_t* Vl = At + BM * AP; bf16_t* Tl = Vl + BM * AP; bf16_t* Sl = Tl + BM * AP;
  f32x16_t acc2[NB];
  acc_zero(acc2);
  if (act) {
    const bf16_t* ab = At + (32 * wk + r) * AP + 8 * h;
#pragma unroll
    for (int kk = 0; kk < KK2; ++kk) {
      const bf16x8_t bfm = *reinterpret_cast<const bf16x8_t*>(ab + kk * 16);
#pragma unroll
      for (int bn = 0; bn < NB; ++bn) {
        acc2[bn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(asfrag(ring2[kk][bn]), bfm, acc2[bn], 0, 0, 0);
      }
    }
  }
  PH(5 + 8 * (3 - J));
  bwd_ring_prologue<RBv, NB>(a.w_in_d[JL], lane, ring);            // the next step's first fragments, then this step's stores
  store_dx();                                                       // (the dX tile stays as it is until the next step's epilogue)
#pragma unroll
  for (int i = 0; i < NPRE; ++i) {
    const int idx = tid + BWD_THREADS * i, row = idx / CPR, c8 = idx - row * CPR;
    if (row >= BMv) continue;
    *reinterpret_cast<uint4*>(Vl + row * AP + c8 * 8) = pre[0][i];
    *reinterpret_cast<uint4*>(Tl + row * AP + c8 * 8) = pre[1][i];
    *reinterpret_cast<uint4*>(Sl + row * AP + c8 * 8) = pre[2][i];
  }
  __syncthreads();
  PH(6 + 8 * (3 - J));
  if (act) {
    bf16_t* dpre_c = static_cast<bf16_t*>(a.dpre_c[JL]);
    const uint32_t seed = (a.drop_seed + (uint32_t)JL) ^ seed_x;
    const bool in = m >= 0 && m < R;
#pragma unroll
    for (int bn = 0; bn < NB; ++bn)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = 32 * (3 * wn + B0 + bn) + 8 * g + 4 * h;
        uint2 pt = make_uint2(0, 0), ps = pt, ct = pt, cs = pt;
        if (in) {
          float vs[4], tt[4], sg[4], dd[4];
          unpack4(*reinterpret_cast<const uint2*>(Vl + t * AP + n), vs);
          unpack4(*reinterpret_cast<const uint2*>(Tl + t * AP + n), tt);
          unpack4(*reinterpret_cast<const uint2*>(Sl + t * AP + n), sg);
#pragma unroll
          for (int q = 0; q < 4; ++q) dd[q] = acc2[bn][4 * g + q] + vs[q];
          gate_bwd4<DROP>(dd, tt, sg, seed, m, n, drop_thresh, drop_scale, pt, ps, ct, cs);
          if (COND && mine_row) {                                    // (speaker-conditioned configs only)
            *reinterpret_cast<uint2*>(dpre_c + (size_t)m * 2 * H + n) = ct;
            *reinterpret_cast<uint2*>(dpre_c + (size_t)m * 2 * H + H + n) = cs;
          }
        }
        *reinterpret_cast<uint2*>(Dt + (t + 2) * DP + n) = pt;
        *reinterpret_cast<uint2*>(Dt + (t + 2) * DP + H + n) = ps;
      }
  }
  PH(7 + 8 * (3 - J));
  __syncthreads();                                                   // the next conv's input tile is complete
  PH(8 + 8 * (3 - J));
  {
    // d pre_{j-1} of the owned rows: whole 768-byte rows from the tile (read-only until the next step's exchange, which follows a barrier)
    bf16_t* dpre = static_cast<bf16_t*>(a.dpre[JL]);
    const int own = BMv - 2 * halo;
    constexpr int CPR2 = 2 * H / 8, NC = (BM * CPR2 + BWD_THREADS - 1) / BWD_THREADS, NP = 3;   // 6 chunks per thread, in passes of NP
#pragma unroll
    for (int i0 = 0; i0 < NC; i0 += NP) {
      uint4 vx[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int idx = tid + BWD_THREADS * (i0 + i), row = idx / CPR2, c8 = idx - row * CPR2;
        vx[i] = make_uint4(0, 0, 0, 0);
        if (idx < own * CPR2) vx[i] = *reinterpret_cast<const uint4*>(Dt + (halo + row + 2) * DP + c8 * 8);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int idx = tid + BWD_THREADS * (i0 + i), row = idx / CPR2, c8 = idx - row * CPR2, mm = s0 + halo + row;
        if (idx < own * CPR2 && mm < R) *reinterpret_cast<uint4*>(dpre + (size_t)mm * 2 * H + c8 * 8) = vx[i];
      }
    }
  }
  PH(9 + 8 * (3 - J));
}

// the whole launch as one wave sees it: NB (2 or 1) column blocks per stage (see the section's header)
template <bool COND, bool DROP, int NBM, int NB>
__device__ __forceinline__ void bwd_wave(const gt_wn_stack_bwd_args& a, uint32_t drop_thresh, float drop_scale)
{
  constexpr int BMv = 32 * NBM, XRv = BMv + TAPS - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  PH(0);
  const uint32_t seed_x = a.seed_dev ? *a.seed_dev : 0u;
  const int lane = threadIdx.x & 63, simd = (threadIdx.x >> 6) & 3;
  const int n_layers = a.n_layers, R = a.R;
  const int halo = 2 * (n_layers - 1), own = BMv - 2 * halo;
  const int s0 = blockIdx.x * own - halo;
  bf16_t* Dt = reinterpret_cast<bf16_t*>(smem);
  float* Ex = reinterpret_cast<float*>(smem);
  bf16_t* At = reinterpret_cast<bf16_t*>(smem + BWD_DT);
  const bf16_t* via = static_cast<const bf16_t*>(a.via_skip);
  constexpr int RBv = NBM == 1 ? RB1 : RB;
  uint4 ring[RBv][2][NB];
  bwd_ring_prologue<RBv, NB>(pick(a.w_in_d, n_layers - 1), lane, ring);   // ahead of the head's d pre stores
  float rm;                                                         // the row mask of the row this lane finishes in every dX epilogue
  {
    const int m = s0 + 32 * (simd >> 1) + (lane & 31);
    rm = (m >= 0 && m < R) ? a.rowmask[m] : 0.0f;
  }

  // top layer: d acts = the skip-path gradient only -> d pre on all 68 rows of the tile (row-local).  Whole rows, 16 bytes per lane,
  // EVERY load issued before the first use: as a loop of 8-byte loads, each waited for where it was used, this head was 13 serial
  // L2 round trips = 30 k of the launch's 189 k cycles (tools/wn_stack_phases.py).
  {
    const int L = n_layers - 1;
    const bf16_t* Tt = static_cast<const bf16_t*>(pick(a.gate_t, L));
    const bf16_t* Ss = static_cast<const bf16_t*>(pick(a.gate_s, L));
    bf16_t* dpre = static_cast<bf16_t*>(pick(a.dpre, L));
    bf16_t* dpre_c = static_cast<bf16_t*>(pick(a.dpre_c, L));
    const uint32_t seed = (a.drop_seed + (uint32_t)L) ^ seed_x;
    constexpr int NH = (XR * CPR + BWD_THREADS - 1) / BWD_THREADS;   // 4 chunks of 8 channels per thread
    uint4 hv[3][NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const int idx = threadIdx.x + BWD_THREADS * i, u = idx / CPR, c8 = idx - u * CPR, m = s0 - 2 + u;
      hv[0][i] = hv[1][i] = hv[2][i] = make_uint4(0, 0, 0, 0);
      if (u < XRv && m >= 0 && m < R) {
        hv[0][i] = *reinterpret_cast<const uint4*>(via + (size_t)m * a.ldvs + L * H + c8 * 8);
        hv[1][i] = *reinterpret_cast<const uint4*>(Tt + (size_t)m * H + c8 * 8);
        hv[2][i] = *reinterpret_cast<const uint4*>(Ss + (size_t)m * H + c8 * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < NH; ++i) {
      const int idx = threadIdx.x + BWD_THREADS * i, u = idx / CPR, c8 = idx - u * CPR, m = s0 - 2 + u, n = c8 * 8;
      if (u >= XRv) continue;
      uint2 pt[2], ps[2], ct[2], cs[2];
      pt[0] = pt[1] = ps[0] = ps[1] = ct[0] = ct[1] = cs[0] = cs[1] = make_uint2(0, 0);
      if (m >= 0 && m < R) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          float dd[4], t[4], sg[4];
          unpack4(q ? make_uint2(hv[0][i].z, hv[0][i].w) : make_uint2(hv[0][i].x, hv[0][i].y), dd);
          unpack4(q ? make_uint2(hv[1][i].z, hv[1][i].w) : make_uint2(hv[1][i].x, hv[1][i].y), t);
          unpack4(q ? make_uint2(hv[2][i].z, hv[2][i].w) : make_uint2(hv[2][i].x, hv[2][i].y), sg);
          gate_bwd4<DROP>(dd, t, sg, seed, m, n + 4 * q, drop_thresh, drop_scale, pt[q], ps[q], ct[q], cs[q]);
        }
        if (u - 2 >= halo && u - 2 < BMv - halo) {
          *reinterpret_cast<uint4*>(dpre + (size_t)m * 2 * H + n) = make_uint4(pt[0].x, pt[0].y, pt[1].x, pt[1].y);
          *reinterpret_cast<uint4*>(dpre + (size_t)m * 2 * H + H + n) = make_uint4(ps[0].x, ps[0].y, ps[1].x, ps[1].y);
          if (COND) {
            *reinterpret_cast<uint4*>(dpre_c + (size_t)m * 2 * H + n) = make_uint4(ct[0].x, ct[0].y, ct[1].x, ct[1].y);
            *reinterpret_cast<uint4*>(dpre_c + (size_t)m * 2 * H + H + n) = make_uint4(cs[0].x, cs[0].y, cs[1].x, cs[1].y);
          }
        }
      }
      *reinterpret_cast<uint4*>(Dt + u * DP + n) = make_uint4(pt[0].x, pt[0].y, pt[1].x, pt[1].y);
      *reinterpret_cast<uint4*>(Dt + u * DP + H + n) = make_uint4(ps[0].x, ps[0].y, ps[1].x, ps[1].y);
    }
  }
  __syncthreads();
  PH(1);
  // the chain, top to bottom (workgroup-uniform branches; each step is its own straight-line code)
  if (n_layers > 3) bwd_step<3, COND, DROP, NBM, NB>(a, drop_thresh, drop_scale, seed_x, Dt, Ex, At, s0, halo, ring, rm);
  if (n_layers > 2) bwd_step<2, COND, DROP, NBM, NB>(a, drop_thresh, drop_scale, seed_x, Dt, Ex, At, s0, halo, ring, rm);
  if (n_layers > 1) bwd_step<1, COND, DROP, NBM, NB>(a, drop_thresh, drop_scale, seed_x, Dt, Ex, At, s0, halo, ring, rm);
  bwd_step<0, COND, DROP, NBM, NB>(a, drop_thresh, drop_scale, seed_x, Dt, Ex, At, s0, halo, ring, rm);
  PH(40);
}

// Both halves run the same sequence of barriers; the branch is on a wave-uniform scalar.  A static s_setprio 1 for waves 4-7 (the
// arbitration losers of an 8-wave workgroup) measured slower: 78.5 against 74.5 us per launch back to back at cfg 2's rows.
template <bool COND, bool DROP, int NBM>
__global__ __launch_bounds__(BWD_THREADS) void gt_wn_stack_bwd_kernel(gt_wn_stack_bwd_args a, uint32_t drop_thresh, float drop_scale)
{
  if (wave_scalar() < 4) bwd_wave<COND, DROP, NBM, 2>(a, drop_thresh, drop_scale);
  else bwd_wave<COND, DROP, NBM, 1>(a, drop_thresh, drop_scale);
}

}  // namespace

#if WNS_PHASES
extern "C" int gt_dev_wns_phases(void* dst, size_t bytes)
{
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wns_ph), bytes < sizeof(g_wns_ph) ? bytes : sizeof(g_wns_ph)) == hipSuccess ? 0 : -1;
}
#endif

#ifndef WNS_SMALL_TILE_MAX_WGS
#define WNS_SMALL_TILE_MAX_WGS 80             // 64-row tiles give at most this many workgroups -> 32-row tiles (needs n_layers <= 4: 20 owned rows);
                                              // re-checked with the 8-wave backward: 98 gives cfg 4 4.29 vs 4.31 ms, cfg 5 15.09 vs 13.74 ms
#endif
// 32-row blocks per tile for a launch over R rows: 2, or 1 when the 64-row tiling would leave two thirds of the 256 CUs idle.  Measured
// back to back (tools/wn_layer_bench.py stack, WN_BENCH_TY=..., round 3; forward / backward us per launch, 64-row -> 32-row tiles):
// 3 072 rows 61.7 / 71.4 -> 51.2 / 59.3;  3 584 rows 62.0 / 72.9 -> 51.7 / 61.0;  5 120 rows 63.2 / 75.6 -> 57.1 / 68.2 (and nothing left
// of it inside the cfg 4 / cfg 5 steps, whose other branch then finds no free CU: the threshold stays below that);  9 728 rows: 2 rounds.
#ifndef WNS_SMALL_TILE_MAX_WGS_FWD
#define WNS_SMALL_TILE_MAX_WGS_FWD 98         // the FORWARD takes the 32-row form up to here (2.6 x 98 = 255 workgroups: one round of the
                                              // chip; measured at 128, which cfg 4 / cfg 5's 85 / 89 tiles are below either way): with cfg 5's final schedule its decoder forward runs
#endif                                        // alone on the machine for 2.6 ms (14.55-14.64 -> 14.24 ms per step); the backward, which always
                                              // shares it with the predictors' backward, at the same threshold: 15.75 ms
static int stack_row_blocks(int R, int n_layers, bool fwd = false)
{
  const int own2 = BM - 4 * (n_layers - 1), own1 = 32 - 4 * (n_layers - 1);
  return (own1 >= 8 && (R + own2 - 1) / own2 <= (fwd ? WNS_SMALL_TILE_MAX_WGS_FWD : WNS_SMALL_TILE_MAX_WGS)) ? 1 : 2;
}
extern "C" int gt_wn_stack_rows_per_workgroup(int n_layers) { return BM - 4 * (n_layers - 1); }
extern "C" int gt_wn_stack_row_blocks(int R, int n_layers, int fwd) { return stack_row_blocks(R, n_layers, fwd != 0); }

extern "C" int gt_wn_stack_fwd(const gt_wn_stack_fwd_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_wn_stack_fwd_args& a = *args;
  if (a.R < 0) return GT_E_INVAL;
  if (a.R == 0) return GT_OK;
  if (a.H != H || a.taps != TAPS || a.n_layers < 1 || a.n_layers > NLMAX) return GT_E_UNSUPPORTED;
  if (!a.x0 || !a.rowmask || !a.acts || a.ldacts < a.n_layers * H || (a.ldacts & 7) || (a.cond && (a.ldc & 3))) return GT_E_INVAL;
  if (!al16(a.x0) || !al16(a.acts) || !al16(a.cond)) return GT_E_ALIGN;
  // the backward's saves (gate_t, gate_s, x_out): every one of them, or none (synthesis: acts only)
  int n_save = 0, n_given = 0;
  for (int i = 0; i < a.n_layers; ++i) {
    n_save += 2 + (i < a.n_layers - 1);
    n_given += (a.gate_t[i] != nullptr) + (a.gate_s[i] != nullptr) + (i < a.n_layers - 1 && a.x_out[i] != nullptr);
  }
  if (n_given != 0 && n_given != n_save) return GT_E_INVAL;
  const bool save = n_given != 0;
  for (int i = 0; i < a.n_layers; ++i) {
    if (!a.w_in[i] || !a.b_in[i]) return GT_E_INVAL;
    if (i < a.n_layers - 1 && (!a.w_res[i] || !a.b_res[i])) return GT_E_INVAL;
    if (!al16(a.w_in[i]) || !al16(a.b_in[i]) || !al16(a.gate_t[i]) || !al16(a.gate_s[i]) || !al16(a.w_res[i]) || !al16(a.b_res[i]) ||
        !al16(a.x_out[i])) return GT_E_ALIGN;
  }
  if (a.cond && (a.Tp <= 0 || (a.row0 && a.B <= 0))) return GT_E_INVAL;
  const bool affine = a.aff_w || a.aff_b || a.aff_sig;
  if (affine) {
    if (a.cond || !a.aff_w || !a.aff_b || !a.aff_sig || ((H * a.n_layers) % (2 * H))) return GT_E_INVAL;   // (O must hold whole layers: n even)
    if (!al16(a.aff_w) || !al16(a.aff_b) || ((uintptr_t)a.aff_sig & 7)) return GT_E_ALIGN;
  }
  if (a.drop_p >= 1.0f) return GT_E_UNSUPPORTED;
  uint32_t thresh; float scale;
  gt_drop_params(a.drop_p, &thresh, &scale);
  typedef void (*kern_t)(gt_wn_stack_fwd_args, uint32_t, float);
  static const kern_t kerns[12] = {gt_wn_stack_fwd_kernel<0, false, 2>, gt_wn_stack_fwd_kernel<0, true, 2>, gt_wn_stack_fwd_kernel<1, false, 2>,
                                   gt_wn_stack_fwd_kernel<1, true, 2>, gt_wn_stack_fwd_kernel<2, false, 2>, gt_wn_stack_fwd_kernel<2, true, 2>,
                                   gt_wn_stack_fwd_kernel<0, false, 1>, gt_wn_stack_fwd_kernel<0, true, 1>, gt_wn_stack_fwd_kernel<1, false, 1>,
                                   gt_wn_stack_fwd_kernel<1, true, 1>, gt_wn_stack_fwd_kernel<2, false, 1>, gt_wn_stack_fwd_kernel<2, true, 1>};
  // acts only (the synthesis direction: no dropout; no affine conditioning, see SAVE), [row form][COND]
  static const kern_t kerns_nosave[4] = {gt_wn_stack_fwd_kernel<0, false, 2, false>, gt_wn_stack_fwd_kernel<1, false, 2, false>,
                                         gt_wn_stack_fwd_kernel<0, false, 1, false>, gt_wn_stack_fwd_kernel<1, false, 1, false>};
  if (!save && (thresh || affine)) return GT_E_UNSUPPORTED;
  static bool attr = false;                    // > 64 KB of LDS: opt in once per process
  if (!attr) {
    for (int i = 0; i < 12; ++i)
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kerns[i]), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (i % 6) >= 4 ? STACK_FWD_LDS_AFF : STACK_FWD_LDS) != hipSuccess)
        return GT_E_LAUNCH;
    for (int i = 0; i < 4; ++i)
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kerns_nosave[i]), hipFuncAttributeMaxDynamicSharedMemorySize, STACK_FWD_LDS) != hipSuccess)
        return GT_E_LAUNCH;
    attr = true;
  }
  const int nbm = stack_row_blocks(a.R, a.n_layers, true);
  const int own = 32 * nbm - 4 * (a.n_layers - 1);
  const dim3 grid((a.R + own - 1) / own), block(256);
  const int mode = affine ? 2 : (a.cond ? 1 : 0);
  const kern_t kern = save ? kerns[(nbm == 1 ? 6 : 0) + 2 * mode + (thresh ? 1 : 0)] : kerns_nosave[(nbm == 1 ? 2 : 0) + mode];
  hipLaunchKernelGGL(kern, grid, block, affine ? STACK_FWD_LDS_AFF : STACK_FWD_LDS, static_cast<hipStream_t>(stream), a, thresh, scale);
  return gt_launch_status(__func__);
}

extern "C" int gt_wn_stack_bwd(const gt_wn_stack_bwd_args* args, void* stream)
{
  if (!args) return GT_E_INVAL;
  const gt_wn_stack_bwd_args& a = *args;
  if (a.R < 0) return GT_E_INVAL;
  if (a.R == 0) return GT_OK;
  if (a.H != H || a.taps != TAPS || a.n_layers < 1 || a.n_layers > NLMAX) return GT_E_UNSUPPORTED;
  if (!a.via_skip || !a.rowmask || a.ldvs < a.n_layers * H || (a.ldvs & 7)) return GT_E_INVAL;
  if (!al16(a.via_skip)) return GT_E_ALIGN;
  for (int i = 0; i < a.n_layers; ++i) {
    if (!a.w_in_d[i] || !a.gate_t[i] || !a.gate_s[i] || !a.dpre[i] || !a.dx[i]) return GT_E_INVAL;
    if (i < a.n_layers - 1 && !a.w_res_d[i]) return GT_E_INVAL;
    if (!al16(a.w_in_d[i]) || !al16(a.gate_t[i]) || !al16(a.gate_s[i]) || !al16(a.dpre[i]) || !al16(a.dpre_c[i]) || !al16(a.dx[i]) ||
        !al16(a.w_res_d[i])) return GT_E_ALIGN;
  }
  if (a.drop_p >= 1.0f) return GT_E_UNSUPPORTED;
  uint32_t thresh; float scale;
  gt_drop_params(a.drop_p, &thresh, &scale);
  bool cond = false;                           // d cond outputs: all layers or none
  for (int i = 0; i < a.n_layers; ++i) cond = cond || a.dpre_c[i];
  for (int i = 0; i < a.n_layers; ++i) if (cond && !a.dpre_c[i]) return GT_E_INVAL;
  typedef void (*kern_t)(gt_wn_stack_bwd_args, uint32_t, float);
  static const kern_t kerns[8] = {gt_wn_stack_bwd_kernel<false, false, 2>, gt_wn_stack_bwd_kernel<false, true, 2>,
                                  gt_wn_stack_bwd_kernel<true, false, 2>, gt_wn_stack_bwd_kernel<true, true, 2>,
                                  gt_wn_stack_bwd_kernel<false, false, 1>, gt_wn_stack_bwd_kernel<false, true, 1>,
                                  gt_wn_stack_bwd_kernel<true, false, 1>, gt_wn_stack_bwd_kernel<true, true, 1>};
  static bool attr = false;
  if (!attr) {
    for (kern_t k : kerns)
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, SBWD_LDS) != hipSuccess)
        return GT_E_LAUNCH;
    attr = true;
  }
  const int nbm = stack_row_blocks(a.R, a.n_layers);
  const int own = 32 * nbm - 4 * (a.n_layers - 1);
  const dim3 grid((a.R + own - 1) / own), block(BWD_THREADS);
  hipLaunchKernelGGL(kerns[(nbm == 1 ? 4 : 0) + (cond ? 2 : 0) + (thresh ? 1 : 0)], grid, block, SBWD_LDS, static_cast<hipStream_t>(stream), a, thresh, scale);
  return gt_launch_status(__func__);
}
