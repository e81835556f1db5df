// Wave-specialised convolution: every forward layer and data gradient ava_conv3x3_mfma serves, except conv7's forward
// (its second, NCHW output needs conv3x3_mfma_kernel).  512 threads per workgroup: waves 0-3 only stage
// tiles (global -> registers -> BatchNorm prologue -> LDS), waves 4-7 only multiply (weights in registers, MFMA,
// bias/ReLU/statistics epilogue), on two LDS tile buffers.  Every SIMD then hosts one staging wave and one matrix-core
// wave of the workgroup, so the VALU/LDS-write work of tile k+1 runs beside the MFMAs of tile k instead of before them.
// Same arguments, tiles, MSPLIT / PAIR variants and partial-row format as conv3x3_mfma_kernel (EPI_FWD, PRO_BN).
// Measured: 3-8 % per kernel, 27 us per step over the eleven forward shapes.
#include <stdlib.h>
#include <type_traits>
#include "conv_mfma.h"

// Which shapes run the limb form (launch_mfma_ws): every forward-type launch with 16 or more input channels (conv4..conv6, convt1..convt5
// forward and the four 16 x 16 layers' data gradients) and, since the staging waves' prologue lost its serialised LDS reads
// (conv_common.h: TileStager::coef_of) and has room for the split, the forward of conv2 and conv3 (8 input channels:
// isolated 42.2 -> 35.2 and 40.1 -> 32.5 us, step -7 us; whole -m gpu suite unchanged).  Measured earlier on every shape (profiles/r03/limb_conv_forward.txt,
// limb_conv_configs.txt): conv5 16 -> 24: 31.3 -> 24 us, convt5 16 -> 8: 45.8 -> 32 us, the others +-1 us (at one or two
// tiles per workgroup they are bound by launch / prologue latency, not by the matrix pipe; the 24- and 32-channel ones need
// > 128 VGPRs for three limbs of weights and run one workgroup per CU), conv4 29 -> 35 us (stride 2: the fragments are read
// with a 32-byte lane stride, two-way LDS conflicts; 26 us once it holds two tiles in registers).
// Choice among the sets that are about equally fast (-17 .. -26 us per step): every arithmetic (the fp32 MFMA one included)
// flips a different handful of ReLU masks against the reference's fp32 goldens, and the golden /
// trajectory / callers tests pass at their round-2 tolerances for this set and for {convt5}; the faster sets each trip one
// of them by a flip ({conv5, convt5}: golden B8 z64; forward-only sets: six-step trajectory; 16-channel forward set: the
// callers' second-epoch loss at 4.9x the reference's own run-to-run noise against an allowance of 4x).  The mask-imposed
// fp64-oracle gradient tests pass for all of them.

// ACT: storage type of the activations this launch touches -- the input of a forward layer (PRO_BN), the saved
// activation in2 of the ReLU/BatchNorm-backward prologue (PRO_BWD), the raw x of the BatchNorm-backward sums (EPI_BWD)
// and the output of a forward layer (EPI_FWD).  Gradients (PRO_BWD / PRO_ID inputs, EPI_BWD outputs) are always fp32.
// LIMB: the products run on v_mfma_f32_16x16x32_bf16 with fp32 operands split into three bf16 limbs (six limb products,
// fp32-faithful; conv_common.h / conv_mfma.h): the staging waves write limb planes, the matrix-core waves hold limb weights.
template <int CIN, int COUT, int MODE, int PRO, int EPI, int TW, int TH, bool MSPLIT, bool PAIR, typename ACT, bool LIMB = false>
__global__ __launch_bounds__(512) void conv3x3_mfma_ws_kernel(const ConvArgs a) {
  using G = Geom<MODE, TW, TH>;
  using TIN = typename std::conditional<PRO == PRO_BN, ACT, float>::type;
  using TOUT = typename std::conditional<EPI == EPI_FWD, ACT, float>::type;
  constexpr int IR = G::IR, IC = G::IC;
  constexpr int MTA = (COUT + 15) / 16;             // cout tiles of the layer
  constexpr int MT = MSPLIT ? 1 : MTA;              // cout tiles of one matrix-core wave (see conv3x3_mfma_kernel)
  static_assert(!MSPLIT || MTA == 2, "MSPLIT deals exactly two cout tiles to the wave pairs");
  static_assert(!PAIR || (MODE == MODE_S1 && COUT == 8 && !MSPLIT && TH % 2 == 0), "PAIR: stride 1, 8 output channels");
  constexpr int NCLS = n_classes<MODE>();
  static_assert(!LIMB || CIN % 8 == 0, "limb planes are made of channel octets");
  // bf16 arithmetic (act_dtype = bfloat16: BASELINE configs[4] "bf16 conv"): weights rounded to bfloat16 (one limb), and in a
  // forward launch the rounded BatchNorm outputs are one plane (TileStager::BF16_MATH) -- one product instead of six; a
  // data-gradient launch keeps its fp32 gradient in three planes (three products)
  constexpr bool BF16M = std::is_same<ACT, ava_bf16>::value;
  constexpr int NLW = BF16M ? 1 : 3, NLB = ava_stager_limbs<TIN, PRO>();
  constexpr int NPIXP = IR * IC;                               // octet-plane stride of the limb image (pixels)
  constexpr int TILE_F = LIMB ? NPIXP * CIN * NLB / 2 : IR * IC * CIN;        // floats; LIMB: NLB bf16 planes
  extern __shared__ __align__(16) float smem[];
  float* tile0 = smem;                      // two tile buffers
  float* coef = smem + 2 * TILE_F;          // [3][32]
  float* red = coef + 96;                   // [4][2*16*MTA]
  __shared__ double accvals[64];            // consumer prologue scratch (bn_coef_from_acc)

  const int t = threadIdx.x, lane = t & 63, wave8 = t >> 6;
  const bool stager = wave8 < 4;
  const int wave = wave8 & 3;
  const int n = lane & 15, kg = lane >> 4;
  auto origin = [&](int tl, int& b, int& oy0, int& ox0, int& gy0, int& gx0) {
    b = tl / (a.tiles_y * a.tiles_x);
    const int rem = tl - b * (a.tiles_y * a.tiles_x);
    oy0 = (rem / a.tiles_x) * TH;
    ox0 = (rem % a.tiles_x) * TW;
    if (MODE == MODE_S1) { gy0 = oy0 - 1; gx0 = ox0 - 1; }
    else if (MODE == MODE_DOWN) { gy0 = 2 * oy0 - 1; gx0 = 2 * ox0 - 1; }
    else { gy0 = oy0 / 2; gx0 = ox0 / 2; }
  };
  TileWalk walk(a.ntiles);
  typename std::conditional<LIMB, TileStagerL<CIN, PRO, IR, IC, 256, TIN, ACT>,
                            TileStager<CIN, PRO, IR, IC, 256, TIN, ACT>>::type stg;   // staging waves only (threadIdx.x 0..255)
  // DEEP: the limb tiles of the stride-2 layers with >= 16 channels fill the LDS of a CU with ONE workgroup (two buffers of
  // 56 / 43 KB), so one tile in flight per workgroup is all the memory-level parallelism the CU has: the staging waves hold
  // TWO tiles in registers (the workgroup's 8 waves may use 256 VGPRs each) and request tile it+3 while tile it+1 is converted
  // (two register sets of NPF float4 -- twice that with the saved activation of PRO_BWD -- must leave room: <= 128 VGPRs)
  constexpr int STG_NPF = (IR * IC * (CIN / 4) + 255) / 256;
  constexpr bool DEEP = LIMB && (size_t)2 * TILE_F * sizeof(float) > 80 * 1024 &&
                        STG_NPF * (PRO == PRO_BWD ? 2 : 1) * 8 <= 128;
  decltype(stg) stg2;
  auto stg_store = [&](float* tile) __attribute__((always_inline)) {
    if constexpr (LIMB) stg.store(reinterpret_cast<unsigned char*>(tile), coef);
    else stg.store(tile, coef);
  };
  // stride-2 gathers hold the most staging registers: keeping their first tile in flight across the prologue raised
  // conv2's forward from 70 to 112 VGPRs (3 -> 2 resident workgroups per CU, 42 -> 50 us); they load after it instead
  constexpr bool HOIST = MODE != MODE_DOWN || DEEP;
  if (stager) {
    stg.init();
    if constexpr (DEEP) stg2.init();
    if (HOIST && walk.valid()) {                                // tile 0 goes in flight BEFORE the coefficient prologue
      int b, oy0, ox0, gy0, gx0;
      origin(walk.cur, b, oy0, ox0, gy0, gx0);
      stg.load(a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);
    }
  }
  // The matrix-core waves touch the packed weights now: their fragment loads come after the coefficient barrier, where a
  // first-touch miss (every workgroup of the launch asks for the same 2-27 KB at once) was one more exposed memory latency
  // of the prologue.  The values are only held until the barrier (the loads may not be dropped).
  // (one float per 128-byte line and thread: 256 threads cover 32 KB, the largest weight array is 27 KB)
  static_assert(9 * CIN * COUT * 4 <= 256 * 128, "one touch per thread covers the packed weights");
  float wpf = 0.f;
  __shared__ float ems[64];                 // EPI_BWD: mean [0..31], invstd [32..63] of the statistics the final reduction centres with
  if (!stager) {
    wpf = a.G[min(32 * (t - 256), 9 * CIN * COUT - 1)];
    const int e = t - 320;                  // the second matrix-core wave (the first one finalises the coefficients)
    if (EPI == EPI_BWD && e >= 0 && e < 64) {
      const int c = e & 31;
      ems[e] = c < COUT ? (e < 32 ? a.epi_mean[c] : a.epi_invstd[c]) : 0.f;
    }
  }
  if (a.fin.acc != nullptr) {
    // BatchNorm finalised here from the producer's accumulated sums (bn_acc.h), by the first matrix-core wave under the
    // staging waves' first tile load.  (The staging waves finalising them for themselves, without the barrier below, so that
    // the matrix-core waves build their fragments from the entry on: 15 us per step slower, tools/lab/early_init.patch,
    // profiles/NOTES.md item 40.)
    bn_coef_from_acc(coef, accvals, a.fin, 256);
  } else if (t < 96) {
    const int which = t >> 5, c = t & 31;
    const float* src = which == 0 ? a.pa : (which == 1 ? a.pb : a.pc);
    coef[t] = (src != nullptr && c < CIN) ? src[c] : 0.f;
  }
  __syncthreads();                          // coef[] visible
  if (!stager) asm volatile("" ::"v"(wpf));

  if (stager) {
    // ---------------- staging waves ----------------
    // issue priority over the matrix-core waves of the same SIMD: their loads and LDS stores are the longer pipeline
    // (DESIGN.md section 3, item 16); same-box A/B of the step: 1.9141 / 1.9131 ms without, 1.9087 / 1.8979 ms with (the
    // reverse, matrix-core waves first, costs +26 us)
    __builtin_amdgcn_s_setprio(3);
    int b, oy0, ox0, gy0, gx0;
    if constexpr (DEEP) {
      // tile k of this workgroup's list, clamped to a valid tile behind its end (branch-free loads: see store_load)
      auto tile_k = [&](int k) { const int tl = walk.cur + k * walk.step; return tl < walk.end ? tl : walk.cur; };
      unsigned char* const buf0 = reinterpret_cast<unsigned char*>(tile0);
      unsigned char* const buf1 = reinterpret_cast<unsigned char*>(tile0 + TILE_F);
      if (walk.valid()) {
        origin(tile_k(1), b, oy0, ox0, gy0, gx0);
        stg2.load(a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);                     // tile 1 -> register set 2
        origin(tile_k(2), b, oy0, ox0, gy0, gx0);
        stg.store_load(buf0, coef, a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);    // tile 0 -> buffer 0, tile 2 -> register set 1
      }
      __syncthreads();                                                       // (A)
      int it = 0;
      for (; walk.valid(); walk.advance(), ++it) {
        if (walk.has_next()) {
          origin(tile_k(3), b, oy0, ox0, gy0, gx0);                          // relative to the advancing walk.cur: tile it+3
          if ((it & 1) == 0) stg2.store_load(buf1, coef, a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);
          else stg.store_load(buf0, coef, a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);
        }
        __syncthreads();                                                     // (B)
      }
      if (MSPLIT) __syncthreads();
      __syncthreads();
      __syncthreads();
      return;
    }
    if (walk.valid()) {
      if (!HOIST) {
        origin(walk.cur, b, oy0, ox0, gy0, gx0);
        stg.load(a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);
      }
      stg_store(tile0);                                         // tile 0 -> buffer 0
      if (walk.has_next()) {
        origin(walk.next(), b, oy0, ox0, gy0, gx0);
        stg.load(a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);         // tile 1 in flight
      }
    }
    __syncthreads();                                            // (A) tile 0 ready
    int it = 0;
    for (; walk.valid(); walk.advance(), ++it) {
      // while the matrix-core waves multiply tile `it`, store tile it+1 and fetch tile it+2
      if (walk.has_next()) {
        stg_store(tile0 + ((it + 1) & 1) * TILE_F);
        const int nn = walk.next() + walk.step;
        if (nn < walk.end) {
          origin(nn, b, oy0, ox0, gy0, gx0);
          stg.load(a.in, a.in2, b, a.Hi, a.Wi, gy0, gx0);
        }
      }
      __syncthreads();                                          // (B) tile it consumed, tile it+1 ready
    }
    if (MSPLIT) __syncthreads();                                // (Z) zero-fill barrier of the matrix-core waves
    __syncthreads();                                            // (C) matches the statistics barrier below
    __syncthreads();
    return;
  }

  // ---------------- matrix-core waves ----------------
  const int mtb = MSPLIT ? (wave & 1) : 0;  // first cout tile of this wave
  const int wp = wave >> 1;                 // MSPLIT: which half of the pixel groups
  constexpr int LCIN = LIMB ? CIN : 8;      // (the limb classes need CIN % 8 == 0 even where they are not used)
  typename std::conditional<LIMB, typename std::conditional<PAIR, PairFragL<LCIN, IC, NPIXP, false, NLW, NLB>, ClassFragL<LCIN, COUT, MODE, 0, IC, NPIXP, MT, false, NLW, NLB>>::type,
                            typename std::conditional<PAIR, PairFrag<CIN, IC>, ClassFrag<CIN, COUT, MODE, 0, IC, MT>>::type>::type f0;
  typename std::conditional<LIMB, ClassFragL<LCIN, COUT, MODE, (NCLS > 1 ? 1 : 0), IC, NPIXP, MT, false, NLW, NLB>, ClassFrag<CIN, COUT, MODE, (NCLS > 1 ? 1 : 0), IC, MT>>::type f1;
  typename std::conditional<LIMB, ClassFragL<LCIN, COUT, MODE, (NCLS > 1 ? 2 : 0), IC, NPIXP, MT, false, NLW, NLB>, ClassFrag<CIN, COUT, MODE, (NCLS > 1 ? 2 : 0), IC, MT>>::type f2;
  typename std::conditional<LIMB, ClassFragL<LCIN, COUT, MODE, (NCLS > 1 ? 3 : 0), IC, NPIXP, MT, false, NLW, NLB>, ClassFrag<CIN, COUT, MODE, (NCLS > 1 ? 3 : 0), IC, MT>>::type f3;
  constexpr int SP = MODE == MODE_DOWN ? 2 : 1;
  constexpr int PIXU = LIMB ? 1 : CIN;      // what one pixel is worth in the fragments' offset unit (16-byte slots / floats)
  // (the limb fragments take the weights' limb count as a template parameter; the fp32 fragments round at run time)
  auto finit = [&](auto& f, int pixoff) __attribute__((always_inline)) {
    if constexpr (LIMB) f.init(a.G, lane, pixoff, mtb); else f.init(a.G, lane, pixoff, mtb, BF16M);
  };
  finit(f0, SP * n * PIXU);
  if (NCLS > 1) { finit(f1, n * PIXU); finit(f2, n * PIXU); finit(f3, n * PIXU); }
  // LDS address of pixel `pix` of a tile, in the form the fragments' run() takes
  auto pxp = [&](const float* tile, int pix) __attribute__((always_inline)) {
    if constexpr (LIMB) return reinterpret_cast<const unsigned char*>(tile) + pix * 16;
    else return tile + pix * CIN;
  };
  const int lane_out = PAIR ? ((kg >> 1) * a.Wo + n) * COUT + 4 * (kg & 1) : (MODE == MODE_UP ? 2 * n : n) * COUT + 4 * kg;
  const int cq = PAIR ? 4 * (kg & 1) : 4 * kg;
  float bias[MT][4], s1[MT][4], s2[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = 16 * (mtb + mt) + cq + r;
      bias[mt][r] = (EPI == EPI_FWD && co < COUT) ? a.bias[co] : 0.f;
      s1[mt][r] = s2[mt][r] = 0.f;
      asm volatile("" ::"v"(bias[mt][r]));
    }
  constexpr int GROUPS = PAIR ? (TH / 2) * (TW / 16) : ((MODE == MODE_UP) ? TH * TW / 16 : TH * (TW / 16));
  constexpr int GPW = MSPLIT ? GROUPS / 2 : GROUPS / 4;
  static_assert(GROUPS % 4 == 0 && (!MSPLIT || MODE != MODE_UP || GROUPS % 8 == 0), "tile must split evenly");
  auto group_of = [&](int gi) -> int {
    if (!MSPLIT) return wave * GPW + gi;
    if (MODE == MODE_UP) return 8 * (gi >> 2) + 4 * wp + (gi & 3);
    return wp + 2 * gi;
  };
  auto group_out = [&](int g) -> int {
    if (MODE == MODE_UP) return (((2 * (g >> 2)) + ((g & 3) >> 1)) * a.Wo + (g & 1)) * COUT;
    constexpr int GPR = TW / 16;
    return (((PAIR ? 2 : 1) * (g / GPR)) * a.Wo + 16 * (g % GPR)) * COUT;
  };
  // EPI_BWD: raw x at this lane's output pixels (BatchNorm-backward sums), fetched one tile ahead by the matrix-core
  // waves themselves (they hold no staging registers)
  avaf4 exn[EPI == EPI_BWD ? GPW * MT : 1];
  auto load_ex = [&](int tl) {
    int b, oy0, ox0, gy0, gx0;
    origin(tl, b, oy0, ox0, gy0, gx0);
    const ACT* __restrict__ xb = ava_as<ACT>(a.epi_x) + (((size_t)b * a.Ho + oy0) * a.Wo + ox0) * COUT;
#pragma unroll
    for (int gi = 0; gi < GPW; ++gi)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int cb = 16 * (mtb + mt) + cq;
        exn[gi * MT + mt] = ava_ld4<ACT>(
            xb + group_out(group_of(gi)) + (cb < COUT ? lane_out + 16 * (mtb + mt) : lane_out - 4 * kg));
      }
  };
  if (EPI == EPI_BWD && walk.valid()) load_ex(walk.cur);
  __syncthreads();                                              // (A)
  int it = 0;
  for (; walk.valid(); walk.advance(), ++it) {
    int b, oy0, ox0, gy0, gx0;
    origin(walk.cur, b, oy0, ox0, gy0, gx0);
    const float* tile = tile0 + (it & 1) * TILE_F;
    const size_t tile_pix = ((size_t)b * a.Ho + oy0) * a.Wo + ox0;
    TOUT* __restrict__ obase = a.out != nullptr ? ava_as<TOUT>(a.out) + tile_pix * COUT : nullptr;
    avaf4 ex[GPW * MT];
    if (EPI == EPI_BWD) {
#pragma unroll
      for (int i = 0; i < GPW * MT; ++i) ex[i] = exn[i];
      if (walk.has_next()) load_ex(walk.next());
    }
#pragma unroll
    for (int gi = 0; gi < GPW; ++gi) {
      const int g = group_of(gi);
      f32x4 acc[2][MT];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[h][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (MODE == MODE_UP) {
        const int cls = gi & 3, r = g >> 2;
        const auto px = pxp(tile, r * IC);
        if (cls == 0) f0.run(px, acc);
        else if (cls == 1) f1.run(px, acc);
        else if (cls == 2) f2.run(px, acc);
        else f3.run(px, acc);
      } else {
        constexpr int GPR = TW / 16;
        constexpr int S = (MODE == MODE_S1 && !PAIR) ? 1 : 2;
        constexpr int SX = MODE == MODE_DOWN ? 2 : 1;
        f0.run(pxp(tile, S * (g / GPR) * IC + SX * 16 * (g % GPR)), acc);
      }
      const int gout = group_out(g) + lane_out;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int cb = 16 * (mtb + mt) + cq;
        if (cb < COUT) {
          f32x4 v = acc[0][mt] + acc[1][mt];
          if (EPI == EPI_FWD) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float x = ava_stored<TOUT>(fmaxf(v[r] + bias[mt][r], 0.f));   // statistics of what is stored
              v[r] = x;
              s1[mt][r] += x;
              s2[mt][r] = fmaf(x, x, s2[mt][r]);
            }
          } else {
            const avaf4 xr = ex[gi * MT + mt];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              s1[mt][r] += v[r];
              s2[mt][r] = fmaf(v[r], xr[r], s2[mt][r]);      // raw x: centred after the loop
            }
          }
          if (obase != nullptr) ava_st4<TOUT>(obase + gout + 16 * (mtb + mt), avaf4{v[0], v[1], v[2], v[3]});
        }
      }
    }
    __syncthreads();                                            // (B)
  }
  // ---- per-workgroup partial statistics (matrix-core waves only) ----
  if (MSPLIT) {                              // a wave only fills its own cout tile: the other slots must read as 0
    const int tz = t - 256;
    if (tz < 4 * 32 * MTA / 2) { red[tz] = 0.f; red[tz + 4 * 32 * MTA / 2] = 0.f; }
    __syncthreads();                         // the staging waves take part: see (Z) in their branch
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v1 = s1[mt][r], v2 = s2[mt][r];
      if (EPI == EPI_BWD) {
        // the hot loop accumulates sum g*x on RAW x; centred and scaled once per lane here: sum g*xhat = invstd * (sum g*x - mean * sum g)
        const int cc = 16 * (mtb + mt) + cq + r;
        const float mu = ems[cc & 31], is = ems[32 + (cc & 31)];      // requested in the prologue (zero beyond COUT)
        v2 = fmaf(-mu, v1, v2) * is;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) { v1 += __shfl_xor(v1, o, 64); v2 += __shfl_xor(v2, o, 64); }
      if (PAIR) { v1 += __shfl_xor(v1, 32, 64); v2 += __shfl_xor(v2, 32, 64); }
      if (n == 0 && (!PAIR || kg < 2)) {
        const int co = 16 * (mtb + mt) + cq + r;
        red[wave * 32 * MTA + co] = v1;
        red[wave * 32 * MTA + 16 * MTA + co] = v2;
      }
    }
  __syncthreads();                                              // (C)
  const int tc = t - 256;
  if (tc < 2 * COUT && a.acc_out != nullptr) {
    const int which = tc / COUT, co = tc - which * COUT;
    const int idx = which * 16 * MTA + co;
    bn_acc_add(a.acc_out, which * 32 + co, (red[idx] + red[32 * MTA + idx]) + (red[64 * MTA + idx] + red[96 * MTA + idx]));
  } else if (tc < 2 * COUT && a.partials != nullptr) {
    const int which = tc / COUT, co = tc - which * COUT;
    const int idx = which * 16 * MTA + co;
    a.partials[(size_t)blockIdx.x * 2 * COUT + tc] =
        (red[idx] + red[32 * MTA + idx]) + (red[64 * MTA + idx] + red[96 * MTA + idx]);
    for (int r = gridDim.x + blockIdx.x; r < a.part_rows; r += gridDim.x) a.partials[(size_t)r * 2 * COUT + tc] = 0.f;
  }
  __syncthreads();
}

template <int CIN, int COUT, int MODE, int PRO, int EPI, int TW, int TH, typename ACT, bool LIMB = false>
int launch_mfma_ws_t(const ConvArgs& a, int grid, hipStream_t st) {
  using G = Geom<MODE, TW, TH>;
  constexpr int MT = (COUT + 15) / 16;
  constexpr bool MSPLIT = MT == 2 && CIN >= 16;     // same rules as launch_mfma
  constexpr bool PAIR = MODE == MODE_S1 && COUT == 8;
  using TIN = typename std::conditional<PRO == PRO_BN, ACT, float>::type;
  constexpr int NLB = ava_stager_limbs<TIN, PRO>();                 // limb planes of the staged operand (kernel: TILE_F)
  const size_t lds = (size_t)(2 * (LIMB ? (G::IR * G::IC) * CIN * NLB / 2 : G::IR * G::IC * CIN) + 96 + 4 * 32 * MT) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set && lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_mfma_ws_kernel<CIN, COUT, MODE, PRO, EPI, TW, TH, MSPLIT, PAIR, ACT, LIMB>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return AVA_ELAUNCH;
    attr_set = true;
  }
  ConvArgs b = a;
  b.tiles_y = a.Ho / TH;
  b.tiles_x = a.Wo / TW;
  b.ntiles = a.B * b.tiles_y * b.tiles_x;
  int per_cu = 1;
  static int resident = 0;
  if (resident == 0) {
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&conv3x3_mfma_ws_kernel<CIN, COUT, MODE, PRO, EPI, TW, TH, MSPLIT, PAIR, ACT, LIMB>), 512, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    resident = per_cu * 256;
  }
  b.part_rows = grid;
  if (grid > b.ntiles) grid = b.ntiles;
  if (grid > ava_scale_grid(resident)) grid = ava_scale_grid(resident);
  hipLaunchKernelGGL((conv3x3_mfma_ws_kernel<CIN, COUT, MODE, PRO, EPI, TW, TH, MSPLIT, PAIR, ACT, LIMB>), dim3(grid), dim3(512), lds, st, b);
  AVA_CHECK_LAUNCH();
  return AVA_OK;
}

template <int CIN, int COUT, int MODE, int PRO, int EPI, int TW, int TH>
int launch_mfma_ws(const ConvArgs& a, int grid, hipStream_t st) {
  if constexpr (CIN % 8 == 0 && (CIN >= 16 || PRO == PRO_BN)) {     // the limb form: see the table at the top
    if (a.act_bf16) return launch_mfma_ws_t<CIN, COUT, MODE, PRO, EPI, TW, TH, ava_bf16, true>(a, grid, st);
    return launch_mfma_ws_t<CIN, COUT, MODE, PRO, EPI, TW, TH, float, true>(a, grid, st);
  } else {
    if (a.act_bf16) return launch_mfma_ws_t<CIN, COUT, MODE, PRO, EPI, TW, TH, ava_bf16>(a, grid, st);
    return launch_mfma_ws_t<CIN, COUT, MODE, PRO, EPI, TW, TH, float>(a, grid, st);
  }
}

template <int CIN, int COUT, int MODE, int TW, int TH>
static int launch_ws_pe(const ConvArgs& a, int grid, int pro, int epi, hipStream_t st) {
  if (pro == PRO_BN && epi == EPI_FWD) return launch_mfma_ws<CIN, COUT, MODE, PRO_BN, EPI_FWD, TW, TH>(a, grid, st);
  if (pro == PRO_BWD && epi == EPI_BWD) return launch_mfma_ws<CIN, COUT, MODE, PRO_BWD, EPI_BWD, TW, TH>(a, grid, st);
  if (pro == PRO_ID && epi == EPI_BWD) return launch_mfma_ws<CIN, COUT, MODE, PRO_ID, EPI_BWD, TW, TH>(a, grid, st);
  return AVA_EINVAL;
}

// the same shape table as ava_conv3x3_mfma
int ava_conv3x3_mfma_ws(const ConvArgs& a, int grid, int Cin, int Cout, int mode, int pro, int epi, hipStream_t st) {
#define AVA_WS_CASE(ci, co, md, tww, thh) \
  if (Cin == ci && Cout == co && mode == md && a.Wo % tww == 0 && a.Ho % thh == 0) return launch_ws_pe<ci, co, md, tww, thh>(a, grid, pro, epi, st);
  AVA_WS_CASE(8, 8, MODE_DOWN, 32, 4)
  AVA_WS_CASE(8, 16, MODE_S1, 32, 8)
  AVA_WS_CASE(16, 16, MODE_DOWN, 32, 4)
  AVA_WS_CASE(16, 24, MODE_S1, 32, 4)
  AVA_WS_CASE(24, 24, MODE_DOWN, 16, 4)
  AVA_WS_CASE(24, 32, MODE_S1, 16, 8)
  AVA_WS_CASE(32, 24, MODE_S1, 16, 8)
  AVA_WS_CASE(24, 24, MODE_UP, 32, 8)
  AVA_WS_CASE(24, 16, MODE_S1, 32, 4)
  AVA_WS_CASE(16, 16, MODE_UP, 32, 8)
  AVA_WS_CASE(16, 8, MODE_S1, 32, 8)
  AVA_WS_CASE(8, 8, MODE_UP, 32, 8)
#undef AVA_WS_CASE
  return AVA_EINVAL;
}
