// The sdf MLP forward kernel, included three times by mlp.hip (see the comment there): OI_SDF_LATTICE 0 defines
// sdf_mlp_kernel<PREC, FAST, FULL> (points from pts[]), OI_SDF_LATTICE 1 defines sdf_lattice_kernel<PREC, FAST, false>
// (points from the lattice axes through OI_LATTICE_POINT, output scale * sdf), OI_SDF_LATTICE 2 defines
// sdf_band_kernel<PREC, FAST, false> (points of the listed blocks of the lattice through OI_LATTICE_POINT, output scale * sdf
// scattered into the dense field through OI_LATTICE_STORE).  No include guard, on purpose.
template <int PREC, bool FAST, bool FULL>
__global__ void __launch_bounds__(64 * V2_WAVES, 2)
#if OI_SDF_LATTICE == 2
sdf_band_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs, int lat_nx, int lat_ny,
                int lat_nz, int band_lb, const unsigned* __restrict__ band_list, float scale, const char* __restrict__ packed,
                const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ sdf_out,
                long long n_per_elem) {
  static_assert(!FULL, "the block-list point source serves the sdf-only pass");
  float* const grad_out = nullptr;
  float* const rgb_out = nullptr;
  float* const feat_out = nullptr;
  char* const scratch = nullptr;
#elif OI_SDF_LATTICE
sdf_lattice_kernel(const float* __restrict__ xs, const float* __restrict__ ys, const float* __restrict__ zs, int lat_ny,
                   int lat_nz, float scale, const char* __restrict__ packed, const float* __restrict__ gamma,
                   const float* __restrict__ beta, float* __restrict__ sdf_out, long long n_per_elem) {
  static_assert(!FULL, "the lattice point source serves the sdf-only pass");
  float* const grad_out = nullptr;
  float* const rgb_out = nullptr;
  float* const feat_out = nullptr;
  char* const scratch = nullptr;
#else
sdf_mlp_kernel(const float* __restrict__ pts, const char* __restrict__ packed, const float* __restrict__ gamma,
               const float* __restrict__ beta, float* __restrict__ sdf_out, float* __restrict__ grad_out,
               float* __restrict__ rgb_out, float* __restrict__ feat_out, char* __restrict__ scratch,
               long long n_per_elem) {
#endif
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, j = lane & 31;
  const int e = blockIdx.y;
  const float* hdr = reinterpret_cast<const float*>(packed);
  const char* mats = packed + H_BYTES;
  constexpr int LB = layer_bytes(PREC);
  constexpr bool RING2 = v2_two_slots(PREC);
  constexpr int NWV = V2_WAVES;
  constexpr bool REV = PREC == OI_PREC_F16X3 && !FULL;  // FiLM rows in revolutions (see film_sin2)
  // double-buffered ring: the next image is requested at the START of a layer into the other slot.
  // single slot (BF16X6): it is requested right AFTER the layer's MFMAs, behind a barrier, and lands while the
  // FiLM/sin VALU phase runs.
  LaneOff o;
  o.h16 = 16 * h;
  o.h64 = 64 * h;
  o.l16 = 16 * lane;
  o.l16hi = 16 * lane + 32768;
  asm volatile("" : "+v"(o.h16), "+v"(o.h64), "+v"(o.l16), "+v"(o.l16hi));

  const __amdgpu_buffer_rsrc_t img_rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(mats), 0, NMAT * LB, 0x00020000);
  auto stage_early = [&](int image, int slot) {
    if constexpr (RING2) prefetch_image<PREC, NWV>(lds, img_rs, image * LB, slot, wave, o.l16);
  };
  auto stage_late = [&](int image) {
    if constexpr (!RING2) {
      __syncthreads();
      prefetch_image<PREC, NWV>(lds, img_rs, image * LB, 0, wave, o.l16);
    }
  };

  constexpr int NW = NWV, NT = 64 * NW;
  // PERSISTENT workgroups for the sdf-only passes (round 5; launch_mlp_variant sizes the grid): a workgroup walks tiles
  // blockIdx.x, + gridDim.x, ... of its batch element -- tables and FiLM rows are staged once instead of once per tile, the
  // last layer of a tile requests image 0 of the next one (7 images on a two-slot ring: `rb` swaps the slots per tile).
  constexpr bool PERSIST = !FULL && RING2;
  const int ntiles = (int)((n_per_elem + NW * WAVE_PTS - 1) / (NW * WAVE_PTS));
  int tile = blockIdx.x, rb = 0;
  bool valid;
  long long pt;
  auto set_point = [&](int t_) {
    const long long local = (long long)t_ * (NW * WAVE_PTS) + wave * WAVE_PTS + j;
    valid = local < n_per_elem;
    pt = (long long)e * n_per_elem + (valid ? local : n_per_elem - 1);
  };
  set_point(tile);

  constexpr bool HALF_SCR = PREC == OI_PREC_BF16;
  constexpr int SLOT_B = HALF_SCR ? 8192 : 16384;
  FwdScratch<HALF_SCR> ws;
  {
    const long long wt = ((long long)e * gridDim.x + blockIdx.x) * NW + wave;
    char* wbase = FULL ? scratch + wt * (long long)(NSLOT * SLOT_B) : nullptr;
    ws.rs = __builtin_amdgcn_make_buffer_rsrc(wbase, 0, FULL ? NSLOT * SLOT_B : 0, 0x00020000);
  }

  // image sequence: i = 0..6 forward layers 1..7 (mats 0..6), i = 7..13 transposed layers 7..1 (mats 13..7),
  // i = 14 colour head (mat 14); image i lives in ring slot i & 1.
  prefetch_image<PREC, NWV>(lds, img_rs, 0, 0, wave, o.l16);
  {  // small tables + FiLM rows of all 9 layers (gamma | beta | bias), once
    float* tabs = reinterpret_cast<float*>(lds + V2_TABS);
    for (int i = tid; i < H_TABS_END; i += NT) tabs[i] = hdr[i];
    float* film = reinterpret_cast<float*>(lds + V2_FILM);
    for (int i = tid; i < 9 * C; i += NT) {
      const int l = i / C, f = i % C;
      const float gm = gamma[((size_t)e * 9 + l) * C + f];
      // image scale of the layer's MFMA operand folded into the multiplier of u (layer 0 runs on the VALU)
      const float ws = l == 0 ? 1.f : hdr[H_WSCALE + (l < NL_SDF ? l - 1 : 14)];
      constexpr float TO_REV = REV ? 0.15915494309189533577f : 1.f;
      film[l * 256 + f] = gm * ws * TO_REV;
      film[l * 256 + C + f] = fmaf(gm, hdr[H_BIAS + l * C + f], beta[((size_t)e * 9 + l) * C + f]) * TO_REV;
    }
  }
#if OI_SDF_LATTICE
  float px, py, pz;
  OI_LATTICE_POINT(px, py, pz);
#else
  float px = pts[pt * 3 + 0], py = pts[pt * 3 + 1], pz = pts[pt * 3 + 2];
#endif
  __syncthreads();  // tables visible (image 0 still in flight)

  float act[64];
  f32x16 acc[4];
#ifdef OI_PROF
  unsigned long long pacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long tprev = __builtin_readcyclecounter();
  const unsigned long long tstart = tprev;
#endif
  for (;;) {  // ---- one tile per trip (exactly one unless PERSIST)
  const int ntile = tile + (int)gridDim.x;
  float nx = 0.f, ny = 0.f, nz = 0.f;
  if constexpr (PERSIST) {  // the next tile's point, used a tile later (a clamped re-read of this one on the last trip)
    set_point(ntile < ntiles ? ntile : tile);
#if OI_SDF_LATTICE
    OI_LATTICE_POINT(nx, ny, nz);
#else
    nx = pts[pt * 3 + 0], ny = pts[pt * 3 + 1], nz = pts[pt * 3 + 2];
#endif
    set_point(tile);
  }

  // ---- layer 0 (K = 3) on the VALU, overlapping the first image's DMA
  {
    const LayOff y = lay_off<PREC>(o, 0, 0);
    film_sin2<FAST, FULL, 1, FwdScratch<HALF_SCR>, REV>(lds, o, y, acc, act, ws, 0, H_TAB0, px, py, pz);
  }
  PROF_T(0);
  ring_sync();
  PROF_T(4);

  // ---- layers 1..7 on MFMA
  for (int l = 1; l < NL_SDF; ++l) {
    const int i = l - 1;
    // next image: forward layer l+1, or the first transposed image (layer 7) / nothing for the sdf-only variant
    const int next = (l < NL_SDF - 1) ? l : (FULL ? 13 : (PERSIST ? 0 : -1));  // image index, -1: none; PERSIST: the next tile's first
    if (next >= 0) stage_early(next, ((i + 1) & 1) ^ rb);
    const LayOff y = lay_off<PREC>(o, RING2 ? ((i & 1) ^ rb) : 0, l);
    if constexpr (PREC == OI_PREC_F16X3 && RING2) {
      layer_fwd_pipelined<FAST, FULL, REV>(lds, o, y, acc, act, ws, l);
      PROF_T(1);
    } else
    {
      zero_acc(acc);
      gemm_layer2<PREC>(lds, y, act, acc);
      PROF_T(1);
      if (next >= 0) stage_late(next);
      PROF_T(2);
      film_sin2<FAST, FULL, 0, FwdScratch<HALF_SCR>, REV>(lds, o, y, acc, act, ws, l, 0, 0.f, 0.f, 0.f);
    }
    PROF_T(3);
    ring_sync();
    PROF_T(4);
  }

  // ---- sdf = a8 . wsig + bsig   (fields.py:68; LinearLayer std_init=1, bias_init=0)
  float sdf_v;
  {
    float part = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const f32x4 w = lds_f4(lds, V2_TABS + (H_SIG + grp_f0(g)) * 4, o.h16);
#pragma unroll
      for (int k = 0; k < 4; ++k) part = fmaf(act[4 * g + k], w[k], part);
    }
    part += __shfl_xor(part, 32, 64);
    sdf_v = part + *reinterpret_cast<const float*>(lds + V2_TABS + (H_SIG + C) * 4);
  }
#if OI_SDF_LATTICE == 2
  if (valid && h == 0) OI_LATTICE_STORE(scale * sdf_v);
#elif OI_SDF_LATTICE
  if (valid && h == 0) sdf_out[pt] = scale * sdf_v;
#else
  if (valid && h == 0) sdf_out[pt] = sdf_v;
#endif

  if (feat_out != nullptr && valid) {
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = act[4 * g + k];
      *reinterpret_cast<f32x4*>(feat_out + pt * C + grp_f0(g) + 4 * h) = v;
    }
  }

  if (!PERSIST || ntile >= ntiles) break;
  tile = ntile;
  rb ^= 1;
  set_point(tile);
  px = nx, py = ny, pz = nz;
  }  // tiles

  if constexpr (FULL) {
    // park the features (slot 8) and start the reverse sweep with g8 = wsig
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      f32x4 v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = act[4 * g + k];
      ws.store(8, g, o, v);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const f32x4 w = lds_f4(lds, V2_TABS + (H_SIG + grp_f0(g)) * 4, o.h16);
#pragma unroll
      for (int k = 0; k < 4; ++k) act[4 * g + k] = w[k];
    }
    float run = 1.f;
    // gamma * cos(phi) of the layer about to be swept: requested ONE GEMM AHEAD (inside the previous layer's MFMA loop,
    // into registers the consumed B operand has just freed) so that the HBM latency hides under the MFMAs instead of
    // stalling the top of every layer
    f32x4 cn[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) cn[g] = ws.load(NL_SDF - 1, g, o);
    for (int l = NL_SDF - 1; l >= 1; --l) {
      const int i = 14 - l;  // image index of transposed layer l
#pragma unroll
      for (int g = 0; g < 16; ++g) {
#pragma unroll
        for (int k = 0; k < 4; ++k) act[4 * g + k] *= cn[g][k];
      }
      if constexpr (PREC == OI_PREC_F16X3) {
        // adjoints have no a-priori range: bring this point's vector (its 128 entries live in lanes j and j+32)
        // to max |.| in [2^13, 2^14) with an exact power-of-two scale.  The scale is NOT undone layer by layer: `run`
        // carries the product of the inverse scales (true vector = act * run) and multiplies the final gradient once.
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < 64; k += 2) m = fmaxf(m, fmaxf(fabsf(act[k]), fabsf(act[k + 1])));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        int eb = (__builtin_bit_cast(int, m) >> 23) & 0xff;
        eb = eb < 14 ? 14 : (eb > 254 ? 254 : eb);
        float sc = __builtin_bit_cast(float, (267 - eb) << 23);  // 2^(13 - (eb - 127))
        // fence tied to sc (= to every c * g product): keeps the GEMM's A-fragment ds_reads from being scheduled
        // into the scratch-load phase while the 64 c registers are still live (140 spilled VGPRs otherwise)
        asm volatile("" : "+v"(sc) : : "memory");
        run *= __builtin_bit_cast(float, (eb - 13) << 23);             // 1 / sc
#pragma unroll
        for (int k = 0; k < 64; ++k) act[k] *= sc;
      }
      // next image after the scratch loads have been consumed (an in-flight LDS-DMA would otherwise be
      // drained by the vmcnt wait hipcc places in front of the first use of an ordinary load)
      const int next = (l > 1) ? 7 + l - 2 : (rgb_out != nullptr ? 14 : -1);
      if (next >= 0) stage_early(next, (i + 1) & 1);
      const LayOff y = lay_off<PREC>(o, RING2 ? (i & 1) : 0, l);
      zero_acc(acc);
      PROF_T(5);
      gemm_layer2<PREC>(lds, y, act, acc, [&](int s) {
        cn[2 * s] = ws.load(l - 1, 2 * s, o);
        cn[2 * s + 1] = ws.load(l - 1, 2 * s + 1, o);
      });
      PROF_T(6);
      if (next >= 0) stage_late(next);
      PROF_T(7);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) act[16 * t + r] = acc[t][r];
      ring_sync();
      PROF_T(8);
    }
    // layer 0: grad = W0^T (g1 * c0)
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const f32x4 c = cn[g];  // slot 0, requested during the last transposed GEMM
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float v = act[4 * g + k] * c[k];
        const f32x4 w = lds_f4(lds, V2_TABS + H_TAB0 * 4 + (grp_f0(g) + k) * 16, o.h64);
        gx = fmaf(v, w[0], gx);
        gy = fmaf(v, w[1], gy);
        gz = fmaf(v, w[2], gz);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    gx += __shfl_xor(gx, 32, 64);
    gy += __shfl_xor(gy, 32, 64);
    gz += __shfl_xor(gz, 32, 64);
    gx *= run;  // identical in both lanes of a point (the max was taken over the pair)
    gy *= run;
    gz *= run;
    if (valid && h == 0) {
      grad_out[pt * 3 + 0] = gx;
      grad_out[pt * 3 + 1] = gy;
      grad_out[pt * 3 + 2] = gz;
    }

    if (rgb_out != nullptr) {
      // ---- colour head: sigmoid(Wrgb sin(gv * (Wv [feat, grad] + bv) + bv') + brgb)   (fields.py:89-101)
      // image 14 (ring slot 0) was prefetched during transposed layer 1 and is resident after its ring_sync
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const f32x4 v = ws.load(8, g, o);
#pragma unroll
        for (int k = 0; k < 4; ++k) act[4 * g + k] = v[k];
        if ((g & 3) == 3) __builtin_amdgcn_sched_barrier(0);
      }
      const LayOff y = lay_off<PREC>(o, 0, 8);
      zero_acc(acc);
      gemm_layer2<PREC>(lds, y, act, acc);
      // the accumulators carry the image scale 2^k (1 unless F16X3): bring the rank-3 gradient term to the same scale
      const float cs = 1.0f / hdr[H_WSCALE + 14];
      film_sin2<FAST, false, 2>(lds, o, y, acc, act, ws, 0, H_TABV, gx * cs, gy * cs, gz * cs);
      float r0 = 0.f, r1 = 0.f, r2 = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const f32x4 w0 = lds_f4(lds, V2_TABS + (H_RGB + 0 * C + grp_f0(g)) * 4, o.h16);
        const f32x4 w1 = lds_f4(lds, V2_TABS + (H_RGB + 1 * C + grp_f0(g)) * 4, o.h16);
        const f32x4 w2 = lds_f4(lds, V2_TABS + (H_RGB + 2 * C + grp_f0(g)) * 4, o.h16);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          r0 = fmaf(act[4 * g + k], w0[k], r0);
          r1 = fmaf(act[4 * g + k], w1[k], r1);
          r2 = fmaf(act[4 * g + k], w2[k], r2);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      r0 += __shfl_xor(r0, 32, 64);
      r1 += __shfl_xor(r1, 32, 64);
      r2 += __shfl_xor(r2, 32, 64);
      if (valid && h == 0) {
        const float* brgb = reinterpret_cast<const float*>(lds + V2_TABS + (H_RGB + 3 * C) * 4);
        rgb_out[pt * 3 + 0] = oi::sigmoidf_(r0 + brgb[0]);
        rgb_out[pt * 3 + 1] = oi::sigmoidf_(r1 + brgb[1]);
        rgb_out[pt * 3 + 2] = oi::sigmoidf_(r2 + brgb[2]);
      }
    }
  }
#ifdef OI_PROF
  PROF_T(9);
  if (lane == 0 && FULL) {
    for (int i = 0; i < 10; ++i) atomicAdd(&oi_prof[i], pacc[i]);
    atomicAdd(&oi_prof[10], __builtin_readcyclecounter() - tstart);
    atomicAdd(&oi_prof[11], 1ull);
  }
#endif
}

