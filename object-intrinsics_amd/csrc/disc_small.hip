// DC discriminator forward at batch 1-4 (the per-GPU batch of training and of the D-images/s metric), gfx950.
//
// Replaces, for the 64 x 64 / n_feat 512 network of configs/train.yaml (reference src/models/discriminator.py:57-85 with
// AugmentPipe.forward, src/third_party/ada/augment.py:284-301, in front), the nine dependent launches of the general path
// (csrc/disc.hip: pad + up-FIR | resample + down-FIR | five split-K MFMA convolutions | copies) by FIVE (four when the canvas is built inside d_aug_conv1_kernel<true>, see there):
//     ada_pad_up2_kernel (disc.hip)                         canvas
//     d_aug_conv1_kernel       resample + down-FIR + conv 1 + LeakyReLU           (C -> 64, 64^2 -> 32^2)
//     d_conv_small_kernel x 3  conv 2, conv 3, conv 4 (+ the 4 x 4 head)          (64 -> 128 -> 256 -> 512 -> out_dim)
// At these sizes a layer is a weight stream (0.5 / 2 / 8 MB) against 0.03 GFLOP and a handful of output pixels: what
// matters is that every load of a layer is in flight at once and that nothing waits on another workgroup.
//   * d_conv_small_kernel: one workgroup per output channel; the INPUT CHANNEL sits on the lane (64 per wave), a wave owns
//     16 output pixels and one 64-channel block of the K sum: 4 weight loads + <= 32 input loads per lane, all issued
//     before the first multiply -- ONE memory round trip per layer instead of one per K chunk (the split-K MFMA kernel
//     walks its K range in trips of 8 kernel rows, each a full round trip: 8 us per layer at batch 1).  The 16 pixel sums
//     of a wave are reduced over the lanes with a transposed butterfly, then over the waves through LDS: fixed summation
//     order, no atomics, bit-reproducible.  fp32 FMA on the vector units: with <= 64 output pixels per image the 32-wide
//     matrix-core tile would be 3/4 padding, and the layer is bandwidth-bound either way (the batch >= 16 path of disc.hip
//     stays on the matrix cores).
//   * the head (512 x 4 x 4 -> out_dim) rides on conv 4: every workgroup adds its channel's share of the logits to a
//     partial table, the LAST workgroup to arrive sums the table in channel order (agent-scope write-through hand-off as in
//     render.hip's compositing statistics; nobody spins).
//   * d_aug_conv1_kernel: an 8 x 8 tile of the augmented image (+ the convolution's halo) is resampled from the canvas into
//     LDS (30 x 30 grid points per channel), filtered down (12 taps, both axes) and convolved (4 x 4 stride 2, 64 channels)
//     without leaving the workgroup; the sampling matrix arrives BY VALUE in the kernel arguments (no host-to-device copy).
#include "oi_common.h"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

// ---- shared with disc.hip (same expressions) ------------------------------------------------------------------------
__device__ __forceinline__ void affine_src_s(const float* th, int ox, int oy, int Wo, int Ho, int Wi, int Hi, float& ix,
                                             float& iy) {
  const float xn = (2.0f * ox + 1.0f) / Wo - 1.0f;  // affine_grid base grid, align_corners=False
  const float yn = (2.0f * oy + 1.0f) / Ho - 1.0f;
  const float gx = th[0] * xn + th[1] * yn + th[2];
  const float gy = th[3] * xn + th[4] * yn + th[5];
  ix = ((gx + 1.0f) * Wi - 1.0f) * 0.5f;  // grid_sampler unnormalize, align_corners=False
  iy = ((gy + 1.0f) * Hi - 1.0f) * 0.5f;
}

constexpr int DS_MAX_B = 4, DS_MAX_C = 4;
constexpr int DA_T = 4;                    // augmented-image tile edge (-> 2 x 2 outputs of conv 1): 256 workgroups per image
constexpr int DA_P = DA_T + 2;             // 6: + the convolution's halo (pad 1, 4 taps, stride 2)
constexpr int DA_TAPS = 12, DA_PAD = 6;    // Hz_geom; the resampled grid is 2 (H + 6) x 2 (W + 6)
constexpr int DA_G = 2 * DA_P + DA_TAPS - 2;  // 22 grid points per axis under a patch

struct ThetaArg {
  float t[DS_MAX_B][6];
};

__device__ __forceinline__ int reflect_idx_s(int i, int n) {   // (disc.hip's reflect_idx)
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// FOLD: the canvas (reflect pad + x2 up-FIR: disc.hip's ada_pad_up2_kernel) is not read from memory -- the workgroup builds the
// canvas pixels its 22 x 22 grid points touch (their bounding box, <= DA_CT per axis) in LDS from the source image, with the
// SAME two passes and the same association of the sums as that kernel (bit-identical), and resamples from there: one launch
// and its boundary less.  The launcher checks on the host that the footprint fits (fold_fits), else it takes the canvas form.
constexpr int DA_CT = 40;                  // canvas tile capacity per axis (identity scale needs 24; scale 0.57 fills it)
constexpr int DA_PS = DA_CT / 2 + 6;       // 26: padded-image rows / columns under a canvas tile

// x [B][C][H][W] (theta_on = 0: no augmentation; FOLD: the image the canvas is built from) or canvas [B][C][Hc][Wc]
//   -> y [B][C1][H/2][W/2] = lrelu(conv1(aug(x)))
template <bool FOLD>
__global__ void __launch_bounds__(256)
d_aug_conv1_kernel(const float* __restrict__ src, const ThetaArg th, const float* __restrict__ theta_dev, int theta_on,
                   const float* __restrict__ f,
                   const float* __restrict__ w1, float* __restrict__ y, int C, int H, int W, int Hc, int Wc, int C1, float slope,
                   int mx0, int my0) {
  __shared__ float aug[DS_MAX_C][DA_P][DA_P + 1]; // augmented patch (zero outside the image: the convolution's padding)
  __shared__ float fs[DA_TAPS];
  // g: resampled grid patch; gv: after the vertical pass.  FOLD adds cv (canvas tile), ps (padded-image patch), tm (after the
  // row pass); ps and tm are dead before g / gv are written and share their memory
  constexpr int G_FLOATS = DS_MAX_C * DA_G * (DA_G + 1), GV_FLOATS = DS_MAX_C * DA_P * (DA_G + 1);
  constexpr int TM_FLOATS = FOLD ? DS_MAX_C * DA_PS * (DA_CT + 1) : 0, PS_FLOATS = FOLD ? DS_MAX_C * DA_PS * (DA_PS + 1) : 0;
  __shared__ float pool_a[G_FLOATS > TM_FLOATS ? G_FLOATS : TM_FLOATS];
  __shared__ float pool_b[GV_FLOATS > PS_FLOATS ? GV_FLOATS : PS_FLOATS];
  __shared__ float cv_[FOLD ? DS_MAX_C * DA_CT * (DA_CT + 1) : 1];
  __shared__ float fr[FOLD ? DA_TAPS : 1];
  float (*g)[DA_G][DA_G + 1] = reinterpret_cast<float (*)[DA_G][DA_G + 1]>(pool_a);
  float (*gv)[DA_P][DA_G + 1] = reinterpret_cast<float (*)[DA_P][DA_G + 1]>(pool_b);
  float (*tm)[DA_PS][DA_CT + 1] = reinterpret_cast<float (*)[DA_PS][DA_CT + 1]>(pool_a);
  float (*ps)[DA_PS][DA_PS + 1] = reinterpret_cast<float (*)[DA_PS][DA_PS + 1]>(pool_b);
  float (*cv)[DA_CT][DA_CT + 1] = reinterpret_cast<float (*)[DA_CT][DA_CT + 1]>(cv_);
  const int tid = threadIdx.x, b = blockIdx.z;
  const int ay0 = blockIdx.y * DA_T - 1, ax0 = blockIdx.x * DA_T - 1;  // patch origin in the augmented image
  // conv 1 weights of this thread's output channel: requested now, used after the last barrier (their round trip would
  // otherwise sit at the end of the kernel, behind everything)
  constexpr int OTT = (DA_T / 2) * (DA_T / 2);
  float4 wq[DS_MAX_C][4];
  {
    const int ch = min(tid / OTT, C1 - 1);
#pragma unroll
    for (int c_ = 0; c_ < DS_MAX_C; ++c_)
#pragma unroll
      for (int ky = 0; ky < 4; ++ky)
        wq[c_][ky] = c_ < C ? *reinterpret_cast<const float4*>(w1 + ((size_t)ch * C + c_) * 16 + ky * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (theta_on) {
    if (tid < DA_TAPS) fs[tid] = f[tid];  // flip_filter = True: the correlation taps are the filter itself
    const int Ho = 2 * (H + DA_PAD), Wo = 2 * (W + DA_PAD);
    const int gy0 = 2 * ay0 + 1, gx0 = 2 * ax0 + 1;  // aug[a][b] = sum_{k,l} f[k] f[l] G[2 a + k + 1][2 b + l + 1]
    int u0 = 0, v0 = 0;   // FOLD: canvas coordinates of cv[.][0][0] (even)
    if constexpr (FOLD) {
      if (tid < DA_TAPS) fr[tid] = 2.0f * f[DA_TAPS - 1 - tid];  // up-FIR correlation taps: reversed, sqrt(gain) = 2 per axis
      // bounding box of the canvas pixels the tile's grid points touch: the map is affine, so the extremes sit at the corners of
      // the in-range part of the 22 x 22 grid patch (points outside the grid carry zero weights: what they read is unused)
      int bbox[4] = {0x7fffffff, 0x7fffffff, -1, -1};   // [min y, min x, max y, max x]
      {
        float tb[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) tb[q] = theta_dev != nullptr ? theta_dev[b * 6 + q] : th.t[b][q];
        const int ya = max(gy0, 0), yb = min(gy0 + DA_G - 1, Ho - 1), xa = max(gx0, 0), xb = min(gx0 + DA_G - 1, Wo - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float ix, iy;
          affine_src_s(tb, (k & 1) ? xb : xa, (k & 2) ? yb : ya, Wo, Ho, Wc, Hc, ix, iy);
          const int x0 = (int)floorf(ix), y0 = (int)floorf(iy);
          bbox[0] = min(bbox[0], min(max(y0, 0), Hc - 1));
          bbox[1] = min(bbox[1], min(max(x0, 0), Wc - 1));
          bbox[2] = max(bbox[2], min(max(y0 + 1, 0), Hc - 1));
          bbox[3] = max(bbox[3], min(max(x0 + 1, 0), Wc - 1));
        }
      }
      u0 = bbox[0] & ~1;
      v0 = bbox[1] & ~1;
      const int TH = min(bbox[2] - u0 + 1, DA_CT), TW = min(bbox[3] - v0 + 1, DA_CT);   // (<= DA_CT: checked by the launcher)
      const int r_min = u0 / 2 - 3, c_min = v0 / 2 - 3;       // padded-image index of the first tap of canvas row u0 / column v0
      const int NR = TH / 2 + 6, NC = TW / 2 + 6;             // rows / columns of the padded image under the tile (<= DA_PS)
      const int Hp = Hc / 2, Wp = Wc / 2;
      // thread -> (row, column) with power-of-two strides: run-time divisors cost more than the idle lanes
      {
        const int bb = tid & 31, a0 = tid >> 5;               // 32 columns x 8 rows per step (NC <= 26)
        const int c = c_min + bb;
        const bool c_ok = bb < NC && c >= 0 && c < Wp;
        const int cs = reflect_idx_s(min(max(c, 0), Wp - 1) - mx0, W);
        float pv[4][DS_MAX_C];                                // every load of the patch in flight before the first store
#pragma unroll
        for (int k = 0; k < 4; ++k) {                         // (NR <= 26 = 4 steps of 8 rows; rows past NR: a clamped, harmless load)
          const int r = r_min + a0 + 8 * k;
          const int rs = reflect_idx_s(min(max(r, 0), Hp - 1) - my0, H);
#pragma unroll
          for (int c_ = 0; c_ < DS_MAX_C; ++c_)
            pv[k][c_] = c_ < C ? src[(((size_t)b * C + c_) * H + rs) * W + cs] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int a = a0 + 8 * k, r = r_min + a;
          const bool ok = c_ok && r >= 0 && r < Hp;
          if (a < NR && bb < NC)
#pragma unroll
            for (int c_ = 0; c_ < DS_MAX_C; ++c_)
              if (c_ < C) ps[c_][a][bb] = ok ? pv[k][c_] : 0.f;
        }
      }
      __syncthreads();
      {
        const int vl = tid & 63, a0 = tid >> 6;               // 64 columns (TW <= 40) x 4 rows per step
        const int kv = vl & 1, pl = (vl + kv) / 2;
        if (vl < TW)
          for (int a = a0; a < NR; a += 4)                    // rows: the six taps k = kv, kv + 2, .. (ada_pad_up2_kernel's order)
            for (int c_ = 0; c_ < C; ++c_) {
              float s_ = 0.f;
#pragma unroll
              for (int q = 0; q < 6; ++q) s_ = fmaf(fr[kv + 2 * q], ps[c_][a][pl + q], s_);
              tm[c_][a][vl] = s_;
            }
      }
      __syncthreads();
      {
        const int vl = tid & 63, ul0 = tid >> 6;
        if (vl < TW)
          for (int ul = ul0; ul < TH; ul += 4) {              // columns
            const int ku = ul & 1, pl = (ul + ku) / 2;
            for (int c_ = 0; c_ < C; ++c_) {
              float acc = 0.f;
#pragma unroll
              for (int q = 0; q < 6; ++q) acc = fmaf(fr[ku + 2 * q], tm[c_][pl + q][vl], acc);
              cv[c_][ul][vl] = acc;
            }
          }
      }
      __syncthreads();   // (tm is dead: g may be written)
    }
    for (int i = tid; i < DA_G * DA_G; i += 256) {
      const int r = i / DA_G, c = i % DA_G;
      const int gyi = gy0 + r, gxi = gx0 + c;
      const bool in = gyi >= 0 && gyi < Ho && gxi >= 0 && gxi < Wo;
      float ix, iy;
      float tb[6];   // the sampling matrix: by value (eager callers) or from device memory (captured graphs)
#pragma unroll
      for (int q = 0; q < 6; ++q) tb[q] = theta_dev != nullptr ? theta_dev[b * 6 + q] : th.t[b][q];
      affine_src_s(tb, in ? gxi : 0, in ? gyi : 0, Wo, Ho, Wc, Hc, ix, iy);
      const float fx = floorf(ix), fy = floorf(iy);
      const int x0 = (int)fx, y0 = (int)fy;
      const float tx = ix - fx, ty = iy - fy;
      // unconditional loads from clamped addresses, out-of-range taps zeroed through their weights (a branch per tap made
      // the four loads of a point four dependent round trips)
      const bool xa = x0 >= 0 && x0 < Wc, xb = x0 + 1 >= 0 && x0 + 1 < Wc, ya = y0 >= 0 && y0 < Hc, yb = y0 + 1 >= 0 && y0 + 1 < Hc;
      const int cx0 = min(max(x0, 0), Wc - 1), cx1 = min(max(x0 + 1, 0), Wc - 1);
      const int cy0 = min(max(y0, 0), Hc - 1), cy1 = min(max(y0 + 1, 0), Hc - 1);
      const float w00 = (in && xa && ya) ? (1.f - tx) * (1.f - ty) : 0.f, w01 = (in && xb && ya) ? tx * (1.f - ty) : 0.f;
      const float w10 = (in && xa && yb) ? (1.f - tx) * ty : 0.f, w11 = (in && xb && yb) ? tx * ty : 0.f;
      for (int c_ = 0; c_ < C; ++c_) {
        float v00, v01, v10, v11;
        if constexpr (FOLD) {
          const int ly0 = min(max(cy0 - u0, 0), DA_CT - 1), ly1 = min(max(cy1 - u0, 0), DA_CT - 1);
          const int lx0 = min(max(cx0 - v0, 0), DA_CT - 1), lx1 = min(max(cx1 - v0, 0), DA_CT - 1);
          v00 = cv[c_][ly0][lx0]; v01 = cv[c_][ly0][lx1];
          v10 = cv[c_][ly1][lx0]; v11 = cv[c_][ly1][lx1];
        } else {
          const float* cp = src + ((size_t)b * C + c_) * Hc * Wc;
          v00 = cp[(size_t)cy0 * Wc + cx0]; v01 = cp[(size_t)cy0 * Wc + cx1];
          v10 = cp[(size_t)cy1 * Wc + cx0]; v11 = cp[(size_t)cy1 * Wc + cx1];
        }
        float v = 0.f;   // (the order of disc.hip's ada_resample_down2_kernel)
        v += v00 * w00;
        v += v01 * w01;
        v += v10 * w10;
        v += v11 * w11;
        g[c_][r][c] = v;
      }
    }
    __syncthreads();
    for (int i = tid; i < C * DA_P * DA_G; i += 256) {  // vertical pass
      const int c_ = i / (DA_P * DA_G), t = (i / DA_G) % DA_P, c = i % DA_G;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < DA_TAPS; ++k) s = fmaf(fs[k], g[c_][2 * t + k][c], s);
      gv[c_][t][c] = s;
    }
    __syncthreads();
    for (int i = tid; i < C * DA_P * DA_P; i += 256) {  // horizontal pass
      const int c_ = i / (DA_P * DA_P), t = (i / DA_P) % DA_P, u = i % DA_P;
      float s = 0.f;
#pragma unroll
      for (int l = 0; l < DA_TAPS; ++l) s = fmaf(fs[l], gv[c_][t][2 * u + l], s);
      const int ay = ay0 + t, ax = ax0 + u;
      aug[c_][t][u] = (ay >= 0 && ay < H && ax >= 0 && ax < W) ? s : 0.f;
    }
  } else {
    for (int i = tid; i < C * DA_P * DA_P; i += 256) {
      const int c_ = i / (DA_P * DA_P), t = (i / DA_P) % DA_P, u = i % DA_P;
      const int ay = ay0 + t, ax = ax0 + u;
      const bool in = ay >= 0 && ay < H && ax >= 0 && ax < W;
      const float v = src[(((size_t)b * C + c_) * H + min(max(ay, 0), H - 1)) * W + min(max(ax, 0), W - 1)];
      aug[c_][t][u] = in ? v : 0.f;
    }
  }
  __syncthreads();
  // conv 1: C1 channels x (DA_T / 2)^2 outputs of this tile; K = 16 C taps per output, summed (c, ky, kx)-major.
  // Output in the layout the next layer reads with the input channel on the lane: y[b][oy][ox / 4][ch][ox % 4]
  constexpr int OT = DA_T / 2;
  const int Ho1 = H / 2, Wo1 = W / 2;
  static_assert(OT * OT * 64 == 256, "one conv 1 output per thread (C1 <= 64: 64 channels at 64 x 64, 32 at 128 x 128)");
  if (tid < C1 * OT * OT) {
    const int ch = tid / (OT * OT), py = (tid / OT) % OT, px = tid % OT;
    float acc = 0.f;
#pragma unroll
    for (int c_ = 0; c_ < DS_MAX_C; ++c_) {
      if (c_ < C) {
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
          const float4 wv = wq[c_][ky];
          const float* ar = &aug[c_][2 * py + ky][2 * px];
          acc = fmaf(wv.x, ar[0], acc);
          acc = fmaf(wv.y, ar[1], acc);
          acc = fmaf(wv.z, ar[2], acc);
          acc = fmaf(wv.w, ar[3], acc);
        }
      }
    }
    const int oy = blockIdx.y * OT + py, ox = blockIdx.x * OT + px;
    if (oy < Ho1 && ox < Wo1) y[((((size_t)b * Ho1 + oy) * (Wo1 / 4) + ox / 4) * C1 + ch) * 4 + (ox & 3)] = acc > 0.f ? acc : acc * slope;
  }
}

// ---- conv 2 .. 4 ------------------------------------------------------------------------------------------------------
// sum over the 64 lanes of v[i], i < 16: lane l returns the total of v[l & 15] (transposed butterfly: at step s two registers
// become one -- each lane keeps the partial sum of the value its lane bit s selects)
__device__ __forceinline__ float xpose_sum16(const float (&v)[16], int lane) {
  float a[8], b[4], c[2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool bit = lane & 1;
    const float keep = bit ? v[2 * i + 1] : v[2 * i], give = bit ? v[2 * i] : v[2 * i + 1];
    a[i] = keep + __shfl_xor(give, 1, 64);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool bit = lane & 2;
    const float keep = bit ? a[2 * i + 1] : a[2 * i], give = bit ? a[2 * i] : a[2 * i + 1];
    b[i] = keep + __shfl_xor(give, 2, 64);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const bool bit = lane & 4;
    const float keep = bit ? b[2 * i + 1] : b[2 * i], give = bit ? b[2 * i] : b[2 * i + 1];
    c[i] = keep + __shfl_xor(give, 4, 64);
  }
  const bool bit = lane & 8;
  float d = (bit ? c[1] : c[0]) + __shfl_xor(bit ? c[0] : c[1], 8, 64);
  d += __shfl_xor(d, 16, 64);
  d += __shfl_xor(d, 32, 64);
  return d;   // value index (lane & 15): bit s of the index was selected by lane bit s
}

// Activations between the layers live in the layout  A[b][y][x / 4][channel][x % 4]:  with the input channel on the lane a
// wave's float4 load of (y, x / 4) is 1 KiB of consecutive memory (channel-major planes gave 64 different cache lines per
// load instruction: the address path, not the data, then set the layer's time).
//   x A[B][HIN][HIN/4][CIN][4] -> y A[B][HO][HO/4][COUT][4] = lrelu(conv4x4 s2 p1 (x, w)), w [COUT][CIN][4][4], HO = HIN / 2.
// grid (COUT / NCH, wave tasks / WPB); block 64 WPB.  A wave task = (64-channel block cb of the K sum, 16 consecutive output
// pixels) for NCH output channels (they share the input registers); the tasks of one pixel group sit in one workgroup.
// HEAD (HIN = 8 only): logits[b][k] = bhead[k] + sum_{n, p} whead[k][n][p] y[b][n][p] (4 x 4 valid convolution), combined
// by the last workgroup to arrive.
template <int CIN, int HIN, int WPB, int NCH, bool HEAD>
__global__ void __launch_bounds__(64 * WPB)
d_conv_small_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int B, int COUT, float slope,
                    const float* __restrict__ whead, const float* __restrict__ bhead, int KOUT, float* __restrict__ partials,
                    unsigned* __restrict__ ticket, float* __restrict__ logits) {
  constexpr int HO = HIN / 2, CW = CIN / 64;
  constexpr int RPP = 16 / HO;            // output rows per wave task: 1 (HO 16), 2 (HO 8), 4 (HO 4)
  constexpr int NIR = 2 * RPP + 2;        // input rows under them
  constexpr int Q = HIN / 4;              // float4 per input row
  constexpr int NG = WPB / CW;            // pixel groups per workgroup
  static_assert(RPP * HO == 16 && WPB % CW == 0, "wave task = 16 output pixels x one 64-channel block");
  __shared__ float red[WPB][NCH][16];
  __shared__ float act[DS_MAX_B][NCH][16];
  __shared__ float hsum[256];
  __shared__ int is_last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * NCH;
  const int task = blockIdx.y * WPB + wave, cb = task % CW, grp = task / CW;  // pixel group: output rows grp RPP ..
  const int cin = cb * 64 + lane;
  const int oy0 = grp * RPP, iy0 = 2 * oy0 - 1;
  // every load of the task is issued before the first multiply: one round trip per layer
  float wk[NCH][16];
#pragma unroll
  for (int c_ = 0; c_ < NCH; ++c_) {
    const float4* wp = reinterpret_cast<const float4*>(w + ((size_t)(n0 + c_) * CIN + cin) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = wp[q];
      wk[c_][4 * q] = v.x; wk[c_][4 * q + 1] = v.y; wk[c_][4 * q + 2] = v.z; wk[c_][4 * q + 3] = v.w;
    }
  }
  // the head's weights of this thread's logit: requested with everything else (their round trip would otherwise start after
  // the convolution, in front of the hand-off)
  float whr[HEAD ? NCH : 1][16];
  if constexpr (HEAD) {
    const int t = threadIdx.x;
    if (t < B * KOUT) {
#pragma unroll
      for (int c_ = 0; c_ < NCH; ++c_) {
        const float4* wh4 = reinterpret_cast<const float4*>(whead + ((size_t)(t % KOUT) * COUT + n0 + c_) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 v = wh4[q];
          whr[c_][4 * q] = v.x; whr[c_][4 * q + 1] = v.y; whr[c_][4 * q + 2] = v.z; whr[c_][4 * q + 3] = v.w;
        }
      }
    }
  }
  for (int b = 0; b < B; ++b) {
    float xin[NIR][HIN + 2];
#pragma unroll
    for (int r = 0; r < NIR; ++r) {
      const int iy = iy0 + r;
      const bool ok = iy >= 0 && iy < HIN;
      const float4* rp = reinterpret_cast<const float4*>(x + (((size_t)b * HIN + min(max(iy, 0), HIN - 1)) * Q * CIN + cin) * 4);
      xin[r][0] = 0.f;
      xin[r][HIN + 1] = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float4 v = rp[(size_t)q * CIN];
        xin[r][1 + 4 * q] = ok ? v.x : 0.f;
        xin[r][2 + 4 * q] = ok ? v.y : 0.f;
        xin[r][3 + 4 * q] = ok ? v.z : 0.f;
        xin[r][4 + 4 * q] = ok ? v.w : 0.f;
      }
    }
#pragma unroll
    for (int c_ = 0; c_ < NCH; ++c_) {
      float acc[16];
#pragma unroll
      for (int r = 0; r < RPP; ++r)
#pragma unroll
        for (int ox = 0; ox < HO; ++ox) {
          float s = 0.f;
#pragma unroll
          for (int ky = 0; ky < 4; ++ky)
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) s = fmaf(wk[c_][4 * ky + kx], xin[2 * r + ky][2 * ox + kx], s);  // column 2 ox - 1 + kx (+ 1: border)
          acc[r * HO + ox] = s;
        }
      const float tot = xpose_sum16(acc, lane);
      if (lane < 16) red[wave][c_][lane] = tot;
    }
    __syncthreads();
    // pixel group g of this workgroup = waves g CW .. g CW + CW - 1, summed in that order
    for (int i = threadIdx.x; i < NG * NCH * 16; i += 64 * WPB) {
      const int gl = i / (NCH * 16), c_ = (i >> 4) % NCH, p = i & 15;
      float s = red[gl * CW][c_][p];
#pragma unroll
      for (int k = 1; k < CW; ++k) s += red[gl * CW + k][c_][p];
      s = s > 0.f ? s : s * slope;
      const int g_ = blockIdx.y * NG + gl;
      const int oy = g_ * RPP + p / HO, ox = p % HO;
      constexpr int QO = HO / 4;
      y[((((size_t)b * HO + oy) * QO + ox / 4) * COUT + n0 + c_) * 4 + (ox & 3)] = s;
      if (HEAD) act[b][c_][p] = s;
    }
    __syncthreads();
  }
  if constexpr (HEAD) {
    const int t = threadIdx.x;
    const int nv = B * KOUT;   // <= 32 logits
    if (t < nv) {
      const int b = t / KOUT, k = t % KOUT;
      float s = 0.f;
#pragma unroll
      for (int c_ = 0; c_ < NCH; ++c_)
#pragma unroll
        for (int p = 0; p < 16; ++p) s = fmaf(whr[c_][p], act[b][c_][p], s);
      __hip_atomic_store(partials + (size_t)blockIdx.x * 32 + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (t < 32) {
      __hip_atomic_store(partials + (size_t)blockIdx.x * 32 + t, 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (unused columns: defined)
    }
    if (wave == 0) {  // (the stores above are this wave's)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) is_last = oi::last_arriver(ticket, blockIdx.x, gridDim.x);
    }
    __syncthreads();
    if (!is_last) return;
    // the last workgroup sums the table [gridDim.x][32] in a fixed order: 8 threads per logit take every 8th row (all
    // loads independent), then a fixed 8-term sum per logit
    {
      const int v = t & 31, part = t >> 5;  // 256 threads = 32 logits x 8 parts of NROWS / 8 consecutive rows
      constexpr int NROWS = 512 / NCH, PER = NROWS / 8;   // (the head exists for the 512-channel layer only: gridDim.x = NROWS)
      float vals[PER];
#pragma unroll
      for (int j = 0; j < PER; ++j)   // all loads in flight at once (a run-time trip count made this a chain of round trips)
        vals[j] = __hip_atomic_load(partials + (size_t)(part * PER + j) * 32 + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j) s += vals[j];
      hsum[t] = v < nv ? s : 0.f;
    }
    __syncthreads();
    if (t < nv) {
      float s = bhead != nullptr ? bhead[t % KOUT] : 0.f;
#pragma unroll
      for (int part = 0; part < 8; ++part) s += hsum[part * 32 + t];
      logits[t] = s;
    }
  }
}

// ---- the shipped 128 x 128 network's second block: 32 -> 64 channels, 64 x 64 -> 32 x 32 (round 6) ---------------------------
// (configs/train.yaml:78-102: img_size 128 = five blocks 3 | 1 -> 32 -> 64 -> 128 -> 256 -> 512; the last three are the 64 x 64
// network's conv 2..4 + head, the first rides on d_aug_conv1_kernel with C1 = 32.)  With 32 input channels the "input channel on
// the lane" form of d_conv_small_kernel has half a wave of work per task; this layer is 33.5 M MACs per image over 128 KB of
// weights -- arithmetic, not a weight stream: one workgroup per (output row, quarter of the output channels), the four input rows
// under the output row and the 16 channels' weights staged in LDS once, a thread = one output channel x two consecutive
// output pixels, 1024 FMAs per thread in a fixed (c_in, ky, kx) order.  (Halves of the channels x four pixels per thread: 18.4 us;
// this form: see DESIGN.)
//   x A[B][64][16][32][4] -> y A[B][32][8][64][4] = lrelu(conv4x4 s2 p1 (x, w)), w [64][32][4][4]
constexpr int DC32_ROW = 72;          // staged input row of one channel: x = -4 .. 67 (zero outside the image)
constexpr int DC32_WST = 512 + 4;     // weights of one output channel (+ 4: the four channels of a wave in distinct 16-byte slots)
constexpr int DC32_CO = 16;           // output channels per workgroup: 32 rows x 4 quarters = 128 workgroups per image
constexpr int DC32_LDS = (4 * 32 * DC32_ROW + DC32_CO * DC32_WST) * 4;   // 69,888 bytes
__global__ void __launch_bounds__(256) d_conv_c32_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y,
                                                         float slope) {
  extern __shared__ __attribute__((aligned(16))) float dc32_lds[];
  float* in_l = dc32_lds;                       // [ky 4][c_in 32][DC32_ROW]
  float* w_l = dc32_lds + 4 * 32 * DC32_ROW;    // [c_out 16][DC32_WST]
  const int tid = threadIdx.x, oy = blockIdx.x, quarter = blockIdx.y, b = blockIdx.z;
  // weights of this quarter's 16 output channels: 16 x 512 floats, float4 per thread and step
  for (int i = tid; i < DC32_CO * 128; i += 256) {
    const int co = i >> 7, q = i & 127;
    *reinterpret_cast<float4*>(w_l + co * DC32_WST + 4 * q) = *reinterpret_cast<const float4*>(w + ((size_t)(quarter * DC32_CO + co) * 512 + 4 * q));
  }
  // input rows 2 oy - 1 .. 2 oy + 2: [row][xq 16][c 32][4] in memory -> [row][c][4 + 4 xq ..] in LDS; halo columns zero
  {
    const int r = tid >> 6, c = (tid >> 1) & 31, side = tid & 1;   // the two halo quads of every (row, channel): 256 of them
    *reinterpret_cast<float4*>(in_l + (r * 32 + c) * DC32_ROW + (side ? 68 : 0)) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int i = tid; i < 4 * 16 * 32; i += 256) {
    const int r = i >> 9, xq = (i >> 5) & 15, c = i & 31;
    const int iy = 2 * oy - 1 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (iy >= 0 && iy < 64) v = *reinterpret_cast<const float4*>(x + ((((size_t)b * 64 + iy) * 16 + xq) * 32 + c) * 4);
    *reinterpret_cast<float4*>(in_l + (r * 32 + c) * DC32_ROW + 4 + 4 * xq) = v;
  }
  __syncthreads();
  // thread = output channel co x output pixels ox = 2 xh, 2 xh + 1: input x = 4 xh + 2 j - 1 + kx  ->  staged index 4 xh + 2 j + 3 + kx
  const int co = tid >> 4, xh = tid & 15;
  float acc[2] = {0.f, 0.f};
  const float* wp = w_l + co * DC32_WST;
  const float* ip = in_l + 4 * xh;
  for (int c = 0; c < 32; ++c) {
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      const float4 wv = *reinterpret_cast<const float4*>(wp + c * 16 + ky * 4);
      const float* row = ip + (ky * 32 + c) * DC32_ROW;
      const float4 a0 = *reinterpret_cast<const float4*>(row), a1 = *reinterpret_cast<const float4*>(row + 4);
      const float4 a2 = *reinterpret_cast<const float4*>(row + 8);
      const float v[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[j] = fmaf(wv.x, v[2 * j + 3], acc[j]);
        acc[j] = fmaf(wv.y, v[2 * j + 4], acc[j]);
        acc[j] = fmaf(wv.z, v[2 * j + 5], acc[j]);
        acc[j] = fmaf(wv.w, v[2 * j + 6], acc[j]);
      }
    }
  }
  float2 o;
  o.x = acc[0] > 0.f ? acc[0] : acc[0] * slope;
  o.y = acc[1] > 0.f ? acc[1] : acc[1] * slope;
  // y A[b][oy][ox / 4][channel][ox % 4]: ox = 2 xh + j
  *reinterpret_cast<float2*>(y + ((((size_t)b * 32 + oy) * 8 + (xh >> 1)) * 64 + quarter * DC32_CO + co) * 4 + 2 * (xh & 1)) = o;
}

}  // namespace

// Does every tile's canvas footprint fit d_aug_conv1_kernel<true>'s LDS tile?  Conservative: over the 21 grid steps of a tile
// the source coordinate moves by at most 21 Wc (|t0| / Wo + |t1| / Ho) canvas pixels (affine_src_s), the touched pixels are
// floor + 1, and the tile origin is rounded down to an even pixel.
static bool fold_fits(const float* theta, int B, int H, int W, int Hp, int Wp) {
  const float Ho = 2.0f * (H + DA_PAD), Wo = 2.0f * (W + DA_PAD), Hc = 2.0f * Hp, Wc = 2.0f * Wp;
  for (int b = 0; b < B; ++b) {
    const float* t = theta + b * 6;
    const float dx = (DA_G - 1) * Wc * (fabsf(t[0]) / Wo + fabsf(t[1]) / Ho), dy = (DA_G - 1) * Hc * (fabsf(t[3]) / Wo + fabsf(t[4]) / Ho);
    if (!(dx + 4.0f <= DA_CT && dy + 4.0f <= DA_CT)) return false;   // (also false for NaN)
  }
  return true;
}

// disc.hip: the canvas of the augmentation (reflect pad + x2 up-FIR) for a given stream
extern "C" int oi_ada_pad_up2(const float* x, const float* f, float* canvas, int B, int C, int H, int W, int mx0, int mx1, int my0,
                              int my1, oi_stream_t stream);

extern "C" {

}  // extern "C"

// w0 != NULL: the 128 x 128 / five-block network (C -> 32 -> 64 -> 128 -> 256 -> 512 -> out_dim), else the 64 x 64 / four-block one
static size_t small_workspace_floats(int B, int C, int R, int mx0, int mx1, int my0, int my1) {
  const size_t canvas = (size_t)B * C * (2 * (R + my0 + my1)) * (2 * (R + mx0 + mx1));
  return (canvas + 63) / 64 * 64 + (R == 128 ? (size_t)B * 32 * 64 * 64 : 0) + (size_t)B * (64 * 32 * 32 + 128 * 16 * 16 + 256 * 8 * 8) +
         (size_t)512 * DS_MAX_B * 8;
}

static int disc_fwd_small_impl(const float* x, const float* theta_host, const float* theta_dev, const float* f12, int mx0, int mx1, int my0,
                               int my1, const float* w0, const float* w1, const float* w2, const float* w3, const float* w4, const float* whead,
                               const float* bhead, float* workspace, unsigned* ticket, float* logits, int B, int C, int H, int W, int n_feat,
                               int out_dim, float slope, oi_stream_t stream) {
  OI_REQUIRE(x && f12 && w1 && w2 && w3 && w4 && whead && workspace && ticket && logits, "oi_disc_fwd_small: null pointer");
  OI_REQUIRE(theta_host == nullptr || theta_dev == nullptr, "oi_disc_fwd_small: theta_host and theta_dev are alternatives");
  const int R = w0 != nullptr ? 128 : 64;
  if (!(B >= 1 && B <= DS_MAX_B && C >= 1 && C <= DS_MAX_C && H == R && W == R && n_feat == 512 && out_dim >= 1 && out_dim <= 8))
    return oi::fail(OI_ERR_UNSUPPORTED, "oi_disc_fwd_small: only B <= %d, C <= %d, %d x %d, n_feat 512, out_dim <= 8 (got B=%d C=%d %dx%d n_feat=%d out_dim=%d)",
                    DS_MAX_B, DS_MAX_C, R, R, B, C, H, W, n_feat, out_dim);
  hipStream_t st = oi::as_stream(stream);
  const bool aug = theta_host != nullptr || theta_dev != nullptr;
  float* canvas = workspace;
  const int Hp = H + my0 + my1, Wp = W + mx0 + mx1;
  const size_t canvas_n = aug ? (size_t)B * C * (2 * Hp) * (2 * Wp) : 0;
  float* a0 = workspace + (canvas_n + 63) / 64 * 64;   // 128 x 128 only: block 1's output (32 channels, 64 x 64)
  float* a1 = a0 + (R == 128 ? (size_t)B * 32 * 64 * 64 : 0);   // 64 channels, 32 x 32; dead after the next block: conv 4's output lands here again
  float* a2 = a1 + (size_t)B * 64 * 32 * 32;
  float* a3 = a2 + (size_t)B * 128 * 16 * 16;
  float* partials = a3 + (size_t)B * 256 * 8 * 8;
  const float* wfirst = R == 128 ? w0 : w1;
  float* afirst = R == 128 ? a0 : a1;
  const int c_first = R == 128 ? 32 : 64;
  ThetaArg th = {};
  int rc = OI_OK;
  // the canvas built inside d_aug_conv1_kernel (one launch less) when the host can see that every tile's footprint fits
  const bool fold = aug && theta_host != nullptr && fold_fits(theta_host, B, H, W, Hp, Wp);
  if (aug) {
    if (theta_host != nullptr)
      for (int b = 0; b < B; ++b)
        for (int i = 0; i < 6; ++i) th.t[b][i] = theta_host[b * 6 + i];
    if (!fold) {
      rc = oi_ada_pad_up2(x, f12, canvas, B, C, H, W, mx0, mx1, my0, my1, stream);
      if (rc != OI_OK) return rc;
    }
  }
  if (fold)
    hipLaunchKernelGGL(d_aug_conv1_kernel<true>, dim3(W / DA_T, H / DA_T, B), dim3(256), 0, st, x, th, theta_dev, 1, f12, wfirst, afirst, C, H, W,
                       2 * Hp, 2 * Wp, c_first, slope, mx0, my0);
  else
    hipLaunchKernelGGL(d_aug_conv1_kernel<false>, dim3(W / DA_T, H / DA_T, B), dim3(256), 0, st, aug ? canvas : x, th, theta_dev,
                       aug ? 1 : 0, f12, wfirst, afirst, C, H, W, 2 * Hp, 2 * Wp, c_first, slope, mx0, my0);
  rc = oi::check_launch("oi_disc_fwd_small(aug + conv1)");
  if (rc != OI_OK) return rc;
  if (R == 128) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(d_conv_c32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DC32_LDS);
    hipLaunchKernelGGL(d_conv_c32_kernel, dim3(32, 64 / DC32_CO, B), dim3(256), DC32_LDS, st, a0, w1, a1, slope);
    rc = oi::check_launch("oi_disc_fwd_small(conv 32 -> 64)");
    if (rc != OI_OK) return rc;
  }
  hipLaunchKernelGGL((d_conv_small_kernel<64, 32, 8, 2, false>), dim3(128 / 2, 2), dim3(512), 0, st, a1, w2, a2, B, 128, slope, nullptr,
                     nullptr, 0, nullptr, nullptr, nullptr);
  rc = oi::check_launch("oi_disc_fwd_small(conv2)");
  if (rc != OI_OK) return rc;
  hipLaunchKernelGGL((d_conv_small_kernel<128, 16, 8, 2, false>), dim3(256 / 2, 1), dim3(512), 0, st, a2, w3, a3, B, 256, slope, nullptr,
                     nullptr, 0, nullptr, nullptr, nullptr);
  rc = oi::check_launch("oi_disc_fwd_small(conv3)");
  if (rc != OI_OK) return rc;
  static_assert(512 / 2 <= oi::LA_GROUP * (oi::LA_WORDS - 1), "conv4 + head: the arrival counters cover the grid");
  hipLaunchKernelGGL((d_conv_small_kernel<256, 8, 4, 2, true>), dim3(512 / 2, 1), dim3(256), 0, st, a3, w4, a1, B, 512, slope, whead, bhead,
                     out_dim, partials, ticket, logits);
  return oi::check_launch("oi_disc_fwd_small(conv4 + head)");
}

extern "C" {

size_t oi_disc_fwd_small_workspace_floats(int B, int C, int mx0, int mx1, int my0, int my1) {
  return small_workspace_floats(B, C, 64, mx0, mx1, my0, my1);
}
size_t oi_disc_fwd_small128_workspace_floats(int B, int C, int mx0, int mx1, int my0, int my1) {
  return small_workspace_floats(B, C, 128, mx0, mx1, my0, my1);
}

int oi_disc_fwd_small(const float* x, const float* theta_host, const float* theta_dev, const float* f12, int mx0, int mx1, int my0,
                      int my1, const float* w1, const float* w2, const float* w3, const float* w4, const float* whead,
                      const float* bhead, float* workspace, unsigned* ticket, float* logits, int B, int C, int H, int W, int n_feat,
                      int out_dim, float slope, oi_stream_t stream) {
  return disc_fwd_small_impl(x, theta_host, theta_dev, f12, mx0, mx1, my0, my1, nullptr, w1, w2, w3, w4, whead, bhead, workspace, ticket,
                             logits, B, C, H, W, n_feat, out_dim, slope, stream);
}

int oi_disc_fwd_small128(const float* x, const float* theta_host, const float* theta_dev, const float* f12, int mx0, int mx1, int my0,
                         int my1, const float* w0, const float* w1, const float* w2, const float* w3, const float* w4, const float* whead,
                         const float* bhead, float* workspace, unsigned* ticket, float* logits, int B, int C, int n_feat, int out_dim,
                         float slope, oi_stream_t stream) {
  OI_REQUIRE(w0 != nullptr, "oi_disc_fwd_small128: null pointer");
  return disc_fwd_small_impl(x, theta_host, theta_dev, f12, mx0, mx1, my0, my1, w0, w1, w2, w3, w4, whead, bhead, workspace, ticket, logits,
                             B, C, 128, 128, n_feat, out_dim, slope, stream);
}

}  // extern "C"

// ---- the same launches as ONE hipGraph whose per-call inputs are kernel-node PARAMETERS -----------------------------------
// A graph captured by the framework has its input pointer and the sampling matrices baked in, so every replay needs a staging
// launch in front (copy the image to the static buffer, write the matrices: 4.5 us of a 41 us replay).  Here the library owns
// the graph: captured once from oi_disc_fwd_small on a private stream, and before each launch the nodes that read per-call
// data get them through hipGraphExecKernelNodeSetParams -- the image POINTER (first node) and the matrices BY VALUE (ThetaArg
// of d_aug_conv1_kernel).  Nothing else changes between launches; weights, workspace, ticket and logits are fixed addresses.
// With the augmentation there are two captured variants: canvas built inside d_aug_conv1_kernel (4 nodes), or by
// ada_pad_up2_kernel in front (5 nodes) for matrices whose footprint does not fit the LDS tile (fold_fits, decided per launch).
namespace {
constexpr int N_ARGS_PAD = 10, N_ARGS_AUG = 17;   // ada_pad_up2_kernel / d_aug_conv1_kernel
struct GraphVariant {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  int n_nodes = 0;                                  // leading nodes that take per-call parameters
  hipGraphNode_t node[2] = {nullptr, nullptr};
  hipKernelNodeParams kp[2] = {};
  std::vector<void*> args[2];
};
}  // namespace

struct oi_disc_graph {
  GraphVariant v[2];          // aug: [0] folded, [1] canvas form; no aug: [0] only
  const float* x_arg = nullptr;
  ThetaArg th_arg = {};
  int aug = 0, B = 0, H = 0, W = 0, Hp = 0, Wp = 0;
  // everything oi_disc_fwd_small takes besides the image and the matrices (oi_disc_graph_launch_eager)
  const float *f12 = nullptr, *w1 = nullptr, *w2 = nullptr, *w3 = nullptr, *w4 = nullptr, *whead = nullptr, *bhead = nullptr;
  const float* w0 = nullptr;   // the 128 x 128 network's first block (oi_disc_graph_create128); NULL: the 64 x 64 network
  float* workspace = nullptr;
  unsigned* ticket = nullptr;
  float* logits = nullptr;
  int C = 0, mx0 = 0, mx1 = 0, my0 = 0, my1 = 0, n_feat = 0, out_dim = 0;
  float slope = 0.f;
};

static void graph_variant_free(GraphVariant& v) {
  if (v.exec) (void)hipGraphExecDestroy(v.exec);
  if (v.graph) (void)hipGraphDestroy(v.graph);
  v.exec = nullptr;
  v.graph = nullptr;
}

extern "C" {

int oi_disc_graph_create(oi_disc_graph** out, int aug, const float* f12, int mx0, int mx1, int my0, int my1, const float* w1,
                         const float* w2, const float* w3, const float* w4, const float* whead, const float* bhead,
                         float* workspace, unsigned* ticket, float* logits, int B, int C, int H, int W, int n_feat, int out_dim,
                         float slope) {
  OI_REQUIRE(out != nullptr && workspace != nullptr && ticket != nullptr && logits != nullptr && w1 && w2 && w3 && w4 && whead,
             "oi_disc_graph_create: null pointer");
  OI_REQUIRE(!aug || f12 != nullptr, "oi_disc_graph_create: augmentation without the filter taps");
  *out = nullptr;
  if (!(B >= 1 && B <= DS_MAX_B && C >= 1 && C <= DS_MAX_C && H == 64 && W == 64 && n_feat == 512 && out_dim >= 1 && out_dim <= 8))
    return oi::fail(OI_ERR_UNSUPPORTED, "oi_disc_graph_create: only B <= %d, C <= %d, 64 x 64, n_feat 512, out_dim <= 8", DS_MAX_B, DS_MAX_C);
  oi_disc_graph* g = new oi_disc_graph();
  g->aug = aug ? 1 : 0;
  g->B = B; g->H = H; g->W = W; g->Hp = H + my0 + my1; g->Wp = W + mx0 + mx1;
  g->f12 = f12; g->w1 = w1; g->w2 = w2; g->w3 = w3; g->w4 = w4; g->whead = whead; g->bhead = bhead;
  g->workspace = workspace; g->ticket = ticket; g->logits = logits;
  g->C = C; g->mx0 = mx0; g->mx1 = mx1; g->my0 = my0; g->my1 = my1; g->n_feat = n_feat; g->out_dim = out_dim; g->slope = slope;
  *out = g;   // (the hipGraph variants are captured by the first oi_disc_graph_launch: an object that is only ever launched
  return OI_OK;   //  eagerly makes no capture -- and can therefore be created while its caller is capturing)
}

int oi_disc_graph_create128(oi_disc_graph** out, int aug, const float* f12, int mx0, int mx1, int my0, int my1, const float* w0,
                            const float* w1, const float* w2, const float* w3, const float* w4, const float* whead, const float* bhead,
                            float* workspace, unsigned* ticket, float* logits, int B, int C, int n_feat, int out_dim, float slope) {
  OI_REQUIRE(out != nullptr && workspace != nullptr && ticket != nullptr && logits != nullptr && w0 && w1 && w2 && w3 && w4 && whead,
             "oi_disc_graph_create128: null pointer");
  OI_REQUIRE(!aug || f12 != nullptr, "oi_disc_graph_create128: augmentation without the filter taps");
  *out = nullptr;
  if (!(B >= 1 && B <= DS_MAX_B && C >= 1 && C <= DS_MAX_C && n_feat == 512 && out_dim >= 1 && out_dim <= 8))
    return oi::fail(OI_ERR_UNSUPPORTED, "oi_disc_graph_create128: only B <= %d, C <= %d, n_feat 512, out_dim <= 8", DS_MAX_B, DS_MAX_C);
  oi_disc_graph* g = new oi_disc_graph();
  g->aug = aug ? 1 : 0;
  g->B = B; g->H = 128; g->W = 128; g->Hp = 128 + my0 + my1; g->Wp = 128 + mx0 + mx1;
  g->f12 = f12; g->w0 = w0; g->w1 = w1; g->w2 = w2; g->w3 = w3; g->w4 = w4; g->whead = whead; g->bhead = bhead;
  g->workspace = workspace; g->ticket = ticket; g->logits = logits;
  g->C = C; g->mx0 = mx0; g->mx1 = mx1; g->my0 = my0; g->my1 = my1; g->n_feat = n_feat; g->out_dim = out_dim; g->slope = slope;
  *out = g;
  return OI_OK;
}

// captures the variants (private stream, relaxed mode) on first use
static int graph_capture(oi_disc_graph* g) {
  if (g->v[0].exec != nullptr) return OI_OK;
  if (g->w0 != nullptr)
    return oi::fail(OI_ERR_UNSUPPORTED, "oi_disc_graph_launch: the 128 x 128 plan is launched launch by launch (oi_disc_graph_launch_eager)");
  hipStream_t cs = nullptr;
  if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) return oi::fail(OI_ERR_LAUNCH, "oi_disc_graph_launch: stream");
  int rc = OI_OK;
  const char* what = nullptr;
  for (int vi = 0; vi < (g->aug ? 2 : 1) && rc == OI_OK && what == nullptr; ++vi) {
    GraphVariant& v = g->v[vi];
    // placeholders for the per-call arguments (nothing runs at capture time): `workspace` as the image pointer; a zero matrix
    // (fits: the folded form is captured) or an enormous one (does not fit: the canvas form)
    float th0[DS_MAX_B * 6] = {};
    if (vi == 1)
      for (int b = 0; b < g->B; ++b) th0[b * 6] = 1e9f;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) { what = hipGetErrorString(e); break; }
    rc = oi_disc_fwd_small(g->workspace, g->aug ? th0 : nullptr, nullptr, g->f12 != nullptr ? g->f12 : g->workspace, g->mx0, g->mx1, g->my0,
                           g->my1, g->w1, g->w2, g->w3, g->w4, g->whead, g->bhead, g->workspace, g->ticket, g->logits, g->B, g->C, g->H,
                           g->W, g->n_feat, g->out_dim, g->slope, reinterpret_cast<oi_stream_t>(cs));
    e = hipStreamEndCapture(cs, &v.graph);
    if (rc != OI_OK) break;
    if (e != hipSuccess || v.graph == nullptr) { what = hipGetErrorString(e); break; }
    if (hipGraphInstantiate(&v.exec, v.graph, nullptr, nullptr, 0) != hipSuccess) { what = "hipGraphInstantiate"; break; }
    size_t n_root = 1;
    if (hipGraphGetRootNodes(v.graph, &v.node[0], &n_root) != hipSuccess || n_root != 1) { what = "root node"; break; }
    v.n_nodes = (g->aug && vi == 1) ? 2 : 1;
    if (v.n_nodes == 2) {
      size_t n_dep = 1;
      if (hipGraphNodeGetDependentNodes(v.node[0], &v.node[1], &n_dep) != hipSuccess || n_dep != 1) { what = "second node"; break; }
    }
    for (int i = 0; i < v.n_nodes && what == nullptr; ++i) {
      if (hipGraphKernelNodeGetParams(v.node[i], &v.kp[i]) != hipSuccess || v.kp[i].kernelParams == nullptr) { what = "kernel node parameters"; break; }
      const int n_args = (v.n_nodes == 2 && i == 0) ? N_ARGS_PAD : N_ARGS_AUG;
      v.args[i].assign(v.kp[i].kernelParams, v.kp[i].kernelParams + n_args);
      v.kp[i].kernelParams = v.args[i].data();
    }
    if (what != nullptr) break;
    v.args[0][0] = &g->x_arg;                                   // the image pointer: first argument of the first kernel
    if (g->aug) v.args[v.n_nodes - 1][1] = &g->th_arg;          // d_aug_conv1_kernel(src, ThetaArg th, ...)
  }
  (void)hipStreamDestroy(cs);
  if (rc != OI_OK || what != nullptr) {
    graph_variant_free(g->v[0]);
    graph_variant_free(g->v[1]);
    return rc != OI_OK ? rc : oi::fail(OI_ERR_LAUNCH, "oi_disc_graph_launch: capture: %s", what);
  }
  return OI_OK;
}

int oi_disc_graph_launch(oi_disc_graph* g, const float* x, const float* theta_host, oi_stream_t stream) {
  OI_REQUIRE(g != nullptr && x != nullptr, "oi_disc_graph_launch: null pointer");
  OI_REQUIRE((theta_host != nullptr) == (g->aug != 0), "oi_disc_graph_launch: the graph was created %s augmentation", g->aug ? "with" : "without");
  {
    const int rc = graph_capture(g);
    if (rc != OI_OK) return rc;
  }
  g->x_arg = x;
  int vi = 0;
  if (g->aug) {
    for (int b = 0; b < g->B; ++b)
      for (int i = 0; i < 6; ++i) g->th_arg.t[b][i] = theta_host[b * 6 + i];
    vi = (fold_fits(theta_host, g->B, g->H, g->W, g->Hp, g->Wp)) ? 0 : 1;
  }
  GraphVariant& v = g->v[vi];
  for (int i = 0; i < v.n_nodes; ++i) {
    const hipError_t e = hipGraphExecKernelNodeSetParams(v.exec, v.node[i], &v.kp[i]);
    if (e != hipSuccess) return oi::fail(OI_ERR_LAUNCH, "oi_disc_graph_launch: hipGraphExecKernelNodeSetParams: %s", hipGetErrorString(e));
  }
  const hipError_t e = hipGraphLaunch(v.exec, oi::as_stream(stream));
  if (e != hipSuccess) return oi::fail(OI_ERR_LAUNCH, "oi_disc_graph_launch: hipGraphLaunch: %s", hipGetErrorString(e));
  return OI_OK;
}

// The same launches issued one by one on `stream` (no graph): a graph launch costs ~5 us of GPU time between two replays on
// this runtime, four eager launches from one call cost host time instead (which one wins depends on the host).
int oi_disc_graph_launch_eager(oi_disc_graph* g, const float* x, const float* theta_host, float* logits, oi_stream_t stream) {
  OI_REQUIRE(g != nullptr && x != nullptr, "oi_disc_graph_launch_eager: null pointer");
  OI_REQUIRE((theta_host != nullptr) == (g->aug != 0), "oi_disc_graph_launch_eager: the object was created %s augmentation", g->aug ? "with" : "without");
  return disc_fwd_small_impl(x, theta_host, nullptr, g->f12 != nullptr ? g->f12 : g->workspace, g->mx0, g->mx1, g->my0, g->my1, g->w0, g->w1,
                             g->w2, g->w3, g->w4, g->whead, g->bhead, g->workspace, g->ticket, logits != nullptr ? logits : g->logits, g->B,
                             g->C, g->H, g->W, g->n_feat, g->out_dim, g->slope, stream);
}

// ---- AugmentPipe's parameter draws for the shipped configuration (xint + scale), inside the library --------------------------
// One 64-bit seed per forward (the caller takes it from ITS random stream: one draw per call instead of four numpy calls and
// ~60 numpy scalar operations, which cost more host time than the four launches of the forward) is expanded by a counter-based
// generator (splitmix64) into the draws of src/third_party/ada/augment.py:213-230 -- per image, in this order: t_x, t_y ~ U[0, 1),
// the xint gate ~ U[0, 1), the scale's N(0, 1) (Box-Muller on two further uniforms), the scale gate ~ U[0, 1) -- with the
// reference's fp32 arithmetic: t = (u * 2 - 1) * xint_max if gate < xint * p else 0;  s = exp2(n * scale_std) if gate < scale * p
// else 1;  G_inv = T(-round(t_x W), -round(t_y H)) . S(1 / s, 1 / s) (round half to even, as torch.round).  The sampling matrix
// theta = [S(2 / Wp, 2 / Hp) T(-.5, -.5) S(2, 2) T((mx0 - mx1) / 2, (my0 - my1) / 2)] G_inv [S(.5, .5) T(.5, .5) S(Wo / 2, Ho / 2)]
// (augment.py:285-297; Wp, Hp = the padded x2 canvas, Wo, Ho = 2 (W + 6), 2 (H + 6)) is formed in double and rounded once.
namespace {
struct SplitMix64 {
  unsigned long long s;
  unsigned long long next() {
    unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  float uniform() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }   // 24 bits: [0, 1), exactly representable
  double uniform53() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

void mat3_mul(const double a[9], const double b[9], double out[9]) {
  double t[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) t[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
  for (int i = 0; i < 9; ++i) out[i] = t[i];
}

void ada_theta_draw(unsigned long long seed, int B, int H, int W, int mx0, int mx1, int my0, int my1, float p_xint, float xint_max,
                    float p_scale, float scale_std, float* theta, float* ts) {
  SplitMix64 rng{seed};
  const double Wp = 2.0 * (W + mx0 + mx1), Hp = 2.0 * (H + my0 + my1), Wo = 2.0 * (W + DA_PAD), Ho = 2.0 * (H + DA_PAD);
  const double S1[9] = {2 / Wp, 0, 0, 0, 2 / Hp, 0, 0, 0, 1}, T1[9] = {1, 0, -0.5, 0, 1, -0.5, 0, 0, 1}, S2[9] = {2, 0, 0, 0, 2, 0, 0, 0, 1};
  const double Tm[9] = {1, 0, (mx0 - mx1) / 2.0, 0, 1, (my0 - my1) / 2.0, 0, 0, 1};
  const double S3[9] = {0.5, 0, 0, 0, 0.5, 0, 0, 0, 1}, T2[9] = {1, 0, 0.5, 0, 1, 0.5, 0, 0, 1}, S4[9] = {Wo / 2, 0, 0, 0, Ho / 2, 0, 0, 0, 1};
  double L[9], R[9];
  mat3_mul(S1, T1, L); mat3_mul(L, S2, L); mat3_mul(L, Tm, L);
  mat3_mul(S3, T2, R); mat3_mul(R, S4, R);
  for (int b = 0; b < B; ++b) {
    const float u_tx = rng.uniform(), u_ty = rng.uniform(), g_t = rng.uniform();
    const double u1 = rng.uniform53(), u2 = rng.uniform53();
    const float g_s = rng.uniform();
    const float n = (float)(sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586476925 * u2));
    const bool t_on = g_t < p_xint, s_on = g_s < p_scale;
    const float tx = t_on ? (u_tx * 2.0f - 1.0f) * xint_max : 0.0f, ty = t_on ? (u_ty * 2.0f - 1.0f) * xint_max : 0.0f;
    const float sc = s_on ? exp2f(n * scale_std) : 1.0f;
    const float inv = 1.0f / sc;
    const double G[9] = {inv, 0, -(double)nearbyintf(tx * (float)W), 0, inv, -(double)nearbyintf(ty * (float)H), 0, 0, 1};
    double M[9];
    mat3_mul(L, G, M); mat3_mul(M, R, M);
    for (int i = 0; i < 6; ++i) theta[b * 6 + i] = (float)M[i];
    if (ts != nullptr) ts[b * 3] = tx, ts[b * 3 + 1] = ty, ts[b * 3 + 2] = sc;
  }
}
}  // namespace

int oi_ada_theta_xint_scale(unsigned long long seed, int B, int H, int W, int mx0, int mx1, int my0, int my1, float p_xint,
                            float xint_max, float p_scale, float scale_std, float* theta_host, float* ts_host) {
  OI_REQUIRE(theta_host != nullptr && B >= 1 && H >= 1 && W >= 1, "oi_ada_theta_xint_scale: bad argument");
  OI_REQUIRE(mx0 >= 0 && mx1 >= 0 && my0 >= 0 && my1 >= 0, "oi_ada_theta_xint_scale: negative margin");
  ada_theta_draw(seed, B, H, W, mx0, mx1, my0, my1, p_xint, xint_max, p_scale, scale_std, theta_host, ts_host);
  return OI_OK;
}

int oi_disc_graph_launch_ada(oi_disc_graph* g, const float* x, unsigned long long seed, float p_xint, float xint_max, float p_scale,
                             float scale_std, float* logits, int eager, oi_stream_t stream) {
  OI_REQUIRE(g != nullptr && x != nullptr, "oi_disc_graph_launch_ada: null pointer");
  OI_REQUIRE(g->aug != 0, "oi_disc_graph_launch_ada: the object was created without augmentation");
  float theta[DS_MAX_B * 6];
  ada_theta_draw(seed, g->B, g->H, g->W, g->mx0, g->mx1, g->my0, g->my1, p_xint, xint_max, p_scale, scale_std, theta, nullptr);
  if (eager) return oi_disc_graph_launch_eager(g, x, theta, logits, stream);
  OI_REQUIRE(logits == nullptr, "oi_disc_graph_launch_ada: a graph replay writes the buffer the object was created with");
  return oi_disc_graph_launch(g, x, theta, stream);
}

void oi_disc_graph_destroy(oi_disc_graph* g) {
  if (g == nullptr) return;
  graph_variant_free(g->v[0]);
  graph_variant_free(g->v[1]);
  delete g;
}

}  // extern "C"
