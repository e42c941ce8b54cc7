// Relighting of a captured render for gfx950 (include/oi_relight.h): N rays x T captured samples shaded and composited
// under L directional lights in one launch.
//
// One 64-lane wavefront owns one ray, as in composite_fwd_kernel (render.hip).  The wave first reads its ray's capture
// (32 bytes per sample: weight, raw gradient, albedo, mid_z) and parks what no light depends on -- the unit normal, the
// unit view vector, the weight and the albedo, 10 floats -- in its own slice of LDS.  Each lane stages exactly the samples
// it later reads back (sample c0 + lane of every 64-sample chunk), so there is no exchange between lanes or waves and no
// barrier.  Then the wave walks its lights in groups of G: per group the light terms live in registers, every staged
// sample is shaded under each light of the group, per-lane sums run over the chunks, and one wavefront sum per quantity
// ends the group.  The capture is read once whatever L is; the per-light work is the Phong arithmetic alone.
//
// Rays whose samples do not fit the LDS budget (T > 1600) take the same code with the staging replaced by the global
// loads of each group (identical values, identical order).
#include "shade_common.h"
#include "../../include/oi_relight.h"

namespace {

using oi::wave_sum;

constexpr int LDS_BUDGET = 65536;  // bytes of dynamic LDS a workgroup gets without an opt-in
constexpr int STAGE_FLOATS = 10;   // per staged sample: n (3), v (3), w, albedo (3)
constexpr int G = 4;                // lights per group: 121 VGPRs image-only, 159 with the three extra maps, no scratch
                                   // (8 lights per group: 219, two waves per SIMD)

struct Sample {
  float nx, ny, nz, vx, vy, vz, w, c_r, c_g, c_b;
};

// The light-independent terms of sample k of ray (o, d).
__device__ __forceinline__ Sample load_sample(const oi_relight_params& p, long long k, float ox, float oy, float oz, float dx,
                                              float dy, float dz) {
  Sample s;
  const float mz = p.mid_z[k];
  const float gx = p.grad[k * 3 + 0], gy = p.grad[k * 3 + 1], gz = p.grad[k * 3 + 2];
  s.w = p.weights[k];
  s.c_r = p.rgb[k * 3 + 0];
  s.c_g = p.rgb[k * 3 + 1];
  s.c_b = p.rgb[k * 3 + 2];
  const float px = ox + dx * mz, py = oy + dy * mz, pz = oz + dz * mz;
  unit_normal(gx, gy, gz, s.nx, s.ny, s.nz);
  unit_view(ox, oy, oz, px, py, pz, s.vx, s.vy, s.vz);
  return s;
}

// MAPS: shading / diffuse / specular accumulated too; STAGED: the capture parked in LDS (`tpad` floats
// per field and ray, `rpb` rays per workgroup).
template <bool MAPS, bool STAGED>
__global__ void __launch_bounds__(256) relight_kernel(const oi_relight_params p, int rpb, int tpad) {
  extern __shared__ float stage[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long r = (long long)blockIdx.x * rpb + wave;
  if (r >= p.N) return;  // the whole wave: nothing in this kernel synchronises the workgroup
  const int T = p.T;
  const long long hw = p.N / p.B;
  const int e = (int)(r / hw);
  const long long px_ = r - (long long)e * hw;

  const float ox = p.rays_o[r * 3 + 0], oy = p.rays_o[r * 3 + 1], oz = p.rays_o[r * 3 + 2];
  const float dx = p.rays_d[r * 3 + 0], dy = p.rays_d[r * 3 + 1], dz = p.rays_d[r * 3 + 2];
  const float* Wb = p.w2b + (size_t)e * 16;
  const float b0 = p.bg ? p.bg[e * 3 + 0] : 0.f, b1 = p.bg ? p.bg[e * 3 + 1] : 0.f, b2 = p.bg ? p.bg[e * 3 + 2] : 0.f;
  float* st = stage + (size_t)wave * STAGE_FLOATS * tpad;

  if constexpr (STAGED) {
    for (int c0 = 0; c0 < T; c0 += 64) {
      const int i = c0 + lane;
      if (i < T) {
        const Sample s = load_sample(p, r * T + i, ox, oy, oz, dx, dy, dz);
        st[0 * tpad + i] = s.nx;
        st[1 * tpad + i] = s.ny;
        st[2 * tpad + i] = s.nz;
        st[3 * tpad + i] = s.vx;
        st[4 * tpad + i] = s.vy;
        st[5 * tpad + i] = s.vz;
        st[6 * tpad + i] = s.w;
        st[7 * tpad + i] = s.c_r;
        st[8 * tpad + i] = s.c_g;
        st[9 * tpad + i] = s.c_b;
      }
    }
  }

  float wsum = 0.f;  // sum w (light independent): formed during the first group, in the same per-lane order
  for (int g0 = 0; g0 < p.L; g0 += G) {
    const int gn = min(G, p.L - g0);
    // light terms of the group, the direction in this element's box frame
    float lx[G], ly[G], lz[G], ca[G][3], cd[G][3], cs[G][3], sh[G];
#pragma unroll
    for (int j = 0; j < G; ++j) {
      const float* lt = p.lights + (size_t)(g0 + (j < gn ? j : 0)) * OI_RELIGHT_LIGHT_FLOATS;
      light_dir(lt, Wb, lx[j], ly[j], lz[j]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ca[j][c] = lt[4 + c];
        cd[j][c] = lt[8 + c];
        cs[j][c] = lt[12 + c];
      }
      sh[j] = lt[15];
    }
    float a_i[G][3], a_sh[G][3], a_df[G][3], a_sp[G][3];
#pragma unroll
    for (int j = 0; j < G; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) a_i[j][c] = a_sh[j][c] = a_df[j][c] = a_sp[j][c] = 0.f;
    float a_w = 0.f;

    for (int c0 = 0; c0 < T; c0 += 64) {
      const int i = c0 + lane;
      if (i >= T) continue;
      Sample s;
      if constexpr (STAGED) {
        s.nx = st[0 * tpad + i];
        s.ny = st[1 * tpad + i];
        s.nz = st[2 * tpad + i];
        s.vx = st[3 * tpad + i];
        s.vy = st[4 * tpad + i];
        s.vz = st[5 * tpad + i];
        s.w = st[6 * tpad + i];
        s.c_r = st[7 * tpad + i];
        s.c_g = st[8 * tpad + i];
        s.c_b = st[9 * tpad + i];
      } else {
        s = load_sample(p, r * T + i, ox, oy, oz, dx, dy, dz);
      }
      const float w = s.w;
      const float alb[3] = {s.c_r, s.c_g, s.c_b};
      if (g0 == 0) a_w += w;
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if (j >= gn) break;
        const PhongGeometry ph = phong_geometry(s.nx, s.ny, s.nz, lx[j], ly[j], lz[j], s.vx, s.vy, s.vz);
        const float rl = fmaxf(ph.ndl, 0.f);
        const float pw = powf(ph.al, sh[j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float diff = cd[j][c] * rl;
          const float spec = cs[j][c] * pw;
          const float shade = ca[j][c] + diff;
          a_i[j][c] += w * (shade * alb[c] + spec);
          if constexpr (MAPS) {
            a_sh[j][c] += w * shade;
            a_df[j][c] += w * diff;
            a_sp[j][c] += w * spec;
          }
        }
      }
    }
    if (g0 == 0) wsum = wave_sum(a_w);
    const float t = 1.0f - wsum;  // generator.py:159
    const float bgc[3] = {b0, b1, b2};
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (j >= gn) break;
      const long long base = ((long long)(g0 + j) * p.B + e) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float im = wave_sum(a_i[j][c]);
        float sh_ = 0.f, df = 0.f, sp = 0.f;
        if constexpr (MAPS) {
          sh_ = wave_sum(a_sh[j][c]);
          df = wave_sum(a_df[j][c]);
          sp = wave_sum(a_sp[j][c]);
        }
        if (lane == 0) {
          const long long o = (base + c) * hw + px_;
          if (p.image_no_bg) p.image_no_bg[o] = im;
          if (p.image) p.image[o] = im + bgc[c] * t;
          if constexpr (MAPS) {
            if (p.shading) p.shading[o] = sh_;
            if (p.diffuse) p.diffuse[o] = df;
            if (p.specular) p.specular[o] = sp;
          }
        }
      }
    }
  }
}

template <bool MAPS>
int launch(const oi_relight_params* p, hipStream_t st) {
  const int tpad = (int)oi::cdiv(p->T, 64) * 64;
  const long long ray_bytes = (long long)STAGE_FLOATS * tpad * (long long)sizeof(float);
  int rpb = 4;
  while (rpb > 1 && rpb * ray_bytes > LDS_BUDGET) rpb >>= 1;
  if (rpb * ray_bytes <= LDS_BUDGET) {
    hipLaunchKernelGGL((relight_kernel<MAPS, true>), dim3(oi::cdiv(p->N, rpb)), dim3(64 * rpb), (size_t)(rpb * ray_bytes), st,
                       *p, rpb, tpad);
  } else {
    hipLaunchKernelGGL((relight_kernel<MAPS, false>), dim3(oi::cdiv(p->N, 4)), dim3(256), 0, st, *p, 4, 0);
  }
  return oi::check_launch("oi_relight_fwd");
}

}  // namespace

extern "C" int oi_relight_fwd(const oi_relight_params* p, oi_stream_t stream) {
  OI_REQUIRE(p != nullptr, "oi_relight_fwd: null params");
  OI_REQUIRE(p->weights && p->grad && p->rgb && p->mid_z && p->rays_o && p->rays_d && p->w2b && p->lights,
             "oi_relight_fwd: null input pointer");
  OI_REQUIRE(p->N > 0 && p->T > 0 && p->B > 0 && p->N % p->B == 0, "oi_relight_fwd: N=%lld T=%d B=%d (N %% B must be 0)", p->N,
             p->T, p->B);
  OI_REQUIRE(p->L >= 1 && p->L <= OI_RELIGHT_MAX_LIGHTS, "oi_relight_fwd: L=%d (1 .. %d lights per launch)", p->L,
             OI_RELIGHT_MAX_LIGHTS);
  OI_REQUIRE(p->N < (1LL << 31), "oi_relight_fwd: N=%lld rays exceed one launch's grid", p->N);
  if (!p->image && !p->image_no_bg && !p->shading && !p->diffuse && !p->specular) return OI_OK;  // nothing asked for
  const hipStream_t st = oi::as_stream(stream);
  if (p->shading || p->diffuse || p->specular) return launch<true>(p, st);
  return launch<false>(p, st);
}
