// One pixel of a captured view under F environments: the body of env_shade_kernel (envlight.hip),
// env_shade_bounce_kernel (envbounce.hip, 4.22), env_shade_glossy_kernel (envgloss.hip, 4.20) and env_shade_glossy_dirs_kernel
// (scene_gloss.hip, 4.25), and the arguments their C entries check alike.  They differ in one term per environment, chosen at
// compile time (EnvTerm); the diffuse chain, its rounding and the stores are written once.  Everything here has internal linkage.
#ifndef OI_ENV_SHADE_COMMON_H_
#define OI_ENV_SHADE_COMMON_H_

#include "trace_common.h"
#include "../../include/oi_envgloss.h"

namespace {

constexpr int NC = OI_ENV_COEFFS;
constexpr int ES_THREADS = 64;  // the shade kernels: one wave per workgroup, so a 128 x 128 view still covers every CU
constexpr float kPiF = 3.14159265358979323846f;

// beside transfer . coefficients: nothing, bounce[ch] . coefficients, the lobe's map looked up along the reflected view vector
// the kernel forms (GLOSSY) or along a world-frame direction the caller gives per pixel (GLOSSY_DIRS: a scene's plane)
enum class EnvTerm { NONE, BOUNCE, GLOSSY, GLOSSY_DIRS };
constexpr bool is_glossy(EnvTerm x) { return x == EnvTerm::GLOSSY || x == EnvTerm::GLOSSY_DIRS; }

// what travels in the glossy kernel's arguments beside oi_env_shade_params: the checked map of every environment
struct MapIndex {
  uint8_t v[OI_ENV_MAX_ENVS];
};
static_assert(OI_ENV_MAX_ENVS <= 256, "a map index fits a byte");

struct GlossArgs {
  const float* rays_o;
  const float* hit_points;
  const float* grad;
  const float* w2b;
  const float* spec_vis;
  const float* glossy;
  const float* rot;
  const float* k_s;
  float* specular;
  int Hp, Wp;
  const float* dirs;  // GLOSSY_DIRS: [N][3] world frame, in place of rays_o / hit_points / grad / w2b (not read otherwise)
};

__device__ __forceinline__ float lerp_(float a, float b, float f) { return __fmaf_rn(f, b - a, a); }

// kv G_s(R^T rw) per channel: the rotated direction's bilinear lookup in one prefiltered map of Hp x Wp texels
__device__ __forceinline__ void gloss_lookup(const float* __restrict__ R, const float* __restrict__ map, int Hp, int Wp,
                                             const float* rw, const float* kv, float* spec) {
  const long long O = (long long)Hp * Wp;
  const float dx = R[0] * rw[0] + R[3] * rw[1] + R[6] * rw[2];  // R_f^T r_w
  const float dy = R[1] * rw[0] + R[4] * rw[1] + R[7] * rw[2];
  const float dz = R[2] * rw[0] + R[5] * rw[1] + R[8] * rw[2];
  const float theta = acosf(fminf(fmaxf(dz, -1.0f), 1.0f));
  float phi = atan2f(dy, dx);
  if (phi < 0.f) phi += 2.0f * kPiF;
  const float u = theta / kPiF * (float)Hp - 0.5f, v = phi / (2.0f * kPiF) * (float)Wp - 0.5f;
  const float fi = floorf(u), fj = floorf(v);
  const float fu = u - fi, fv = v - fj;
  // (a NaN direction lands on row 0, column 0: min / max drop it, and the remainder of 0 is 0)
  const int i0 = (int)fminf(fmaxf(fi, 0.f), (float)(Hp - 1)), i1 = (int)fminf(fmaxf(fi + 1.0f, 0.f), (float)(Hp - 1));
  int j0 = (int)fminf(fmaxf(fj, -1.0f), (float)Wp) % Wp;
  if (j0 < 0) j0 += Wp;
  const int j1 = j0 + 1 == Wp ? 0 : j0 + 1;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* __restrict__ m = map + ch * O;
    const float top = lerp_(m[(long long)i0 * Wp + j0], m[(long long)i0 * Wp + j1], fv);
    const float bot = lerp_(m[(long long)i1 * Wp + j0], m[(long long)i1 * Wp + j1], fv);
    spec[ch] = __fmul_rn(kv[ch], lerp_(top, bot, fu));
  }
}

// Pixel blockIdx.x * ES_THREADS + threadIdx.x of p (oi_env_shade_params, or oi_env_shade_bounce_params for BOUNCE); g, mi:
// read for the glossy terms only.  Its transfer (and bounce) values are read once, then per environment and channel
//   d = the 9-term fmaf chain transfer . coefficients           BOUNCE: in = the same chain over bounce[ch], s = d + in
//   shading = s, image = max(s, 0) albedo                        GLOSSY, GLOSSY_DIRS: image + spec where spec != 0
// on the mask; 0 and bg off it.
template <EnvTerm X, class P>
__device__ __forceinline__ void env_shade_pixel(const P& p, const GlossArgs& g = GlossArgs{}, const MapIndex& mi = MapIndex{}) {
  const long long i = (long long)blockIdx.x * ES_THREADS + threadIdx.x;
  if (i >= p.N) return;
  const bool hit = p.status[i] == OI_TRACE_HIT;
  float t[NC], alb[3] = {0.f, 0.f, 0.f};
  [[maybe_unused]] float b[3][NC], rw[3] = {0.f, 0.f, 0.f}, kv[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NC; ++c) t[c] = p.transfer[c * p.N + i];
  if constexpr (X == EnvTerm::BOUNCE) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int c = 0; c < NC; ++c) b[ch][c] = p.bounce[((long long)ch * NC + c) * p.N + i];
  }
  if (hit && (is_glossy(X) || p.image)) {
    const long long k = p.hit_slot[i];
    if (p.image) alb[0] = p.rgb[k * 3 + 0], alb[1] = p.rgb[k * 3 + 1], alb[2] = p.rgb[k * 3 + 2];
    if constexpr (X == EnvTerm::GLOSSY) {
      float n[3], r[3];
      reflect_view(g.grad, g.hit_points, k, g.rays_o + i * 3, n, r);
      to_world(g.w2b, r[0], r[1], r[2], rw[0], rw[1], rw[2]);
    }
    if constexpr (X == EnvTerm::GLOSSY_DIRS) rw[0] = g.dirs[i * 3 + 0], rw[1] = g.dirs[i * 3 + 1], rw[2] = g.dirs[i * 3 + 2];
    if constexpr (is_glossy(X)) {
      const float vis = g.spec_vis ? g.spec_vis[i] : 1.0f;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) kv[ch] = __fmul_rn(g.k_s[ch], vis);
    }
  }
  const float b3[3] = {p.bg ? p.bg[0] : 0.f, p.bg ? p.bg[1] : 0.f, p.bg ? p.bg[2] : 0.f};
  for (int f = 0; f < p.F; ++f) {
    const float* __restrict__ env = p.envs + (long long)f * OI_ENV_FLOATS;  // the same for every lane
    [[maybe_unused]] float spec[3] = {0.f, 0.f, 0.f};
    if constexpr (is_glossy(X)) {
      if (hit) gloss_lookup(g.rot + (long long)f * 9, g.glossy + (long long)mi.v[f] * 3 * g.Hp * g.Wp, g.Hp, g.Wp, rw, kv, spec);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) s = __fmaf_rn(t[c], env[c * 3 + ch], s);
      [[maybe_unused]] float in = 0.f;
      if constexpr (X == EnvTerm::BOUNCE) {
#pragma unroll
        for (int c = 0; c < NC; ++c) in = __fmaf_rn(b[ch][c], env[c * 3 + ch], in);
        s = __fadd_rn(s, in);
      }
      const long long o = ((long long)f * 3 + ch) * p.N + i;
      if (p.shading) p.shading[o] = hit ? s : 0.f;
      if constexpr (X == EnvTerm::BOUNCE) {
        if (p.indirect) p.indirect[o] = hit ? in : 0.f;
      }
      if constexpr (is_glossy(X)) {
        if (g.specular) g.specular[o] = spec[ch];
      }
      if (p.image) {
        // (the product is rounded before the glossy sum; kept as these two expressions, which compile to v_mul + v_add)
        const float base = __fmul_rn(fmaxf(s, 0.f), alb[ch]);
        if constexpr (is_glossy(X)) p.image[o] = hit ? (spec[ch] != 0.f ? __fadd_rn(base, spec[ch]) : base) : b3[ch];
        else p.image[o] = hit ? base : b3[ch];
      }
    }
  }
}

// The arguments oi_env_shade, oi_env_shade_bounce and oi_env_shade_glossy check alike (P: oi_env_shade_params or a struct with
// the same fields).  has_output: whether any of the entry's outputs is given; outputs: how the message names them.
template <class P>
inline int check_env_shade(const char* what, const P* p, bool has_output, const char* outputs) {
  OI_REQUIRE(p != nullptr, "%s: null params", what);
  OI_TRY(check_pixels(what, p->N, p->n_hit));
  OI_REQUIRE(p->F >= 1 && p->F <= OI_ENV_MAX_ENVS, "%s: F=%d (1 .. %d environments)", what, p->F, OI_ENV_MAX_ENVS);
  OI_REQUIRE(p->status && p->hit_slot && p->transfer && p->envs, "%s: null input pointer", what);
  OI_REQUIRE(has_output, "%s: no output (%s)", what, outputs);
  OI_REQUIRE(p->rgb || p->n_hit == 0 || !p->image, "%s: null rgb with n_hit=%lld and an image", what, p->n_hit);
  return OI_OK;
}

inline bool shininess_ok(float s) { return s >= (float)OI_ENVGLOSS_MIN_SHININESS && s <= (float)OI_ENVGLOSS_MAX_SHININESS; }

// What oi_env_shade_glossy and oi_env_shade_glossy_dirs check alike: the sizes of the prefiltered maps, and every
// environment's map index (HOST memory), which travels in the kernel's arguments.
inline int check_gloss_maps(const char* what, int M, int Hp, int Wp) {
  OI_REQUIRE(M >= 1 && M <= OI_ENV_MAX_ENVS && Hp >= 1 && Wp >= 1 && (long long)M * 3 * Hp * Wp < (1ll << 31),
             "%s: M=%d, Hp=%d, Wp=%d (1 <= M <= %d, sizes >= 1, M * 3 * Hp * Wp < 2^31)", what, M, Hp, Wp, OI_ENV_MAX_ENVS);
  return OI_OK;
}
inline int pack_map_index(const char* what, int F, int M, const int* map_index, MapIndex& mi) {
  for (int f = 0; f < F; ++f) {
    OI_REQUIRE(map_index[f] >= 0 && map_index[f] < M, "%s: map_index[%d]=%d (0 <= map_index < M=%d)", what, f, map_index[f], M);
    mi.v[f] = (uint8_t)map_index[f];
  }
  return OI_OK;
}

}  // namespace

#endif  // OI_ENV_SHADE_COMMON_H_
