// Glossy environment lighting on the sphere-traced surface (include/oi_envgloss.h), gfx950.
//   env_prefilter         equirectangular maps -> the Phong-lobe convolution G_s on an equirectangular grid: a dense sphere-to-
//                         sphere sum, per-chunk partials, then one thread per output value
//   occlusion_lobe_begin  S rays per visible point distributed as cos^s about the reflected view vector, written and compacted
//                         by trace_common.h's write_ray and enter_rays as occlusion.hip's begin kernels; the march and the
//                         resolve are occlusion.hip's
//   env_shade_glossy      envlight.hip's shading plus k_s V_spec G_s(R_f^T r_world): rotated bilinear lookups, F per thread
//                         (env_shade_common.h's pixel with the GLOSSY term)
// No float atomics, no scratch; every sum has one fixed order.  The only atomics are the compaction's integer counters.
#include "env_shade_common.h"

namespace {

constexpr int PF_THREADS = 256;            // oi_env_prefilter: output texels per workgroup, one per thread
constexpr int PF_CHUNK = OI_ENVGLOSS_CHUNK;  // input pixels per workgroup
constexpr int PF_BATCH = PF_THREADS;       // records in LDS at a time: each thread forms one
constexpr int PF_INNER = 32;               // terms a thread sums in one chain
constexpr int PF_FINAL = 32;               // stage 2: chains of 32 partials, nested four times (32^4 = 2^20 chunks)
constexpr long long PF_MAX_WORKGROUPS = 1ll << 23;  // the header's limit on E * chunks * tiles
static_assert(PF_CHUNK % PF_BATCH == 0 && PF_BATCH % PF_INNER == 0, "whole batches, whole chains");
static_assert(PF_INNER + PF_BATCH / PF_INNER + PF_CHUNK / PF_BATCH + 4 * PF_FINAL == 176, "the header states the additions");
static_assert((long long)PF_FINAL * PF_FINAL * PF_FINAL * PF_FINAL * PF_CHUNK >= (1ll << 31), "stage 2 covers E * He * We < 2^31");

// the unit direction of pixel (r, c) of an H x W equirectangular map and sin(theta): envlight.hip's expressions
__device__ __forceinline__ void texel_dir(long long r, long long c, int H, int W, float& x, float& y, float& z, float& st) {
  float ct, sp, cp;
  sincospif((float)(((double)r + 0.5) / (double)H), &st, &ct);        // theta = pi (r + 1/2) / H
  sincospif((float)((2.0 * (double)c + 1.0) / (double)W), &sp, &cp);  // phi = 2 pi (c + 1/2) / W
  x = st * cp, y = st * sp, z = ct;
}

// stage 1: partial[e][k][ch][o] = the sum over input pixels [k * PF_CHUNK, (k + 1) * PF_CHUNK) of (w / pi) L K(d_o . d_p).
// blockIdx.x = (e * nb + k) * nt + tile.  The LDS reads of the inner loop have one address for the whole wave: a broadcast,
// no bank conflict.
__global__ void __launch_bounds__(PF_THREADS) env_prefilter_partial_kernel(const float* __restrict__ radiance, int He, int We,
                                                                           float wscale, float shininess, int Hp, int Wp,
                                                                           long long nb, long long nt,
                                                                           float* __restrict__ partial) {
  __shared__ float4 rec_d[PF_BATCH];   // (d.x, d.y, d.z, -)
  __shared__ float4 rec_l[PF_BATCH];   // (w / pi) (L.r, L.g, L.b), -
  const long long P = (long long)He * We, O = (long long)Hp * Wp;
  const long long tile = blockIdx.x % nt, ek = blockIdx.x / nt;
  const long long k = ek % nb, e = ek / nb;
  const float* __restrict__ img = radiance + e * 3 * P;
  const long long o = tile * PF_THREADS + threadIdx.x;
  float ox = 0.f, oy = 0.f, oz = 0.f, unused;
  if (o < O) texel_dir(o / Wp, o % Wp, Hp, Wp, ox, oy, oz, unused);
  float acc[3] = {0.f, 0.f, 0.f};
  for (int b = 0; b < PF_CHUNK / PF_BATCH; ++b) {
    const long long p = k * PF_CHUNK + (long long)b * PF_BATCH + threadIdx.x;  // consecutive threads, consecutive pixels
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f), l = make_float4(0.f, 0.f, 0.f, 0.f);  // past the map: K(0) = 0, an exact + 0
    if (p < P) {
      float st;
      texel_dir(p / We, p % We, He, We, d.x, d.y, d.z, st);
      const float w = st * wscale;  // 2 sin(theta) sin(pi / (2 He)) 2 pi / We / pi
      l.x = w * img[p], l.y = w * img[P + p], l.z = w * img[2 * P + p];
    }
    __syncthreads();  // the previous batch's reads
    rec_d[threadIdx.x] = d;
    rec_l[threadIdx.x] = l;
    __syncthreads();
    float mid[3] = {0.f, 0.f, 0.f};
    for (int g = 0; g < PF_BATCH; g += PF_INNER) {
      float in[3] = {0.f, 0.f, 0.f};
#pragma unroll 8
      for (int i = 0; i < PF_INNER; ++i) {
        const float4 dd = rec_d[g + i], ll = rec_l[g + i];
        const float x = __fmaf_rn(oz, dd.z, __fmaf_rn(oy, dd.y, __fmul_rn(ox, dd.x)));
        // v_log_f32 / v_exp_f32: log2 and exp2 at the hardware's rate; a product below -126 gives 0
        const float kx = x > 0.f ? __builtin_amdgcn_exp2f(__fmul_rn(shininess, __builtin_amdgcn_logf(x))) : 0.f;
        in[0] = __fmaf_rn(ll.x, kx, in[0]);
        in[1] = __fmaf_rn(ll.y, kx, in[1]);
        in[2] = __fmaf_rn(ll.z, kx, in[2]);
      }
      mid[0] += in[0], mid[1] += in[1], mid[2] += in[2];
    }
    acc[0] += mid[0], acc[1] += mid[1], acc[2] += mid[2];
  }
  if (o < O) {
    float* __restrict__ out = partial + ek * 3 * O + o;
    out[0] = acc[0], out[O] = acc[1], out[2 * O] = acc[2];
  }
}

// stage 2: glossy[e][ch][o] = the sum of the nb partials.  One thread per output value; partial k, k + 1, ... in chains of
// PF_FINAL nested four times, so the order is a function of nb alone.  Coalesced across o.
__global__ void __launch_bounds__(PF_THREADS) env_prefilter_final_kernel(const float* __restrict__ partial, long long nb,
                                                                         long long O3, long long total,
                                                                         float* __restrict__ glossy) {
  const long long i = (long long)blockIdx.x * PF_THREADS + threadIdx.x;  // e * 3 * O + ch * O + o
  if (i >= total) return;
  const long long e = i / O3, v = i - e * O3;
  const float* __restrict__ src = partial + e * nb * O3 + v;
  constexpr long long F1 = PF_FINAL, F2 = F1 * PF_FINAL, F3 = F2 * PF_FINAL;
  float s3 = 0.f;
  for (long long k3 = 0; k3 < nb; k3 += F3) {
    float s2 = 0.f;
    for (long long k2 = k3; k2 < nb && k2 < k3 + F3; k2 += F2) {
      float s1 = 0.f;
      for (long long k1 = k2; k1 < nb && k1 < k2 + F2; k1 += F1) {
        float s0 = 0.f;
        for (long long k0 = k1; k0 < nb && k0 < k1 + F1; ++k0) s0 += src[k0 * O3];
        s1 += s0;
      }
      s2 += s1;
    }
    s3 += s2;
  }
  glossy[i] = s3;
}

// occlusion.hip's begin kernel with the lobe about r in place of the hemisphere about n
__global__ void __launch_bounds__(TR_THREADS) occlusion_lobe_begin_kernel(const oi_trace_state s, const float* __restrict__ rays_o,
                                                                          const float* __restrict__ hit_points,
                                                                          const float* __restrict__ grad,
                                                                          const int* __restrict__ hit_index, long long n_hit, int S,
                                                                          float inv_s1, float bias, unsigned seed) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool traced = false;
  float ox = 0.f, oy = 0.f, oz = 0.f;
  if (q < s.N) {
    const long long j = q / n_hit, i = q - j * n_hit;
    const long long pix = hit_index[i];
    float n[3], a[3];
    reflect_view(grad, hit_points, i, rays_o + pix * 3, n, a);
    float dx, dy, dz;
    traced = lobe_direction(n, a, (unsigned)pix, seed, (unsigned)j, S, inv_s1, dx, dy, dz);
    offset_origin(hit_points + i * 3, bias, n[0], n[1], n[2], ox, oy, oz);
    const float o[3] = {ox, oy, oz}, d[3] = {dx, dy, dz};
    write_ray(s, q, o, d, 0.f, unit_sphere_exit(ox, oy, oz, dx, dy, dz), traced ? OI_TRACE_MARCH : OI_TRACE_BACKFACING);
  }
  enter_rays(s, q, traced, ox, oy, oz, lds);
}

__global__ void __launch_bounds__(ES_THREADS) env_shade_glossy_kernel(const oi_env_shade_params p, const GlossArgs g,
                                                                      const MapIndex mi) {
  env_shade_pixel<EnvTerm::GLOSSY>(p, g, mi);
}

long long prefilter_chunks(int He, int We) { return ((long long)He * We + PF_CHUNK - 1) / PF_CHUNK; }
long long prefilter_tiles(int Hp, int Wp) { return ((long long)Hp * Wp + PF_THREADS - 1) / PF_THREADS; }

bool prefilter_args_ok(int E, int He, int We, int Hp, int Wp) {
  if (!(E >= 1 && E <= OI_ENV_MAX_ENVS && He >= 1 && We >= 1 && Hp >= 1 && Wp >= 1)) return false;
  if ((long long)E * He * We >= (1ll << 31) || (long long)E * 3 * Hp * Wp >= (1ll << 31)) return false;
  // the workgroups of stage 1 (each factor is below 2^8, 2^20 and 2^23: the product fits 64 bits): no more than the largest
  // grid any other entry of the library launches, n_blocks(N) for N < 2^31
  return (long long)E * prefilter_chunks(He, We) * prefilter_tiles(Hp, Wp) <= PF_MAX_WORKGROUPS;
}

}  // namespace

extern "C" {

size_t oi_env_prefilter_partial_floats(int E, int He, int We, int Hp, int Wp) {
  return prefilter_args_ok(E, He, We, Hp, Wp) ? (size_t)E * (size_t)prefilter_chunks(He, We) * 3 * (size_t)Hp * (size_t)Wp : 0;
}

int oi_env_prefilter(const float* radiance, int E, int He, int We, float shininess, int Hp, int Wp, float* partial,
                     float* glossy, oi_stream_t stream) {
  OI_REQUIRE(shininess_ok(shininess), "oi_env_prefilter: shininess %g (%d .. %d, finite)", (double)shininess,
             OI_ENVGLOSS_MIN_SHININESS, OI_ENVGLOSS_MAX_SHININESS);
  OI_REQUIRE(prefilter_args_ok(E, He, We, Hp, Wp),
             "oi_env_prefilter: E=%d, He=%d, We=%d, Hp=%d, Wp=%d (1 <= E <= %d, sizes >= 1, E * He * We and E * 3 * Hp * Wp below 2^31, "
             "the workgroups E * ceil(He * We / %d) * ceil(Hp * Wp / %d) at most 2^23)",
             E, He, We, Hp, Wp, OI_ENV_MAX_ENVS, PF_CHUNK, PF_THREADS);
  OI_REQUIRE(radiance && partial && glossy, "oi_env_prefilter: null pointer");
  const long long nb = prefilter_chunks(He, We), nt = prefilter_tiles(Hp, Wp);
  const long long O3 = 3ll * Hp * Wp, total = (long long)E * O3;
  const double kPi = 3.14159265358979323846;
  const float wscale = (float)(2.0 * sin(kPi / (2.0 * He)) * (2.0 / We));  // oi_env_project's weight over pi
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(env_prefilter_partial_kernel, dim3((unsigned)(E * nb * nt)), dim3(PF_THREADS), 0, st, radiance, He, We, wscale,
                     shininess, Hp, Wp, nb, nt, partial);
  hipLaunchKernelGGL(env_prefilter_final_kernel, dim3((unsigned)((total + PF_THREADS - 1) / PF_THREADS)), dim3(PF_THREADS), 0, st,
                     (const float*)partial, nb, O3, total, glossy);
  return oi::check_launch("oi_env_prefilter");
}

int oi_occlusion_lobe_begin(const oi_trace_state* s, const float* rays_o, const float* hit_points, const float* grad,
                            const int* hit_index, long long n_hit, int S, float shininess, float bias, unsigned seed,
                            oi_stream_t stream) {
  const char* what = "oi_occlusion_lobe_begin";
  OI_TRY(check_state(s, what));
  OI_TRY(check_samples(what, S));
  OI_REQUIRE(n_hit >= 1 && n_hit < (1ll << 31) && n_hit * S == s->N, "%s: n_hit=%lld, S=%d, N=%lld (N must be S * n_hit, below 2^31)",
             what, n_hit, S, s->N);
  OI_REQUIRE(shininess_ok(shininess), "%s: shininess %g (%d .. %d, finite)", what, (double)shininess, OI_ENVGLOSS_MIN_SHININESS,
             OI_ENVGLOSS_MAX_SHININESS);
  OI_TRY(check_bias(what, bias));
  OI_REQUIRE(rays_o && hit_points && grad && hit_index, "%s: null input pointer", what);
  return launch_begin(what, s, stream, occlusion_lobe_begin_kernel, rays_o, hit_points, grad, hit_index, n_hit, S,
                      1.0f / (shininess + 1.0f), bias, seed);
}

int oi_env_shade_glossy(const oi_env_shade_params* p, const float* rays_o, const float* hit_points, const float* grad,
                        const float* w2b, const float* spec_vis, const float* glossy, int M, int Hp, int Wp,
                        const int* map_index, const float* rot, const float* k_s, float* specular, oi_stream_t stream) {
  const char* what = "oi_env_shade_glossy";
  OI_TRY(check_env_shade(what, p, p && (p->shading || p->image || specular), "shading, image and specular are all null"));
  OI_TRY(check_gloss_maps(what, M, Hp, Wp));
  OI_REQUIRE(rays_o && w2b && glossy && map_index && rot && k_s, "%s: null glossy input pointer", what);
  OI_REQUIRE(p->n_hit == 0 || (hit_points && grad), "%s: null hit arrays with n_hit=%lld", what, p->n_hit);
  MapIndex mi = {};
  OI_TRY(pack_map_index(what, p->F, M, map_index, mi));
  const GlossArgs g = {rays_o, hit_points, grad, w2b, spec_vis, glossy, rot, k_s, specular, Hp, Wp, nullptr};
  hipLaunchKernelGGL(env_shade_glossy_kernel, dim3((unsigned)((p->N + ES_THREADS - 1) / ES_THREADS)), dim3(ES_THREADS), 0,
                     oi::as_stream(stream), *p, g, mi);
  return oi::check_launch(what);
}

}  // extern "C"
