// One diffuse interreflection bounce under environment lighting (include/oi_envbounce.h), gfx950.
//   bounce_resolve        the final states of a closest-hit trace of the transfer rays, the normals and albedo at their hits
//                         -> the per-channel bounce transfer [3][9][N], one thread per pixel, 27 sums in registers
//   env_shade_bounce      (transfer + bounce[ch]) . coefficients for F environments, one thread per pixel, its 36 values read once
//                         (env_shade_common.h's pixel with the BOUNCE term)
// The pixel shape and the sample count are checked by trace_common.h's check_pixels and check_samples, as envlight.hip's.
// The per-sample term of bounce_resolve is bounce_common.h's bounce_sample, shared with scene_bounce.hip.
// No atomics at all, no LDS, no scratch; every sum has one fixed order.
#include "bounce_common.h"
#include "env_shade_common.h"
#include "../../include/oi_envbounce.h"

namespace {

__global__ void __launch_bounds__(TR_THREADS) bounce_resolve_kernel(const uint8_t* __restrict__ status,
                                                                    const float* __restrict__ rays_d,
                                                                    const int* __restrict__ hit_slot2,
                                                                    const float* __restrict__ grad2,
                                                                    const float* __restrict__ rgb2,
                                                                    const int* __restrict__ hit_slot, long long N,
                                                                    long long n_hit, long long n_hit2, int S,
                                                                    const float* __restrict__ w2b, float* __restrict__ bounce) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N) return;
  const int slot = hit_slot[i];
  BounceSums sums;
  auto& acc = sums.v;
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[0][c] = acc[1][c] = acc[2][c] = 0.f;
  if (slot >= 0 && n_hit2 > 0) {
    for (int j = 0; j < S; ++j) {
      const long long q = (long long)j * n_hit + slot;
      if (status[q] != OI_TRACE_HIT) continue;
      const long long k = hit_slot2[q];
      if (k < 0 || k >= n_hit2) continue;  // (a finished state lists every HIT; nothing is read outside grad2 / rgb2 whatever it holds)
      sums = bounce_sample(grad2, rgb2, k, rays_d, q, w2b, sums);  // bounce_common.h: the term scene_bounce.hip shares
    }
    const float s = (float)S;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[0][c] /= s, acc[1][c] /= s, acc[2][c] /= s;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int c = 0; c < NC; ++c) bounce[((long long)ch * NC + c) * N + i] = acc[ch][c];
}

__global__ void __launch_bounds__(ES_THREADS) env_shade_bounce_kernel(const oi_env_shade_bounce_params p) {
  env_shade_pixel<EnvTerm::BOUNCE>(p);
}

}  // namespace

extern "C" {

int oi_bounce_resolve(const uint8_t* status, const float* rays_d, const int* hit_slot2, const float* grad2, const float* rgb2,
                      const int* hit_slot, long long N, long long n_hit, long long n_hit2, int S, const float* w2b, float* bounce,
                      oi_stream_t stream) {
  OI_TRY(check_pixels("oi_bounce_resolve", N, n_hit));
  OI_TRY(check_samples("oi_bounce_resolve", S));
  OI_REQUIRE(n_hit * S < (1ll << 31), "oi_bounce_resolve: S * n_hit = %lld rays (below 2^31)", n_hit * S);
  OI_REQUIRE(n_hit2 >= 0 && n_hit2 <= n_hit * S, "oi_bounce_resolve: n_hit2=%lld secondary hits of %lld rays", n_hit2, n_hit * S);
  OI_REQUIRE(hit_slot && w2b && bounce && ((status && rays_d && hit_slot2) || n_hit == 0), "oi_bounce_resolve: null pointer");
  OI_REQUIRE((grad2 && rgb2) || n_hit2 == 0, "oi_bounce_resolve: null grad2 / rgb2 with n_hit2=%lld", n_hit2);
  hipLaunchKernelGGL(bounce_resolve_kernel, dim3(n_blocks(N)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, rays_d, hit_slot2,
                     grad2, rgb2, hit_slot, N, n_hit, n_hit2, S, w2b, bounce);
  return oi::check_launch("oi_bounce_resolve");
}

int oi_env_shade_bounce(const oi_env_shade_bounce_params* p, oi_stream_t stream) {
  const char* what = "oi_env_shade_bounce";
  OI_TRY(check_env_shade(what, p, p && (p->shading || p->image || p->indirect), "shading, image and indirect are all null"));
  OI_REQUIRE(p->bounce != nullptr, "%s: null bounce (oi_env_shade shades a capture without one)", what);
  hipLaunchKernelGGL(env_shade_bounce_kernel, dim3((unsigned)((p->N + ES_THREADS - 1) / ES_THREADS)), dim3(ES_THREADS), 0,
                     oi::as_stream(stream), *p);
  return oi::check_launch(what);
}

}  // extern "C"
