// Environment lighting on the sphere-traced surface (include/oi_envlight.h), gfx950.
//   env_project           equirectangular maps -> 9 x 3 SH coefficients: per-workgroup partials, then one workgroup per map
//   transfer_resolve      the final states and directions of an ambient-occlusion trace -> the transfer map, one thread per pixel
//   transfer_normal       the unshadowed closed form
//   env_shade             transfer . coefficients for F environments, one thread per pixel, its transfer read once
//                         (env_shade_common.h's pixel without a further term)
// The pixel shape and the sample count are checked by trace_common.h's check_pixels and check_samples, as occlusion.hip's.
// No atomics at all, no scratch; every sum has one fixed order.
#include "env_shade_common.h"

namespace {

constexpr int EP_THREADS = 256;              // oi_env_project's workgroup
constexpr int EP_PER_THREAD = 32;            // pixels a thread sums in sequence
constexpr int EP_CHUNK = EP_THREADS * EP_PER_THREAD;  // pixels per workgroup: the 8192 of the header
constexpr int EP_INNER = 32;                 // the final pass: chains of 32 partials, nested twice (32 x 32 x 256 = 2^18 partials)
static_assert(EP_CHUNK == 8192, "the header states the chunk");
static_assert((long long)EP_INNER * EP_INNER * EP_THREADS * EP_CHUNK >= (1ll << 31), "the final pass covers E * He * We < 2^31");

// Sum of v over the workgroup's EP_THREADS threads in one fixed tree (6 butterfly levels in the wave, then the 4 waves as
// (w0 + w1) + (w2 + w3)); valid in thread 0.  Every thread calls it.  lds: 4 words.
__device__ __forceinline__ float wg_tree_sum(float v, float* lds) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();  // the previous call's reads of lds
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// stage 1: partial[e][b][27] = the sum over pixels [b * EP_CHUNK, (b + 1) * EP_CHUNK) of environment e
__global__ void __launch_bounds__(EP_THREADS) env_project_partial_kernel(const float* __restrict__ radiance, int He, int We,
                                                                         float wscale, float* __restrict__ partial) {
  __shared__ float lds[4];
  const long long P = (long long)He * We;
  const long long e = blockIdx.y, b = blockIdx.x;
  const float* __restrict__ img = radiance + e * 3 * P;
  float acc[NC][3];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c][0] = acc[c][1] = acc[c][2] = 0.f;
  for (int k = 0; k < EP_PER_THREAD; ++k) {
    const long long p = b * EP_CHUNK + (long long)k * EP_THREADS + threadIdx.x;  // consecutive threads, consecutive pixels
    if (p >= P) break;
    const long long r = p / We, c = p - r * We;
    float st, ct, sp, cp;
    sincospif((float)(((double)r + 0.5) / (double)He), &st, &ct);        // theta = pi (r + 1/2) / He
    sincospif((float)((2.0 * (double)c + 1.0) / (double)We), &sp, &cp);  // phi = 2 pi (c + 1/2) / We
    float y[NC];
    sh9(st * cp, st * sp, ct, y);
    const float w = st * wscale;  // 2 sin(theta) sin(pi / (2 He)) 2 pi / We
    const float l0 = img[p], l1 = img[P + p], l2 = img[2 * P + p];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      const float wy = w * y[q];
      acc[q][0] = __fmaf_rn(wy, l0, acc[q][0]);
      acc[q][1] = __fmaf_rn(wy, l1, acc[q][1]);
      acc[q][2] = __fmaf_rn(wy, l2, acc[q][2]);
    }
  }
  float* __restrict__ out = partial + (e * gridDim.x + b) * OI_ENV_FLOATS;
#pragma unroll
  for (int q = 0; q < NC; ++q)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float s = wg_tree_sum(acc[q][ch], lds);
      if (threadIdx.x == 0) out[q * 3 + ch] = s;
    }
}

// stage 2: coeffs[e][27] = the sum of the nb partials of environment e.  Thread t takes partials t, t + 256, ...: chains of
// EP_INNER terms, their sums in a chain of at most EP_INNER, then the tree.
__global__ void __launch_bounds__(EP_THREADS) env_project_final_kernel(const float* __restrict__ partial, long long nb,
                                                                       float* __restrict__ coeffs) {
  __shared__ float lds[4];
  const long long e = blockIdx.x;
  const float* __restrict__ src = partial + e * nb * OI_ENV_FLOATS;
  for (int v = 0; v < OI_ENV_FLOATS; ++v) {
    float outer = 0.f;
    for (long long b0 = threadIdx.x; b0 < nb; b0 += (long long)EP_THREADS * EP_INNER) {
      float inner = 0.f;
      for (int k = 0; k < EP_INNER; ++k) {
        const long long b = b0 + (long long)k * EP_THREADS;
        if (b >= nb) break;
        inner += src[b * OI_ENV_FLOATS + v];
      }
      outer += inner;
    }
    const float s = wg_tree_sum(outer, lds);
    if (threadIdx.x == 0) coeffs[e * OI_ENV_FLOATS + v] = s;
  }
}

__global__ void __launch_bounds__(TR_THREADS) transfer_resolve_kernel(const uint8_t* __restrict__ status,
                                                                      const float* __restrict__ rays_d,
                                                                      const int* __restrict__ hit_slot, long long N,
                                                                      long long n_hit, int S, const float* __restrict__ w2b,
                                                                      float* __restrict__ transfer) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N) return;
  const int slot = hit_slot[i];
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.f;
  if (slot >= 0) {
    for (int j = 0; j < S; ++j) {
      const long long q = (long long)j * n_hit + slot;
      if (status[q] != OI_TRACE_MISS) continue;
      float x, y, z;
      to_world(w2b, rays_d[q * 3 + 0], rays_d[q * 3 + 1], rays_d[q * 3 + 2], x, y, z);
      normalize3(x, y, z, 1e-6f);
      float sh[NC];
      sh9(x, y, z, sh);
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[c] += sh[c];
    }
    const float s = (float)S;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] /= s;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) transfer[c * N + i] = acc[c];
}

__global__ void __launch_bounds__(TR_THREADS) transfer_normal_kernel(const float* __restrict__ grad,
                                                                     const int* __restrict__ hit_slot, long long N,
                                                                     const float* __restrict__ w2b,
                                                                     float* __restrict__ transfer) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N) return;
  const long long k = hit_slot[i];
  float t[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) t[c] = 0.f;
  if (k >= 0) {
    float nx, ny, nz;
    unit_normal(grad, k, nx, ny, nz);
    normal_transfer(w2b, nx, ny, nz, t);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) transfer[c * N + i] = t[c];
}

__global__ void __launch_bounds__(ES_THREADS) env_shade_kernel(const oi_env_shade_params p) {
  env_shade_pixel<EnvTerm::NONE>(p);
}

long long project_blocks(int He, int We) { return ((long long)He * We + EP_CHUNK - 1) / EP_CHUNK; }

bool project_args_ok(int E, int He, int We) {
  return E >= 1 && E <= OI_ENV_MAX_ENVS && He >= 1 && We >= 1 && (long long)E * He * We < (1ll << 31);
}

}  // namespace

extern "C" {

size_t oi_env_project_partial_floats(int E, int He, int We) {
  return project_args_ok(E, He, We) ? (size_t)E * (size_t)project_blocks(He, We) * OI_ENV_FLOATS : 0;
}

int oi_env_project(const float* radiance, int E, int He, int We, float* partial, float* coeffs, oi_stream_t stream) {
  OI_REQUIRE(project_args_ok(E, He, We), "oi_env_project: E=%d, He=%d, We=%d (1 <= E <= %d, He >= 1, We >= 1, E * He * We < 2^31)",
             E, He, We, OI_ENV_MAX_ENVS);
  OI_REQUIRE(radiance && partial && coeffs, "oi_env_project: null pointer");
  const long long nb = project_blocks(He, We);
  const double kPi = 3.14159265358979323846;
  const float wscale = (float)(2.0 * sin(kPi / (2.0 * He)) * (2.0 * kPi / We));
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(env_project_partial_kernel, dim3((unsigned)nb, (unsigned)E), dim3(EP_THREADS), 0, st, radiance, He, We, wscale,
                     partial);
  hipLaunchKernelGGL(env_project_final_kernel, dim3((unsigned)E), dim3(EP_THREADS), 0, st, (const float*)partial, nb, coeffs);
  return oi::check_launch("oi_env_project");
}

int oi_transfer_resolve(const uint8_t* status, const float* rays_d, const int* hit_slot, long long N, long long n_hit, int S,
                        const float* w2b, float* transfer, oi_stream_t stream) {
  OI_TRY(check_pixels("oi_transfer_resolve", N, n_hit));
  OI_TRY(check_samples("oi_transfer_resolve", S));
  OI_REQUIRE(n_hit * S < (1ll << 31), "oi_transfer_resolve: S * n_hit = %lld rays (below 2^31)", n_hit * S);
  OI_REQUIRE(hit_slot && w2b && transfer && ((status && rays_d) || n_hit == 0), "oi_transfer_resolve: null pointer");
  hipLaunchKernelGGL(transfer_resolve_kernel, dim3(n_blocks(N)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, rays_d, hit_slot,
                     N, n_hit, S, w2b, transfer);
  return oi::check_launch("oi_transfer_resolve");
}

int oi_transfer_normal(const float* grad, const int* hit_slot, long long N, long long n_hit, const float* w2b, float* transfer,
                       oi_stream_t stream) {
  OI_TRY(check_pixels("oi_transfer_normal", N, n_hit));
  OI_REQUIRE(hit_slot && w2b && transfer && (grad || n_hit == 0), "oi_transfer_normal: null pointer");
  hipLaunchKernelGGL(transfer_normal_kernel, dim3(n_blocks(N)), dim3(TR_THREADS), 0, oi::as_stream(stream), grad, hit_slot, N, w2b,
                     transfer);
  return oi::check_launch("oi_transfer_normal");
}

int oi_env_shade(const oi_env_shade_params* p, oi_stream_t stream) {
  OI_TRY(check_env_shade("oi_env_shade", p, p && (p->shading || p->image), "shading and image are both null"));
  hipLaunchKernelGGL(env_shade_kernel, dim3((unsigned)((p->N + ES_THREADS - 1) / ES_THREADS)), dim3(ES_THREADS), 0,
                     oi::as_stream(stream), *p);
  return oi::check_launch("oi_env_shade");
}

}  // extern "C"
