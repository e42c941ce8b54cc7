// One diffuse interreflection bounce between the instances of a scene for gfx950 (include/oi_scene_bounce.h, DESIGN section
// 4.26): the glue between scene_light.hip's sampled rays against every instance, marched to their CLOSEST hit, and
// envbounce.hip's bounce transfer.  Small memory-bound kernels, one thread per ray or scene pixel:
//   bounce_nearest   per ray the element whose hit is nearest, or none: a fixed-order loop over the elements
//   bounce_visible   per element the dense list of the rays it wins (scene.hip's visible, keyed by the winner): the input of
//                    the gather and of the full MLP pass, so hits that a nearer instance hides never reach the MLP
//   bounce_resolve   per scene pixel the 27 running sums of the bounce transfer over the chunk's samples, in sample order,
//                    kept in the output between chunks; the per-sample term is bounce_common.h's, envbounce.hip's own
// The only atomics are the compaction's integer counters (wg_slot); no LDS beyond its counter words, no scratch.
#include "bounce_common.h"
#include "scene_common.h"

#include "../../include/oi_scene_bounce.h"

namespace {

constexpr int NC = OI_ENV_COEFFS;

__global__ void __launch_bounds__(TR_THREADS) scene_bounce_nearest_kernel(const uint8_t* __restrict__ status,
                                                                          const float* __restrict__ t, int E, long long Nr,
                                                                          int* __restrict__ winner) {
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= Nr) return;
  int best = -1;
  float best_t = INFINITY;
  bool dead = false;
  for (int e = 0; e < E; ++e) {  // no early exit: the order is fixed
    const unsigned st = status[(long long)e * Nr + q];
    if (st == OI_TRACE_HIT) {
      const float te = t[(long long)e * Nr + q];
      if (best < 0 || te < best_t) best = e, best_t = te;  // equal t: the lowest element index stays
    } else if (st != OI_TRACE_MISS) {
      dead = true;
    }
  }
  winner[q] = dead ? -1 : best;
}

__global__ void __launch_bounds__(TR_THREADS) scene_bounce_clear_kernel(int* __restrict__ counts, int* __restrict__ live, int E) {
  clear_hit_words(counts, live, E);
}

__global__ void __launch_bounds__(TR_THREADS) scene_bounce_visible_kernel(int* __restrict__ counts, int* __restrict__ live,
                                                                          long long Nr, const int* __restrict__ winner,
                                                                          int* __restrict__ sel_index,
                                                                          int* __restrict__ sel_slot) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const int e = blockIdx.y;
  const long long r = (long long)blockIdx.x * TR_THREADS + threadIdx.x, base = (long long)e * Nr;
  const bool mine = r < Nr && winner[r] == e;
  const long long slot = wg_slot(mine, counts + (long long)e * OI_TRACE_COUNT_WORDS + N_HIT_WORD, lds, live + N_HIT_WORD);
  if (r < Nr) sel_slot[base + r] = mine ? (int)slot : -1;
  if (mine) sel_index[base + slot] = (int)r;
}

__global__ void __launch_bounds__(TR_THREADS) scene_bounce_resolve_kernel(
    const int* __restrict__ winner, const int* __restrict__ sel_slot, const float* __restrict__ rays_d,
    const float* __restrict__ grad2, const float* __restrict__ rgb2, long long n_pad2, const int* __restrict__ owner,
    const int* __restrict__ owner_ray, const int* __restrict__ vis_slot, const int* __restrict__ offset,
    const float* __restrict__ w2b, int E, long long N, int S, int j0, int Sc, long long n_vis, long long M, int last,
    float* __restrict__ bounce) {
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= M) return;
  const int e = owner[q];
  BounceSums sums;
  auto& acc = sums.v;
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[0][c] = acc[1][c] = acc[2][c] = 0.f;
  if (e >= 0) {
    if (j0 > 0) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[ch][c] = bounce[((long long)ch * NC + c) * M + q];
    }
    if (n_pad2 > 0) {
      const long long g = (long long)offset[e] + vis_slot[(long long)e * N + owner_ray[q]], rays = (long long)Sc * n_vis;
      for (int jj = 0; jj < Sc; ++jj) {
        const long long ray = (long long)jj * n_vis + g;
        const int w = winner[ray];
        if (w < 0 || w >= E) continue;  // no winner: free, or ended without a verdict in some element
        const long long r = (long long)w * rays + ray, k = sel_slot[r];
        if (k < 0 || k >= n_pad2) continue;  // (nothing is read outside grad2 / rgb2 whatever the lists hold)
        sums = bounce_sample(grad2, rgb2, (long long)w * n_pad2 + k, rays_d, r, w2b + (long long)w * 16, sums);
      }
    }
    if (last) {
      const float s = (float)S;
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[0][c] /= s, acc[1][c] /= s, acc[2][c] /= s;
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int c = 0; c < NC; ++c) bounce[((long long)ch * NC + c) * M + q] = acc[ch][c];
}

}  // namespace

extern "C" {

int oi_scene_bounce_nearest(const uint8_t* status, const float* t, int E, long long Nr, int* winner, oi_stream_t stream) {
  const char* what = "oi_scene_bounce_nearest";
  OI_TRY(check_scene_rays(what, E, Nr));
  OI_REQUIRE(status && t && winner, "%s: null pointer", what);
  hipLaunchKernelGGL(scene_bounce_nearest_kernel, dim3(n_blocks(Nr)), dim3(TR_THREADS), 0, oi::as_stream(stream), status, t, E, Nr,
                     winner);
  return oi::check_launch(what);
}

int oi_scene_bounce_visible(const oi_trace_batch* sb, const int* winner, int* sel_index, int* sel_slot, oi_stream_t stream) {
  const char* what = "oi_scene_bounce_visible";
  OI_TRY(check_batch(sb, what));
  OI_REQUIRE(winner && sel_index && sel_slot, "%s: null pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(scene_bounce_clear_kernel, dim3(n_blocks(sb->E)), dim3(TR_THREADS), 0, st, sb->s.counts, sb->live, sb->E);
  hipLaunchKernelGGL(scene_bounce_visible_kernel, dim3(n_blocks(sb->s.N), sb->E), dim3(TR_THREADS), 0, st, sb->s.counts, sb->live,
                     sb->s.N, winner, sel_index, sel_slot);
  return oi::check_launch(what);
}

int oi_scene_bounce_resolve(const int* winner, const int* sel_slot, const float* rays_d, const float* grad2, const float* rgb2,
                            long long n_pad2, const int* owner, const int* owner_ray, const int* vis_slot, const int* offset,
                            const float* w2b, int E, long long N, int S, int j0, int Sc, long long n_vis, int scene_S, int last,
                            float* bounce, oi_stream_t stream) {
  const char* what = "oi_scene_bounce_resolve";
  OI_TRY(check_chunk(what, 1, S, j0, Sc));
  OI_TRY(check_resolve(what, E, N, 1, Sc, n_vis, scene_S));
  OI_REQUIRE(n_pad2 >= 0 && n_pad2 <= Sc * n_vis, "%s: n_pad2=%lld secondary points per element of %lld rays", what, n_pad2,
             Sc * n_vis);
  OI_REQUIRE(winner && sel_slot && rays_d && owner && owner_ray && vis_slot && offset && w2b && bounce, "%s: null pointer", what);
  OI_REQUIRE((grad2 && rgb2) || n_pad2 == 0, "%s: null grad2 / rgb2 with n_pad2=%lld", what, n_pad2);
  const long long M = (long long)scene_S * scene_S;
  hipLaunchKernelGGL(scene_bounce_resolve_kernel, dim3(n_blocks(M)), dim3(TR_THREADS), 0, oi::as_stream(stream), winner, sel_slot,
                     rays_d, grad2, rgb2, n_pad2, owner, owner_ray, vis_slot, offset, w2b, E, N, S, j0, Sc, n_vis, M, last, bounce);
  return oi::check_launch(what);
}

}  // extern "C"
