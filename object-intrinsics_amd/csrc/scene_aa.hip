// Adaptive anti-aliasing of a scene of many instances for gfx950 (include/oi_scene_aa.h): the two kernels
// the scene needs beside aa.hip's and scene.hip's, small and memory-bound, one thread per scene pixel or ray:
//   classify   a scene pixel is flagged when a neighbour differs in the mask or in the owner, or -- same owner -- leaves its
//              tangent plane or turns its normal away (aa_common.h's aa_pair_edge, the single view's arithmetic); the flagged
//              pixels compacted like a trace step's survivors (trace_common.h's wg_slot)
//   begin      per instance the sub-pixel rays of the flagged pixels (ray_common.h's make_ray_at), under the primary's window
//              rule and scene.hip's cull (scene_common.h's unit_sphere_chord), stored through write_ray and compacted within
//              their element through enter_rays
// The classifier reads its eight neighbours straight from global memory: the owner maps, the slots, the points and the
// gradients of a scene image are L2-resident, and the kernel is a few microseconds beside the 64-step chain that follows.
// The rays' layout is the virtual scene image of oi_scene_aa.h, so every later stage is scene.hip's own.  No LDS beyond the
// compaction's five words, no scratch, no float atomics.
#include "aa_common.h"
#include "ray_common.h"
#include "scene_common.h"

#include "../../include/oi_scene_aa.h"

namespace {

// The row of the visible hit that owns scene pixel p in hit_points / grad [E][n_pad][3], or -1 ("not owned"); e: its owner.
__device__ __forceinline__ long long owned_row(const int* __restrict__ owner, const int* __restrict__ owner_ray,
                                               const int* __restrict__ vis_slot, int E, long long N, long long n_pad, long long p,
                                               int& e) {
  e = owner[p];
  if (e < 0 || e >= E) return -1;
  const long long r = owner_ray[p];
  if (r < 0 || r >= N) return -1;
  const long long k = vis_slot[(long long)e * N + r];
  if (k < 0 || k >= n_pad) return -1;
  return (long long)e * n_pad + k;
}

__global__ void __launch_bounds__(TR_THREADS) scene_aa_classify_kernel(const int* __restrict__ owner, const int* __restrict__ owner_ray,
                                                                       const int* __restrict__ vis_slot,
                                                                       const float* __restrict__ hit_points,
                                                                       const float* __restrict__ grad, int E, long long N,
                                                                       long long n_pad, int S, float s2, float c2,
                                                                       int* __restrict__ edge_index, int* __restrict__ edge_slot,
                                                                       int* __restrict__ count) {
#pragma clang fp contract(off)
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long M = (long long)S * S;
  const long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool flag = false;
  if (p < M) {
    const int y = (int)(p / S), x = (int)(p - (long long)y * S);
    int ep;
    const long long kp = owned_row(owner, owner_ray, vis_slot, E, N, n_pad, p, ep);
    const bool hp = kp >= 0;
    float xp[3] = {0.f, 0.f, 0.f}, gp[3] = {0.f, 0.f, 0.f}, gpp = 0.f;
    if (hp) {
#pragma unroll
      for (int a = 0; a < 3; ++a) xp[a] = hit_points[kp * 3 + a], gp[a] = grad[kp * 3 + a];
      gpp = dot3(gp, gp);
    }
    for (int dy = -1; dy <= 1; ++dy) {
      const int yq = y + dy;
      if (yq < 0 || yq >= S) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xq = x + dx;
        if (xq < 0 || xq >= S || (dx == 0 && dy == 0)) continue;
        int eq;
        const long long kq = owned_row(owner, owner_ray, vis_slot, E, N, n_pad, (long long)yq * S + xq, eq);
        const bool hq = kq >= 0;
        if (hq != hp) flag = true;
        if (!(hq && hp)) continue;
        if (eq != ep) {  // two instances meet: their box frames differ, and no tangent plane says the contour away
          flag = true;
          continue;
        }
        float pq[3], gq[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pq[a] = hit_points[kq * 3 + a], gq[a] = grad[kq * 3 + a];
        if (aa_pair_edge(xp, gp, gpp, pq, gq, s2, c2)) flag = true;
      }
    }
  }
  const long long slot = wg_slot(flag, count, lds);
  if (p < M) edge_slot[p] = flag ? (int)slot : -1;
  if (flag) edge_index[slot] = (int)p;
}

__global__ void __launch_bounds__(TR_THREADS) scene_aa_begin_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                    const float* __restrict__ c2b, const float* __restrict__ kinv,
                                                                    const int* __restrict__ window, int W, int S,
                                                                    const int* __restrict__ edge_index, long long n_edge,
                                                                    long long n_sub, const float* __restrict__ offsets) {
#pragma clang fp contract(off)
  __shared__ unsigned lds[TR_WAVES + 1];
  const int e = blockIdx.y;
  const oi_trace_state v = element_view(s, e);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool entered = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (q < s.N) {
    // (padding, and a pixel outside the image, have no ray: the slot holds pixel (0, 0)'s centre ray, never traced)
    int X = 0, Y = 0;
    float ox = 0.f, oy = 0.f;
    bool covered = false;
    if (q < n_sub) {
      const long long j1 = q / n_edge, k = q - j1 * n_edge;  // j1 = j - 1
      const long long pix = edge_index[k];
      if (pix >= 0 && pix < (long long)S * S) {
        Y = (int)(pix / S), X = (int)(pix - (long long)Y * S);
        const long long i = (long long)X - window[e * 2 + 0], j = (long long)Y - window[e * 2 + 1];
        covered = i >= 0 && i < W && j >= 0 && j < W;
        const float pitch = (float)S / (float)(S - 1);
        ox = offsets[(j1 + 1) * 2 + 0] * pitch, oy = offsets[(j1 + 1) * 2 + 1] * pitch;
      }
    }
    const RayOD ry = make_ray_at(c2b + (long long)e * 16, kinv, pixel_coord(S, X, 0.f) + ox, pixel_coord(S, Y, 0.f) + oy);
    float near_ = 0.f, far_ = 0.f;
    entered = unit_sphere_chord(ry.o, ry.d, near_, far_) && covered;
    if (!entered) near_ = far_ = 0.f;
    write_ray(v, q, ry.o, ry.d, near_, far_, entered ? OI_TRACE_MARCH : OI_TRACE_MISS);
    px = __fmaf_rn(near_, ry.d[0], ry.o[0]), py = __fmaf_rn(near_, ry.d[1], ry.o[1]), pz = __fmaf_rn(near_, ry.d[2], ry.o[2]);
  }
  enter_rays(v, q, entered, px, py, pz, lds, live);
}

}  // namespace

extern "C" {

int oi_scene_aa_classify(const int* owner, const int* owner_ray, const int* vis_slot, const float* hit_points, const float* grad,
                         int E, long long N, long long n_pad, int S, float plane_threshold, float cos_threshold,
                         int* edge_index, int* edge_slot, int* count, oi_stream_t stream) {
  const char* what = "oi_scene_aa_classify";
  OI_TRY(check_scene_rays(what, E, N));
  OI_TRY(check_resolution(what, "S", S));
  OI_REQUIRE(n_pad >= 0 && n_pad <= N, "%s: n_pad=%lld (0 <= n_pad <= N=%lld)", what, n_pad, N);
  OI_TRY(check_aa_thresholds(what, plane_threshold, cos_threshold));
  OI_REQUIRE(owner && owner_ray && vis_slot && edge_index && edge_slot && count, "%s: null pointer", what);
  OI_REQUIRE(n_pad == 0 || (hit_points && grad), "%s: null hit arrays with n_pad=%lld", what, n_pad);
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(aa_clear_kernel, dim3(1), dim3(64), 0, st, count);
  hipLaunchKernelGGL(scene_aa_classify_kernel, dim3(n_blocks((long long)S * S)), dim3(TR_THREADS), 0, st, owner, owner_ray, vis_slot,
                     hit_points, grad, E, N, n_pad, S, plane_threshold * plane_threshold, cos_threshold * cos_threshold, edge_index,
                     edge_slot, count);
  return oi::check_launch(what);
}

int oi_scene_aa_begin(const oi_trace_batch* b, const float* c2b, const float* kinv, const int* window, int W, int S,
                      const int* edge_index, long long n_edge, const float* offsets, int Sa, oi_stream_t stream) {
  const char* what = "oi_scene_aa_begin";
  OI_TRY(check_batch(b, what));
  OI_TRY(check_aa_samples(what, Sa));
  OI_REQUIRE(W >= 1, "%s: W=%d (W >= 1)", what, W);
  OI_REQUIRE(S >= 2 && S <= OI_SCENE_MAX_RESOLUTION, "%s: S=%d (2 .. %d)", what, S, OI_SCENE_MAX_RESOLUTION);
  OI_REQUIRE(n_edge >= 1 && n_edge <= (long long)S * S && (Sa - 1) * n_edge <= b->s.N,
             "%s: n_edge=%lld, Sa=%d, N=%lld, S=%d (1 <= n_edge <= S * S, (Sa - 1) * n_edge <= N)", what, n_edge, Sa, b->s.N, S);
  OI_REQUIRE(c2b && kinv && window && edge_index && offsets, "%s: null input pointer", what);
  const hipStream_t st = oi::as_stream(stream);
  const dim3 grid(n_blocks(b->s.N), b->E);
  hipLaunchKernelGGL(scene_clear_kernel, grid, dim3(TR_THREADS), 0, st, b->s, b->live);
  hipLaunchKernelGGL(scene_aa_begin_kernel, grid, dim3(TR_THREADS), 0, st, b->s, b->live, c2b, kinv, window, W, S, edge_index, n_edge,
                     (Sa - 1) * n_edge, offsets);
  return oi::check_launch(what);
}

}  // extern "C"
