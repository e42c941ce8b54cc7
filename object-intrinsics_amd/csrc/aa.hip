// Adaptive anti-aliasing of the sphere-traced surface renderer for gfx950 (include/oi_aa.h): three small
// memory-bound kernels around the march and the shade that serve any ray set, one thread per pixel, ray or plane value:
//   classify   a pixel is flagged when a neighbour differs in the mask, leaves its tangent plane or turns its normal away;
//              the flagged pixels compacted like a trace step's survivors (trace_common.h's wg_slot)
//   begin      the sub-pixel camera rays of the flagged pixels (ray_common.h's make_ray_at: oi_gen_rays' arithmetic), started
//              as oi_trace_begin starts rays
//   resolve    the centre value, or the mean of a flagged pixel's samples (the planes of the sub-samples at any stride)
// The classifier reads its eight neighbours straight from global memory: an image's status, slots, points and gradients are
// L2-resident, and the kernel is a few microseconds beside the 64-step chain that follows it.  No LDS beyond the compaction's
// five words, no scratch, no float atomics.
#include "aa_common.h"
#include "ray_common.h"

#include "../../include/oi_scene_aa.h"  // oi_aa_resolve_strided: oi_aa_resolve's kernel at the scene's stride

namespace {

__global__ void __launch_bounds__(TR_THREADS) aa_classify_kernel(const uint8_t* __restrict__ status, const int* __restrict__ hit_slot,
                                                                 const float* __restrict__ hit_points,
                                                                 const float* __restrict__ grad, long long n_hit, int H, int W,
                                                                 float s2, float c2, int* __restrict__ edge_index,
                                                                 int* __restrict__ edge_slot, int* __restrict__ count) {
#pragma clang fp contract(off)
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long N = (long long)H * W;
  const long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  bool flag = false;
  if (p < N) {
    const int y = (int)(p / W), x = (int)(p - (long long)y * W);
    const long long kp = status[p] == OI_TRACE_HIT ? (long long)hit_slot[p] : -1;
    const bool hp = kp >= 0 && kp < n_hit;
    float xp[3] = {0.f, 0.f, 0.f}, gp[3] = {0.f, 0.f, 0.f}, gpp = 0.f;
    if (hp) {
#pragma unroll
      for (int a = 0; a < 3; ++a) xp[a] = hit_points[kp * 3 + a], gp[a] = grad[kp * 3 + a];
      gpp = dot3(gp, gp);
    }
    for (int dy = -1; dy <= 1; ++dy) {
      const int yq = y + dy;
      if (yq < 0 || yq >= H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xq = x + dx;
        if (xq < 0 || xq >= W || (dx == 0 && dy == 0)) continue;
        const long long q = (long long)yq * W + xq;
        const long long kq = status[q] == OI_TRACE_HIT ? (long long)hit_slot[q] : -1;
        const bool hq = kq >= 0 && kq < n_hit;
        if (hq != hp) flag = true;
        if (!(hq && hp)) continue;
        float pq[3], gq[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) pq[a] = hit_points[kq * 3 + a], gq[a] = grad[kq * 3 + a];
        if (aa_pair_edge(xp, gp, gpp, pq, gq, s2, c2)) flag = true;
      }
    }
  }
  const long long slot = wg_slot(flag, count, lds);
  if (p < N) edge_slot[p] = flag ? (int)slot : -1;
  if (flag) edge_index[slot] = (int)p;
}

__global__ void __launch_bounds__(TR_THREADS) aa_begin_kernel(const oi_trace_state s, const float* __restrict__ c2b,
                                                              const float* __restrict__ kinv, const float* __restrict__ offs, int R,
                                                              const int* __restrict__ edge_index, long long n_edge,
                                                              const float* __restrict__ offsets) {
#pragma clang fp contract(off)
  clear_counts(s.counts, (int)s.N);
  const long long q = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (q >= s.N) return;
  const long long j1 = q / n_edge, e = q - j1 * n_edge;  // j1 = j - 1
  const int pix = edge_index[e];
  const int y = pix / R, x = pix - y * R;
  const float pitch = (float)R / (float)(R - 1);
  const float ox = offsets[(j1 + 1) * 2 + 0] * pitch, oy = offsets[(j1 + 1) * 2 + 1] * pitch;
  const float px = pixel_coord(R, x, offs[0]) + ox, py = pixel_coord(R, y, offs[1]) + oy;
  const RayOD ry = make_ray_at(c2b, kinv, px, py);
  write_ray(s, q, ry.o, ry.d, ry.near_, ry.far_, OI_TRACE_MARCH);
  s.active[q] = (int)q;
  // point_at's fmaf of the values just written
  s.points[q * 3 + 0] = __fmaf_rn(ry.near_, ry.d[0], ry.o[0]);
  s.points[q * 3 + 1] = __fmaf_rn(ry.near_, ry.d[1], ry.o[1]);
  s.points[q * 3 + 2] = __fmaf_rn(ry.near_, ry.d[2], ry.o[2]);
}

__global__ void __launch_bounds__(TR_THREADS) aa_resolve_kernel(const float* __restrict__ centre, const float* __restrict__ sub,
                                                                const int* __restrict__ edge_slot, long long N, long long n_edge,
                                                                int S, long long sub_stride, long long total, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= total) return;
  const long long plane = i / N, p = i - plane * N;
  const long long e = edge_slot[p];
  float acc = centre[i];
  if (e >= 0 && e < n_edge) {
    const float* __restrict__ sp = sub + plane * sub_stride + e;
    for (int j = 1; j < S; ++j) acc += sp[(long long)(j - 1) * n_edge];
    acc /= (float)S;
  }
  out[i] = acc;
}

// Arguments of oi_aa_resolve and oi_aa_resolve_strided, then the launch: one kernel for both.
inline int launch_resolve(const char* what, const float* centre, const float* sub, long long sub_stride, const int* edge_slot,
                          long long N, long long n_edge, int S, int P, float* out, oi_stream_t stream) {
  OI_TRY(check_pixels(what, N, n_edge));
  OI_TRY(check_aa_samples(what, S));
  OI_REQUIRE((S - 1) * n_edge < (1ll << 31), "%s: S=%d x n_edge=%lld sub-samples ((S - 1) * n_edge < 2^31)", what, S, n_edge);
  OI_REQUIRE(sub_stride >= (S - 1) * n_edge && sub_stride < (1ll << 31),
             "%s: sub_stride=%lld ((S - 1) * n_edge = %lld <= sub_stride < 2^31)", what, sub_stride, (S - 1) * n_edge);
  OI_REQUIRE(P >= 1 && (long long)P * N < (1ll << 39), "%s: P=%d planes of N=%lld (P >= 1, P * N < 2^39)", what, P, N);
  OI_REQUIRE(centre && edge_slot && out && (sub || n_edge == 0), "%s: null pointer", what);
  const long long total = (long long)P * N;
  hipLaunchKernelGGL(aa_resolve_kernel, dim3(n_blocks(total)), dim3(TR_THREADS), 0, oi::as_stream(stream), centre, sub, edge_slot, N,
                     n_edge, S, sub_stride, total, out);
  return oi::check_launch(what);
}

}  // namespace

extern "C" {

int oi_aa_classify(const uint8_t* status, const int* hit_slot, const float* hit_points, const float* grad, long long n_hit,
                   int H, int W, float plane_threshold, float cos_threshold, int* edge_index, int* edge_slot, int* count,
                   oi_stream_t stream) {
  const char* what = "oi_aa_classify";
  OI_REQUIRE(H >= 1 && W >= 1, "%s: H=%d, W=%d", what, H, W);
  OI_TRY(check_pixels(what, (long long)H * W, n_hit));
  OI_TRY(check_aa_thresholds(what, plane_threshold, cos_threshold));
  OI_REQUIRE(status && hit_slot && edge_index && edge_slot && count, "%s: null pointer", what);
  OI_REQUIRE(n_hit == 0 || (hit_points && grad), "%s: null hit arrays with n_hit=%lld", what, n_hit);
  const hipStream_t st = oi::as_stream(stream);
  hipLaunchKernelGGL(aa_clear_kernel, dim3(1), dim3(64), 0, st, count);
  hipLaunchKernelGGL(aa_classify_kernel, dim3(n_blocks((long long)H * W)), dim3(TR_THREADS), 0, st, status, hit_slot, hit_points,
                     grad, n_hit, H, W, plane_threshold * plane_threshold, cos_threshold * cos_threshold, edge_index, edge_slot,
                     count);
  return oi::check_launch(what);
}

int oi_aa_begin(const oi_trace_state* s, const float* c2b, const float* kinv, const float* offs, int R, const int* edge_index,
                long long n_edge, const float* offsets, int S, oi_stream_t stream) {
  const char* what = "oi_aa_begin";
  OI_TRY(check_state(s, what));
  OI_TRY(check_aa_samples(what, S));
  OI_REQUIRE(R >= 2 && R <= 46340, "%s: R=%d (2 <= R, R * R < 2^31)", what, R);
  OI_REQUIRE(n_edge >= 1 && n_edge <= (long long)R * R && (S - 1) * n_edge == s->N,
             "%s: n_edge=%lld, S=%d, N=%lld, R=%d (1 <= n_edge <= R * R, N must be (S - 1) * n_edge)", what, n_edge, S, s->N, R);
  OI_REQUIRE(c2b && kinv && offs && edge_index && offsets, "%s: null input pointer", what);
  hipLaunchKernelGGL(aa_begin_kernel, dim3(n_blocks(s->N)), dim3(TR_THREADS), 0, oi::as_stream(stream), *s, c2b, kinv, offs, R,
                     edge_index, n_edge, offsets);
  return oi::check_launch(what);
}

int oi_aa_resolve_strided(const float* centre, const float* sub, long long sub_stride, const int* edge_slot, long long N,
                          long long n_edge, int S, int P, float* out, oi_stream_t stream) {
  return launch_resolve("oi_aa_resolve_strided", centre, sub, sub_stride, edge_slot, N, n_edge, S, P, out, stream);
}

int oi_aa_resolve(const float* centre, const float* sub, const int* edge_slot, long long N, long long n_edge, int S, int P,
                  float* out, oi_stream_t stream) {
  return launch_resolve("oi_aa_resolve", centre, sub, (S - 1) * n_edge, edge_slot, N, n_edge, S, P, out, stream);
}

}  // extern "C"
