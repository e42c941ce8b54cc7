// Batched sphere tracing for gfx950 (include/oi_trace_batch.h): the kernels of trace.hip with
// blockIdx.y = element.  Each workgroup takes its element's view of the batched state -- every pointer moved to the element's
// segment, a valid oi_trace_state of N rays -- and runs trace_common.h's per-ray functions on it: the ray state machine and
// the compaction are trace.hip's, not a copy.  What is new is `live`, the per-step maximum of the elements' counters that
// the host reads instead of a single count (wg_slot: one integer atomicMax per workgroup), and the padded gather of the hit
// points, which makes the E ragged hit lists one (E, n_pad) input of the library's full MLP pass.
#include "trace_common.h"

namespace {

__global__ void __launch_bounds__(TR_THREADS) trace_batch_begin_kernel(const oi_trace_state s, int* __restrict__ live) {
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int i = threadIdx.x; i < OI_TRACE_COUNT_WORDS; i += TR_THREADS) live[i] = i == 0 ? (int)s.N : 0;
  trace_begin_rays(element_view(s, blockIdx.y));
}

__global__ void __launch_bounds__(TR_THREADS) trace_batch_step_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                      const float* __restrict__ sdf, long long bound, int k,
                                                                      float tol, float omega) {
  __shared__ unsigned lds[TR_WAVES + 1];
  trace_step_rays<false>(element_view(s, blockIdx.y), sdf + (long long)blockIdx.y * s.N, bound, k, tol, omega, lds, live + k + 1);
}

__global__ void __launch_bounds__(TR_THREADS) trace_batch_finish_kernel(const oi_trace_state s, int* __restrict__ live,
                                                                        int* __restrict__ hit_index,
                                                                        int* __restrict__ hit_slot) {
  __shared__ unsigned lds[TR_WAVES + 1];
  const long long o = (long long)blockIdx.y * s.N;
  trace_finish_rays<false>(element_view(s, blockIdx.y), hit_index + o, nullptr, hit_slot + o, lds, live + N_HIT_WORD);
}

__global__ void __launch_bounds__(TR_THREADS) trace_batch_gather_kernel(const oi_trace_state s, const int* __restrict__ hit_index,
                                                                        long long n_pad, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= n_pad) return;
  const oi_trace_state v = element_view(s, blockIdx.y);
  float* dst = out + ((long long)blockIdx.y * n_pad + i) * 3;
  if (i < v.counts[N_HIT_WORD]) {
    const long long r = hit_index[(long long)blockIdx.y * s.N + i];
    point_at(v.rays_o, v.rays_d, r, v.t[r], dst);
  } else {
    dst[0] = dst[1] = dst[2] = 0.f;  // padding: a valid point for the full pass, whose output for it nobody reads
  }
}

}  // namespace

extern "C" {

int oi_trace_batch_begin(const oi_trace_batch* b, oi_stream_t stream) {
  int rc = check_batch(b, "oi_trace_batch_begin");
  if (rc != OI_OK) return rc;
  hipLaunchKernelGGL(trace_batch_begin_kernel, dim3(n_blocks(b->s.N), b->E), dim3(TR_THREADS), 0, oi::as_stream(stream), b->s,
                     b->live);
  return oi::check_launch("oi_trace_batch_begin");
}

int oi_trace_batch_step(const oi_trace_batch* b, const float* sdf, long long bound, int k, float tol, float omega,
                        oi_stream_t stream) {
  const char* what = "oi_trace_batch_step";
  int rc = check_batch(b, what);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(k >= 0 && k < OI_TRACE_MAX_STEPS, "%s: step k=%d (0 <= k < %d)", what, k, OI_TRACE_MAX_STEPS);
  OI_REQUIRE(bound >= 0 && bound <= b->s.N, "%s: bound=%lld (0 <= bound <= N=%lld)", what, bound, b->s.N);
  OI_REQUIRE(tol > 0.f && omega > 0.f && tol < INFINITY && omega < INFINITY, "%s: tol %g, omega %g (both > 0, finite)", what,
             (double)tol, (double)omega);
  if (bound == 0) return OI_OK;
  OI_REQUIRE(sdf != nullptr, "%s: null sdf", what);
  hipLaunchKernelGGL(trace_batch_step_kernel, dim3(n_blocks(bound), b->E), dim3(TR_THREADS), 0, oi::as_stream(stream), b->s,
                     b->live, sdf, bound, k, tol, omega);
  return oi::check_launch(what);
}

int oi_trace_batch_finish(const oi_trace_batch* b, int* hit_index, int* hit_slot, oi_stream_t stream) {
  int rc = check_batch(b, "oi_trace_batch_finish");
  if (rc != OI_OK) return rc;
  OI_REQUIRE(hit_index && hit_slot, "oi_trace_batch_finish: null output pointer");
  hipLaunchKernelGGL(trace_batch_finish_kernel, dim3(n_blocks(b->s.N), b->E), dim3(TR_THREADS), 0, oi::as_stream(stream), b->s,
                     b->live, hit_index, hit_slot);
  return oi::check_launch("oi_trace_batch_finish");
}

int oi_trace_batch_gather(const oi_trace_batch* b, const int* hit_index, long long n_pad, float* hit_points_padded,
                          oi_stream_t stream) {
  const char* what = "oi_trace_batch_gather";
  int rc = check_batch(b, what);
  if (rc != OI_OK) return rc;
  OI_REQUIRE(n_pad >= 0 && n_pad <= b->s.N, "%s: n_pad=%lld (0 <= n_pad <= N=%lld)", what, n_pad, b->s.N);
  if (n_pad == 0) return OI_OK;
  OI_REQUIRE(hit_index && hit_points_padded, "%s: null pointer", what);
  hipLaunchKernelGGL(trace_batch_gather_kernel, dim3(n_blocks(n_pad), b->E), dim3(TR_THREADS), 0, oi::as_stream(stream), b->s,
                     hit_index, n_pad, hit_points_padded);
  return oi::check_launch(what);
}

}  // extern "C"
