// Host-side argument checks of csrc/trace_batch.hip under the host sanitizers: a stand-alone program, no GPU needed.
// Every call below is invalid and must return OI_ERR_INVALID_ARG with its text BEFORE any launch (no pointer here is real).
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/dbg/trace_batch_args.hip -o tools/dbg/bin/trace_batch_args && tools/dbg/bin/trace_batch_args
//
// (oi_sdf_mlp_fwd_segments lives in csrc/mlp.hip, which links against the rest of the library: its refusals are covered by
// tests/test_trace_batch_cpu.py only.)
#include "../../object-intrinsics_amd/csrc/trace_batch.hip"

#include <cstdio>
#include <cstring>

static int failures = 0;

static void expect(int rc, const char* entry, const char* text) {
  const char* msg = oi::err_buf();
  const bool ok = rc == OI_ERR_INVALID_ARG && strncmp(msg, entry, strlen(entry)) == 0 && strstr(msg, text) != nullptr;
  printf("%s %-24s rc=%d  %s\n", ok ? "ok  " : "FAIL", entry, rc, msg);
  failures += !ok;
}

static oi_trace_batch batch(int E, long long N) {
  static int word;  // a non-null address for every array; never dereferenced
  void* f = &word;
  oi_trace_batch b;
  b.s.N = N;
  b.s.rays_o = b.s.rays_d = b.s.near_ = b.s.far_ = b.s.t = b.s.bracket = b.s.points = (float*)f;
  b.s.status = b.s.side = (uint8_t*)f;
  b.s.steps = (uint16_t*)f;
  b.s.active = b.s.counts = (int*)f;
  b.E = E;
  b.live = (int*)f;
  return b;
}

int main() {
  static float fl;
  static int in;
  oi_trace_batch b = batch(3, 5);
  expect(oi_trace_batch_begin(nullptr, nullptr), "oi_trace_batch_begin", "null batch");
  b = batch(0, 5);
  expect(oi_trace_batch_begin(&b, nullptr), "oi_trace_batch_begin", "E=0");
  b = batch(1025, 5);
  expect(oi_trace_batch_begin(&b, nullptr), "oi_trace_batch_begin", "E=1025");
  expect(oi_trace_batch_step(&b, &fl, 5, 0, 1e-5f, 1.0f, nullptr), "oi_trace_batch_step", "E=1025");
  expect(oi_trace_batch_finish(&b, &in, &in, nullptr), "oi_trace_batch_finish", "E=1025");
  expect(oi_trace_batch_gather(&b, &in, 2, &fl, nullptr), "oi_trace_batch_gather", "E=1025");
  b = batch(3, 0);
  expect(oi_trace_batch_begin(&b, nullptr), "oi_trace_batch_begin", "N=0");
  b = batch(1024, 1ll << 21);
  expect(oi_trace_batch_begin(&b, nullptr), "oi_trace_batch_begin", "2^31");
  b = batch(3, 5);
  b.s.t = nullptr;
  expect(oi_trace_batch_begin(&b, nullptr), "oi_trace_batch_begin", "null pointer");
  b = batch(3, 5);
  b.live = nullptr;
  expect(oi_trace_batch_begin(&b, nullptr), "oi_trace_batch_begin", "null live");
  b = batch(3, 5);
  expect(oi_trace_batch_step(&b, &fl, 6, 0, 1e-5f, 1.0f, nullptr), "oi_trace_batch_step", "bound=6");
  expect(oi_trace_batch_step(&b, &fl, -1, 0, 1e-5f, 1.0f, nullptr), "oi_trace_batch_step", "bound=-1");
  expect(oi_trace_batch_step(&b, &fl, 5, 1024, 1e-5f, 1.0f, nullptr), "oi_trace_batch_step", "k=1024");
  expect(oi_trace_batch_step(&b, &fl, 5, 0, 0.0f, 1.0f, nullptr), "oi_trace_batch_step", "tol");
  expect(oi_trace_batch_step(&b, nullptr, 5, 0, 1e-5f, 1.0f, nullptr), "oi_trace_batch_step", "null sdf");
  expect(oi_trace_batch_finish(&b, nullptr, &in, nullptr), "oi_trace_batch_finish", "null output");
  expect(oi_trace_batch_gather(&b, &in, 6, &fl, nullptr), "oi_trace_batch_gather", "n_pad=6");
  expect(oi_trace_batch_gather(&b, &in, 2, nullptr, nullptr), "oi_trace_batch_gather", "null pointer");
  // the two calls that succeed without a launch
  if (oi_trace_batch_step(&b, nullptr, 0, 3, 1e-5f, 1.0f, nullptr) != OI_OK) ++failures, printf("FAIL bound = 0\n");
  if (oi_trace_batch_gather(&b, nullptr, 0, nullptr, nullptr) != OI_OK) ++failures, printf("FAIL n_pad = 0\n");
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
