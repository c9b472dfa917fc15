// order_probe.cpp -- TEST-ONLY: three toy launches whose results depend on the order of execution, built against tests/emu/hipemu.h by
// tests/test_schedule_emu.py (g++ -include tests/emu/hipemu.h) and run once per HIPEMU_SCHEDULE.  They show that a schedule changes the
// order that is actually executed, and give the block-order net and the wave-local shuffle one demonstrated failure each:
//   visit    every thread of 3 blocks x 128 threads appends (block, thread) to a log: the order of execution itself
//   sweep    an in-place sweep in which block b adds row b + 1 to row b: right where block b runs before block b + 1 (the serial
//            ascending order), wrong where a higher-numbered block has already written its row
//   shuffle  two waves exchange through LDS with NO __syncthreads() between the store and the load, only a __shfl_xor: right where
//            the shuffle is two whole-block barriers (the default schedule, which hides the missing barrier), wrong where a wave
//            passes its shuffle alone
// Prints one line per launch (the shuffle launch: what was read from LDS, and the shuffled value); the test compares the lines.
#include <cstdio>
#include <vector>

struct Args {
  int* log;
  int* count;
  float* rows;
  int n;
  int* out;
};

static void visit_kernel(Args a) {
  const int i = __atomic_fetch_add(a.count, 1, __ATOMIC_SEQ_CST);
  a.log[i] = (int)blockIdx.x * 1000 + (int)threadIdx.x;
}

static void sweep_kernel(Args a) {
  const unsigned b = blockIdx.x, t = threadIdx.x;
  const float next = b + 1 < gridDim.x ? a.rows[(b + 1) * a.n + t] : 0.0f;
  a.rows[b * a.n + t] += next;
}

static void shuffle_kernel(Args a) {
  int* lds = (int*)hipemu::smem();
  const int t = (int)threadIdx.x;
  lds[t] = t + 1;
  const int partner = __shfl_xor(t, 1);  // (no __syncthreads(): the bug)
  a.out[t] = lds[(t + 64) % 128];
  a.out[128 + t] = partner;
}

int main() {
  const int blocks = 3, threads = 128, n = 8;
  std::vector<int> log(blocks * threads, -1), out(2 * threads, -1);
  std::vector<float> rows(5 * n);
  int count = 0;
  Args a{log.data(), &count, rows.data(), n, out.data()};
  hipemu::launch(dim3(blocks), dim3(threads), 0, visit_kernel, a);
  printf("visit");
  for (int v : log) printf(" %d", v);
  printf("\n");
  for (int b = 0; b < 5; ++b)
    for (int t = 0; t < n; ++t) rows[b * n + t] = (float)(1 << b);
  hipemu::launch(dim3(5), dim3(n), 0, sweep_kernel, a);
  printf("sweep");
  for (int b = 0; b < 5; ++b) printf(" %g", rows[b * n]);
  printf("\n");
  hipemu::launch(dim3(1), dim3(threads), threads * sizeof(int), shuffle_kernel, a);
  printf("shuffle");
  for (int t = 0; t < threads; ++t) printf(" %d", out[t]);
  printf("\npartner");
  for (int t = 0; t < threads; ++t) printf(" %d", out[threads + t]);
  printf("\n");
  return 0;
}
