// Phase-cost probe for mlp_step_fused_kernel: build with -DPROBE_SKIP_*
// to excise a phase and difference the step time (timing only — skipped
// phases leave garbage math, never use for numerics).
//
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 \
//         -o benchmarks/probe_base.bin benchmarks/probe_floor.hip
//   hipcc ... -DPROBE_SKIP_FWDBWD -o benchmarks/probe_nofwd.bin ...
// (the -mllvm flag is the extension's, setup.py: without it the probe times
// a kernel that fetches its first arguments by a scalar load)
//
// Two more switches, for the tail behind the hand-off:
//   -DPROBE_CONST_CORR   the Adam bias corrections are constants (no pow):
//                        base minus this is what the two pow expansions cost
//   -DPROBE_COUNT_POLLS  workgroup 0's polling wave bins its poll rounds per
//                        launch (1 .. 13, 14+) in the spare words behind slab
//                        0's tag; the probe prints the histogram of the timed
//                        launches (the atomic add is in the timing: read the
//                        counts of this build, not its time)
// And one for where the waves stand inside the step:
//   -DPROBE_STAMPS       every wave records the wall clock and the cycle
//                        counter at fourteen points (ST_* in the kernel file)
//                        into a buffer of the probe's; the probe prints which
//                        wave is last at the second and at the third barrier,
//                        how often and by how much, and the span of the
//                        16-slab load batch (the stamps are in the timing:
//                        read the tables of this build, not its time)
//
#include "../unionml_amd/ops/hip/tabular_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
  fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e), __FILE__, __LINE__); \
  exit(1); } } while (0)

#ifdef PROBE_STAMPS
#include <vector>

static const char* const ST_NAMES[ST_POINTS] = {
    "entry", "behind b1", "row seg end", "last MFMA", "store drain", "poll matched",
    "behind b4", "first slab load", "loads issued", "loads arrived", "verdict read",
    "g folded", "p computed", "last store"};

// which wave of a workgroup reaches `point` last (cycle counter: one CU), how
// often, and its mean lead over the second-to-last wave
static void report_last_wave(const std::vector<unsigned long long>& st, int first,
                             int launches, int n_wg, int point, const char* what) {
  long long times[WAVES] = {0};
  double margin[WAVES] = {0};
  for (int s = first; s < first + launches; ++s)
    for (int g = 0; g < n_wg; ++g) {
      const unsigned long long* wg = &st[((size_t)s * n_wg + g) * WAVES * 2 * ST_POINTS];
      int last = 0;
      unsigned long long top = 0, second = 0;
      for (int w = 0; w < WAVES; ++w) {
        const unsigned long long c = wg[w * 2 * ST_POINTS + ST_POINTS + point];
        if (c > top) { second = top; top = c; last = w; }
        else if (c > second) second = c;
      }
      ++times[last];
      margin[last] += (double)(top - second);
    }
  printf("last wave at %s (of %lld workgroup-launches; mean cycles ahead of the next):\n",
         what, (long long)launches * n_wg);
  for (int w = 0; w < WAVES; ++w)
    printf("  wave %d: %lld times, %.1f cycles\n", w, times[w],
           times[w] ? margin[w] / times[w] : 0.0);
}

static void report_stamps(const unsigned long long* st_dev, int first, int launches,
                          int n_wg) {
  const size_t per_launch = (size_t)n_wg * WAVES * 2 * ST_POINTS;
  std::vector<unsigned long long> st((size_t)(first + launches) * per_launch);
  CHECK(hipMemcpy(st.data(), st_dev, st.size() * 8, hipMemcpyDeviceToHost));
  // mean of every point per wave: cycles since the wave's own entry, and wall
  // clock ticks (10 ns) since the launch's earliest entry
  printf("mean cycles since the wave's entry | mean 10-ns ticks since the launch's first entry\n");
  for (int k = 0; k < ST_POINTS; ++k) {
    printf("%-16s", ST_NAMES[k]);
    for (int pass = 0; pass < 2; ++pass) {
      for (int w = 0; w < WAVES; ++w) {
        double sum = 0;
        long long n = 0;
        for (int s = first; s < first + launches; ++s) {
          unsigned long long t0 = ~0ull;
          for (int g = 0; g < n_wg; ++g)
            for (int x = 0; x < WAVES; ++x)
              t0 = std::min(t0, st[s * per_launch + (size_t)(g * WAVES + x) * 2 * ST_POINTS]);
          for (int g = 0; g < n_wg; ++g) {
            const unsigned long long* r = &st[s * per_launch + (size_t)(g * WAVES + w) * 2 * ST_POINTS];
            if (r[ST_POINTS + k] == 0) continue;   // the wave does not pass this point
            sum += pass == 0 ? (double)(r[ST_POINTS + k] - r[ST_POINTS + ST_ENTRY])
                             : (double)(r[k] - t0);
            ++n;
          }
        }
        printf(" %8.1f", n ? sum / n : 0.0);
      }
      printf(pass == 0 ? " |" : "\n");
    }
  }
  report_last_wave(st, first, launches, n_wg, ST_ROWSEG, "the second barrier");
  report_last_wave(st, first, launches, n_wg, ST_DRAIN, "the third barrier");
  // the 16-slab batch: first load to last load issued, and to its arrival
  double issue = 0, arrive = 0;
  long long n = 0;
  for (int s = first; s < first + launches; ++s)
    for (int g = 0; g < n_wg; ++g)
      for (int w = 0; w < WAVES; ++w) {
        const unsigned long long* c =
            &st[s * per_launch + (size_t)(g * WAVES + w) * 2 * ST_POINTS + ST_POINTS];
        if (c[ST_LD_FIRST] == 0) continue;
        issue += (double)(c[ST_LD_ISSUED] - c[ST_LD_FIRST]);
        arrive += (double)(c[ST_LD_ARRIVED] - c[ST_LD_FIRST]);
        ++n;
      }
  printf("16-slab batch, mean cycles over %lld waves: first load to last load issued "
         "%.1f, to arrival %.1f\n", n, n ? issue / n : 0.0, n ? arrive / n : 0.0);
}
#endif

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 2048;
  const int iters = argc > 2 ? atoi(argv[2]) : 2000;
  const int n_wg = (B + ROWS - 1) / ROWS;

  unsigned short *Xbf, *W1bf, *W2bf, *bfmirror;
  int *y, *t_dev;
  unsigned* counter;
  float *master, *m, *v, *slabs, *loss;
  unsigned short* wimg;
  CHECK(hipMalloc(&Xbf, (size_t)B * IN * 2));
  CHECK(hipMalloc(&W1bf, IN * HID * 2));
  CHECK(hipMalloc(&W2bf, HID * CPAD * 2));
  CHECK(hipMalloc(&bfmirror, (NPARAM + 8) * 2));
  CHECK(hipMalloc(&y, (size_t)B * 4));
  CHECK(hipMalloc(&t_dev, 4));
  CHECK(hipMalloc(&counter, 4));
  CHECK(hipMalloc(&master, NPARAM * 4));
  CHECK(hipMalloc(&m, NPARAM * 4));
  CHECK(hipMalloc(&v, NPARAM * 4));
  CHECK(hipMalloc(&slabs, (size_t)n_wg * SLAB * 4));
  CHECK(hipMalloc(&loss, 4));
  CHECK(hipMalloc(&wimg, DIGITS_WIMG_N * 2));
  CHECK(hipMemset(wimg, 0, DIGITS_WIMG_N * 2));
  CHECK(hipMemset(Xbf, 0, (size_t)B * IN * 2));
  CHECK(hipMemset(W1bf, 0, IN * HID * 2));
  CHECK(hipMemset(W2bf, 0, HID * CPAD * 2));
  CHECK(hipMemset(y, 0, (size_t)B * 4));
  CHECK(hipMemset(t_dev, 0, 4));
  CHECK(hipMemset(counter, 0, 4));
  CHECK(hipMemset(master, 0, NPARAM * 4));
  CHECK(hipMemset(m, 0, NPARAM * 4));
  CHECK(hipMemset(v, 0, NPARAM * 4));
  CHECK(hipMemset(slabs, 0, (size_t)n_wg * SLAB * 4));

#ifdef PROBE_STAMPS
  // one record per launch, warm-up included (the kernel indexes by its epoch)
  const size_t st_launches = 100 + (size_t)iters;
  const size_t st_words = st_launches * n_wg * WAVES * 2 * ST_POINTS;
  unsigned long long* st_dev;
  CHECK(hipMalloc(&st_dev, st_words * 8));
  CHECK(hipMemset(st_dev, 0, st_words * 8));
  const unsigned st_cap = (unsigned)st_launches;
  CHECK(hipMemcpyToSymbol(HIP_SYMBOL(probe_stamps), &st_dev, sizeof(st_dev)));
  CHECK(hipMemcpyToSymbol(HIP_SYMBOL(probe_stamps_launches), &st_cap, sizeof(st_cap)));
#endif

  for (int i = 0; i < 100; ++i) {
    if (launch_mlp_step_fused(Xbf, y, B, W1bf, W2bf, master, bfmirror, m, v,
                              t_dev, slabs, counter, loss, 1.0f / B, 1e-3f,
                              0.9f, 0.999f, 1e-8f, n_wg, nullptr, wimg, 0) != 0) {
      fprintf(stderr, "launch failed\n");
      return 1;
    }
  }
  CHECK(hipDeviceSynchronize());
#ifdef PROBE_COUNT_POLLS
  constexpr int POLL_BINS = SLAB - (NPARAM + 2);
  static_assert(POLL_BINS >= 14, "the kernel's bins fit behind slab 0's tag");
  CHECK(hipMemset(slabs + NPARAM + 2, 0, POLL_BINS * 4));   // drop the warm-up's
#endif

  hipEvent_t t0, t1;
  CHECK(hipEventCreate(&t0));
  CHECK(hipEventCreate(&t1));
  CHECK(hipEventRecord(t0, 0));
  for (int i = 0; i < iters; ++i) {
    launch_mlp_step_fused(Xbf, y, B, W1bf, W2bf, master, bfmirror, m, v, t_dev,
                          slabs, counter, loss, 1.0f / B, 1e-3f, 0.9f, 0.999f,
                          1e-8f, n_wg, nullptr, wimg, 0);
  }
  CHECK(hipEventRecord(t1, 0));
  CHECK(hipEventSynchronize(t1));
  float ms = 0.f;
  CHECK(hipEventElapsedTime(&ms, t0, t1));
  printf("B=%d n_wg=%d us_per_launch=%.3f\n", B, n_wg, ms * 1000.0f / iters);
#ifdef PROBE_COUNT_POLLS
  unsigned bins[POLL_BINS];
  CHECK(hipMemcpy(bins, slabs + NPARAM + 2, sizeof(bins), hipMemcpyDeviceToHost));
  printf("poll rounds per launch (1 .. 13, 14+):");
  for (int k = 0; k < 14; ++k) printf(" %u", bins[k]);
  printf("\n");
#endif
#ifdef PROBE_STAMPS
  report_stamps(st_dev, 100, iters, n_wg);
#endif
  return 0;
}
