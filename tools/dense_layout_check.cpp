// Host-only check of the dense solve's workspace layout (gslam_amd/csrc/dense_solve.h), no GPU: every segment in order, disjoint,
// on a 128-byte line and of the size its contract names, the single-launch state there exactly when the shape fits the CUs, and
// the launch-per-step path's X rows inside `xwork` at every step of its panel loop.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -Iinclude -Igslam_amd/csrc -I/opt/rocm/include \
//       tools/dense_layout_check.cpp -o build/dense_layout_check && build/dense_layout_check
// (tests/test_dense_layout_cpu.py builds and runs it.)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dense_solve.h"

static int failures = 0;
#define CHECK(cond)                                                                                               \
  do {                                                                                                            \
    if (!(cond)) {                                                                                                \
      printf("n %d extra %d cus %d: %s (line %d)\n", n, extra, cus, #cond, __LINE__);                             \
      ++failures;                                                                                                 \
    }                                                                                                             \
  } while (0)

static size_t div_up(size_t a, size_t b) { return (a + b - 1) / b; }

// chol.hip, the comment at the single launch: one chain workgroup, one accumulator workgroup per tile row below the first, and
// ceil((i - 1) / 6) workers for tile row i >= 2 -- all resident at once, one per CU (256 when the CU count is unknown)
static bool flow_fits(int n, int extra, int cus) {
  const int ntr = (int)div_up((size_t)n + extra, 64);
  int groups = 0;
  for (int i = 2; i < ntr; ++i) groups += (i - 1 + 5) / 6;
  return 1 + (ntr - 1 > 0 ? ntr - 1 : 0) + groups <= (cus > 0 ? cus : 256);
}

// the panel loop of potrf_stepwise (chol.hip), reduced to what decides where a step parks its X rows
static void walk_xwork(int n, int extra, int cus, const DenseLayout& L, const DenseWork& w, bool pair_switch) {
  const int nr = n + extra;
  const int nbo = n >= 32768 ? 1024 : (n >= 16384 ? 512 : 256);
  const bool pair_blocks = pair_switch && n >= 16384;
  auto lower_tiles = [](int ti, int tj) { return tj * (tj + 1) / 2 + (ti - tj) * tj; };
  auto fused = [&](int cb, int ce) { return lower_tiles((int)div_up(nr - cb, 64), (int)div_up(ce - cb, 64)) <= 256; };
  int xsel = 0;
  for (int c0 = 0; c0 < n; c0 += nbo) {
    const int pw = n - c0 < nbo ? n - c0 : nbo;
    int deferred_k = -1;
    for (int k = c0; k < c0 + pw; k += 64) {
      const int kb = c0 + pw - k < 64 ? c0 + pw - k : 64;
      const int cb = k + kb, ce = c0 + pw;
      if (cb >= nr) continue;
      if (deferred_k >= 0) {
        deferred_k = -1;
        continue;
      }
      if (kb == 64 && cb < ce && fused(cb, ce)) {
        const size_t last = (size_t)xsel * 64 * nr + (size_t)63 * nr + (size_t)(nr - cb - 1);  // column 63, row nr - 1
        CHECK(last < L.xwork_doubles);
        CHECK((const char*)(w.xwork + last + 1) <= (const char*)w.xh);
        xsel ^= 1;
      } else if (pair_blocks && kb == 64 && cb + 64 < ce && !fused(cb + 64, ce)) {
        deferred_k = k;
      }
    }
  }
}

int main() {
  const int ns[] = {1, 63, 64, 65, 127, 128, 129, 777, 4095, 4096, 4097, 8192, 8193, 16384, 60000};
  const int cu_counts[] = {0, 1, 8, 256, 304};
  int cases = 0;
  for (int n : ns)
    for (int extra = 0; extra <= 1; ++extra)
      for (int cus : cu_counts) {
        const DenseLayout L = dense_layout(n, extra, cus);
        const size_t nb = div_up(n, 64);
        // the sizes of the contract
        CHECK(L.dinv_doubles == nb * 4096);
        CHECK(L.work_doubles == (size_t)n);
        CHECK(L.xwork_doubles == (size_t)2 * 64 * (n + extra));
        CHECK(L.xh_doubles == nb * 64);
        CHECK(L.n_xh_words == 2 * nb * 64);
        // in order, disjoint, inside the total, every start on a 128-byte line, info on a line of its own
        const size_t start[] = {L.info, L.dinv, L.work, L.xwork, L.xh, L.flow_state};
        const size_t bytes[] = {sizeof(int), L.dinv_doubles * 8, L.work_doubles * 8, L.xwork_doubles * 8, L.xh_doubles * 8, L.flow_words * 4};
        CHECK(L.info == 0 && L.dinv >= 128);
        for (int s = 0; s < 6; ++s) {
          CHECK(start[s] % 128 == 0);
          CHECK(start[s] + bytes[s] <= (s + 1 < 6 ? start[s + 1] : L.bytes));
        }
        // the single-launch state: there exactly when the shape fits the CUs
        const bool fits = flow_fits(n, extra, cus);
        CHECK((L.flow_words != 0) == fits);
        CHECK((L.flow_workers >= 0) == fits);
        CHECK(L.n_flow_flag_words % 32 == 0);
        CHECK((L.n_flow_flag_words != 0) == fits);
        if (fits) {
          const size_t ntr = div_up((size_t)n + extra, 64);
          CHECK(L.n_flow_flag_words >= ntr * nb + nb + ntr + 1);  // tile, block and hand-over flags, the abort word
          CHECK(L.flow_words == L.n_flow_flag_words + ntr * 8192 * 2);
          CHECK((L.flow_state + (size_t)L.n_flow_flag_words * 4) % 128 == 0);  // the hand-over tiles start on a line too
        }
        // the carve, on real memory: the sanitizers see every first and last element
        std::vector<char> block(L.bytes + 128);
        char* base = block.data() + (128 - (size_t)block.data() % 128) % 128;
        const DenseWork w = dense_carve(base, L);
        CHECK((char*)w.info == base + L.info && (char*)w.dinv == base + L.dinv && (char*)w.work == base + L.work);
        CHECK((char*)w.xwork == base + L.xwork && (char*)w.xh == base + L.xh);
        CHECK((w.flow_state == nullptr) == (L.flow_words == 0));
        CHECK(w.n_flow_flag_words == L.n_flow_flag_words && w.n_xh_words == L.n_xh_words);
        *w.info = 0;
        w.dinv[0] = w.dinv[L.dinv_doubles - 1] = 0.0;
        w.work[0] = w.work[L.work_doubles - 1] = 0.0;
        w.xwork[0] = w.xwork[L.xwork_doubles - 1] = 0.0;
        w.xh[0] = w.xh[L.xh_doubles - 1] = 0.0;
        if (w.flow_state) w.flow_state[0] = w.flow_state[L.flow_words - 1] = 0u;
        const DenseReady r = dense_ready(w);
        CHECK(r.info == w.info && r.n_xh == L.n_xh_words && r.n_flow == L.n_flow_flag_words);
        CHECK(r.words() == (r.n_flow > r.n_xh ? r.n_flow : r.n_xh));
        walk_xwork(n, extra, cus, L, w, true);
        walk_xwork(n, extra, cus, L, w, false);
        ++cases;
      }
  printf("%d layouts checked, %d failures\n", cases, failures);
  return failures ? 1 : 0;
}
