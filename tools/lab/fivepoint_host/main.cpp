// main.cpp -- reads one rp_five_point_consensus call from a file, runs it through ../eightpoint_host/shim.h, writes the outputs (see run.py)
#include "kernel.cpp"  // made by run.py: five_point.hip with its includes redirected to shim.h
// file: int n, P, M, seed, has_w; then x1[n*P*2], x2, w[n*P], tau[n]
// -> out file: E[n*9], stat[n*4], w_out[n*P], hyp_E[n*M*90], hyp_cost[n*M*10] (float), then best[n*2], samples[n*M*5] (int)
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[5]; fread(h, 4, 5, f);
  int n = h[0], P = h[1], M = h[2], seed = h[3], has_w = h[4];
  std::vector<float> x1((size_t)n * P * 2), x2(x1.size()), w((size_t)n * P), tau(n);
  // exact sizes on the heap: AddressSanitizer sees a write one element past any of them
  std::vector<float> E(n * 9, NAN), st(n * 4, NAN), wo((size_t)n * P, NAN), hE((size_t)n * M * 90, NAN), hc((size_t)n * M * 10, NAN);
  std::vector<int> best(n * 2, -7), smp((size_t)n * M * 5, -7);
  fread(x1.data(), 4, x1.size(), f); fread(x2.data(), 4, x2.size(), f); fread(w.data(), 4, w.size(), f); fread(tau.data(), 4, n, f); fclose(f);
  int rc = rp_five_point_consensus(x1.data(), x2.data(), has_w ? w.data() : nullptr, tau.data(), seed, E.data(), best.data(), st.data(),
                                   wo.data(), hE.data(), hc.data(), smp.data(), P, M, n, nullptr);
  if (rc) { printf("rc %d\n", rc); return 1; }
  f = fopen(argv[2], "wb");
  fwrite(E.data(), 4, E.size(), f); fwrite(st.data(), 4, st.size(), f); fwrite(wo.data(), 4, wo.size(), f); fwrite(hE.data(), 4, hE.size(), f);
  fwrite(hc.data(), 4, hc.size(), f); fwrite(best.data(), 4, best.size(), f); fwrite(smp.data(), 4, smp.size(), f);
  fclose(f);
  return 0;
}
