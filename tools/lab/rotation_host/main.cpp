// main.cpp -- reads one problem batch from a file and runs the two entry points of relpose_rotation.h through
// ../eightpoint_host/shim.h: consensus -> refine (from the consensus winner); writes the outputs (see run.py)
#include "kernel.cpp"  // made by run.py: rotation.hip with its includes redirected to shim.h
// file: int n, P, M, seed, has_w, iters; then x1[n*P*2], x2, w[n*P], tau[n]
// -> out file (float): R[n*9], stat[n*4], w_out[n*P], hyp_R[n*M*9], hyp_cost[n*M] | rR[n*9], pose[n*7], rstat[n*4], rw[n*P];
//    then (int) best[n], samples[n*M*2]
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[6]; fread(h, 4, 6, f);
  int n = h[0], P = h[1], M = h[2], seed = h[3], has_w = h[4], iters = h[5];
  std::vector<float> x1((size_t)n * P * 2), x2(x1.size()), w((size_t)n * P), tau(n);
  // exact sizes on the heap: AddressSanitizer sees a write one element past any of them
  std::vector<float> R(n * 9, NAN), st(n * 4, NAN), wo((size_t)n * P, NAN), hR((size_t)n * M * 9, NAN), hc((size_t)n * M, NAN);
  std::vector<float> rR(n * 9, NAN), pose(n * 7, NAN), rst(n * 4, NAN), rw((size_t)n * P, NAN);
  std::vector<int> best(n, -7), smp((size_t)n * M * 2, -7);
  fread(x1.data(), 4, x1.size(), f); fread(x2.data(), 4, x2.size(), f); fread(w.data(), 4, w.size(), f); fread(tau.data(), 4, n, f); fclose(f);
  const float* W = has_w ? w.data() : nullptr;
  int rc = rp_rotation_consensus(x1.data(), x2.data(), W, tau.data(), seed, R.data(), best.data(), st.data(), wo.data(), hR.data(), hc.data(),
                                 smp.data(), P, M, n, nullptr);
  if (!rc) rc = rp_rotation_refine(x1.data(), x2.data(), W, tau.data(), R.data(), iters, rR.data(), pose.data(), rst.data(), rw.data(), P, n, nullptr);
  if (rc) { printf("rc %d\n", rc); return 1; }
  f = fopen(argv[2], "wb");
  for (auto* v : {&R, &st, &wo, &hR, &hc, &rR, &pose, &rst, &rw}) fwrite(v->data(), 4, v->size(), f);
  for (auto* v : {&best, &smp}) fwrite(v->data(), 4, v->size(), f);
  fclose(f);
  return 0;
}
