// main.cpp -- reads one problem batch from a file and runs the three entry points of relpose_homography.h through
// ../eightpoint_host/shim.h: consensus -> refine (from the consensus winner) -> decomposition (of the refined H); writes the outputs (see run.py)
#include "kernel.cpp"  // made by run.py: homography.hip with its includes redirected to shim.h
// file: int n, P, M, seed, has_w, iters; then x1[n*P*2], x2, w[n*P], tau[n]
// -> out file (float): H[n*9], stat[n*4], w_out[n*P], hyp_H[n*M*9], hyp_cost[n*M] | rH[n*9], rstat[n*4], rw[n*P] | pose[n*28], normal[n*12],
//    cstat[n*16]; then (int) best[n], samples[n*M*4], pick[n*2]
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[6]; fread(h, 4, 6, f);
  int n = h[0], P = h[1], M = h[2], seed = h[3], has_w = h[4], iters = h[5];
  std::vector<float> x1((size_t)n * P * 2), x2(x1.size()), w((size_t)n * P), tau(n);
  // exact sizes on the heap: AddressSanitizer sees a write one element past any of them
  std::vector<float> H(n * 9, NAN), st(n * 4, NAN), wo((size_t)n * P, NAN), hH((size_t)n * M * 9, NAN), hc((size_t)n * M, NAN);
  std::vector<float> rH(n * 9, NAN), rst(n * 4, NAN), rw((size_t)n * P, NAN), pose(n * 28, NAN), nrm(n * 12, NAN), cs(n * 16, NAN);
  std::vector<int> best(n, -7), smp((size_t)n * M * 4, -7), pick(n * 2, -7);
  fread(x1.data(), 4, x1.size(), f); fread(x2.data(), 4, x2.size(), f); fread(w.data(), 4, w.size(), f); fread(tau.data(), 4, n, f); fclose(f);
  const float* W = has_w ? w.data() : nullptr;
  int rc = rp_homography_consensus(x1.data(), x2.data(), W, tau.data(), seed, H.data(), best.data(), st.data(), wo.data(), hH.data(), hc.data(),
                                   smp.data(), P, M, n, nullptr);
  if (!rc) rc = rp_homography_refine(x1.data(), x2.data(), W, tau.data(), H.data(), iters, rH.data(), rst.data(), rw.data(), P, n, nullptr);
  if (!rc) rc = rp_pose_from_homography(rH.data(), x1.data(), x2.data(), W, tau.data(), 0.99f, pose.data(), nrm.data(), cs.data(), pick.data(), P, n,
                                        nullptr);
  if (rc) { printf("rc %d\n", rc); return 1; }
  f = fopen(argv[2], "wb");
  for (auto* v : {&H, &st, &wo, &hH, &hc, &rH, &rst, &rw, &pose, &nrm, &cs}) fwrite(v->data(), 4, v->size(), f);
  for (auto* v : {&best, &smp, &pick}) fwrite(v->data(), 4, v->size(), f);
  fclose(f);
  return 0;
}
