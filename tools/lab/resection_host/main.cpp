// main.cpp -- reads one problem batch from a file and runs the two entry points of relpose_resection.h through
// ../eightpoint_host/shim.h: consensus -> refine (from the consensus winner, `iters` iterations) -> refine again in place (aliased);
// writes the outputs (see run.py)
#include "kernel.cpp"  // made by run.py: resection.hip with its includes redirected to shim.h
// file: int n, P, M, seed, has_w, iters; then X[n*P*3], x[n*P*2], w[n*P], tau[n]
// -> out file (float): pose[n*7], stat[n*4], w_out[n*P], hyp_pose[n*M*7], hyp_cost[n*M] | rpose[n*7], rstat[n*4], rw[n*P], apose[n*7];
//    then (int) best[n], hyp_count[n*M], samples[n*M*3]
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[6]; fread(h, 4, 6, f);
  int n = h[0], P = h[1], M = h[2], seed = h[3], has_w = h[4], iters = h[5];
  std::vector<float> X((size_t)n * P * 3), x((size_t)n * P * 2), w((size_t)n * P), tau(n);
  // exact sizes on the heap: AddressSanitizer sees a write one element past any of them
  std::vector<float> pose(n * 7, NAN), st(n * 4, NAN), wo((size_t)n * P, NAN), hp((size_t)n * M * 7, NAN), hc((size_t)n * M, NAN);
  std::vector<float> rpose(n * 7, NAN), rst(n * 4, NAN), rw((size_t)n * P, NAN), apose(n * 7, NAN), ast(n * 4, NAN);
  std::vector<int> best(n, -7), cnt((size_t)n * M, -7), smp((size_t)n * M * 3, -7);
  fread(X.data(), 4, X.size(), f); fread(x.data(), 4, x.size(), f); fread(w.data(), 4, w.size(), f); fread(tau.data(), 4, n, f); fclose(f);
  const float* W = has_w ? w.data() : nullptr;
  int rc = rp_p3p_consensus(X.data(), x.data(), W, tau.data(), seed, pose.data(), best.data(), st.data(), wo.data(), hp.data(), hc.data(),
                            cnt.data(), smp.data(), P, M, n, nullptr);
  if (!rc) rc = rp_pnp_refine(X.data(), x.data(), W, tau.data(), pose.data(), iters, rpose.data(), rst.data(), rw.data(), P, n, nullptr);
  apose = pose;
  if (!rc) rc = rp_pnp_refine(X.data(), x.data(), W, tau.data(), apose.data(), iters, apose.data(), ast.data(), nullptr, P, n, nullptr);
  if (rc) { printf("rc %d\n", rc); return 1; }
  f = fopen(argv[2], "wb");
  for (auto* v : {&pose, &st, &wo, &hp, &hc, &rpose, &rst, &rw, &apose}) fwrite(v->data(), 4, v->size(), f);
  for (auto* v : {&best, &cnt, &smp}) fwrite(v->data(), 4, v->size(), f);
  fclose(f);
  return 0;
}
