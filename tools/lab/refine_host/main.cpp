// main.cpp -- reads one rp_refine_pose call from a file, runs it through ../eightpoint_host/shim.h, writes pose | E | stat | w_out (see run.py)
#include "kernel.cpp"  // made by run.py: refine_pose.hip with its includes redirected to shim.h
// file: int n, P, iters, has_w; then pose0[n*7], x1[n*P*2], x2, w[n*P], tau[n]  -> out file: pose[n*7], E[n*9], stat[n*4], w_out[n*P]
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[4]; fread(h, 4, 4, f);
  int n = h[0], P = h[1], iters = h[2], has_w = h[3];
  std::vector<float> p0(n * 7), x1((size_t)n * P * 2), x2(x1.size()), w((size_t)n * P), tau(n);
  std::vector<float> pose(n * 7, -7.f), E(n * 9, -7.f), st(n * 4, -7.f), wo((size_t)n * P, -7.f);
  fread(p0.data(), 4, p0.size(), f); fread(x1.data(), 4, x1.size(), f); fread(x2.data(), 4, x2.size(), f); fread(w.data(), 4, w.size(), f);
  fread(tau.data(), 4, n, f); fclose(f);
  int rc = rp_refine_pose(p0.data(), x1.data(), x2.data(), has_w ? w.data() : nullptr, tau.data(), pose.data(), E.data(), st.data(), wo.data(),
                          P, iters, n, nullptr);
  if (rc) { printf("rc %d\n", rc); return 1; }
  f = fopen(argv[2], "wb");
  fwrite(pose.data(), 4, pose.size(), f); fwrite(E.data(), 4, E.size(), f); fwrite(st.data(), 4, st.size(), f); fwrite(wo.data(), 4, wo.size(), f);
  fclose(f);
  return 0;
}
