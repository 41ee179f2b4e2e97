// main.cpp -- reads one problem batch from a file and runs rp_triangulate of relpose_triangulate.h through ../eightpoint_host/shim.h;
// writes the outputs (see run.py)
#include "kernel.cpp"  // made by run.py: triangulate.hip with its includes redirected to shim.h
// file: int n, P, has_w, has_xc; then pose[n*7], x1[n*P*2], x2, w[n*P], tau[n]
// -> out file (float): X[n*P*3], aux[n*P*4], stat[n*4], xc[n*P*4] (has_xc only)
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[4]; fread(h, 4, 4, f);
  int n = h[0], P = h[1], has_w = h[2], has_xc = h[3];
  std::vector<float> pose(n * 7), x1((size_t)n * P * 2), x2(x1.size()), w((size_t)n * P), tau(n);
  // exact sizes on the heap: AddressSanitizer sees a write one element past any of them
  std::vector<float> X((size_t)n * P * 3, NAN), aux((size_t)n * P * 4, NAN), st(n * 4, NAN), xc(has_xc ? (size_t)n * P * 4 : 0, NAN);
  fread(pose.data(), 4, pose.size(), f); fread(x1.data(), 4, x1.size(), f); fread(x2.data(), 4, x2.size(), f); fread(w.data(), 4, w.size(), f);
  fread(tau.data(), 4, n, f); fclose(f);
  int rc = rp_triangulate(pose.data(), x1.data(), x2.data(), has_w ? w.data() : nullptr, tau.data(), X.data(), aux.data(),
                          has_xc ? xc.data() : nullptr, st.data(), P, n, nullptr);
  if (rc) { printf("rc %d\n", rc); return 1; }
  f = fopen(argv[2], "wb");
  for (auto* v : {&X, &aux, &st, &xc}) if (!v->empty()) fwrite(v->data(), 4, v->size(), f);
  fclose(f);
  return 0;
}
