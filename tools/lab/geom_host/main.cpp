// main.cpp -- reads one call of csrc/geom.hip or csrc/se3loss.hip from a file, runs it through shim.h, writes its outputs (see run.py)
#include "kernel.cpp"  // made by run.py: geom.hip and se3loss.hip with their includes redirected to shim.h
// file: int op, n, P; then the inputs as float32.  Outputs are exactly as large as the header documents, so a write past them is caught.
//   op 0  rp_svd3x3               A[n*9]                        -> U[n*9], S[n*3], V[n*9]
//   op 1  rp_pose_from_essential  E[n*9], x1[n*P*2], x2[n*P*2]  -> pose[n*7], count[n] (as float)
//   op 2  rp_geodesic_loss        Ps[n*14], Gs[n*14]            -> losses[2], dmean[2*n*14]
//   op 3  rp_essential_from_pose  pose[n*7]                     -> E[n*9]
static std::vector<float> rd(FILE* f, size_t k) { std::vector<float> v(k); if (fread(v.data(), 4, k, f) != k) { printf("short input\n"); exit(2); } return v; }
static void wr(FILE* f, const std::vector<float>& v) { fwrite(v.data(), 4, v.size(), f); }
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[3]; if (fread(h, 4, 3, f) != 3) return 2;
  const int op = h[0], n = h[1], P = h[2];
  FILE* o = fopen(argv[2], "wb");
  int rc = 0;
  if (op == 0) {
    auto A = rd(f, (size_t)n * 9);
    std::vector<float> U(n * 9, -7.f), S(n * 3, -7.f), V(n * 9, -7.f);
    rc = rp_svd3x3(A.data(), U.data(), S.data(), V.data(), n, nullptr);
    wr(o, U); wr(o, S); wr(o, V);
  } else if (op == 1) {
    auto E = rd(f, (size_t)n * 9), x1 = rd(f, (size_t)n * P * 2), x2 = rd(f, (size_t)n * P * 2);
    std::vector<float> pose(n * 7, -7.f), cf(n);
    std::vector<int> count(n, -7);
    rc = rp_pose_from_essential(E.data(), x1.data(), x2.data(), P, pose.data(), count.data(), n, nullptr);
    for (int i = 0; i < n; ++i) cf[i] = (float)count[i];
    wr(o, pose); wr(o, cf);
  } else if (op == 2) {
    auto Ps = rd(f, (size_t)n * 14), Gs = rd(f, (size_t)n * 14);
    std::vector<float> losses(2, -7.f), dmean((size_t)2 * n * 14, -7.f), scratch((size_t)60 * n, -7.f);
    rc = rp_geodesic_loss(Ps.data(), Gs.data(), losses.data(), dmean.data(), scratch.data(), n, nullptr);
    wr(o, losses); wr(o, dmean);
  } else if (op == 3) {
    auto pose = rd(f, (size_t)n * 7);
    std::vector<float> E(n * 9, -7.f);
    rc = rp_essential_from_pose(pose.data(), E.data(), n, nullptr);
    wr(o, E);
  } else rc = -1;
  fclose(f); fclose(o);
  if (rc) { printf("rc %d\n", rc); return 1; }
  return 0;
}
