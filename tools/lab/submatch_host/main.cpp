// main.cpp -- reads one rp_emm_submatch call from a file, runs it through shim_extra.h, writes win and quad (see run.py)
#include "kernel.cpp"  // made by run.py: submatch.hip with its includes redirected to shim_extra.h
// file: int Z, H, ld, swap, single, radius, has_clse; float scale; then q[Z*576*ld], k[Z*576*ld], rlse[Z*H*576], clse[Z*H*576], idx[Z*H*576]
// -> out file: win[Z*H*576*4], quad[Z*H*576*4]
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); int h[7]; float scale;
  if (fread(h, 4, 7, f) != 7 || fread(&scale, 4, 1, f) != 1) return 2;
  const int Z = h[0], H = h[1], ld = h[2], swap = h[3], single = h[4], radius = h[5], has_clse = h[6];
  // exact sizes on the heap: AddressSanitizer sees a read or write one element outside any of them.  q and k end with the last row's
  // H*64 columns, not with a whole ld
  const size_t nqk = ((size_t)Z * 576 - 1) * ld + (size_t)H * 64, no = (size_t)Z * H * 576;
  std::vector<float> q(nqk), k(nqk), rl(no), cl(no), win(no * 4, NAN), quad(no * 4, NAN);
  std::vector<int> idx(no);
  std::vector<float> row(ld);
  for (std::vector<float>* t : {&q, &k})
    for (size_t r = 0; r < (size_t)Z * 576; ++r) {
      if (fread(row.data(), 4, ld, f) != (size_t)ld) return 2;
      memcpy(t->data() + r * ld, row.data(), 4 * (r + 1 == (size_t)Z * 576 ? (size_t)H * 64 : (size_t)ld));
    }
  if (fread(rl.data(), 4, no, f) != no || fread(cl.data(), 4, no, f) != no || fread(idx.data(), 4, no, f) != no) return 2;
  fclose(f);
  int rc = rp_emm_submatch(q.data(), k.data(), rl.data(), has_clse ? cl.data() : nullptr, idx.data(), win.data(), quad.data(), Z, H, ld, ld,
                           scale, swap, single, radius, nullptr);
  if (rc) { printf("rc %d\n", rc); return 1; }
  f = fopen(argv[2], "wb");
  fwrite(win.data(), 4, win.size(), f); fwrite(quad.data(), 4, quad.size(), f);
  fclose(f);
  return 0;
}
