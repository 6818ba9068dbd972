// Prints the four-product moment constants the library uploads as sys.qf_tab (csrc/aomarl_qf4_host.h), for
// tests/test_qf_four_products.py and for a host sanitizer build:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ao_marl_amd/csrc tools/qf4_table.cpp -o qf4_table && ./qf4_table
// Output: "err <|H'H'^T - M|/|M|> <|H'LH'^T - S|/|S|>", "t <8 values>", 16 lines "H <16 values>" (double, row x),
// then 64 lines "lane <8 floats>".
#include <cstdio>
#include "aomarl_qf4_host.h"

int main() {
  float tab[64 * 8];
  aomarl_qf4::Basis b;
  const bool ok = aomarl_qf4::build_table(tab, &b);
  std::printf("err %.17g %.17g\n", b.err_m, b.err_s);
  std::printf("t");
  for (int k = 0; k < 8; k++) std::printf(" %.17g", b.t[k]);
  std::printf("\n");
  for (int x = 0; x < 16; x++) {
    std::printf("H");
    for (int a = 0; a < 16; a++) std::printf(" %.17g", b.H[x][a]);
    std::printf("\n");
  }
  if (!ok) { std::fprintf(stderr, "qf4: factorisation check failed\n"); return 1; }
  for (int lane = 0; lane < 64; lane++) {
    std::printf("lane");
    for (int k = 0; k < 8; k++) std::printf(" %.9g", tab[8 * lane + k]);
    std::printf("\n");
  }
  return 0;
}
